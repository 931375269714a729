// test_passes_unlit.cpp — vqhip::UnlitDrawsPass (include/vqhip_passes.hpp; docs/DESIGN_DETAILS.md §7.23) against the stand-in of the engine's RenderPass.h,
// host-only: the adaptor turns the light gizmos of RenderSceneColor and the light volumes of RenderLightBounds into vqhip_unlit_draws calls — the LightMeshes front
// opaque into scene colour, the LightBounds front opaque into the bounding-volumes target when reflections are on and blended into scene colour when they are
// off —, counts the triangles for the work size, owns the work buffer, keeps the library's status and refuses bad parameter blocks without calling.
// The entry point, its size function and the two allocator calls are defined HERE (the executable's definitions are the ones the adaptor binds to): nothing
// touches a device. Built by tests/test_unlit_draws_cpu.py with the command line tests/test_displace_cpu.py uses.
#ifndef VQHIP_ENGINE_RENDERPASS_H
#define VQHIP_ENGINE_RENDERPASS_H "mock_engine/RenderPass.h"
#endif
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include "vqhip_passes.hpp"

static vqhip_unlit_targets gTargets;
static std::vector<vqhip_unlit_draw> gDraws;
static int gWidth = 0, gHeight = 0, gBlend = -1, gCalls = 0, gAllocs = 0, gFrees = 0, gStatus = VQHIP_OK;
static vqhip_ctx* gCtx = nullptr; static void* gStream = nullptr; static void* gWork = nullptr; static size_t gWorkBytes = 0, gAllocBytes = 0;
static uint64_t gSizeTriangles = 0;
static bool gDrawsNull = false;

extern "C" size_t vqhip_unlit_draws_work_bytes(uint64_t triangles) { gSizeTriangles = triangles; return triangles >= 1000000 ? 0 : 256 + (size_t)triangles * 448; }
extern "C" int vqhip_unlit_draws(vqhip_ctx* ctx, void* stream, const vqhip_unlit_draw* draws, int numDraws, int width, int height, int blend,
                                 const vqhip_unlit_targets* out, void* work, size_t workBytes) {
    ++gCalls; gCtx = ctx; gStream = stream; gDrawsNull = draws == nullptr; gDraws.assign(draws, draws + numDraws); gWidth = width; gHeight = height; gBlend = blend;
    gTargets = *out; gWork = work; gWorkBytes = workBytes;
    return gStatus;
}
extern "C" hipError_t hipMalloc(void** p, size_t bytes) { ++gAllocs; gAllocBytes = bytes; *p = std::malloc(bytes); return *p ? hipSuccess : hipErrorOutOfMemory; }
extern "C" hipError_t hipFree(void* p) { ++gFrees; std::free(p); return hipSuccess; }

#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static int adaptor(vqhip_ctx* ctx) {
    using Pass = vqhip::UnlitDrawsPass;
    std::shared_ptr<::IRenderPass> pPass = std::make_shared<Pass>(ctx);
    Pass* pass = static_cast<Pass*>(pPass.get());
    EXPECT(pPass->Initialize());
    EXPECT(!std::make_shared<Pass>(nullptr)->Initialize());
    pPass->RecordCommands(nullptr);
    EXPECT(pass->LastStatus() == VQHIP_ERR_INVALID_ARG && gCalls == 0);
    Pass::FDrawParameters none;
    EXPECT(none.Target == nullptr && none.SceneDepth == nullptr && none.Writer == nullptr && !none.Blend && none.TargetPitch == 0 && none.DepthPitch == 0);
    pPass->RecordCommands(&none);                                                                               // no target: no call
    EXPECT(pass->LastStatus() == VQHIP_ERR_INVALID_ARG && gCalls == 0 && gAllocs == 0);

    static uint16_t color[4], volumes[4]; static float depth[1]; static uint32_t wr[1]; static VQ_UnlitData cbs[2];     // addresses only
    std::vector<vqhip_unlit_draw> draws(3);
    std::memset(draws.data(), 0, draws.size() * sizeof(draws[0]));
    draws[0].mesh.numIndices = 36; draws[0].cb = cbs; draws[1].mesh.numIndices = 0; draws[1].cb = cbs; draws[2].mesh.numIndices = 300; draws[2].cb = cbs + 1;
    for (vqhip_unlit_draw& d : draws) d.cullMode = VQHIP_CULL_BACK;
    const Pass::FTarget sceneColor = { color, 2048 }, boundingVolumes = { volumes, 0 };
    pPass->OnCreateWindowSizeDependentResources(1920, 1080, nullptr);

    // the gizmos: opaque, into scene colour
    Pass::FDrawParameters p = Pass::LightMeshes(&none, &draws, sceneColor, depth, 1984);
    EXPECT(!p.Blend && p.Target == color && p.TargetPitch == 2048 && p.SceneDepth == depth && p.DepthPitch == 1984 && p.Writer == nullptr);
    Pass::FDrawParameters noDepth = p;
    noDepth.SceneDepth = nullptr;
    pPass->RecordCommands(&noDepth);                                                                            // no depth: no call
    EXPECT(pass->LastStatus() == VQHIP_ERR_INVALID_ARG && gCalls == 0);
    p.Writer = wr;
    gStatus = 4321;                                                                                             // the library's status is kept
    pPass->RecordCommands(&p);
    EXPECT(gCalls == 1 && pass->LastStatus() == 4321);
    gStatus = VQHIP_OK;
    pPass->RecordCommands(&p);
    EXPECT(gCalls == 2 && pass->LastStatus() == VQHIP_OK);
    EXPECT(gCtx == ctx && gStream == &none && gWidth == 1920 && gHeight == 1080 && gBlend == 0 && gDraws.size() == 3 &&
           std::memcmp(gDraws.data(), draws.data(), 3 * sizeof(draws[0])) == 0);
    EXPECT(gTargets.sceneColor == color && gTargets.pitch == 2048 && gTargets.sceneDepth == depth && gTargets.depth_pitch == 1984 && gTargets.writer == wr &&
           gTargets.writer_pitch == 0 && gTargets.reserved == 0);
    EXPECT(gSizeTriangles == 12 + 100 && gAllocs == 1 && gAllocBytes == 256 + 112 * 448 && gWork == pass->GetWorkBuffer() && gWorkBytes == gAllocBytes && gFrees == 0);

    // the light volumes with reflections: opaque, into the bounding-volumes target
    p = Pass::LightBounds(&none, &draws, true, sceneColor, boundingVolumes, depth);
    EXPECT(!p.Blend && p.Target == volumes && p.TargetPitch == 0 && p.DepthPitch == 0);
    pPass->RecordCommands(&p);
    EXPECT(gCalls == 3 && gBlend == 0 && gTargets.sceneColor == volumes && gTargets.pitch == 0 && gTargets.sceneDepth == depth && gTargets.writer == nullptr && gAllocs == 1);
    // ... and without: blended, straight into scene colour
    p = Pass::LightBounds(&none, &draws, false, sceneColor, boundingVolumes, depth, 1984);
    EXPECT(p.Blend && p.Target == color && p.TargetPitch == 2048);
    pPass->RecordCommands(&p);
    EXPECT(gCalls == 4 && gBlend == 1 && gTargets.sceneColor == color && gTargets.pitch == 2048 && gTargets.depth_pitch == 1984 && gAllocs == 1);

    draws.resize(1);                                                                                            // fewer triangles: the buffer is kept
    pPass->RecordCommands(&p);
    EXPECT(gCalls == 5 && gAllocs == 1 && gSizeTriangles == 12 && gWorkBytes == 256 + 112 * 448);
    draws.resize(2); draws[1] = draws[0]; draws[1].mesh.numIndices = 3000;                                      // more: it grows (the old one is freed first)
    pPass->RecordCommands(&p);
    EXPECT(gCalls == 6 && gAllocs == 2 && gFrees == 1 && gWorkBytes == 256 + 1012 * 448);
    p.Draws = nullptr;                                                                                          // no lights: the call is made, with no draws
    pPass->RecordCommands(&p);
    EXPECT(gCalls == 7 && gDrawsNull && gDraws.empty() && gSizeTriangles == 0 && pass->LastStatus() == VQHIP_OK && gAllocs == 2);
    std::vector<vqhip_unlit_draw> empty;
    p.Draws = &empty;
    pPass->RecordCommands(&p);
    EXPECT(gCalls == 8 && gDrawsNull && gDraws.empty());
    draws[1].mesh.numIndices = 3000000;                                                                         // beyond the library's limit: the size function says 0, no call
    p.Draws = &draws;
    pPass->RecordCommands(&p);
    EXPECT(gCalls == 8 && pass->LastStatus() == VQHIP_ERR_HIP);
    pPass->Destroy();
    EXPECT(gFrees == 2 && pass->GetWorkBuffer() == nullptr && pass->GetWorkBytes() == 0);
    return 0;
}

int main() {
    static_assert(std::is_base_of<::IRenderPass, vqhip::UnlitDrawsPass>::value, "the adaptor derives from the engine's IRenderPass");
    vqhip_ctx* ctx = reinterpret_cast<vqhip_ctx*>(static_cast<uintptr_t>(0x1000));      // never dereferenced: the library call is the recorder above
    if (int rc = adaptor(ctx)) return rc;
    EXPECT(gFrees == gAllocs);
    std::printf("unlit draws adaptor OK\n");
    return 0;
}
