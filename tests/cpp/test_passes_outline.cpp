// test_passes_outline.cpp — vqhip::OutlinePass (include/vqhip_passes.hpp; docs/DESIGN_DETAILS.md §7.21) against the stand-in of the engine's RenderPass.h, host-only:
// the adaptor turns the selected draws of RenderOutline and the scene colour into one vqhip_outline call, counts the triangles for the work size, owns the work
// buffer, keeps the library's status and refuses bad parameter blocks without calling.
// The entry point, its size function and the two allocator calls are defined HERE (the executable's definitions are the ones the adaptor binds to): nothing
// touches a device. Built by tests/test_outline_cpu.py with the command line tests/test_masked_depth_cpu.py uses.
#ifndef VQHIP_ENGINE_RENDERPASS_H
#define VQHIP_ENGINE_RENDERPASS_H "mock_engine/RenderPass.h"
#endif
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include "vqhip_passes.hpp"

static vqhip_outline_targets gTargets;
static std::vector<vqhip_outline_draw> gDraws;
static int gWidth = 0, gHeight = 0, gCalls = 0, gAllocs = 0, gFrees = 0, gStatus = VQHIP_OK;
static vqhip_ctx* gCtx = nullptr; static void* gStream = nullptr; static void* gWork = nullptr; static size_t gWorkBytes = 0, gAllocBytes = 0;
static uint64_t gSizeTriangles = 0;
static bool gDrawsNull = false;

extern "C" size_t vqhip_outline_work_bytes(uint64_t triangles) { gSizeTriangles = triangles; return triangles >= 1000000 ? 0 : 512 + (size_t)triangles * 900; }
extern "C" int vqhip_outline(vqhip_ctx* ctx, void* stream, const vqhip_outline_draw* draws, int numDraws, int width, int height, const vqhip_outline_targets* out,
                             void* work, size_t workBytes) {
    ++gCalls; gCtx = ctx; gStream = stream; gDrawsNull = draws == nullptr; gDraws.assign(draws, draws + numDraws); gWidth = width; gHeight = height; gTargets = *out;
    gWork = work; gWorkBytes = workBytes;
    return gStatus;
}
extern "C" hipError_t hipMalloc(void** p, size_t bytes) { ++gAllocs; gAllocBytes = bytes; *p = std::malloc(bytes); return *p ? hipSuccess : hipErrorOutOfMemory; }
extern "C" hipError_t hipFree(void* p) { ++gFrees; std::free(p); return hipSuccess; }

#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static int adaptor(vqhip_ctx* ctx) {
    std::shared_ptr<::IRenderPass> pPass = std::make_shared<vqhip::OutlinePass>(ctx);
    vqhip::OutlinePass* pass = static_cast<vqhip::OutlinePass*>(pPass.get());
    EXPECT(pPass->Initialize());
    EXPECT(!std::make_shared<vqhip::OutlinePass>(nullptr)->Initialize());
    pPass->RecordCommands(nullptr);
    EXPECT(pass->LastStatus() == VQHIP_ERR_INVALID_ARG && gCalls == 0);
    vqhip::OutlinePass::FDrawParameters p;
    EXPECT(p.SceneColor == nullptr && p.Selection == nullptr && p.Writer == nullptr && p.SceneColorPitch == 0);
    pPass->RecordCommands(&p);                                                                                  // no scene colour: no call
    EXPECT(pass->LastStatus() == VQHIP_ERR_INVALID_ARG && gCalls == 0 && gAllocs == 0);

    static uint16_t color[4]; static uint8_t sel[1]; static uint32_t wr[1]; static VQ_OutlineData cbs[2];      // addresses only
    std::vector<vqhip_outline_draw> draws(3);
    std::memset(draws.data(), 0, draws.size() * sizeof(draws[0]));
    draws[0].mesh.numIndices = 36; draws[0].cb = cbs; draws[1].mesh.numIndices = 0; draws[1].cb = cbs; draws[2].mesh.numIndices = 300; draws[2].cb = cbs + 1;
    p.Stream = &p; p.Draws = &draws; p.SceneColor = color; p.SceneColorPitch = 2048; p.Selection = sel; p.Writer = wr;
    pPass->OnCreateWindowSizeDependentResources(1920, 1080, nullptr);
    gStatus = 4321;                                                                                             // the library's status is kept
    pPass->RecordCommands(&p);
    EXPECT(gCalls == 1 && pass->LastStatus() == 4321);
    gStatus = VQHIP_OK;
    pPass->RecordCommands(&p);
    EXPECT(gCalls == 2 && pass->LastStatus() == VQHIP_OK);
    EXPECT(gCtx == ctx && gStream == &p && gWidth == 1920 && gHeight == 1080 && gDraws.size() == 3 && std::memcmp(gDraws.data(), draws.data(), 3 * sizeof(draws[0])) == 0);
    EXPECT(gTargets.sceneColor == color && gTargets.pitch == 2048 && gTargets.selection == sel && gTargets.writer == wr && gTargets.selection_pitch == 0 &&
           gTargets.writer_pitch == 0 && gTargets.reserved == 0);
    EXPECT(gSizeTriangles == 12 + 100 && gAllocs == 1 && gAllocBytes == 512 + 112 * 900 && gWork == pass->GetWorkBuffer() && gWorkBytes == gAllocBytes && gFrees == 0);

    p.Selection = nullptr; p.Writer = nullptr; p.SceneColorPitch = 0;                                           // the engine's own output alone
    draws.resize(1);                                                                                            // fewer triangles: the buffer is kept
    pPass->RecordCommands(&p);
    EXPECT(gCalls == 3 && gAllocs == 1 && gSizeTriangles == 12 && gTargets.selection == nullptr && gTargets.writer == nullptr && gTargets.pitch == 0 && gWorkBytes == 512 + 112 * 900);
    draws.resize(2); draws[1] = draws[0]; draws[1].mesh.numIndices = 3000;                                      // more: it grows (the old one is freed first)
    pPass->RecordCommands(&p);
    EXPECT(gCalls == 4 && gAllocs == 2 && gFrees == 1 && gWorkBytes == 512 + 1012 * 900);
    p.Draws = nullptr;                                                                                          // nothing selected: the call is made, with no draws
    pPass->RecordCommands(&p);
    EXPECT(gCalls == 5 && gDrawsNull && gDraws.empty() && gSizeTriangles == 0 && pass->LastStatus() == VQHIP_OK && gAllocs == 2);
    std::vector<vqhip_outline_draw> none;
    p.Draws = &none;
    pPass->RecordCommands(&p);
    EXPECT(gCalls == 6 && gDrawsNull && gDraws.empty());
    draws[1].mesh.numIndices = 3000000;                                                                         // beyond the library's limit: the size function says 0, no call
    p.Draws = &draws;
    pPass->RecordCommands(&p);
    EXPECT(gCalls == 6 && pass->LastStatus() == VQHIP_ERR_HIP);
    pPass->Destroy();
    EXPECT(gFrees == 2 && pass->GetWorkBuffer() == nullptr && pass->GetWorkBytes() == 0);
    return 0;
}

int main() {
    static_assert(std::is_base_of<::IRenderPass, vqhip::OutlinePass>::value, "the adaptor derives from the engine's IRenderPass");
    vqhip_ctx* ctx = reinterpret_cast<vqhip_ctx*>(static_cast<uintptr_t>(0x1000));      // never dereferenced: the library call is the recorder above
    if (int rc = adaptor(ctx)) return rc;
    EXPECT(gFrees == gAllocs);
    std::printf("outline adaptor OK\n");
    return 0;
}
