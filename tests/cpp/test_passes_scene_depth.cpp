// test_passes_scene_depth.cpp — vqhip::DepthPrePass (include/vqhip_passes.hpp) against the stand-in of the engine's RenderPass.h, host-only: the adaptor turns what
// RenderDepthPrePass holds — the main view's draw list, the window's W and H, bMSAA — into one vqhip_scene_depth call (4 samples when bMSAA, else 1; layers only with
// MSAA), sizes and owns the work buffer, keeps the library's status and refuses a NULL parameter block without calling the library.
// vqhip_scene_depth, its size function and the two allocator calls are defined HERE (the executable's definitions are the ones the adaptor binds to): nothing
// touches a device. Built by tests/test_scene_depth_cpu.py with the command line tests/test_shadow_raster_cpu.py uses.
#ifndef VQHIP_ENGINE_RENDERPASS_H
#define VQHIP_ENGINE_RENDERPASS_H "mock_engine/RenderPass.h"
#endif
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include "vqhip_passes.hpp"

static vqhip_scene_depth_targets gTargets;
static const vqhip_scene_depth_draw* gDraws = nullptr;
static int gNumDraws = 0, gWidth = 0, gHeight = 0, gSamples = 0, gCalls = 0, gSizeCalls = 0, gAllocs = 0, gFrees = 0;
static vqhip_ctx* gCtx = nullptr; static void* gStream = nullptr; static void* gWork = nullptr; static size_t gWorkBytes = 0, gAllocBytes = 0;
static uint64_t gSizeTriangles = 0;

extern "C" size_t vqhip_scene_depth_work_bytes(uint64_t instancedTriangles) {
    ++gSizeCalls; gSizeTriangles = instancedTriangles;
    return 1000 + (size_t)instancedTriangles * 10;
}
extern "C" int vqhip_scene_depth(vqhip_ctx* ctx, void* stream, const vqhip_scene_depth_draw* draws, int numDraws, int width, int height, int samples,
                                 const vqhip_scene_depth_targets* out, void* work, size_t workBytes) {
    ++gCalls; gCtx = ctx; gStream = stream; gDraws = draws; gNumDraws = numDraws; gWidth = width; gHeight = height; gSamples = samples; gTargets = *out;
    gWork = work; gWorkBytes = workBytes;
    return 4321;
}
extern "C" hipError_t hipMalloc(void** p, size_t bytes) { ++gAllocs; gAllocBytes = bytes; *p = std::malloc(bytes); return *p ? hipSuccess : hipErrorOutOfMemory; }
extern "C" hipError_t hipFree(void* p) { ++gFrees; std::free(p); return hipSuccess; }

#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static vqhip_scene_depth_draw makeDraw(uint32_t numIndices, uint32_t numInstances) {
    vqhip_scene_depth_draw d;
    std::memset(&d, 0, sizeof(d));
    d.mesh.numIndices = numIndices; d.mesh.indexBits = 16; d.mesh.strideBytes = 44; d.numInstances = numInstances; d.cullMode = VQHIP_CULL_BACK;
    return d;
}

int main() {
    static_assert(std::is_base_of<::IRenderPass, vqhip::DepthPrePass>::value, "the adaptor derives from the engine's IRenderPass");
    vqhip_ctx* ctx = reinterpret_cast<vqhip_ctx*>(static_cast<uintptr_t>(0x1000));      // never dereferenced: the library call is the recorder above
    {
        std::shared_ptr<::IRenderPass> pPass = std::make_shared<vqhip::DepthPrePass>(ctx);
        vqhip::DepthPrePass* pass = static_cast<vqhip::DepthPrePass*>(pPass.get());
        EXPECT(pPass->Initialize());
        EXPECT(!std::make_shared<vqhip::DepthPrePass>(nullptr)->Initialize());
        pPass->RecordCommands(nullptr);                                                  // the NULL refusal
        EXPECT(pass->LastStatus() == VQHIP_ERR_INVALID_ARG && gCalls == 0);

        static float depth[4]; static uint32_t prim[4], lp0[4], lp1[4]; static uint8_t cov0[4], cov1[4];       // addresses only
        std::vector<vqhip_scene_depth_draw> draws = { makeDraw(36, 2), makeDraw(300, 64) };                  // 24 + 6400 triangles
        vqhip::DepthPrePass::FDrawParameters p;
        EXPECT(p.bMSAA && p.NumLayers == 0);                                                                 // 4x MSAA is the engine's default
        p.Stream = &p; p.Draws = &draws; p.SceneDepth = depth; p.Primitive = prim;
        p.NumLayers = 2; p.Coverage[0] = cov0; p.Coverage[1] = cov1; p.LayerPrimitive[0] = lp0; p.LayerPrimitive[1] = lp1;
        pPass->OnCreateWindowSizeDependentResources(1920, 1080, nullptr);
        pPass->RecordCommands(&p);
        EXPECT(gCalls == 1 && pass->LastStatus() == 4321);                                                   // the library's status is kept
        EXPECT(gCtx == ctx && gStream == &p && gDraws == draws.data() && gNumDraws == 2);
        EXPECT(gWidth == 1920 && gHeight == 1080 && gSamples == 4);
        EXPECT(gSizeTriangles == 6424 && gAllocs == 1 && gAllocBytes == 1000 + 6424 * 10);
        EXPECT(gWork == pass->GetWorkBuffer() && gWorkBytes == gAllocBytes && pass->GetWorkBytes() == gAllocBytes);
        EXPECT(gTargets.depth == depth && gTargets.primitive == prim && gTargets.layers == 2 && gTargets.pitch == 0 && gTargets.coverage_pitch == 0 && gTargets.reserved == 0);
        EXPECT(gTargets.coverage[0] == cov0 && gTargets.coverage[1] == cov1 && gTargets.coverage[2] == nullptr && gTargets.layerPrimitive[0] == lp0 &&
               gTargets.layerPrimitive[1] == lp1 && gTargets.layerPrimitive[3] == nullptr);
        pPass->RecordCommands(&p);                                                                           // the same frame again: the buffer is kept
        EXPECT(gCalls == 2 && gAllocs == 1 && gFrees == 0);
        p.bMSAA = false;                                                                                     // one sample: no layers, whatever NumLayers says
        pPass->OnDestroyWindowSizeDependentResources();
        pPass->OnCreateWindowSizeDependentResources(1280, 720, nullptr);
        pPass->RecordCommands(&p);
        EXPECT(gCalls == 3 && gSamples == 1 && gWidth == 1280 && gHeight == 720 && gTargets.layers == 0 && gTargets.coverage[0] == nullptr && gTargets.layerPrimitive[0] == nullptr);
        draws.push_back(makeDraw(3000, 1));                                                                  // a frame that needs more: freed and sized anew
        pPass->RecordCommands(&p);
        EXPECT(gCalls == 4 && gAllocs == 2 && gFrees == 1 && gAllocBytes == 1000 + 7424 * 10 && gNumDraws == 3);
        EXPECT(pass->Reserve(10) && gAllocs == 2);                                                           // smaller: nothing happens
        p.Draws = nullptr;                                                                                   // nothing to draw: the call still clears the target
        pPass->RecordCommands(&p);
        EXPECT(gCalls == 5 && gNumDraws == 0 && gDraws == nullptr && gTargets.depth == depth);
        p.NumLayers = 5;
        pPass->RecordCommands(&p);
        EXPECT(gCalls == 5 && pass->LastStatus() == VQHIP_ERR_INVALID_ARG);
    }
    EXPECT(gFrees == 2);                                                                                     // the destructor releases the buffer
    std::printf("scene depth adaptor OK\n");
    return 0;
}
