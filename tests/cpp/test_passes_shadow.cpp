// test_passes_shadow.cpp — vqhip::ShadowDepthPass (include/vqhip_passes.hpp) against the stand-in of the engine's RenderPass.h, host-only: the adaptor turns what
// RenderDirectionalShadowMaps / RenderSpotShadowMaps / RenderPointShadowMaps hold per view into ONE vqhip_shadow_depth call — slices of the three depth arrays, z/w for
// the directional and spot views, LINEAR_DEPTH with the caster's position and range for the point faces, views with an empty draw list skipped as the engine skips
// them —, sizes and owns the work buffer, keeps the library's status and refuses a NULL parameter block without calling the library.
// vqhip_shadow_depth, its size function and the two allocator calls are defined HERE (the executable's definitions are the ones the adaptor binds to): nothing
// touches a device. Built by tests/test_shadow_raster_cpu.py with the command line tests/cpp/Makefile uses for test_passes_engine.
#ifndef VQHIP_ENGINE_RENDERPASS_H
#define VQHIP_ENGINE_RENDERPASS_H "mock_engine/RenderPass.h"
#endif
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include "vqhip_passes.hpp"

static vqhip_shadow_view gViews[64];
static int gNumViews = 0, gCalls = 0, gSizeCalls = 0, gAllocs = 0, gFrees = 0;
static vqhip_ctx* gCtx = nullptr; static void* gStream = nullptr; static void* gWork = nullptr; static size_t gWorkBytes = 0, gAllocBytes = 0;
static uint64_t gSizeTriangles = 0;

extern "C" size_t vqhip_shadow_depth_work_bytes(uint64_t instancedTriangles, int numViews) {
    ++gSizeCalls; gSizeTriangles = instancedTriangles;
    return numViews == VQHIP_SHADOW_MAX_VIEWS ? 1000 + (size_t)instancedTriangles * 10 : 0;
}
extern "C" int vqhip_shadow_depth(vqhip_ctx* ctx, void* stream, const vqhip_shadow_view* views, int numViews, void* work, size_t workBytes) {
    ++gCalls; gCtx = ctx; gStream = stream; gNumViews = numViews; gWork = work; gWorkBytes = workBytes;
    std::memcpy(gViews, views, sizeof(vqhip_shadow_view) * (size_t)numViews);
    return 4321;
}
extern "C" hipError_t hipMalloc(void** p, size_t bytes) { ++gAllocs; gAllocBytes = bytes; *p = std::malloc(bytes); return *p ? hipSuccess : hipErrorOutOfMemory; }
extern "C" hipError_t hipFree(void* p) { ++gFrees; std::free(p); return hipSuccess; }

#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static vqhip_shadow_draw makeDraw(uint32_t numIndices, uint32_t numInstances) {
    vqhip_shadow_draw d;
    std::memset(&d, 0, sizeof(d));
    d.mesh.numIndices = numIndices; d.mesh.indexBits = 16; d.mesh.strideBytes = 44; d.numInstances = numInstances; d.cullMode = VQHIP_CULL_BACK;
    return d;
}

int main() {
    static_assert(std::is_base_of<::IRenderPass, vqhip::ShadowDepthPass>::value, "the adaptor derives from the engine's IRenderPass");
    vqhip_ctx* ctx = reinterpret_cast<vqhip_ctx*>(static_cast<uintptr_t>(0x1000));      // never dereferenced: the library call is the recorder above
    {
        std::shared_ptr<::IRenderPass> pPass = std::make_shared<vqhip::ShadowDepthPass>(ctx);
        vqhip::ShadowDepthPass* pass = static_cast<vqhip::ShadowDepthPass*>(pPass.get());
        EXPECT(pPass->Initialize());
        EXPECT(!std::make_shared<vqhip::ShadowDepthPass>(nullptr)->Initialize());
        pPass->RecordCommands(nullptr);                                                  // the NULL refusal
        EXPECT(pass->LastStatus() == VQHIP_ERR_INVALID_ARG && gCalls == 0);

        static float dir[4], spot[4], point[4];                                         // addresses only
        std::vector<vqhip_shadow_draw> dirDraws = { makeDraw(36, 2), makeDraw(300, 1) };      // 24 + 100 triangles
        std::vector<vqhip_shadow_draw> spot1 = { makeDraw(30, 128) };                         // 1280
        std::vector<vqhip_shadow_draw> empty;
        std::vector<vqhip_shadow_draw> face[6];
        for (int f = 0; f < 6; ++f) if (f != 3) face[f] = { makeDraw(3 * (f + 1), 1) };       // 1 + 2 + 3 + 5 + 6 = 17; face 3 draws nothing
        vqhip::ShadowDepthPass::FDrawParameters p;
        EXPECT(p.DirectionalDim == 2048 && p.SpotDim == 1024 && p.PointDim == 1024);
        p.Stream = &p; p.ShadowMapsDirectional = dir; p.ShadowMapsSpot = spot; p.ShadowMapsPoint = point;
        p.DirectionalDim = 64; p.SpotDim = 32; p.PointDim = 16;
        p.DirectionalDraws = &dirDraws;
        p.NumSpotShadowViews = 2; p.SpotDraws[0] = &empty; p.SpotDraws[1] = &spot1;           // spot 0 has nothing to draw: skipped
        p.NumPointShadowViews = 2;                                                            // light 0 draws nothing at all, light 1 five faces
        for (int f = 0; f < 6; ++f) p.PointDraws[6 + f] = &face[f];
        p.PointPosition[1] = VQ_float3{ 1.0f, 2.0f, 3.0f }; p.PointRange[1] = 25.0f;
        pPass->RecordCommands(&p);
        EXPECT(gCalls == 1 && pass->LastStatus() == 4321 && pass->LastViewCount() == 7);      // the library's status is kept
        EXPECT(gCtx == ctx && gStream == &p && gNumViews == 7);
        EXPECT(gSizeTriangles == 124 + 1280 + 17 && gAllocs == 1 && gAllocBytes == 1000 + 1421 * 10);
        EXPECT(gWork == pass->GetWorkBuffer() && gWorkBytes == gAllocBytes && pass->GetWorkBytes() == gAllocBytes);
        EXPECT(gViews[0].depth == dir && gViews[0].dim == 64 && gViews[0].linearDepth == 0 && gViews[0].pitchBytes == 0 && gViews[0].draws == dirDraws.data() && gViews[0].numDraws == 2);
        EXPECT(gViews[1].depth == spot + 1 * 32 * 32 && gViews[1].dim == 32 && gViews[1].linearDepth == 0 && gViews[1].draws == spot1.data() && gViews[1].numDraws == 1);
        const int faces[5] = { 0, 1, 2, 4, 5 };
        for (int k = 0; k < 5; ++k) {
            const vqhip_shadow_view& v = gViews[2 + k];
            EXPECT(v.depth == point + (size_t)(6 + faces[k]) * 16 * 16 && v.dim == 16 && v.linearDepth == 1 && v.draws == face[faces[k]].data() && v.numDraws == 1);
            EXPECT(v.cameraPosition.x == 1.0f && v.cameraPosition.y == 2.0f && v.cameraPosition.z == 3.0f && v.farPlane == 25.0f);
        }
        pPass->RecordCommands(&p);                                                            // the same frame again: the buffer is kept
        EXPECT(gCalls == 2 && gAllocs == 1 && gFrees == 0);
        dirDraws.push_back(makeDraw(3000, 1));                                                // a frame that needs more: freed and sized anew
        pPass->RecordCommands(&p);
        EXPECT(gCalls == 3 && gAllocs == 2 && gFrees == 1 && gAllocBytes == 1000 + 2421 * 10 && gViews[0].numDraws == 3);
        EXPECT(pass->Reserve(10) && gAllocs == 2);                                            // smaller: nothing happens
        p.DirectionalDraws = nullptr; p.NumSpotShadowViews = 0; p.NumPointShadowViews = 0;    // nothing casts: no call, status OK
        pPass->RecordCommands(&p);
        EXPECT(gCalls == 3 && pass->LastStatus() == VQHIP_OK && pass->LastViewCount() == 0);
        p.NumSpotShadowViews = VQ_NUM_SHADOWING_LIGHTS__SPOT + 1;
        pPass->RecordCommands(&p);
        EXPECT(gCalls == 3 && pass->LastStatus() == VQHIP_ERR_INVALID_ARG);
    }
    EXPECT(gFrees == 2);                                                                      // the destructor releases the buffer
    std::printf("shadow depth adaptor OK\n");
    return 0;
}
