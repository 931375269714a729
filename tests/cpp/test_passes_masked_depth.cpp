// test_passes_masked_depth.cpp — vqhip::MaskedDepthPrePass and vqhip::MaskedShadowDepthPass (include/vqhip_passes.hpp) against the stand-in of the engine's
// RenderPass.h, host-only: the adaptors turn the draw lists of RenderDepthPrePass / DrawShadowViewMeshList, the per-draw material indices and the host material
// array into one vqhip_scene_masked_depth / vqhip_shadow_masked_depth call each — material and texDiffuseAlpha pointers built per draw, the masked instanced
// triangles counted by the header's rule for the work size —, own the work buffer, keep the library's status and refuse bad parameter blocks without calling.
// The two entry points, their size functions and the two allocator calls are defined HERE (the executable's definitions are the ones the adaptors bind to):
// nothing touches a device. Built by tests/test_masked_depth_cpu.py with the command line tests/test_scene_depth_cpu.py uses.
#ifndef VQHIP_ENGINE_RENDERPASS_H
#define VQHIP_ENGINE_RENDERPASS_H "mock_engine/RenderPass.h"
#endif
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include "vqhip_passes.hpp"

static vqhip_scene_depth_targets gTargets;
static std::vector<vqhip_scene_masked_depth_draw> gDraws;
static std::vector<vqhip_shadow_masked_view> gViews;
static std::vector<std::vector<vqhip_shadow_masked_draw>> gViewDraws;
static int gWidth = 0, gHeight = 0, gSamples = 0, gSceneCalls = 0, gShadowCalls = 0, gAllocs = 0, gFrees = 0, gSizeDraws = 0, gSizeViews = 0;
static vqhip_ctx* gCtx = nullptr; static void* gStream = nullptr; static void* gWork = nullptr; static size_t gWorkBytes = 0, gAllocBytes = 0;
static uint64_t gSizeTriangles = 0, gSizeMasked = 0;

extern "C" size_t vqhip_scene_masked_depth_work_bytes(uint64_t instancedTriangles, uint64_t maskedInstancedTriangles, int numDraws) {
    gSizeTriangles = instancedTriangles; gSizeMasked = maskedInstancedTriangles; gSizeDraws = numDraws;
    return 1000 + (size_t)instancedTriangles * 10 + (size_t)maskedInstancedTriangles * 64 + (size_t)numDraws * 48;
}
extern "C" int vqhip_scene_masked_depth(vqhip_ctx* ctx, void* stream, const vqhip_scene_masked_depth_draw* draws, int numDraws, int width, int height, int samples,
                                        const vqhip_scene_depth_targets* out, void* work, size_t workBytes) {
    ++gSceneCalls; gCtx = ctx; gStream = stream; gDraws.assign(draws, draws + numDraws); gWidth = width; gHeight = height; gSamples = samples; gTargets = *out;
    gWork = work; gWorkBytes = workBytes;
    return 4321;
}
extern "C" size_t vqhip_shadow_masked_depth_work_bytes(uint64_t instancedTriangles, uint64_t maskedInstancedTriangles, int numViews, int numDraws) {
    gSizeTriangles = instancedTriangles; gSizeMasked = maskedInstancedTriangles; gSizeViews = numViews; gSizeDraws = numDraws;
    return 2000 + (size_t)instancedTriangles * 10 + (size_t)maskedInstancedTriangles * 64 + (size_t)numDraws * 48;
}
extern "C" int vqhip_shadow_masked_depth(vqhip_ctx* ctx, void* stream, const vqhip_shadow_masked_view* views, int numViews, void* work, size_t workBytes) {
    ++gShadowCalls; gCtx = ctx; gStream = stream; gViews.assign(views, views + numViews); gWork = work; gWorkBytes = workBytes;
    gViewDraws.clear();
    for (int v = 0; v < numViews; ++v) gViewDraws.emplace_back(views[v].draws, views[v].draws + views[v].numDraws);
    return 8765;
}
extern "C" hipError_t hipMalloc(void** p, size_t bytes) { ++gAllocs; gAllocBytes = bytes; *p = std::malloc(bytes); return *p ? hipSuccess : hipErrorOutOfMemory; }
extern "C" hipError_t hipFree(void* p) { ++gFrees; std::free(p); return hipSuccess; }

#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static vqhip_scene_depth_draw sceneDraw(uint32_t numIndices, uint32_t numInstances) {
    vqhip_scene_depth_draw d;
    std::memset(&d, 0, sizeof(d));
    d.mesh.numIndices = numIndices; d.mesh.indexBits = 16; d.mesh.strideBytes = 44; d.numInstances = numInstances; d.cullMode = VQHIP_CULL_NONE;
    return d;
}
static vqhip_shadow_draw shadowDraw(uint32_t numIndices, uint32_t numInstances) {
    vqhip_shadow_draw d;
    std::memset(&d, 0, sizeof(d));
    d.mesh.numIndices = numIndices; d.mesh.indexBits = 32; d.mesh.strideBytes = 44; d.numInstances = numInstances; d.cullMode = VQHIP_CULL_NONE;
    return d;
}

static int sceneAdaptor(vqhip_ctx* ctx, const vqhip_material* mats) {
    std::shared_ptr<::IRenderPass> pPass = std::make_shared<vqhip::MaskedDepthPrePass>(ctx);
    vqhip::MaskedDepthPrePass* pass = static_cast<vqhip::MaskedDepthPrePass*>(pPass.get());
    EXPECT(pPass->Initialize());
    EXPECT(!std::make_shared<vqhip::MaskedDepthPrePass>(nullptr)->Initialize());
    pPass->RecordCommands(nullptr);
    EXPECT(pass->LastStatus() == VQHIP_ERR_INVALID_ARG && gSceneCalls == 0);

    static float depth[4]; static uint32_t prim[4], lp0[4]; static uint8_t cov0[4];                             // addresses only
    std::vector<vqhip_scene_depth_draw> draws = { sceneDraw(36, 2), sceneDraw(300, 64), sceneDraw(6, 50), sceneDraw(12, 1) };   // 24, 6400, 100, 4 triangles
    std::vector<int32_t> index = { 0, -1, 1, 2 };                                                             // opaque material, none, masked, masked without the diffuse bit
    vqhip::MaskedDepthPrePass::FDrawParameters p;
    EXPECT(p.bMSAA && p.NumLayers == 0 && p.MaterialIndex == nullptr && p.Materials == nullptr);
    p.Stream = &p; p.Draws = &draws; p.SceneDepth = depth; p.Primitive = prim; p.NumLayers = 1; p.Coverage[0] = cov0; p.LayerPrimitive[0] = lp0;
    p.MaterialIndex = &index; p.Materials = mats; p.NumMaterials = 3;
    pPass->OnCreateWindowSizeDependentResources(1920, 1080, nullptr);
    pPass->RecordCommands(&p);
    EXPECT(gSceneCalls == 1 && pass->LastStatus() == 4321);                                                   // the library's status is kept
    EXPECT(gCtx == ctx && gStream == &p && gDraws.size() == 4 && gWidth == 1920 && gHeight == 1080 && gSamples == 4);
    EXPECT(gDraws[0].material == mats && gDraws[1].material == nullptr && gDraws[2].material == mats + 1 && gDraws[3].material == mats + 2);
    for (size_t d = 0; d < 4; ++d) EXPECT(std::memcmp(&gDraws[d].draw, &draws[d], sizeof(vqhip_scene_depth_draw)) == 0);
    EXPECT(gSizeTriangles == 6528 && gSizeMasked == 104 && gSizeDraws == 4 && pass->LastMaskedTriangles() == 104);      // the flag decides, not the diffuse bit
    EXPECT(gAllocs == 1 && gAllocBytes == 1000 + 6528 * 10 + 104 * 64 + 4 * 48 && gWork == pass->GetWorkBuffer() && gWorkBytes == gAllocBytes);
    EXPECT(gTargets.depth == depth && gTargets.primitive == prim && gTargets.layers == 1 && gTargets.coverage[0] == cov0 && gTargets.layerPrimitive[0] == lp0 &&
           gTargets.coverage[1] == nullptr && gTargets.pitch == 0 && gTargets.reserved == 0);
    pPass->RecordCommands(&p);                                                                                // the same frame again: the buffer is kept
    EXPECT(gSceneCalls == 2 && gAllocs == 1 && gFrees == 0);
    p.MaterialIndex = nullptr;                                                                                // no list: every draw opaque, a smaller need
    p.bMSAA = false;
    pPass->RecordCommands(&p);
    EXPECT(gSceneCalls == 3 && gSamples == 1 && gTargets.layers == 0 && gSizeMasked == 0 && gAllocs == 1);
    for (size_t d = 0; d < 4; ++d) EXPECT(gDraws[d].material == nullptr);
    std::vector<int32_t> all = { 1, 1, 1, 1 };                                                                // a frame that needs more: freed and sized anew
    p.MaterialIndex = &all;
    pPass->RecordCommands(&p);
    EXPECT(gSceneCalls == 4 && gSizeMasked == 6528 && gAllocs == 2 && gFrees == 1);
    std::vector<int32_t> bad = { 0, 3, 0, 0 }, shorter = { 0, 0, 0 };                                         // an index past the array, a list of the wrong length
    p.MaterialIndex = &bad;
    pPass->RecordCommands(&p);
    EXPECT(gSceneCalls == 4 && pass->LastStatus() == VQHIP_ERR_INVALID_ARG);
    p.MaterialIndex = &shorter;
    pPass->RecordCommands(&p);
    EXPECT(gSceneCalls == 4 && pass->LastStatus() == VQHIP_ERR_INVALID_ARG);
    p.MaterialIndex = &index; p.Materials = nullptr;                                                          // indices without an array
    pPass->RecordCommands(&p);
    EXPECT(gSceneCalls == 4 && pass->LastStatus() == VQHIP_ERR_INVALID_ARG);
    p.Draws = nullptr; p.MaterialIndex = nullptr;                                                             // nothing to draw: the call still clears the target
    pPass->RecordCommands(&p);
    EXPECT(gSceneCalls == 5 && gDraws.empty() && gTargets.depth == depth);
    return 0;
}

static int shadowAdaptor(vqhip_ctx* ctx, const vqhip_material* mats) {
    std::shared_ptr<::IRenderPass> pPass = std::make_shared<vqhip::MaskedShadowDepthPass>(ctx);
    vqhip::MaskedShadowDepthPass* pass = static_cast<vqhip::MaskedShadowDepthPass*>(pPass.get());
    EXPECT(pPass->Initialize());
    pPass->RecordCommands(nullptr);
    EXPECT(pass->LastStatus() == VQHIP_ERR_INVALID_ARG && gShadowCalls == 0);
    const int allocs0 = gAllocs, frees0 = gFrees;

    static float dirMap[4], spotMaps[4 * 2 * 2], pointMaps[6 * 2 * 2];
    std::vector<vqhip_shadow_draw> dir = { shadowDraw(30, 1), shadowDraw(6, 10) }, spot1 = { shadowDraw(12, 3) }, face2 = { shadowDraw(6, 1), shadowDraw(9, 2), shadowDraw(3, 1) };
    std::vector<int32_t> dirIndex = { 0, 1 }, faceIndex = { 2, -1, 1 };                                        // spot1 has no list: opaque
    vqhip::MaskedShadowDepthPass::FDrawParameters p;
    p.Stream = &p; p.ShadowMapsDirectional = dirMap; p.DirectionalDim = 2; p.ShadowMapsSpot = spotMaps; p.SpotDim = 2; p.ShadowMapsPoint = pointMaps; p.PointDim = 2;
    p.DirectionalDraws = &dir; p.DirectionalMaterialIndex = &dirIndex;
    p.NumSpotShadowViews = 2; p.SpotDraws[1] = &spot1;                                                        // spot view 0 has nothing to draw: skipped
    p.NumPointShadowViews = 1; p.PointDraws[2] = &face2; p.PointMaterialIndex[2] = &faceIndex;
    p.PointPosition[0] = VQ_float3{ 1.0f, 2.0f, 3.0f }; p.PointRange[0] = 25.0f;
    p.Materials = mats; p.NumMaterials = 3;
    pPass->RecordCommands(&p);
    EXPECT(gShadowCalls == 1 && pass->LastStatus() == 8765 && pass->LastViewCount() == 3 && gViews.size() == 3 && gCtx == ctx && gStream == &p);
    EXPECT(gViews[0].depth == dirMap && gViews[0].dim == 2 && gViews[0].linearDepth == 0 && gViews[0].numDraws == 2);
    EXPECT(gViews[1].depth == spotMaps + 4 && gViews[1].linearDepth == 0 && gViews[1].numDraws == 1);
    EXPECT(gViews[2].depth == pointMaps + 2 * 4 && gViews[2].linearDepth == 1 && gViews[2].numDraws == 3 && gViews[2].farPlane == 25.0f && gViews[2].cameraPosition.y == 2.0f);
    EXPECT(gViewDraws[0][0].texDiffuseAlpha == nullptr && gViewDraws[0][1].texDiffuseAlpha == &mats[1].texDiffuse);          // material 0 is not flagged
    EXPECT(gViewDraws[1][0].texDiffuseAlpha == nullptr);
    EXPECT(gViewDraws[2][0].texDiffuseAlpha == &mats[2].texDiffuse && gViewDraws[2][1].texDiffuseAlpha == nullptr && gViewDraws[2][2].texDiffuseAlpha == &mats[1].texDiffuse);
    EXPECT(std::memcmp(&gViewDraws[2][1].draw, &face2[1], sizeof(vqhip_shadow_draw)) == 0 && std::memcmp(&gViewDraws[0][1].draw, &dir[1], sizeof(vqhip_shadow_draw)) == 0);
    // triangles: 10 + 20 | 12 | 2 + 6 + 1 = 51; masked: 20 (dir 1) + 2 + 1 (face) = 23; six draws in all
    EXPECT(gSizeTriangles == 51 && gSizeMasked == 23 && gSizeDraws == 6 && gSizeViews == VQHIP_SHADOW_MAX_VIEWS && pass->LastMaskedTriangles() == 23);
    EXPECT(gAllocs == allocs0 + 1 && gAllocBytes == 2000 + 51 * 10 + 23 * 64 + 6 * 48 && gWork == pass->GetWorkBuffer() && gWorkBytes == gAllocBytes);
    pPass->RecordCommands(&p);
    EXPECT(gShadowCalls == 2 && gAllocs == allocs0 + 1 && gFrees == frees0);
    std::vector<int32_t> wrong = { 0 };                                                                        // a list of the wrong length, an index past the array
    p.DirectionalMaterialIndex = &wrong;
    pPass->RecordCommands(&p);
    EXPECT(gShadowCalls == 2 && pass->LastStatus() == VQHIP_ERR_INVALID_ARG);
    std::vector<int32_t> past = { 0, 7 };
    p.DirectionalMaterialIndex = &past;
    pPass->RecordCommands(&p);
    EXPECT(gShadowCalls == 2 && pass->LastStatus() == VQHIP_ERR_INVALID_ARG);
    p.DirectionalMaterialIndex = &dirIndex; p.NumSpotShadowViews = VQ_NUM_SHADOWING_LIGHTS__SPOT + 1;
    pPass->RecordCommands(&p);
    EXPECT(gShadowCalls == 2 && pass->LastStatus() == VQHIP_ERR_INVALID_ARG);
    p.NumSpotShadowViews = 0; p.NumPointShadowViews = 0; p.DirectionalDraws = nullptr;                        // nothing casts a shadow: no call, no error
    pPass->RecordCommands(&p);
    EXPECT(gShadowCalls == 2 && pass->LastStatus() == VQHIP_OK && pass->LastViewCount() == 0);
    return 0;
}

int main() {
    static_assert(std::is_base_of<::IRenderPass, vqhip::MaskedDepthPrePass>::value && std::is_base_of<::IRenderPass, vqhip::MaskedShadowDepthPass>::value,
                  "the adaptors derive from the engine's IRenderPass");
    vqhip_ctx* ctx = reinterpret_cast<vqhip_ctx*>(static_cast<uintptr_t>(0x1000));      // never dereferenced: the library calls are the recorders above
    static vqhip_material mats[3];                                                       // 0: opaque; 1: masked with a diffuse map; 2: masked, diffuse bit clear, null SRV
    std::memset(mats, 0, sizeof(mats));
    mats[1].texDiffuse.reserved = VQHIP_MATERIAL_ALPHA_MASKED; mats[1].data.textureConfig = 1.0f; mats[1].texDiffuse.width = mats[1].texDiffuse.height = 8; mats[1].texDiffuse.mips = 4;
    mats[2].texDiffuse.reserved = VQHIP_MATERIAL_ALPHA_MASKED;
    const int frees0 = gFrees;
    if (int rc = sceneAdaptor(ctx, mats)) return rc;
    EXPECT(gFrees == frees0 + 2);                                                        // the destructor releases the buffer
    const int frees1 = gFrees;
    if (int rc = shadowAdaptor(ctx, mats)) return rc;
    EXPECT(gFrees == frees1 + 1);
    std::printf("masked depth adaptors OK\n");
    return 0;
}
