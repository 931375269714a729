// test_passes_object_ids.cpp — vqhip::ObjectIDPass (include/vqhip_passes.hpp; docs/DESIGN_DETAILS.md §7.21) against the stand-in of the engine's RenderPass.h,
// host-only: the adaptor turns the main view's draw list, the per-draw ids and the host material array into the pass's own depth call (vqhip_scene_masked_depth at
// one sample, every cullMode forced to VQHIP_CULL_NONE) and a vqhip_object_ids call over that call's owner plane, owns the three planes and both work buffers,
// keeps the library's status, refuses bad parameter blocks without calling, and reads one pixel back.
// The entry points, their size functions, the allocator calls and the copy are defined HERE (the executable's definitions are the ones the adaptor binds to):
// nothing touches a device. Built by tests/test_object_ids_cpu.py with the command line tests/test_masked_depth_cpu.py uses.
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
static std::vector<vqhip_object_id_draw> gIdDraws;
static int gDepthCalls = 0, gIdsCalls = 0, gAllocs = 0, gFrees = 0, gCopies = 0, gSyncs = 0, gSamples = 0, gSizeDraws = 0, gIdsSizeDraws = 0;
static int gWidth = 0, gHeight = 0, gIdsWidth = 0, gIdsHeight = 0, gOwnerPitch = -1, gIdsPitch = -1, gDepthStatus = VQHIP_OK, gIdsStatus = VQHIP_OK, gOrder = 0, gDepthAt = 0, gIdsAt = 0;
static vqhip_ctx* gCtx = nullptr; static void* gStream = nullptr; static void* gCopyStream = nullptr; static void* gSyncStream = nullptr;
static void* gDepthWork = nullptr; static void* gIdsWork = nullptr; static size_t gDepthWorkBytes = 0, gIdsWorkBytes = 0;
static const uint32_t* gOwner = nullptr; static int32_t* gIds = nullptr; static const void* gCopySrc = nullptr; static size_t gCopyBytes = 0;
static uint64_t gSizeTriangles = 0, gSizeMasked = 0;
static std::vector<size_t> gAllocSizes;
static hipError_t gCopyResult = hipSuccess;

extern "C" size_t vqhip_scene_masked_depth_work_bytes(uint64_t instancedTriangles, uint64_t maskedInstancedTriangles, int numDraws) {
    gSizeTriangles = instancedTriangles; gSizeMasked = maskedInstancedTriangles; gSizeDraws = numDraws;
    return 1000 + (size_t)instancedTriangles * 10 + (size_t)maskedInstancedTriangles * 64 + (size_t)numDraws * 48;
}
extern "C" int vqhip_scene_masked_depth(vqhip_ctx* ctx, void* stream, const vqhip_scene_masked_depth_draw* draws, int numDraws, int width, int height, int samples,
                                        const vqhip_scene_depth_targets* out, void* work, size_t workBytes) {
    ++gDepthCalls; gDepthAt = ++gOrder; gCtx = ctx; gStream = stream; gDraws.assign(draws, draws + numDraws); gWidth = width; gHeight = height; gSamples = samples; gTargets = *out;
    gDepthWork = work; gDepthWorkBytes = workBytes;
    return gDepthStatus;
}
extern "C" size_t vqhip_object_ids_work_bytes(int numDraws) { gIdsSizeDraws = numDraws; return numDraws < 0 ? 0 : 300 + (size_t)numDraws * 32; }
extern "C" int vqhip_object_ids(vqhip_ctx* ctx, void* stream, const vqhip_object_id_draw* draws, int numDraws, int width, int height, const uint32_t* owner, int owner_pitch_px,
                                int32_t* ids, int ids_pitch_px, void* work, size_t workBytes) {
    ++gIdsCalls; gIdsAt = ++gOrder; gCtx = ctx; gStream = stream; gIdDraws.assign(draws, draws + numDraws); gIdsWidth = width; gIdsHeight = height; gOwner = owner; gOwnerPitch = owner_pitch_px;
    gIds = ids; gIdsPitch = ids_pitch_px; gIdsWork = work; gIdsWorkBytes = workBytes;
    return gIdsStatus;
}
extern "C" hipError_t hipMalloc(void** p, size_t bytes) { ++gAllocs; gAllocSizes.push_back(bytes); *p = std::calloc(1, bytes); return *p ? hipSuccess : hipErrorOutOfMemory; }
extern "C" hipError_t hipFree(void* p) { ++gFrees; std::free(p); return hipSuccess; }
extern "C" hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t stream) {
    ++gCopies; gCopySrc = src; gCopyBytes = bytes; gCopyStream = stream;
    if (kind != hipMemcpyDeviceToHost) return hipErrorInvalidValue;
    if (gCopyResult == hipSuccess) std::memcpy(dst, src, bytes);
    return gCopyResult;
}
extern "C" hipError_t hipStreamSynchronize(hipStream_t stream) { ++gSyncs; gSyncStream = stream; return hipSuccess; }

#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static int adaptor(vqhip_ctx* ctx, const vqhip_material* mats) {
    std::shared_ptr<::IRenderPass> pPass = std::make_shared<vqhip::ObjectIDPass>(ctx);
    vqhip::ObjectIDPass* pass = static_cast<vqhip::ObjectIDPass*>(pPass.get());
    EXPECT(pPass->Initialize());
    EXPECT(!std::make_shared<vqhip::ObjectIDPass>(nullptr)->Initialize());
    vqhip::ObjectIDPass::FDrawParameters p;
    pPass->RecordCommands(&p);                                                                                  // no window yet: no planes, no call
    EXPECT(pass->LastStatus() == VQHIP_ERR_INVALID_ARG && gDepthCalls == 0 && gIdsCalls == 0);
    vqhip::ObjectIDPass::FPixel px = pass->ReadBackPixel(0, 0);
    EXPECT(px.x == -1 && px.y == -1 && px.z == -1 && px.w == -1 && gCopies == 0);

    pPass->OnCreateWindowSizeDependentResources(40, 30, nullptr);
    EXPECT(gAllocs == 3 && gAllocSizes[0] == 40 * 30 * 4 && gAllocSizes[1] == 40 * 30 * 4 && gAllocSizes[2] == 40 * 30 * 16);
    EXPECT(pass->GetObjectIDs() && pass->GetDepth() && pass->GetOwner());
    pPass->RecordCommands(nullptr);
    EXPECT(pass->LastStatus() == VQHIP_ERR_INVALID_ARG && gDepthCalls == 0);

    static int32_t ids0[4 * 2], ids1[4], ids2[4 * 3];                                                          // addresses only
    std::vector<vqhip_scene_depth_draw> draws(3);
    std::memset(draws.data(), 0, draws.size() * sizeof(draws[0]));
    draws[0].mesh.numIndices = 36; draws[0].numInstances = 2; draws[0].cullMode = VQHIP_CULL_BACK;
    draws[1].mesh.numIndices = 0;  draws[1].numInstances = 1; draws[1].cullMode = VQHIP_CULL_FRONT;
    draws[2].mesh.numIndices = 6;  draws[2].numInstances = 3; draws[2].cullMode = VQHIP_CULL_NONE;
    std::vector<vqhip::ObjectIDPass::FObjectID> ids = { { ids0, 11, 21 }, { ids1, 12, 22 }, { ids2, 13, 23 } };
    std::vector<int32_t> matIndex = { 0, -1, 1 };
    p.Stream = &p; p.Draws = &draws; p.IDs = &ids; p.MaterialIndex = &matIndex; p.Materials = mats; p.NumMaterials = 2;
    pPass->RecordCommands(&p);
    EXPECT(pass->LastStatus() == VQHIP_OK && gDepthCalls == 1 && gIdsCalls == 1 && gDepthAt < gIdsAt);         // the depth call first, on the same stream
    EXPECT(gCtx == ctx && gStream == &p && gWidth == 40 && gHeight == 30 && gSamples == 1 && gIdsWidth == 40 && gIdsHeight == 30);
    EXPECT(gDraws.size() == 3 && gIdDraws.size() == 3);
    for (int d = 0; d < 3; ++d) {
        EXPECT(gDraws[d].draw.cullMode == VQHIP_CULL_NONE);                                                     // forced, whatever the list says
        EXPECT(gDraws[d].draw.mesh.numIndices == draws[d].mesh.numIndices && gDraws[d].draw.numInstances == draws[d].numInstances);
        EXPECT(gIdDraws[d].numIndices == draws[d].mesh.numIndices && gIdDraws[d].numInstances == draws[d].numInstances);
        EXPECT(gIdDraws[d].objID == ids[d].ObjID && gIdDraws[d].meshID == ids[d].MeshID && gIdDraws[d].materialID == ids[d].MaterialID);
    }
    EXPECT(draws[0].cullMode == VQHIP_CULL_BACK);                                                               // the caller's list is not modified
    EXPECT(gDraws[0].material == mats && gDraws[1].material == nullptr && gDraws[2].material == mats + 1);
    EXPECT(gSizeTriangles == 12 * 2 + 2 * 3 && gSizeMasked == 2 * 3 && gSizeDraws == 3 && gIdsSizeDraws == 3);
    EXPECT(gTargets.depth == pass->GetDepth() && gTargets.primitive == pass->GetOwner() && gTargets.layers == 0 && gTargets.pitch == 0 && gTargets.reserved == 0);
    EXPECT(gOwner == pass->GetOwner() && gIds == pass->GetObjectIDs() && gOwnerPitch == 0 && gIdsPitch == 0);
    EXPECT(gAllocs == 5 && gDepthWorkBytes == 1000 + 30 * 10 + 6 * 64 + 3 * 48 && gIdsWorkBytes == 300 + 3 * 32 && gDepthWork != gIdsWork);
    EXPECT(pass->GetDepthWorkBytes() == gDepthWorkBytes && pass->GetIdsWorkBytes() == gIdsWorkBytes);

    pPass->RecordCommands(&p);                                                                                  // the buffers are kept
    EXPECT(gAllocs == 5 && gDepthCalls == 2 && gIdsCalls == 2);
    gDepthStatus = 4321;                                                                                        // a refused depth call: no resolve over a stale owner plane
    pPass->RecordCommands(&p);
    EXPECT(gDepthCalls == 3 && gIdsCalls == 2 && pass->LastStatus() == 4321);
    gDepthStatus = VQHIP_OK; gIdsStatus = 8765;
    pPass->RecordCommands(&p);
    EXPECT(gDepthCalls == 4 && gIdsCalls == 3 && pass->LastStatus() == 8765);
    gIdsStatus = VQHIP_OK;

    std::vector<vqhip::ObjectIDPass::FObjectID> shortIds(ids.begin(), ids.begin() + 2);                         // bad parameter blocks: no call
    p.IDs = &shortIds;
    pPass->RecordCommands(&p);
    EXPECT(gDepthCalls == 4 && pass->LastStatus() == VQHIP_ERR_INVALID_ARG);
    p.IDs = nullptr;
    pPass->RecordCommands(&p);
    EXPECT(gDepthCalls == 4 && pass->LastStatus() == VQHIP_ERR_INVALID_ARG);
    p.IDs = &ids;
    std::vector<int32_t> past = { 0, -1, 2 };
    p.MaterialIndex = &past;
    pPass->RecordCommands(&p);
    EXPECT(gDepthCalls == 4 && pass->LastStatus() == VQHIP_ERR_INVALID_ARG);
    std::vector<int32_t> shortIndex = { 0, -1 };
    p.MaterialIndex = &shortIndex;
    pPass->RecordCommands(&p);
    EXPECT(gDepthCalls == 4 && pass->LastStatus() == VQHIP_ERR_INVALID_ARG);
    p.MaterialIndex = nullptr;                                                                                  // no materials: every draw opaque
    pPass->RecordCommands(&p);
    EXPECT(gDepthCalls == 5 && gIdsCalls == 4 && pass->LastStatus() == VQHIP_OK && gSizeMasked == 0 && gDraws[0].material == nullptr && gDraws[2].material == nullptr);
    p.Draws = nullptr; p.IDs = nullptr;                                                                         // an empty frame: both calls, with no draws (the planes are cleared)
    pPass->RecordCommands(&p);
    EXPECT(gDepthCalls == 6 && gIdsCalls == 5 && pass->LastStatus() == VQHIP_OK && gDraws.empty() && gIdDraws.empty() && gSizeDraws == 0 && gIdsSizeDraws == 0);

    // ReadBackPixel: 16 bytes from [y][x] of the ids plane on the caller's stream, then a wait on it; outside the window (-1, -1, -1, -1) and no copy
    int32_t* plane = const_cast<int32_t*>(pass->GetObjectIDs());
    const size_t at = ((size_t)7 * 40 + 5) * 4;
    plane[at] = 101; plane[at + 1] = -202; plane[at + 2] = 303; plane[at + 3] = 404;
    px = pass->ReadBackPixel(5, 7, &p);
    EXPECT(px.x == 101 && px.y == -202 && px.z == 303 && px.w == 404 && gCopies == 1 && gSyncs == 1 && gCopyBytes == 16 && gCopySrc == plane + at);
    EXPECT(gCopyStream == (void*)&p && gSyncStream == (void*)&p);
    const int bad[][2] = { { -1, 0 }, { 0, -1 }, { 40, 0 }, { 0, 30 }, { 1 << 30, 1 << 30 } };
    for (const auto& c : bad) {
        px = pass->ReadBackPixel(c[0], c[1], &p);
        EXPECT(px.x == -1 && px.y == -1 && px.z == -1 && px.w == -1 && gCopies == 1);
    }
    px = pass->ReadBackPixel(39, 29);
    EXPECT(px.x == 0 && px.w == 0 && gCopies == 2 && gCopySrc == plane + ((size_t)29 * 40 + 39) * 4);
    gCopyResult = hipErrorInvalidValue;
    px = pass->ReadBackPixel(5, 7);
    EXPECT(px.x == -1 && px.w == -1 && gCopies == 3);
    gCopyResult = hipSuccess;

    const int frees = gFrees;
    pPass->OnCreateWindowSizeDependentResources(8, 4, nullptr);                                                 // a resize frees the three planes and allocates them anew
    EXPECT(gFrees == frees + 3 && gAllocs == 8 && gAllocSizes[7] == 8 * 4 * 16);
    px = pass->ReadBackPixel(8, 0);
    EXPECT(px.x == -1);
    return 0;
}

int main() {
    static_assert(std::is_base_of<::IRenderPass, vqhip::ObjectIDPass>::value, "the adaptor derives from the engine's IRenderPass");
    vqhip_ctx* ctx = reinterpret_cast<vqhip_ctx*>(static_cast<uintptr_t>(0x1000));      // never dereferenced: the library calls are the recorders above
    static vqhip_material mats[2];                                                       // 0: opaque; 1: masked with a diffuse map
    std::memset(mats, 0, sizeof(mats));
    mats[1].texDiffuse.reserved = VQHIP_MATERIAL_ALPHA_MASKED; mats[1].data.textureConfig = 1.0f; mats[1].texDiffuse.width = mats[1].texDiffuse.height = 8; mats[1].texDiffuse.mips = 4;
    const int frees0 = gFrees;
    if (int rc = adaptor(ctx, mats)) return rc;
    EXPECT(gFrees - frees0 == gAllocs);                                                  // the destructor releases the planes and both work buffers
    std::printf("object id adaptor OK\n");
    return 0;
}
