// test_passes_quad.cpp — vqhip::QuadInterpolantsPass and vqhip::QuadLitDrawPass (include/vqhip_passes.hpp; docs/DESIGN_DETAILS.md §7.20) against the stand-in of the
// engine's RenderPass.h, host-only: the resolve adaptor turns SceneInterpolantsPass's inputs and one more plane into a vqhip_scene_quad_interpolants call, owns the
// work buffer and remembers the quad-uv plane of a successful call; the lit-draw adaptor takes that plane from it and calls one of the three _quad producers.
// The entry points, the size function and the two allocator calls are defined HERE (the executable's definitions are the ones the adaptors bind to): nothing
// touches a device. Built by tests/test_quad_interp_cpu.py with the command line tests/test_masked_depth_cpu.py uses.
#ifndef VQHIP_ENGINE_RENDERPASS_H
#define VQHIP_ENGINE_RENDERPASS_H "mock_engine/RenderPass.h"
#endif
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include "vqhip_passes.hpp"

static vqhip_scene_quad_targets gTargets;
static std::vector<vqhip_scene_surface_draw> gDraws;
static int gWidth = 0, gHeight = 0, gResolveCalls = 0, gAllocs = 0, gFrees = 0, gSizeDraws = 0, gOwnerPitch = 0, gResolveStatus = VQHIP_OK;
static vqhip_ctx* gCtx = nullptr; static void* gStream = nullptr; static void* gWork = nullptr; static size_t gWorkBytes = 0, gAllocBytes = 0;
static const uint32_t* gOwner = nullptr;
static int gGbufferCalls = 0, gForwardCalls = 0, gNormalsCalls = 0, gQuadPitch = 0, gOutPitch = 0, gOutFmt = 0, gNumMaterials = 0;
static const void* gQuadUV = nullptr; static const vqhip_interpolants* gIn = nullptr; static const vqhip_gbuffer* gGbOut = nullptr; static void* gOut = nullptr;
static const vqhip_psmain_targets* gMrt = nullptr; static float gAmbient = 0.0f; static const vqhip_ssao* gSsao = nullptr;

extern "C" size_t vqhip_scene_interpolants_work_bytes(int numDraws) { gSizeDraws = numDraws; return numDraws < 0 ? 0 : 500 + (size_t)numDraws * 80; }
extern "C" int vqhip_scene_quad_interpolants(vqhip_ctx* ctx, void* stream, const vqhip_scene_surface_draw* draws, int numDraws, int width, int height,
                                             const uint32_t* owner, int owner_pitch_px, const vqhip_scene_quad_targets* out, void* work, size_t workBytes) {
    ++gResolveCalls; gCtx = ctx; gStream = stream; gDraws.assign(draws, draws + numDraws); gWidth = width; gHeight = height; gOwner = owner; gOwnerPitch = owner_pitch_px;
    gTargets = *out; gWork = work; gWorkBytes = workBytes;
    return gResolveStatus;
}
extern "C" int vqhip_gbuffer_from_materials_quad(vqhip_ctx* ctx, void* stream, const vqhip_interpolants* in, const vqhip_material*, int numMaterials, float ambient,
                                                 const vqhip_ssao* ssao, const vqhip_gbuffer* out, const void* quadUV, int quad_pitch_px) {
    ++gGbufferCalls; gCtx = ctx; gStream = stream; gIn = in; gNumMaterials = numMaterials; gAmbient = ambient; gSsao = ssao; gGbOut = out; gQuadUV = quadUV; gQuadPitch = quad_pitch_px;
    return 111;
}
extern "C" int vqhip_forward_lighting_from_materials_quad(vqhip_ctx* ctx, void* stream, const vqhip_interpolants* in, const vqhip_material*, int numMaterials,
        const vqhip_ssao* ssao, const VQ_PerFrameData*, const VQ_PerViewLightingData*, const VQ_PointLight*, int, const vqhip_envmap*, const vqhip_shadowmaps*,
        void* out, int out_row_pitch_px, vqhip_format outFmt, const vqhip_psmain_targets* targets, const void* quadUV, int quad_pitch_px) {
    ++gForwardCalls; gCtx = ctx; gStream = stream; gIn = in; gNumMaterials = numMaterials; gSsao = ssao; gOut = out; gOutPitch = out_row_pitch_px; gOutFmt = outFmt; gMrt = targets;
    gQuadUV = quadUV; gQuadPitch = quad_pitch_px;
    return 222;
}
extern "C" int vqhip_scene_normals_from_materials_quad(vqhip_ctx* ctx, void* stream, const vqhip_interpolants* in, const vqhip_material*, int numMaterials,
                                                       void* out, vqhip_format outFmt, int out_row_pitch_px, const void* quadUV, int quad_pitch_px) {
    ++gNormalsCalls; gCtx = ctx; gStream = stream; gIn = in; gNumMaterials = numMaterials; gOut = out; gOutFmt = outFmt; gOutPitch = out_row_pitch_px; gQuadUV = quadUV; gQuadPitch = quad_pitch_px;
    return 333;
}
extern "C" hipError_t hipMalloc(void** p, size_t bytes) { ++gAllocs; gAllocBytes = bytes; *p = std::malloc(bytes); return *p ? hipSuccess : hipErrorOutOfMemory; }
extern "C" hipError_t hipFree(void* p) { ++gFrees; std::free(p); return hipSuccess; }

#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static int adaptors(vqhip_ctx* ctx) {
    std::shared_ptr<::IRenderPass> pResolve = std::make_shared<vqhip::QuadInterpolantsPass>(ctx);
    vqhip::QuadInterpolantsPass* resolve = static_cast<vqhip::QuadInterpolantsPass*>(pResolve.get());
    EXPECT(pResolve->Initialize());
    EXPECT(!std::make_shared<vqhip::QuadInterpolantsPass>(nullptr)->Initialize());
    pResolve->RecordCommands(nullptr);
    EXPECT(resolve->LastStatus() == VQHIP_ERR_INVALID_ARG && gResolveCalls == 0 && resolve->GetQuadUV() == nullptr);

    static float ip0[4], ip1[4], ip2[4], svc[4], svp[4], quad[4]; static uint32_t owner[4];                      // addresses only
    std::vector<vqhip_scene_surface_draw> draws(3);
    std::memset(draws.data(), 0, draws.size() * sizeof(draws[0]));
    draws[1].materialIndex = 7; draws[2].numInstances = 5;
    vqhip::QuadInterpolantsPass::FDrawParameters p;
    EXPECT(p.QuadUV == nullptr && p.QuadPitch == 0 && p.Owner == nullptr);
    p.Stream = &p; p.Draws = &draws; p.Owner = owner; p.OwnerPitch = 2048; p.Ip0 = ip0; p.Ip1 = ip1; p.Ip2 = ip2; p.SvPositionCurr = svc; p.SvPositionPrev = svp;
    p.QuadUV = quad;
    pResolve->OnCreateWindowSizeDependentResources(1920, 1080, nullptr);
    gResolveStatus = 4321;                                                                                       // a refusal: the status is kept, no plane is handed on
    pResolve->RecordCommands(&p);
    EXPECT(gResolveCalls == 1 && resolve->LastStatus() == 4321 && resolve->GetQuadUV() == nullptr);
    gResolveStatus = VQHIP_OK;
    pResolve->RecordCommands(&p);
    EXPECT(gResolveCalls == 2 && resolve->LastStatus() == VQHIP_OK && resolve->GetQuadUV() == quad && resolve->GetQuadPitch() == 1920);
    EXPECT(gCtx == ctx && gStream == &p && gDraws.size() == 3 && gWidth == 1920 && gHeight == 1080 && gOwner == owner && gOwnerPitch == 2048);
    EXPECT(std::memcmp(gDraws.data(), draws.data(), 3 * sizeof(draws[0])) == 0);
    EXPECT(gTargets.planes.ip0 == ip0 && gTargets.planes.ip1 == ip1 && gTargets.planes.ip2 == ip2 && gTargets.planes.svPositionCurr == svc &&
           gTargets.planes.svPositionPrev == svp && gTargets.planes.pitch == 0 && gTargets.quadUV == quad && gTargets.quad_pitch == 0 && gTargets.pad_ == 0);
    EXPECT(gSizeDraws == 3 && gAllocs == 1 && gAllocBytes == 500 + 3 * 80 && gWork == resolve->GetWorkBuffer() && gWorkBytes == gAllocBytes && gFrees == 0);
    p.QuadPitch = 2000;
    pResolve->RecordCommands(&p);                                                                                // the same frame again: the buffer is kept
    EXPECT(gResolveCalls == 3 && gAllocs == 1 && gTargets.quad_pitch == 2000 && resolve->GetQuadPitch() == 2000);

    // the lit draw takes the plane from the resolve
    std::shared_ptr<::IRenderPass> pLit = std::make_shared<vqhip::QuadLitDrawPass>(ctx);
    vqhip::QuadLitDrawPass* lit = static_cast<vqhip::QuadLitDrawPass*>(pLit.get());
    EXPECT(pLit->Initialize());
    pLit->OnCreateWindowSizeDependentResources(1920, 1080, nullptr);
    EXPECT(gAllocs == 2 && gAllocBytes == (size_t)1920 * 1080 * 8 && lit->GetSceneColor() != nullptr);
    pLit->RecordCommands(nullptr);
    EXPECT(lit->LastStatus() == VQHIP_ERR_INVALID_ARG);
    static vqhip_interpolants in; static vqhip_material mats[2]; static VQ_PerFrameData pf; static VQ_PerViewLightingData pv; static vqhip_ssao ssao;
    static vqhip_psmain_targets mrt; static vqhip_gbuffer gb; static uint32_t normals[4];
    pf.fAmbientLightingFactor = 0.25f;
    vqhip::QuadLitDrawPass::FDrawParameters q;
    q.Stream = &q; q.pInterpolants = &in; q.pMaterials = mats; q.NumMaterials = 2; q.pPerFrame = &pf; q.pPerView = &pv; q.pScreenSpaceAO = &ssao; q.pTargets = &mrt;
    pLit->RecordCommands(&q);                                                                                    // no resolve named
    EXPECT(lit->LastStatus() == VQHIP_ERR_INVALID_ARG && gForwardCalls == 0);
    q.pQuadInterpolants = resolve;
    pLit->RecordCommands(&q);
    EXPECT(gForwardCalls == 1 && lit->LastStatus() == 222 && gStream == &q && gIn == &in && gNumMaterials == 2 && gSsao == &ssao && gMrt == &mrt);
    EXPECT(gOut == lit->GetSceneColor() && gOutPitch == 1920 && gOutFmt == VQHIP_FMT_RGBA16F && gQuadUV == quad && gQuadPitch == 2000);
    q.pGBufferOut = &gb;                                                                                         // one 4x layer
    pLit->RecordCommands(&q);
    EXPECT(gGbufferCalls == 1 && gForwardCalls == 1 && lit->LastStatus() == 111 && gGbOut == &gb && gAmbient == 0.25f && gQuadUV == quad && gQuadPitch == 2000);
    q.pSceneNormalsOut = normals;                                                                                // both: refused without a call
    pLit->RecordCommands(&q);
    EXPECT(lit->LastStatus() == VQHIP_ERR_INVALID_ARG && gNormalsCalls == 0 && gGbufferCalls == 1);
    q.pGBufferOut = nullptr; q.pPerFrame = nullptr;                                                              // the pre-pass target needs no lighting constants
    pLit->RecordCommands(&q);
    EXPECT(gNormalsCalls == 1 && lit->LastStatus() == 333 && gOut == normals && gOutFmt == VQHIP_FMT_R10G10B10A2_UNORM && gOutPitch == 0 && gQuadUV == quad);
    q.pSceneNormalsOut = nullptr;
    pLit->RecordCommands(&q);                                                                                    // the lit frame does
    EXPECT(lit->LastStatus() == VQHIP_ERR_INVALID_ARG && gForwardCalls == 1);
    q.pPerFrame = &pf;
    gResolveStatus = 9;                                                                                          // a resolve that failed hands nothing on
    pResolve->RecordCommands(&p);
    pLit->RecordCommands(&q);
    EXPECT(resolve->GetQuadUV() == nullptr && lit->LastStatus() == VQHIP_ERR_INVALID_ARG && gForwardCalls == 1);
    gResolveStatus = VQHIP_OK;
    std::vector<vqhip_scene_surface_draw> more(40);                                                              // a frame that needs more: freed and sized anew
    std::memset(more.data(), 0, more.size() * sizeof(more[0]));
    p.Draws = &more;
    pResolve->RecordCommands(&p);
    EXPECT(gAllocs == 3 && gFrees == 1 && gAllocBytes == 500 + 40 * 80 && gWorkBytes == gAllocBytes);
    p.Draws = nullptr;                                                                                           // nothing to draw: the call still writes the no-owner records
    pResolve->RecordCommands(&p);
    EXPECT(gDraws.empty() && gSizeDraws == 0 && resolve->LastStatus() == VQHIP_OK && gAllocs == 3);
    return 0;
}

int main() {
    static_assert(std::is_base_of<::IRenderPass, vqhip::QuadInterpolantsPass>::value && std::is_base_of<::IRenderPass, vqhip::QuadLitDrawPass>::value,
                  "the adaptors derive from the engine's IRenderPass");
    static_assert(std::is_base_of<vqhip::SceneInterpolantsPass::FDrawParameters, vqhip::QuadInterpolantsPass::FDrawParameters>::value, "the inputs of SceneInterpolantsPass");
    vqhip_ctx* ctx = reinterpret_cast<vqhip_ctx*>(static_cast<uintptr_t>(0x1000));      // never dereferenced: the library calls are the recorders above
    const int frees0 = gFrees;
    if (int rc = adaptors(ctx)) return rc;
    EXPECT(gFrees == frees0 + 3);                                                        // the destructors release the work buffer (twice sized) and the scene colour
    std::printf("quad adaptors OK\n");
    return 0;
}
