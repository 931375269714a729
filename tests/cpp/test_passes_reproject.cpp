// test_passes_reproject.cpp — vqhip::HipSSRReprojectPass (include/vqhip_passes.hpp) against the stand-in of the engine's RenderPass.h, host-only: the adaptor
// forwards every plane of its FDrawParameters into the field of vqhip_ssr_reproject_surfaces that has its role (ScreenSpaceReflections.cpp:1177-1198), with the
// engine's formats and tight pitches, and refuses a NULL parameter block without calling the library. vqhip_ssr_reproject is defined HERE (the executable's
// definition is the one the adaptor binds to) and records what it was given. Built by tests/test_ssr_reproject_cpu.py with the command line tests/cpp/Makefile
// uses for test_passes_engine.
#ifndef VQHIP_ENGINE_RENDERPASS_H
#define VQHIP_ENGINE_RENDERPASS_H "mock_engine/RenderPass.h"
#endif
#include <cstdio>
#include <cstring>
#include <memory>
#include "vqhip_passes.hpp"

static int gCalls = 0;
static vqhip_ssr_reproject_surfaces gSeen;
static vqhip_ctx* gCtx = nullptr;
static void* gStream = nullptr;
static VQ_SSSRConstants gCb;

extern "C" int vqhip_ssr_reproject(vqhip_ctx* ctx, void* stream, const vqhip_ssr_reproject_surfaces* io, const VQ_SSSRConstants* cb) {
    ++gCalls; gCtx = ctx; gStream = stream; gSeen = *io; gCb = *cb;
    return 1234;
}

#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
    static_assert(std::is_base_of<::IRenderPass, vqhip::HipSSRReprojectPass>::value, "the adaptor derives from the engine's IRenderPass");
    vqhip_ctx* ctx = reinterpret_cast<vqhip_ctx*>(static_cast<uintptr_t>(0x1000));      // never dereferenced: the library call is the recorder above
    std::shared_ptr<::IRenderPass> pPass = std::make_shared<vqhip::HipSSRReprojectPass>(ctx);
    vqhip::HipSSRReprojectPass* pass = static_cast<vqhip::HipSSRReprojectPass*>(pPass.get());
    EXPECT(pPass->Initialize());
    EXPECT(!std::make_shared<vqhip::HipSSRReprojectPass>(nullptr)->Initialize());
    EXPECT(pPass->CollectPSOCreationParameters().empty());
    pPass->RecordCommands(nullptr);                                                      // the NULL refusal: reported, the library is not called
    EXPECT(pass->LastStatus() == VQHIP_ERR_INVALID_ARG && gCalls == 0);
    static unsigned char pool[32];                                                       // 19 distinct addresses
    auto at = [&](int i) { return static_cast<void*>(pool + i); };
    vqhip::HipSSRReprojectPass::FDrawParameters p;
    p.Stream = at(0);
    p.ffxCBuffer.bufferDimensions[0] = 640; p.ffxCBuffer.bufferDimensions[1] = 360; p.ffxCBuffer.roughnessThreshold = 0.25f;
    p.TexDenoiserTileList = static_cast<const uint32_t*>(at(1)); p.TexRayCounter = static_cast<const uint32_t*>(at(2));
    p.TexDepthHierarchy = static_cast<const float*>(at(3)); p.TexExtractedRoughness = static_cast<const uint8_t*>(at(4)); p.TexNormals = at(5);
    p.TexDepthHistory = static_cast<const float*>(at(6)); p.TexRoughnessHistory = static_cast<const uint8_t*>(at(7)); p.TexNormalsHistory = at(8);
    p.TexRadianceIn = at(9); p.TexRadianceHistory = at(10); p.TexMotionVectors = at(11); p.TexVarianceHistory = at(12); p.TexSampleCountHistory = at(13);
    p.TexReprojectedRadiance = at(14); p.TexAvgRadianceOut = at(15); p.TexVarianceOut = at(16); p.TexSampleCountOut = at(17);
    pPass->RecordCommands(&p);
    EXPECT(gCalls == 1 && pass->LastStatus() == 1234);                                   // the library's status is kept
    EXPECT(gCtx == ctx && gStream == at(0));
    EXPECT(gCb.bufferDimensions[0] == 640 && gCb.bufferDimensions[1] == 360 && gCb.roughnessThreshold == 0.25f);
    EXPECT(gSeen.tile_list == at(1) && gSeen.counters == at(2));
    EXPECT(gSeen.depth == at(3) && gSeen.roughness == at(4) && gSeen.normals == at(5));
    EXPECT(gSeen.depth_history == at(6) && gSeen.roughness_history == at(7) && gSeen.normal_history == at(8));
    EXPECT(gSeen.radiance == at(9) && gSeen.radiance_history == at(10) && gSeen.motion_vectors == at(11));
    EXPECT(gSeen.variance_history == at(12) && gSeen.sample_count_history == at(13));
    EXPECT(gSeen.out_reprojected == at(14) && gSeen.out_average == at(15) && gSeen.out_variance == at(16) && gSeen.out_sample_count == at(17));
    EXPECT(gSeen.normals_fmt == VQHIP_FMT_R10G10B10A2_UNORM && gSeen.normal_history_fmt == VQHIP_FMT_R10G10B10A2_UNORM);
    EXPECT(gSeen.radiance_fmt == VQHIP_FMT_RGBA16F && gSeen.radiance_history_fmt == VQHIP_FMT_RGBA16F && gSeen.out_reprojected_fmt == VQHIP_FMT_RGBA16F);
    EXPECT(gSeen.motion_fmt == VQHIP_FMT_RG16F && gSeen.out_average_fmt == VQHIP_FMT_R11G11B10_FLOAT);
    const int32_t* pitches = &gSeen.depth_pitch_px;                                      // fourteen pitches, all 0 = tight
    for (int i = 0; i < 14; ++i) EXPECT(pitches[i] == 0);
    std::printf("reproject adaptor OK\n");
    return 0;
}
