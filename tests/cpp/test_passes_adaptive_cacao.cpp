// test_passes_adaptive_cacao.cpp — vqhip::AdaptiveAmbientOcclusionPass (include/vqhip_passes.hpp) against the stand-in of the engine's RenderPass.h, host-only:
// the adaptor sizes its work buffer with vqhip_adaptive_cacao_work_bytes, forwards every field of its FDrawParameters to vqhip_adaptive_cacao with the engine's
// format and tight pitches, keeps the library's status, and refuses a NULL parameter block (or a pass without window-size resources) without calling the library.
// vqhip_adaptive_cacao, its size function and the two allocator calls are defined HERE (the executable's definitions are the ones the adaptor binds to): nothing
// touches a device. Built by tests/test_cacao_adaptive_cpu.py with the command line tests/cpp/Makefile uses for test_passes_engine.
#ifndef VQHIP_ENGINE_RENDERPASS_H
#define VQHIP_ENGINE_RENDERPASS_H "mock_engine/RenderPass.h"
#endif
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include "vqhip_passes.hpp"

struct Seen {
    vqhip_ctx* ctx; void* stream; const float* depth; size_t depthPitch; const void* normals; int fmt; size_t normalPitch; VQ_CacaoConstants shared, perPass[4];
    int blur; void* work; size_t workBytes; uint8_t* ao; size_t aoPitch; int width, height;
};
static Seen gSeen;
static int gCalls = 0, gSizeCalls = 0, gAllocs = 0, gFrees = 0;
static size_t gAllocBytes = 0;

extern "C" size_t vqhip_adaptive_cacao_work_bytes(int width, int height) { ++gSizeCalls; return (size_t)width * 1000 + (size_t)height; }
extern "C" int vqhip_adaptive_cacao(vqhip_ctx* ctx, void* stream, const float* depth, size_t depthPitchBytes, const void* normals, int normalFmt, size_t normalPitchBytes,
        const VQ_CacaoConstants* shared, const VQ_CacaoConstants perPass[4], int blurPassCount, void* work, size_t workBytes, uint8_t* ao, size_t aoPitchBytes,
        int width, int height) {
    ++gCalls;
    gSeen = Seen{ ctx, stream, depth, depthPitchBytes, normals, normalFmt, normalPitchBytes, *shared, { perPass[0], perPass[1], perPass[2], perPass[3] },
                  blurPassCount, work, workBytes, ao, aoPitchBytes, width, height };
    return 4321;
}
extern "C" hipError_t hipMalloc(void** p, size_t bytes) { ++gAllocs; gAllocBytes = bytes; *p = std::malloc(bytes); return *p ? hipSuccess : hipErrorOutOfMemory; }
extern "C" hipError_t hipFree(void* p) { ++gFrees; std::free(p); return hipSuccess; }

#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
    static_assert(std::is_base_of<::IRenderPass, vqhip::AdaptiveAmbientOcclusionPass>::value, "the adaptor derives from the engine's IRenderPass");
    static_assert(std::is_same<vqhip::AdaptiveAmbientOcclusionPass::FDrawParameters, vqhip::AmbientOcclusionPass::FDrawParameters>::value, "one parameter block for both levels");
    vqhip_ctx* ctx = reinterpret_cast<vqhip_ctx*>(static_cast<uintptr_t>(0x1000));      // never dereferenced: the library call is the recorder above
    {
        std::shared_ptr<::IRenderPass> pPass = std::make_shared<vqhip::AdaptiveAmbientOcclusionPass>(ctx);
        vqhip::AdaptiveAmbientOcclusionPass* pass = static_cast<vqhip::AdaptiveAmbientOcclusionPass*>(pPass.get());
        EXPECT(pPass->Initialize());
        EXPECT(!std::make_shared<vqhip::AdaptiveAmbientOcclusionPass>(nullptr)->Initialize());
        static unsigned char pool[8];
        auto at = [&](int i) { return static_cast<void*>(pool + i); };
        vqhip::AdaptiveAmbientOcclusionPass::FDrawParameters p;
        EXPECT(p.BlurPassCount == 2);                                                    // FFX_CACAO_DEFAULT_SETTINGS.blurPassCount
        p.Stream = at(0); p.TexSceneDepthResolve = static_cast<const float*>(at(1)); p.TexSceneNormals = at(2); p.TexAmbientOcclusion = static_cast<uint8_t*>(at(3));
        p.BlurPassCount = 3;
        p.Constants.AdaptiveSampleCountLimit = 0.45f; p.Constants.LoadCounterAvgDiv = 0.125f; p.Constants.ImportanceMapDimensions[0] = 160; p.Constants.ImportanceMapDimensions[1] = 90;
        for (int i = 0; i < 4; ++i) { p.PerPassConstants[i] = p.Constants; p.PerPassConstants[i].PassIndex = i; }
        pPass->RecordCommands(&p);                                                       // no window-size resources yet: refused, the library is not called
        EXPECT(pass->LastStatus() == VQHIP_ERR_INVALID_ARG && gCalls == 0 && pass->GetWorkBuffer() == nullptr);
        pPass->OnCreateWindowSizeDependentResources(640, 360);
        EXPECT(gSizeCalls == 1 && gAllocs == 1 && gAllocBytes == 640360 && pass->GetWorkBuffer() != nullptr);
        pPass->RecordCommands(nullptr);                                                  // the NULL refusal
        EXPECT(pass->LastStatus() == VQHIP_ERR_INVALID_ARG && gCalls == 0);
        pPass->RecordCommands(&p);
        EXPECT(gCalls == 1 && pass->LastStatus() == 4321);                               // the library's status is kept
        EXPECT(gSeen.ctx == ctx && gSeen.stream == at(0) && gSeen.depth == at(1) && gSeen.normals == at(2) && gSeen.ao == at(3));
        EXPECT(gSeen.depthPitch == 640 * 4 && gSeen.normalPitch == 640 * 4 && gSeen.aoPitch == 640 && gSeen.fmt == VQHIP_FMT_R10G10B10A2_UNORM);
        EXPECT(gSeen.width == 640 && gSeen.height == 360 && gSeen.blur == 3);
        EXPECT(gSeen.work == pass->GetWorkBuffer() && gSeen.workBytes == 640360);
        EXPECT(std::memcmp(&gSeen.shared, &p.Constants, sizeof(VQ_CacaoConstants)) == 0);
        for (int i = 0; i < 4; ++i) EXPECT(std::memcmp(&gSeen.perPass[i], &p.PerPassConstants[i], sizeof(VQ_CacaoConstants)) == 0 && gSeen.perPass[i].PassIndex == i);
        pPass->OnCreateWindowSizeDependentResources(320, 200);                           // a resize frees the old buffer and sizes a new one
        EXPECT(gFrees == 1 && gAllocs == 2 && gAllocBytes == 320200);
    }
    EXPECT(gFrees == 2);                                                                 // the destructor releases the buffer
    std::printf("adaptive cacao adaptor OK\n");
    return 0;
}
