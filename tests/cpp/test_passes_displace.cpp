// test_passes_displace.cpp — vqhip::HeightmapDisplacementPass (include/vqhip_passes.hpp; docs/DESIGN_DETAILS.md §7.22) against the stand-in of the engine's
// RenderPass.h, host-only: the adaptor turns a list of (mesh LOD, material) pairs into ONE vqhip_displace_meshes call — one job per stream asked for, the full-stride
// job before the 12-byte one —, owns nothing, keeps the library's status and refuses a missing parameter block without calling.
// The entry point is defined HERE (the executable's definition is the one the adaptor binds to): nothing touches a device. Built by tests/test_displace_cpu.py with
// the command line tests/test_masked_depth_cpu.py uses, and once more with the host sanitizers.
#ifndef VQHIP_ENGINE_RENDERPASS_H
#define VQHIP_ENGINE_RENDERPASS_H "mock_engine/RenderPass.h"
#endif
#include <cstdio>
#include <cstring>
#include <memory>
#include "vqhip_passes.hpp"

static std::vector<vqhip_displace_job> gJobs;
static int gCalls = 0, gNumJobs = -1, gStatus = VQHIP_OK;
static bool gNullJobs = false;
static vqhip_ctx* gCtx = nullptr; static void* gStream = nullptr;

extern "C" int vqhip_displace_meshes(vqhip_ctx* ctx, void* stream, const vqhip_displace_job* jobs, int numJobs) {
    ++gCalls; gCtx = ctx; gStream = stream; gNumJobs = numJobs; gNullJobs = jobs == nullptr;
    gJobs.assign(jobs, jobs + (jobs ? numJobs : 0));
    return gStatus;
}

#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
    vqhip_ctx* ctx = (vqhip_ctx*)0x1000;
    std::shared_ptr<::IRenderPass> pPass = std::make_shared<vqhip::HeightmapDisplacementPass>(ctx);
    vqhip::HeightmapDisplacementPass* pass = static_cast<vqhip::HeightmapDisplacementPass*>(pPass.get());
    EXPECT(pPass->Initialize());
    pPass->OnCreateWindowSizeDependentResources(640, 360);                      // owns nothing: no effect
    char terrain[44 * 9], prop[48 * 5], fullA[44 * 9], posA[12 * 9], posB[12 * 5], texels[64];
    std::vector<vqhip::HeightmapDisplacementPass::FMesh> meshes(3);
    meshes[0].Vertices = terrain; meshes[0].NumVertices = 9; meshes[0].Heightmap = { texels, 4, 4, 1, 0 };
    meshes[0].uvScaleOffset = { 2.0f, 3.0f, 0.25f, -0.5f }; meshes[0].Displacement = 100.0f; meshes[0].OutFull = fullA; meshes[0].OutPositions = posA;
    meshes[1].Vertices = prop; meshes[1].StrideBytes = 48; meshes[1].NumVertices = 5; meshes[1].Displacement = -1.5f; meshes[1].OutPositions = posB;   // null SRV
    meshes[2].Vertices = prop; meshes[2].StrideBytes = 48; meshes[2].NumVertices = 5;                                                                   // no stream asked for
    vqhip::HeightmapDisplacementPass::FDrawParameters params;
    params.Stream = (void*)0x2000; params.Meshes = &meshes;
    pPass->RecordCommands(&params);
    EXPECT(gCalls == 1 && gCtx == ctx && gStream == (void*)0x2000 && gNumJobs == 3 && pass->GetNumJobs() == 3 && pass->LastStatus() == VQHIP_OK);
    const vqhip_displace_job& a = gJobs[0]; const vqhip_displace_job& b = gJobs[1]; const vqhip_displace_job& c = gJobs[2];
    EXPECT(a.vertices == terrain && a.strideBytes == 44 && a.numVertices == 9 && a.out == fullA && a.outStrideBytes == 44 && a.reserved == 0);
    EXPECT(a.heightmap.texels == texels && a.heightmap.width == 4 && a.heightmap.height == 4 && a.heightmap.mips == 1);
    EXPECT(a.uvScaleOffset.x == 2.0f && a.uvScaleOffset.y == 3.0f && a.uvScaleOffset.z == 0.25f && a.uvScaleOffset.w == -0.5f && a.displacement == 100.0f);
    EXPECT(b.vertices == terrain && b.out == posA && b.outStrideBytes == 12 && b.strideBytes == 44 && b.displacement == 100.0f && b.heightmap.texels == texels);
    EXPECT(c.vertices == prop && c.strideBytes == 48 && c.numVertices == 5 && c.out == posB && c.outStrideBytes == 12 && c.heightmap.texels == nullptr && c.displacement == -1.5f);
    EXPECT(c.uvScaleOffset.x == 1.0f && c.uvScaleOffset.y == 1.0f && c.uvScaleOffset.z == 0.0f && c.uvScaleOffset.w == 0.0f && c.reserved == 0);
    // the library's status is the pass's
    gStatus = VQHIP_ERR_UNSUPPORTED;
    pPass->RecordCommands(&params);
    EXPECT(gCalls == 2 && pass->LastStatus() == VQHIP_ERR_UNSUPPORTED);
    gStatus = VQHIP_OK;
    // nothing to do is a call with no jobs (VQHIP_OK in the library); a missing parameter block is refused without calling
    std::vector<vqhip::HeightmapDisplacementPass::FMesh> none;
    params.Meshes = &none;
    pPass->RecordCommands(&params);
    EXPECT(gCalls == 3 && gNumJobs == 0 && gNullJobs && pass->LastStatus() == VQHIP_OK);
    params.Meshes = nullptr;
    pPass->RecordCommands(&params);
    EXPECT(gCalls == 4 && gNumJobs == 0 && gNullJobs && pass->GetNumJobs() == 0);
    pPass->RecordCommands(nullptr);
    EXPECT(gCalls == 4 && pass->LastStatus() == VQHIP_ERR_INVALID_ARG);
    pPass->OnDestroyWindowSizeDependentResources();
    pPass->Destroy();
    std::printf("heightmap displacement adaptor OK\n");
    return 0;
}
