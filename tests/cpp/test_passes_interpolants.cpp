// test_passes_interpolants.cpp — drives vqhip::DepthPrePass and vqhip::SceneInterpolantsPass (include/vqhip_passes.hpp) the way VQRenderer would: the main view's
// draw list goes through the Z pre-pass, whose owner planes (Primitive without MSAA, the LayerPrimitive planes with it) go with the same list through the
// interpolant pass, one call per plane. Inputs / outputs are raw files in a directory given on the command line (written / checked by
// tests/test_gpu_scene_interp.py):
//   draws.txt   one line per draw: numVertices strideBytes indexBits numIndices numInstances materialIndex cullMode
//   d<k>_{vertices,indices,wvp,world,normal,prev}.bin
//   -> owner<p>.bin, ip0_<p>.bin, ip1_<p>.bin, ip2_<p>.bin, sv_curr_<p>.bin, sv_prev_<p>.bin for plane p (0 at 1 sample, 0 .. 3 at 4)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "vqhip_passes.hpp"

static std::vector<char> readFile(const std::string& p) {
    FILE* f = fopen(p.c_str(), "rb"); if (!f) { fprintf(stderr, "cannot open %s\n", p.c_str()); exit(2); }
    fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<char> b(n); if (fread(b.data(), 1, n, f) != (size_t)n) exit(2); fclose(f); return b;
}
static void writeDev(const std::string& p, const void* dev, size_t bytes) {
    std::vector<char> h(bytes);
    if (hipMemcpy(h.data(), dev, bytes, hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "copy back failed\n"); exit(3); }
    FILE* f = fopen(p.c_str(), "wb");
    if (!f || fwrite(h.data(), 1, bytes, f) != bytes || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", p.c_str()); exit(2); }
}
static void* upload(const std::vector<char>& h) {
    void* d = nullptr;
    if (hipMalloc(&d, h.size()) != hipSuccess || hipMemcpy(d, h.data(), h.size(), hipMemcpyHostToDevice) != hipSuccess) { fprintf(stderr, "upload failed\n"); exit(3); }
    return d;
}
static void* alloc(size_t bytes) {
    void* d = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess) { fprintf(stderr, "hipMalloc failed\n"); exit(3); }
    return d;
}
#define CHECK(pass) do { if ((pass).LastStatus() != VQHIP_OK) { fprintf(stderr, "%s failed: %d %s\n", #pass, (pass).LastStatus(), vqhip_last_error(ctx)); return 4; } } while (0)

int main(int argc, char** argv) {
    if (argc < 5) { fprintf(stderr, "usage: test_passes_interpolants <dir> <W> <H> <samples>\n"); return 1; }
    const std::string dir = argv[1];
    const int W = atoi(argv[2]), H = atoi(argv[3]), samples = atoi(argv[4]);
    if (W < 1 || H < 1 || (samples != 1 && samples != 4)) { fprintf(stderr, "bad size or sample count\n"); return 1; }
    vqhip_ctx* ctx = nullptr;
    if (vqhip_create(0, &ctx) != VQHIP_OK) { fprintf(stderr, "vqhip_create: %s\n", vqhip_last_error(nullptr)); return 3; }
    hipStream_t stream; (void)hipStreamCreate(&stream);

    // FSceneDrawData::mainViewDrawParams: one list, read by both passes
    std::vector<vqhip_scene_depth_draw> depthDraws;
    std::vector<vqhip_scene_surface_draw> surfaceDraws;
    FILE* f = fopen((dir + "/draws.txt").c_str(), "r");
    if (!f) { fprintf(stderr, "cannot open draws.txt\n"); return 2; }
    unsigned nv, stride, ni, inst; int bits, material, cull;
    while (fscanf(f, "%u %u %d %u %u %d %d", &nv, &stride, &bits, &ni, &inst, &material, &cull) == 7) {
        const std::string d = dir + "/d" + std::to_string(surfaceDraws.size()) + "_";
        vqhip_scene_surface_draw s = {};
        s.mesh.positions = upload(readFile(d + "vertices.bin")); s.mesh.strideBytes = stride; s.mesh.numVertices = nv;
        s.mesh.indices = upload(readFile(d + "indices.bin")); s.mesh.indexBits = bits; s.mesh.numIndices = ni;
        s.matWorldViewProj = (const VQ_matrix*)upload(readFile(d + "wvp.bin")); s.matWorld = (const VQ_matrix*)upload(readFile(d + "world.bin"));
        s.matNormal = (const VQ_matrix*)upload(readFile(d + "normal.bin")); s.matWorldViewProjPrev = (const VQ_matrix*)upload(readFile(d + "prev.bin"));
        s.numInstances = inst; s.materialIndex = material;
        surfaceDraws.push_back(s);
        vqhip_scene_depth_draw z = {};
        z.mesh = s.mesh; z.matWorldViewProj = s.matWorldViewProj; z.numInstances = inst; z.cullMode = cull;
        depthDraws.push_back(z);
    }
    fclose(f);

    // --- RenderDepthPrePass
    const size_t px = (size_t)W * H;
    const int planes = samples == 4 ? 4 : 1;
    vqhip::DepthPrePass zpass(ctx);
    zpass.Initialize();
    zpass.OnCreateWindowSizeDependentResources(W, H);
    vqhip::DepthPrePass::FDrawParameters zp;
    zp.Stream = stream; zp.Draws = &depthDraws; zp.bMSAA = samples == 4;
    zp.SceneDepth = (float*)alloc(px * 4 * samples);
    const uint32_t* owner[4] = {};
    if (samples == 4) {
        zp.NumLayers = 4;
        for (int k = 0; k < 4; ++k) { zp.Coverage[k] = (uint8_t*)alloc(px); zp.LayerPrimitive[k] = (uint32_t*)alloc(px * 4); owner[k] = zp.LayerPrimitive[k]; }
    } else {
        zp.Primitive = (uint32_t*)alloc(px * 4); owner[0] = zp.Primitive;
    }
    zpass.RecordCommands(&zp);
    CHECK(zpass);

    // --- RenderSceneColor's vertex stage and interpolation: one call per owner plane
    vqhip::SceneInterpolantsPass ipass(ctx);
    ipass.Initialize();
    ipass.OnCreateWindowSizeDependentResources(W, H);
    void* out[4][5];
    for (int p = 0; p < planes; ++p) {
        for (int k = 0; k < 5; ++k) out[p][k] = alloc(px * 16);
        vqhip::SceneInterpolantsPass::FDrawParameters ip;
        ip.Stream = stream; ip.Draws = &surfaceDraws; ip.Owner = owner[p];
        ip.Ip0 = out[p][0]; ip.Ip1 = out[p][1]; ip.Ip2 = out[p][2]; ip.SvPositionCurr = out[p][3]; ip.SvPositionPrev = out[p][4];
        ipass.RecordCommands(&ip);
        CHECK(ipass);
    }
    if (hipStreamSynchronize(stream) != hipSuccess) { fprintf(stderr, "stream sync failed\n"); return 3; }
    static const char* names[5] = { "ip0", "ip1", "ip2", "sv_curr", "sv_prev" };
    for (int p = 0; p < planes; ++p) {
        writeDev(dir + "/owner" + std::to_string(p) + ".bin", owner[p], px * 4);
        for (int k = 0; k < 5; ++k) writeDev(dir + "/" + names[k] + "_" + std::to_string(p) + ".bin", out[p][k], px * 16);
    }
    if (ipass.GetWorkBytes() < vqhip_scene_interpolants_work_bytes((int)surfaceDraws.size())) { fprintf(stderr, "work buffer too small\n"); return 5; }
    vqhip_destroy(ctx);
    printf("scene interpolants adaptor OK\n");
    return 0;
}
