// test_passes_lines.cpp — vqhip::WireframePass and vqhip::VertexAxesPass (include/vqhip_passes.hpp; docs/DESIGN_DETAILS.md §7.24) against the stand-in of the
// engine's RenderPass.h, host-only: the adaptors turn the bounding boxes of RenderBoundingBoxes, the wire half of RenderLightBounds and the point lists of
// RenderDebugVertexAxes into vqhip_line_draws calls — into the bounding-volumes target when reflections are on, into scene colour when they are off —, count
// the lines for the work size, own the work buffer, keep the library's status and refuse bad parameter blocks without calling.
// The entry point, its size function and the two allocator calls are defined HERE (the executable's definitions are the ones the adaptor binds to): nothing
// touches a device. Built by tests/test_line_draws_cpu.py with the command line tests/test_unlit_draws_cpu.py uses.
#ifndef VQHIP_ENGINE_RENDERPASS_H
#define VQHIP_ENGINE_RENDERPASS_H "mock_engine/RenderPass.h"
#endif
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include "vqhip_passes.hpp"

static vqhip_unlit_targets gTargets;
static std::vector<vqhip_line_draw> gDraws;
static int gWidth = 0, gHeight = 0, gCalls = 0, gAllocs = 0, gFrees = 0, gStatus = VQHIP_OK;
static vqhip_ctx* gCtx = nullptr; static void* gStream = nullptr; static void* gWork = nullptr; static size_t gWorkBytes = 0, gAllocBytes = 0;
static uint64_t gSizeLines = 0;
static bool gDrawsNull = false;

extern "C" size_t vqhip_line_draws_work_bytes(uint64_t lines) { gSizeLines = lines; return lines >= 10000000 ? 0 : 256 + (size_t)lines * 40; }
extern "C" int vqhip_line_draws(vqhip_ctx* ctx, void* stream, const vqhip_line_draw* draws, int numDraws, int width, int height, const vqhip_unlit_targets* out,
                                void* work, size_t workBytes) {
    ++gCalls; gCtx = ctx; gStream = stream; gDrawsNull = draws == nullptr; gDraws.assign(draws, draws + numDraws); gWidth = width; gHeight = height;
    gTargets = *out; gWork = work; gWorkBytes = workBytes;
    return gStatus;
}
extern "C" hipError_t hipMalloc(void** p, size_t bytes) { ++gAllocs; gAllocBytes = bytes; *p = std::malloc(bytes); return *p ? hipSuccess : hipErrorOutOfMemory; }
extern "C" hipError_t hipFree(void* p) { ++gFrees; std::free(p); return hipSuccess; }

#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static int wireframe(vqhip_ctx* ctx) {
    using Pass = vqhip::WireframePass;
    std::shared_ptr<::IRenderPass> pPass = std::make_shared<Pass>(ctx);
    Pass* pass = static_cast<Pass*>(pPass.get());
    EXPECT(pPass->Initialize());
    EXPECT(!std::make_shared<Pass>(nullptr)->Initialize());
    pPass->RecordCommands(nullptr);
    EXPECT(pass->LastStatus() == VQHIP_ERR_INVALID_ARG && gCalls == 0);
    Pass::FDrawParameters none;
    EXPECT(none.Target == nullptr && none.SceneDepth == nullptr && none.Writer == nullptr && none.TargetPitch == 0 && none.DepthPitch == 0);
    pPass->RecordCommands(&none);                                                                               // no target: no call
    EXPECT(pass->LastStatus() == VQHIP_ERR_INVALID_ARG && gCalls == 0 && gAllocs == 0);

    static uint16_t color[4], volumes[4]; static float depth[1]; static uint32_t wr[1]; static VQ_UnlitData cbs[2];     // addresses only
    static unsigned char instanced[VQHIP_LINES_MAX_INSTANCES * 64 + 16];
    vqhip_shadow_mesh cube = {};
    cube.numIndices = 36; cube.strideBytes = 44; cube.indexBits = 32;
    // the instanced cbuffer: the matrices first, the colour behind all 512 of them whatever the batch holds
    const vqhip_line_draw box = Pass::Box(cube, instanced, 512), last = Pass::Box(cube, instanced, 1);
    EXPECT(box.kind == VQHIP_LINES_WIREFRAME && box.numInstances == 512 && (const void*)box.matModelViewProj == (const void*)instanced &&
           (const unsigned char*)box.color == instanced + 512 * 64 && box.axes == nullptr && box.mesh.numIndices == 36);
    EXPECT(last.numInstances == 1 && (const unsigned char*)last.color == instanced + 512 * 64);
    vqhip_shadow_mesh sphere = {};
    sphere.numIndices = 300;
    const vqhip_line_draw bound = Pass::Bound(sphere, cbs + 1);
    EXPECT(bound.kind == VQHIP_LINES_WIREFRAME && bound.numInstances == 1 && bound.matModelViewProj == &cbs[1].matModelViewProj && bound.color == &cbs[1].color &&
           (const unsigned char*)bound.color - (const unsigned char*)bound.matModelViewProj == 64 && bound.axes == nullptr);
    EXPECT(Pass::Lines(box) == 36 * 512 && Pass::Lines(last) == 36 && Pass::Lines(bound) == 300);

    std::vector<vqhip_line_draw> boxes = { box, last };
    const Pass::FTarget sceneColor = { color, 2048 }, boundingVolumes = { volumes, 0 };
    pPass->OnCreateWindowSizeDependentResources(1920, 1080, nullptr);
    // the boxes with reflections: into the bounding-volumes target
    Pass::FDrawParameters p = Pass::BoundingBoxes(&none, &boxes, true, sceneColor, boundingVolumes, depth, 1984);
    EXPECT(p.Target == volumes && p.TargetPitch == 0 && p.SceneDepth == depth && p.DepthPitch == 1984 && p.Writer == nullptr);
    Pass::FDrawParameters noDepth = p;
    noDepth.SceneDepth = nullptr;
    pPass->RecordCommands(&noDepth);                                                                            // no depth: no call
    EXPECT(pass->LastStatus() == VQHIP_ERR_INVALID_ARG && gCalls == 0);
    p.Writer = wr;
    gStatus = 4321;                                                                                             // the library's status is kept
    pPass->RecordCommands(&p);
    EXPECT(gCalls == 1 && pass->LastStatus() == 4321);
    gStatus = VQHIP_OK;
    pPass->RecordCommands(&p);
    EXPECT(gCalls == 2 && pass->LastStatus() == VQHIP_OK);
    EXPECT(gCtx == ctx && gStream == &none && gWidth == 1920 && gHeight == 1080 && gDraws.size() == 2 && std::memcmp(gDraws.data(), boxes.data(), 2 * sizeof(boxes[0])) == 0);
    EXPECT(gTargets.sceneColor == volumes && gTargets.pitch == 0 && gTargets.sceneDepth == depth && gTargets.depth_pitch == 1984 && gTargets.writer == wr &&
           gTargets.writer_pitch == 0 && gTargets.reserved == 0);
    EXPECT(gSizeLines == 36 * 513 && gAllocs == 1 && gAllocBytes == 256 + 36 * 513 * 40 && gWork == pass->GetWorkBuffer() && gWorkBytes == gAllocBytes && gFrees == 0);
    // ... and without: straight into scene colour
    p = Pass::BoundingBoxes(&none, &boxes, false, sceneColor, boundingVolumes, depth);
    EXPECT(p.Target == color && p.TargetPitch == 2048 && p.DepthPitch == 0);
    pPass->RecordCommands(&p);
    EXPECT(gCalls == 3 && gTargets.sceneColor == color && gTargets.pitch == 2048 && gTargets.writer == nullptr && gAllocs == 1);

    // the light volumes as wire: fewer lines, the buffer is kept
    std::vector<vqhip_line_draw> bounds = { bound, Pass::Bound(sphere, cbs) };
    p = Pass::LightBounds(&none, &bounds, true, sceneColor, boundingVolumes, depth);
    EXPECT(p.Target == volumes);
    pPass->RecordCommands(&p);
    EXPECT(gCalls == 4 && gSizeLines == 600 && gAllocs == 1 && gWorkBytes == 256 + 36 * 513 * 40 && gDraws.size() == 2 && gDraws[1].color == &cbs[0].color);
    bounds[1].mesh.numIndices = 30000;                                                                          // more: it grows (the old one is freed first)
    pPass->RecordCommands(&p);
    EXPECT(gCalls == 5 && gAllocs == 2 && gFrees == 1 && gWorkBytes == 256 + 30300 * 40);
    p.Draws = nullptr;                                                                                          // nothing to draw: the call is made, with no draws
    pPass->RecordCommands(&p);
    EXPECT(gCalls == 6 && gDrawsNull && gDraws.empty() && gSizeLines == 0 && pass->LastStatus() == VQHIP_OK && gAllocs == 2);
    bounds[1].mesh.numIndices = 30000000;                                                                       // beyond the library's limit: the size function says 0, no call
    p.Draws = &bounds;
    pPass->RecordCommands(&p);
    EXPECT(gCalls == 6 && pass->LastStatus() == VQHIP_ERR_HIP);
    pPass->Destroy();
    EXPECT(gFrees == 2 && pass->GetWorkBuffer() == nullptr && pass->GetWorkBytes() == 0);
    return 0;
}

static int vertexAxes(vqhip_ctx* ctx) {
    using Pass = vqhip::VertexAxesPass;
    const int calls0 = gCalls, allocs0 = gAllocs;
    std::shared_ptr<::IRenderPass> pPass = std::make_shared<Pass>(ctx);
    Pass* pass = static_cast<Pass*>(pPass.get());
    EXPECT(pPass->Initialize());
    static uint16_t color[4], volumes[4]; static float depth[1]; static VQ_VertexAxesData cb;
    vqhip_shadow_mesh mesh = {};
    mesh.numIndices = 1001; mesh.strideBytes = 44; mesh.indexBits = 16;                                         // a point list: any number of indices
    const vqhip_line_draw d = Pass::Mesh(mesh, &cb);
    EXPECT(d.kind == VQHIP_LINES_VERTEX_AXES && d.axes == &cb && d.matModelViewProj == nullptr && d.color == nullptr && d.numInstances == 1 && Pass::Lines(d) == 3003);
    std::vector<vqhip_line_draw> draws = { d };
    const Pass::FTarget sceneColor = { color, 0 }, boundingVolumes = { volumes, 4096 };
    pPass->OnCreateWindowSizeDependentResources(3840, 2160, nullptr);
    Pass::FDrawParameters p = Pass::VertexAxes(nullptr, &draws, true, sceneColor, boundingVolumes, depth);
    pPass->RecordCommands(&p);
    EXPECT(gCalls == calls0 + 1 && gAllocs == allocs0 + 1 && gSizeLines == 3003 && gWidth == 3840 && gHeight == 2160 && gTargets.sceneColor == volumes && gTargets.pitch == 4096 &&
           gStream == nullptr && gDraws.size() == 1 && gDraws[0].axes == &cb && pass->LastStatus() == VQHIP_OK);
    p = Pass::VertexAxes(nullptr, &draws, false, sceneColor, boundingVolumes, depth);
    pPass->RecordCommands(&p);
    EXPECT(gCalls == calls0 + 2 && gTargets.sceneColor == color && gTargets.pitch == 0 && gAllocs == allocs0 + 1);
    pPass->OnDestroyWindowSizeDependentResources();
    pPass->Destroy();
    return 0;
}

int main() {
    static_assert(std::is_base_of<::IRenderPass, vqhip::WireframePass>::value && std::is_base_of<::IRenderPass, vqhip::VertexAxesPass>::value,
                  "the adaptors derive from the engine's IRenderPass");
    vqhip_ctx* ctx = reinterpret_cast<vqhip_ctx*>(static_cast<uintptr_t>(0x1000));      // never dereferenced: the library call is the recorder above
    if (int rc = wireframe(ctx)) return rc;
    if (int rc = vertexAxes(ctx)) return rc;
    EXPECT(gFrees == gAllocs);
    std::printf("line draws adaptor OK\n");
    return 0;
}
