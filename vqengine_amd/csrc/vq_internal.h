// vq_internal.h — shared declarations between the C-ABI translation unit (capi.hip) and the kernel
// translation units. Not part of the public boundary (that is include/vqhip.h).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/vqhip.h"

namespace vqk {

// roctx range around the host side of an entry point, named after the GPU marker the reference opens at the call it replaces
// (SCOPED_GPU_MARKER, e.g. SceneRendering.cpp:1630 "RenderSceneColor"), so a rocprofv3 --marker-trace timeline reads like a PIX capture of
// the engine. The marker library (librocprofiler-sdk-roctx / libroctx64) is bound at run time; absent library or VQHIP_ROCTX=0: no-op.
struct Range {
    explicit Range(const char* name);
    ~Range();
    Range(const Range&) = delete;
    Range& operator=(const Range&) = delete;
    bool on;
};

// Tuning / A-B options of one context (vqhip_set_option, include/vqhip.h). Read by the launchers from the context the call came through — never
// from the process environment: getenv racing a host setenv is undefined behaviour in glibc and the engine is heavily threaded. 0 / "" = the default.
struct Options {
    int shadeWg = 0;            // "shade_wg"          : 64 | 128 | 256 lanes per workgroup of the shade kernels k_forward_lighting and k_msaa_shade (default: by frame size)
    int psmainWaves = 0;        // "psmain_waves"      : 4 | 5 | 6 waves per SIMD of the fused PSMain kernel
    int blurYWgs = 0;           // "blur_y_wgs"        : workgroups of k_blur_y_tonemap_lut
    int msaaEdgeWgs = 0;        // "msaa_edge_wgs"     : 256-lane workgroups of the persistent k_msaa_edges (default: as many as fill every CU once; clamped at launch)
    int postForm = 0;           // "post_form"         : 1 "two" = blur X, then blur Y + tonemap (two kernels) whatever the frame; 2 "chain" = k_post_chain whatever the size
                                //                       (default: k_post_chain for RGBA16F -> RGBA8 frames of >= 2^20 pixels with a per-channel display curve, else two kernels)
    int postStrips = 0;         // "post_strips"       : row strips per column strip of k_post_chain (default: CUs / column strips — one workgroup per CU)
    int lutForm = 0;            // "lut_form"          : 1 "general" (every range test left in)
    int diffuseForm = 0;        // "diffuse_form"      : 1 "texels", 2 "general" (default: footprint records)
    int specularForm = 0;       // "specular_form"     : 1 "general" (default: the branch-free sample with one validity flag)
    int diffuseSeqForm = 0;     // "diffuse_seq_form"  : 1 "lane" (default: k_conv_diffuse_ordered)
    int interpForm = 0;         // "interp_form"       : lane | wave — k_scene_interpolants with or without the one-owner-per-wave path (default: profiles/r16a_scene_interpolants.md)
    int rasterTile = 0;         // "raster_tile"       : 32 | 64 texels per side of k_raster_fill's tile (default 32, profiles/r14a_shadow_raster.md)
};

// Device-resident per-call constant block == the cbuffers b0/b1 of ForwardLighting.hlsl:76-77 plus the
// resource descriptors that replace its SRV tables. Uploaded once per vqhip_forward_lighting call into a
// slot of the context's constant ring (the analogue of the reference's DynamicBufferHeap bump allocation,
// SceneRendering.cpp:432-434,455-457). `extra` lights follow the struct in the same slot.
struct alignas(16) FrameConstants {
    VQ_PerFrameData        perFrame;       // 7120 B
    VQ_PerViewLightingData perView;        // 320 B
    vqhip_envmap           env;            // device pointers
    vqhip_shadowmaps       sm;             // device pointers
    int32_t                hasEnv;
    int32_t                numPointAll;    // numPointLights + numExtraPoint
    int32_t                pow5ExpLog;     // vqhip_set_fresnel_pow: 0 = product (default), 1 = exp2(5*log2 x)
    int32_t                pointFastOK;    // every point light's rangeSq <= 2^60 (or never lit) and every coordinate of its position is 0 or has magnitude in [2^-40, 2^40]:
                                           // preconditions of the unchecked light loop (vq_shade.h)
    float                  hdriSin, hdriCos;   // sin / cos(-fHDRIOffsetInRadians): frame-uniform, taken CORRECTLY ROUNDED on the host (double libm
                                               // rounded to float, capi.hip; contract v5 — the oracle does the same), not the contract's polynomial
    int32_t                pointSkipOK;    // every point light's color*brightness is finite: precondition of the back-facing-light skip (shade.hip)
    int32_t                pointNegZeroAxes;   // bit c: some point light has the coordinate -0.0 on axis c (then a pixel whose P has +0.0 there takes the IEEE loop: (-0) - (+0) = -0)
    // What the spot / directional lights hand to every pixel alike, formed once on the host with the operations the shader would use (round 6):
    // spot[0..20) belong to Lights.spot_lights, spot[20..25) to Lights.spot_casters
    struct alignas(16) DevSpotLight {
        float sdx, sdy, sdz;       // normalize(l.spotDir) in the context's reading (Lighting.hlsl:60): IEEE quotients by the length | v * correctly rounded rsqrt
        float rConeDen;            // RN(1 / (outerConeAngle - innerConeAngle)), the divisor of the penumbra quotient (:71)
        float cbx, cby, cbz;       // l.color * l.brightness (:330)
        int32_t flags;             // bit 0: outer - inner and its reciprocal are normal numbers (the penumbra quotient may use the corrected product);
                                   // bit 1: color * brightness is finite (a light that adds w = +0 times a finite BRDF may be skipped)
    } spot[VQ_NUM_LIGHTS__SPOT + VQ_NUM_SHADOWING_LIGHTS__SPOT];
    float                  dirWi[3];           // normalize(-directional.lightDirection) in the context's reading (Lighting.hlsl:337)
    int32_t                pad6[1];
    // DevPointLight pts[numPointAll] follows
};
using DevSpotLight = FrameConstants::DevSpotLight;
// Non-shadowing point lights as the hot loop reads them (one s_load_dwordx8 per light): point_lights[0..numPointLights)
// followed by the extension array, with the loop-invariant product color*brightness formed once on the host (IEEE
// multiply, identical to the in-shader product).
// `rangeSq` is the exact threshold of the range cull in squared distance: the smallest float t with sqrtf(t) >= range, so that
// (sqrt(dd) < range) == (dd < rangeSq) for every dd (sqrt is correctly rounded, hence monotonic) and culled lights need no sqrt.
struct alignas(16) DevPointLight { float px, py, pz, range; float cbx, cby, cbz, rangeSq; };
static constexpr int    kMaxExtraPointLights = 1024;
static constexpr size_t kConstSlotBytes = (sizeof(FrameConstants) + (VQ_NUM_LIGHTS__POINT + kMaxExtraPointLights) * sizeof(DevPointLight) + 255) & ~(size_t)255;

// the draw's other render targets (vqhip_psmain_targets, include/vqhip.h): pointers NULL = target not bound (wave-uniform tests in the kernels)
struct MrtArgs {
    void* albedo; void* motion;                     // SV_TARGET1 (ForwardLighting.hlsl:383), motion vectors (:387)
    const float4* svCurr; const float4* svPrev;     // PSInput :49-52
    int albedoPitch, motionPitch, svPitch;
    int albedoF32, motionF32;                       // storage: 0 = RGBA16F / RG16F (the reference's formats), 1 = RGBA32F / RG32F
};
struct ShadeArgs {
    const float4* gb0; const float4* gb1; const float4* gb2; const float4* gb3;
    void* out;
    const FrameConstants* fc;   // device
    int width, height, pitch, outPitch;
    int arithDxc;               // vqhip_set_arithmetic: 0 literal reading, 1 DXC reading (selects the kernel instantiation)
    MrtArgs mrt;                // last: the kernels without extra targets keep their argument offsets
};

// G-buffer producer (§8f.1): per-call constants in a ring slot — cbPerObject.materialData + descriptor tables of every
// material referenced by the interpolant planes.
struct alignas(16) GbufConstants {
    float      ambient;          // cbPerFrame.fAmbientLightingFactor
    int32_t    numMaterials;
    vqhip_ssao ssao;             // device pointer or NULL
    int32_t    arithDxc;         // vqhip_set_arithmetic: the reading of dot / normalize / length in the producer (wave-uniform run-time flag)
    int32_t    pad[1];
    vqhip_material mats[1];      // numMaterials entries
};
static constexpr int kMaxMaterials = (int)((kConstSlotBytes - offsetof(GbufConstants, mats)) / sizeof(vqhip_material));
struct GbufArgs {
    const float4* ip0; const float4* ip1; const float4* ip2;
    float4* gb0; float4* gb1; float4* gb2; float4* gb3;
    const GbufConstants* gc;     // device
    int width, height, pitch, outPitch;
};
hipError_t launch_gbuffer_from_materials(hipStream_t s, const GbufArgs& a);
hipError_t launch_scene_normals_from_materials(hipStream_t s, const GbufArgs& a, void* out, int outFmt);   // a.gb* unused, a.outPitch = pitch of `out`
struct FrameConstants;
hipError_t launch_forward_from_materials(hipStream_t s, const GbufArgs& a, const FrameConstants* fc, bool hasEnv, bool hasCasters, void* out, int outPitch, int outFmt, int arithDxc, const Options& opt, const MrtArgs& mrt);
// §7.20: the quad-uv plane, float4 [height][pitch] = the owner primitive's vertex uv at the helper lanes (i ^ 1, j) and (i, j ^ 1). Written by the QUAD instantiations of
// k_scene_interpolants (raster_attr.hip), read by the QUAD instantiations of the surface producers (gbuffer.hip); it travels as a kernel parameter of its own, so
// that every other instantiation keeps its parameter list.
struct QuadPlane { void* uv; uint32_t pitch; };
hipError_t launch_gbuffer_from_materials_quad(hipStream_t s, const GbufArgs& a, const QuadPlane& quad);
hipError_t launch_scene_normals_from_materials_quad(hipStream_t s, const GbufArgs& a, void* out, int outFmt, const QuadPlane& quad);
hipError_t launch_forward_from_materials_quad(hipStream_t s, const GbufArgs& a, const FrameConstants* fc, bool hasEnv, bool hasCasters, void* out, int outPitch, int outFmt, int arithDxc, const Options& opt, const MrtArgs& mrt, const QuadPlane& quad);
hipError_t launch_mip_box_rgba8(hipStream_t s, const void* src, void* dst, int sw, int sh, int dw, int dh);
hipError_t launch_skydome(hipStream_t s, const float4* eq0, int w0, int h0, const VQ_SkydomeParams& sp, const float4* cov, int covPitch,
                          void* color, int W, int H, int pitch, int fmt);

struct UnlitColors { float4 c[VQHIP_MAX_UNLIT_COLORS]; };
hipError_t launch_unlit_composite(hipStream_t s, const float4* cov, int covPitch, const UnlitColors& cols, int n, void* color, int W, int H, int pitch, int fmt);

// HDRI ingest (§8f.3, hdri.hip): host-side header parse / run expansion (0 or -1 with *err set), device conversion
int hdr_parse_header(const uint8_t* f, size_t n, int* w, int* h, size_t* off, const char** err);
int hdr_expand_rgbe(const uint8_t* f, size_t n, size_t off, int w, int h, uint8_t* rgbe, const char** err);
hipError_t launch_rgbe_to_rgba32f(hipStream_t s, const void* rgbe, void* out, size_t n);
int hdr_walk_runs(const uint8_t* f, size_t n, size_t off, int w, int h, uint32_t* planeOff, const char** err);
bool hdr_expand_fits(const uint32_t* planeOff, int w, int h, int ldsLimit, int* encCap, int* pitch, int* ldsBytes);
hipError_t launch_hdr_expand(hipStream_t s, const void* file, const void* planeOff, void* out, int w, int h, int encCap, int pitch, int ldsBytes);
hipError_t launch_downsize_box(hipStream_t s, const void* src, void* dst, int sw, int sh, int k);

// FSR 1.0 (§8f.4, fsr.hip)
hipError_t launch_fsr_easu(hipStream_t s, const void* in, int inW, int inH, int inFmt, const uint32_t* con16, void* out, int outW, int outH, int outFmt);
hipError_t launch_fsr_rcas(hipStream_t s, const void* in, void* out, int W, int H, const uint32_t* con4, int inFmt, int outFmt);
hipError_t launch_visualize(hipStream_t s, const void* in, void* out, int W, int H, const VQ_VizParams& p, int inFmt, int outFmt);
hipError_t launch_apply_reflections(hipStream_t s, const void* refl, const void* boundingVolumes, void* scene, int W, int H, int fmt);   // boundingVolumes NULL: plain permutation

// SSR environment fallback (§8f.4, ssr.hip): what the kernel reads of VQ_SSSRConstants + the resource descriptors, by value
struct SsrArgs {
    const void* scene; const float* depth; const void* normals; void* out; uint8_t* outRoughness;
    int width, height, scenePitch, depthPitch, normalPitch, outPitch;
    VQ_matrix invProj, view, invView;
    float rot[3][3];                      // upper-left 3x3 of envMapRotation
    float invDimX, invDimY, roughnessThreshold, mipCount;
    int pow5ExpLog, arithDxc;
    vqhip_envmap env;
};
hipError_t launch_ssr_env_fallback(hipStream_t s, const SsrArgs& a, int sceneFmt, int normalFmt, int outFmt);

// SSR ray list + hierarchical march (vqhip_ssr_classify / vqhip_ssr_intersect, ssr_trace.hip; docs/DESIGN_DETAILS.md §7.11)
static constexpr int kMaxSsrTiles = 512 * 512;    // 8 x 8 tiles of a 4096 x 4096 frame
struct SsrClassifyArgs {
    const void* scene; const float* depth; const void* variance;      // variance: R16F plane or NULL (reads 0)
    uint32_t* rayList; uint32_t* counters; uint32_t* tileList;        // tileList may be NULL
    uint32_t* tileRays; uint32_t* tileFlag;                           // context-owned, kMaxSsrTiles each: per-tile ray count / "has a glossy reflective pixel", scanned in place
    int width, height, scenePitch, depthPitch, variancePitch, sceneF32, tilesX, tilesY;
    float roughnessThreshold, varianceThreshold;
    uint32_t samplesPerQuad, varianceGuided;
};
struct SsrTraceArgs {
    const uint32_t* rayList; const uint32_t* counters;
    const void* lit; const float* mips; const void* normals; const uint8_t* roughness; const uint8_t* noise; void* out;
    int width, height, litPitch, normalPitch, outPitch, litF32, normF32, outF32, levels;
    VQ_matrix invViewProj, proj, invProj, view, invView;
    float rot[3][3];                      // upper-left 3x3 of envMapRotation
    float invDimX, invDimY, thickness;
    uint32_t maxIter, minOcc, mostDetailedMip;
    int pow5ExpLog, arithDxc;
    vqhip_envmap env;
};
hipError_t launch_ssr_classify(hipStream_t s, const SsrClassifyArgs& a);
hipError_t launch_ssr_intersect(hipStream_t s, const SsrTraceArgs& a, int nCUs);

// SSR denoiser passes 2 and 3 (vqhip_ssr_prefilter / vqhip_ssr_resolve_temporal, ssr_denoise.hip; docs/DESIGN_DETAILS.md §7.12). One argument block for both:
// the prefilter leaves reprojected / sampleCount NULL, the temporal resolve depth / normals. Pitches in pixels.
struct SsrDenoiseArgs {
    const uint32_t* tileList; const uint32_t* counters;               // counters[1] tiles, read on the device and clamped to tilesX * tilesY
    const float* depth; const void* normals; const uint8_t* roughness; const void* avg;
    const void* radiance; const void* reprojected; const void* variance; const void* sampleCount;
    void* outRadiance; void* outVariance;
    int width, height, tilesX, tilesY, avgW, avgH;
    int depthPitch, normalPitch, radiancePitch, reprojectedPitch, variancePitch, sampleCountPitch, outPitch, outVariancePitch;
    int normF32, avgF32, radF32, reprojF32, outF32, arithDxc;
    float ipZ[4], ipW[4];                                             // columns 2 and 3 of invProjection: all GetLinearDepth reads
    float roughnessThreshold, temporalStability;
    float roundUp8W, roundUp8H;                                       // float2(FFX_DNSR_Reflections_RoundUp8(screen_size)), as written: value + 8 unless a multiple of 8
};
hipError_t launch_ssr_prefilter(hipStream_t s, const SsrDenoiseArgs& a, int nCUs);
hipError_t launch_ssr_resolve_temporal(hipStream_t s, const SsrDenoiseArgs& a, int nCUs);

// SSR denoiser pass 1 (vqhip_ssr_reproject, ssr_reproject.hip; docs/DESIGN_DETAILS.md §7.13). Pitches in pixels.
struct SsrReprojectArgs {
    const uint32_t* tileList; const uint32_t* counters;               // counters[1] tiles, read on the device and clamped to tilesX * tilesY
    const float* depth; const void* normals; const uint8_t* roughness;
    const float* depthHist; const void* normalHist; const uint8_t* roughnessHist;
    const void* radiance; const void* radianceHist; const void* motion; const void* varianceHist; const void* sampleCountHist;
    void* outReprojected; void* outAverage; void* outVariance; void* outSampleCount;
    int width, height, tilesX, tilesY;
    int depthPitch, normalPitch, roughnessPitch, depthHistPitch, normalHistPitch, roughnessHistPitch, radiancePitch, radianceHistPitch, motionPitch,
        varianceHistPitch, sampleCountHistPitch, outReprojectedPitch, outVariancePitch, outSampleCountPitch;
    int normF32, normHistF32, radF32, radHistF32, motionF32, outF32, avgF32, arithDxc;
    VQ_matrix invProj, invView, prevViewProj;
    float roughnessThreshold;
};
hipError_t launch_ssr_reproject(hipStream_t s, const SsrReprojectArgs& a, int nCUs);

// 4x MSAA lit draw + resolve (vqhip_forward_lighting_msaa, msaa.hip). Edge pixels (samples with more than one owner) are listed by the
// shading kernel in edgeList[0 .. *edgeCount) as y * width + x; *edgeCount is zeroed on the call's stream before the launch.
struct MsaaLayer { const float4* gb0; const float4* gb1; const float4* gb2; const float4* gb3; const uint8_t* cov; int pitch; };
struct MsaaArgs {
    MsaaLayer L[VQHIP_MSAA_MAX_LAYERS];
    const void* bg;             // background plane in the output format, NULL = (0,0,0,0)
    void* out;
    const FrameConstants* fc;   // device
    uint32_t* edgeCount; uint32_t* edgeList;
    int width, height, layers, covPitch, bgPitch, outPitch;
};
hipError_t launch_forward_lighting_msaa(hipStream_t s, const MsaaArgs& a, bool hasEnv, bool hasCasters, int outFmt, int arithDxc, int nCUs, const Options& opt);

// 4x MSAA surface resolve + depth hierarchy (vqhip_msaa_resolve_surfaces / vqhip_depth_hierarchy, depth.hip). Output pointers NULL = that output is not live.
struct SurfLayer { const uint8_t* cov; const void* normals; const float4* gb1; int nPitch, rPitch; };
struct SurfArgs {
    SurfLayer L[VQHIP_MSAA_MAX_LAYERS];
    const float4* depthMS;      // one float4 per pixel: the four samples
    const void* bg;             // background plane in the scene colour's format, NULL = alpha 0
    float* outDepth; void* outNormals; void* scene;
    int width, height, layers, covPitch, depthPitch, bgPitch, outDepthPitch, outNormalsPitch, scenePitch;
    int nInF32, nOutF32, sceneF32, arithDxc;
};
static constexpr int kMaxDepthLevels = 13;        // 4096 x 4096
static constexpr int kMaxDepthTiles = 64 * 64;    // 64 x 64 tiles of level 0
struct HierArgs {
    const float* src;           // R32F plane (srcPitch floats per row) or, for the MSAA form, the four samples per pixel (srcPitch pixels per row)
    float* mips;
    float* tileMin;             // context-owned: kMaxDepthTiles per-tile minima (TRUE_TOP on a frame of more than one tile), else unused
    uint32_t off[kMaxDepthLevels];   // start of level l in floats
    int width, height, srcPitch, levels, flags;
};
hipError_t launch_resolve_surfaces(hipStream_t s, const SurfArgs& a);
hipError_t launch_depth_hierarchy(hipStream_t s, const HierArgs& a, bool ms);

// FidelityFX CACAO at quality HIGH (vqhip_cacao, cacao.hip; docs/DESIGN_DETAILS.md §7.14). depthPitch in floats, normalPitch in pixels, aoPitch in bytes;
// off*: byte offsets of the planes inside the work buffer (vqhip_cacao_plane_offset_bytes), mw / mh: the sizes of the four depth mips.
struct CacaoArgs {
    const float* depth; const void* normals; uint8_t* work; uint8_t* ao;
    size_t offDepth[4], offNormals, offPing, offPong;
    int mw[4], mh[4];
    int width, height, hw, hh, depthPitch, normalPitch, aoPitch, normF32, blurPasses;
};
hipError_t launch_cacao(hipStream_t s, const CacaoArgs& a, const VQ_CacaoConstants& shared, const VQ_CacaoConstants perPass[4]);
// Quality HIGHEST (vqhip_adaptive_cacao; §7.15): the three planes appended to the work buffer — the importance map and its pong, R8_UNORM iw x ih, and the load counter
struct CacaoAdaptiveArgs { size_t offImportance, offImportancePong, offCounter; int iw, ih; };
hipError_t launch_cacao_adaptive(hipStream_t s, const CacaoArgs& a, const CacaoAdaptiveArgs& ad, const VQ_CacaoConstants& shared, const VQ_CacaoConstants perPass[4]);

// Shadow-map rasteriser (vqhip_shadow_depth, raster.hip; docs/DESIGN_DETAILS.md §7.16). The view table and the draw jobs travel in constant-ring slots.
// Work buffer: 64 record counters (one per view), the records' texel boxes (8 B each), the records (80 B each); a view owns the region
// [recBase, recBase + recCap) of both arrays, recCap = 6 x its instanced triangles.
struct alignas(16) RasterView {
    float* depth; uint64_t recBase, recCap;
    uint32_t pitch;                  // floats per row
    int32_t dim, linear;
    uint32_t firstFillBlock;         // of k_raster_fill's grid
    float cam[3]; float farPlane;
};
struct alignas(16) RasterJob {       // one vqhip_shadow_draw of one view
    const uint8_t* positions; const void* indices; const VQ_matrix* wvp; const VQ_matrix* world;
    uint32_t strideBytes, numVertices, numTris, numInstances;
    int32_t indexBits, cullMode, view;
    uint32_t firstBlock;             // of this k_raster_setup launch: ceil(numTris * numInstances / 256) blocks per job
};
static constexpr size_t kRasterBoxBytes = 8, kRasterRecordBytes = 80, kRasterCounterBytes = 256;
hipError_t launch_raster_begin(hipStream_t s, uint32_t* counters, int numViews);
// setup and fill take the call's MaskArgs (§7.19, below) as one more argument when a draw of the call is alpha-tested: JOB = RasterJob, or RasterMaskedJob with MaskArgs
template <class JOB, class... MA>
hipError_t launch_raster_setup(hipStream_t s, const JOB* jobs, int numJobs, uint32_t blocks, const RasterView* views, uint32_t* counters, void* boxes, void* records, const MA&... mask);
template <class... MA>
hipError_t launch_raster_fill(hipStream_t s, const RasterView* views, int numViews, uint32_t blocks, int tile, const uint32_t* counters, const void* boxes, const void* records, const MA&... mask);

// Main-view depth pre-pass (vqhip_scene_depth, raster_view.hip; docs/DESIGN_DETAILS.md §7.17). The draw jobs travel in constant-ring slots, the targets as kernel arguments.
// Work buffer: one record counter (256 B), the records' pixel boxes (8 B each), the records (48 B each: three snapped vertices, three z/w, q); recCap = 8 x the
// call's instanced triangles (a triangle clipped by seven planes is a fan of at most eight).
struct SceneDepthArgs {
    float* depth; uint32_t* primitive;
    uint8_t* coverage[4]; uint32_t* layerPrimitive[4];
    uint64_t recCap;
    uint32_t pitch, coveragePitch;   // pixels per row of depth / primitive / layerPrimitive; bytes per row of coverage
    int32_t width, height, samples, layers;
};
struct alignas(16) SceneDepthJob {   // one vqhip_scene_depth_draw
    const uint8_t* positions; const void* indices; const VQ_matrix* wvp;
    uint32_t strideBytes, numVertices, numTris, numInstances;
    int32_t indexBits, cullMode;
    uint32_t firstBlock;             // of this k_scene_setup launch: ceil(numTris * numInstances / 256) blocks per job
    uint32_t firstQ;                 // sequence number of (instance 0, triangle 0): the instanced triangles of the draws before
    uint32_t maskSlot, firstMasked;  // read by k_scene_setup<MaskArgs> alone (the struct's tail padding before): see MaskTex below
};
static_assert(sizeof(SceneDepthJob) == 64, "SceneDepthJob is four uint4");
static constexpr size_t kSceneBoxBytes = 8, kSceneRecordBytes = 48, kSceneCounterBytes = 256, kSceneFanMax = 8;
int scene_depth_tile(int rasterTile, int samples);      // pixels per side of k_scene_fill's tile: the option where the LDS budget allows it (not 64 at 4x), else 32
// as the shadow rasteriser's: with the call's MaskArgs when a draw of the call is alpha-tested, without it otherwise
template <class... MA>
hipError_t launch_scene_setup(hipStream_t s, const SceneDepthJob* jobs, int numJobs, uint32_t blocks, const SceneDepthArgs& a, uint32_t* counter, void* boxes, void* records, const MA&... mask);
template <class... MA>
hipError_t launch_scene_fill(hipStream_t s, const SceneDepthArgs& a, int tile, const uint32_t* counter, const void* boxes, const void* records, const MA&... mask);

// Alpha-tested geometry in both rasterisers (vqhip_scene_masked_depth, vqhip_shadow_masked_depth; docs/DESIGN_DETAILS.md §7.19). A masked call appends to the
// work buffer of the opaque call: MaskTex[number of draws] | MaskSide[masked instanced triangles], each part rounded up to 256 bytes. The table travels through constant-ring slots
// into the work buffer (k_table_copy), as vqhip_scene_interpolants' draw table does. A job's maskSlot is 1 + its entry in the table, 0 for an opaque draw;
// firstMasked is the number of masked instanced triangles of the jobs before it. Setup writes the side record of masked triangle firstMasked + t when the
// triangle emits a record, and stores 1 + that number in the record's last-but-one word (0 in an opaque draw's records, as before): the fan pieces of a
// clipped triangle share one side record, so M2's uv cannot depend on the piece.
struct alignas(16) MaskTex {         // what the alpha test reads of a draw's material: 48 bytes
    const void* texels; int32_t width, height, mips;
    int32_t pad0;
    float sx, sy, ox, oy;            // uvScaleOffset (scene depth); unused by the shadow rule
    uint32_t pad1[2];
};
static_assert(sizeof(MaskTex) == 48, "MaskTex is three uint4");
struct alignas(16) MaskSide {        // per masked triangle: the unclipped clip-space (x, y, w) and the uv of its three vertices, the draw's table entry
    float c[9]; float uv[6]; uint32_t slot;
};
static_assert(sizeof(MaskSide) == 64, "MaskSide is four uint4");
struct MaskArgs { const MaskTex* table; MaskSide* side; uint64_t sideCap; uint32_t tableCap; };
struct alignas(16) RasterMaskedJob : RasterJob { uint32_t maskSlot, firstMasked, pad[2]; };
static_assert(sizeof(RasterMaskedJob) == 80, "RasterMaskedJob is five uint4");

// The lit draw's interpolants from meshes (vqhip_scene_interpolants, raster_attr.hip; docs/DESIGN_DETAILS.md §7.18). The draw table travels through constant-ring
// slots into the work buffer (one k_table_copy launch per slot): the resolve looks up any draw from any pixel, so the table needs a home that outlives the slots.
// Work buffer: SurfaceJob[number of draws with numIndices > 0], nothing else.
struct alignas(16) SurfaceJob {      // one vqhip_scene_surface_draw
    const uint8_t* vertices; const void* indices; const VQ_matrix* wvp; const VQ_matrix* world; const VQ_matrix* normal; const VQ_matrix* wvpPrev;
    uint32_t strideBytes, numVertices, numTris, numInstances;
    int32_t indexBits, materialIndex;
    uint32_t firstQ;                 // sequence number of (instance 0, triangle 0): the instanced triangles of the draws before
};
static_assert(sizeof(SurfaceJob) == 80, "SurfaceJob is five uint4");
struct SceneInterpArgs {
    const uint32_t* owner; void* ip[3]; void* sv[2];      // sv: both or neither
    uint32_t ownerPitch, pitch, svPitch;                  // pixels per row
    int32_t width, height, numJobs;
    uint32_t totalTris;                                   // q at or beyond it owns nothing
};
hipError_t launch_table_copy(hipStream_t s, const void* src, void* dst, uint32_t numUint4);
hipError_t launch_scene_interpolants(hipStream_t s, const SceneInterpArgs& a, const SurfaceJob* table, bool waveForm);   // waveForm: waves with one owner fetch it once
hipError_t launch_scene_quad_interpolants(hipStream_t s, const SceneInterpArgs& a, const SurfaceJob* table, bool waveForm, const QuadPlane& quad);

// The ObjectID pass's render target from an owner plane (vqhip_object_ids, raster_ids.hip; docs/DESIGN_DETAILS.md §7.21 P0). The draw table travels as
// vqhip_scene_interpolants' does: ring slots -> k_table_copy -> the work buffer. Work buffer: ObjectIdJob[number of draws with numIndices > 0], nothing else.
struct alignas(16) ObjectIdJob {     // one vqhip_object_id_draw
    const int32_t* objID;
    uint32_t numTris, numInstances;
    int32_t meshID, materialID;
    uint32_t firstQ;                 // sequence number of (instance 0, triangle 0): the instanced triangles of the draws before
    uint32_t pad;
};
static_assert(sizeof(ObjectIdJob) == 32, "ObjectIdJob is two uint4");
struct ObjectIdArgs {
    const uint32_t* owner; int32_t* ids;
    uint32_t ownerPitch, idsPitch;                        // pixels per row
    int32_t width, height, numJobs;
    uint32_t totalTris;                                   // q at or beyond it owns nothing
};
hipError_t launch_object_ids(hipStream_t s, const ObjectIdArgs& a, const ObjectIdJob* table, bool waveForm);   // waveForm: waves with one owner fetch its draw once

// The Outline pass (vqhip_outline, raster_outline.hip; docs/DESIGN_DETAILS.md §7.21 O1 .. O6). The draw jobs travel in constant-ring slots.
// Work buffer: one record counter (256 B) | OutlineColor[min(triangles, 20 000)] (one per draw with indices: the four colour halfs and the draw's index, written by
// the setup kernel) | the records' pixel boxes (8 B each) | the records (48 B each: three snapped vertices, three z/w, 0 for a mark record or 1 + the job's number
// for a paint record); recCap = 16 x the call's triangles (each pass: a triangle clipped by seven planes is a fan of at most eight).
struct alignas(16) OutlineJob {      // one vqhip_outline_draw
    const uint8_t* positions; const void* indices; const VQ_OutlineData* cb;
    uint32_t strideBytes, numVertices, numTris;
    int32_t indexBits;
    uint32_t firstBlock;             // of this k_outline_setup launch: ceil(numTris / 256) blocks per job
    uint32_t drawIndex;              // into the caller's draws
};
static_assert(sizeof(OutlineJob) == 48, "OutlineJob is three uint4");
struct alignas(16) OutlineColor { uint32_t rg, ba, drawIndex, pad; };
struct OutlineArgs {
    void* sceneColor; uint8_t* selection; uint32_t* writer;
    OutlineColor* colors;
    uint64_t recCap;
    uint32_t pitch, selectionPitch, writerPitch, colorCap;
    int32_t width, height;
};
static constexpr size_t kOutlineBoxBytes = 8, kOutlineRecordBytes = 48, kOutlineCounterBytes = 256, kOutlineFanMax = 16;
hipError_t launch_outline_setup(hipStream_t s, const OutlineJob* jobs, int numJobs, uint32_t firstJob, uint32_t blocks, const OutlineArgs& a, uint32_t* counter, void* boxes, void* records);
hipError_t launch_outline_fill(hipStream_t s, const OutlineArgs& a, int tile, const uint32_t* counter, const void* boxes, const void* records);

// Heightmap displacement of vertex streams (vqhip_displace_meshes, displace.hip; docs/DESIGN_DETAILS.md §7.22 H1 .. H4). The jobs travel in constant-ring slots,
// one launch per slot; no work buffer. Jobs without vertices are not in the table.
struct alignas(16) DisplaceJob {     // one vqhip_displace_job
    const void* vertices; void* out; const void* texels;    // texels NULL: the null SRV, the sample is 0
    uint32_t strideBytes, outStrideBytes, numVertices;
    int32_t width, height;           // level 0 of the height map
    uint32_t firstBlock;             // of this k_displace_vertices launch: ceil(numVertices / 256) blocks per job
    float sx, sy, ox, oy;            // uvScaleOffset
    float displacement;
    uint32_t pad[3];
};
static_assert(sizeof(DisplaceJob) == 80, "DisplaceJob is five uint4");
static constexpr int kDisplaceLanes = 256;               // vertices per block
hipError_t launch_displace(hipStream_t s, const DisplaceJob* jobs, int numJobs, uint32_t blocks);

// Unlit draws (vqhip_unlit_draws, raster_unlit.hip; docs/DESIGN_DETAILS.md §7.23 U1 .. U7). The draw jobs travel in constant-ring slots.
// Work buffer: UnlitColor[min(triangles, 20 000), at least 1] (one per draw with indices: the four colour floats and the draw's index, written by the setup kernel)
// | the triangles' pixel boxes (8 B each: the union of the triangle's slot boxes, what a tile looks at first) | the slots' pixel boxes (8 B each) | the slots'
// records (48 B each: three snapped vertices, three z/w, the job's number). Fan piece k of triangle q (§7.17's sequence number) lives in the FIXED slot 8 q + k; an
// unused slot, and a triangle without slots, holds the empty box: no append counter, and memory order is submission order.
struct alignas(16) UnlitJob {        // one vqhip_unlit_draw
    const uint8_t* positions; const void* indices; const VQ_UnlitData* cb;
    uint32_t strideBytes, numVertices, numTris;
    int32_t indexBits;
    uint32_t firstBlock;             // of this k_unlit_setup launch: ceil(numTris / 256) blocks per job
    uint32_t drawIndex;              // into the caller's draws
    uint32_t firstQ;                 // U4: the triangles of the jobs before this one, across ring slots
    int32_t cullMode;
    uint32_t pad[2];
};
static_assert(sizeof(UnlitJob) == 64, "UnlitJob is four uint4");
struct alignas(16) UnlitColor { float c[4]; uint32_t drawIndex, pad[3]; };
struct UnlitArgs {
    void* sceneColor; const float* sceneDepth; uint32_t* writer;
    UnlitColor* colors;
    uint32_t slots;                  // 8 x the call's triangles
    uint32_t pitch, depthPitch, writerPitch, colorCap;
    int32_t width, height, blend;
};
static constexpr size_t kUnlitBoxBytes = 8, kUnlitRecordBytes = 48, kUnlitFanMax = 8;
static constexpr uint32_t kUnlitEmptyBox = 0x0000ffffu;  // both words: first pixel 65535 > last pixel 0, beyond any target
hipError_t launch_unlit_setup(hipStream_t s, const UnlitJob* jobs, int numJobs, uint32_t firstJob, uint32_t blocks, const UnlitArgs& a, void* triBoxes, void* boxes, void* records);
hipError_t launch_unlit_fill(hipStream_t s, const UnlitArgs& a, int tile, const void* triBoxes, const void* boxes, const void* records);

// Line draws (vqhip_line_draws, raster_lines.hip; docs/DESIGN_DETAILS.md §7.24 L1 .. L8). The draw jobs travel in constant-ring slots.
// Work buffer: LineColor[4 x min(lines, 20 000), at least 4] (four per draw with lines: the wireframe colour, or the three axis colours, as halfs, and the draw's
// index, written by the setup kernel) | the lines' pixel boxes (8 B each) | the lines' records (32 B each: the snapped ends, the two z / w, the colour-table entry,
// the major axis). Line q (L7's sequence number) lives in the FIXED slot q; a dropped line holds the empty box: no append counter.
struct alignas(16) LineJob {         // one vqhip_line_draw
    const uint8_t* vertices; const void* indices; const VQ_float4* color;
    const void* cb;                  // WIREFRAME: VQ_matrix[numInstances]; VERTEX_AXES: one VQ_VertexAxesData
    uint32_t strideBytes, numVertices;
    uint32_t numPrims;               // WIREFRAME: triangles of one instance; VERTEX_AXES: indices (points)
    uint32_t numLines;               // WIREFRAME: 3 x numPrims x numInstances; VERTEX_AXES: 3 x numPrims
    uint16_t indexBits, kind;
    uint32_t firstBlock;             // of this k_lines_setup launch: ceil(numLines / 256) blocks per job
    uint32_t drawIndex;              // into the caller's draws
    uint32_t firstQ;                 // L7: the lines of the jobs before this one, across ring slots
};
static_assert(sizeof(LineJob) == 64, "LineJob is four uint4");
struct alignas(16) LineColor { uint32_t rg, ba, drawIndex, pad; };
struct LineArgs {
    void* sceneColor; const float* sceneDepth; uint32_t* writer;
    LineColor* colors;
    uint32_t lines;                  // the call's lines: the slots
    uint32_t pitch, depthPitch, writerPitch;
    uint32_t colorCap;               // entries of colors: four per job
    int32_t width, height;
};
static constexpr size_t kLineBoxBytes = 8, kLineRecordBytes = 32;
static constexpr uint32_t kLineColorsPerJob = 4;
static constexpr uint32_t kLineEmptyBox = 0x0000ffffu;   // both words: first pixel 65535 > last pixel 0, beyond any target
hipError_t launch_lines_setup(hipStream_t s, const LineJob* jobs, int numJobs, uint32_t firstJob, uint32_t blocks, const LineArgs& a, void* boxes, void* records);
hipError_t launch_lines_fill(hipStream_t s, const LineArgs& a, int tile, const void* boxes, const void* records);

// launchers (each returns the hipError_t of the launch)
hipError_t launch_forward_lighting(hipStream_t s, const ShadeArgs& a, bool hasEnv, bool hasCasters, int outFmt, const Options& opt);
hipError_t launch_blur_x(hipStream_t s, const void* in, void* out, int W, int H, int fmt, const Options& opt);
hipError_t launch_blur_y(hipStream_t s, const void* in, void* out, const void* haloTop, const void* haloBottom, int haloRows, int W, int H, int fmt);
bool tonemap_uses_lut(const VQ_TonemapperParams& p, int inFmt, int outFmt, size_t nPixels);
bool blur_y_tonemap_uses_lut(const VQ_TonemapperParams& p, int blurFmt, int outFmt, size_t nPixels);
hipError_t launch_tonemap_lut_build(hipStream_t s, void* table, const VQ_TonemapperParams& p, int outFmt);
hipError_t launch_tonemap(hipStream_t s, const void* in, void* out, int W, int H, const VQ_TonemapperParams& p, int inFmt, int outFmt, const void* lutTable, const Options& opt);
hipError_t launch_blur_y_tonemap(hipStream_t s, const void* in, void* out, const void* haloTop, const void* haloBottom, int haloRows, int W, int H,
                                 const VQ_TonemapperParams& p, int fmt, int outFmt, const void* lutTable, const Options& opt);
bool post_chain_applies(const VQ_TonemapperParams& p, int inFmt, int outFmt, int W, int H, const Options& opt);
hipError_t launch_post_chain(hipStream_t s, const void* in, void* out, const void* haloTop, const void* haloBottom, int haloRows, int W, int H,
                             const void* lutTable, int nCUs, const Options& opt);
hipError_t launch_brdf_lut(hipStream_t s, void* out, int size, int samples, int fmt, int pow5ExpLog, const Options& opt);
hipError_t launch_mip_min(hipStream_t s, const float4* src, float4* dst, int sw, int sh, int dw, int dh);
size_t conv_diffuse_record_bytes(int w0, int h0, int nMips);
hipError_t launch_conv_diffuse_tables(hipStream_t s, const float4* chain, int w0, int h0, int nMips, int res,
                                      const float* phis, int nPhi, const float* thetas, int nTheta, int order, void* out, int fmt, void* recBuf, const Options& opt);
hipError_t launch_conv_specular_all(hipStream_t s, const float4* chain, int w0, int h0, int nMips, int res0, int MIPS, int order, void* out, int fmt, const Options& opt);

} // namespace vqk
