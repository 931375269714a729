/*
 * vqhip.h — C ABI of the MI355X-native offscreen PBR-shading / IBL / post path.
 *
 * This is the drop-in boundary: plain C, pointers + sizes, no torch / HIP types.
 * Every entry point cites the reference call it replaces (paths relative to the VQEngine tree).
 *
 * Conventions
 *   - every `const void* / void*` image argument is a DEVICE pointer owned by the caller;
 *   - every `VQ_*` struct pointer is a HOST pointer (the reference fills these on the CPU and
 *     bump-allocates them into an upload heap: Source/Renderer/Rendering/SceneRendering.cpp:429-467);
 *   - every call enqueues on `stream` (a hipStream_t passed as void*; NULL = the null stream) and
 *     returns without synchronising, mirroring "record into a command list";
 *   - return value: VQHIP_OK (0) or a negative vqhip_status; vqhip_last_error() gives the text.
 *     (The reference returns void and asserts/logs: e.g. EnvironmentMapRendering.cpp:139, Renderer.cpp:871.)
 *   - images are dense row-major, `row_pitch_px` pixels between rows where stated, otherwise == width.
 *     An image (or row tile) has at most 65 535 rows: several kernels map rows to grid.y; taller inputs fail with VQHIP_ERR_HIP.
 *
 * Struct layouts are byte-for-byte those of Shaders/LightingConstantBufferData.h (namespace
 * VQ_SHADER_DATA); the static asserts below pin the offsets derived in SURVEY.md §8(b).
 */
#ifndef VQHIP_H
#define VQHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__cplusplus)
#define VQHIP_STATIC_ASSERT(c, m) static_assert(c, m)
#define VQHIP_ALIGNAS(n) alignas(n)
#else
#define VQHIP_STATIC_ASSERT(c, m) _Static_assert(c, m)
#define VQHIP_ALIGNAS(n) _Alignas(n)
#endif

#define VQHIP_API __attribute__((visibility("default")))

/* ------------------------------------------------------------------------------------------------
 * status / formats
 * ---------------------------------------------------------------------------------------------- */
typedef enum vqhip_status {
    VQHIP_OK                = 0,
    VQHIP_ERR_INVALID_ARG   = -1,
    VQHIP_ERR_HIP           = -2,   /* a HIP runtime call failed; see vqhip_last_error()            */
    VQHIP_ERR_UNSUPPORTED   = -3,   /* format / parameter combination not implemented              */
    VQHIP_ERR_NO_DEVICE     = -4,   /* no gfx950 device visible — there is NO CPU fallback          */
    VQHIP_ERR_RCCL          = -5    /* RCCL could not be loaded or a collective call failed (row-tiled multi-GPU mode) */
} vqhip_status;

/* Storage formats of the reference render targets:
 *   scene colour / blur / env cubemaps : DXGI_FORMAT_R16G16B16A16_FLOAT  (RenderResources.cpp:40,144-161,221-243;
 *                                                                          EnvironmentMapRendering.cpp:32-53)
 *   SDR tonemapper output              : DXGI_FORMAT_R8G8B8A8_UNORM      (RenderResources.cpp:41,245-261)
 *   BRDF integration LUT               : DXGI_FORMAT_R16G16_FLOAT        (Renderer.cpp:1026-1032)
 *   HDRI equirect                      : DXGI_FORMAT_R32G32B32A32_FLOAT  (TextureManager.cpp:590-592)
 * RGBA32F / RG32F variants are offered for every output so parity can also be judged before the
 * storage rounding. fp32 -> fp16 is round-to-nearest-even, fp32 -> UNORM8 is trunc(sat(x)*255 + 0.5). */
typedef enum vqhip_format {
    VQHIP_FMT_RGBA32F     = 0,
    VQHIP_FMT_RGBA16F     = 1,
    VQHIP_FMT_RGBA8_UNORM = 2,
    VQHIP_FMT_RG16F       = 3,
    VQHIP_FMT_RG32F       = 4,
    VQHIP_FMT_R10G10B10A2_UNORM = 5,  /* Tex_SceneNormals (RenderResources.cpp:185-197): output of vqhip_scene_normals_from_materials, input of vqhip_ssr_environment_fallback */
    VQHIP_FMT_R11G11B10_FLOAT = 6     /* TexAverageRadiance of the reflection denoiser: one uint32 per texel, R bits 0-10, G 11-21, B 22-31; unsigned, 5-bit exponent (bias 15),
                                       * 6 / 6 / 5 mantissa bits, denormals / inf / NaN as DXGI; decoded exactly. Read by vqhip_ssr_prefilter, vqhip_ssr_resolve_temporal; written by vqhip_ssr_reproject */
} vqhip_format;

/* ------------------------------------------------------------------------------------------------
 * VQ_SHADER_DATA mirror  (Shaders/LightingConstantBufferData.h:39-186, Shaders/VQPlatform.h:21-41)
 * ---------------------------------------------------------------------------------------------- */
#define VQ_NUM_LIGHTS__POINT                 100   /* LightingConstantBufferData.h:39 */
#define VQ_NUM_LIGHTS__SPOT                  20    /* :40 */
#define VQ_NUM_SHADOWING_LIGHTS__POINT       5     /* :42 */
#define VQ_NUM_SHADOWING_LIGHTS__SPOT        5     /* :43 */
#define VQ_NUM_SHADOWING_LIGHTS__DIRECTIONAL 1     /* :44 */

typedef struct VQ_float2 { float x, y; } VQ_float2;
typedef struct VQ_float3 { float x, y, z; } VQ_float3;
typedef struct VQ_float4 { float x, y, z, w; } VQ_float4;
/* DirectX::XMMATRIX: 4 rows of 4 floats, 16-byte aligned, row-major on the CPU. HLSL reads a cbuffer
 * `matrix` column-major, so HLSL `mul(M, v)` == row-vector v * M_cpu  (SURVEY.md §8b). */
typedef struct VQ_matrix { VQHIP_ALIGNAS(16) float m[4][4]; } VQ_matrix;

typedef struct VQ_PointLight {          /* LightingConstantBufferData.h:50-61 */
    VQ_float3 position;    float range;
    VQ_float3 color;       float brightness;
    VQ_float3 attenuation; float depthBias;
} VQ_PointLight;

typedef struct VQ_SpotLight {           /* :63-78 (its "48 bytes" comment is wrong: 64) */
    VQ_float3 position;    float outerConeAngle;
    VQ_float3 color;       float brightness;
    VQ_float3 spotDir;     float depthBias;
    float innerConeAngle;  float range; float dummy1; float dummy2;
} VQ_SpotLight;

typedef struct VQ_DirectionalLight {    /* :80-90 */
    VQ_float3 lightDirection; float brightness;
    VQ_float3 color;          float depthBias;
    int32_t shadowing;        int32_t enabled;
} VQ_DirectionalLight;

typedef struct VQ_SceneLighting {       /* :92-109 */
    int32_t numPointLights, numSpotLights, numPointCasters, numSpotCasters;
    VQ_DirectionalLight directional;
    VQ_matrix     shadowViewDirectional;
    VQ_PointLight point_lights [VQ_NUM_LIGHTS__POINT];
    VQ_PointLight point_casters[VQ_NUM_SHADOWING_LIGHTS__POINT];
    VQ_SpotLight  spot_lights  [VQ_NUM_LIGHTS__SPOT];
    VQ_SpotLight  spot_casters [VQ_NUM_SHADOWING_LIGHTS__SPOT];
    VQ_matrix     shadowViews  [VQ_NUM_SHADOWING_LIGHTS__SPOT];
} VQ_SceneLighting;

typedef struct VQ_PerFrameData {        /* :164-172 ; filled at SceneRendering.cpp:429-450 */
    VQ_SceneLighting Lights;
    VQ_float2 f2PointLightShadowMapDimensions;
    VQ_float2 f2SpotLightShadowMapDimensions;
    VQ_float2 f2DirectionalLightShadowMapDimensions;
    float fAmbientLightingFactor;
    float fHDRIOffsetInRadians;
} VQ_PerFrameData;

typedef struct VQ_PerViewLightingData { /* :173-186 ; filled at SceneRendering.cpp:452-467 */
    VQ_matrix matView, matViewToWorld, matProjInverse;
    VQ_float4 WorldFrustumPlanes[6];
    VQ_float3 CameraPosition; float MaxEnvMapLODLevels;
    VQ_float2 ScreenDimensions;
    int32_t   EnvironmentMapDiffuseOnlyIllumination;
    float     pad1;
} VQ_PerViewLightingData;

typedef struct VQ_MaterialData {        /* :126-143 ; Material::GetCBufferData Material.h:120-127 */
    VQHIP_ALIGNAS(16) VQ_float3 diffuse; float alpha;
    VQ_float3 emissiveColor;  float emissiveIntensity;
    VQ_float3 specular;       float normalMapMipBias;
    VQ_float4 uvScaleOffset;
    float roughness, metalness, displacement, textureConfig;
} VQ_MaterialData;

/* Tonemapper.hlsl:98-104 cbuffer == first 16 bytes of FPostProcessParameters::FTonemapper
 * (Source/Engine/PostProcess/PostProcess.h:84-91). Enums: Source/Renderer/Rendering/HDR.h:78-95. */
typedef enum VQ_EColorSpace   { VQ_COLOR_SPACE_REC_709 = 0, VQ_COLOR_SPACE_REC_2020 = 1 } VQ_EColorSpace;
typedef enum VQ_EDisplayCurve { VQ_DISPLAY_CURVE_SRGB = 0, VQ_DISPLAY_CURVE_ST2084 = 1, VQ_DISPLAY_CURVE_LINEAR = 2 } VQ_EDisplayCurve;
typedef struct VQ_TonemapperParams {
    int32_t ContentColorSpaceEnum;            /* default REC_709 */
    int32_t OutputDisplayCurveEnum;           /* default sRGB    */
    float   DisplayReferenceBrightnessLevel;  /* default 200.0f  */
    int32_t ToggleGammaCorrection;            /* default 1       */
} VQ_TonemapperParams;

/* GaussianBlur.hlsl:65-68 cbuffer == FPostProcessParameters::FBlurParams (PostProcess.h:92-96). */
typedef struct VQ_BlurParams { int32_t iImageSizeX, iImageSizeY; } VQ_BlurParams;

VQHIP_STATIC_ASSERT(sizeof(VQ_PointLight) == 48, "PointLight");
VQHIP_STATIC_ASSERT(offsetof(VQ_PointLight, range) == 12 && offsetof(VQ_PointLight, color) == 16 &&
                    offsetof(VQ_PointLight, brightness) == 28 && offsetof(VQ_PointLight, attenuation) == 32 &&
                    offsetof(VQ_PointLight, depthBias) == 44, "PointLight offsets");
VQHIP_STATIC_ASSERT(sizeof(VQ_SpotLight) == 64, "SpotLight");
VQHIP_STATIC_ASSERT(offsetof(VQ_SpotLight, outerConeAngle) == 12 && offsetof(VQ_SpotLight, spotDir) == 32 &&
                    offsetof(VQ_SpotLight, depthBias) == 44 && offsetof(VQ_SpotLight, innerConeAngle) == 48 &&
                    offsetof(VQ_SpotLight, range) == 52, "SpotLight offsets");
VQHIP_STATIC_ASSERT(sizeof(VQ_DirectionalLight) == 40, "DirectionalLight");
VQHIP_STATIC_ASSERT(offsetof(VQ_DirectionalLight, shadowing) == 32 && offsetof(VQ_DirectionalLight, enabled) == 36, "DirectionalLight offsets");
VQHIP_STATIC_ASSERT(sizeof(VQ_SceneLighting) == 7088, "SceneLighting");
VQHIP_STATIC_ASSERT(offsetof(VQ_SceneLighting, directional) == 16 && offsetof(VQ_SceneLighting, shadowViewDirectional) == 64 &&
                    offsetof(VQ_SceneLighting, point_lights) == 128 && offsetof(VQ_SceneLighting, point_casters) == 4928 &&
                    offsetof(VQ_SceneLighting, spot_lights) == 5168 && offsetof(VQ_SceneLighting, spot_casters) == 6448 &&
                    offsetof(VQ_SceneLighting, shadowViews) == 6768, "SceneLighting offsets");
VQHIP_STATIC_ASSERT(sizeof(VQ_PerFrameData) == 7120, "PerFrameData");
VQHIP_STATIC_ASSERT(offsetof(VQ_PerFrameData, f2PointLightShadowMapDimensions) == 7088 &&
                    offsetof(VQ_PerFrameData, f2SpotLightShadowMapDimensions) == 7096 &&
                    offsetof(VQ_PerFrameData, f2DirectionalLightShadowMapDimensions) == 7104 &&
                    offsetof(VQ_PerFrameData, fAmbientLightingFactor) == 7112 &&
                    offsetof(VQ_PerFrameData, fHDRIOffsetInRadians) == 7116, "PerFrameData offsets");
VQHIP_STATIC_ASSERT(sizeof(VQ_PerViewLightingData) == 320, "PerViewLightingData");
VQHIP_STATIC_ASSERT(offsetof(VQ_PerViewLightingData, WorldFrustumPlanes) == 192 && offsetof(VQ_PerViewLightingData, CameraPosition) == 288 &&
                    offsetof(VQ_PerViewLightingData, MaxEnvMapLODLevels) == 300 && offsetof(VQ_PerViewLightingData, ScreenDimensions) == 304 &&
                    offsetof(VQ_PerViewLightingData, EnvironmentMapDiffuseOnlyIllumination) == 312, "PerViewLightingData offsets");
VQHIP_STATIC_ASSERT(sizeof(VQ_MaterialData) == 80, "MaterialData");
VQHIP_STATIC_ASSERT(offsetof(VQ_MaterialData, uvScaleOffset) == 48 && offsetof(VQ_MaterialData, roughness) == 64 &&
                    offsetof(VQ_MaterialData, textureConfig) == 76, "MaterialData offsets");
VQHIP_STATIC_ASSERT(sizeof(VQ_TonemapperParams) == 16, "TonemapperParams");
VQHIP_STATIC_ASSERT(sizeof(VQ_BlurParams) == 8, "BlurParams");

/* ------------------------------------------------------------------------------------------------
 * resource descriptors (replace the SRV tables bound at SceneRendering.cpp:1687-1717)
 * ---------------------------------------------------------------------------------------------- */

/* Image-based-lighting inputs of ForwardLighting.hlsl:93-95 (t10 texEnvMapDiff, t11 texEnvMapSpec,
 * t12 texBRDFIntegral). Layouts:
 *   diffuse_cube  : [6][diffuse_res][diffuse_res] RGBA16F (Tex_IrradianceDiffBlurred, 1 mip; EnvironmentMapRendering.cpp:32-43)
 *   specular_cube : mip-major, [mip][6][res>>mip][res>>mip] RGBA16F, densely packed, spec_mips levels
 *                   (Tex_IrradianceSpec; MIPS = CalculateMipLevelCount(res,res) - 1, EnvironmentMapRendering.cpp:55-63)
 *   brdf_lut      : [lut_size][lut_size] RG16F, u = NdotV along x, v = roughness along y (Renderer.cpp:1026-1032)
 * Face order +X,-X,+Y,-Y,+Z,-Z (CubemapUtility.h:26-36). */
typedef struct vqhip_envmap {
    const void* diffuse_cube;   int32_t diffuse_res;
    const void* specular_cube;  int32_t spec_res0;  int32_t spec_mips;
    const void* brdf_lut;       int32_t lut_size;
} vqhip_envmap;

/* Shadow maps of ForwardLighting.hlsl:97-99 as linear R32F arrays (depth targets are D32; point
 * casters store distance/far, Lighting.hlsl:161-163):
 *   directional : [dir_dim][dir_dim]                 (2048 in the reference, SceneRendering.cpp:441)
 *   spot        : [VQ_NUM_SHADOWING_LIGHTS__SPOT][spot_dim][spot_dim]      (1024, :440)
 *   point       : [VQ_NUM_SHADOWING_LIGHTS__POINT][6][point_dim][point_dim] (1024, :439)
 * Any pointer may be NULL when the matching caster count is 0 / directional.shadowing == 0. */
typedef struct vqhip_shadowmaps {
    const float* directional;  int32_t dir_dim;
    const float* spot;         int32_t spot_dim;
    const float* point;        int32_t point_dim;
} vqhip_shadowmaps;

/* Linear float4 G-buffer = the state of ForwardLighting.hlsl:PSMain at :284-293.
 * Four SoA planes of float4, row-major:
 *   gb0 = (P.xyz world position, ao)        ao = fAmbientLightingFactor*localAO*ssao   (:247,269,281)
 *   gb1 = (Surface.N.xyz raw (not renormalised), Surface.roughness)                     (:267,272-277)
 *   gb2 = (Surface.diffuseColor.rgb linear, Surface.metalness)                          (:249,253)
 *   gb3 = (Surface.emissiveColor.rgb, Surface.emissiveIntensity)                        (:250-251) */
typedef struct vqhip_gbuffer {
    const void* gb0; const void* gb1; const void* gb2; const void* gb3;
    int32_t width, height, row_pitch_px;
} vqhip_gbuffer;

/* Output of the load-time environment-map prefilter (FEnvironmentMapRenderingResources,
 * EnvironmentMapRendering.h:30-64): caller-allocated device buffers, same layouts as vqhip_envmap. */
typedef struct vqhip_envmap_out {
    void* diffuse_unblurred;    /* Tex_IrradianceDiff        [6][dres][dres] RGBA16F (optional, may be NULL) */
    void* diffuse_blurred;      /* Tex_IrradianceDiffBlurred [6][dres][dres] RGBA16F                          */
    void* blur_tmp;             /* Tex_BlurTemp              [dres][dres]    RGBA16F (scratch)                */
    void* specular;             /* Tex_IrradianceSpec        mip-major RGBA16F                                */
} vqhip_envmap_out;

/* ---- the G-buffer producer's inputs -------------------------------------------- */

/* One material texture = the reference's DXGI_FORMAT_R8G8B8A8_UNORM Texture2D with its full mip chain
 * (TextureManager.cpp:590; mips by VQ_DXGI_UTILS::MipImage's 4-byte branch, DXGIUtils.cpp:264-285).
 * texels : device pointer, level 0 first, levels densely packed, `mips` levels, level l is
 *          max(1,width>>l) x max(1,height>>l). NULL == the null SRV bound for a missing map
 *          (Renderer_Resources.cpp:385-387): every sample returns 0. */
typedef struct vqhip_texture2d {
    const void* texels;
    int32_t width, height, mips, reserved;   /* reserved: 0, except vqhip_material.texDiffuse.reserved = material flags (below) */
} vqhip_texture2d;
/* vqhip_material.texDiffuse.reserved bit 0: the material is drawn with the "_AlphaMasked" PSO permutation, i.e. PSMain compiled with
 * ENABLE_ALPHA_MASK (PipelineStateObjects.cpp:1477,1571) — chosen by Material::IsAlphaMasked (Material.cpp:39: an alpha-mask map is
 * bound, or the diffuse map uses its alpha channel). Then `if (HasDiffuseMap(TEX_CFG) && AlbedoAlpha.a < 0.01f) discard;`
 * (ForwardLighting.hlsl:237-240): vqhip_gbuffer_from_materials gives such a pixel an all-zero record AND rewrites its material index in
 * ip2.w to -1 (in place), so that it reads as "no geometry" to vqhip_skydome / vqhip_unlit_composite, like a discarded fragment. */
#define VQHIP_MATERIAL_ALPHA_MASKED 1

/* cbPerObject.materialData + the descriptor table t0..t7 of ForwardLighting.hlsl:84-92 that
 * AssetLoader.cpp:406-420 fills per material (t3 texAlphaMask and t8 texHeightmap are not read by
 * the non-tessellated, non-alpha-masked PSMain and are omitted). */
typedef struct vqhip_material {
    VQ_MaterialData data;
    vqhip_texture2d texDiffuse;         /* t0 */
    vqhip_texture2d texNormals;         /* t1 */
    vqhip_texture2d texEmissive;        /* t2 */
    vqhip_texture2d texMetalness;       /* t4 */
    vqhip_texture2d texRoughness;       /* t5 */
    vqhip_texture2d texOcclRoughMetal;  /* t6 */
    vqhip_texture2d texLocalAO;         /* t7 */
} vqhip_material;

VQHIP_STATIC_ASSERT(sizeof(vqhip_texture2d) == 24, "vqhip_texture2d");
VQHIP_STATIC_ASSERT(sizeof(vqhip_material) == 256 && offsetof(vqhip_material, texDiffuse) == 80 &&
                    offsetof(vqhip_material, texLocalAO) == 224, "vqhip_material");

/* The rasteriser's output that PSMain consumes (struct PSInput, ForwardLighting.hlsl:42-53), one record
 * per pixel in three SoA float4 planes (device pointers, row_pitch_px pixels per row):
 *   ip0 = (WorldSpacePosition.xyz, uv.x)
 *   ip1 = (WorldSpaceNormal.xyz,   uv.y)
 *   ip2 = (WorldSpaceTangent.xyz,  asfloat(int32 materialIndex))   materialIndex < 0: no geometry
 * SV_POSITION.xy is implied: (x + 0.5, y + 0.5). vqhip_scene_interpolants produces these planes from
 * meshes and the owner plane of vqhip_scene_depth (a visibility-buffer resolve); a caller with a
 * rasteriser of its own may hand over its planes instead. */
typedef struct vqhip_interpolants {
    const void* ip0; const void* ip1; const void* ip2;
    int32_t width, height, row_pitch_px;
} vqhip_interpolants;

/* texScreenSpaceAO (t9): R8_UNORM [height][width] (RenderResources.cpp:358-371) — the plane vqhip_cacao writes (FidelityFX CACAO, below) —, or NULL when
 * SSAO is off (the reference then clears the target to 1.0, SceneRendering.cpp:1543-1553). */
typedef struct vqhip_ssao {
    const void* texels; int32_t width, height;
} vqhip_ssao;

typedef struct vqhip_ctx vqhip_ctx;

/* summation order of the convolution integrals (DESIGN.md "Convolution order"):
 *   SEQUENTIAL : every texel's taps are accumulated in the HLSL loop order (CubemapConvolution.hlsl:132-159,183-219): the
 *                reference's result. Default. The taps are evaluated wave-parallel and parked in LDS; one lane per (texel,
 *                channel) adds them in order (conv.hip:k_conv_diffuse_ordered / k_conv_specular_ordered).
 *   WAVE64     : one 64-lane wave per texel; lane l accumulates taps l, l+64, ... in order, then a fixed
 *                xor-butterfly (32,16,8,4,2,1) combines the 64 partial sums: a better-conditioned sum that is up to 2 RGBA16F
 *                ulps from the reference's on BASELINE config 4, 1.26 x faster for the diffuse integral. The oracle implements both. */
typedef enum vqhip_conv_order { VQHIP_CONV_SEQUENTIAL = 0, VQHIP_CONV_WAVE64 = 1 } vqhip_conv_order;

/* ------------------------------------------------------------------------------------------------
 * entry points
 * ---------------------------------------------------------------------------------------------- */

/* Replaces VQRenderer::Initialize device/queue creation (Source/Renderer/Renderer.cpp:204) for this path:
 * binds the context to HIP device `device_ordinal`. Fails with VQHIP_ERR_NO_DEVICE when no GPU is visible. */
VQHIP_API int  vqhip_create(int device_ordinal, vqhip_ctx** out_ctx);
VQHIP_API void vqhip_destroy(vqhip_ctx* ctx);
VQHIP_API const char* vqhip_last_error(const vqhip_ctx* ctx);   /* ctx may be NULL: process-wide last error */
VQHIP_API int  vqhip_abi_version(void);                          /* == VQHIP_ABI_VERSION */

/* How pow(1 - cos, 5.0) of the three Fresnel terms (BRDF.hlsl:135, :155, :274) is evaluated by vqhip_forward_lighting and
 * vqhip_brdf_lut issued through this context (contract v4):
 *   VQHIP_FRESNEL_POW_PRODUCT   (default) x*((x*x)*(x*x)) — FXC's / DXC -Gec's mul-only pattern: 21 % fewer instructions in the
 *                               light loop, finite where dot(H,V) rounds a hair above 1;
 *   VQHIP_FRESNEL_POW_EXP2_LOG2 exp2(5*log2(x)) — what DXC emits with the engine's own flags (no -Gec): NaN for a negative base,
 *                               values within ~3 binary32 ulps of the product elsewhere (the contract of rounds v1-v3). */
typedef enum vqhip_fresnel_pow { VQHIP_FRESNEL_POW_PRODUCT = 0, VQHIP_FRESNEL_POW_EXP2_LOG2 = 1 } vqhip_fresnel_pow;
VQHIP_API int  vqhip_set_fresnel_pow(vqhip_ctx* ctx, vqhip_fresnel_pow mode);
/* The READING of the HLSL intrinsics whose lowering the source does not fix — dot, normalize, length, reflect — in every later
 * vqhip_forward_lighting / vqhip_gbuffer_from_materials / vqhip_forward_lighting_from_materials / vqhip_ssr_environment_fallback through this context
 * (the reference's own HLSL is built in both readings: oracle/ref_src/hlsl_shim.h):
 *   VQHIP_ARITH_LITERAL (default) products and sums rounded one by one, left to right; normalize(v) = v / length(v), one IEEE quotient per component;
 *   VQHIP_ARITH_DXC     what DXC's HLOperationLower emits (Source/Renderer/Pipeline/ShaderCompileUtils.cpp:53-56 selects no flag that changes it): DXIL Dot3 as
 *                       the FMA chain fma(az,bz, fma(ay,by, ax*bx)), normalize(v) = v * Rsqrt(dot(v,v)) with a correctly rounded rsqrt, length = sqrt of that dot.
 * Together with VQHIP_FRESNEL_POW_EXP2_LOG2 this is the second build of the reference's sources (tests/golden/ref_outputs_dxc.npz): each mode is within one
 * RGBA16F ulp of ITS reading; the two readings lie up to 15 ulps apart on highlight pixels. A maintainer who calibrates against D3D12 WARP
 * (docs/WARP_CALIBRATION.md) selects whichever WARP turns out to follow. */
/* Tuning / A-B options of a context, read by the launchers at call time (never from the process environment: getenv racing a host setenv is
 * undefined behaviour, and VQEngine records on many threads, SceneRendering.cpp:563-706). value NULL, "" or "default" restores the default. Every
 * form selected here gives the bits of the default form (tests/test_gpu_conv_forms.py, tests/test_gpu_round3.py; psmain_waves and shade_wg in every instantiation of their
 * kernels: tests/test_gpu_psmain_variants.py); unknown keys / values: VQHIP_ERR_INVALID_ARG.
 *   shade_wg 64|128|256 · psmain_waves 4|5|6 · blur_y_wgs n · msaa_edge_wgs n · post_form two|chain · post_strips n · lut_form general ·
 *   specular_form general · diffuse_form records|texels|general · diffuse_seq_form ordered|lane · raster_tile 32|64 · interp_form lane|wave
 * (the non-default values are the general / fallback forms of the same kernels; the measured-and-rejected kernel forms of rounds 2-5 — the compact tonemap
 * tables, the per-sample LUT and per-mip specular kernels, the persistent X pass, the rolling-ring Y pass — are not in the library: docs/HISTORY.md).
 * shade_wg sets the lanes per workgroup of vqhip_forward_lighting and of the first kernel of vqhip_forward_lighting_msaa (default: 64 below 4 Mi pixels, else 256);
 * msaa_edge_wgs the number of 256-lane workgroups of the persistent edge kernel of vqhip_forward_lighting_msaa (default: as many as fill every CU once; a
 * larger n is clamped to one lane per pixel and to 65536; the kernel walks the edge list whatever its length — tests/test_gpu_msaa_edges.py).
 * psmain_waves applies to the literal reading only (the DXC-reading instantiation of the fused PSMain kernel has one register cap). post_form: "two" = vqhip_post_process[_tile] always runs blur X, then blur Y + tonemap (two kernels); "chain" = the one-kernel chain whatever the frame size
 * (default: the chain for RGBA16F -> RGBA8 frames of >= 2^20 pixels and a per-channel display curve, the two kernels otherwise). */
VQHIP_API int  vqhip_set_option(vqhip_ctx* ctx, const char* key, const char* value);
typedef enum vqhip_arithmetic { VQHIP_ARITH_LITERAL = 0, VQHIP_ARITH_DXC = 1 } vqhip_arithmetic;
VQHIP_API int  vqhip_set_arithmetic(vqhip_ctx* ctx, vqhip_arithmetic mode);
#define VQHIP_ABI_VERSION 3   /* 3 (round 5): + vqhip_post_process_tile; options blur_x_wgs / blur_y_form / blur_y_rows removed, post_form / post_strips added.
                               * 2 (round 4): + vqhip_set_arithmetic, vqhip_set_option, vqhip_ssr_environment_fallback, VQHIP_FMT_R10G10B10A2_UNORM; conv order default SEQUENTIAL;
                               * later in round 4, additions only: vqhip_forward_lighting_mrt, vqhip_forward_lighting_from_materials_mrt, vqhip_scene_normals_from_materials,
                               * vqhip_composite_reflections; vqhip_visualize reads R10G10B10A2 / RG16F / RG32F inputs.
                               * Later additions to 3: vqhip_gbuffer_msaa, vqhip_forward_lighting_msaa; vqhip_msaa_surfaces, vqhip_msaa_resolve_surfaces, vqhip_depth_hierarchy (+ _bytes, _level_offset_bytes);
                               * vqhip_ssr_classify, vqhip_ssr_intersect; vqhip_ssr_prefilter, vqhip_ssr_resolve_temporal, VQHIP_FMT_R11G11B10_FLOAT; vqhip_ssr_reproject, vqhip_ssr_reproject_surfaces;
                               * VQ_CacaoConstants, vqhip_cacao (+ _work_bytes, _plane_offset_bytes); vqhip_adaptive_cacao (+ _work_bytes, _plane_offset_bytes) and three plane ids;
                               * vqhip_shadow_depth (+ _work_bytes), vqhip_shadow_mesh / _draw / _view, VQHIP_CULL_*, option raster_tile;
                               * vqhip_scene_depth (+ _work_bytes), vqhip_scene_depth_draw / _targets;
                               * vqhip_scene_interpolants (+ _work_bytes), vqhip_scene_surface_draw, vqhip_scene_interpolant_targets, option interp_form;
                               * vqhip_scene_masked_depth, vqhip_shadow_masked_depth (+ _work_bytes), vqhip_scene_masked_depth_draw, vqhip_shadow_masked_draw / _view;
                               * vqhip_scene_quad_interpolants and the three _quad producers, vqhip_scene_quad_targets;
                               * vqhip_object_ids (+ _work_bytes), vqhip_object_id_draw; vqhip_outline (+ _work_bytes), VQ_OutlineData, vqhip_outline_draw / _targets;
                               * vqhip_displace_meshes, vqhip_displace_job, VQHIP_DISPLACE_MAX_JOBS;
                               * vqhip_unlit_draws (+ _work_bytes), VQ_UnlitData, vqhip_unlit_draw / _targets, VQHIP_UNLIT_QUEUE_CAPACITY;
                               * vqhip_line_draws (+ _work_bytes), vqhip_line_kind, VQ_VertexAxesData, vqhip_line_draw, VQHIP_LINES_MAX_INSTANCES */

/* Replaces VQRenderer::RenderSceneColor's lit draw loop (SceneRendering.cpp:1619-1785, hot part :1730-1784)
 * == ForwardLighting.hlsl:PSMain :289-380 evaluated for every pixel of the G-buffer.
 *   perFrame / perView : the cbuffers b0 / b1 of ForwardLighting.hlsl:76-77.
 *   extraPoint[numExtraPoint] : extension — point lights beyond the 100-slot cbuffer array (BASELINE cfg5);
 *                               accumulated right after point_lights[0..numPointLights) in index order.
 *   env  : NULL => NullCubemap / NullTex2D path (SceneRendering.cpp:1698-1709): IBL contributes 0.
 *   sm   : NULL allowed iff numPointCasters == numSpotCasters == 0 and !directional.shadowing.
 *   out  : float4(I_total, roughness) per pixel (ForwardLighting.hlsl:380), outFmt RGBA16F (reference RT0,
 *          PipelineStateObjects.cpp:1454) or RGBA32F; out_row_pitch_px pixels per row. */
VQHIP_API int vqhip_forward_lighting(vqhip_ctx* ctx, void* stream,
        const vqhip_gbuffer* gbuf,
        const VQ_PerFrameData* perFrame, const VQ_PerViewLightingData* perView,
        const VQ_PointLight* extraPoint, int numExtraPoint,
        const vqhip_envmap* env, const vqhip_shadowmaps* sm,
        void* out, int out_row_pitch_px, vqhip_format outFmt);

/* The other render targets of the same draw: the PSO permutations OUTPUT_ALBEDO / OUTPUT_MOTION_VECTORS of ForwardLighting.hlsl
 * (PipelineStateObjects.cpp:1499-1504,1547-1563; PSOutput :57-68; written at :382-389; bound by RenderSceneColor, SceneRendering.cpp:1647-1680):
 *   albedo_metallic : SV_TARGET1 = float4(Surface.diffuseColor, Surface.metalness) (:383) — Tex_SceneVisualization, RGBA16F (RenderResources.cpp:171-175)
 *                     | RGBA32F; NULL = the permutation without OUTPUT_ALBEDO
 *   motion_vectors  : float2(svPositionCurr.xy / svPositionCurr.w - svPositionPrev.xy / svPositionPrev.w) (:387) — Tex_SceneMotionVectors, RG16F
 *                     (RenderResources.cpp:178-182) | RG32F; NULL = the permutation without OUTPUT_MOTION_VECTORS
 *   svPositionCurr / svPositionPrev : two more planes of the rasteriser's output (PSInput :49-52, TEXCOORD1 / TEXCOORD2): the interpolated clip-space
 *                     positions mul(matWorldViewProj, v) and mul(matWorldViewProjPrev, v) of TransformVertex :172-185, float4 per pixel, sv_pitch_px
 *                     pixels per row (0 = width). Required iff motion_vectors is set.
 * Every pixel of the frame is written from the planes as given (a rasteriser leaves uncovered pixels at the clear value: give them equal
 * positions with w = 1, or composite afterwards). Device pointers; pitches in pixels (0 = width). */
typedef struct vqhip_psmain_targets {
    void*       albedo_metallic;  vqhip_format albedo_fmt;  int32_t albedo_pitch_px;
    void*       motion_vectors;   vqhip_format motion_fmt;  int32_t motion_pitch_px;
    const void* svPositionCurr;   const void*  svPositionPrev;  int32_t sv_pitch_px;  int32_t pad_;
} vqhip_psmain_targets;
VQHIP_STATIC_ASSERT(sizeof(vqhip_psmain_targets) == 56, "vqhip_psmain_targets");

/* vqhip_forward_lighting + the extra targets, in the same kernel (the G-buffer record is in registers: + 8 B/pixel written for SV_TARGET1,
 * + 32 B read and 4 B written per pixel for the motion vectors). targets == NULL or both outputs NULL: exactly vqhip_forward_lighting. */
VQHIP_API int vqhip_forward_lighting_mrt(vqhip_ctx* ctx, void* stream,
        const vqhip_gbuffer* gb,
        const VQ_PerFrameData* perFrame, const VQ_PerViewLightingData* perView,
        const VQ_PointLight* extraPoint, int numExtraPoint,
        const vqhip_envmap* env, const vqhip_shadowmaps* sm,
        void* out, int out_row_pitch_px, vqhip_format outFmt, const vqhip_psmain_targets* targets);

/* ---- 4x MSAA scene colour (docs/DESIGN_DETAILS.md §7.9) -----------------------------------------------------------------
 * Replaces the bMSAA branch of RenderSceneColor (the lit draw into the 4-sample Tex_SceneColorMSAA, MSAA_SAMPLE_COUNT = 4,
 * RenderResources.h:26, RenderResources.cpp:114-130, targets picked at SceneRendering.cpp:1644-1650) AND VQRenderer::ResolveMSAA's
 * ResolveSubresource of that target (SceneRendering.cpp:2060-2112): PSMain declares no sample / centroid inputs, so it runs once per
 * (pixel, primitive) and its result goes to every sample the primitive covers. The caller supplies up to 4 fragment layers:
 *   layer[k]    : a full vqhip_gbuffer (same planes and meaning as vqhip_forward_lighting; same width / height in every used layer,
 *                 own row_pitch_px each)
 *   coverage[k] : uint8 [height][coverage_pitch]; bit s (0..3) = "the fragment of layer k covers sample s" (D3D's standard 4x pattern),
 *                 bits 4-7 ignored. Any masks are valid: sample s is owned by the LOWEST layer k < layers whose mask has bit s, else it is
 *                 background. A layer that owns no sample of a pixel is not shaded there (its record may hold anything, NaN included).
 * Sample value: owned = shade_pixel(record of the owner) stored in outFmt (RGBA16F RNE | RGBA32F); background = background[p] (a plane in
 * outFmt, background_pitch_px pixels per row, e.g. the skydome drawn into it; must not be `out`) or (0,0,0,0) when background == NULL
 * (the clear value, SceneRendering.cpp:1660-1669). Resolve per channel: r = (((s0 + s1) + s2) + s3) * 0.25f in binary32 with the samples
 * widened from outFmt, stored to outFmt (RNE for RGBA16F); NaN / Inf propagate. A pixel whose four samples share one owner therefore holds
 * exactly the RGBA16F bits vqhip_forward_lighting writes for that record. Pitches in pixels; coverage_pitch in bytes (0 = width).
 * vqhip_set_arithmetic / vqhip_set_fresnel_pow apply as for vqhip_forward_lighting. The context keeps an edge-pixel list of 4 + 4*width*height
 * bytes (grown on demand: a growth waits for the device); calls on different streams are ordered on it by an event, nothing else synchronises. */
#define VQHIP_MSAA_MAX_LAYERS 4
typedef struct vqhip_gbuffer_msaa {
    vqhip_gbuffer  layer[VQHIP_MSAA_MAX_LAYERS];     /* same width / height in every used layer; own row_pitch_px each */
    const uint8_t* coverage[VQHIP_MSAA_MAX_LAYERS];  /* [height][coverage_pitch] sample masks, bit s = sample s */
    int32_t        layers;                           /* 1..4; entries >= layers are ignored */
    int32_t        coverage_pitch;                   /* bytes per row, 0 = width */
} vqhip_gbuffer_msaa;
VQHIP_STATIC_ASSERT(sizeof(vqhip_gbuffer) == 48, "vqhip_gbuffer");
VQHIP_STATIC_ASSERT(sizeof(vqhip_gbuffer_msaa) == 232 && offsetof(vqhip_gbuffer_msaa, coverage) == 192 &&
                    offsetof(vqhip_gbuffer_msaa, layers) == 224 && offsetof(vqhip_gbuffer_msaa, coverage_pitch) == 228, "vqhip_gbuffer_msaa layout");
VQHIP_API int vqhip_forward_lighting_msaa(vqhip_ctx* ctx, void* stream, const vqhip_gbuffer_msaa* gb,
        const VQ_PerFrameData* perFrame, const VQ_PerViewLightingData* perView,
        const VQ_PointLight* extraPoint, int numExtraPoint,
        const vqhip_envmap* env, const vqhip_shadowmaps* sm,
        const void* background, int background_pitch_px,      /* NULL = clear value 0 */
        void* out, int out_row_pitch_px, vqhip_format outFmt);  /* RGBA16F | RGBA32F */

/* ---- 4x MSAA depth / normals / roughness resolve and the depth hierarchy (docs/DESIGN_DETAILS.md §7.10) -------------------
 * vqhip_msaa_resolve_surfaces replaces DepthMSAAResolvePass (Shaders/DepthResolve.hlsl:CSMain :36-100; VQRenderer::ResolveMSAA_DepthPrePass,
 * SceneRendering.cpp:1455-1471, called at :484-487; the OUTPUT_ROUGHNESS permutation: call site :2115-2147): from the 4-sample depth and the 4-sample
 * packed normals, Tex_SceneDepthResolve and Tex_SceneNormals — the `depth` and `normals` arguments of vqhip_ssr_environment_fallback — and the roughness
 * of the nearest sample into the alpha of the resolved scene colour (its `sceneColorRoughness` argument). Inputs, in the representation of
 * vqhip_forward_lighting_msaa (layers + coverage masks, same ownership rule: the lowest layer whose mask has bit s owns sample s, no owner = background):
 *   depth_ms     : float [height][depth_pitch_px][4], 16-byte aligned — the Texture2DMS<float> depth, sample s of a pixel at [..][s]; NDC z, far plane /
 *                  clear value 1. vqhip_scene_depth produces it (samples 4); a caller's own rasteriser may hand over its z instead.
 *   coverage[k]  : as vqhip_gbuffer_msaa; read only when outNormals or sceneColor is given
 *   normals[k]   : layer k's pre-pass normals == what vqhip_scene_normals_from_materials writes for that layer's interpolants, normals_fmt
 *                  R10G10B10A2_UNORM | RGBA32F (one format for all layers), normals_pitch_px[k] pixels per row. A background sample reads the clear value 0.
 *                  Read only when outNormals is given.
 *   roughness[k] : layer k's gb1 plane (float4 per pixel, .w = roughness), roughness_pitch_px[k]; background: the scene colour's background plane (its alpha is a
 *                  background sample's alpha; NULL = 0) — the two things vqhip_forward_lighting_msaa was given. Read only when sceneColor is given.
 * Outputs, each optional, at least one required (every one NULL: VQHIP_ERR_INVALID_ARG — the permutation the reference refuses to compile):
 *   outDepth     : R32F. min(min(min(s0, s1), s2), s3) in binary32 (`half` in that shader is float: the PSO is built without 16-bit types). min is fminf: a NaN
 *                  sample is dropped, which of +0 / -0 wins is not specified; the tested domain is finite depth in [0, 1].
 *   outNormals   : R10G10B10A2_UNORM | RGBA32F. Each sample's rgb (UNORM10: c / 1023 correctly rounded) * 2 - 1, summed left to right ((N0 + N1) + N2) + N3,
 *                  * 0.25, normalize in the reading vqhip_set_arithmetic selects, (+ 1) * 0.5, stored like vqhip_scene_normals_from_materials
 *                  (trunc(saturate(c) * 1023 + 0.5)). A zero sum normalises to NaN: the UNORM store writes code 0 in all three channels (saturate(NaN) = 0), the
 *                  RGBA32F store the NaN. The shader writes a float3 to a four-channel UAV — alpha undefined in the reference: 1 is written (alpha bits 3).
 *   sceneColor   : RGBA16F | RGBA32F, IN PLACE: alpha := the alpha the 4-sample colour target holds at sample iSample — an owned sample: gb1.w of the owner's
 *                  record stored in sceneFmt (what vqhip_forward_lighting writes), a background sample: the background's alpha. rgb is not touched.
 *                  iSample starts at 0, then `if (minDepth == s1) iSample = 1; .. s2 ..; .. s3 ..`: on a tie the HIGHEST equal index wins (:59-62).
 *   hierarchy    : the buffer of vqhip_depth_hierarchy (flags as there). The resolved depth is then not written and re-read: the hierarchy kernel takes "min of
 *                  the pixel's four samples" as its level-0 load — resolve + level 0 + levels 1-6 in one launch, 16 B/px in. outDepth may be NULL (level 0 IS the
 *                  resolved depth); outNormals / sceneColor of the same call run as the per-pixel kernel on the same stream.
 * An output must not alias an input. Pitches in pixels, 0 = width; coverage_pitch in bytes, 0 = width. 4 samples only (DepthMSAAResolve.cpp:73). */
typedef struct vqhip_msaa_surfaces {
    const float*   depth_ms;
    const uint8_t* coverage[VQHIP_MSAA_MAX_LAYERS];
    const void*    normals[VQHIP_MSAA_MAX_LAYERS];
    const void*    roughness[VQHIP_MSAA_MAX_LAYERS];
    const void*    background;
    int32_t        normals_pitch_px[VQHIP_MSAA_MAX_LAYERS];
    int32_t        roughness_pitch_px[VQHIP_MSAA_MAX_LAYERS];
    int32_t        width, height;
    int32_t        layers;                             /* 1..4 */
    int32_t        coverage_pitch;
    int32_t        depth_pitch_px, background_pitch_px;
    int32_t        normals_fmt;                        /* vqhip_format: R10G10B10A2_UNORM | RGBA32F */
    int32_t        pad_;
} vqhip_msaa_surfaces;
VQHIP_STATIC_ASSERT(sizeof(vqhip_msaa_surfaces) == 176 && offsetof(vqhip_msaa_surfaces, coverage) == 8 && offsetof(vqhip_msaa_surfaces, normals) == 40 &&
                    offsetof(vqhip_msaa_surfaces, roughness) == 72 && offsetof(vqhip_msaa_surfaces, background) == 104 &&
                    offsetof(vqhip_msaa_surfaces, normals_pitch_px) == 112 && offsetof(vqhip_msaa_surfaces, roughness_pitch_px) == 128 &&
                    offsetof(vqhip_msaa_surfaces, width) == 144 && offsetof(vqhip_msaa_surfaces, layers) == 152 &&
                    offsetof(vqhip_msaa_surfaces, depth_pitch_px) == 160 && offsetof(vqhip_msaa_surfaces, normals_fmt) == 168, "vqhip_msaa_surfaces layout");
VQHIP_API int vqhip_msaa_resolve_surfaces(vqhip_ctx* ctx, void* stream, const vqhip_msaa_surfaces* in,
        float* outDepth, int outDepthPitchPx,
        void* outNormals, vqhip_format outNormalsFmt, int outNormalsPitchPx,
        void* sceneColor, vqhip_format sceneFmt, int scenePitchPx,
        float* hierarchy, unsigned flags);

/* Replaces VQRenderer::DownsampleDepth (SceneRendering.cpp:2151-2183, called at :496-499; Shaders/DownsampleDepth.hlsl + FidelityFX SPD): the min-depth pyramid
 * Tex_DownsampledSceneDepth (R32F, full chain, RenderResources.cpp:95-112) of a single-sample depth plane (MSAA off; an MSAA frame passes `hierarchy` to
 * vqhip_msaa_resolve_surfaces instead). Writes all L = vqhip_mip_level_count(width, height) levels into `mips`: level 0 first, levels densely packed, level l is
 * max(1, width >> l) x max(1, height >> l) floats (the convention of vqhip_mip_chain_min_rgba32f); vqhip_depth_hierarchy_bytes sizes the buffer.
 *   level 0      = a copy of `depth` (depth_pitch_px floats per row, 0 = width);
 *   level l >= 1 : texel (x, y) = min(min(a, b), min(c, d)) over level l-1 at (2x, 2y), (2x+1, 2y), (2x, 2y+1), (2x+1, 2y+1), where a coordinate outside level l-1
 *                  reads 0.0 (D3D's out-of-bounds typed load): with floor-halved sizes that happens once one dimension has been clamped to 1 and the other has not
 *                  (1280 x 720: level 9 is 2 x 1, so level 10 = 0);
 *   the 1 x 1 top level, default: min(top, 0.0) whenever L <= 12 — the reference hands SPD its number of LEVELS as the number of reductions, and the surplus
 *                  reduction (the top texel and three out-of-extent neighbours) lands on the last subresource (DownsampleDepth.hlsl:82-85,105;
 *                  RenderResources.cpp:110-111). That is what the reference's SSR reads.
 *   flags & VQHIP_DEPTH_HIERARCHY_TRUE_TOP : the 1 x 1 top level holds the minimum over all of level 0 instead (for culling); nothing else changes.
 * This reading of the out-of-bounds and top-level behaviour comes from the sources and is NOT yet confirmed against a D3D12 run (docs/WARP_CALIBRATION.md).
 * max(width, height) > 4096: VQHIP_ERR_UNSUPPORTED (the reference's SPD instance covers 12 reductions; above that it produces no pyramid — BASELINE cfg5's
 * 7680 x 4320 frame is out of range). Two kernel launches (levels 0-6 per 64 x 64 tile, then levels 7+ by one workgroup), one for frames of <= 64 x 64. TRUE_TOP
 * keeps 16 KiB of per-tile minima in the context; calls on different streams are ordered on it by an event. `mips` must not overlap `depth`. */
#define VQHIP_DEPTH_HIERARCHY_TRUE_TOP 1u
#define VQHIP_DEPTH_HIERARCHY_MAX_DIM  4096
VQHIP_API size_t vqhip_depth_hierarchy_bytes(int width, int height);
VQHIP_API size_t vqhip_depth_hierarchy_level_offset_bytes(int width, int height, int level);
VQHIP_API int    vqhip_depth_hierarchy(vqhip_ctx* ctx, void* stream, const float* depth, int depth_pitch_px, int width, int height,
        float* mips, unsigned flags);

/* Replaces the GaussianBlur.hlsl CSMain_X / CSMain_Y dispatches (EnvironmentMapRendering.cpp:279-373,
 * SceneRendering.cpp:2582-2638): 21-tap separable Gaussian, clamp-to-edge, alpha := 1.
 * fmt (RGBA16F = reference, or RGBA32F) applies to in, tmp and out alike; the intermediate is rounded
 * to `fmt` between the passes exactly like the reference's Tex_BlurTemp / BlurIntermediate. */
VQHIP_API int vqhip_gaussian_blur(vqhip_ctx* ctx, void* stream, const void* in, void* tmp, void* out,
        const VQ_BlurParams* params, vqhip_format fmt);
VQHIP_API int vqhip_gaussian_blur_x(vqhip_ctx* ctx, void* stream, const void* in, void* out,
        const VQ_BlurParams* params, vqhip_format fmt);
/* Y pass over a row tile. halo_top = the `halo_rows` rows just above row 0 of `in` (row -halo_rows first),
 * halo_bottom = the rows just below the tile; NULL => that side is the image border (clamp).
 * halo_rows must be 0 (both NULL) or >= 10 (= KERNEL_RANGE-1, GaussianBlur.hlsl:54-55). Used by the
 * row-tiled multi-GPU mode where neighbours exchange X-blurred rows over RCCL. */
VQHIP_API int vqhip_gaussian_blur_y(vqhip_ctx* ctx, void* stream, const void* in, void* out,
        const void* halo_top, const void* halo_bottom, int halo_rows,
        const VQ_BlurParams* params, vqhip_format fmt);

/* Fused form of the last two dispatches of the post chain when the blur is enabled: CSMain_Y (GaussianBlur.hlsl:155-187,
 * SceneRendering.cpp:2613-2638) immediately followed by Tonemapper.hlsl:CSMain (:2640-2656). The blurred value is rounded
 * to `blurFmt` exactly as if it had been stored to BlurOutput and re-read, then tonemapped in registers: identical bits to
 * vqhip_gaussian_blur_y + vqhip_tonemap, one image round trip through HBM less. */
VQHIP_API int vqhip_gaussian_blur_y_tonemap(vqhip_ctx* ctx, void* stream, const void* in, void* out,
        const void* halo_top, const void* halo_bottom, int halo_rows,
        const VQ_BlurParams* blurParams, const VQ_TonemapperParams* tonemapParams, vqhip_format blurFmt, vqhip_format outFmt);

/* Replaces the Tonemapper.hlsl:CSMain dispatch (SceneRendering.cpp:2640-2656).
 * inFmt RGBA16F|RGBA32F; outFmt RGBA8_UNORM (SDR swapchain path) | RGBA16F (HDR path) | RGBA32F.
 * Table cache: the calls that tonemap through a 65 536-entry table (this one, vqhip_gaussian_blur_y_tonemap, vqhip_post_process; RGBA16F input, a curve that
 * does not mix channels) keep the tables of the FOUR most recent (parameters, output format) sets in the context. A fifth set rebuilds the least recently used
 * table on the calling stream, behind an event recorded after that table's last reader — no host wait, legal under stream capture — unless the table has been
 * read from more than one stream: then the call waits for the whole device once (hipDeviceSynchronize: a host stall, and an error under stream capture).
 * An application that animates tonemapper parameters from several streams should serialise those calls on one stream. */
VQHIP_API int vqhip_tonemap(vqhip_ctx* ctx, void* stream, const void* in, void* out, int width, int height,
        const VQ_TonemapperParams* params, vqhip_format inFmt, vqhip_format outFmt);

/* Replaces the blur + tonemapper part of VQRenderer::RenderPostProcess as ONE call (SceneRendering.cpp:2579-2656: "BlurCS" { CSMain_X, CSMain_Y }
 * when bEnableGaussianBlur, then "TonemapperCS"): sceneColor -> out. BlurIntermediate lives in a scratch buffer of the context; for the
 * reference's formats (RGBA16F scene colour, RGBA8 SDR target) and a display curve that does not mix channels (sRGB, LINEAR, ST2084 on Rec.2020
 * content) the Y pass and the tonemapper are one kernel and BlurOutput never exists; for frames of >= 2^20 pixels the X pass joins them (k_post_chain: 8 B read +
 * 4 B written per pixel, BlurIntermediate never exists either). Identical bits to vqhip_gaussian_blur_x -> _y ->
 * vqhip_tonemap (the intermediate roundings to the blur format are reproduced). enableGaussianBlur == 0: the tonemapper alone. */
VQHIP_API int vqhip_post_process(vqhip_ctx* ctx, void* stream, const void* sceneColor, void* out, int width, int height,
        const VQ_TonemapperParams* tonemapParams, int enableGaussianBlur, vqhip_format inFmt, vqhip_format outFmt);
/* The same chain (blur enabled) over ONE ROW TILE of a frame that is split between GPUs. halo_top = the `halo_rows` SCENE-COLOUR rows just above
 * row 0 of `sceneColor` (row -halo_rows first), halo_bottom = the rows just below the tile, in `inFmt`; NULL => that side is the image border (clamp).
 * halo_rows must be 0 (both NULL) or >= 10. The X pass is purely horizontal, so the neighbour's shaded rows are filtered in X here like the tile's own and the
 * Y window reaches them: neighbours exchange 10 rows of scene colour (vqhip_exchange_blur_halos moves rows of any RGBA16F / RGBA32F image) right after the
 * shade kernel instead of 10 X-blurred rows after the X pass — the same bytes, one dependency earlier. Identical bits to the untiled frame. */
VQHIP_API int vqhip_post_process_tile(vqhip_ctx* ctx, void* stream, const void* sceneColor, void* out,
        const void* halo_top, const void* halo_bottom, int halo_rows, int width, int height,
        const VQ_TonemapperParams* tonemapParams, vqhip_format inFmt, vqhip_format outFmt);

/* Replaces VQRenderer::ComputeBRDFIntegrationLUT (Renderer.cpp:871-909) == CubemapConvolution.hlsl:
 * CSMain_BRDFIntegration :225-240. Reference values: size 1024, samples 2048, RG16F. */
VQHIP_API int vqhip_brdf_lut(vqhip_ctx* ctx, void* stream, void* outRG, int size, int samples, vqhip_format fmt);

/* Replaces VQ_DXGI_UTILS::MipImage's 16-byte branch (Source/Renderer/Resources/DXGIUtils.cpp:289-317) as
 * driven by TextureManager::GenerateMips (TextureManager.cpp:643-738): per-channel MIN of each 2x2 block,
 * alpha := 1. `mips` = device buffer holding level 0 (w0 x h0 RGBA32F) followed by space for all further
 * levels, densely packed; levels 1..nMips-1 are written. vqhip_mip_chain_bytes() sizes the buffer and
 * vqhip_mip_level_count() == Image::CalculateMipLevelCount == floor(log2(max(w,h)))+1. */
VQHIP_API int    vqhip_mip_level_count(int w, int h);
VQHIP_API size_t vqhip_mip_chain_bytes(int w0, int h0, int nMips);
VQHIP_API size_t vqhip_mip_level_offset_bytes(int w0, int h0, int level);
VQHIP_API int    vqhip_mip_chain_min_rgba32f(vqhip_ctx* ctx, void* stream, void* mips, int w0, int h0, int nMips);

/* Cube-map helpers: number of mips of the specular cube == CalculateMipLevelCount(res,res) - 1
 * (EnvironmentMapRendering.cpp:63) and byte sizes of the packed RGBA16F cubes. */
VQHIP_API int    vqhip_specular_mip_count(int spec_res0);
VQHIP_API size_t vqhip_cube_bytes(int res0, int nMips, vqhip_format fmt);

/* Replaces the diffuse-irradiance draws (EnvironmentMapRendering.cpp:181-277) ==
 * CubemapConvolution.hlsl:PSMain_DiffuseIrradiance :112-163 over all 6 faces.
 * equirect_mips = RGBA32F mip chain (layout of vqhip_mip_chain_min_rgba32f); the shader samples mip 3
 * with a TRILINEAR_WRAP sampler (RootSignatures.cpp:402). step = INTEGRATION_STEP_DIFFUSE_IRRADIANCE
 * (0.050 / 0.025 / 0.010, PipelineStateObjects.cpp:1298-1306).
 * When the sampled mip is a power-of-two image the call first rewrites it, on `stream`, as 48-byte footprint records in a buffer the context
 * owns (3 x the mip: 3 MB for a 2048^2 chain) and the taps gather from those; the buffer is rewritten by every call, and a call on another
 * stream waits (hipStreamWaitEvent) for the previous call's kernel before it does so. */
VQHIP_API int vqhip_conv_diffuse(vqhip_ctx* ctx, void* stream, const void* equirect_mips, int w0, int h0, int nMips,
        int diffuseRes, float step, vqhip_conv_order order, void* outCube, vqhip_format fmt);

/* Replaces the specular-prefilter draws (EnvironmentMapRendering.cpp:386-472) ==
 * CubemapConvolution.hlsl:PSMain_SpecularIrradiance :168-223 for every (mip, face); roughness =
 * mip/(MIPS-1), TextureDimensionsLOD0 = (w0,h0) of the equirect (:431-435). */
VQHIP_API int vqhip_conv_specular(vqhip_ctx* ctx, void* stream, const void* equirect_mips, int w0, int h0, int nMips,
        int specRes0, vqhip_conv_order order, void* outCubeMips, vqhip_format fmt);

/* Replaces VQRenderer::PreFilterEnvironmentMap (EnvironmentMapRendering.cpp:139-486): diffuse
 * convolution -> per-face blur X,Y -> specular mips, all outputs RGBA16F like the reference. */
VQHIP_API int vqhip_envmap_prefilter(vqhip_ctx* ctx, void* stream, const void* equirect_mips, int w0, int h0, int nMips,
        int diffuseRes, float diffuseStep, int specRes0, vqhip_conv_order order, const vqhip_envmap_out* out);

/* ---- G-buffer producer ----------------------------------------------------------
 * Replaces the surface-assembly half of ForwardLighting.hlsl:PSMain (:226-287): uv transform, the seven
 * material-map fetches, SRGBToLinear (ShadingMath.hlsl:65), Has*Map() selection
 * (LightingConstantBufferData.h:116-124), UnpackNormal (ShadingMath.hlsl:44-52), the ORM / AO / SSAO
 * multiplies — for every pixel of the interpolant planes at once, each pixel using
 * materials[materialIndex] (the reference binds one material per draw: SceneRendering.cpp:1744-1750).
 * Writes the four planes of `out` (their pointers are written through despite the const in
 * vqhip_gbuffer); pixels without geometry get all-zero records, and so do the fragments an alpha-masked material discards
 * (VQHIP_MATERIAL_ALPHA_MASKED: their index in in->ip2 is overwritten with -1).
 *   materials : HOST array (copied; numMaterials <= vqhip_max_materials())
 *   fAmbientLightingFactor : cbPerFrame.fAmbientLightingFactor (:247)
 *   ssao : NULL or a descriptor with texels == NULL => factor 1.0
 * Sampler s2 is ANISOTROPIC_WRAP with MaxAnisotropy = 0 (RootSignatures.cpp:111,149), s0 TRILINEAR_WRAP:
 * both are evaluated as isotropic trilinear WRAP with the LOD of the pixel quad's uv differences
 * (DESIGN.md "G-buffer producer"). */
VQHIP_API int vqhip_max_materials(void);
VQHIP_API int vqhip_gbuffer_from_materials(vqhip_ctx* ctx, void* stream,
        const vqhip_interpolants* in, const vqhip_material* materials, int numMaterials,
        float fAmbientLightingFactor, const vqhip_ssao* ssao, const vqhip_gbuffer* out);

/* PSMain as the engine runs it (Shaders/ForwardLighting.hlsl:226-380; the lit draws of VQRenderer::RenderSceneColor,
 * SceneRendering.cpp:1619-1760): vqhip_gbuffer_from_materials and vqhip_forward_lighting in ONE kernel. The 64-byte G-buffer record of a
 * pixel never leaves registers (128 B/pixel of HBM traffic less than the two calls); the result is bit-identical to the two calls with
 * fAmbientLightingFactor = perFrame->fAmbientLightingFactor (the same cbuffer field PSMain reads, :247). Pixels without geometry and
 * discarded fragments shade the all-zero record exactly like the two calls do — composite the sky over them with vqhip_skydome
 * (alpha-masked discards are marked -1 in in->ip2.w as by vqhip_gbuffer_from_materials). Arguments: as the two calls. */
VQHIP_API int vqhip_forward_lighting_from_materials(vqhip_ctx* ctx, void* stream,
        const vqhip_interpolants* in, const vqhip_material* materials, int numMaterials, const vqhip_ssao* ssao,
        const VQ_PerFrameData* perFrame, const VQ_PerViewLightingData* perView,
        const VQ_PointLight* extraPoint, int numExtraPoint,
        const vqhip_envmap* env, const vqhip_shadowmaps* sm,
        void* out, int out_row_pitch_px, vqhip_format outFmt);
/* the same with the extra render targets of the draw (vqhip_psmain_targets above); bit-identical to vqhip_gbuffer_from_materials + vqhip_forward_lighting_mrt
 * on every pixel a fragment covers. Pixels WITHOUT geometry and alpha-mask discards are not written in albedo_metallic / motion_vectors — they keep the
 * values the caller cleared the targets to, as under the rasteriser (PSMain never runs there; the G-buffer form above cannot know and writes them all). */
VQHIP_API int vqhip_forward_lighting_from_materials_mrt(vqhip_ctx* ctx, void* stream,
        const vqhip_interpolants* in, const vqhip_material* materials, int numMaterials, const vqhip_ssao* ssao,
        const VQ_PerFrameData* perFrame, const VQ_PerViewLightingData* perView,
        const VQ_PointLight* extraPoint, int numExtraPoint,
        const vqhip_envmap* env, const vqhip_shadowmaps* sm,
        void* out, int out_row_pitch_px, vqhip_format outFmt, const vqhip_psmain_targets* targets);

/* Replaces the pixel shader of the Z pre-pass (VQRenderer::RenderDepthPrePass, SceneRendering.cpp:1264-1360; Shaders/DepthPrePass.hlsl:PSMain :153-171) for
 * every pixel of the interpolant planes: Tex_SceneNormals, the packed surface normals that SSR (`g_normal` of vqhip_ssr_environment_fallback) and
 * FFX-CACAO read —
 *     float4((SurfaceN + 1) * 0.5, 1),   SurfaceN = length(Normal) < 0.01 ? normalize(WorldSpaceNormal) : UnpackNormal(Normal, N, T)
 * the surface normal of ForwardLighting.hlsl:265-267, except that the normal map is fetched with Sample — no normalMapMipBias (:164) — and the diffuse map
 * only for the alpha test of the "_AlphaMasked" PSOs (VQHIP_MATERIAL_ALPHA_MASKED, :157-161). Pixels without geometry and discarded fragments keep the
 * target's clear value 0 (SceneRendering.cpp:1289-1300). The coverage plane in->ip2.w is NOT modified (the lighting pass repeats the discard itself).
 *   out    : outFmt R10G10B10A2_UNORM — the reference's format (RenderResources.cpp:185-197, PipelineStateObjects.cpp:1634-1635): one uint32 per pixel,
 *            r in bits 0-9, g 10-19, b 20-29, alpha 30-31 (1 -> 3); float -> UNORM n = trunc(saturate(c) * (2^n - 1) + 0.5) —
 *            or RGBA32F holding the unquantised float4 (w = 1 covered / 0 not). out_row_pitch_px pixels per row (0 = width).
 *   materials : HOST array, as for vqhip_gbuffer_from_materials; vqhip_set_arithmetic selects the reading of normalize / dot here too.
 * The depth half of the pre-pass is vqhip_scene_depth; the interpolant planes are vqhip_scene_interpolants'. */
VQHIP_API int vqhip_scene_normals_from_materials(vqhip_ctx* ctx, void* stream,
        const vqhip_interpolants* in, const vqhip_material* materials, int numMaterials,
        void* out, vqhip_format outFmt, int out_row_pitch_px);

/* Replaces VQ_DXGI_UTILS::MipImage's 4-byte branch (DXGIUtils.cpp:264-285) as driven by
 * TextureManager::GenerateMips: each channel = (sum of the 2x2 block) / 4, integer division.
 * Same buffer convention as vqhip_mip_chain_min_rgba32f with 4-byte texels; w0, h0 powers of two. */
VQHIP_API size_t vqhip_mip_chain_bytes_rgba8(int w0, int h0, int nMips);
VQHIP_API int    vqhip_mip_chain_box_rgba8(vqhip_ctx* ctx, void* stream, void* mips, int w0, int h0, int nMips);

/* ---- skydome ----------------------------------------------------------------------
 * Replaces the "Draw Environment Map" draw of VQRenderer::RenderSceneColor (SceneRendering.cpp:1822-1850) ==
 * Skydome.hlsl:VSMain/PSMain (:39-56): every pixel no geometry covers gets
 * float4(texEquirectEnvironmentMap.SampleLevel(TRILINEAR_WRAP, DirectionToEquirectUV(normalize(dir)), 0).rgb, 1).
 * The cube mesh is centred on the sky camera (position 0, yaw = camera yaw + HDRIYawOffset, pitch = camera pitch,
 * projection of the main camera: Scene.cpp:573-584) and CubemapLookDirection = normalize(position) is linear on
 * every cube face, so its perspective-correct interpolant at a pixel is parallel to the pixel's view ray:
 *   dir = forward + (ndc.x * tanHalfFovX) * right + (ndc.y * tanHalfFovY) * up,
 *   ndc = (2(x+.5)/W - 1, 1 - 2(y+.5)/H)          (VQ_SkydomeParams holds the sky camera's world-space basis).
 *   equirect_level0 : RGBA32F w0 x h0 (level 0 of the HDRI chain; SRV_HDREnvironment, EnvironmentMap.cpp:142-209)
 *   coverage        : NULL => every pixel is sky; else only pixels whose ip2.w material index is < 0 are written
 *   color           : scene colour target (RGBA16F reference format, or RGBA32F), written in place. */
typedef struct VQ_SkydomeParams {
    VQ_float3 right;   float tanHalfFovX;
    VQ_float3 up;      float tanHalfFovY;
    VQ_float3 forward; float pad;
} VQ_SkydomeParams;
VQHIP_API int vqhip_skydome(vqhip_ctx* ctx, void* stream, const void* equirect_level0, int w0, int h0,
        const VQ_SkydomeParams* params, const vqhip_interpolants* coverage,
        void* color, int width, int height, int row_pitch_px, vqhip_format fmt);

/* Light gizmo meshes — the other half of SURVEY.md §8(f).2 — are drawn by the reference with Unlit.hlsl (SceneRendering.cpp:1787-1819):
 * VSMain transforms the mesh, PSMain (:58-61) returns the light's colour for every covered, depth-tested pixel. The rasterised route is
 * vqhip_unlit_draws (below: meshes in, depth-tested colour out, opaque or blended). This call is the route for an engine that rasterises
 * the gizmos itself; what crosses the boundary is then the result, in the same plane the skydome reads: a pixel whose ip2.w index is
 * -(2+k) is covered by gizmo k (index -1 = sky, >= 0 = material). Those pixels receive colors[k] (all four channels, as PSMain
 * returns float4(color)); every other pixel is left untouched. colors is a HOST array of numColors <= VQHIP_MAX_UNLIT_COLORS entries
 * (FFrameConstantBufferUnlit::color of each FLightRenderData, SceneRendering.cpp:1799). */
#define VQHIP_MAX_UNLIT_COLORS 64
VQHIP_API int vqhip_unlit_composite(vqhip_ctx* ctx, void* stream, const vqhip_interpolants* coverage,
        const VQ_float4* colors, int numColors, void* color, int width, int height, int row_pitch_px, vqhip_format fmt);

/* ---- HDRI ingest -------------------------------------------------------------------
 * Replaces Image::LoadFromFile -> stbi_loadf for Radiance .hdr files (call site TextureManager.cpp:566; the decoder
 * itself lives in stb_image inside the un-vendored Libs/VQUtils submodule — its published algorithm, stb_image.h
 * v2.2x stbi__hdr_load / stbi__hdr_convert, is what is restated): header "#?RADIANCE" | "#?RGBE", a
 * "FORMAT=32-bit_rle_rgbe" line, blank line, "-Y <height> +X <width>", then per scanline either new-style RLE
 * (02 02 hi lo + four run-length coded byte planes) or flat RGBE quadruples (width < 8, width >= 32768, or no
 * 02 02 marker); pixel = (r,g,b) * 2^(e-136), (0,0,0) when e == 0, alpha := 1.
 * The host parses the header and walks the run headers (count bytes only: where every byte plane of every scanline starts, and whether the file is sound); the
 * encoded bytes go to the GPU as they are, and one kernel expands the runs (a workgroup per scanline, a wave per byte plane, through LDS) and converts RGBE -> RGBA32F
 * straight into level 0 of the chain that vqhip_mip_chain_min_rgba32f completes. Flat files and scanlines wider than ~19 000 pixels: expansion on the host.
 *   file / bytes : HOST memory holding the whole .hdr file
 * Truncated or corrupt run data returns VQHIP_ERR_INVALID_ARG (stb_image reads zeros past the end of the file). */
VQHIP_API int vqhip_hdr_parse_header(const void* file, size_t bytes, int* width, int* height, size_t* data_offset);
VQHIP_API int vqhip_hdr_decode_rgba32f(vqhip_ctx* ctx, void* stream, const void* file, size_t bytes,
        void* out_rgba32f, int width, int height);
/* Replaces Image::CreateResizedImage as CreateEnvironmentMapTextureFromHiResAndSaveToDisk uses it (EnvironmentMap.cpp:142-209, call :167):
 * when the HDRI of the chosen resolution is missing, the next higher one (8k / 4k / 2k of LookupResolutionX/Y :163-164) is downsized to it.
 * The resampler itself (stb_image_resize inside the un-vendored Libs/VQUtils submodule, version and filter not pinned by the reference tree)
 * is NOT restated — PARITY UNPINNED for this entry point: every target texel is the plain mean of its k x k source block, k = width /
 * out_width = height / out_height an integer (2, 4, 8 for the engine's table) — which is also what the engine's alternative branch (:183-200,
 * repeated CreateHalfResolutionFromImage) converges to. Any other ratio returns VQHIP_ERR_UNSUPPORTED. RGBA32F device images, alpha := 1. */
VQHIP_API int vqhip_hdr_downsize_rgba32f(vqhip_ctx* ctx, void* stream, const void* in_rgba32f, int width, int height,
        void* out_rgba32f, int out_width, int out_height);

/* ---- FidelityFX Super Resolution 1.0 (post chain tail) ------------------------------
 * Replace the FSR-EASU and FSR-RCAS dispatches of VQRenderer::RenderPostProcess (SceneRendering.cpp:2695-2784):
 * Shaders/AMDFidelityFX.hlsl:FSR_EASU_CSMain / FSR_RCAS_CSMain, compiled without FSR_FP16
 * (PipelineStateObjects.cpp:1366-1374) == FsrEasuF / FsrRcasF of Shaders/AMDFidelityFX/FSR1.0/ffx_fsr1.h.
 * The constant blocks are exactly the reference's cbuffers: FFSR1_EASU::EASUConstantBlock[16] and
 * FFSR1_RCAS::RCASConstantBlock[4] (PostProcess.h:114-130), filled by vqhip_fsr_easu_con / vqhip_fsr_rcas_con ==
 * FsrEasuCon / FsrRcasCon on the CPU (PostProcess.cpp:39-79; default RCASSharpnessStops 0.2).
 *   EASU : in (inW x inH, the tonemapper output: RGBA8_UNORM SDR or RGBA16F HDR; RGBA32F also accepted) -> out (outW x outH)
 *   RCAS : in/out of the same size. Alpha is undefined in the reference (RWTexture2D<float3>): 1 is written. */
VQHIP_API void vqhip_fsr_easu_con(uint32_t con[16], float inputViewportW, float inputViewportH,
        float inputSizeW, float inputSizeH, float outputW, float outputH);
VQHIP_API void vqhip_fsr_rcas_con(uint32_t con[4], float sharpnessStops);
VQHIP_API int vqhip_fsr_easu(vqhip_ctx* ctx, void* stream, const void* in, int inW, int inH, vqhip_format inFmt,
        const uint32_t con[16], void* out, int outW, int outH, vqhip_format outFmt);
VQHIP_API int vqhip_fsr_rcas(vqhip_ctx* ctx, void* stream, const void* in, void* out, int width, int height,
        const uint32_t con[4], vqhip_format inFmt, vqhip_format outFmt);

/* Replaces the debug-visualisation dispatch of RenderPostProcess (SceneRendering.cpp:2541-2576) == Visualization.hlsl:CSMain
 * :34-120. VQ_VizParams == FPostProcessParameters::FVizualizationParams (the cbuffer :26-31); iDrawMode uses the SHADER's
 * numbering (:71-80): 1 DEPTH pow(r,500), 2 NORMALS, 3 ROUGHNESS / 4 METALLIC (alpha), 5 AO (red), 6 ALBEDO / 7 REFLECTIONS
 * (rgb), 8 MOTION_VECTORS; anything else (including 0) writes magenta. Output alpha = input alpha. The caller binds the
 * image the reference's switch selects (:2555-2565) in the format that target has: inFmt RGBA8_UNORM | RGBA16F | RGBA32F (scene colour, Tex_SceneVisualization of
 * vqhip_forward_lighting_mrt, reflections), R10G10B10A2_UNORM (Tex_SceneNormals of vqhip_scene_normals_from_materials: c / 1023, alpha / 3), RG16F | RG32F
 * (Tex_SceneMotionVectors: the missing channels read 0 and 1 like a typed SRV load); single-channel sources are passed expanded to (r,0,0,1).
 * outFmt RGBA8_UNORM | RGBA16F | RGBA32F. */
/* Replaces ApplyReflectionsPass::RecordCommands (ApplyReflections.cpp:45-80) == ApplyReflections.hlsl:CSMain :30-50 without
 * COMPOSITE_BOUNDING_VOLUMES: sceneColor.rgb += reflectionRadiance.rgb, alpha (roughness) kept; in place on the scene colour.
 * (The reflection radiance comes from vqhip_ssr_environment_fallback + vqhip_ssr_classify + vqhip_ssr_intersect below, denoised by vqhip_ssr_reproject +
 * vqhip_ssr_prefilter + vqhip_ssr_resolve_temporal; of the FidelityFX reflection DENOISER only PrepareBlueNoiseTexture is out of scope.) fmt: RGBA16F | RGBA32F for both. */
VQHIP_API int vqhip_apply_reflections(vqhip_ctx* ctx, void* stream, const void* reflectionRadiance, void* sceneColor,
        int width, int height, vqhip_format fmt);
/* Replaces VQRenderer::CompositeReflections (SceneRendering.cpp:2362-2403): ApplyReflectionsPass in the permutation its parameters select
 * (ApplyReflections.cpp:62-68). boundingVolumes == NULL: vqhip_apply_reflections. Otherwise "[PSO] ApplyReflectionsAndBoundingVolumes"
 * (COMPOSITE_BOUNDING_VOLUMES, ApplyReflections.hlsl:44-48): Tex_SceneColorBoundingVolumes (the light-bounds target of RenderLightBounds,
 * same format as the scene colour; produced by vqhip_unlit_draws in opaque mode over a zero-cleared plane, vqhip::UnlitDrawsPass::LightBounds) is blended over the sum,
 *     rgb = BV.rgb * BV.a + (scene.rgb + reflection.rgb) * (1 - BV.a),   alpha = BV.a,
 * every product and sum rounded on its own, as written. In place on sceneColor; the inputs must not alias it. fmt: RGBA16F | RGBA32F for all three. */
VQHIP_API int vqhip_composite_reflections(vqhip_ctx* ctx, void* stream, const void* reflectionRadiance, const void* boundingVolumes, void* sceneColor,
        int width, int height, vqhip_format fmt);

/* ---- SSR's consumption of the specular cube + BRDF LUT ---------------------------
 * == FFX_SSSRConstants (Source/Renderer/Rendering/RenderPass/ScreenSpaceReflections.h:43-65), the cbuffer `Constants` of
 * Shaders/ScreenSpaceReflections/Common.hlsl:26-48, byte for byte (XMMATRIX: row-major, 16-aligned), as VQRenderer::RenderReflections fills it
 * (SceneRendering.cpp:2221-2242). */
typedef struct VQ_SSSRConstants {
    VQ_matrix invViewProjection, projection, invProjection, view, invView, prevViewProjection, envMapRotation;
    uint32_t bufferDimensions[2];
    float    inverseBufferDimensions[2];
    float    temporalStabilityFactor, depthBufferThickness, roughnessThreshold, varianceThreshold;
    uint32_t frameIndex, maxTraversalIntersections, minTraversalOccupancy, mostDetailedMip, samplesPerQuad,
             temporalVarianceGuidedTracingEnabled, envMapSpecularIrradianceCubemapMipLevelCount;
    uint32_t pad_[1];
} VQ_SSSRConstants;
VQHIP_STATIC_ASSERT(sizeof(VQ_SSSRConstants) == 512, "FFX_SSSRConstants is 7 matrices + 15 dwords, padded to 16");
VQHIP_STATIC_ASSERT(offsetof(VQ_SSSRConstants, bufferDimensions) == 448 && offsetof(VQ_SSSRConstants, roughnessThreshold) == 472 &&
                    offsetof(VQ_SSSRConstants, envMapSpecularIrradianceCubemapMipLevelCount) == 504, "FFX_SSSRConstants layout");

/* Replaces the part of the "FFX DNSR ClassifyTiles" dispatch (ScreenSpaceReflections.cpp:262-276) that consumes the prefiltered specular cube and
 * the BRDF LUT: for every pixel, ClassifyReflectionTiles.hlsl:ClassifyTiles :146-152 + SampleEnvironmentMap :78-94 —
 *     radiance = (depth < 1 && !(roughness < roughnessThreshold)) ? float4(SampleEnvironmentMap(pixel, roughness, mipCount), 0) : 0
 * i.e. surfaces too rough for a traced ray get the environment's prefiltered reflection: view-space reflect of the view ray about the G-buffer normal,
 * g_environment_map.SampleLevel(envMapRotation * R_world, roughness * (mipCount - 1)) — a FRACTIONAL level: trilinear between cube mips, seamless
 * (csrc/vq_sampling.h:sample_cube_lod_rgba16f) — times EnvironmentBRDF(NdotV, roughness, metallic 1, ...) from the LUT (BRDF.hlsl:196-207).
 * The ray classification / ray list / denoiser tile list of the same dispatch is vqhip_ssr_classify, the traced rays are vqhip_ssr_intersect (below); the denoiser's
 * Reproject, Prefilter and ResolveTemporal are vqhip_ssr_reproject / vqhip_ssr_prefilter / vqhip_ssr_resolve_temporal; what stays out of scope is
 * PrepareBlueNoiseTexture with its Sobol tables.
 *   sceneColorRoughness : g_roughness   == the scene colour whose alpha is the roughness (ForwardLighting.hlsl:380), RGBA16F | RGBA32F
 *   depth               : g_depth_buffer == mip 0 of the depth hierarchy, R32F, NDC z (far plane 1)
 *   normals             : g_normal      == Tex_SceneNormals, R10G10B10A2_UNORM (one uint32 per pixel, r in bits 0-9) | RGBA32F holding the same [0,1] values
 *   cb                  : host pointer; invProjection, view, invView, envMapRotation, inverseBufferDimensions, roughnessThreshold and
 *                         envMapSpecularIrradianceCubemapMipLevelCount are read (mipCount must be in [1, env->spec_mips])
 *   env                 : specular_cube / spec_res0 / spec_mips and brdf_lut / lut_size are read (device pointers)
 *   outRadiance         : g_intersection_output, RGBA16F (TexRadiance, ScreenSpaceReflections.cpp:129) | RGBA32F; alpha = 0
 *   outExtractedRoughness: g_extracted_roughness (CSMain :196), R8_UNORM, one byte per pixel, row pitch = width; may be NULL
 * Pitches in pixels (0 = width). */
VQHIP_API int vqhip_ssr_environment_fallback(vqhip_ctx* ctx, void* stream,
        const void* sceneColorRoughness, vqhip_format sceneFmt, int scenePitchPx,
        const float* depth, int depthPitchPx,
        const void* normals, vqhip_format normalFmt, int normalPitchPx,
        int width, int height, const VQ_SSSRConstants* cb, const vqhip_envmap* env,
        void* outRadiance, vqhip_format outFmt, int outPitchPx, uint8_t* outExtractedRoughness);

/* The ray list of the same dispatch: ClassifyReflectionTiles.hlsl:ClassifyTiles :96-145,157-161 without the fallback radiance (that stays
 * vqhip_ssr_environment_fallback). Per pixel, as written: needs_ray = on screen && depth < 1 && roughness < roughnessThreshold; needs_denoiser = needs_ray &&
 * !(roughness < 0.04); IsBaseRay for samplesPerQuad 1 / 2 / other (:65-74) deactivates glossy rays, never mirror rays; with temporalVarianceGuidedTracingEnabled a
 * deactivated pixel whose variance history exceeds varianceThreshold traces again; the three copy flags are read from the quad neighbours (lanes l^1, l^2, l^3 under
 * FFX_DNSR_Reflections_RemapLane8x8). The reference appends with atomics, so any permutation is a valid reference result; this library's ORDER is part of its contract
 * (docs/DESIGN_DETAILS.md §7.11): 8 x 8 tiles row-major, inside a tile lanes 0..63 of RemapLane8x8, rays compacted in that order, the tile list in tile order —
 * built as count -> scan -> scatter (three launches; no workgroup waits for another). The frame is cb->bufferDimensions (each <= 4096, else VQHIP_ERR_UNSUPPORTED).
 *   sceneColorRoughness : as vqhip_ssr_environment_fallback reads it (alpha = roughness), RGBA16F | RGBA32F
 *   depth               : level 0 of the depth hierarchy (vqhip_depth_hierarchy), R32F
 *   varianceHistory     : g_variance_history, an R16F plane (one half per pixel), or NULL = every pixel reads 0
 *   cb                  : host pointer; bufferDimensions, roughnessThreshold, varianceThreshold, samplesPerQuad, temporalVarianceGuidedTracingEnabled are read
 *   rayList             : uint32[width * height], PackRayCoords (Common.hlsl:62-71): x bits 0-14, y 15-28, copy horizontal 29, vertical 30, diagonal 31
 *   counters            : uint32[2] = { ray count, denoiser tile count }
 *   denoiserTileList    : NULL, or uint32[ceil(w/8) * ceil(h/8)]: (y << 16) | x of the first pixel of each tile in which some lane is glossy && depth < 1 — as written
 *                         (:126) that test is not masked by the screen test, and lanes beyond the frame load 0: the partial tiles of the right / bottom edge are listed
 * All outputs are device memory, written on `stream`; pitches in pixels (0 = width). */
VQHIP_API int vqhip_ssr_classify(vqhip_ctx* ctx, void* stream,
        const void* sceneColorRoughness, vqhip_format sceneFmt, int scenePitchPx,
        const float* depth, int depthPitchPx,
        const void* varianceHistory, int variancePitchPx,
        const VQ_SSSRConstants* cb,
        uint32_t* rayList, uint32_t* counters, uint32_t* denoiserTileList);

/* Replaces the "FFX SSSR Intersection" dispatch == Intersect.hlsl:CSMain :145-216 + AMDFidelityFX/SSSR/ffx_sssr.h for every entry of the ray list: the GGX-VNDF
 * reflection direction from the blue-noise sample, the hierarchical march through the min-depth pyramid, FFX_SSSR_ValidateHit, and
 *     radiance.rgb = lerp(SampleEnvironmentMap(level 0), g_lit_scene at the hit, confidence),   radiance.a = world_ray_length
 * written IN PLACE into the buffer vqhip_ssr_environment_fallback filled, at the ray's pixel and at its up to three copy targets (coords ^ 1). The ray count is read on
 * the device (no host synchronisation). The float32 contract — expression order, load / convert rules, and the wave term: WaveActiveCountBits(true) <=
 * minTraversalOccupancy is evaluated over the rays [64g, 64g + 64) of the list still in the loop, one wave per 64 consecutive rays — is docs/DESIGN_DETAILS.md §7.11.
 *   rayList, counters   : as vqhip_ssr_classify wrote them (counters[0] rays; clamped to width * height)
 *   litScene            : g_lit_scene, RGBA16F | RGBA32F; must not overlap `radiance`
 *   hierarchy           : the buffer of vqhip_depth_hierarchy for the same frame size, whatever flags it was built with
 *   normals             : g_normal, R10G10B10A2_UNORM | RGBA32F
 *   extractedRoughness  : g_roughness == outExtractedRoughness of vqhip_ssr_environment_fallback, R8_UNORM, row pitch = width; decoded c / 255 correctly rounded
 *   blueNoise           : g_blue_noise_texture, 128 x 128 R8G8_UNORM (two bytes per texel, row pitch 128 texels), provided by the caller
 *   cb                  : host pointer; maxTraversalIntersections > 256 or mostDetailedMip > 5: VQHIP_ERR_UNSUPPORTED
 *   env                 : specular_cube / spec_res0 / spec_mips and brdf_lut / lut_size are read (device pointers)
 * The frame is cb->bufferDimensions (each <= 4096). Pitches in pixels (0 = width). PARITY UNPINNED like §7.9 / §7.10 (docs/WARP_CALIBRATION.md §6). */
VQHIP_API int vqhip_ssr_intersect(vqhip_ctx* ctx, void* stream,
        const uint32_t* rayList, const uint32_t* counters,
        const void* litScene, vqhip_format litFmt, int litPitchPx,
        const float* hierarchy,
        const void* normals, vqhip_format normalFmt, int normalPitchPx,
        const uint8_t* extractedRoughness, const uint8_t* blueNoise,
        const VQ_SSSRConstants* cb, const vqhip_envmap* env,
        void* radiance, vqhip_format radianceFmt, int radiancePitchPx);

/* Replaces the "FFX DNSR Prefilter" and "FFX DNSR Resolve Temporal" dispatches (ScreenSpaceReflections.cpp, between the march and the composite) ==
 * Prefilter.hlsl:CSMain + ffx_denoiser_reflections_prefilter.h (15-tap edge-stopping spatial filter) and ResolveTemporal.hlsl:CSMain +
 * ffx_denoiser_reflections_resolve_temporal.h (9 x 9 local moments, history clip, blend) for every 8 x 8 tile of the denoiser tile list. The float32 contract —
 * expression order, the binary16 round trip of the values the reference packs into group-shared memory, exp(x) = exp2(x * 1.44269502f), loads outside the frame
 * reading 0, FFX_DNSR_Reflections_RoundUp8 as written, the bilinear CLAMP fetch of the 1/8-resolution average radiance — is docs/DESIGN_DETAILS.md §7.12;
 * tests/ssr_denoise_ref.py states it in numpy. Reproject (pass 1), which produces averageRadiance, variance, sampleCount and reprojectedRadiance, is
 * vqhip_ssr_reproject (below).
 *   denoiserTileList, counters : as vqhip_ssr_classify wrote them; counters[1] tiles, read on the device (no host synchronisation) and clamped to
 *                                ceil(w/8) * ceil(h/8), the number of entries the list must hold. An entry is (y << 16) | x; its tile is DEFINED by this contract as (x >> 3, y >> 3) — for the 8-aligned entries
 *                                vqhip_ssr_classify writes that is what CSMain computes; the shader itself gives an unaligned entry no single tile; an entry
 *                                beyond the tile grid is skipped, duplicates and any order are fine. Pixels of unlisted tiles are not written.
 *   depth                      : level 0 of the depth hierarchy, R32F
 *   normals                    : g_normal, R10G10B10A2_UNORM | RGBA32F
 *   extractedRoughness         : R8_UNORM, row pitch = width (vqhip_ssr_environment_fallback's output)
 *   averageRadiance            : [ceil(h/8)][ceil(w/8)], tightly packed, R11G11B10_FLOAT | RGBA32F
 *   radiance                   : RGBA16F | RGBA32F — the traced radiance (prefilter) / the prefiltered radiance (temporal resolve)
 *   reprojectedRadiance        : RGBA16F | RGBA32F
 *   variance, sampleCount      : R16F planes (one half per pixel)
 *   cb                         : host pointer; bufferDimensions (each <= 4096, else VQHIP_ERR_UNSUPPORTED), roughnessThreshold, invProjection (prefilter),
 *                                temporalStabilityFactor (temporal resolve) are read
 *   outRadiance                : RGBA16F | RGBA32F, radiance.xyzz (alpha = blue); outVariance: R16F. Stores round to nearest even. The sample-count target the
 *                                shaders declare is never written by them and is not an argument.
 * Outputs must not overlap any input of the same call (the apron reads neighbours other tiles write; the engine ping-pongs): VQHIP_ERR_INVALID_ARG.
 * Pitches in pixels (0 = width). PARITY UNPINNED like §7.9 - §7.11 (docs/WARP_CALIBRATION.md §7). */
VQHIP_API int vqhip_ssr_prefilter(vqhip_ctx* ctx, void* stream,
        const uint32_t* denoiserTileList, const uint32_t* counters,
        const float* depth, int depthPitchPx,
        const void* normals, vqhip_format normalFmt, int normalPitchPx,
        const uint8_t* extractedRoughness,
        const void* averageRadiance, vqhip_format avgFmt,
        const void* radiance, vqhip_format radianceFmt, int radiancePitchPx,
        const void* variance, int variancePitchPx,
        const VQ_SSSRConstants* cb,
        void* outRadiance, vqhip_format outFmt, int outPitchPx, void* outVariance, int outVariancePitchPx);
VQHIP_API int vqhip_ssr_resolve_temporal(vqhip_ctx* ctx, void* stream,
        const uint32_t* denoiserTileList, const uint32_t* counters,
        const uint8_t* extractedRoughness,
        const void* averageRadiance, vqhip_format avgFmt,
        const void* radiance, vqhip_format radianceFmt, int radiancePitchPx,
        const void* reprojectedRadiance, vqhip_format reprojectedFmt, int reprojectedPitchPx,
        const void* variance, int variancePitchPx, const void* sampleCount, int sampleCountPitchPx,
        const VQ_SSSRConstants* cb,
        void* outRadiance, vqhip_format outFmt, int outPitchPx, void* outVariance, int outVariancePitchPx);

/* Replaces the "FFX DNSR Reproject" dispatch (ScreenSpaceReflections.cpp, the first of the denoiser's three between the march and the composite) ==
 * Reproject.hlsl:CSMain + ffx_denoiser_reflections_reproject.h for every 8 x 8 tile of the denoiser tile list: the 9 x 9 local moments of the traced radiance, the
 * choice between hit-point and surface (motion-vector) reprojection, the 3 x 3 search and the 2 x 2 path where the history is disoccluded, the temporal variance and
 * sample count, and the 1/8-resolution average radiance. It writes the four planes vqhip_ssr_prefilter / vqhip_ssr_resolve_temporal consume. The float32 contract is
 * docs/DESIGN_DETAILS.md §7.13 (tile-list semantics, loads outside the frame, exp, the two arithmetic readings as §7.11 / §7.12; bilinear history fetches: texels
 * decoded to binary32, CLAMP, 8-bit fractions; the centre radiance is not rounded through binary16; a discarded history stores (0,0,0) / 1 / 1);
 * tests/ssr_reproject_ref.py states it in numpy. g_blue_noise_texture and g_average_radiance_history are bound by the engine but never read by the shader: they are
 * not arguments. Clearing the history (the engine's bClearHistoryBuffers) is a plain clear of the history planes by the caller.
 *   tile_list, counters          : as vqhip_ssr_classify wrote them (semantics as vqhip_ssr_prefilter)
 *   depth, depth_history         : R32F (level 0 of the depth hierarchy of this frame / of the previous one)
 *   normals, normal_history      : R10G10B10A2_UNORM | RGBA32F, each with its own format
 *   roughness, roughness_history : R8_UNORM (vqhip_ssr_environment_fallback's extracted roughness)
 *   radiance                     : RGBA16F | RGBA32F, the traced radiance; alpha = ray length
 *   radiance_history             : RGBA16F | RGBA32F, last frame's vqhip_ssr_resolve_temporal output
 *   motion_vectors               : RG16F | RG32F as vqhip_forward_lighting_mrt writes them
 *   variance_history, sample_count_history : R16F (last frame's resolved variance / this pass's sample count of last frame)
 *   out_reprojected              : RGBA16F | RGBA32F; alpha is written as 0 (the shader stores a float3)
 *   out_average                  : [ceil(h/8)][ceil(w/8)], tightly packed, R11G11B10_FLOAT | RGBA32F (alpha 0); written for listed tiles only. R11G11B10: one rounding to
 *                                  nearest even from binary32, overflow to inf, negative and -0 to 0, NaN to exponent 31 with a non-zero mantissa, denormals kept
 *   out_variance, out_sample_count : R16F. A pixel with roughness >= roughnessThreshold stores nothing to the three full-resolution outputs.
 *   cb                           : host pointer; bufferDimensions (each <= 4096, else VQHIP_ERR_UNSUPPORTED), invProjection, invView, prevViewProjection,
 *                                  roughnessThreshold are read (temporalStabilityFactor is passed to the shader function and never used there)
 * An output overlapping an input or another output: VQHIP_ERR_INVALID_ARG (the engine ping-pongs). Pitches in pixels, 0 = width. PARITY UNPINNED (docs/WARP_CALIBRATION.md §7). */
typedef struct vqhip_ssr_reproject_surfaces {
    const uint32_t* tile_list;
    const uint32_t* counters;
    const float*    depth;
    const void*     normals;
    const uint8_t*  roughness;
    const float*    depth_history;
    const void*     normal_history;
    const uint8_t*  roughness_history;
    const void*     radiance;
    const void*     radiance_history;
    const void*     motion_vectors;
    const void*     variance_history;
    const void*     sample_count_history;
    void*           out_reprojected;
    void*           out_average;
    void*           out_variance;
    void*           out_sample_count;
    int32_t         depth_pitch_px, normals_pitch_px, roughness_pitch_px, depth_history_pitch_px, normal_history_pitch_px, roughness_history_pitch_px;
    int32_t         radiance_pitch_px, radiance_history_pitch_px, motion_pitch_px, variance_history_pitch_px, sample_count_history_pitch_px;
    int32_t         out_reprojected_pitch_px, out_variance_pitch_px, out_sample_count_pitch_px;
    int32_t         normals_fmt, normal_history_fmt, radiance_fmt, radiance_history_fmt, motion_fmt, out_reprojected_fmt, out_average_fmt;   /* vqhip_format */
    int32_t         pad_;
} vqhip_ssr_reproject_surfaces;
VQHIP_STATIC_ASSERT(sizeof(vqhip_ssr_reproject_surfaces) == 224 && offsetof(vqhip_ssr_reproject_surfaces, radiance) == 64 &&
                    offsetof(vqhip_ssr_reproject_surfaces, out_reprojected) == 104 && offsetof(vqhip_ssr_reproject_surfaces, depth_pitch_px) == 136 &&
                    offsetof(vqhip_ssr_reproject_surfaces, normals_fmt) == 192, "vqhip_ssr_reproject_surfaces layout");
VQHIP_API int vqhip_ssr_reproject(vqhip_ctx* ctx, void* stream, const vqhip_ssr_reproject_surfaces* io, const VQ_SSSRConstants* cb);

typedef struct VQ_VizParams { int32_t iDrawMode; int32_t iUnpackNormals; float fInputStrength; } VQ_VizParams;
VQHIP_API int vqhip_visualize(vqhip_ctx* ctx, void* stream, const void* in, void* out, int width, int height,
        const VQ_VizParams* params, vqhip_format inFmt, vqhip_format outFmt);

/* ---- one frame row-tiled over the GPUs of a node ------------------------------------------------------
 * No reference analogue (VQEngine renders on one adapter; the limit being exceeded is the single command queue of
 * SceneRendering.cpp:2507). One process per GPU; rank r owns rows [row0, row0+rows) of the frame and only that part of the
 * G-buffer, lights / env maps / LUT are replicated. vqhip_forward_lighting, vqhip_gaussian_blur_x and the tonemapper need
 * no communication; the two exchanges below are the whole multi-GPU data path:
 *
 *   vqhip_forward_lighting(tile) -> vqhip_exchange_blur_halos(scene colour) -> vqhip_post_process_tile(tile, halo_top, halo_bottom) -> vqhip_composite_tiles
 *   or, pass by pass:
 *   vqhip_gaussian_blur_x(tile) -> vqhip_exchange_blur_halos(X-blurred) -> vqhip_gaussian_blur_y[_tonemap](tile, halo_top, halo_bottom) -> vqhip_composite_tiles
 *
 * A vqhip_comm wraps an RCCL communicator (one rank per GPU, xGMI point-to-point). RCCL is loaded at run time
 * (librccl.so.1, or the library named by $VQHIP_RCCL_LIBRARY): single-GPU hosts never touch it. Like every other entry point
 * the two exchanges enqueue on `stream` and return without synchronising.
 *   vqhip_comm_unique_id : rank 0 makes the 128-byte id (ncclGetUniqueId) and hands it to the other ranks out of band
 *   vqhip_comm_create    : every rank, collectively (ncclCommInitRank on the calling thread's current HIP device)
 *   vqhip_comm_adopt     : wrap an ncclComm_t the host already owns (not destroyed by vqhip_comm_destroy) */
#define VQHIP_HALO_ROWS      10        /* KERNEL_RANGE - 1, Shaders/GaussianBlur.hlsl:54-55 */
#define VQHIP_COMM_ID_BYTES  128       /* sizeof(ncclUniqueId) */
#define VQHIP_ALL_RANKS      (-1)
typedef struct vqhip_comm vqhip_comm;
/* rows of rank `rank`: frame_height / world each, the first frame_height % world ranks one more. world > 1 needs >= 10 rows per tile. */
VQHIP_API int  vqhip_rowtile(int frame_height, int world, int rank, int* row0, int* rows);
VQHIP_API int  vqhip_comm_unique_id(void* id128);
VQHIP_API int  vqhip_comm_create(const void* id128, int world, int rank, vqhip_comm** out_comm);
VQHIP_API int  vqhip_comm_adopt(void* nccl_comm, int world, int rank, vqhip_comm** out_comm);
VQHIP_API void vqhip_comm_destroy(vqhip_comm* comm);
/* ncclCommAbort: ends the transfers in flight on the communicator (a watchdog's way out of an exchange that does not complete) and frees
 * it like vqhip_comm_destroy; collective in effect — every rank must abort and build a new communicator before it exchanges again. */
VQHIP_API int  vqhip_comm_abort(vqhip_comm* comm);
/* What the communicator itself reports (read back from RCCL, not from the arguments of vqhip_comm_create): size and rank as RCCL sees
 * them (ncclCommCount / ncclCommUserRank), the library's version (ncclGetVersion; 0 = the test stand-in) and the path it was loaded from. */
typedef struct vqhip_comm_info {
    int32_t world, rank;                 /* as given to vqhip_comm_create / vqhip_comm_adopt */
    int32_t nranks_seen, rank_seen;      /* as RCCL reports them; -1 when the library lacks the query */
    int32_t rccl_version;                /* ncclGetVersion: e.g. 22105; -1 when unavailable */
    int32_t reserved;
    char    library_path[232];           /* dladdr of ncclSend */
} vqhip_comm_info;
VQHIP_API int  vqhip_comm_query(const vqhip_comm* comm, vqhip_comm_info* out_info);
/* Diagnostic: ONE grouped ncclSend + ncclRecv of `bytes` bytes from this rank to ITSELF, enqueued on `stream` like the exchanges below (RCCL serves
 * a self-addressed pair as a device copy). A single-GPU host can so check that the point-to-point entry points of the RCCL it bound
 * (ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd, stream semantics, byte counts) work from inside libvqhip.so before a multi-GPU frame
 * depends on them. src and dst: device buffers of `bytes` bytes that do not overlap. */
VQHIP_API int  vqhip_comm_loopback(vqhip_comm* comm, void* stream, const void* src, void* dst, size_t bytes);
/* Exchange 1. xblur_tile: this rank's X-blurred tile (tile_rows x width, row_pitch_px pixels per row, fmt RGBA16F | RGBA32F).
 * Sends its first 10 rows to rank-1 and its last 10 rows to rank+1 and receives theirs into halo_top / halo_bottom (dense
 * 10 x width buffers, the layout vqhip_gaussian_blur_y takes; ignored — may be NULL — at the frame's top / bottom edge).
 * ONE message per neighbour and direction whatever the pitch: rows of a pitched tile are first packed into a dense staging block
 * owned by the communicator (hipMemcpy2DAsync on `stream`), so both sides always post one send and one receive of 10*width pixels. */
VQHIP_API int  vqhip_exchange_blur_halos(vqhip_comm* comm, void* stream, const void* xblur_tile, int width, int tile_rows,
        int row_pitch_px, vqhip_format fmt, void* halo_top, void* halo_bottom);
/* Exchange 2. tile: this rank's finished tile (dense rows, fmt e.g. RGBA8_UNORM). root >= 0: only that rank receives the
 * frame (frame_height x width, dense; NULL elsewhere) — the GPU that presents, like the reference's one swap chain;
 * root == VQHIP_ALL_RANKS: every rank receives it. Transfers are grouped point-to-point messages straight into the frame. */
VQHIP_API int  vqhip_composite_tiles(vqhip_comm* comm, void* stream, const void* tile, int width, int frame_height,
        vqhip_format fmt, int root, void* frame);

/* ---- FidelityFX CACAO ambient occlusion (VQRenderer::RenderAmbientOcclusion, SceneRendering.cpp:1503-1555; AmbientOcclusionPass -> FFX_CACAO_D3D12Draw,
 * AMDFidelityFX/CACAO/ffx_cacao_impl.cpp:1922-2259; Shaders/AMDFidelityFX/CACAO/ffx_cacao.hlsl). docs/DESIGN_DETAILS.md §7.14; tests/cacao_ref.py states it in numpy.
 * Writes Tex_AmbientOcclusion (R8_UNORM), the texScreenSpaceAO of the lit draw, from Tex_SceneDepthResolve (R32F) and Tex_SceneNormals at native resolution:
 *   CSPrepareNativeDepthsAndMips -> CSPrepareNativeNormalsFromInputNormals -> CSGenerateQ2 x 4 passes -> CSEdgeSensitiveBlur<blurPassCount> x 4 -> CSApply,
 * five kernels on `stream` (the four passes of a stage are ONE launch), no host synchronisation, no allocation: every intermediate lives in `work`.
 * Implemented: quality HIGH (FFX_CACAO_QUALITY_HIGH) here and HIGHEST, the adaptive stage on top of this pipeline, as vqhip_adaptive_cacao below; useDownsampledSsao
 * off, generateNormals off. The lower levels, the downsampled path and normal generation return VQHIP_ERR_UNSUPPORTED, and so does HIGHEST passed to vqhip_cacao.
 * VQ_CacaoConstants == FFX_CACAO_Constants (ffx_cacao.h:95-154): the engine keeps calling FFX_CACAO_UpdateBufferSizeInfo / _UpdateConstants /
 * _UpdatePerPassConstants (ffx_cacao.cpp:48-262) and hands the shared block and the four per-pass blocks over as FFX_CACAO_D3D12Draw uploads them. */
typedef struct VQ_CacaoConstants {
    float DepthUnpackConsts[2], CameraTanHalfFOV[2], NDCToViewMul[2], NDCToViewAdd[2], DepthBufferUVToViewMul[2], DepthBufferUVToViewAdd[2];
    float EffectRadius, EffectShadowStrength, EffectShadowPow, EffectShadowClamp;
    float EffectFadeOutMul, EffectFadeOutAdd, EffectHorizonAngleThreshold, EffectSamplingRadiusNearLimitRec;
    float DepthPrecisionOffsetMod, NegRecEffectRadius, LoadCounterAvgDiv, AdaptiveSampleCountLimit;
    float InvSharpness; int32_t PassIndex; float BilateralSigmaSquared, BilateralSimilarityDistanceSigma;
    float PatternRotScaleMatrices[5][4];
    float NormalsUnpackMul, NormalsUnpackAdd, DetailAOStrength, Dummy0;
    float SSAOBufferDimensions[2], SSAOBufferInverseDimensions[2], DepthBufferDimensions[2], DepthBufferInverseDimensions[2];
    int32_t DepthBufferOffset[2]; float PerPassFullResUVOffset[2];
    float InputOutputBufferDimensions[2], InputOutputBufferInverseDimensions[2], ImportanceMapDimensions[2], ImportanceMapInverseDimensions[2];
    float DeinterleavedDepthBufferDimensions[2], DeinterleavedDepthBufferInverseDimensions[2], DeinterleavedDepthBufferOffset[2], DeinterleavedDepthBufferNormalisedOffset[2];
    struct { float m[4][4]; } NormalsWorldToViewspaceMatrix;   /* FFX_CACAO_Matrix4x4: row-major floats; the shader's cbuffer reads them column-major (§7.14) */
} VQ_CacaoConstants;
VQHIP_STATIC_ASSERT(sizeof(VQ_CacaoConstants) == 384 && offsetof(VQ_CacaoConstants, EffectRadius) == 48 && offsetof(VQ_CacaoConstants, InvSharpness) == 96 &&
                    offsetof(VQ_CacaoConstants, PassIndex) == 100 && offsetof(VQ_CacaoConstants, PatternRotScaleMatrices) == 112 &&
                    offsetof(VQ_CacaoConstants, NormalsUnpackMul) == 192 && offsetof(VQ_CacaoConstants, SSAOBufferDimensions) == 208 &&
                    offsetof(VQ_CacaoConstants, DepthBufferOffset) == 240 && offsetof(VQ_CacaoConstants, DeinterleavedDepthBufferNormalisedOffset) == 312 &&
                    offsetof(VQ_CacaoConstants, NormalsWorldToViewspaceMatrix) == 320, "VQ_CacaoConstants layout");
typedef enum vqhip_cacao_quality {   /* FFX_CACAO_Quality */
    VQHIP_CACAO_QUALITY_LOWEST = 0, VQHIP_CACAO_QUALITY_LOW = 1, VQHIP_CACAO_QUALITY_MEDIUM = 2, VQHIP_CACAO_QUALITY_HIGH = 3, VQHIP_CACAO_QUALITY_HIGHEST = 4
} vqhip_cacao_quality;
typedef enum vqhip_cacao_plane {
    VQHIP_CACAO_PLANE_DEPTHS = 0,    /* deinterleaved view-space depths, R16F: slice 0..3, mip 0..3; mip k is max(1, hw >> k) x max(1, hh >> k) */
    VQHIP_CACAO_PLANE_NORMALS = 1,   /* deinterleaved view-space normals, R8G8B8A8_SNORM: slice 0..3, hw x hh */
    VQHIP_CACAO_PLANE_PING = 2,      /* (occlusion, packed edges), R8G8_UNORM, as CSGenerateQ2 wrote them: slice 0..3, hw x hh */
    VQHIP_CACAO_PLANE_PONG = 3,      /* the same after the edge-sensitive blur (not written when blurPassCount == 0) */
    /* vqhip_adaptive_cacao only (below): iw = (hw + 1) / 2, ih = (hh + 1) / 2; slice 0, mip 0 */
    VQHIP_CACAO_PLANE_IMPORTANCE = 4,        /* the importance map after CSPostprocessImportanceMapB, R8_UNORM, iw x ih, dense rows */
    VQHIP_CACAO_PLANE_IMPORTANCE_PONG = 5,   /* the map after CSPostprocessImportanceMapA, the same shape */
    VQHIP_CACAO_PLANE_LOAD_COUNTER = 6       /* one uint32: the sum CSPostprocessImportanceMapB's InterlockedAdd left */
} vqhip_cacao_plane;
#define VQHIP_CACAO_MAX_DIM 16384
#define VQHIP_CACAO_MAX_BLUR_PASSES 8
/* The work buffer of a width x height frame, hw = (width + 1) / 2, hh = (height + 1) / 2: every plane above, dense rows, slice after slice.
 * _plane_offset_bytes: where slice `slice` (mip `mip` of DEPTHS; 0 otherwise) starts, so that a caller or a test can address every intermediate.
 * Both return 0 for arguments out of range (offset 0 is also the valid start of DEPTHS slice 0 mip 0). Host-only. */
VQHIP_API size_t vqhip_cacao_work_bytes(int width, int height);
VQHIP_API size_t vqhip_cacao_plane_offset_bytes(int width, int height, int plane, int slice, int mip);
/*   depth     : R32F [height] rows of depthPitchBytes bytes (a multiple of 4, >= 4 * width)
 *   normals   : normalFmt R10G10B10A2_UNORM (4 B per pixel) or RGBA32F (16 B), world space as (n + 1) / 2; rows of normalPitchBytes bytes (a multiple of the pixel size)
 *   shared / perPass[4] : the constant blocks; their buffer sizes must be those of this frame and perPass[i].PassIndex == i
 *   qualityLevel : VQHIP_CACAO_QUALITY_HIGH; blurPassCount 0..8 (0: the blur is skipped and CSApply reads the ping planes)
 *   work      : vqhip_cacao_work_bytes(width, height) bytes, 256-byte aligned, not overlapping the other buffers
 *   ao        : R8_UNORM [height] rows of aoPitchBytes bytes (>= width); bytes between width and the pitch are not written
 * Returns VQHIP_ERR_INVALID_ARG for NULL pointers, non-positive sizes, pitches or workBytes too small, constants of another frame size;
 * VQHIP_ERR_UNSUPPORTED for another quality level, normal format or a frame above VQHIP_CACAO_MAX_DIM — without launching anything. */
VQHIP_API int vqhip_cacao(vqhip_ctx* ctx, void* stream, const float* depth, size_t depthPitchBytes, const void* normals, int normalFmt, size_t normalPitchBytes,
        const VQ_CacaoConstants* shared, const VQ_CacaoConstants perPass[4], int qualityLevel, int blurPassCount,
        void* work, size_t workBytes, uint8_t* ao, size_t aoPitchBytes, int width, int height);

/* ---- Quality HIGHEST, FFX_CACAO_DEFAULT_SETTINGS' own level (ffx_cacao.h:72-90; AmbientOcclusion.cpp:38 constructs the pass from them): the pipeline above with
 * an adaptive stage in place of CSGenerateQ2 (FFX_CACAO_D3D12Draw, ffx_cacao_impl.cpp:1950-2150). docs/DESIGN_DETAILS.md §7.15; tests/cacao_adaptive_ref.py states
 * it in numpy.
 *   prepare depths, prepare normals (as above) -> CSGenerateQ3Base x 4 (5 taps; (obscurance, weight / 20) into the PONG slices) -> CSGenerateImportanceMap ->
 *   CSPostprocessImportanceMapA -> CSPostprocessImportanceMapB (+ the load counter) -> CSGenerateQ3 x 4 (1 .. 27 more taps per texel, by importance; into PING) ->
 *   CSEdgeSensitiveBlur<blurPassCount> x 4 -> CSApply,
 * ten kernels on `stream` (nine when blurPassCount == 0), no host synchronisation, no allocation, no memset: a lane of the first importance kernel clears the counter.
 * It is an entry point of its own because its work buffer is larger: HIGH's layout is the prefix (the same offsets for DEPTHS, NORMALS, PING and PONG), and three
 * planes follow, each on a 256-byte boundary: VQHIP_CACAO_PLANE_IMPORTANCE, _IMPORTANCE_PONG and _LOAD_COUNTER; iw x ih are the constants' ImportanceMapDimensions. */
/* After a call with blurPassCount == 0 the PONG slices hold the base pass's output (R8G8_UNORM: obscurance, weight / 20); with a blur they hold the blurred planes,
 * as at HIGH (the blur overwrites the base values, as it does in the source). PING holds CSGenerateQ3's output either way.
 * _plane_offset_bytes takes the seven plane ids; slice and mip must be 0 for the three new ones. Both size functions return 0 for arguments out of range. Host-only. */
VQHIP_API size_t vqhip_adaptive_cacao_work_bytes(int width, int height);
VQHIP_API size_t vqhip_adaptive_cacao_plane_offset_bytes(int width, int height, int plane, int slice, int mip);
/* Arguments and refusals as vqhip_cacao's, without qualityLevel; work is vqhip_adaptive_cacao_work_bytes(width, height) bytes, and the constants'
 * ImportanceMapDimensions must be (iw, ih) too. The blocks' LoadCounterAvgDiv and AdaptiveSampleCountLimit (settings.adaptiveQualityLimit) are used as handed over. */
VQHIP_API int vqhip_adaptive_cacao(vqhip_ctx* ctx, void* stream, const float* depth, size_t depthPitchBytes, const void* normals, int normalFmt, size_t normalPitchBytes,
        const VQ_CacaoConstants* shared, const VQ_CacaoConstants perPass[4], int blurPassCount,
        void* work, size_t workBytes, uint8_t* ao, size_t aoPitchBytes, int width, int height);

/* ---- Shadow-map rasteriser: VQRenderer::RenderDirectionalShadowMaps / RenderSpotShadowMaps / RenderPointShadowMaps (SceneRendering.cpp:996-1263) ==
 * ShadowDepthPass.hlsl drawn through the shadow PSOs (PipelineStateObjects.cpp:1697-1741): indexed, instanced triangle lists in, the R32F slices of
 * vqhip_shadowmaps out. ALL views of a frame in one call (the engine: 37 clear-and-draw sequences). docs/DESIGN_DETAILS.md §7.16 is the normative statement
 * (R1 vertex stage, R2 clipping against w >= 2^-24 and the four side planes — no z planes: DepthClipEnable is FALSE —, R3 viewport and 16.8 snap, R4 top-left
 * coverage in int64, R5 z/w and R6 LINEAR_DEPTH interpolation); tests/shadow_raster_ref.py states it in numpy. R2, R5 and R6 are UNPINNED against a D3D12
 * device (docs/WARP_CALIBRATION.md §5).
 * The ENABLE_ALPHA_MASK variant is vqhip_shadow_masked_depth (below). Out of scope: the tessellation variants (the heightmap variant is vqhip_displace_meshes in front of this call; the null heightmap's + 0.0f is kept), wireframe.
 * Three kernels on `stream` (plus one setup launch per further ~700 draws): counters, triangle setup, tile fill. No allocation, no memset node; the call clears
 * each map itself (uncovered texels read 1.0; a view with numDraws == 0 yields all 1.0). View and draw descriptors are host memory, consumed before the call
 * returns; meshes and matrices are device memory, read when the kernels run. The maps of one call must not overlap each other, the work buffer or the inputs. */
typedef enum vqhip_cull_mode { VQHIP_CULL_NONE = 0, VQHIP_CULL_FRONT = 1, VQHIP_CULL_BACK = 2 } vqhip_cull_mode;   /* iFaceCull, DrawData.h:161 */
typedef struct vqhip_shadow_mesh {      /* device pointers */
    const void* positions;  uint32_t strideBytes;   /* float3 at offset 0 of each vertex; 12 (tight) or the engine's 44-byte vertex, any multiple of 4 >= 12 */
    uint32_t    numVertices;                        /* a triangle with an index >= numVertices is dropped */
    const void* indices;    int32_t indexBits;      /* 16 | 32 */
    uint32_t    numIndices;                         /* multiple of 3: triangle list */
} vqhip_shadow_mesh;
typedef struct vqhip_shadow_draw {      /* one DrawIndexedInstanced of DrawShadowViewMeshList */
    vqhip_shadow_mesh mesh;
    const VQ_matrix* matWorldViewProj;  /* device, [numInstances]: PerObjectShadowData.matWorldViewProj */
    const VQ_matrix* matWorld;          /* device, [numInstances]: PerObjectShadowData.matWorld; may be NULL when the view is not linear-depth */
    uint32_t numInstances;              /* 1 .. 128 (MAX_INSTANCE_COUNT__SHADOW_MESHES) */
    int32_t  cullMode;                  /* VQHIP_CULL_NONE | _FRONT | _BACK  (iFaceCull) */
} vqhip_shadow_draw;
typedef struct vqhip_shadow_view {
    float*  depth;  size_t pitchBytes;  int32_t dim;   /* one dim x dim R32F slice of vqhip_shadowmaps; pitch 0 = dense */
    int32_t linearDepth;                               /* 0: z/w (directional, spot); 1: LINEAR_DEPTH (point faces) */
    VQ_float3 cameraPosition;  float farPlane;         /* PerShadowViewData; read only when linearDepth */
    const vqhip_shadow_draw* draws;  int32_t numDraws; /* host array */
} vqhip_shadow_view;
#define VQHIP_SHADOW_MAX_DIM 8192
#define VQHIP_SHADOW_MAX_VIEWS 64
#define VQHIP_SHADOW_MAX_INSTANCES 128
/* Bytes of work for a call whose views draw `instancedTriangles` triangles in all (sum over views and draws of numIndices / 3 * numInstances): six records per
 * triangle (a triangle clipped by five planes is a fan of at most six). 0 for numViews outside 1 .. 64 or a size that does not fit size_t. Host-only. */
VQHIP_API size_t vqhip_shadow_depth_work_bytes(uint64_t instancedTriangles, int numViews);
/* Returns VQHIP_ERR_INVALID_ARG — launching nothing, leaving the maps untouched — for NULL pointers (ctx, views, a view's depth, draws with numDraws > 0, a
 * mesh's positions or indices, matWorldViewProj, matWorld of a linear-depth view, work), numViews outside 1 .. 64, dim outside 1 .. 8192, a pitch below 4 * dim or not
 * a multiple of 4, numDraws < 0, an indexBits other than 16 / 32, numIndices % 3 != 0, a stride below 12 or not a multiple of 4, numInstances outside 1 .. 128, an
 * unknown cullMode, positions or matrices not 4-byte aligned, indices not aligned to their size, work not 256-byte aligned or workBytes below vqhip_shadow_depth_work_bytes of the
 * call's own triangle count; VQHIP_ERR_UNSUPPORTED for more than 20 000 draws or 2^31 triangle lanes in one call. */
VQHIP_API int vqhip_shadow_depth(vqhip_ctx* ctx, void* stream, const vqhip_shadow_view* views, int numViews, void* work, size_t workBytes);

/* ---- Main-view depth pre-pass: VQRenderer::RenderDepthPrePass (SceneRendering.cpp:1265-1363) == DepthPrePass.hlsl drawn through FDepthPrePassPSOs
 * (PipelineStateObjects.cpp:1580-1635): the rasteriser above with the four things the Z pre-pass changes — a rectangular viewport {0, 0, W, H, 0, 1}, DepthClipEnable
 * TRUE (two z planes), SampleDesc.Count 1 or 4 (D3D's standard 4x pattern, coverage per sample), and DepthFunc LESS with depth writes on, whose winner the call can
 * report. docs/DESIGN_DETAILS.md §7.17 is the normative statement (V1 vertex stage = R1, V2 clipping against seven planes, V3 viewport, V4 sample positions, V5
 * per-sample z/w and the depth test as one 64-bit minimum); tests/scene_depth_ref.py states it in numpy. V2's z planes (a guard band is as legal), V4's sample
 * positions and V5's interpolation precision are UNPINNED against a D3D12 device (docs/WARP_CALIBRATION.md §5).
 * The ENABLE_ALPHA_MASK variant is vqhip_scene_masked_depth (below). Out of scope: the tessellation variants (the heightmap variant is vqhip_displace_meshes in front of this call; the null heightmap's + 0.0f is kept), wireframe, the pass's normals target
 * (vqhip_scene_normals_from_materials writes it from interpolants). The interpolant planes are vqhip_scene_interpolants' (below), from this call's owner planes.
 * Outputs (pitches in pixels, coverage_pitch in bytes, 0 = dense = width; every pointer but depth may be NULL):
 *   depth           samples 1: float [height][pitch] — the `depth` of vqhip_depth_hierarchy; samples 4: float [height][pitch][4], 16-byte aligned — the depth_ms of
 *                   vqhip_msaa_resolve_surfaces. An uncovered sample holds 1.0.
 *   primitive       uint32, the shape (and at 4x the alignment) of depth: the sequence number of the primitive that owns the sample, 0xFFFFFFFF for none.
 *                   q = first(draw) + instance * numTris + tri, first(draw) = the instanced triangles of the draws before: D3D's submission order. Among the
 *                   fragments of a sample the smallest depth wins, and on equal depth bits the smallest q (LESS rejects the later equal fragment); a fragment whose
 *                   saturated depth is 1.0 fails against the clear value and leaves depth and primitive untouched.
 *   coverage[k], layerPrimitive[k]  (samples 4 only, k < layers <= 4): uint8 [height][coverage_pitch] masks in the representation vqhip_gbuffer_msaa and
 *                   vqhip_msaa_surfaces read, and uint32 [height][pitch]. Per pixel, walking samples 0, 1, 2, 3: a sample with no owner belongs to no layer; a
 *                   sample whose owner is the layerPrimitive of an open layer sets bit s of that layer's mask; otherwise it opens the next layer. Unused layers
 *                   hold mask 0 and primitive 0xFFFFFFFF; bits 4-7 are 0; the masks are disjoint. A pixel has at most four owners: when `layers` is smaller than
 *                   the pixel needs, the owners beyond it are DROPPED FROM THE LAYER PLANES ONLY (their samples are in no mask) — depth and primitive never change.
 * Three kernels on `stream` (plus one setup launch per further ~700 draws): counter, triangle setup, tile fill. No allocation, no memset node, no readback; the
 * call clears its own outputs (numDraws == 0 yields all 1.0 / 0xFFFFFFFF / mask 0). Draw descriptors are host memory, consumed before the call returns; meshes and
 * matrices are device memory, read when the kernels run. The outputs must not overlap the work buffer. Option raster_tile 64 is honoured at samples 1; at samples 4
 * the tile stays 32 x 32 (64 x 64 x 4 keys would be 128 KiB of LDS). */
typedef struct vqhip_scene_depth_draw {  /* one DrawIndexedInstanced of RenderDepthPrePass */
    vqhip_shadow_mesh mesh;
    const VQ_matrix* matWorldViewProj;  /* device, [numInstances]: PerObjectData.matWorldViewProj */
    uint32_t numInstances;              /* 1 .. 64 (MAX_INSTANCE_COUNT__SCENE_MESHES) */
    int32_t  cullMode;                  /* VQHIP_CULL_NONE | _FRONT | _BACK */
} vqhip_scene_depth_draw;
typedef struct vqhip_scene_depth_targets {   /* device pointers */
    float*    depth;
    uint32_t* primitive;                /* or NULL */
    uint8_t*  coverage[4];              /* [k] or NULL, k < layers */
    uint32_t* layerPrimitive[4];        /* [k] or NULL, k < layers */
    int32_t   layers;                   /* 0 .. 4; must be 0 when samples == 1 */
    int32_t   pitch;                    /* pixels per row of depth, primitive and layerPrimitive; 0 = width */
    int32_t   coverage_pitch;           /* bytes per row of coverage; 0 = width */
    int32_t   reserved;                 /* 0 */
} vqhip_scene_depth_targets;
VQHIP_STATIC_ASSERT(sizeof(vqhip_scene_depth_draw) == 48 && offsetof(vqhip_scene_depth_draw, numInstances) == 40, "vqhip_scene_depth_draw layout");
VQHIP_STATIC_ASSERT(sizeof(vqhip_scene_depth_targets) == 96 && offsetof(vqhip_scene_depth_targets, layers) == 80, "vqhip_scene_depth_targets layout");
#define VQHIP_SCENE_DEPTH_MAX_DIM 8192
#define VQHIP_SCENE_DEPTH_MAX_INSTANCES 64
#define VQHIP_SCENE_DEPTH_MAX_LAYERS 4
/* Bytes of work for a call that draws `instancedTriangles` triangles (sum over draws of numIndices / 3 * numInstances): eight records per triangle (a triangle
 * clipped by seven planes is a fan of at most eight). 0 for a count of 2^29 or more, or a size that does not fit size_t. Host-only. */
VQHIP_API size_t vqhip_scene_depth_work_bytes(uint64_t instancedTriangles);
/* Returns VQHIP_ERR_INVALID_ARG — launching nothing, leaving the outputs untouched — for NULL pointers (ctx, out, out->depth, draws with numDraws > 0, a mesh's
 * positions or indices, matWorldViewProj, work), samples other than 1 or 4, layers outside 0 .. 4 or not 0 at samples 1, width or height outside 1 .. 8192, a pitch
 * below width (either kind) or negative, reserved != 0, depth or primitive not 4-byte (samples 1) / 16-byte (samples 4) aligned, layerPrimitive not 4-byte aligned,
 * numDraws < 0, an indexBits other than 16 / 32, numIndices % 3 != 0, a stride below 12 or not a multiple of 4, numInstances outside 1 .. 64, an unknown cullMode,
 * positions or matrices not 4-byte aligned, indices not aligned to their size, work not 256-byte aligned, workBytes below vqhip_scene_depth_work_bytes of the call's
 * own triangle count, or an output that overlaps the work buffer; VQHIP_ERR_UNSUPPORTED for 2^29 or more instanced triangles (q must stay below the no-owner value, which
 * alone would allow up to 2^32 - 2; eight records per triangle must also fit the 32-bit record counter) or more than 20 000 draws in one call. */
VQHIP_API int vqhip_scene_depth(vqhip_ctx* ctx, void* stream, const vqhip_scene_depth_draw* draws, int numDraws, int width, int height, int samples,
        const vqhip_scene_depth_targets* out, void* work, size_t workBytes);

/* ---- The lit draw's interpolants from meshes: the vertex stage of ForwardLighting.hlsl (TransformVertex, :143-188) and the perspective-correct interpolation of
 * PSInput at the pixel centre, as a visibility-buffer resolve over the owner plane vqhip_scene_depth writes. With it the chain meshes -> vqhip_scene_depth ->
 * vqhip_scene_interpolants -> vqhip_gbuffer_from_materials / vqhip_forward_lighting_from_materials[_mrt] / vqhip_scene_normals_from_materials runs inside the
 * library, at 1x and — one call per layer — at 4x MSAA. docs/DESIGN_DETAILS.md §7.18 is the normative statement (I0 owner lookup, I1 vertex stage in binary32
 * whatever vqhip_set_arithmetic says, I2 weights at the pixel centre and I3 attributes in binary64, rounded once); tests/scene_interp_ref.py states it in numpy.
 * I2 and I3 are UNPINNED against a D3D12 device (docs/WARP_CALIBRATION.md §5): D3D leaves interpolation precision to the device.
 *   draws   the draw list of the vqhip_scene_depth call that produced `owner`: the same order, index counts and instance counts — that gives q its meaning.
 *   owner   uint32 [height][owner_pitch_px] (0 = width), 4-byte aligned: `primitive` at 1x, one `layerPrimitive[k]` at 4x. Any content is safe: a pixel whose q
 *           is 0xFFFFFFFF, at or beyond the call's instanced triangles, or whose triangle has an index >= numVertices has NO OWNER and receives
 *           ip0 = ip1 = (0, 0, 0, 0), ip2 = (0, 0, 0, asfloat(int32 -1)) and, if asked for, svPositionCurr = svPositionPrev = (0, 0, 0, 1).
 *   out     ip0 = (world, uv.x), ip1 = (N, uv.y), ip2 = (T, asfloat(materialIndex)): the planes of vqhip_interpolants; svPositionCurr = clip, svPositionPrev =
 *           the previous frame's clip: the planes of vqhip_psmain_targets (both or neither). A NaN is stored as 0x7FC00000. At 4x a pixel centre outside its
 *           owner extrapolates, as D3D does for a PSInput without `centroid`.
 *   work    vqhip_scene_interpolants_work_bytes(numDraws) bytes, 256-byte aligned: the device home of the draw table (any pixel may look up any draw).
 * The table is staged through the context's constant ring (one table-copy launch per ring slot of 556 draws), then ONE kernel (a wave whose 64 pixels share
 * one owner fetches it once; option interp_form lane switches that path off, same bits). No allocation, no memset node, no
 * readback. Draw descriptors are host memory, consumed before the call returns; meshes and matrices are device memory, read when the kernel runs. Not modelled:
 * tessellation (the heightmap variant is vqhip_displace_meshes in front of this call; the null heightmap's float3 add is kept). The alpha mask needs nothing here: vqhip_scene_masked_depth keeps discarded fragments out of
 * the owner plane, and the shading entry points repeat the discard. vqhip_gbuffer_from_materials still takes its uv LOD from neighbouring pixels
 * of the planes, so at primitive edges it differs from a helper-lane derivative. vqhip_scene_quad_interpolants and the _quad producers (below, after the
 * masked-depth section) carry the helper lanes' uv from this resolve to the producers and close that gap. */
typedef struct vqhip_scene_surface_draw {   /* one DrawIndexedInstanced of the lit pass */
    vqhip_shadow_mesh mesh;                 /* the engine's vertex: position @0, normal @12, tangent @24, uv @36; strideBytes >= 44, a multiple of 4 */
    const VQ_matrix* matWorldViewProj;      /* device, [numInstances]: PerObjectLightingData */
    const VQ_matrix* matWorld;
    const VQ_matrix* matNormal;
    const VQ_matrix* matWorldViewProjPrev;  /* may be NULL when no svPosition plane is asked for */
    uint32_t numInstances;                  /* 1 .. 64 */
    int32_t  materialIndex;                 /* >= 0; written to ip2.w */
} vqhip_scene_surface_draw;
typedef struct vqhip_scene_interpolant_targets {   /* device pointers, float4 planes, 16-byte aligned */
    void* ip0; void* ip1; void* ip2;               /* the planes of vqhip_interpolants */
    void* svPositionCurr; void* svPositionPrev;    /* both or neither: the planes of vqhip_psmain_targets */
    int32_t pitch, sv_pitch;                       /* pixels per row of ip0..2 / of the sv planes; 0 = width */
} vqhip_scene_interpolant_targets;
VQHIP_STATIC_ASSERT(sizeof(vqhip_scene_surface_draw) == 72 && offsetof(vqhip_scene_surface_draw, matWorldViewProj) == 32 &&
                    offsetof(vqhip_scene_surface_draw, numInstances) == 64, "vqhip_scene_surface_draw layout");
VQHIP_STATIC_ASSERT(sizeof(vqhip_scene_interpolant_targets) == 48 && offsetof(vqhip_scene_interpolant_targets, svPositionCurr) == 24 &&
                    offsetof(vqhip_scene_interpolant_targets, pitch) == 40, "vqhip_scene_interpolant_targets layout");
/* Bytes of work for a call of numDraws draws: 80 per draw, rounded up to 256 (256 for numDraws == 0). 0 for numDraws < 0. Host-only. */
VQHIP_API size_t vqhip_scene_interpolants_work_bytes(int numDraws);
/* Returns VQHIP_ERR_INVALID_ARG — launching nothing, leaving the outputs untouched — for NULL pointers (ctx, out, ip0, ip1, ip2, owner, work, draws with
 * numDraws > 0, a mesh's positions or indices, matWorldViewProj, matWorld, matNormal), numDraws < 0, exactly one of the two sv planes, sv planes asked for while a
 * draw has matWorldViewProjPrev == NULL, width or height outside 1 .. 8192, a pitch (owner, ip, sv) that is negative or below width, a target not 16-byte aligned,
 * owner not 4-byte aligned, a stride below 44 or not a multiple of 4, an indexBits other than 16 / 32, numIndices % 3 != 0, numInstances outside 1 .. 64,
 * materialIndex < 0, positions or matrices not 4-byte aligned, indices not aligned to their size, work not 256-byte aligned, workBytes below
 * vqhip_scene_interpolants_work_bytes(numDraws), or an output that overlaps the work buffer or the owner plane; VQHIP_ERR_UNSUPPORTED for more than 20 000 draws with numIndices > 0 (empty draws are not counted,
 * though the work size is that of numDraws)
 * or 2^29 or more instanced triangles in one call (the limits of vqhip_scene_depth). */
VQHIP_API int vqhip_scene_interpolants(vqhip_ctx* ctx, void* stream, const vqhip_scene_surface_draw* draws, int numDraws, int width, int height,
        const uint32_t* owner, int owner_pitch_px, const vqhip_scene_interpolant_targets* out, void* work, size_t workBytes);

/* ---- Alpha-tested geometry in the depth pre-pass and the shadow maps: the "_AlphaMasked" PSO permutations of both passes (PipelineStateObjects.cpp:1617, 1683,
 * 1731, 1787; drawn by SceneRendering.cpp:1008-1030, 1318-1337), i.e. DepthPrePass.hlsl:155-161 and ShadowDepthPass.hlsl:136-140 compiled with ENABLE_ALPHA_MASK.
 * vqhip_scene_masked_depth and vqhip_shadow_masked_depth are SUPERSETS of vqhip_scene_depth and vqhip_shadow_depth: outputs, clears, q numbering, limits and
 * refusal rules are theirs, opaque and masked draws mix freely in one call and share one q sequence (vqhip_scene_interpolants consumes the owner planes
 * unchanged), and a call without a masked draw launches the very kernels of the opaque entry point. docs/DESIGN_DETAILS.md §7.19 is the normative statement;
 * tests/masked_depth_ref.py states it in numpy:
 *   M1  the pixel shader runs once per (primitive, pixel) at the pixel centre — at 4x without `centroid`: a pixel with any covered sample evaluates at its centre
 *       even when the centre lies outside the triangle (extrapolation, as §7.18) — and a discard removes all of that primitive's samples in the pixel. Shadow
 *       maps: pixel = texel.
 *   M2  the uv at the pixel centre is §7.18 I2 / I3: binary64 weights from the UNCLIPPED triangle's binary32 clip-space (x, y, w), one rounding to binary32; the
 *       decision depends on (q, pixel) only, never on the fan piece of a clipped triangle that covers the sample.
 *   M3  scene depth: uv * uvScaleOffset.xy + uvScaleOffset.zw as vqhip_gbuffer_from_materials evaluates it; Sample(AnisoSampler) = that call's isotropic trilinear
 *       WRAP fetch (bias 0); the derivatives come from the 2 x 2 quad aligned to even pixel coordinates, whose other lanes are HELPER LANES: the same primitive
 *       evaluated by M2 at (i ^ 1, j) and (i, j ^ 1), covered or not, inside the viewport or not. Discard iff HasDiffuseMap(textureConfig) && a < 0.01f.
 *   M4  shadow: the raw vertex uv (texScaleBias feeds only the heightmap), SampleLevel(.., 0) = the bilinear WRAP fetch of level 0, discard iff a < 0.01f. There
 *       is NO HasDiffuseMap test in that shader: a masked draw whose diffuse SRV is null (texDiffuseAlpha->texels == NULL) samples 0 and LOSES EVERY FRAGMENT.
 *       In scene depth a NULL texels with the diffuse bit set discards everything as well; with the bit clear nothing is discarded.
 *   M5  coverage, top-left rule, depth interpolation, saturate, the < 1.0 rejection and the 64-bit minimum are unchanged: a discarded fragment never reaches the minimum.
 * M2's precision and M3's derivative form are UNPINNED against a D3D12 device (docs/WARP_CALIBRATION.md §5).
 * A masked draw's mesh is the engine's vertex: uv at byte 36, strideBytes >= 44. Textures are vqhip_texture2d: RGBA8_UNORM mip chains in device memory; the
 * descriptors (materials, texDiffuseAlpha) are HOST memory, consumed before the call returns.
 * (The names put `masked` before `depth` so that the prefixes vqhip_scene_depth* / vqhip_shadow_depth* keep denoting the opaque pair alone.)
 * Out of scope: the tessellation variants (the heightmap variant is vqhip_displace_meshes in front of these calls), the separate texAlphaMask map (t3: bound, not read by these shaders), the Outline pass's
 * masked permutation (the ObjectID pass's rides on this call: vqhip_object_ids, below).
 * Work: the opaque call's layout is the prefix; behind it a device table of the draws' textures (48 bytes per draw, staged through the constant ring like
 * vqhip_scene_interpolants' table: one table-copy launch per ring slot) and one 64-byte side record per masked instanced triangle (the unclipped clip-space
 * x, y, w and the uv of its three vertices, the draw's table slot). Kernels with a masked draw: counter(s), table copy, setup, fill. No allocation, no memset
 * node, no readback. */
typedef struct vqhip_scene_masked_depth_draw {
    vqhip_scene_depth_draw draw;
    const vqhip_material*  material;   /* HOST, or NULL. Masked iff non-NULL and (texDiffuse.reserved & VQHIP_MATERIAL_ALPHA_MASKED). Read: data.uvScaleOffset, data.textureConfig, texDiffuse */
} vqhip_scene_masked_depth_draw;
typedef struct vqhip_shadow_masked_draw {
    vqhip_shadow_draw draw;
    const vqhip_texture2d* texDiffuseAlpha;   /* HOST, or NULL = the opaque PSO. Non-NULL = the masked PSO, whatever `reserved` holds; texels NULL = null SRV (M4) */
} vqhip_shadow_masked_draw;
typedef struct vqhip_shadow_masked_view {      /* vqhip_shadow_view with draws of the type above */
    float*  depth;  size_t pitchBytes;  int32_t dim;
    int32_t linearDepth;
    VQ_float3 cameraPosition;  float farPlane;
    const vqhip_shadow_masked_draw* draws;  int32_t numDraws;
} vqhip_shadow_masked_view;
VQHIP_STATIC_ASSERT(sizeof(vqhip_scene_masked_depth_draw) == 56 && offsetof(vqhip_scene_masked_depth_draw, material) == 48, "vqhip_scene_masked_depth_draw layout");
VQHIP_STATIC_ASSERT(sizeof(vqhip_shadow_masked_draw) == 64 && offsetof(vqhip_shadow_masked_draw, texDiffuseAlpha) == 56, "vqhip_shadow_masked_draw layout");
VQHIP_STATIC_ASSERT(sizeof(vqhip_shadow_masked_view) == sizeof(vqhip_shadow_view) && offsetof(vqhip_shadow_masked_view, draws) == offsetof(vqhip_shadow_view, draws),
                    "vqhip_shadow_masked_view layout");
/* Bytes of work: vqhip_scene_depth_work_bytes(instancedTriangles) + 48 per draw and 64 per masked instanced triangle (the triangles of the draws that are masked
 * by the rule above), each part rounded up to 256. 0 where the opaque function returns 0, for maskedInstancedTriangles > instancedTriangles, or numDraws < 0. Host-only. */
VQHIP_API size_t vqhip_scene_masked_depth_work_bytes(uint64_t instancedTriangles, uint64_t maskedInstancedTriangles, int numDraws);
/* vqhip_scene_depth's refusals (with the work size above), and VQHIP_ERR_INVALID_ARG — launching nothing, leaving the outputs untouched — for a masked draw whose
 * strideBytes is below 44, whose texDiffuse has texels and a width or height outside 1 .. 16384, mips < 1 or more than vqhip_mip_level_count(width, height), or
 * texels that are not 4-byte aligned. */
VQHIP_API int vqhip_scene_masked_depth(vqhip_ctx* ctx, void* stream, const vqhip_scene_masked_depth_draw* draws, int numDraws, int width, int height, int samples,
        const vqhip_scene_depth_targets* out, void* work, size_t workBytes);
/* numDraws: the draws of all views. Otherwise as above over vqhip_shadow_depth_work_bytes(instancedTriangles, numViews). */
VQHIP_API size_t vqhip_shadow_masked_depth_work_bytes(uint64_t instancedTriangles, uint64_t maskedInstancedTriangles, int numViews, int numDraws);
/* vqhip_shadow_depth's refusals (with the work size above), the masked draw's refusals of vqhip_scene_masked_depth, and VQHIP_ERR_UNSUPPORTED for more than
 * 10 000 draws in a call that has a masked draw (the texture table and the larger draw jobs share the constant ring with the view table) or 2^32 - 1 or more
 * masked instanced triangles in one call. */
VQHIP_API int vqhip_shadow_masked_depth(vqhip_ctx* ctx, void* stream, const vqhip_shadow_masked_view* views, int numViews, void* work, size_t workBytes);
#define VQHIP_MASK_TEXTURE_MAX_DIM 16384

/* ---- Helper-lane uv derivatives for the lit draw (docs/DESIGN_DETAILS.md §7.20; tests/quad_interp_ref.py states it in numpy). D3D takes the implicit derivatives
 * of Texture2D.Sample from the 2 x 2 quad aligned to even pixel coordinates, and the quad's other lanes run the OWN primitive as helper lanes — covered or not,
 * inside the viewport or not. vqhip_scene_masked_depth already evaluates its discard that way (M3); the producers of vqhip_interpolants planes read the planes'
 * neighbours instead, which belong to whatever owns those pixels. The calls below carry the helper lanes' uv from the resolve to the producers, so that the
 * pre-pass and the lit draw take the same derivative — and the same alpha-test decision — for every (primitive, pixel).
 *   Q1  vqhip_scene_quad_interpolants = vqhip_scene_interpolants (the five planes hold exactly what that call writes; its work size, limits and refusals) + one
 *       float4 plane quadUV [height][quad_pitch]: for an owned pixel (i, j) (I0's rule) quadUV = (u_h, v_h, u_v, v_v), the owner triangle's vertex uv at the centres
 *       of pixels (i ^ 1, j) and (i, j ^ 1) by §7.18 I2 / I3 (weights and quotients afresh in binary64 at that centre, one rounding, NaN = 0x7FC00000). i ^ 1 may
 *       equal width and j ^ 1 height; the triangle need not cover the partner; at 4x the own centre may already lie outside it. A pixel with no owner holds
 *       (0, 0, 0, 0). Both interp_form values give the same bits.
 *   Q2  the _quad producers = their siblings with ddx = own - helper_h on odd i, helper_h - own on even i (ddy alike with j and helper_v), where helper =
 *       uv_helper * uvScaleOffset.xy + uvScaleOffset.zw rounded as the own uv' is. No material comparison and no image-bounds test: a helper lane always belongs
 *       to the own primitive. Footprint, LOD, taps, normalMapMipBias, the discard and its -1 into ip2.w, SSAO and both arithmetic readings are the siblings'.
 *       quadUV: 16-byte aligned, quad_pitch_px pixels per row (0 = in->row_pitch_px), smaller than 4 GiB.
 * The derivative form is the UNPINNED M3 form (docs/WARP_CALIBRATION.md §5). vqhip_gbuffer_from_materials and its siblings keep the neighbour rule for callers
 * who bring planes from a rasteriser of their own. */
typedef struct vqhip_scene_quad_targets {
    vqhip_scene_interpolant_targets planes;   /* as for vqhip_scene_interpolants */
    void*   quadUV;                            /* float4 [height][quad_pitch], 16-byte aligned, required */
    int32_t quad_pitch;                        /* pixels per row, 0 = width */
    int32_t pad_;
} vqhip_scene_quad_targets;
VQHIP_STATIC_ASSERT(sizeof(vqhip_scene_quad_targets) == 64 && offsetof(vqhip_scene_quad_targets, quadUV) == 48 && offsetof(vqhip_scene_quad_targets, quad_pitch) == 56,
                    "vqhip_scene_quad_targets layout");
/* work: vqhip_scene_interpolants_work_bytes(numDraws). vqhip_scene_interpolants' refusals, and VQHIP_ERR_INVALID_ARG — launching nothing, leaving the outputs
 * untouched — for quadUV NULL or not 16-byte aligned, quad_pitch negative or below width, quadUV overlapping the owner plane, the work buffer or another output. */
VQHIP_API int vqhip_scene_quad_interpolants(vqhip_ctx* ctx, void* stream, const vqhip_scene_surface_draw* draws, int numDraws, int width, int height,
        const uint32_t* owner, int owner_pitch_px, const vqhip_scene_quad_targets* out, void* work, size_t workBytes);
/* The siblings' refusals, and VQHIP_ERR_INVALID_ARG for quadUV NULL or not 16-byte aligned, quad_pitch_px negative or below in->width, quadUV overlapping an
 * output (ip2 included: its w receives the discard's -1); VQHIP_ERR_UNSUPPORTED for a quadUV plane of 4 GiB or more. */
VQHIP_API int vqhip_gbuffer_from_materials_quad(vqhip_ctx* ctx, void* stream,
        const vqhip_interpolants* in, const vqhip_material* materials, int numMaterials,
        float fAmbientLightingFactor, const vqhip_ssao* ssao, const vqhip_gbuffer* out, const void* quadUV, int quad_pitch_px);
/* targets: as for vqhip_forward_lighting_from_materials_mrt; NULL = no extra targets */
VQHIP_API int vqhip_forward_lighting_from_materials_quad(vqhip_ctx* ctx, void* stream,
        const vqhip_interpolants* in, const vqhip_material* materials, int numMaterials, const vqhip_ssao* ssao,
        const VQ_PerFrameData* perFrame, const VQ_PerViewLightingData* perView,
        const VQ_PointLight* extraPoint, int numExtraPoint, const vqhip_envmap* env, const vqhip_shadowmaps* sm,
        void* out, int out_row_pitch_px, vqhip_format outFmt, const vqhip_psmain_targets* targets, const void* quadUV, int quad_pitch_px);
VQHIP_API int vqhip_scene_normals_from_materials_quad(vqhip_ctx* ctx, void* stream,
        const vqhip_interpolants* in, const vqhip_material* materials, int numMaterials,
        void* out, vqhip_format outFmt, int out_row_pitch_px, const void* quadUV, int quad_pitch_px);

/* ---- The ObjectID pass (picking): ObjectIDPass::RecordCommands (ObjectIDPass.cpp:160-278) == ObjectID.hlsl, as a visibility-buffer resolve over an owner plane.
 * The pass clears its own D32 depth to 1.0 and its R32G32B32A32_SINT target to (0, 0, 0, 0), sets the viewport {0, 0, W, H, 0, 1} at one sample, and draws the main
 * view's draw list with cull NONE for EVERY draw (the pass ignores iFaceCull), DepthClipEnable TRUE, depth LESS with writes; PSMain returns
 * int4(ObjID[instance].x, meshID, materialID, ObjID[instance].w). Its rasteriser therefore is vqhip_scene_depth (or vqhip_scene_masked_depth) at samples 1 with
 * every draw's cullMode set to VQHIP_CULL_NONE — the pass's OWN depth call, not the pre-pass's, whose cull modes differ — and its pixel shader is this call over that
 * call's `primitive` plane. docs/DESIGN_DETAILS.md §7.21 is the normative statement; tests/object_ids_ref.py states it in numpy:
 *   P0  q is decoded as §7.18 I0 decodes it: first(draw) = the instanced triangles of the draws before it, instance = (q - first(draw)) / numTris. A pixel whose q
 *       is 0xFFFFFFFF, or at or beyond the call's instanced triangles, receives (0, 0, 0, 0), the pass's clear colour; any other pixel receives
 *       (objID[instance].x, meshID, materialID, objID[instance].w). Any owner content is safe: no q moves a load or a store out of bounds.
 *   draws   host array, consumed before the call returns: the draw list of the depth call that produced `owner`, in its order, with its index and instance
 *           counts — that gives q its meaning. objID is device memory, read when the kernel runs. Draws with numIndices == 0 own no q.
 *   owner   uint32 [height][owner_pitch_px] (0 = width), 4-byte aligned.
 *   ids     int32 [height][ids_pitch_px][4] (0 = width), 16-byte aligned: the pass's render target; one texel of it is what the engine reads back (ReadBackPixel).
 *   work    vqhip_object_ids_work_bytes(numDraws) bytes, 256-byte aligned: the device home of the draw table.
 * The table is staged through the context's constant ring (one table-copy launch per ring slot, which holds well over 1 000 draws), then ONE kernel. No allocation, no memset node, no
 * readback. Option interp_form lane | wave selects the resolve's form as it does for vqhip_scene_interpolants (a wave whose 64 pixels share one q fetches the
 * draw once); both give the same bits. Default: wave for frames of 2^22 pixels or more, lane below (profiles/r22a_editor_passes.md).
 * The "_AlphaMasked" permutation (ObjectID.hlsl: discard where texDiffuse.Sample(AnisoSampler, uv * scale + offset).a < 0.01) rides on vqhip_scene_masked_depth's
 * rule M3: fragments that rule discards never reach the owner plane, so the ids show what lies behind the holes. One difference from ObjectID.hlsl: M3 discards
 * only when the material's HasDiffuseMap bit is set, ObjectID.hlsl has no such test. It shows only for a material flagged masked WITHOUT a diffuse map, which
 * Material::IsAlphaMasked excludes.
 * Out of scope: the tessellation variants of the pass (the heightmap variant is vqhip_displace_meshes in front of the depth call). The Outline pass is vqhip_outline (below); the Magnifier pass runs on the swap-chain image. */
typedef struct vqhip_object_id_draw {   /* one DrawIndexedInstanced of ObjectIDPass::RecordCommands, in the order of the depth call that produced `owner` */
    uint32_t numIndices, numInstances;  /* what that call drew: gives q its meaning (numIndices a multiple of 3, numInstances 1 .. 64) */
    const int32_t* objID;               /* device, int4 [numInstances], 4-byte aligned: PerObjectLightingData.ObjID; .x and .w are read */
    int32_t meshID, materialID;
} vqhip_object_id_draw;
VQHIP_STATIC_ASSERT(sizeof(vqhip_object_id_draw) == 24 && offsetof(vqhip_object_id_draw, objID) == 8 && offsetof(vqhip_object_id_draw, meshID) == 16,
                    "vqhip_object_id_draw layout");
/* Bytes of work for a call of numDraws draws: 32 per draw, rounded up to 256 (256 for numDraws == 0). 0 for numDraws < 0. Host-only. */
VQHIP_API size_t vqhip_object_ids_work_bytes(int numDraws);
/* Returns VQHIP_ERR_INVALID_ARG — launching nothing, leaving `ids` untouched — for NULL pointers (ctx, owner, ids, work, draws with numDraws > 0, a draw's objID),
 * numDraws < 0, width or height outside 1 .. 8192, a pitch that is negative or below width, ids not 16-byte aligned, owner or an objID not 4-byte aligned,
 * numInstances outside 1 .. 64, numIndices % 3 != 0, work not 256-byte aligned, workBytes below vqhip_object_ids_work_bytes(numDraws), or ids overlapping the owner
 * plane or the work buffer; VQHIP_ERR_UNSUPPORTED for more than 20 000 draws with numIndices > 0 or 2^29 or more instanced triangles in one call (the limits of
 * vqhip_scene_depth). */
VQHIP_API int vqhip_object_ids(vqhip_ctx* ctx, void* stream, const vqhip_object_id_draw* draws, int numDraws, int width, int height,
        const uint32_t* owner, int owner_pitch_px, int32_t* ids /* int4 [height][ids_pitch_px], 16-byte aligned */, int ids_pitch_px,
        void* work, size_t workBytes);

/* ---- The Outline pass (selection highlight): both passes of OutlinePass::RecordCommands (OutlinePass.cpp:247-405, Outline.hlsl; drawn last into scene colour,
 * SceneRendering.cpp:514) in one call, at 1 sample per pixel. The pass clears its own D24S8 (depth 1.0, stencil 0); each selected (mesh, material) pair is one
 * non-instanced draw with a constant buffer OutlineData. Every draw runs pass 0 ("RenderStencil": no render target, position = mul(mul(matProj, matWorldView),
 * vPosition), cull NONE, depth LESS with writes, stencil ALWAYS / REPLACE 1), then every draw runs pass 1 ("RenderOutline": the vertex moved in view space by
 * normalize(mul(matNormalView, float4(Normal, 0)).xyx) * 0.5 — the swizzle is .xyx in the reference and is kept as written —, depth ALWAYS without writes, stencil
 * NOT_EQUAL 1, blending off, PSMain returns the interpolated pow(Color, 2.2) into the RGBA16F target). docs/DESIGN_DETAILS.md §7.21 is the normative statement
 * (rules O1 .. O6); tests/outline_ref.py states it in numpy on top of tests/scene_depth_ref.py:
 *   O1  pass-0 vertex: P = (x, y + 0.0f, z); WVP.m[r][c] = ((WV[r][0]*Pr[0][c] + WV[r][1]*Pr[1][c]) + WV[r][2]*Pr[2][c]) + WV[r][3]*Pr[3][c], every operation
 *       rounded in binary32; clip[j] = §7.16 R1's mulPoint(P, WVP, j). Binary32 whatever vqhip_set_arithmetic says.
 *   O2  pass-1 vertex: V[j] = mulPoint(P, matWorldView, j) for j < 3; n[j] = ((N.x*M[0][j] + N.y*M[1][j]) + N.z*M[2][j]) + 0.0f*M[3][j] with M = matNormalView;
 *       v = (n[0], n[1], n[0]); viewNormal = the contract's as-written normalize(v); E = V + viewNormal * 0.5f componentwise (one product, one sum);
 *       clip[j] = mulPoint(E, matProj, j). A vertex with a non-finite clip component drops its triangle (both rules) — in particular a normal whose view-space x
 *       and y are both zero drops every pass-1 triangle that uses it.
 *   O3  both passes then run §7.17's V2 (seven planes), V3 (viewport, 16.8 snap) and R4 (int64 edge functions, top-left rule, the sample at the pixel centre). Cull NONE.
 *   O4  the mark: a pixel is marked iff some pass-0 fragment of ANY draw covers it with a V5 depth whose saturated value is below 1.0 (LESS against the cleared D24:
 *       every binary32 below 1.0 converts to a code below 0xFFFFFF). Order-independent.
 *   O5  the write: a pixel is written iff it is not marked and at least one pass-1 fragment covers it (depth ALWAYS: any depth counts). It receives the colour of
 *       the covering draw SUBMITTED LAST; the four channels are pow_(Color.c, 2.2f) in the contract's pow, each stored round-to-nearest-even as a half (a NaN as
 *       0x7E00 with its sign). Every other pixel of sceneColor keeps its bits.
 *   O6  the interpolated constant attribute equals the constant.
 * O1's matrix product, O4's D24 conversion and O6 are UNPINNED against a D3D12 device (docs/WARP_CALIBRATION.md §5), beside what §7.17 lists (V2, V5).
 * Kernels on `stream`: counter, one setup launch per ring slot of draws (both vertex stages, both clips, records of two kinds), one tile fill (a 32-bit LDS word
 * per pixel: a mark bit by atomic OR, 1 + the draw's number by atomic MAX — no order dependence), which also clears selection / writer. No allocation, no memset
 * node, no readback. Draw descriptors are host memory, consumed before the call returns; meshes and constant buffers are device memory, read when the kernels run.
 * numDraws == 0 leaves sceneColor untouched and clears selection / writer. Option raster_tile 64 is honoured.
 * Out of scope: 4x MSAA (the library has no per-sample scene colour: vqhip_forward_lighting_msaa shades and resolves in one kernel; it would take a sample-mask /
 * writer output here and an override input in that resolve), the pass's "_AlphaMasked" permutation, the tessellation variants (the heightmap variant is
 * vqhip_displace_meshes in front of this call; the null heightmap's + 0.0f is kept), the Magnifier pass. */
typedef struct VQ_OutlineData {  /* byte for byte the cbuffer OutlineData of Outline.hlsl / FOutlineRenderData::FConstantBuffer (DrawData.h:69-79) */
    VQ_matrix matWorld, matWorldView, matNormalView, matProj, matViewInverse;
    VQ_float4 Color, uvScaleBias; float Scale, HeightDisplacement;
    float pad_[2];               /* the tail padding of the 16-byte aligned C++ struct */
} VQ_OutlineData;
typedef struct vqhip_outline_draw {
    vqhip_shadow_mesh mesh;      /* the engine's vertex: position @0, normal @12; strideBytes >= 24, a multiple of 4 */
    const VQ_OutlineData* cb;    /* device, 4-byte aligned; read when the kernels run: matWorldView, matNormalView, matProj, Color */
} vqhip_outline_draw;
typedef struct vqhip_outline_targets {   /* device */
    void*     sceneColor;        /* RGBA16F [height][pitch], 8-byte aligned: modified IN PLACE, only where O5 writes */
    uint8_t*  selection;         /* or NULL: 1 where pass 0 marked the pixel (the stencil), else 0 */
    uint32_t* writer;            /* or NULL, 4-byte aligned: index (into draws) of the draw whose colour the pixel received, 0xFFFFFFFF for none */
    int32_t pitch, selection_pitch, writer_pitch, reserved;   /* pixels (= bytes for selection) per row, 0 = width; reserved 0 */
} vqhip_outline_targets;
VQHIP_STATIC_ASSERT(sizeof(VQ_OutlineData) == 368 && offsetof(VQ_OutlineData, matWorldView) == 64 && offsetof(VQ_OutlineData, matNormalView) == 128 &&
                    offsetof(VQ_OutlineData, matProj) == 192 && offsetof(VQ_OutlineData, matViewInverse) == 256 && offsetof(VQ_OutlineData, Color) == 320 &&
                    offsetof(VQ_OutlineData, uvScaleBias) == 336 && offsetof(VQ_OutlineData, Scale) == 352 && offsetof(VQ_OutlineData, HeightDisplacement) == 356,
                    "VQ_OutlineData layout");
VQHIP_STATIC_ASSERT(sizeof(vqhip_outline_draw) == 40 && offsetof(vqhip_outline_draw, cb) == 32, "vqhip_outline_draw layout");
VQHIP_STATIC_ASSERT(sizeof(vqhip_outline_targets) == 40 && offsetof(vqhip_outline_targets, pitch) == 24, "vqhip_outline_targets layout");
/* Bytes of work for a call that draws `triangles` triangles (sum over draws of numIndices / 3): a counter, 16 bytes per draw of the colour table (sized for
 * min(triangles, 20 000) draws: a draw with indices has a triangle) and sixteen records of 56 bytes per triangle (each pass: a fan of at most eight). 0 for 2^28
 * or more triangles (the records must fit the 32-bit counter) or a size that does not fit size_t. Host-only. */
VQHIP_API size_t vqhip_outline_work_bytes(uint64_t triangles);
/* Returns VQHIP_ERR_INVALID_ARG — launching nothing, leaving the outputs untouched — for NULL pointers (ctx, out, sceneColor, work, draws with numDraws > 0, a
 * mesh's positions or indices, cb), numDraws < 0, width or height outside 1 .. 8192, a negative pitch or one below width, reserved != 0, sceneColor not 8-byte
 * aligned, writer not 4-byte aligned, an indexBits other than 16 / 32, numIndices % 3 != 0, a stride below 24 or not a multiple of 4, positions or cb not 4-byte
 * aligned, indices not aligned to their size, work not 256-byte aligned, workBytes below vqhip_outline_work_bytes of the call's own triangle count, or an output
 * overlapping another output or the work buffer; VQHIP_ERR_UNSUPPORTED for more than 20 000 draws with indices or 2^28 or more triangles in one call. */
VQHIP_API int vqhip_outline(vqhip_ctx* ctx, void* stream, const vqhip_outline_draw* draws, int numDraws, int width, int height,
        const vqhip_outline_targets* out, void* work, size_t workBytes);

/* ---- Heightmap displacement for every rasterised pass: CalcHeightOffset of the five vertex stages (ForwardLighting.hlsl:136-154, DepthPrePass.hlsl:96-100,
 * ShadowDepthPass.hlsl:61-66, ObjectID.hlsl:70-74, Outline.hlsl:78-82), each of which runs
 *     vPosition.xyz += float3(0, texHeightmap.SampleLevel(LinearSamplerTess, uv * scale + offset, 0).r * displacement, 0)
 * before any matrix. Batching.cpp:156-157 hands the shadow pass the (tiling, uv_bias) and displacement that Material::GetCBufferData hands the others, and the
 * Outline pass receives the same number as HeightDisplacement: the offset is a function of (vertex, material) alone. This call therefore writes a displaced COPY of
 * a mesh's vertex stream, once per (mesh LOD, material), and every rasteriser of this library consumes that copy unchanged: the add happens once, in binary32,
 * before any matrix, exactly where the reference does it. docs/DESIGN_DETAILS.md §7.22 is the normative statement; tests/displace_ref.py states it in numpy:
 *   H1  u = uv.x * scale.x + offset.x, v likewise: binary32, product and sum rounded separately, whatever vqhip_set_arithmetic says (§7.18 I1's statement).
 *   H2  s = the bilinear WRAP fetch of LEVEL 0 of the RGBA8_UNORM chain (LinearSamplerTess is TRILINEAR_WRAP, RootSignatures.cpp:151, :361; SampleLevel 0), red
 *       channel: 8-bit fixed-point fractions, exact weights, the FMA chain of the sampling contract, then * RN(1 / 255). Only level 0 is read, whatever `mips`
 *       says. texels == NULL is the null SRV: s = 0.0f. Any uv is safe, NaN and +-inf included: no lane reads outside level 0.
 *   H3  h = s * displacement (one product); y' = y + h (one sum); x and z are copied bit for bit (the reference's + 0.0f on x and z is the one the rasterisers
 *       keep downstream).
 *   H4  the one known deviation, a sign of zero: the consumers' retained y + 0.0f turns a stored y' = -0 into +0, the reference's single y + h keeps -0 (only
 *       when y and h are both -0). No tested output can tell: §7.22.
 * outStrideBytes == strideBytes: the whole vertex is copied with y replaced (normal @12, tangent @24, uv @36 and any tail words bit for bit) — the stream of the
 * lit, Outline and masked draws. outStrideBytes == 12: the displaced position alone — the compact stream of the opaque depth and shadow draws. One call takes many
 * meshes: the job table is staged through the context's constant ring (a slot holds 556 jobs), ONE kernel launch per ring slot, never one per mesh. No allocation,
 * no memset node, no readback. Jobs are host memory, consumed before the call returns; vertices, out and the height map are device memory, read and written when
 * the kernels run. H2 in a vertex stage is UNPINNED against a D3D12 device (docs/WARP_CALIBRATION.md §5), like every other Sample* here.
 * Out of scope: the tessellated permutations (and their height-derived normals, ForwardLighting.hlsl:255-262), height maps in other formats, displacing in place. */
typedef struct vqhip_displace_job {
    const void* vertices;  uint32_t strideBytes;   /* device, 4-byte aligned; the engine's vertex: position @0, uv @36; 44 .. 2048 (D3D12's vertex stride limit), a multiple of 4 */
    uint32_t    numVertices;                       /* 0 allowed: nothing written */
    void*       out;       uint32_t outStrideBytes;/* device, 4-byte aligned; == strideBytes (full copy) or 12 (positions only) */
    uint32_t    reserved;                          /* 0 */
    vqhip_texture2d heightmap;                     /* RGBA8_UNORM chain, level 0 read; texels NULL = null SRV */
    VQ_float4   uvScaleOffset;                     /* MaterialData.uvScaleOffset == PerObjectShadowData.texScaleBias */
    float       displacement;                      /* MaterialData.displacement == Outline's HeightDisplacement */
} vqhip_displace_job;
VQHIP_STATIC_ASSERT(sizeof(vqhip_displace_job) == 80 && offsetof(vqhip_displace_job, strideBytes) == 8 && offsetof(vqhip_displace_job, numVertices) == 12 &&
                    offsetof(vqhip_displace_job, out) == 16 && offsetof(vqhip_displace_job, outStrideBytes) == 24 && offsetof(vqhip_displace_job, reserved) == 28 &&
                    offsetof(vqhip_displace_job, heightmap) == 32 && offsetof(vqhip_displace_job, uvScaleOffset) == 56 && offsetof(vqhip_displace_job, displacement) == 72,
                    "vqhip_displace_job layout");
/* Jobs WITH vertices in one call: what 31 of the constant ring's 32 slots hold, so that one call never laps the ring. */
#define VQHIP_DISPLACE_MAX_JOBS 17236
/* Returns VQHIP_ERR_INVALID_ARG — launching nothing, leaving the outputs untouched — for a NULL ctx, NULL jobs with numJobs > 0, numJobs < 0, and for a job with:
 * NULL vertices or out while numVertices > 0; a stride outside 44 .. 2048 or not a multiple of 4; an outStrideBytes that is neither 12 nor strideBytes;
 * reserved != 0; vertices or out not 4-byte aligned; a height map with texels whose width or height is outside 1 .. 16384, whose mips is below 1 or above
 * vqhip_mip_level_count(width, height), or whose texels are not 4-byte aligned; an output that overlaps its own input, any other job's input or output, or a
 * height map (measured over numVertices * stride bytes and the whole chain). In-place operation is refused: a second call would displace twice.
 * VQHIP_ERR_UNSUPPORTED for 2^31 or more vertices in one call, or more than VQHIP_DISPLACE_MAX_JOBS jobs with vertices. numJobs == 0 is VQHIP_OK. */
VQHIP_API int vqhip_displace_meshes(vqhip_ctx* ctx, void* stream, const vqhip_displace_job* jobs, int numJobs);

/* ---- Unlit draws: the light gizmo meshes (SceneRendering.cpp:1787-1819) and the solid half of RenderLightBounds (:1940-1989), both Unlit.hlsl — VSMain: one matrix,
 * PSMain: one colour per draw — through UNLIT_PSO / UNLIT_BLEND_PSO (PipelineStateObjects.cpp:1174-1232): cull BACK, depth LESS WITHOUT depth writes against the
 * scene's D32 depth, into the RGBA16F scene colour; UNLIT_BLEND_PSO adds SRC_ALPHA / INV_SRC_ALPHA blending. The light bounds go to scene colour with blending
 * when reflections are off (:507-510) and to the cleared Tex_SceneColorBoundingVolumes without blending when they are on (:2296-2336: the boundingVolumes plane of
 * vqhip_composite_reflections). One call, one sample per pixel. docs/DESIGN_DETAILS.md §7.23 is the normative statement (rules U1 .. U7); tests/unlit_ref.py states
 * it in numpy on top of tests/scene_depth_ref.py:
 *   U1  vertex: clip[j] = §7.16 R1's mulPoint((x, y + 0.0f, z), matModelViewProj, j). Binary32 whatever vqhip_set_arithmetic says; the host forms
 *       matWorldTransformation * viewProj, as the reference's CPU code does. A vertex with a non-finite clip component drops its triangle.
 *   U2  raster: §7.17's V2 (seven planes), V3 (viewport {0, 0, W, H, 0, 1}, 16.8 snap), R4 (int64 edge functions, top-left rule, the sample at the pixel centre)
 *       and V5 (the fragment's depth), unchanged. One sample per pixel. cullMode per draw (the reference: VQHIP_CULL_BACK).
 *   U3  depth test: a fragment passes iff its V5 depth is strictly below sceneDepth[pixel] (binary32 compare; a NaN there passes nothing). sceneDepth is never
 *       written: re-submitting the mesh and matrix that produced sceneDepth writes nothing where that mesh is the visible surface.
 *   U4  submission order: q = first(draw) + tri, §7.17's sequence number with one instance per draw; the fan pieces of a clipped triangle in fan order.
 *   U5  blend == 0 (UNLIT_PSO): a pixel with a passing fragment receives the colour of the passing fragment with the largest q, the four channels stored with
 *       exactly O5's half conversion (round to nearest even; a NaN as 0x7E00 with its sign). Every other pixel keeps its bits.
 *   U6  blend == 1 (UNLIT_BLEND_PSO): per pixel a fold over the passing fragments in ascending q, starting from the stored halfs decoded exactly:
 *       ia = 1.0f - a; c' = RN16(RN32(RN32(s.c * a) + RN32(d.c * ia))) for c = r, g, b; a' = RN16(s.a) — rounded to half after EVERY fragment (the render target
 *       holds halfs between fragments), no FMA contraction. A NaN result stores 0x7E00, sign cleared. Every pixel without a passing fragment keeps its bits.
 *   U7  writer (optional): the index, into draws, of the last passing fragment's draw; 0xFFFFFFFF where none passed. The call clears it.
 * U6's blend precision and per-fragment rounding are UNPINNED against a D3D12 device (docs/WARP_CALIBRATION.md §5: D3D bounds them from below only), beside what
 * §7.17 lists (V2, V5).
 * Kernels on `stream`: one setup launch per ring slot of draws (fan piece k of triangle q into the FIXED slot 8 q + k, the empty box elsewhere: no counter, memory
 * order is submission order), one tile fill (every lane owns its pixels in registers; the triangles' boxes, then the slots of those that touch the tile, are scanned
 * in order and compacted in order into an LDS queue of VQHIP_UNLIT_QUEUE_CAPACITY records, drained front to back whenever it would overflow: the result does not
 * depend on scheduling), which also clears writer. No
 * allocation, no memset node, no readback. Draw descriptors are host memory, consumed before the call returns; meshes, constant buffers and planes are device
 * memory, read when the kernels run. numDraws == 0 leaves sceneColor untouched and clears writer. Option raster_tile 64 is honoured.
 * Out of scope: the WIREFRAME PSOs (bounding boxes, the second half of RenderLightBounds: D3D's line rasterisation), RenderDebugVertexAxes, 4x MSAA (the library
 * has no per-sample scene colour, as the Outline pass notes), the instanced cbuffer variant. The first two and the instanced cbuffer are vqhip_line_draws' (below);
 * 4x MSAA stays out of scope there as well. */
typedef struct VQ_UnlitData {    /* byte for byte FFrameConstantBufferUnlit, the cbuffer of Unlit.hlsl */
    VQ_matrix matModelViewProj;
    VQ_float4 color;
} VQ_UnlitData;
typedef struct vqhip_unlit_draw {
    vqhip_shadow_mesh mesh;      /* position @0; strideBytes >= 12, a multiple of 4 */
    const VQ_UnlitData* cb;      /* device, 4-byte aligned; read when the kernels run */
    int32_t cullMode;            /* VQHIP_CULL_* (the reference: VQHIP_CULL_BACK) */
    int32_t reserved;            /* 0 */
} vqhip_unlit_draw;
typedef struct vqhip_unlit_targets {     /* device */
    void*        sceneColor;     /* RGBA16F [height][pitch], 8-byte aligned: modified IN PLACE, only where a fragment passes */
    const float* sceneDepth;     /* float [height][depth_pitch], 4-byte aligned: the depth of vqhip_scene_depth at 1 sample; read, never written */
    uint32_t*    writer;         /* or NULL, 4-byte aligned: U7 */
    int32_t pitch, depth_pitch, writer_pitch, reserved;   /* pixels per row, 0 = width; reserved 0 */
} vqhip_unlit_targets;
VQHIP_STATIC_ASSERT(sizeof(VQ_UnlitData) == 80 && offsetof(VQ_UnlitData, color) == 64, "VQ_UnlitData layout");
VQHIP_STATIC_ASSERT(sizeof(vqhip_unlit_draw) == 48 && offsetof(vqhip_unlit_draw, cb) == 32 && offsetof(vqhip_unlit_draw, cullMode) == 40, "vqhip_unlit_draw layout");
VQHIP_STATIC_ASSERT(sizeof(vqhip_unlit_targets) == 40 && offsetof(vqhip_unlit_targets, sceneDepth) == 8 && offsetof(vqhip_unlit_targets, writer) == 16 &&
                    offsetof(vqhip_unlit_targets, pitch) == 24, "vqhip_unlit_targets layout");
/* Records the fill's LDS queue holds: a tile touched by more records than this is drained more than once (the result is the same). */
#define VQHIP_UNLIT_QUEUE_CAPACITY 256
/* Bytes of work for a call that draws `triangles` triangles (sum over draws of numIndices / 3): 32 bytes per draw of the colour table (sized for
 * min(triangles, 20 000) draws, at least one), 8 bytes of pixel box and eight slots of 56 bytes per triangle. 0 for 2^28 or more triangles or a size that does
 * not fit size_t. Host-only. */
VQHIP_API size_t vqhip_unlit_draws_work_bytes(uint64_t triangles);
/* Returns VQHIP_ERR_INVALID_ARG — launching nothing, leaving the outputs untouched — for NULL pointers (ctx, out, sceneColor, sceneDepth, work, draws with
 * numDraws > 0, a mesh's positions or indices, cb), numDraws < 0, width or height outside 1 .. 8192, blend outside 0 / 1, a negative pitch or one below width,
 * reserved != 0 (targets or a draw), an unknown cullMode, sceneColor not 8-byte aligned, sceneDepth or writer not 4-byte aligned, an indexBits other than 16 / 32,
 * numIndices % 3 != 0, a stride below 12 or not a multiple of 4, positions or cb not 4-byte aligned, indices not aligned to their size, work not 256-byte
 * aligned, workBytes below vqhip_unlit_draws_work_bytes of the call's own triangle count, an output overlapping another output or the work buffer, or sceneDepth
 * overlapping an output or the work buffer; VQHIP_ERR_UNSUPPORTED for more than 20 000 draws with indices or 2^28 or more triangles in one call. */
VQHIP_API int vqhip_unlit_draws(vqhip_ctx* ctx, void* stream, const vqhip_unlit_draw* draws, int numDraws, int width, int height, int blend,
        const vqhip_unlit_targets* out, void* work, size_t workBytes);

/* ---- Line draws: what keeps RenderSceneBoundingVolumes (SceneRendering.cpp:2286-2345) from running inside the library after vqhip_unlit_draws and vqhip_outline —
 * the WIREFRAME PSOs of Unlit.hlsl (RenderBoundingBoxes, :1853-1922, through the instanced cbuffer, up to 512 boxes per draw; the second half of RenderLightBounds,
 * :1991-2014, the solid bounds' meshes drawn again as wire) and RenderDebugVertexAxes (:2018-2058, VertexDebug.hlsl: an indexed POINT list whose geometry shader
 * emits three coloured lines per point). Both are D3D's ALIASED line rasterisation (MultisampleEnable and AntialiasedLineEnable at their defaults,
 * PipelineStateObjects.cpp:1186, 1234-1258, 1391-1422): depth LESS WITHOUT depth writes against the scene's D32 depth, cull NONE, no blending, into the RGBA16F
 * scene colour, which is modified IN PLACE (vqhip_unlit_targets, unchanged). One call, one sample per pixel, draws of both kinds in submission order. docs/DESIGN_DETAILS.md §7.24 is the normative statement (rules L1 .. L8);
 * tests/line_ref.py states it in numpy on top of tests/scene_depth_ref.py:
 *   L1  wireframe vertex: U1 as it stands — clip[j] = mulPoint((x, y + 0.0f, z), matModelViewProj[instance], j), binary32 whatever vqhip_set_arithmetic says. A
 *       triangle with an index past numVertices is dropped; a line with a non-finite clip component at either end is dropped.
 *   L2  wireframe lines: triangle (i0, i1, i2) yields the directed lines i0->i1, i1->i2, i2->i0, in that order. Every line is drawn (a shared edge twice); each is
 *       clipped as a segment of its own: clipping introduces no edge along a clip plane.
 *   L3  vertex axes: one point per INDEX in index order (an index past numVertices drops its three lines). tbn0 = normalize(T), tbn1 = normalize(cross(N, T)),
 *       tbn2 = normalize(N); P = mul(matWorld, float4(p, 1)).xyz; O_k = normalize(mul(matNormal, float4(tbn_k, 0)).xyz) * LocalAxisSize; the line k runs from
 *       mul(matViewProj, float4(P, 1)) to mul(matViewProj, float4(P + O_k, 1)). Binary32, every product and sum rounded in the written order (mulPoint's
 *       association), the contract's as-written normalize. Colours in emission order: tangent (0.6, 0, 0), cross(N, T) (0, 0, 0.6) — BLUE —, normal (0, 0.6, 0),
 *       alpha 1. No + 0.0f, no heightmap. A line with a non-finite end is dropped on its own.
 *   L4  the segment is clipped against V2's seven planes, from the inside end towards the outside end, the direction kept; V3's viewport {0, 0, W, H, 0, 1} and
 *       16.8 snap; z_i = clip_i.z / clip_i.w of the two post-clip ends.
 *   L5  coverage, the diamond-exit rule, in integers on the snapped ends: x-major when |dx| >= |dy|, else y-major. Pixel (i, j) has the diamond
 *       |x - cx| + |y - cy| < 128 around (256 i + 128, 256 j + 128), plus its lower-left edge, lower-right edge and bottom corner (y grows downwards), plus — for
 *       y-major lines — its right corner. Covered iff the closed segment meets that set and the segment's END point is not in it. Zero length covers nothing.
 *   L6  depth: with m the major axis and c the pixel centre on it, t = saturate((float)(c - m_0) / (float)(m_1 - m_0)), d = saturate(z_0 + t * (z_1 - z_0));
 *       the fragment passes iff d is strictly below sceneDepth[pixel] (binary32; a NaN there passes nothing). sceneDepth is never written.
 *   L7  order and colour: wireframe q = 3 * (first(draw) + instance * numTris + tri) + edge, axes q = first + 3 * point + axis, draws in submission order across
 *       both kinds. A pixel with a passing fragment receives the colour of the passing fragment with the largest q, stored with O5's half conversion (a NaN as
 *       0x7E00 with its sign). Every other pixel keeps its bits. No blending.
 *   L8  writer (optional): as U7 — the index, into draws, of that fragment's draw; 0xFFFFFFFF where none passed. The call clears it.
 * L5 (the maintainers' reading of the diamond-exit rule), L2's edge order and clipping, and L6's interpolation precision are UNPINNED against a D3D12 device
 * (docs/WARP_CALIBRATION.md §5), beside what §7.17 lists (V2).
 * Kernels on `stream`: one setup launch per ring slot of draws (k_lines_setup: line q into the FIXED slot q, the empty box for a dropped line: no counter), one tile
 * fill (k_lines_fill: one LDS word per pixel, atomicMax of q + 1: the result does not depend on scheduling), which also clears writer. No allocation, no memset
 * node, no readback. Draw descriptors are host memory, consumed before the call returns; meshes, matrices, colours, constant buffers and planes are device memory,
 * read when the kernels run. numDraws == 0 leaves sceneColor untouched and clears writer. Option raster_tile 64 is honoured.
 * Out of scope: 4x MSAA (the library has no per-sample scene colour), the FillMode WIREFRAME permutations of the lit, depth and ObjectID PSOs, antialiased or
 * quadrilateral lines. */
typedef enum { VQHIP_LINES_WIREFRAME = 0, VQHIP_LINES_VERTEX_AXES = 1 } vqhip_line_kind;
typedef struct VQ_VertexAxesData {   /* byte for byte FObjectConstantBufferDebugVertexVectors, the cbuffer of VertexDebug.hlsl */
    VQ_matrix matWorld, matNormal, matViewProj;
    float LocalAxisSize;
    float pad_[3];
} VQ_VertexAxesData;
typedef struct vqhip_line_draw {
    vqhip_shadow_mesh mesh;            /* WIREFRAME: position @0, stride >= 12, numIndices % 3 == 0; VERTEX_AXES: position @0, normal @12, tangent @24, stride >= 36, any numIndices */
    const VQ_matrix* matModelViewProj; /* WIREFRAME: device, [numInstances] — &VQ_UnlitData.matModelViewProj or the instanced cbuffer's array; else NULL */
    const VQ_float4* color;            /* WIREFRAME: device — the cbuffer's colour (offset 64, or 512 * 64 in the instanced cbuffer); else NULL */
    const VQ_VertexAxesData* axes;     /* VERTEX_AXES: device; else NULL */
    uint32_t numInstances;             /* WIREFRAME: 1 .. 512 (MAX_INSTANCE_COUNT__UNLIT_SHADER); VERTEX_AXES: 1 */
    int32_t  kind;                     /* vqhip_line_kind */
} vqhip_line_draw;
VQHIP_STATIC_ASSERT(sizeof(VQ_VertexAxesData) == 208 && offsetof(VQ_VertexAxesData, matNormal) == 64 && offsetof(VQ_VertexAxesData, matViewProj) == 128 &&
                    offsetof(VQ_VertexAxesData, LocalAxisSize) == 192, "VQ_VertexAxesData layout");
VQHIP_STATIC_ASSERT(sizeof(vqhip_line_draw) == 64 && offsetof(vqhip_line_draw, matModelViewProj) == 32 && offsetof(vqhip_line_draw, color) == 40 &&
                    offsetof(vqhip_line_draw, axes) == 48 && offsetof(vqhip_line_draw, numInstances) == 56 && offsetof(vqhip_line_draw, kind) == 60,
                    "vqhip_line_draw layout");
#define VQHIP_LINES_MAX_INSTANCES 512    /* MAX_INSTANCE_COUNT__UNLIT_SHADER */
/* Bytes of work for a call that draws `lines` lines (sum over draws of numIndices * numInstances for WIREFRAME, 3 * numIndices for VERTEX_AXES): 64 bytes per draw
 * of the colour table (sized for min(lines, 20 000) draws, at least one), 8 bytes of pixel box and 32 bytes of record per line. 0 for 2^31 or more lines or a size
 * that does not fit size_t. Host-only. */
VQHIP_API size_t vqhip_line_draws_work_bytes(uint64_t lines);
/* Returns VQHIP_ERR_INVALID_ARG — launching nothing, leaving the outputs untouched — for NULL pointers (ctx, out, sceneColor, sceneDepth, work, draws with
 * numDraws > 0, a mesh's positions or indices), numDraws < 0, width or height outside 1 .. 8192, a negative pitch or one below width, reserved != 0 (targets), an
 * unknown kind, pointers that do not fit the kind (WIREFRAME: matModelViewProj and color set, axes NULL; VERTEX_AXES: axes set, the other two NULL), numInstances
 * outside 1 .. 512 (WIREFRAME) or other than 1 (VERTEX_AXES), sceneColor not 8-byte aligned, sceneDepth or writer not 4-byte aligned, an indexBits other than
 * 16 / 32, numIndices % 3 != 0 (WIREFRAME), a stride below 12 (WIREFRAME) or 36 (VERTEX_AXES) or not a multiple of 4, positions, matrices, colour or axes not
 * 4-byte aligned, indices not aligned to their size, work not 256-byte aligned, workBytes below vqhip_line_draws_work_bytes of the call's own line count, an output
 * overlapping another output or the work buffer, or sceneDepth overlapping an output or the work buffer; VQHIP_ERR_UNSUPPORTED for more than 20 000 draws with
 * indices or 2^31 or more lines in one call. */
VQHIP_API int vqhip_line_draws(vqhip_ctx* ctx, void* stream, const vqhip_line_draw* draws, int numDraws, int width, int height,
        const vqhip_unlit_targets* out, void* work, size_t workBytes);

#ifdef __cplusplus
}
#endif
#endif /* VQHIP_H */
