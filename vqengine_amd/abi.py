"""ctypes mirror of include/vqhip.h (the C ABI structs == VQ_SHADER_DATA of
Shaders/LightingConstantBufferData.h:50-186). Pure layout, no compute; importable without a GPU.
Sizes/offsets are asserted against SURVEY.md §8(b) at import time."""
import ctypes as C

VQHIP_OK = 0
VQHIP_ERR_INVALID_ARG = -1
VQHIP_ERR_HIP = -2
VQHIP_ERR_UNSUPPORTED = -3
VQHIP_ERR_NO_DEVICE = -4
VQHIP_ERR_RCCL = -5

FMT_RGBA32F, FMT_RGBA16F, FMT_RGBA8_UNORM, FMT_RG16F, FMT_RG32F = 0, 1, 2, 3, 4
FMT_R10G10B10A2_UNORM = 5          # Tex_SceneNormals: input of ssr_environment_fallback only
FMT_R11G11B10_FLOAT = 6            # TexAverageRadiance: written by ssr_reproject, read by ssr_prefilter / ssr_resolve_temporal (one uint32 per texel)
FMT_BPP = {FMT_RGBA32F: 16, FMT_RGBA16F: 8, FMT_RGBA8_UNORM: 4, FMT_RG16F: 4, FMT_RG32F: 8}
CONV_SEQUENTIAL, CONV_WAVE64 = 0, 1
ARITH_LITERAL, ARITH_DXC = 0, 1
ABI_VERSION = 3
COLOR_SPACE_REC_709, COLOR_SPACE_REC_2020 = 0, 1
DISPLAY_CURVE_SRGB, DISPLAY_CURVE_ST2084, DISPLAY_CURVE_LINEAR = 0, 1, 2

NUM_LIGHTS__POINT = 100
NUM_LIGHTS__SPOT = 20
NUM_SHADOWING_LIGHTS__POINT = 5
NUM_SHADOWING_LIGHTS__SPOT = 5


class float2(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float)]


class float3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]

    def set(self, v):
        self.x, self.y, self.z = float(v[0]), float(v[1]), float(v[2])


class float4(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("w", C.c_float)]


class matrix(C.Structure):  # DirectX::XMMATRIX, row-major, 16-byte aligned (padding is explicit in the parents)
    _fields_ = [("m", (C.c_float * 4) * 4)]


class PointLight(C.Structure):
    _fields_ = [("position", float3), ("range", C.c_float), ("color", float3), ("brightness", C.c_float),
                ("attenuation", float3), ("depthBias", C.c_float)]


class SpotLight(C.Structure):
    _fields_ = [("position", float3), ("outerConeAngle", C.c_float), ("color", float3), ("brightness", C.c_float),
                ("spotDir", float3), ("depthBias", C.c_float), ("innerConeAngle", C.c_float), ("range", C.c_float),
                ("dummy1", C.c_float), ("dummy2", C.c_float)]


class DirectionalLight(C.Structure):
    _fields_ = [("lightDirection", float3), ("brightness", C.c_float), ("color", float3), ("depthBias", C.c_float),
                ("shadowing", C.c_int32), ("enabled", C.c_int32)]


class SceneLighting(C.Structure):
    _fields_ = [("numPointLights", C.c_int32), ("numSpotLights", C.c_int32), ("numPointCasters", C.c_int32),
                ("numSpotCasters", C.c_int32), ("directional", DirectionalLight), ("_pad0", C.c_byte * 8),
                ("shadowViewDirectional", matrix),
                ("point_lights", PointLight * NUM_LIGHTS__POINT), ("point_casters", PointLight * NUM_SHADOWING_LIGHTS__POINT),
                ("spot_lights", SpotLight * NUM_LIGHTS__SPOT), ("spot_casters", SpotLight * NUM_SHADOWING_LIGHTS__SPOT),
                ("shadowViews", matrix * NUM_SHADOWING_LIGHTS__SPOT)]


class PerFrameData(C.Structure):
    _fields_ = [("Lights", SceneLighting), ("f2PointLightShadowMapDimensions", float2),
                ("f2SpotLightShadowMapDimensions", float2), ("f2DirectionalLightShadowMapDimensions", float2),
                ("fAmbientLightingFactor", C.c_float), ("fHDRIOffsetInRadians", C.c_float)]


class PerViewLightingData(C.Structure):
    _fields_ = [("matView", matrix), ("matViewToWorld", matrix), ("matProjInverse", matrix),
                ("WorldFrustumPlanes", float4 * 6), ("CameraPosition", float3), ("MaxEnvMapLODLevels", C.c_float),
                ("ScreenDimensions", float2), ("EnvironmentMapDiffuseOnlyIllumination", C.c_int32), ("pad1", C.c_float)]


class MaterialData(C.Structure):
    _fields_ = [("diffuse", float3), ("alpha", C.c_float), ("emissiveColor", float3), ("emissiveIntensity", C.c_float),
                ("specular", float3), ("normalMapMipBias", C.c_float), ("uvScaleOffset", float4),
                ("roughness", C.c_float), ("metalness", C.c_float), ("displacement", C.c_float), ("textureConfig", C.c_float)]


class TonemapperParams(C.Structure):  # FPostProcessParameters::FTonemapper defaults, PostProcess.h:84-91
    _fields_ = [("ContentColorSpaceEnum", C.c_int32), ("OutputDisplayCurveEnum", C.c_int32),
                ("DisplayReferenceBrightnessLevel", C.c_float), ("ToggleGammaCorrection", C.c_int32)]

    @staticmethod
    def default():
        return TonemapperParams(COLOR_SPACE_REC_709, DISPLAY_CURVE_SRGB, 200.0, 1)


class BlurParams(C.Structure):
    _fields_ = [("iImageSizeX", C.c_int32), ("iImageSizeY", C.c_int32)]


class EnvMap(C.Structure):
    _fields_ = [("diffuse_cube", C.c_void_p), ("diffuse_res", C.c_int32), ("specular_cube", C.c_void_p),
                ("spec_res0", C.c_int32), ("spec_mips", C.c_int32), ("brdf_lut", C.c_void_p), ("lut_size", C.c_int32)]


class ShadowMaps(C.Structure):
    _fields_ = [("directional", C.c_void_p), ("dir_dim", C.c_int32), ("spot", C.c_void_p), ("spot_dim", C.c_int32),
                ("point", C.c_void_p), ("point_dim", C.c_int32)]


class GBuffer(C.Structure):
    _fields_ = [("gb0", C.c_void_p), ("gb1", C.c_void_p), ("gb2", C.c_void_p), ("gb3", C.c_void_p),
                ("width", C.c_int32), ("height", C.c_int32), ("row_pitch_px", C.c_int32)]


class PsmainTargets(C.Structure):    # vqhip_psmain_targets: the lit draw's other render targets (ForwardLighting.hlsl:57-68,382-389)
    _fields_ = [("albedo_metallic", C.c_void_p), ("albedo_fmt", C.c_int32), ("albedo_pitch_px", C.c_int32),
                ("motion_vectors", C.c_void_p), ("motion_fmt", C.c_int32), ("motion_pitch_px", C.c_int32),
                ("svPositionCurr", C.c_void_p), ("svPositionPrev", C.c_void_p), ("sv_pitch_px", C.c_int32), ("pad_", C.c_int32)]


assert C.sizeof(PsmainTargets) == 56

MSAA_MAX_LAYERS = 4   # VQHIP_MSAA_MAX_LAYERS
MSAA_SAMPLE_POSITIONS = ((-2, -6), (6, -2), (-6, 2), (2, 6))   # D3D's standard 4x pattern, in 1/16 pixel from the pixel centre; sample s = bit s of a coverage byte


class GBufferMSAA(C.Structure):   # vqhip_gbuffer_msaa: up to 4 fragment layers + their per-pixel sample masks (vqhip_forward_lighting_msaa)
    _fields_ = [("layer", GBuffer * MSAA_MAX_LAYERS), ("coverage", C.c_void_p * MSAA_MAX_LAYERS), ("layers", C.c_int32), ("coverage_pitch", C.c_int32)]


class MSAASurfaces(C.Structure):   # vqhip_msaa_surfaces: the 4-sample depth + per-layer normals / roughness planes of vqhip_msaa_resolve_surfaces
    _fields_ = [("depth_ms", C.c_void_p), ("coverage", C.c_void_p * MSAA_MAX_LAYERS), ("normals", C.c_void_p * MSAA_MAX_LAYERS),
                ("roughness", C.c_void_p * MSAA_MAX_LAYERS), ("background", C.c_void_p),
                ("normals_pitch_px", C.c_int32 * MSAA_MAX_LAYERS), ("roughness_pitch_px", C.c_int32 * MSAA_MAX_LAYERS),
                ("width", C.c_int32), ("height", C.c_int32), ("layers", C.c_int32), ("coverage_pitch", C.c_int32),
                ("depth_pitch_px", C.c_int32), ("background_pitch_px", C.c_int32), ("normals_fmt", C.c_int32), ("pad_", C.c_int32)]


class SSRReprojectSurfaces(C.Structure):   # vqhip_ssr_reproject_surfaces: every plane, pitch and format of vqhip_ssr_reproject
    _fields_ = ([(n, C.c_void_p) for n in ("tile_list", "counters", "depth", "normals", "roughness", "depth_history", "normal_history", "roughness_history", "radiance",
                                            "radiance_history", "motion_vectors", "variance_history", "sample_count_history", "out_reprojected", "out_average",
                                            "out_variance", "out_sample_count")]
                + [(n, C.c_int32) for n in ("depth_pitch_px", "normals_pitch_px", "roughness_pitch_px", "depth_history_pitch_px", "normal_history_pitch_px",
                                            "roughness_history_pitch_px", "radiance_pitch_px", "radiance_history_pitch_px", "motion_pitch_px", "variance_history_pitch_px",
                                            "sample_count_history_pitch_px", "out_reprojected_pitch_px", "out_variance_pitch_px", "out_sample_count_pitch_px",
                                            "normals_fmt", "normal_history_fmt", "radiance_fmt", "radiance_history_fmt", "motion_fmt", "out_reprojected_fmt", "out_average_fmt",
                                            "pad_")])


assert C.sizeof(SSRReprojectSurfaces) == 224

DEPTH_HIERARCHY_TRUE_TOP = 1     # VQHIP_DEPTH_HIERARCHY_TRUE_TOP
DEPTH_HIERARCHY_MAX_DIM = 4096   # VQHIP_DEPTH_HIERARCHY_MAX_DIM


class CommInfo(C.Structure):    # vqhip_comm_info
    _fields_ = [("world", C.c_int32), ("rank", C.c_int32), ("nranks_seen", C.c_int32), ("rank_seen", C.c_int32),
                ("rccl_version", C.c_int32), ("reserved", C.c_int32), ("library_path", C.c_char * 232)]


class EnvMapOut(C.Structure):
    _fields_ = [("diffuse_unblurred", C.c_void_p), ("diffuse_blurred", C.c_void_p), ("blur_tmp", C.c_void_p),
                ("specular", C.c_void_p)]


class Texture2D(C.Structure):  # vqhip_texture2d: RGBA8_UNORM mip chain, texels NULL == null SRV
    _fields_ = [("texels", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("mips", C.c_int32), ("reserved", C.c_int32)]


MATERIAL_ALPHA_MASKED = 1   # VQHIP_MATERIAL_ALPHA_MASKED: flag in vqhip_material.texDiffuse.reserved (the "_AlphaMasked" PSO permutation)
MATERIAL_TEXTURE_SLOTS = ("texDiffuse", "texNormals", "texEmissive", "texMetalness", "texRoughness", "texOcclRoughMetal", "texLocalAO")


class MaterialDesc(C.Structure):  # vqhip_material
    _fields_ = [("data", MaterialData)] + [(s, Texture2D) for s in MATERIAL_TEXTURE_SLOTS] + [("_tail_pad", C.c_int32 * 2)]  # alignas(16)


class Interpolants(C.Structure):  # vqhip_interpolants
    _fields_ = [("ip0", C.c_void_p), ("ip1", C.c_void_p), ("ip2", C.c_void_p),
                ("width", C.c_int32), ("height", C.c_int32), ("row_pitch_px", C.c_int32)]


class SSAO(C.Structure):  # vqhip_ssao
    _fields_ = [("texels", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32)]


class VizParams(C.Structure):  # VQ_VizParams == FPostProcessParameters::FVizualizationParams (Visualization.hlsl:26-31)
    _fields_ = [("iDrawMode", C.c_int32), ("iUnpackNormals", C.c_int32), ("fInputStrength", C.c_float)]


class SkydomeParams(C.Structure):  # VQ_SkydomeParams
    _fields_ = [("right", float3), ("tanHalfFovX", C.c_float), ("up", float3), ("tanHalfFovY", C.c_float),
                ("forward", float3), ("pad", C.c_float)]


class SSSRConstants(C.Structure):  # VQ_SSSRConstants == FFX_SSSRConstants (ScreenSpaceReflections.h:43-65)
    _fields_ = [(k, matrix) for k in ("invViewProjection", "projection", "invProjection", "view", "invView", "prevViewProjection", "envMapRotation")] + [
        ("bufferDimensions", C.c_uint32 * 2), ("inverseBufferDimensions", C.c_float * 2),
        ("temporalStabilityFactor", C.c_float), ("depthBufferThickness", C.c_float), ("roughnessThreshold", C.c_float), ("varianceThreshold", C.c_float),
        ("frameIndex", C.c_uint32), ("maxTraversalIntersections", C.c_uint32), ("minTraversalOccupancy", C.c_uint32), ("mostDetailedMip", C.c_uint32),
        ("samplesPerQuad", C.c_uint32), ("temporalVarianceGuidedTracingEnabled", C.c_uint32), ("envMapSpecularIrradianceCubemapMipLevelCount", C.c_uint32),
        ("pad_", C.c_uint32)]


class CacaoConstants(C.Structure):  # VQ_CacaoConstants == FFX_CACAO_Constants (AMDFidelityFX/CACAO/ffx_cacao.h:95-154)
    _fields_ = [(k, C.c_float * 2) for k in ("DepthUnpackConsts", "CameraTanHalfFOV", "NDCToViewMul", "NDCToViewAdd", "DepthBufferUVToViewMul", "DepthBufferUVToViewAdd")] + [
        (k, C.c_float) for k in ("EffectRadius", "EffectShadowStrength", "EffectShadowPow", "EffectShadowClamp", "EffectFadeOutMul", "EffectFadeOutAdd",
                                 "EffectHorizonAngleThreshold", "EffectSamplingRadiusNearLimitRec", "DepthPrecisionOffsetMod", "NegRecEffectRadius", "LoadCounterAvgDiv",
                                 "AdaptiveSampleCountLimit", "InvSharpness")] + [
        ("PassIndex", C.c_int32), ("BilateralSigmaSquared", C.c_float), ("BilateralSimilarityDistanceSigma", C.c_float),
        ("PatternRotScaleMatrices", (C.c_float * 4) * 5),
        ("NormalsUnpackMul", C.c_float), ("NormalsUnpackAdd", C.c_float), ("DetailAOStrength", C.c_float), ("Dummy0", C.c_float),
        ("SSAOBufferDimensions", C.c_float * 2), ("SSAOBufferInverseDimensions", C.c_float * 2),
        ("DepthBufferDimensions", C.c_float * 2), ("DepthBufferInverseDimensions", C.c_float * 2),
        ("DepthBufferOffset", C.c_int32 * 2), ("PerPassFullResUVOffset", C.c_float * 2),
        ("InputOutputBufferDimensions", C.c_float * 2), ("InputOutputBufferInverseDimensions", C.c_float * 2),
        ("ImportanceMapDimensions", C.c_float * 2), ("ImportanceMapInverseDimensions", C.c_float * 2),
        ("DeinterleavedDepthBufferDimensions", C.c_float * 2), ("DeinterleavedDepthBufferInverseDimensions", C.c_float * 2),
        ("DeinterleavedDepthBufferOffset", C.c_float * 2), ("DeinterleavedDepthBufferNormalisedOffset", C.c_float * 2),
        ("NormalsWorldToViewspaceMatrix", matrix)]


CULL_NONE, CULL_FRONT, CULL_BACK = 0, 1, 2   # VQHIP_CULL_*: iFaceCull
SHADOW_MAX_DIM = 8192                        # VQHIP_SHADOW_MAX_DIM
SHADOW_MAX_VIEWS = 64                        # VQHIP_SHADOW_MAX_VIEWS
SHADOW_MAX_INSTANCES = 128                   # VQHIP_SHADOW_MAX_INSTANCES == MAX_INSTANCE_COUNT__SHADOW_MESHES


class ShadowMesh(C.Structure):  # vqhip_shadow_mesh
    _fields_ = [("positions", C.c_void_p), ("strideBytes", C.c_uint32), ("numVertices", C.c_uint32), ("indices", C.c_void_p), ("indexBits", C.c_int32),
                ("numIndices", C.c_uint32)]


class ShadowDraw(C.Structure):  # vqhip_shadow_draw
    _fields_ = [("mesh", ShadowMesh), ("matWorldViewProj", C.c_void_p), ("matWorld", C.c_void_p), ("numInstances", C.c_uint32), ("cullMode", C.c_int32)]


class ShadowView(C.Structure):  # vqhip_shadow_view
    _fields_ = [("depth", C.c_void_p), ("pitchBytes", C.c_size_t), ("dim", C.c_int32), ("linearDepth", C.c_int32), ("cameraPosition", float3), ("farPlane", C.c_float),
                ("draws", C.POINTER(ShadowDraw)), ("numDraws", C.c_int32)]


SCENE_DEPTH_MAX_DIM = 8192                   # VQHIP_SCENE_DEPTH_MAX_DIM
SCENE_DEPTH_MAX_INSTANCES = 64               # VQHIP_SCENE_DEPTH_MAX_INSTANCES == MAX_INSTANCE_COUNT__SCENE_MESHES
SCENE_DEPTH_MAX_LAYERS = 4                   # VQHIP_SCENE_DEPTH_MAX_LAYERS
NO_PRIMITIVE = 0xFFFFFFFF                    # vqhip_scene_depth's primitive / layerPrimitive value for "no owner"


class SceneDepthDraw(C.Structure):  # vqhip_scene_depth_draw
    _fields_ = [("mesh", ShadowMesh), ("matWorldViewProj", C.c_void_p), ("numInstances", C.c_uint32), ("cullMode", C.c_int32)]


class SceneDepthTargets(C.Structure):  # vqhip_scene_depth_targets
    _fields_ = [("depth", C.c_void_p), ("primitive", C.c_void_p), ("coverage", C.c_void_p * 4), ("layerPrimitive", C.c_void_p * 4), ("layers", C.c_int32),
                ("pitch", C.c_int32), ("coverage_pitch", C.c_int32), ("reserved", C.c_int32)]


class SceneSurfaceDraw(C.Structure):  # vqhip_scene_surface_draw
    _fields_ = [("mesh", ShadowMesh), ("matWorldViewProj", C.c_void_p), ("matWorld", C.c_void_p), ("matNormal", C.c_void_p), ("matWorldViewProjPrev", C.c_void_p),
                ("numInstances", C.c_uint32), ("materialIndex", C.c_int32)]


class SceneInterpolantTargets(C.Structure):  # vqhip_scene_interpolant_targets
    _fields_ = [("ip0", C.c_void_p), ("ip1", C.c_void_p), ("ip2", C.c_void_p), ("svPositionCurr", C.c_void_p), ("svPositionPrev", C.c_void_p),
                ("pitch", C.c_int32), ("sv_pitch", C.c_int32)]


class SceneQuadTargets(C.Structure):  # vqhip_scene_quad_targets
    _fields_ = [("planes", SceneInterpolantTargets), ("quadUV", C.c_void_p), ("quad_pitch", C.c_int32), ("pad_", C.c_int32)]


class SceneDepthMaskedDraw(C.Structure):  # vqhip_scene_masked_depth_draw
    _fields_ = [("draw", SceneDepthDraw), ("material", C.POINTER(MaterialDesc))]


class ShadowMaskedDraw(C.Structure):  # vqhip_shadow_masked_draw
    _fields_ = [("draw", ShadowDraw), ("texDiffuseAlpha", C.POINTER(Texture2D))]


class ShadowMaskedView(C.Structure):  # vqhip_shadow_masked_view
    _fields_ = [("depth", C.c_void_p), ("pitchBytes", C.c_size_t), ("dim", C.c_int32), ("linearDepth", C.c_int32), ("cameraPosition", float3), ("farPlane", C.c_float),
                ("draws", C.POINTER(ShadowMaskedDraw)), ("numDraws", C.c_int32)]


MASK_TEXTURE_MAX_DIM = 16384                 # VQHIP_MASK_TEXTURE_MAX_DIM
MASK_TABLE_ENTRY_BYTES = 48                  # one draw's entry of the masked rasterisers' texture table in their work buffer
MASK_SIDE_RECORD_BYTES = 64                  # one masked instanced triangle's side record
SURFACE_VERTEX_BYTES = 44                    # the engine's vertex: position @0, normal @12, tangent @24, uv @36
SURFACE_JOB_BYTES = 80                       # one draw's entry of vqhip_scene_interpolants' table in its work buffer


class ObjectIdDraw(C.Structure):  # vqhip_object_id_draw
    _fields_ = [("numIndices", C.c_uint32), ("numInstances", C.c_uint32), ("objID", C.c_void_p), ("meshID", C.c_int32), ("materialID", C.c_int32)]


OBJECT_ID_JOB_BYTES = 32                     # one draw's entry of vqhip_object_ids' table in its work buffer


class OutlineData(C.Structure):  # VQ_OutlineData == the cbuffer OutlineData of Outline.hlsl / FOutlineRenderData::FConstantBuffer
    _fields_ = [("matWorld", matrix), ("matWorldView", matrix), ("matNormalView", matrix), ("matProj", matrix), ("matViewInverse", matrix),
                ("Color", float4), ("uvScaleBias", float4), ("Scale", C.c_float), ("HeightDisplacement", C.c_float), ("pad_", C.c_float * 2)]


class OutlineDraw(C.Structure):  # vqhip_outline_draw
    _fields_ = [("mesh", ShadowMesh), ("cb", C.c_void_p)]


class OutlineTargets(C.Structure):  # vqhip_outline_targets
    _fields_ = [("sceneColor", C.c_void_p), ("selection", C.c_void_p), ("writer", C.c_void_p), ("pitch", C.c_int32), ("selection_pitch", C.c_int32),
                ("writer_pitch", C.c_int32), ("reserved", C.c_int32)]


OUTLINE_DATA_BYTES = 368                     # sizeof(VQ_OutlineData)
OUTLINE_RECORDS_PER_TRIANGLE = 16            # vqhip_outline's work buffer: eight mark and eight paint records per triangle, 8 + 48 bytes each
NO_WRITER = 0xFFFFFFFF                       # vqhip_outline's writer value for "not written"


class DisplaceJob(C.Structure):  # vqhip_displace_job
    _fields_ = [("vertices", C.c_void_p), ("strideBytes", C.c_uint32), ("numVertices", C.c_uint32), ("out", C.c_void_p), ("outStrideBytes", C.c_uint32),
                ("reserved", C.c_uint32), ("heightmap", Texture2D), ("uvScaleOffset", float4), ("displacement", C.c_float)]


DISPLACE_MAX_JOBS = 17236                    # VQHIP_DISPLACE_MAX_JOBS: jobs with vertices in one vqhip_displace_meshes call (31 constant-ring slots of 556)
DISPLACE_POSITION_BYTES = 12                 # outStrideBytes of the compact stream: the displaced position alone


class UnlitData(C.Structure):  # VQ_UnlitData == FFrameConstantBufferUnlit, the cbuffer of Unlit.hlsl
    _fields_ = [("matModelViewProj", matrix), ("color", float4)]


class UnlitDraw(C.Structure):  # vqhip_unlit_draw
    _fields_ = [("mesh", ShadowMesh), ("cb", C.c_void_p), ("cullMode", C.c_int32), ("reserved", C.c_int32)]


class UnlitTargets(C.Structure):  # vqhip_unlit_targets
    _fields_ = [("sceneColor", C.c_void_p), ("sceneDepth", C.c_void_p), ("writer", C.c_void_p), ("pitch", C.c_int32), ("depth_pitch", C.c_int32),
                ("writer_pitch", C.c_int32), ("reserved", C.c_int32)]


class VertexAxesData(C.Structure):  # VQ_VertexAxesData == FObjectConstantBufferDebugVertexVectors, the cbuffer of VertexDebug.hlsl
    _fields_ = [("matWorld", matrix), ("matNormal", matrix), ("matViewProj", matrix), ("LocalAxisSize", C.c_float), ("pad_", C.c_float * 3)]


class LineDraw(C.Structure):  # vqhip_line_draw
    _fields_ = [("mesh", ShadowMesh), ("matModelViewProj", C.c_void_p), ("color", C.c_void_p), ("axes", C.c_void_p), ("numInstances", C.c_uint32), ("kind", C.c_int32)]


LINES_WIREFRAME, LINES_VERTEX_AXES = 0, 1    # vqhip_line_kind
LINES_MAX_INSTANCES = 512                    # VQHIP_LINES_MAX_INSTANCES == MAX_INSTANCE_COUNT__UNLIT_SHADER
VERTEX_AXES_DATA_BYTES = 208                 # sizeof(VQ_VertexAxesData)
LINE_BYTES = 8 + 32                          # vqhip_line_draws' work buffer: line q in the fixed slot q, a pixel box and a record
UNLIT_DATA_BYTES = 80                        # sizeof(VQ_UnlitData)
UNLIT_SLOTS_PER_TRIANGLE = 8                 # vqhip_unlit_draws' work buffer: fan piece k of triangle q in the fixed slot 8 q + k, 8 + 48 bytes each
UNLIT_QUEUE_CAPACITY = 256                   # VQHIP_UNLIT_QUEUE_CAPACITY: records the fill's LDS queue holds between two drains


def _chk(t, size, **offs):
    assert C.sizeof(t) == size, (t.__name__, C.sizeof(t), size)
    for k, v in offs.items():
        assert getattr(t, k).offset == v, (t.__name__, k, getattr(t, k).offset, v)


_chk(PointLight, 48, range=12, color=16, brightness=28, attenuation=32, depthBias=44)
_chk(SpotLight, 64, outerConeAngle=12, spotDir=32, depthBias=44, innerConeAngle=48, range=52)
_chk(DirectionalLight, 40, shadowing=32, enabled=36)
_chk(SceneLighting, 7088, directional=16, shadowViewDirectional=64, point_lights=128, point_casters=4928,
     spot_lights=5168, spot_casters=6448, shadowViews=6768)
_chk(PerFrameData, 7120, f2PointLightShadowMapDimensions=7088, fAmbientLightingFactor=7112, fHDRIOffsetInRadians=7116)
_chk(PerViewLightingData, 320, WorldFrustumPlanes=192, CameraPosition=288, MaxEnvMapLODLevels=300,
     ScreenDimensions=304, EnvironmentMapDiffuseOnlyIllumination=312)
_chk(MaterialData, 80, uvScaleOffset=48, roughness=64, textureConfig=76)
_chk(Texture2D, 24, width=8, mips=16)
_chk(MaterialDesc, 256, texDiffuse=80, texLocalAO=224)
_chk(GBuffer, 48, width=32, row_pitch_px=40)
_chk(GBufferMSAA, 232, coverage=192, layers=224, coverage_pitch=228)
_chk(MSAASurfaces, 176, coverage=8, normals=40, roughness=72, background=104, normals_pitch_px=112, roughness_pitch_px=128, width=144, layers=152,
     depth_pitch_px=160, normals_fmt=168)
_chk(TonemapperParams, 16)
_chk(BlurParams, 8)
_chk(SSSRConstants, 512, bufferDimensions=448, roughnessThreshold=472, envMapSpecularIrradianceCubemapMipLevelCount=504)
_chk(ShadowMesh, 32, strideBytes=8, numVertices=12, indices=16, indexBits=24, numIndices=28)
_chk(ShadowDraw, 56, matWorldViewProj=32, matWorld=40, numInstances=48, cullMode=52)
_chk(SceneDepthDraw, 48, matWorldViewProj=32, numInstances=40, cullMode=44)
_chk(SceneDepthTargets, 96, primitive=8, coverage=16, layerPrimitive=48, layers=80, pitch=84, coverage_pitch=88, reserved=92)
_chk(SceneSurfaceDraw, 72, matWorldViewProj=32, matWorld=40, matNormal=48, matWorldViewProjPrev=56, numInstances=64, materialIndex=68)
_chk(SceneInterpolantTargets, 48, ip1=8, ip2=16, svPositionCurr=24, svPositionPrev=32, pitch=40, sv_pitch=44)
_chk(SceneQuadTargets, 64, quadUV=48, quad_pitch=56, pad_=60)
_chk(SceneDepthMaskedDraw, 56, material=48)
_chk(ShadowMaskedDraw, 64, texDiffuseAlpha=56)
_chk(ShadowMaskedView, 56, pitchBytes=8, dim=16, linearDepth=20, cameraPosition=24, farPlane=36, draws=40, numDraws=48)
_chk(ShadowView, 56, pitchBytes=8, dim=16, linearDepth=20, cameraPosition=24, farPlane=36, draws=40, numDraws=48)
_chk(ObjectIdDraw, 24, numInstances=4, objID=8, meshID=16, materialID=20)
_chk(OutlineData, 368, matWorldView=64, matNormalView=128, matProj=192, matViewInverse=256, Color=320, uvScaleBias=336, Scale=352, HeightDisplacement=356)
_chk(OutlineDraw, 40, cb=32)
_chk(OutlineTargets, 40, selection=8, writer=16, pitch=24, selection_pitch=28, writer_pitch=32, reserved=36)
_chk(UnlitData, 80, color=64)
_chk(UnlitDraw, 48, cb=32, cullMode=40, reserved=44)
_chk(UnlitTargets, 40, sceneDepth=8, writer=16, pitch=24, depth_pitch=28, writer_pitch=32, reserved=36)
_chk(VertexAxesData, 208, matNormal=64, matViewProj=128, LocalAxisSize=192)
_chk(LineDraw, 64, matModelViewProj=32, color=40, axes=48, numInstances=56, kind=60)
_chk(DisplaceJob, 80, strideBytes=8, numVertices=12, out=16, outStrideBytes=24, reserved=28, heightmap=32, uvScaleOffset=56, displacement=72)
_chk(CacaoConstants, 384, EffectRadius=48, InvSharpness=96, PassIndex=100, PatternRotScaleMatrices=112, NormalsUnpackMul=192, SSAOBufferDimensions=208,
     DepthBufferOffset=240, PerPassFullResUVOffset=248, DeinterleavedDepthBufferNormalisedOffset=312, NormalsWorldToViewspaceMatrix=320)


def mip_level_count(w, h):
    """Image::CalculateMipLevelCount (VQUtils, absent; semantics from EnvironmentMapRendering.cpp:63)."""
    m, n = max(w, h), 1
    while m > 1:
        m >>= 1
        n += 1
    return n


def mip_dim(d0, level):
    return max(1, d0 >> level)


def mip_chain_px(w0, h0, n_mips):
    return sum(mip_dim(w0, l) * mip_dim(h0, l) for l in range(n_mips))


def depth_hierarchy_shapes(w, h):
    """[(rows, cols)] of every level of the depth hierarchy of a w x h frame (vqhip_depth_hierarchy: floor-halved, clamped to 1)"""
    return [(mip_dim(h, l), mip_dim(w, l)) for l in range(mip_level_count(w, h))]


def specular_mip_count(res0):
    return mip_level_count(res0, res0) - 1


def cube_px(res0, n_mips):
    return sum(6 * (res0 >> m) ** 2 for m in range(n_mips))


# ---- vqhip_ssr_classify / vqhip_ssr_intersect (docs/DESIGN_DETAILS.md §7.11) ------------------------------------------------------------------
SSR_MAX_TRAVERSAL_INTERSECTIONS = 256   # above: VQHIP_ERR_UNSUPPORTED (the engine's slider range)
SSR_MAX_MOST_DETAILED_MIP = 5           # above: VQHIP_ERR_UNSUPPORTED
SSR_BLUE_NOISE_SIZE = 128               # g_blue_noise_texture: 128 x 128 R8G8_UNORM


def ssr_remap_lane8x8(lane):
    """FFX_DNSR_Reflections_RemapLane8x8: lane 0..63 of an 8 x 8 tile -> (x, y) inside the tile; four neighbouring lanes form a 2 x 2 quad"""
    return (lane & 1) | ((lane >> 2) & 6), ((lane >> 1) & 3) | ((lane >> 3) & 4)


def pack_ray_coords(x, y, copy_horizontal=False, copy_vertical=False, copy_diagonal=False):
    """PackRayCoords (Common.hlsl:62-71): x in bits 0-14, y in 15-28, the copy flags in 29 / 30 / 31"""
    return (int(bool(copy_diagonal)) << 31) | (int(bool(copy_vertical)) << 30) | (int(bool(copy_horizontal)) << 29) | ((int(y) & 0x3FFF) << 15) | (int(x) & 0x7FFF)


def unpack_ray_coords(packed):
    """UnpackRayCoords (Common.hlsl:73-79): (x, y, copy_horizontal, copy_vertical, copy_diagonal)"""
    packed = int(packed)
    return packed & 0x7FFF, (packed >> 15) & 0x3FFF, bool((packed >> 29) & 1), bool((packed >> 30) & 1), bool((packed >> 31) & 1)


# ---- vqhip_cacao (docs/DESIGN_DETAILS.md §7.14) -------------------------------------------------------------------------------------------------
CACAO_QUALITY_LOWEST, CACAO_QUALITY_LOW, CACAO_QUALITY_MEDIUM, CACAO_QUALITY_HIGH, CACAO_QUALITY_HIGHEST = 0, 1, 2, 3, 4   # FFX_CACAO_Quality
CACAO_PLANE_DEPTHS, CACAO_PLANE_NORMALS, CACAO_PLANE_PING, CACAO_PLANE_PONG = 0, 1, 2, 3
CACAO_PLANE_IMPORTANCE, CACAO_PLANE_IMPORTANCE_PONG, CACAO_PLANE_LOAD_COUNTER = 4, 5, 6   # vqhip_adaptive_cacao only (§7.15)
CACAO_DEPTH_MIPS = 4                    # SSAO_DEPTH_MIP_LEVELS
CACAO_MAX_BLUR_PASSES = 8
CACAO_MAX_DIM = 16384                   # above: VQHIP_ERR_UNSUPPORTED


def cacao_half_dims(w, h):
    """(hw, hh) of the deinterleaved buffers of a w x h frame (FFX_CACAO_UpdateBufferSizeInfo: (w + 1) / 2)"""
    return (w + 1) // 2, (h + 1) // 2
