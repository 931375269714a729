"""Host mirror of FidelityFX CACAO's constant setup (AMDFidelityFX/CACAO/ffx_cacao.h:72-90, ffx_cacao.cpp:48-262): FFX_CACAO_DEFAULT_SETTINGS,
FFX_CACAO_UpdateBufferSizeInfo, FFX_CACAO_UpdateConstants and FFX_CACAO_UpdatePerPassConstants, operation by operation in binary32. The engine keeps calling
FidelityFX's own functions and hands the five blocks to vqhip_cacao or vqhip_adaptive_cacao; this mirror exists for callers that have no FidelityFX at hand (the tests, the benchmark
script). tests/test_cacao_cpu.py pins it to the output of the reference's own C++ (tests/golden/cacao_constants.json). Pure numpy; importable without a GPU."""
import numpy as np

from . import abi

F = np.float32

# FFX_CACAO_DEFAULT_SETTINGS (ffx_cacao.h:72-90). qualityLevel there is HIGHEST: vqhip_adaptive_cacao (docs/DESIGN_DETAILS.md §7.15); vqhip_cacao runs HIGH (§7.14).
DEFAULT_SETTINGS = {
    "radius": 1.2, "shadowMultiplier": 1.0, "shadowPower": 1.50, "shadowClamp": 0.98, "horizonAngleThreshold": 0.06, "fadeOutFrom": 50.0, "fadeOutTo": 300.0,
    "qualityLevel": abi.CACAO_QUALITY_HIGHEST, "adaptiveQualityLimit": 0.45, "blurPassCount": 2, "sharpness": 0.98, "temporalSupersamplingAngleOffset": 0.0,
    "temporalSupersamplingRadiusOffset": 0.0, "detailShadowStrength": 0.5, "generateNormals": False, "bilateralSigmaSquared": 5.0,
    "bilateralSimilarityDistanceSigma": 0.01,
}


def settings(**overrides):
    """FFX_CACAO_DEFAULT_SETTINGS with `overrides`; unknown names are refused"""
    s = dict(DEFAULT_SETTINGS)
    for k, v in overrides.items():
        if k not in s:
            raise KeyError(f"FFX_CACAO_Settings has no field {k!r}")
        s[k] = v
    return s


def buffer_size_info(width, height, use_downsampled_ssao=False):
    """FFX_CACAO_UpdateBufferSizeInfo (ffx_cacao.cpp:48-104) as a dict of the struct's fields"""
    half_w, half_h = (width + 1) // 2, (height + 1) // 2
    quarter_w, quarter_h = (half_w + 1) // 2, (half_h + 1) // 2
    eighth_w, eighth_h = (quarter_w + 1) // 2, (quarter_h + 1) // 2
    b = {"inputOutputBufferWidth": width, "inputOutputBufferHeight": height, "depthBufferXOffset": 0, "depthBufferYOffset": 0,
         "depthBufferWidth": width, "depthBufferHeight": height, "deinterleavedDepthBufferXOffset": 0, "deinterleavedDepthBufferYOffset": 0}
    if use_downsampled_ssao:
        b.update(ssaoBufferWidth=quarter_w, ssaoBufferHeight=quarter_h, deinterleavedDepthBufferWidth=quarter_w, deinterleavedDepthBufferHeight=quarter_h,
                 importanceMapWidth=eighth_w, importanceMapHeight=eighth_h, downsampledSsaoBufferWidth=half_w, downsampledSsaoBufferHeight=half_h)
    else:
        b.update(ssaoBufferWidth=half_w, ssaoBufferHeight=half_h, deinterleavedDepthBufferWidth=half_w, deinterleavedDepthBufferHeight=half_h,
                 importanceMapWidth=quarter_w, importanceMapHeight=quarter_h, downsampledSsaoBufferWidth=1, downsampledSsaoBufferHeight=1)
    return b


def _clamp(v, lo, hi):
    v, lo, hi = F(v), F(lo), F(hi)
    v = v if v > lo else lo                      # FFX_CACAO_MAX(value, lower)
    return v if v < hi else hi                   # FFX_CACAO_MIN(.., upper)


def _set2(field, a, b):
    field[0], field[1] = float(a), float(b)


def update_constants(consts, s, bsi, proj, normals_to_view):
    """FFX_CACAO_UpdateConstants (ffx_cacao.cpp:106-230). proj / normals_to_view: 4 x 4, row-major (FFX_CACAO_Matrix4x4.elements)"""
    proj = np.asarray(proj, F)
    one = F(1.0)
    consts.BilateralSigmaSquared = float(F(s["bilateralSigmaSquared"]))
    consts.BilateralSimilarityDistanceSigma = float(F(s["bilateralSimilarityDistanceSigma"]))
    m = np.eye(4, dtype=F) if s["generateNormals"] else np.asarray(normals_to_view, F)
    for i in range(4):
        for j in range(4):
            consts.NormalsWorldToViewspaceMatrix.m[i][j] = float(m[i, j])
    # 9.0f / (float)(w * h * 255.0): the product is a double
    consts.LoadCounterAvgDiv = float(F(9.0) / F(float(bsi["importanceMapWidth"] * bsi["importanceMapHeight"]) * 255.0))
    mul, add = -proj[3, 2], proj[2, 2]
    if mul * add < 0:
        add = -add
    _set2(consts.DepthUnpackConsts, mul, add)
    tan_y, tan_x = one / proj[1, 1], one / proj[0, 0]
    _set2(consts.CameraTanHalfFOV, tan_x, tan_y)
    ndc_mul = (tan_x * F(2.0), tan_y * F(-2.0))
    ndc_add = (tan_x * F(-1.0), tan_y * F(1.0))
    _set2(consts.NDCToViewMul, *ndc_mul)
    _set2(consts.NDCToViewAdd, *ndc_add)
    ratio = F(bsi["inputOutputBufferWidth"]) / F(bsi["depthBufferWidth"])
    border = (one - ratio) / F(2.0)
    for i in range(2):
        consts.DepthBufferUVToViewMul[i] = float(ndc_mul[i] / ratio)
        consts.DepthBufferUVToViewAdd[i] = float(ndc_add[i] - ndc_mul[i] * border / ratio)
    radius = F(s["radius"])
    consts.EffectRadius = float(_clamp(radius, 0.0, 100000.0))
    consts.EffectShadowStrength = float(_clamp(F(s["shadowMultiplier"]) * F(4.3), 0.0, 10.0))
    consts.EffectShadowPow = float(_clamp(s["shadowPower"], 0.0, 10.0))
    consts.EffectShadowClamp = float(_clamp(s["shadowClamp"], 0.0, 1.0))
    fade = F(s["fadeOutTo"]) - F(s["fadeOutFrom"])
    consts.EffectFadeOutMul = float(F(-1.0) / fade)
    consts.EffectFadeOutAdd = float(F(s["fadeOutFrom"]) / fade + one)
    consts.EffectHorizonAngleThreshold = float(_clamp(s["horizonAngleThreshold"], 0.0, 1.0))
    near_limit = radius * F(1.2)
    consts.DepthPrecisionOffsetMod = float(F(0.9992))
    if s["qualityLevel"] <= abi.CACAO_QUALITY_LOW:
        near_limit = near_limit * F(1.50)
        if s["qualityLevel"] == abi.CACAO_QUALITY_LOWEST:
            consts.EffectRadius = float(F(consts.EffectRadius) * F(0.8))
    near_limit = near_limit / tan_y
    consts.EffectSamplingRadiusNearLimitRec = float(one / near_limit)
    consts.AdaptiveSampleCountLimit = float(F(s["adaptiveQualityLimit"]))
    consts.NegRecEffectRadius = float(F(-1.0) / F(consts.EffectRadius))
    consts.InvSharpness = float(_clamp(one - F(s["sharpness"]), 0.0, 1.0))
    consts.DetailAOStrength = float(F(s["detailShadowStrength"]))
    for name, w, h in (("SSAOBuffer", "ssaoBufferWidth", "ssaoBufferHeight"), ("DepthBuffer", "depthBufferWidth", "depthBufferHeight"),
                       ("InputOutputBuffer", "inputOutputBufferWidth", "inputOutputBufferHeight"), ("ImportanceMap", "importanceMapWidth", "importanceMapHeight"),
                       ("DeinterleavedDepthBuffer", "deinterleavedDepthBufferWidth", "deinterleavedDepthBufferHeight")):
        _set2(getattr(consts, name + "Dimensions"), F(bsi[w]), F(bsi[h]))
        _set2(getattr(consts, name + "InverseDimensions"), one / F(bsi[w]), one / F(bsi[h]))
    consts.DepthBufferOffset[0], consts.DepthBufferOffset[1] = bsi["depthBufferXOffset"], bsi["depthBufferYOffset"]
    _set2(consts.DeinterleavedDepthBufferOffset, F(bsi["deinterleavedDepthBufferXOffset"]), F(bsi["deinterleavedDepthBufferYOffset"]))
    _set2(consts.DeinterleavedDepthBufferNormalisedOffset, F(bsi["deinterleavedDepthBufferXOffset"]) / F(bsi["deinterleavedDepthBufferWidth"]),
          F(bsi["deinterleavedDepthBufferYOffset"]) / F(bsi["deinterleavedDepthBufferHeight"]))
    consts.NormalsUnpackMul, consts.NormalsUnpackAdd = 2.0, -1.0
    return consts


def update_per_pass_constants(consts, s, bsi, pass_index):
    """FFX_CACAO_UpdatePerPassConstants (ffx_cacao.cpp:232-263). cosf / sinf are numpy's binary32 cosine / sine: the matrices may differ from a libm's by one ulp"""
    _set2(consts.PerPassFullResUVOffset, F(pass_index % 2) / F(bsi["ssaoBufferWidth"]), F(pass_index // 2) / F(bsi["ssaoBufferHeight"]))
    consts.PassIndex = pass_index
    sub_pass_count = 5
    spmap = (0, 1, 4, 3, 2)
    a = pass_index
    for sub_pass in range(sub_pass_count):
        b = spmap[sub_pass]
        angle0 = (F(a) + F(b) / F(sub_pass_count)) * F(3.1415926535897932384626433832795) * F(0.5)
        ca, sa = np.cos(angle0, dtype=F), np.sin(angle0, dtype=F)
        scale = F(1.0) + (F(a) - F(1.5) + (F(b) - (F(sub_pass_count) - F(1.0)) * F(0.5)) / F(sub_pass_count)) * F(0.07)
        m = consts.PatternRotScaleMatrices[sub_pass]
        m[0], m[1], m[2], m[3] = float(scale * ca), float(scale * -sa), float(-scale * sa), float(-scale * ca)
    return consts


def constants(width, height, proj, normals_to_view, s=None):
    """(shared, [4 per-pass blocks]) as FFX_CACAO_D3D12Draw uploads them (ffx_cacao_impl.cpp:1967-1978): every per-pass block is UpdateConstants +
    UpdatePerPassConstants. s: a settings() dict; None: the defaults at quality HIGH, for vqhip_cacao. settings() itself, HIGHEST with adaptiveQualityLimit 0.45, is
    what vqhip_adaptive_cacao takes: LoadCounterAvgDiv, AdaptiveSampleCountLimit and ImportanceMapDimensions are filled either way."""
    s = settings(qualityLevel=abi.CACAO_QUALITY_HIGH) if s is None else s
    bsi = buffer_size_info(width, height)
    shared = update_constants(abi.CacaoConstants(), s, bsi, proj, normals_to_view)
    per_pass = (abi.CacaoConstants * 4)()
    for i in range(4):
        update_constants(per_pass[i], s, bsi, proj, normals_to_view)
        update_per_pass_constants(per_pass[i], s, bsi, i)
    return shared, per_pass
