"""The contract of vqhip_adaptive_cacao (docs/DESIGN_DETAILS.md §7.15) in numpy binary32: FidelityFX CACAO at quality HIGHEST, the level of
FFX_CACAO_DEFAULT_SETTINGS — the stages FFX_CACAO_D3D12Draw (ffx_cacao_impl.cpp:1950-2150) puts between the prepare passes and the blur: CSGenerateQ3Base per pass
(ffx_cacao.hlsl:1150-1161), CSGenerateImportanceMap (:1651-1682), CSPostprocessImportanceMapA (:1689-1710) and B (:1716-1747) with the load counter, and CSGenerateQ3
per pass (:1164-1176, the adaptive branch :995-1048). The arithmetic rules, the samplers and everything the two quality levels share are tests/cacao_ref.py's (§7.14),
imported and unchanged: prepare_depths, prepare_normals, blur, apply. Nothing under oracle/ knows these passes: this file is the checker."""
import numpy as np

from tests import cacao_ref as R
from tests.cacao_ref import D, F, Consts, dot3, dot4, fixed8, from_snorm8, from_unorm8, log2_, exp2_, max0, min_, mirror, sat
from tests.ref_cases import to_unorm8

BASE_TAPS, MAX_TAPS = 5, 32                                          # SSAO_ADAPTIVE_TAP_BASE_COUNT, SSAO_MAX_TAPS
FLEXIBLE_TAPS = MAX_TAPS - BASE_TAPS                                 # SSAO_ADAPTIVE_TAP_FLEXIBLE_COUNT
LIT_BASE_SHARE = D(5 / 32.0)                                         # (SSAO_ADAPTIVE_TAP_BASE_COUNT / (float)SSAO_MAX_TAPS)
LIT_BASE_WEIGHT = D(5 * 4.0)                                         # (float)(SSAO_ADAPTIVE_TAP_BASE_COUNT * 4.0)
LIT_0_8 = D(0.8)
# g_samplePatternMain[0 .. 32): (x, y, weight, log2(length)); the first 12 rows are cacao_ref.SAMPLE_PATTERN
SAMPLE_PATTERN = np.array([
    [0.78488064, 0.56661671, 1.500000, -0.126083], [0.26022232, -0.29575172, 1.500000, -1.064030], [0.10459357, 0.08372527, 1.110000, -2.730563],
    [-0.68286800, 0.04963045, 1.090000, -0.498827], [-0.13570161, -0.64190155, 1.250000, -0.532765], [-0.26193795, -0.08205118, 0.670000, -1.783245],
    [-0.61177456, 0.66664219, 0.710000, -0.044234], [0.43675563, 0.25119025, 0.610000, -1.167283], [0.07884444, 0.86618668, 0.640000, -0.459002],
    [-0.12790935, -0.29869005, 0.600000, -1.729424], [-0.04031125, 0.02413622, 0.600000, -4.792042], [0.16201244, -0.52851415, 0.790000, -1.067055],
    [-0.70991218, 0.47301072, 0.640000, -0.335236], [0.03277707, -0.22349690, 0.600000, -1.982384], [0.68921727, 0.36800742, 0.630000, -0.266718],
    [0.29251814, 0.37775412, 0.610000, -1.422520], [-0.12224089, 0.96582592, 0.600000, -0.426142], [0.11071457, -0.16131058, 0.600000, -2.165947],
    [0.46562141, -0.59747696, 0.600000, -0.189760], [-0.51548797, 0.11804193, 0.600000, -1.246800], [0.89141309, -0.42090443, 0.600000, 0.028192],
    [-0.32402530, -0.01591529, 0.600000, -1.543018], [0.60771245, 0.41635221, 0.600000, -0.605411], [0.02379565, -0.08239821, 0.600000, -3.809046],
    [0.48951152, -0.23657045, 0.600000, -1.189011], [-0.17611565, -0.81696892, 0.600000, -0.513724], [-0.33930185, -0.20732205, 0.600000, -1.698047],
    [-0.91974425, 0.05403209, 0.600000, 0.062246], [-0.15064627, -0.14949332, 0.600000, -1.896062], [0.53180975, -0.35210401, 0.600000, -0.758838],
    [0.41487166, 0.81442589, 0.600000, -0.505648], [-0.24106961, -0.32721516, 0.600000, -1.665244]], np.float64).astype(F)
assert np.array_equal(SAMPLE_PATTERN[:R.NUM_TAPS], R.SAMPLE_PATTERN)


def importance_dims(hw, hh):
    return (hw + 1) // 2, (hh + 1) // 2


def _consts(c):
    return c if isinstance(c, Consts) else Consts(c)


def bilinear_r8(plane, u, v):
    """SampleLevel(g_LinearClampSampler, uv, 0).x of an R8_UNORM plane [rows, cols] (§3.4): cacao_ref's bilinear clamp fetch"""
    return R._bilinear_clamp(np.asarray(plane, np.uint8), np.asarray(u, F), np.asarray(v, F))


# ---- GenerateSSAOShadowsInternal(qualityLevel 3, adaptiveBase) -------------------------------------------------------------------------------------
def _tap_depth(depths, p, level, tx, ty):
    """SampleLevel(g_ViewspaceDepthTapSampler, uv, mip): point filter, clamp, the mip `level` selected per pixel"""
    hh, hw = depths[0].shape[1:]
    z = np.zeros(tx.shape, F)
    for k in range(4):
        mw, mh = R.mip_dims(hw, hh, k)
        sel = level == k
        if sel.any():
            z[sel] = depths[k][p][np.clip(R._floor_i(ty[sel] * F(mh)), 0, mh - 1), np.clip(R._floor_i(tx[sel] * F(mw)), 0, mw - 1)].astype(F)
    return z


def _hit(c, n, pc, falloff, tx, ty, z):
    """DepthBufferUVToViewspace, CalculatePixelObscurance and the haloing-reduction weight of one hit -> (obscurance, 0.6 * reduct + 0.4)"""
    hit = [(c.DepthBufferUVToViewMul[0] * tx + c.DepthBufferUVToViewAdd[0]) * z, (c.DepthBufferUVToViewMul[1] * ty + c.DepthBufferUVToViewAdd[1]) * z, z]
    delta = [hit[k] - pc[k] for k in range(3)]
    obs = R._obscurance(n, delta, falloff, c)
    reduct = sat(max0(-delta[2]) * c.NegRecEffectRadius + F(2.0))
    return obs, D(0.6) * reduct + R.LIT_0_4


def _pixels(depths, normals, c, xs, ys, adaptive=None):
    """The pixels (xs, ys) of pass c.PassIndex. adaptive None: adaptiveBase = true -> (obscuranceSum / weightSum, weightSum). Otherwise adaptive = (importance map
    uint8 [ih, iw], base uint8 [4, hh, hw, 2], counter): adaptiveBase = false -> (occlusion, packed edges, taps): taps = additionalSamplesTo, the number of taps
    the texel's value rests on, the base pass's five included."""
    p = c.PassIndex
    d0 = depths[0][p].astype(F)
    hh, hw = d0.shape
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    sx, sy = xs.astype(F), ys.astype(F)
    inv_d, inv_s = c.DeinterleavedDepthBufferInverseDimensions, c.SSAOBufferInverseDimensions
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        uvx = (sx + F(0.5)) * inv_d[0] + c.DeinterleavedDepthBufferNormalisedOffset[0]
        uvy = (sy + F(0.5)) * inv_d[1] + c.DeinterleavedDepthBufferNormalisedOffset[1]
        gx, _ = fixed8(uvx * F(hw) - F(0.5))
        gy, _ = fixed8(uvy * F(hh) - F(0.5))
        at = lambda ax, ay: d0[mirror(ay, hh), mirror(ax, hw)]
        pix_z, pix_l, pix_t = at(gx, gy), at(gx - 1, gy), at(gx, gy - 1)
        pix_r, pix_b = at(gx + 1, gy), at(gx, gy + 1)
        nspx, nspy = (sx + F(0.5)) * inv_s[0], (sy + F(0.5)) * inv_s[1]
        pc = [(c.NDCToViewMul[0] * nspx + c.NDCToViewAdd[0]) * pix_z, (c.NDCToViewMul[1] * nspy + c.NDCToViewAdd[1]) * pix_z, pix_z]
        nrm = from_snorm8(normals[p][ys, xs, :3])
        n = [nrm[:, 0], nrm[:, 1], nrm[:, 2]]
        dir_rb = [pc[2] * c.NDCToViewMul[0] * inv_s[0], pc[2] * c.NDCToViewMul[1] * inv_s[1]]
        too_close = sat(np.sqrt(dot3(pc, pc)) * c.EffectSamplingRadiusNearLimitRec) * D(0.8) + D(0.2)
        radius = c.EffectRadius * too_close
        lookup = (D(0.85) * radius) / dir_rb[0]
        falloff = F(-1.0) / (radius * radius)
        rs = c.PatternRotScaleMatrices[R._trunc_u(sy * F(2.0) + sx) % 5]
        rot = [rs[:, k] * lookup for k in range(4)]
        pc = [v * c.DepthPrecisionOffsetMod for v in pc]
        mip_offset = log2_(lookup) + R.MIP_GLOBAL_OFFSET
        obs_sum, weight_sum = np.zeros_like(pix_z), np.zeros_like(pix_z)

        def offsets(i):
            s = SAMPLE_PATTERN[i]
            ox = np.rint(rot[0] * s[0] + rot[1] * s[1]).astype(F)
            oy = np.rint(rot[2] * s[0] + rot[3] * s[1]).astype(F)
            return ox, oy, np.clip(R._floor_i((s[3] + mip_offset) + F(0.5)), 0, 3)

        if adaptive is None:
            # SSAOTap x 5 (:658-698): offset * inverse dimensions + uv; the weight carries weightMod = 1.0 * newSample.z
            for i in range(BASE_TAPS):
                ox, oy, level = offsets(i)
                weight_mod = F(1.0) * SAMPLE_PATTERN[i][2]
                for sign in (F(1.0), F(-1.0)):
                    tx, ty = (sign * ox) * inv_d[0] + uvx, (sign * oy) * inv_d[1] + uvy
                    obs, w = _hit(c, n, pc, falloff, tx, ty, _tap_depth(depths, p, level, tx, ty))
                    w = w * weight_mod
                    obs_sum = obs_sum + obs * w
                    weight_sum = weight_sum + w
            return (obs_sum / weight_sum).astype(F), weight_sum.astype(F)

        importance_map, base, counter = adaptive
        # CalculateEdges (:213-219), detail AO (:877-905), normal-based edges (:908-935): as at HIGH
        e = [pix_l - pix_z, pix_r - pix_z, pix_t - pix_z, pix_b - pix_z]
        adj = [e[0] + e[1], e[1] + e[0], e[2] + e[3], e[3] + e[2]]
        e = [min_(np.abs(a), np.abs(b)) for a, b in zip(e, adj)]
        edges = [sat(D(1.3) - a / (pix_z * D(0.040))) for a in e]
        vdz = [pc[0] / pc[2], pc[1] / pc[2], np.ones_like(pc[2])]
        zero = np.zeros_like(pc[2])
        deltas = []
        for z, b in ((pix_l, [-dir_rb[0], zero, zero]), (pix_r, [dir_rb[0], zero, zero]), (pix_t, [zero, -dir_rb[1], zero]), (pix_b, [zero, dir_rb[1], zero])):
            dz = z - pc[2]
            deltas.append([b[k] + vdz[k] * dz for k in range(3)])
        add_obs = [R._obscurance(n, d, F(4.0) * falloff, c) for d in deltas]
        obs_sum = (F(0.0) + c.DetailAOStrength * dot4(add_obs, edges)).astype(F)
        np_ = normals[p]
        for k, (dx, dy) in enumerate(((-1, 0), (1, 0), (0, -1), (0, 1))):
            ax, ay = xs + dx, ys + dy
            ok = (ax >= 0) & (ax < hw) & (ay >= 0) & (ay < hh)
            nb = np.where(ok[:, None], from_snorm8(np_[np.clip(ay, 0, hh - 1), np.clip(ax, 0, hw - 1), :3]), F(0))
            edges[k] = edges[k] * sat(dot3(n, [nb[:, 0], nb[:, 1], nb[:, 2]]) + D(0.5))
        # the adaptive branch (:995-1048)
        importance = bilinear_r8(importance_map, nspx + c.PerPassFullResUVOffset[0], nspy + c.PerPassFullResUVOffset[1])
        obs_sum = obs_sum * (LIT_BASE_SHARE + importance * F(FLEXIBLE_TAPS) / F(MAX_TAPS))
        base_values = from_unorm8(base[p][ys, xs])
        weight_sum = weight_sum + base_values[:, 1] * LIT_BASE_WEIGHT
        obs_sum = obs_sum + base_values[:, 0] * weight_sum
        limiter = importance_limiter(counter, c)
        importance = importance * limiter
        count = F(FLEXIBLE_TAPS) * importance
        count = count + F(1.5)
        to = np.minimum(MAX_TAPS, R._trunc_u(count) + BASE_TAPS)
        # SSAOGetSampleData (:742-757): round(mul(rotScale, xy)) * inverse dimensions, then SSAOGetHits2 (:759-768): uv + offset, uv - offset; SSAOAddHits
        # (:770-792): the weight is overwritten per hit and newSample.z never enters. Tap i is live for the texels with i < to.
        for i in range(BASE_TAPS, MAX_TAPS):
            live = i < to
            if not live.any():
                break
            ox, oy, level = offsets(i)
            ox, oy = ox * inv_d[0], oy * inv_d[1]
            for tx, ty in ((uvx + ox, uvy + oy), (uvx - ox, uvy - oy)):
                obs, w = _hit(c, n, pc, falloff, tx, ty, _tap_depth(depths, p, level, tx, ty))
                obs_sum = np.where(live, obs_sum + obs * w, obs_sum)
                weight_sum = np.where(live, weight_sum + w, weight_sum)
        obscurance = obs_sum / weight_sum
        fade = sat(pc[2] * c.EffectFadeOutMul + c.EffectFadeOutAdd)
        edge_fade = sat((F(1.0) - edges[0] - edges[1]) * D(0.35)) + sat((F(1.0) - edges[2] - edges[3]) * D(0.35))
        fade = fade * sat(F(1.0) - edge_fade)
        obscurance = min_(c.EffectShadowStrength * obscurance, c.EffectShadowClamp) * fade
        occlusion = exp2_(c.EffectShadowPow * log2_(sat(F(1.0) - obscurance)))
    return occlusion.astype(F), R.pack_edges(edges).astype(F), to


def importance_limiter(counter, c):
    """saturate(AdaptiveSampleCountLimit / ((float)counter * LoadCounterAvgDiv)): limit / 0 = +inf -> 1, 0 / 0 = NaN -> 0"""
    with np.errstate(invalid="ignore", divide="ignore"):
        avg = F(np.uint32(counter)) * c.LoadCounterAvgDiv
        return F(sat(c.AdaptiveSampleCountLimit / avg))


def _all_pixels(hh, hw):
    ys, xs = (a.ravel() for a in np.mgrid[0:hh, 0:hw])
    return xs, ys


def generate_base(depths, normals, per_pass):
    """The four CSGenerateQ3Base dispatches -> uint8 [4, hh, hw, 2] (R8G8_UNORM): (obscuranceSum / weightSum, weightSum / 20), what the PONG slices hold until the blur"""
    hh, hw = depths[0].shape[1:]
    out = np.zeros((4, hh, hw, 2), np.uint8)
    xs, ys = _all_pixels(hh, hw)
    for p in range(4):
        shadow, weight = _pixels(depths, normals, _consts(per_pass[p]), xs, ys)
        out[p, ys, xs, 0], out[p, ys, xs, 1] = to_unorm8(shadow), to_unorm8(weight / LIT_BASE_WEIGHT)
    return out


def importance_generate(base, c):
    """CSGenerateImportanceMap (:1651-1682): base uint8 [4, hh, hw, 2] -> uint8 [ih, iw]. `avg` feeds nothing."""
    c = _consts(c)
    _, hh, hw, _ = base.shape
    iw, ih = importance_dims(hw, hh)
    u = (F(2.0) * np.arange(iw, dtype=F) + F(0.5)) * c.SSAOBufferInverseDimensions[0]
    v = (F(2.0) * np.arange(ih, dtype=F) + F(0.5)) * c.SSAOBufferInverseDimensions[1]
    ix, _ = fixed8(u * F(hw) - F(0.5))                                                          # GatherRed(g_PointClampSampler): the bilinear footprint, clamped
    iy, _ = fixed8(v * F(hh) - F(0.5))
    xs, ys = (np.clip(ix, 0, hw - 1), np.clip(ix + 1, 0, hw - 1)), (np.clip(iy, 0, hh - 1), np.clip(iy + 1, 0, hh - 1))
    min_v, max_v = np.full((ih, iw), F(1.0)), np.full((ih, iw), F(0.0))
    for i in range(4):
        for yy in ys:
            for xx in xs:
                val = from_unorm8(base[i, :, :, 0][np.ix_(yy, xx)])
                val = F(1.0) - c.EffectShadowStrength * val
                val = exp2_(c.EffectShadowPow * log2_(sat(val)))
                max_v, min_v = np.maximum(max_v, val), np.minimum(min_v, val)
    diff = max_v - min_v
    return to_unorm8(exp2_(LIT_0_8 * log2_(sat(diff * F(2.0)))))


def _postprocess(src, c, second, rows, cols):
    """The body shared by CSPostprocessImportanceMapA and B for the threads [0, rows) x [0, cols) -> float32: B (second) mirrors A's tap pattern"""
    inv = c.ImportanceMapInverseDimensions
    ty, tx = np.mgrid[0:rows, 0:cols]
    u, v = (tx.astype(F) + F(0.5)) * inv[0], (ty.astype(F) + F(0.5)) * inv[1]
    centre = bilinear_r8(src, u, v)
    hx, hy = F(0.5) * inv[0], F(0.5) * inv[1]
    if not second:
        offs = ((-hx * F(3.0), -hy), (hx, -hy * F(3.0)), (hx * F(3.0), hy), (-hx, hy * F(3.0)))
    else:
        offs = ((-hx, -hy * F(3.0)), (hx * F(3.0), -hy), (hx, hy * F(3.0)), (-hx * F(3.0), hy))
    vals = [bilinear_r8(src, u + F(a), v + F(b)) for a, b in offs]
    avg_val = dot4(vals, [F(0.25)] * 4)
    max_val = np.maximum(centre, np.maximum(np.maximum(vals[0], vals[2]), np.maximum(vals[1], vals[3])))
    return (max_val + F(1.0) * (avg_val - max_val)).astype(F)                                  # lerp(maxVal, avgVal, cSmoothenImportance = 1.0), the contract's lerp


def importance_a(importance, c):
    """CSPostprocessImportanceMapA (:1689-1710): map uint8 [ih, iw] -> its pong"""
    ih, iw = importance.shape
    return to_unorm8(_postprocess(importance, _consts(c), False, ih, iw))


def importance_b(importance_pong, c, count_threads_outside_the_map=True):
    """CSPostprocessImportanceMapB (:1716-1747): pong -> (map, load counter). The dispatch is ceil(iw / 8) x ceil(ih / 8) groups of 8 x 8 with no bounds test: a thread
    outside the map samples clamped texels, its store is dropped, and its InterlockedAdd on element 0 executes. count_threads_outside_the_map = False is the other
    reading (only threads of the map add), kept for the test that tells the two apart."""
    c = _consts(c)
    ih, iw = importance_pong.shape
    rows, cols = (ih + 7) // 8 * 8, (iw + 7) // 8 * 8
    val = _postprocess(importance_pong, c, True, rows, cols)
    ty, tx = np.mgrid[0:rows, 0:cols]
    adds = (tx % 3 + ty % 3) == 0
    if not count_threads_outside_the_map:
        adds &= (tx < iw) & (ty < ih)
    sums = R._trunc_u(sat(val) * F(255.0) + F(0.5))
    return to_unorm8(val[:ih, :iw]), int(sums[adds].sum()) & 0xFFFFFFFF


def generate_adaptive(depths, normals, per_pass, importance, base, counter):
    """The four CSGenerateQ3 dispatches -> (ping uint8 [4, hh, hw, 2], taps int64 [4, hh, hw]: the tap count of every texel, 6 .. 32)"""
    hh, hw = depths[0].shape[1:]
    ping, taps = np.zeros((4, hh, hw, 2), np.uint8), np.zeros((4, hh, hw), np.int64)
    xs, ys = _all_pixels(hh, hw)
    for p in range(4):
        occ, packed, to = _pixels(depths, normals, _consts(per_pass[p]), xs, ys, (importance, base, counter))
        ping[p, ys, xs, 0], ping[p, ys, xs, 1], taps[p, ys, xs] = to_unorm8(occ), to_unorm8(packed), to
    return ping, taps


def wave_tap_stats(taps):
    """Per wave (one 8 x 8 tile of one slice; the lanes inside the slice only) the maximum and the mean tap count -> (max [n], mean [n])"""
    _, hh, hw = taps.shape
    mx, mean = [], []
    for p in range(4):
        for y in range(0, hh, 8):
            for x in range(0, hw, 8):
                t = taps[p, y:y + 8, x:x + 8]
                mx.append(t.max())
                mean.append(t.mean())
    return np.array(mx), np.array(mean)


def frame(depth, normals, fmt, shared, per_pass, blur_passes=2):
    """vqhip_adaptive_cacao in full -> dict: depths, normals, base (PONG before the blur), importance_pong (after A), importance (after B), counter, ping, pong (None
    when blur_passes == 0: the PONG slices then still hold base), ao, stats. stats: `tap_histogram` int64 [33] over every texel's tap count, `counter`, `limiter`,
    `wave_max` / `wave_mean` (wave_tap_stats), `wave_max_mean` and `wave_mean_mean`: the taps a wave executes against those its lanes need, averaged over the waves."""
    cs = Consts(shared)
    cp = [Consts(per_pass[i]) for i in range(4)]
    h, w = np.asarray(depth).shape
    depths = R.prepare_depths(depth, cs)
    nrm = R.prepare_normals(normals, fmt, cs)
    base = generate_base(depths, nrm, cp)
    imp0 = importance_generate(base, cs)
    imp_pong = importance_a(imp0, cs)
    imp, counter = importance_b(imp_pong, cs)
    ping, taps = generate_adaptive(depths, nrm, cp, imp, base, counter)
    pong = R.blur(ping, cp, blur_passes) if blur_passes else None
    ao = R.apply(pong if blur_passes else ping, cs, w, h)
    wmax, wmean = wave_tap_stats(taps)
    stats = {"tap_histogram": np.bincount(taps.ravel(), minlength=MAX_TAPS + 1), "counter": counter, "limiter": float(importance_limiter(counter, cp[0])),
             "wave_max": wmax, "wave_mean": wmean, "wave_max_mean": float(wmax.mean()), "wave_mean_mean": float(wmean.mean()), "taps": taps}
    return {"depths": depths, "normals": nrm, "base": base, "importance_generated": imp0, "importance_pong": imp_pong, "importance": imp, "counter": counter,
            "ping": ping, "pong": pong, "ao": ao, "stats": stats}
