"""The contract of vqhip_ssr_reproject (docs/DESIGN_DETAILS.md §7.13) in numpy binary32: Reproject.hlsl:CSMain + ffx_denoiser_reflections_reproject.h / _common.h /
_config.h and the FFX_DNSR_Reflections_* overrides of ScreenSpaceReflections/Common.hlsl for every 8 x 8 tile of the denoiser tile list — every expression as
written, one rounding per operation, left to right, in either arithmetic reading, under the rules §7.11 / §7.12 fix (imported from tests/ssr_trace_ref.py and
tests/ssr_denoise_ref.py). The centre radiance and ray length are NOT rounded through binary16; the 16 x 16 neighbourhood is. Bilinear history fetches: texels
decoded to binary32, CLAMP, 8-bit fractions, the blend4 FMA chain (`sample_bilinear`: ssr_denoise_ref.sample_average for any plane). The R11G11B10_FLOAT encode of
the average radiance is stated here (`encode_r11g11b10`). Nothing under oracle/ knows this pass: this file is the checker."""
import numpy as np

from tests.depth_ref import _fma32, decode_normals01, normalize32
from tests.ssr_denoise_ref import (F, RADIUS, _apron, _at, _centre, _dot, _floor_i, _length, _lerp, _nb, exp_, f16r, kernel_weight, listed_tiles,
                                   temporal_variance, luminance)
from tests.ssr_trace_ref import _ftoi, _max2, _min2, _mul_m, matrix
from vqengine_amd import abi

THRESHOLD = F(0.9)                      # FFX_DNSR_REFLECTIONS_DISOCCLUSION_THRESHOLD
HALF_THRESHOLD = F(0.9) / F(2.0)
MAX_SAMPLES = F(32.0)                   # CSMain passes 32


def encode_r11g11b10(rgb):
    """float32 [..., 3] -> DXGI R11G11B10_FLOAT words uint32 [...]: ONE rounding to nearest even from binary32 straight to the 6 / 6 / 5-bit mantissas (5-bit
    exponent, bias 15), denormals kept, overflow to inf, negative values and -0 -> 0, NaN -> exponent 31 with the top mantissa bit"""
    u = np.ascontiguousarray(rgb, F).view(np.uint32).astype(np.int64)
    word = np.zeros(u.shape[:-1], np.int64)
    for ch, (shift_out, mb) in enumerate(((0, 6), (11, 6), (22, 5))):
        b = u[..., ch]
        mag, e, m = b & 0x7FFFFFFF, ((b >> 23) & 0xFF) - 112, (b & 0x7FFFFF) | 0x800000          # e: the exponent re-biased to 15
        sh = np.where(e >= 1, 23 - mb, np.clip((23 - mb) + (1 - e), 0, 40))                     # a denormal result drops (1 - e) more bits
        val = np.where(e >= 1, mag - (112 << 23), m)                                             # normal: exponent and mantissa as one integer, the carry runs into the exponent
        q, rem, half = val >> sh, val & ((np.int64(1) << sh) - 1), np.int64(1) << (sh - 1)
        q = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
        q = np.minimum(q, 31 << mb)                                                              # overflow (and +inf) -> inf
        q = np.where(mag > 0x7F800000, (31 << mb) | (1 << (mb - 1)), q)                          # NaN of either sign
        q = np.where((b >> 31 != 0) & (mag <= 0x7F800000), 0, q)                                 # negative, -0, -inf
        word |= q << shift_out
    return word.astype(np.uint32)


def sample_bilinear(plane, u, v):
    """SampleLevel(g_linear_sampler, uv, 0) on float32 [H,W] or [H,W,C] (already decoded): bilinear, CLAMP, §3.4 — 8-bit fractions, the blend4 FMA chain, addresses
    clamped, a NaN coordinate as _floor_i defines. Returns an array of u's shape (+ [C])."""
    h, w = plane.shape[:2]
    fx, fy = _floor_i((u * F(w) - F(0.5)) * F(256.0) + F(0.5)), _floor_i((v * F(h) - F(0.5)) * F(256.0) + F(0.5))
    ix, iy = fx >> 8, fy >> 8
    wx, wy = (fx & 255).astype(F) * F(0.00390625), (fy & 255).astype(F) * F(0.00390625)
    x0, x1, y0, y1 = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1), np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
    w00, w10, w01, w11 = (F(1) - wx) * (F(1) - wy), wx * (F(1) - wy), (F(1) - wx) * wy, wx * wy
    c00, c10, c01, c11 = plane[y0, x0], plane[y0, x1], plane[y1, x0], plane[y1, x1]
    if plane.ndim == 3:
        w00, w10, w01, w11 = (a[..., None] + np.zeros(c00.shape, F) for a in (w00, w10, w01, w11))
    return _fma32(w11, c11, _fma32(w01, c01, _fma32(w10, c10, w00 * c00)))


def load_texel(plane, x, y):
    """Texture.Load at integer coordinates of any sign: outside the frame 0"""
    h, w = plane.shape[:2]
    ok = (x >= 0) & (y >= 0) & (x < w) & (y < h)
    g = plane[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]
    return np.where(ok.reshape(ok.shape + (1,) * (g.ndim - ok.ndim)), g, F(0)).astype(F)


def linear_depth_uv(M, u, v, z):
    """FFX_DNSR_Reflections_GetLinearDepth(uv, depth): |z / w| of InvProjectPosition; only columns 2 and 3 are formed"""
    cy = F(1.0) - v
    cx_, cy_ = F(2.0) * u - F(1.0), F(2.0) * cy - F(1.0)
    pz = ((cx_ * M[0, 2] + cy_ * M[1, 2]) + z * M[2, 2]) + F(1.0) * M[3, 2]
    pw = ((cx_ * M[0, 3] + cy_ * M[1, 3]) + z * M[2, 3]) + F(1.0) * M[3, 3]
    return np.abs(pz / pw)


def _norm3(n01, dxc):
    """normalize(2.0 * n - 1.0) of [..., 3] -> tuple"""
    n = normalize32(F(2.0) * n01 - F(1.0), dxc)
    return n[..., 0], n[..., 1], n[..., 2]


def disocclusion_factor(n, hn, ld, hld, dxc):
    """FFX_DNSR_Reflections_GetDisocclusionFactor: (1 * exp((-|1 - max(0, dot(n, hn))|) * 1.4)) * exp(((-|hld - ld|) / ld) * 1)"""
    d = _dot(n, hn, dxc)
    a = exp_((-np.abs(F(1.0) - _max2(np.zeros(d.shape, F), d))) * F(1.4))
    b = exp_(((-np.abs(hld - ld)) / ld) * F(1.0))
    return (F(1.0) * a) * b


def _frac(x):
    return x - np.floor(x)


def downsample(rad_w):
    """the 8 x 8 -> 1 sum of [T,8,8,4] (radiance * weight, weight): stored through binary16, three levels, each summed in binary32 as
    ((p(ox,oy) + p(ix,oy)) + p(ox,iy)) + p(ix,iy) and stored through binary16 again. Returns [T,4]."""
    p = f16r(rad_w)
    for _ in range(3):
        p = f16r(((p[:, 0::2, 0::2] + p[:, 0::2, 1::2]) + p[:, 1::2, 0::2]) + p[:, 1::2, 1::2])          # [y, x]: (ox,oy) + (ix,oy) + (ox,iy) + (ix,iy)
    return p[:, 0, 0]


def reproject(tile_list, count, depth, normals, normal_fmt, rough8, depth_hist, normal_hist, normal_hist_fmt, rough8_hist, radiance, radiance_hist, motion,
              variance_hist, sample_count_hist, cb, out_reprojected, out_average, avg_fmt, out_variance, out_sample_count, dxc=False, stats=None):
    """radiance / radiance_hist [H,W,4] float16 | float32 (alpha of radiance = ray length); motion [H,W,2] float16 | float32; variance_hist / sample_count_hist float16
    [H,W]; out_*: the images to write into (copies are returned; out_reprojected's dtype is its format, out_average uint32 [H8,W8] or float32 [H8,W8,4] per avg_fmt).
    stats receives per stored-or-not pixel of the listed tiles ON the frame: `glossy`, `hit`, `surface`, `discard`, `early_out`, `search`, `slow`, `uv_outside`."""
    w, h = int(cb.bufferDimensions[0]), int(cb.bufferDimensions[1])
    o_rep, o_avg, o_var, o_cnt = (np.array(a, copy=True) for a in (out_reprojected, out_average, out_variance, out_sample_count))
    X0, Y0 = listed_tiles(tile_list, count, w, h)
    if X0.size == 0:
        return o_rep, o_avg, o_var, o_cnt
    inv_proj, inv_view, prev_vp = matrix(cb.invProjection), matrix(cb.invView), matrix(cb.prevViewProjection)
    K = [kernel_weight(i) for i in range(-RADIUS, RADIUS + 1)]
    fw, fh = F(w), F(h)
    depth, depth_hist = np.asarray(depth, F), np.asarray(depth_hist, F)
    n01, hn01 = decode_normals01(normals, normal_fmt).astype(F), decode_normals01(normal_hist, normal_hist_fmt).astype(F)
    r_hist = np.asarray(rough8_hist).astype(F) / F(255.0)
    rad_full = np.asarray(radiance).astype(F)
    rad_hist = np.asarray(radiance_hist)[..., :3].astype(F)
    var_hist, cnt_hist = np.asarray(variance_hist).astype(F), np.asarray(sample_count_hist).astype(F)
    mv = np.asarray(motion).astype(F)
    with np.errstate(all="ignore"):
        a_rad = f16r(_apron(rad_full[..., :3], X0, Y0)[0])
        px, py = _centre(X0, Y0)
        shape = px.shape
        rough = _at(np.asarray(rough8), px, py) / F(255.0)
        glossy = rough < F(cb.roughnessThreshold)
        centre = _at(rad_full, px, py)
        rad = [centre[..., k] for k in range(3)]
        ray_length = centre[..., 3]
        # ---- FFX_DNSR_Reflections_EstimateLocalNeighborhoodInGroup
        mean, var2, acc = [np.zeros(shape, F) for _ in range(3)], [np.zeros(shape, F) for _ in range(3)], F(0.0)
        for j in range(-RADIUS, RADIUS + 1):
            for i in range(-RADIUS, RADIUS + 1):
                wt = K[i + RADIUS] * K[j + RADIUS]
                acc = acc + wt
                for k in range(3):
                    r = _nb(a_rad[..., k], i, j)
                    mean[k] = mean[k] + r * wt
                    var2[k] = var2[k] + (r * r) * wt
        mean = [mean[k] / acc for k in range(3)]
        var2 = [np.abs(var2[k] / acc - mean[k] * mean[k]) for k in range(3)]
        # ---- FFX_DNSR_Reflections_PickReprojection
        u, v = (px.astype(F) + F(0.5)) / fw, (py.astype(F) + F(0.5)) / fh
        normal = _norm3(_at(n01, px, py), dxc)
        m = _at(mv, px, py)
        s_u, s_v = u - m[..., 0] * F(0.5), v - m[..., 1] * F(-0.5)
        z = _at(depth, px, py)
        cy = F(1.0) - v
        p = _mul_m(inv_proj, F(2.0) * u - F(1.0), F(2.0) * cy - F(1.0), z, 1.0)
        vs = [p[k] / p[3] for k in range(3)]
        surface_depth = _length(tuple(vs), dxc)
        ray = surface_depth + ray_length
        vs = [(vs[k] / surface_depth) * ray for k in range(3)]
        wp = _mul_m(inv_view, vs[0], vs[1], vs[2], 1.0)[:3]
        q = _mul_m(prev_vp, wp[0], wp[1], wp[2], 1.0)
        h_u = F(0.5) * (q[0] / q[3]) + F(0.5)
        h_v = F(1.0) - (F(0.5) * (q[1] / q[3]) + F(0.5))
        s_n, h_n = _norm3(sample_bilinear(hn01, s_u, s_v), dxc), _norm3(sample_bilinear(hn01, h_u, h_v), dxc)
        s_hist, h_hist = sample_bilinear(rad_hist, s_u, s_v), sample_bilinear(rad_hist, h_u, h_v)
        nn = _norm3_again(normal, dxc)
        h_sim = _dot(_norm3_again(h_n, dxc), nn, dxc)
        s_sim = _dot(_norm3_again(s_n, dxc), nn, dxc)
        h_r, s_r = sample_bilinear(r_hist, h_u, h_v), sample_bilinear(r_hist, s_u, s_v)
        hit = (h_sim > F(0.9999)) & (h_sim + F(1.0e-3) > s_sim) & (np.abs(h_r - rough) < np.abs(s_r - rough) + F(1.0e-3))
        d2 = tuple(s_hist[..., k] - mean[k] for k in range(3))
        surface = ~hit & (_dot(d2, d2, dxc) < F(1.5) * _length(tuple(var2), dxc))
        discard = ~hit & ~surface
        r_u, r_v = np.where(hit, h_u, s_u).astype(F), np.where(hit, h_v, s_v).astype(F)
        hist_n = tuple(np.where(hit, h_n[k], s_n[k]).astype(F) for k in range(3))
        rep = [np.where(hit, h_hist[..., k], s_hist[..., k]).astype(F) for k in range(3)]
        hld = linear_depth_uv(inv_proj, r_u, r_v, sample_bilinear(depth_hist, r_u, r_v))
        ld = linear_depth_uv(inv_proj, u, v, z)
        df = disocclusion_factor(normal, hist_n, ld, hld, dxc).astype(F)
        picked = glossy & ~discard
        early = picked & (df > THRESHOLD)
        search = picked & (df < THRESHOLD)
        if search.any():                                                                         # the 3 x 3 search: reprojection_uv is updated INSIDE the loop
            s = search
            su, sv, sdf = r_u[s], r_v[s], df[s]
            nrm, sld = tuple(c[s] for c in normal), ld[s]
            du, dv = F(1.0) / fw, F(1.0) / fh
            for y in (-1, 0, 1):
                for x in (-1, 0, 1):
                    tu, tv = su + F(x) * du, sv + F(y) * dv
                    wgt = disocclusion_factor(nrm, _norm3(sample_bilinear(hn01, tu, tv), dxc), sld, linear_depth_uv(inv_proj, tu, tv, sample_bilinear(depth_hist, tu, tv)), dxc)
                    better = wgt > sdf
                    sdf, su, sv = np.where(better, wgt, sdf).astype(F), np.where(better, tu, su).astype(F), np.where(better, tv, sv).astype(F)
            r_u[s], r_v[s], df[s] = su, sv, sdf
            again = sample_bilinear(rad_hist, su, sv)
            for k in range(3):
                rep[k][s] = again[..., k]
        slow = search & (df < THRESHOLD)
        if slow.any():                                                                           # the 2 x 2 path
            s = slow
            su, sv = r_u[s], r_v[s]
            nrm, sld = tuple(c[s] for c in normal), ld[s]
            uvx, uvy = _frac(fw * su + F(0.5)), _frac(fh * sv + F(0.5))
            tx, ty = _ftoi(fw * su - F(0.5)), _ftoi(fh * sv - F(0.5))
            r_, n_, d_, w_ = [], [], [], []
            for ox, oy in ((0, 0), (1, 0), (0, 1), (1, 1)):
                r_.append(load_texel(rad_hist, tx + ox, ty + oy))
                n_.append(_norm3(load_texel(hn01, tx + ox, ty + oy), dxc))
                d_.append(linear_depth_uv(inv_proj, su, sv, load_texel(depth_hist, tx + ox, ty + oy)))
                w_.append(np.where(disocclusion_factor(nrm, n_[-1], sld, d_[-1], dxc) > HALF_THRESHOLD, F(1.0), F(0.0)).astype(F))
            w_ = [(w_[0] * (F(1.0) - uvx)) * (F(1.0) - uvy), (w_[1] * uvx) * (F(1.0) - uvy), (w_[2] * (F(1.0) - uvx)) * uvy, (w_[3] * uvx) * uvy]
            ws = _max2(((w_[0] + w_[1]) + w_[2]) + w_[3], np.full(su.shape, F(1.0e-3)))
            w_ = [c / ws for c in w_]
            mix = lambda a: ((a[0] * w_[0] + a[1] * w_[1]) + a[2] * w_[2]) + a[3] * w_[3]      # noqa: E731
            for k in range(3):
                rep[k][s] = mix([r_[i][..., k] for i in range(4)])
            df[s] = disocclusion_factor(nrm, tuple(mix([n_[i][k] for i in range(4)]) for k in range(3)), sld, mix(d_), dxc)     # the interpolated normal is not normalised
        late = search                                                                            # past the early-out: the last line of PickReprojection
        df = np.where(late & (df < THRESHOLD), F(0.0), df).astype(F)
        # ---- FFX_DNSR_Reflections_Reproject. The discard branch leaves reprojection_uv / reprojection unset with a factor of 0: inside [0,1]^2 the factor < 0.9
        # stores (0,0,0) / 1 / 1, outside the else branch stores the same — defined here as that outcome
        inside = (r_u > 0) & (r_v > 0) & (r_u < F(1.0)) & (r_v < F(1.0))
        prev_var = sample_bilinear(var_hist, r_u, r_v)
        ns = sample_bilinear(cnt_hist, r_u, r_v) * df
        smax = _max2(np.full(shape, F(8.0)), MAX_SAMPLES * (F(1.0) - exp_((-rough) * F(100.0))))
        ns = _min2(smax, ns + F(1.0)).astype(F)
        new_var = temporal_variance(tuple(rad), tuple(rep), dxc)
        keep = picked & inside & ~(df < THRESHOLD)
        var_mix = _lerp(new_var, prev_var, F(1.0) / ns)
        st_rep = [np.where(keep, rep[k], F(0.0)).astype(F) for k in range(3)]
        st_var = np.where(keep, var_mix, F(1.0)).astype(F)
        st_cnt = np.where(keep, ns, F(1.0)).astype(F)
        rad = [np.where(keep, _lerp(rad[k], rep[k], F(0.3)), rad[k]).astype(F) for k in range(3)]
        # ---- the 8 x 8 -> 1 average
        weight = _max2(exp_((-luminance(tuple(rad), dxc)) * F(0.3)), np.full(shape, F(1.0e-2)))
        rad = [rad[k] * weight for k in range(3)]
        bad = (px >= w) | (py >= h) | (weight > F(1.0e3))
        for k in range(3):
            bad |= ~np.isfinite(rad[k])
        rw = np.stack([np.where(bad, F(0.0), c).astype(F) for c in rad + [weight]], -1)
        total = downsample(rw)
        wacc = _max2(total[:, 3], np.full(total.shape[0], F(1.0e-3)))
        avg = np.stack([total[:, k] / wacc for k in range(3)], -1).astype(F)
    on = (px < w) & (py < h)
    m_st = on & glossy
    val = np.stack(st_rep + [np.zeros(shape, F)], -1)                                            # the shader stores a float3: alpha is written as 0
    with np.errstate(over="ignore", invalid="ignore"):
        o_rep[py[m_st], px[m_st]] = val[m_st].astype(o_rep.dtype)
        o_var[py[m_st], px[m_st]] = st_var[m_st].astype(np.float16)
        o_cnt[py[m_st], px[m_st]] = st_cnt[m_st].astype(np.float16)
    if avg_fmt == abi.FMT_R11G11B10_FLOAT:
        o_avg.view(np.uint32)[Y0 // 8, X0 // 8] = encode_r11g11b10(avg)
    else:
        o_avg[Y0 // 8, X0 // 8] = np.concatenate([avg, np.zeros((avg.shape[0], 1), F)], -1)
    if stats is not None:
        g = glossy
        stats.update(glossy=g[on], hit=(g & hit)[on], surface=(g & surface)[on], discard=(g & discard)[on], early_out=early[on], search=search[on], slow=slow[on],
                     uv_outside=(picked & ~inside)[on], kept=keep[on])
    return o_rep, o_avg, o_var, o_cnt


def _norm3_again(n, dxc):
    """normalize((float3)n) of an already normalised tuple, as written at the two similarity dots"""
    r = normalize32(np.stack(n, -1), dxc)
    return r[..., 0], r[..., 1], r[..., 2]
