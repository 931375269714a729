"""The contract of vqhip_ssr_prefilter and vqhip_ssr_resolve_temporal (docs/DESIGN_DETAILS.md §7.12) in numpy binary32: Prefilter.hlsl and ResolveTemporal.hlsl
with ffx_denoiser_reflections_prefilter.h / _resolve_temporal.h / _common.h for every 8 x 8 tile of the denoiser tile list — every expression as written, one
rounding per operation, left to right, in either arithmetic reading. Values pass through binary16 exactly where the reference packs them into group-shared
memory; min16float is binary32; exp(x) = exp2(x * 1.44269502f). exp2 / log2 come from the CPU oracle's exports (the arithmetic contract's polynomials); numpy's own
binary32 add / mul / div / sqrt are the IEEE operations. Nothing under oracle/ knows these passes: this file is the checker."""
import numpy as np

from tests import oracle_lib as O
from tests.depth_ref import _fma32, decode_normals01, normalize32
from tests.ssr_trace_ref import _max2, matrix
from vqengine_amd import abi

F = np.float32
LOG2E = np.array([0x3FB8AA3B], np.uint32).view(F)[0]              # the binary32 nearest log2(e): exp(x) = exp2(x * LOG2E)
# First 15 numbers of Halton(2,3) stretched to [-3, 3], in the order the shader lists them
OFFSETS = ((0, 1), (-2, 1), (2, -3), (-3, 0), (1, 2), (-1, -2), (3, 0), (-3, 3), (0, -3), (-1, -1), (2, 1), (-2, -2), (1, 0), (0, 2), (3, -1))
RADIUS = 4                                                       # FFX_DNSR_REFLECTIONS_LOCAL_NEIGHBORHOOD_RADIUS


def round_up8(v):
    """FFX_DNSR_Reflections_RoundUp8 AS WRITTEN: a value that is not a multiple of 8 becomes value + 8"""
    v = int(v)
    return v if (v & ~7) == v else v + 8


def f16r(x):
    """f32tof16 then f16tof32: round to nearest even, overflow to inf"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, F).astype(np.float16).astype(F)


def exp_(x):
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        return O.math_array(1, (x * LOG2E).astype(F)).reshape(x.shape)


def pow512(x):
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        return O.math_array(1, (F(512.0) * O.math_array(0, x)).astype(F)).reshape(x.shape)


def kernel_weight(i):
    """FFX_DNSR_Reflections_LocalNeighborhoodKernelWeight: exp(-3.0 * (i * i) / (radius * radius)), radius = 4 + 1"""
    fi = F(i)
    radius = F(RADIUS) + F(1.0)
    return exp_(np.array([(F(-3.0) * (fi * fi)) / (radius * radius)], F))[0]


def decode_r11g11b10(words):
    """DXGI R11G11B10_FLOAT: uint32 [...] -> float32 [..., 3], exact. R bits 0-10, G 11-21, B 22-31; 5-bit exponent (bias 15), 6 / 6 / 5 mantissa bits, unsigned"""
    w = np.asarray(words).view(np.uint32) if np.asarray(words).dtype != np.uint32 else np.asarray(words)
    out = []
    for shift, mbits in ((0, 6), (11, 6), (22, 5)):
        f = (w >> np.uint32(shift)) & np.uint32((1 << (5 + mbits)) - 1)
        e, m = (f >> np.uint32(mbits)).astype(np.uint32), (f & np.uint32((1 << mbits) - 1)).astype(np.uint32)
        normal = (((e + np.uint32(112)) << np.uint32(23)) | (m << np.uint32(23 - mbits))).astype(np.uint32).view(F)
        special = (np.uint32(0x7F800000) | (m << np.uint32(23 - mbits))).astype(np.uint32).view(F)
        denorm = np.ldexp(m.astype(F), -14 - mbits).astype(F)
        out.append(np.where(e == 0, denorm, np.where(e == 31, special, normal)).astype(F))
    return np.stack(out, -1)


def average_rgb(avg, fmt):
    return decode_r11g11b10(avg) if fmt == abi.FMT_R11G11B10_FLOAT else np.asarray(avg, F)[..., :3]


def _dot(a, b, dxc):
    if dxc:
        return _fma32(a[2], b[2], _fma32(a[1], b[1], a[0] * b[0]))
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _length(v, dxc):
    return np.sqrt(_dot(v, v, dxc))


def _lerp(a, b, t):
    return a + t * (b - a)


def _floor_i(x):
    x = np.where(np.isnan(x), F(0), np.floor(x)).astype(np.float64)
    return np.clip(x, -2147483648.0, 2147483647.0).astype(np.int64)


def sample_average(rgb, u, v):
    """SampleLevel(g_linear_sampler, uv, 0) on the 1/8-resolution texture [H8,W8,3]: bilinear, CLAMP, §3.4 (8-bit fractions, the blend4 FMA chain)"""
    h8, w8 = rgb.shape[:2]
    fx, fy = _floor_i((u * F(w8) - F(0.5)) * F(256.0) + F(0.5)), _floor_i((v * F(h8) - F(0.5)) * F(256.0) + F(0.5))
    ix, iy = fx >> 8, fy >> 8
    wx, wy = (fx & 255).astype(F) * F(0.00390625), (fy & 255).astype(F) * F(0.00390625)
    x0, x1, y0, y1 = np.clip(ix, 0, w8 - 1), np.clip(ix + 1, 0, w8 - 1), np.clip(iy, 0, h8 - 1), np.clip(iy + 1, 0, h8 - 1)
    w00, w10, w01, w11 = (F(1) - wx) * (F(1) - wy), wx * (F(1) - wy), (F(1) - wx) * wy, wx * wy
    c00, c10, c01, c11 = rgb[y0, x0], rgb[y0, x1], rgb[y1, x0], rgb[y1, x1]
    return tuple(_fma32(w11, c11[..., k], _fma32(w01, c01[..., k], _fma32(w10, c10[..., k], w00 * c00[..., k]))) for k in range(3))


def listed_tiles(tile_list, count, w, h):
    """first pixels (x0, y0) of the tiles the passes work on: count clamped to the tile grid, an entry beyond the grid skipped, duplicates once"""
    tx, ty = (w + 7) // 8, (h + 7) // 8
    e = np.asarray(tile_list).view(np.uint32)[:min(int(count), tx * ty)].astype(np.int64)
    x, y = (e & 0xFFFF) >> 3, (e >> 16) >> 3
    ok = (x < tx) & (y < ty)
    flat = np.unique(y[ok] * tx + x[ok])
    return (flat % tx) * 8, (flat // tx) * 8


def _apron(plane, X0, Y0):
    """[H,W,...] -> [T,16,16,...]: the 16 x 16 region around each tile, a load outside the frame reads 0"""
    h, w = plane.shape[:2]
    xs, ys = X0[:, None] - 4 + np.arange(16)[None, :], Y0[:, None] - 4 + np.arange(16)[None, :]
    ok = ((ys >= 0) & (ys < h))[:, :, None] & ((xs >= 0) & (xs < w))[:, None, :]
    g = plane[np.clip(ys, 0, h - 1)[:, :, None], np.clip(xs, 0, w - 1)[:, None, :]]
    return np.where(ok.reshape(ok.shape + (1,) * (g.ndim - 3)), g, np.zeros((), g.dtype)), xs, ys


def _centre(X0, Y0):
    return X0[:, None, None] + np.arange(8)[None, None, :] + np.zeros((1, 8, 1), np.int64), Y0[:, None, None] + np.arange(8)[None, :, None] + np.zeros((1, 1, 8), np.int64)


def _at(plane, px, py, dtype=F):
    """Texture.Load at the tile's own pixels [T,8,8]: outside the frame 0"""
    h, w = plane.shape[:2]
    ok = (px < w) & (py < h)
    g = plane[np.minimum(py, h - 1), np.minimum(px, w - 1)]
    return np.where(ok.reshape(ok.shape + (1,) * (g.ndim - 3)), g, np.zeros((), g.dtype)).astype(dtype)


def _nb(a, dx, dy):
    return a[:, 4 + dy:12 + dy, 4 + dx:12 + dx]


def _store(out_rad, out_var, px, py, rgb, var):
    h, w = out_var.shape
    m = (px < w) & (py < h)                                                  # a store outside the target is dropped
    val = np.stack([rgb[0], rgb[1], rgb[2], rgb[2]], -1)                     # radiance.xyzz
    with np.errstate(over="ignore", invalid="ignore"):
        out_rad[py[m], px[m]] = val[m].astype(out_rad.dtype)
        out_var[py[m], px[m]] = var[m].astype(np.float16)


def _uv8(px, py, w, h):
    return (px.astype(F) + F(0.5)) / F(round_up8(w)), (py.astype(F) + F(0.5)) / F(round_up8(h))


def linear_depth(inv_proj, qx, qy, z, w, h):
    """FFX_DNSR_Reflections_GetLinearDepth with uv = (q + 0.5) / float2(screen): |z / w| of InvProjectPosition"""
    u, v = (qx.astype(F) + F(0.5)) / F(w), (qy.astype(F) + F(0.5)) / F(h)
    cy = F(1.0) - v
    cx_, cy_ = F(2.0) * u - F(1.0), F(2.0) * cy - F(1.0)
    M = inv_proj
    pz = ((cx_ * M[0, 2] + cy_ * M[1, 2]) + z * M[2, 2]) + F(1.0) * M[3, 2]
    pw = ((cx_ * M[0, 3] + cy_ * M[1, 3]) + z * M[2, 3]) + F(1.0) * M[3, 3]
    return np.abs(pz / pw)


def _radiance_weight(avg, rad, var, dxc):
    """FFX_DNSR_Reflections_GetRadianceWeight(center = avg, neighbour = rad, variance)"""
    ln = _length(tuple(avg[k] - rad[k] for k in range(3)), dxc)
    return _max2(exp_(-(F(0.6) + var * F(0.1)) * ln), np.full(ln.shape, F(1.0e-2)))


def prefilter(tile_list, count, depth, normals, normal_fmt, rough8, avg, avg_fmt, radiance, variance, cb, out_radiance, out_variance, dxc=False, stats=None, offsets=OFFSETS):
    """radiance [H,W,4] float16 | float32; variance float16 [H,W]; avg: uint32 [H8,W8] (R11G11B10_FLOAT) | float32 [H8,W8,4]. out_radiance / out_variance: the
    images to write into (copies are returned; out_radiance's dtype is the output format). stats receives `denoise` (bool per stored pixel). offsets: NOT the contract when changed —
    for the test that shows the taps and their order are observable."""
    w, h = int(cb.bufferDimensions[0]), int(cb.bufferDimensions[1])
    out_r, out_v = np.array(out_radiance, copy=True), np.array(out_variance, copy=True)
    X0, Y0 = listed_tiles(tile_list, count, w, h)
    if X0.size == 0:
        return out_r, out_v
    inv_proj = matrix(cb.invProjection)
    with np.errstate(all="ignore"):
        a_rad, xs, ys = _apron(np.asarray(radiance)[..., :3].astype(F), X0, Y0)
        a_rad = f16r(a_rad)
        a_var = f16r(_apron(np.asarray(variance).astype(F), X0, Y0)[0])
        n01 = _apron(decode_normals01(normals, normal_fmt).astype(F), X0, Y0)[0]
        a_n = f16r(normalize32(F(2.0) * n01 - F(1.0), dxc))
        qx, qy = xs[:, None, :] + np.zeros_like(ys)[:, :, None], ys[:, :, None] + np.zeros_like(xs)[:, None, :]
        a_d = linear_depth(inv_proj, qx, qy, _apron(np.asarray(depth, F), X0, Y0)[0], w, h).astype(F)
        px, py = _centre(X0, Y0)
        rough = _at(np.asarray(rough8), px, py) / F(255.0)
        c_rad = tuple(_nb(a_rad[..., k], 0, 0) for k in range(3))
        c_var, c_d = _nb(a_var, 0, 0), _nb(a_d, 0, 0)
        c_n = tuple(_nb(a_n[..., k], 0, 0) for k in range(3))
        needs = (c_var > 0) & (rough < F(cb.roughnessThreshold)) & ~(rough < F(0.04))
        u8, v8 = _uv8(px, py, w, h)
        av = sample_average(average_rgb(avg, avg_fmt), u8, v8)
        aw = _radiance_weight(av, c_rad, c_var, dxc)
        ar = [c_rad[k] * aw for k in range(3)]
        avar = (c_var * aw) * aw
        vw = _max2(np.full(c_var.shape, F(0.1)), F(1.0) - exp_(-(c_var * F(4.4))))
        for dx, dy in offsets:
            n_rad = tuple(_nb(a_rad[..., k], dx, dy) for k in range(3))
            n_n = tuple(_nb(a_n[..., k], dx, dy) for k in range(3))
            wn = pow512(_max2(_dot(c_n, n_n, dxc), np.zeros(c_var.shape, F)))
            wd = exp_((-np.abs(c_d - _nb(a_d, dx, dy)) * c_d) * F(4.0))
            wr = _radiance_weight(av, n_rad, c_var, dxc)
            wt = (((F(1.0) * wn) * wd) * wr) * vw
            aw = aw + wt
            ar = [ar[k] + wt * n_rad[k] for k in range(3)]
            avar = avar + (wt * wt) * _nb(a_var, dx, dy)
        ar = [ar[k] / aw for k in range(3)]
        avar = avar / (aw * aw)
        rgb = tuple(np.where(needs, ar[k], c_rad[k]).astype(F) for k in range(3))
        var = np.where(needs, avar, c_var).astype(F)
    _store(out_r, out_v, px, py, rgb, var)
    if stats is not None:
        stats.update(denoise=needs[(px < w) & (py < h)])
    return out_r, out_v


def clip_aabb(lo, hi, prev):
    """FFX_DNSR_Reflections_ClipAABB on tuples of arrays: (clipped, was outside)"""
    centre = tuple(F(0.5) * (hi[k] + lo[k]) for k in range(3))
    extent = tuple(F(0.5) * (hi[k] - lo[k]) + F(0.001) for k in range(3))
    vec = tuple(prev[k] - centre[k] for k in range(3))
    unit = tuple(np.abs(vec[k] / extent[k]) for k in range(3))
    mx = _max2(_max2(unit[0], unit[1]), unit[2])
    outside = mx > F(1.0)
    return tuple(np.where(outside, centre[k] + vec[k] / mx, prev[k]).astype(F) for k in range(3)), outside


def luminance(c, dxc):
    d = _dot(c, (F(0.299), F(0.587), F(0.114)), dxc)
    return _max2(d, np.full(np.shape(d), F(0.001)))


def temporal_variance(history, rad, dxc):
    hl, l = luminance(history, dxc), luminance(rad, dxc)
    diff = np.abs(hl - l) / _max2(_max2(hl, l), np.full(np.shape(hl), F(0.5)))
    return diff * diff


def resolve_temporal(tile_list, count, rough8, avg, avg_fmt, radiance, reprojected, variance, sample_count, cb, out_radiance, out_variance, dxc=False, stats=None):
    """radiance (the prefiltered one) / reprojected [H,W,4] float16 | float32; variance / sample_count float16 [H,W]. stats receives per stored pixel `glossy`,
    `old_clipped`, `new_clipped`, `guard`."""
    w, h = int(cb.bufferDimensions[0]), int(cb.bufferDimensions[1])
    out_r, out_v = np.array(out_radiance, copy=True), np.array(out_variance, copy=True)
    X0, Y0 = listed_tiles(tile_list, count, w, h)
    if X0.size == 0:
        return out_r, out_v
    K = [kernel_weight(i) for i in range(-RADIUS, RADIUS + 1)]
    with np.errstate(all="ignore"):
        a_rad = f16r(_apron(np.asarray(radiance)[..., :3].astype(F), X0, Y0)[0])
        px, py = _centre(X0, Y0)
        new = tuple(_nb(a_rad[..., k], 0, 0) for k in range(3))
        rough = _at(np.asarray(rough8), px, py) / F(255.0)
        new_var = _at(np.asarray(variance), px, py)
        glossy = rough < F(cb.roughnessThreshold)
        ns = _at(np.asarray(sample_count), px, py)
        u8, v8 = _uv8(px, py, w, h)
        av = sample_average(average_rgb(avg, avg_fmt), u8, v8)
        old = tuple(_at(np.asarray(reprojected)[..., k], px, py) for k in range(3))
        mean, var2, acc = [np.zeros(px.shape, F) for _ in range(3)], [np.zeros(px.shape, F) for _ in range(3)], F(0.0)
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
        ln = _length(tuple(mean[k] - av[k] for k in range(3)), dxc)
        std = tuple(((np.sqrt(var2[k]) + ln) * F(cb.temporalStabilityFactor)) * F(1.4) for k in range(3))
        mean = [_lerp(mean[k], av[k], F(0.2)) for k in range(3)]
        old_c, old_out = clip_aabb(tuple(mean[k] - std[k] for k in range(3)), tuple(mean[k] + std[k] for k in range(3)), old)
        one = np.full(px.shape, F(1.0))
        speed = F(1.0) / _max2(ns, one)
        weight = F(1.0) - speed
        sig = tuple(_lerp(new[k], av[k], F(1.0) / _max2(ns + F(1.0), one)) for k in range(3))
        sig, new_out = clip_aabb(tuple(av[k] - std[k] * F(1.0) for k in range(3)), tuple(av[k] + std[k] * F(1.0) for k in range(3)), sig)
        sig = tuple(_lerp(sig[k], old_c[k], weight) for k in range(3))
        nv = _lerp(temporal_variance(sig, old_c, dxc), new_var, weight)
        bad = ~np.isfinite(nv)
        for k in range(3):
            bad |= ~np.isfinite(sig[k])
        sig = tuple(np.where(bad, F(0), sig[k]).astype(F) for k in range(3))
        nv = np.where(bad, F(0), nv).astype(F)
        rgb = tuple(np.where(glossy, sig[k], new[k]).astype(F) for k in range(3))
        var = np.where(glossy, nv, new_var).astype(F)
    _store(out_r, out_v, px, py, rgb, var)
    if stats is not None:
        m = (px < w) & (py < h)
        stats.update(glossy=glossy[m], old_clipped=(old_out & glossy)[m], new_clipped=(new_out & glossy)[m], guard=(bad & glossy)[m])
    return out_r, out_v
