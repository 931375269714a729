"""The contract of vqhip_msaa_resolve_surfaces and vqhip_depth_hierarchy (docs/DESIGN_DETAILS.md §7.10) in numpy: DepthResolve.hlsl:CSMain :36-100 per
pixel, and the min-depth pyramid of DownsampleDepth.hlsl + FidelityFX SPD — once as a closed form (`hierarchy`), once as a walk of SPD's own structure
(`hierarchy_spd_walk`: 64 x 64 tiles, values carried on in a tile for outputs 0-5, the last workgroup re-reading slot 6 for outputs 6-11, stores dropped
outside a level, surplus UAV slots bound to the last subresource). Nothing under oracle/ knows these passes: this file is the checker."""
import numpy as np

from tests.msaa_ref import owners
from vqengine_amd import abi

F = np.float32


# ---- DepthResolve.hlsl ----------------------------------------------------------------------------------------------------------------------
def resolve_depth(depth_ms):
    """depth_ms float32 [H,W,4] -> (minDepth [H,W], iSample int [H,W]): min(min(min(s0, s1), s2), s3); iSample starts at 0 and every later sample equal to
    the minimum replaces it (:59-62: on a tie the highest equal index wins). Finite inputs (np.minimum and fminf differ on NaN only)."""
    d = np.asarray(depth_ms, F)
    m = np.minimum(np.minimum(np.minimum(d[..., 0], d[..., 1]), d[..., 2]), d[..., 3])
    i = np.zeros(m.shape, np.int64)
    for s in (1, 2, 3):
        i = np.where(m == d[..., s], s, i)
    return m, i


def decode_normals01(plane, fmt):
    """.rgb of a normals plane as the shader loads it: UNORM10 c / 1023 correctly rounded (one binary32 division), or the float planes as they are"""
    if fmt == abi.FMT_RGBA32F:
        return np.asarray(plane, F)[..., :3]
    q = np.asarray(plane).view(np.uint32) if np.asarray(plane).dtype != np.uint32 else np.asarray(plane)
    c = np.stack([q & 1023, (q >> 10) & 1023, (q >> 20) & 1023], -1).astype(F)
    return c / F(1023.0)


def _fma32(a, b, c):
    """fma(a, b, c) in binary32, exactly: a * b is exact in binary64; its sum with c is formed by TwoSum and rounded TO ODD in binary64, after which the
    rounding to binary32 is the correct one (53 >= 24 + 2 bits)."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                                      # exact residual of s
    bits = s.view(np.int64)
    fix = (e != 0) & ((bits & 1) == 0) & np.isfinite(s)
    toward = np.where((e > 0) == (s > 0), 1, -1)                       # next binary64 in the residual's direction (s != 0 whenever e != 0)
    s = np.where(fix, (bits + toward).view(np.float64), s)
    return s.astype(F)


def normalize32(v, dxc):
    """normalize of float32 [..., 3] in the reading vqhip_set_arithmetic selects. literal: v / sqrt((x*x + y*y) + z*z), every operation rounded to binary32,
    one IEEE quotient per component. DXC: v * rsqrt(fma(z, z, fma(y, y, x*x))) with rsqrt(x) = (float)(1.0 / sqrt((double)x)). A zero vector gives NaN in both."""
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        if dxc:
            dd = _fma32(z, z, _fma32(y, y, x * x))
            r = (1.0 / np.sqrt(dd.astype(np.float64))).astype(F)
            return v * r[..., None]
        length = np.sqrt((x * x + y * y) + z * z)
        return v / length[..., None]


def unorm10(c):
    """float -> UNORM10 as vqhip_scene_normals_from_materials stores it: trunc(saturate(c) * 1023 + 0.5) in binary32; saturate(NaN) = 0"""
    c = np.asarray(c, F)
    with np.errstate(invalid="ignore"):
        s = np.where(np.isnan(c), F(0), np.clip(c, F(0), F(1))).astype(F)
    return (s * F(1023.0) + F(0.5)).astype(np.uint32)


def resolve_normals_samples(n01, dxc=False, out_fmt=abi.FMT_R10G10B10A2_UNORM, pairwise=False):
    """n01 float32 [..., 4 samples, 3] (the loaded rgb of each sample) -> the stored pixel: uint32 words (alpha bits 3) or float32 [..., 4] (alpha 1).
    pairwise=True is NOT the contract: the sum (N0 + N1) + (N2 + N3), for the test that shows the order is observable."""
    n = np.asarray(n01, F) * F(2.0) - F(1.0)
    if pairwise:
        s = (n[..., 0, :] + n[..., 1, :]) + (n[..., 2, :] + n[..., 3, :])
    else:
        s = ((n[..., 0, :] + n[..., 1, :]) + n[..., 2, :]) + n[..., 3, :]
    with np.errstate(invalid="ignore"):
        o = (normalize32(s * F(0.25), dxc) + F(1.0)) * F(0.5)
    if out_fmt == abi.FMT_RGBA32F:
        return np.concatenate([o, np.ones(o.shape[:-1] + (1,), F)], -1)
    q = unorm10(o)
    return (q[..., 0] | (q[..., 1] << 10) | (q[..., 2] << 20) | (np.uint32(3) << 30)).astype(np.uint32)


def resolve_normals(normals, coverage, fmt=abi.FMT_R10G10B10A2_UNORM, dxc=False, out_fmt=abi.FMT_R10G10B10A2_UNORM):
    """normals: one plane per layer (uint32 [H,W] words or float32 [H,W,4]); a sample no layer owns reads the target's clear value 0"""
    own = owners(coverage)
    samples = np.zeros(own.shape + (3,), F)
    for k, p in enumerate(normals):
        samples = np.where((own == k)[..., None], decode_normals01(p, fmt)[..., None, :], samples)
    return resolve_normals_samples(samples, dxc, out_fmt)


def resolve_roughness(depth_ms, coverage, gb1, background=None, scene_fmt=abi.FMT_RGBA16F):
    """The alpha the OUTPUT_ROUGHNESS permutation writes: the 4-sample colour target's alpha at sample iSample — gb1.w of the owner's record stored in the
    scene format, or the background's alpha (None: 0). Returned in the scene format's dtype."""
    dtype = np.float16 if scene_fmt == abi.FMT_RGBA16F else np.float32
    _, i = resolve_depth(depth_ms)
    own = np.take_along_axis(owners(coverage), i[..., None], -1)[..., 0]
    a = np.zeros(own.shape, dtype) if background is None else np.asarray(background)[..., 3].astype(dtype)
    for k, g in enumerate(gb1):
        a = np.where(own == k, np.asarray(g, F)[..., 3].astype(dtype), a)
    return a


# ---- DownsampleDepth.hlsl + SPD -------------------------------------------------------------------------------------------------------------
def level_count(w, h):
    return abi.mip_level_count(w, h)


def _reduce(p):
    """SpdReduce4 = min(min(v0, v1), min(v2, v3)) over the 2 x 2 blocks of p (even dims)"""
    return np.minimum(np.minimum(p[0::2, 0::2], p[0::2, 1::2]), np.minimum(p[1::2, 0::2], p[1::2, 1::2]))


def hierarchy(depth, true_top=False):
    """The closed form. depth float32 [h, w] -> list of levels: level 0 a copy; level l texel = min over the 2 x 2 parents, a coordinate outside the parent
    level reading 0.0; the 1 x 1 top level min(top, 0) whenever there are <= 12 levels (the reference's surplus reduction), or, true_top, the frame's minimum."""
    depth = np.asarray(depth, F)
    h, w = depth.shape
    L = level_count(w, h)
    lv = [depth.copy()]
    for l in range(1, L):
        pw, ph = max(1, w >> (l - 1)), max(1, h >> (l - 1))
        cw, ch = max(1, w >> l), max(1, h >> l)
        p = np.zeros((2 * ch, 2 * cw), F)
        p[:min(ph, 2 * ch), :min(pw, 2 * cw)] = lv[-1][:min(ph, 2 * ch), :min(pw, 2 * cw)]
        lv.append(_reduce(p))
    if true_top:
        lv[-1] = np.full_like(lv[-1], depth.min())
    elif L <= 12:
        lv[-1] = np.minimum(lv[-1], F(0))
    return lv


def hierarchy_spd_walk(depth):
    """The reference's dispatch restated step by step (default flags). Subresource l of the texture is max(1, w >> l) x max(1, h >> l); UAV slot i is bound to
    subresource min(i, L - 1) (RenderResources.cpp:110-111); a store outside the bound subresource is dropped, a load outside reads 0. Every 64 x 64 tile
    (one workgroup) copies its part of level 0, then performs SPD outputs 0 .. min(mips, 6) - 1 on values it CARRIES (never re-read from the texture), storing
    output i to slot i + 1; mips = the number of LEVELS (DownsampleDepth.hlsl:82-85,105). If mips > 6 the last workgroup loads a 64 x 64 region of slot 6 and
    carries on with outputs 6 .. min(mips, 12) - 1."""
    depth = np.asarray(depth, F)
    h, w = depth.shape
    L = level_count(w, h)
    sub = [np.zeros((max(1, h >> l), max(1, w >> l)), F) for l in range(L)]

    def store(slot, y0, x0, block):
        t = sub[min(slot, L - 1)]
        ys, xs = max(0, min(block.shape[0], t.shape[0] - y0)), max(0, min(block.shape[1], t.shape[1] - x0))
        if ys > 0 and xs > 0:
            t[y0:y0 + ys, x0:x0 + xs] = block[:ys, :xs]

    def load(src, y0, x0, n):
        block = np.zeros((n, n), F)
        part = src[y0:y0 + n, x0:x0 + n]
        block[:part.shape[0], :part.shape[1]] = part
        return block

    mips = L                                                            # what the shader hands SPD as its number of reductions
    for ty in range((h + 63) // 64):
        for tx in range((w + 63) // 64):
            tile = load(depth, ty * 64, tx * 64, 64)                    # SpdLoadSourceImage: the bound SRV, out of bounds 0
            store(0, ty * 64, tx * 64, tile)                            # the copy into slot 0 (CSMain :91-101; the bounds test there == the dropped store)
            for i in range(min(mips, 6)):
                tile = _reduce(tile)
                store(i + 1, ty * tile.shape[0], tx * tile.shape[1], tile)
    if mips > 6:
        tile = load(sub[min(6, L - 1)], 0, 0, 64)                       # SpdLoad: slot 6
        for i in range(6, min(mips, 12)):
            tile = _reduce(tile)
            store(i + 1, 0, 0, tile)
    return sub
