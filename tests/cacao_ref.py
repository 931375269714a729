"""The contract of vqhip_cacao (docs/DESIGN_DETAILS.md §7.14) in numpy binary32: FidelityFX CACAO at quality HIGH, native resolution, engine normals —
AMDFidelityFX/CACAO/ffx_cacao.hlsl as FFX_CACAO_D3D12Draw (ffx_cacao_impl.cpp:1922-2259) dispatches it: CSPrepareNativeDepthsAndMips (:1331-1430),
CSPrepareNativeNormalsFromInputNormals (:1619-1643), CSGenerateQ2 per pass (:803-1147), CSEdgeSensitiveBlur<p> per pass (:381-514) and CSApply (:1188-1242).
Every expression as written: one rounding per + - *, the IEEE quotient, correctly rounded sqrt, left to right; min16float is binary32; a subexpression of literals
alone is folded in binary64 and rounded once (1.0 - 0.6 is the binary32 nearest 0.4, 64.0 / 255.0 the one nearest that quotient); log2 / exp2 are the arithmetic
contract's polynomials (the CPU oracle's exports); binary16 only where the source packs (the R16F depth store, the blur's group-shared tile). Samplers are address
arithmetic (§3.4): a point sample reads texel floor(u * W), clamped or mirrored; GatherRed takes the bilinear footprint of 8-bit fixed-point coordinates; the
point mip filter selects floor(lod + 0.5) clamped to [0, 3]; a Load outside the resource returns 0 and a store outside is dropped.
Nothing under oracle/ knows these passes: this file is the checker."""
import numpy as np

from tests import oracle_lib as O
from tests.depth_ref import decode_normals01
from tests.ref_cases import to_unorm8
from tests.ssr_denoise_ref import f16r

F = np.float32
D = lambda x: F(np.float64(x))                                      # a literal: binary64 -> binary32, once
LIT_0_4 = D(1.0 - 0.6)                                               # (1.0 - SSAO_HALOING_REDUCTION_AMOUNT)
PACK_W = (D(64.0 / 255.0), D(16.0 / 255.0), D(4.0 / 255.0), D(1.0 / 255.0))
NUM_TAPS = 12                                                        # g_numTaps[2]
MIP_GLOBAL_OFFSET = D(-4.3)
# g_samplePatternMain[0 .. 12): (x, y, weight, log2(length))
SAMPLE_PATTERN = np.array([
    [0.78488064, 0.56661671, 1.500000, -0.126083], [0.26022232, -0.29575172, 1.500000, -1.064030], [0.10459357, 0.08372527, 1.110000, -2.730563],
    [-0.68286800, 0.04963045, 1.090000, -0.498827], [-0.13570161, -0.64190155, 1.250000, -0.532765], [-0.26193795, -0.08205118, 0.670000, -1.783245],
    [-0.61177456, 0.66664219, 0.710000, -0.044234], [0.43675563, 0.25119025, 0.610000, -1.167283], [0.07884444, 0.86618668, 0.640000, -0.459002],
    [-0.12790935, -0.29869005, 0.600000, -1.729424], [-0.04031125, 0.02413622, 0.600000, -4.792042], [0.16201244, -0.52851415, 0.790000, -1.067055]], np.float64).astype(F)
BLUR_TILE_W, BLUR_TILE_H = 64, 48                                    # TILE_WIDTH * BLUR_WIDTH, TILE_HEIGHT * BLUR_HEIGHT


class Consts:
    """the fields of one abi.CacaoConstants block as binary32 scalars / arrays"""

    def __init__(self, cb):
        for name, _ in cb._fields_:
            v = getattr(cb, name)
            if name == "PassIndex":
                setattr(self, name, int(v))
            elif name == "NormalsWorldToViewspaceMatrix":
                setattr(self, name, np.array([[v.m[i][j] for j in range(4)] for i in range(4)], F))
            elif hasattr(v, "__len__"):
                setattr(self, name, np.array([list(r) if hasattr(r, "__len__") else r for r in v], F if name != "DepthBufferOffset" else np.int32))
            else:
                setattr(self, name, F(v))


def half_dims(w, h):
    return (w + 1) // 2, (h + 1) // 2


def mip_dims(hw, hh, k):
    return max(1, hw >> k), max(1, hh >> k)


# ---- scalar rules ---------------------------------------------------------------------------------------------------------------------------
def sat(x):
    """saturate: NaN -> 0, -0 -> +0"""
    x = np.asarray(x, F)
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, np.where(x < 1, x, F(1)), F(0)).astype(F)


def max0(x):
    """max(0, x): a NaN operand is dropped, of two zeros +0"""
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, x, F(0)).astype(F)


def min_(a, b):
    """min: a NaN operand is dropped (operands here are never two zeros of different sign)"""
    return np.fmin(a, b).astype(F)


def to_snorm8(x):
    """A store to an R8G8B8A8_SNORM target (D3D11.3 §3.2.3.4 FLOAT -> SNORM): NaN -> 0, clamp to [-1, 1], scale by 127, add +0.5 (value >= 0) or -0.5, truncate"""
    x = np.asarray(x, F)
    with np.errstate(invalid="ignore"):
        c = np.where(np.isnan(x), F(0), np.where(x < -1, F(-1), np.where(x > 1, F(1), x))).astype(F)
        s = c * F(127.0)
        return (s + np.where(s >= 0, F(0.5), F(-0.5))).astype(F).astype(np.int32).astype(np.int8)


def from_snorm8(v):
    """SNORM8 -> float: v / 127 correctly rounded, -128 reads -1"""
    v = np.maximum(np.asarray(v, np.int8).astype(F), F(-127.0))
    return v / F(127.0)


def from_unorm8(v):
    return np.asarray(v, np.uint8).astype(F) / F(255.0)


def _trunc_u(x):
    """(uint) of a float in [0, 2^31): truncation, NaN -> 0"""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), F(0), np.clip(x, F(0), F(2147483520.0))).astype(np.int64)


def _floor_i(x):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), F(0), np.clip(np.floor(x), F(-2147483520.0), F(2147483520.0))).astype(np.int64)


def fixed8(x):
    """(texel, fraction) of a filter coordinate in 8-bit fixed point (§3.4): floor(x * 256 + 0.5), split"""
    fx = _floor_i(x * F(256.0) + F(0.5))
    return fx >> 8, (fx & 255).astype(F) * F(0.00390625)


def mirror(i, n):
    """MIRROR addressing of a texel index: texel -1 reads 0, texel n reads n - 1, period 2n"""
    t = np.mod(i, 2 * n)
    return np.where(t < n, t, 2 * n - 1 - t)


def log2_(x):
    x = np.asarray(x, F)
    return O.math_array(0, x).reshape(x.shape)


def exp2_(x):
    x = np.asarray(x, F)
    return O.math_array(1, x).reshape(x.shape)


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def dot4(a, b):
    return ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]


def pack_edges(e):
    """PackEdges (:163-171): e = 4 arrays LRTB -> the float the R8G8_UNORM store receives"""
    r = [np.rint(sat(c) * D(3.05)).astype(F) for c in e]
    return dot4(r, PACK_W)


def unpack_edges(packed, inv_sharpness):
    """UnpackEdges (:173-183) / UnpackEdgesFloat16_4 (:351-361): the packed float (a UNORM8 value / 255) -> LRTB weights"""
    p = _trunc_u(np.asarray(packed, F) * D(255.5))
    return [sat(((p >> s) & 3).astype(F) / F(3.0) + inv_sharpness) for s in (6, 4, 2, 0)]


# ---- stage 1: CSPrepareNativeDepthsAndMips -----------------------------------------------------------------------------------------------------
def mip_smart_average(d, c):
    """MipSmartAverage (:1313-1320) of float4(d[0..3]); `-1.0f / EffectRadius * EffectRadius` left to right"""
    closest = min_(min_(d[0], d[1]), min_(d[2], d[3]))
    falloff = (F(-1.0) / c.EffectRadius) * c.EffectRadius
    w = []
    for k in range(4):
        dist = d[k] - closest
        w.append(sat(dist * dist * falloff + F(1.0)))
    with np.errstate(invalid="ignore", divide="ignore"):
        return (dot4(w, d) / (((w[0] + w[1]) + w[2]) + w[3])).astype(F)


def prepare_depths(depth, c):
    """depth float32 [H,W] -> [mip0, mip1, mip2, mip3], each float16 [4 slices, rows, cols] (R16F). Every thread of every 8 x 8 group runs: threads outside the
    hw x hh buffer read clamped depths and take part in the averages; their stores are dropped. The mip-3 writer is the thread with bufferCoord == (0, 0)."""
    depth = np.asarray(depth, F)
    h, w = depth.shape
    hw, hh = half_dims(w, h)
    tx, ty = (hw + 7) // 8 * 8, (hh + 7) // 8 * 8
    px = (F(2.0) * np.arange(tx, dtype=F) + F(0.5)) * c.DepthBufferInverseDimensions[0]           # uv = (float2(depthBufferCoord) + 0.5f) * inverse dimensions
    py = (F(2.0) * np.arange(ty, dtype=F) + F(0.5)) * c.DepthBufferInverseDimensions[1]
    ix, _ = fixed8(px * F(w) - F(0.5))                                                              # GatherRed: the bilinear footprint
    iy, _ = fixed8(py * F(h) - F(0.5))
    x0, x1, y0, y1 = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1), np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
    mul, add = c.DepthUnpackConsts
    with np.errstate(divide="ignore", invalid="ignore"):
        # slices 0..3 = samples .w .z .x .y = texels (0,0) (1,0) (0,1) (1,1) of the footprint
        v = np.stack([mul / (add - depth[np.ix_(ys, xs)]) for ys, xs in ((y0, x0), (y0, x1), (y1, x0), (y1, x1))]).astype(F)
        levels = [v]
        for _ in range(3):
            p = levels[-1]
            levels.append(mip_smart_average([p[:, 0::2, 0::2], p[:, 1::2, 0::2], p[:, 0::2, 1::2], p[:, 1::2, 1::2]], c))
    out = []
    for k, p in enumerate(levels):
        mw, mh = mip_dims(hw, hh, k)
        out.append(p[:, :mh, :mw].astype(np.float16))
    return out


# ---- stage 2: CSPrepareNativeNormalsFromInputNormals ---------------------------------------------------------------------------------------------
def prepare_normals(normals, fmt, c):
    """normals: uint32 [H,W] R10G10B10A2_UNORM words or float32 [H,W,4] -> int8 [4, hh, hw, 4] (R8G8B8A8_SNORM, .w = 1). The shader's matrix is the cbuffer's
    column-major view of the block's row-major floats: mul(n, (float3x3)M)[j] = (n.x * m[j][0] + n.y * m[j][1]) + n.z * m[j][2], m the floats as stored."""
    n01 = decode_normals01(normals, fmt)
    h, w = n01.shape[:2]
    hw, hh = half_dims(w, h)
    out = np.zeros((4, hh, hw, 4), np.int8)
    m = c.NormalsWorldToViewspaceMatrix
    for s, (dx, dy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        u = (F(2.0) * np.arange(hw, dtype=F) + F(dx) + F(0.5)) * c.InputOutputBufferInverseDimensions[0]
        v = (F(2.0) * np.arange(hh, dtype=F) + F(dy) + F(0.5)) * c.InputOutputBufferInverseDimensions[1]
        xs, ys = np.clip(_floor_i(u * F(w)), 0, w - 1), np.clip(_floor_i(v * F(h)), 0, h - 1)
        e = n01[np.ix_(ys, xs)]
        n = [e[..., k] * c.NormalsUnpackMul + c.NormalsUnpackAdd for k in range(3)]
        for j in range(3):
            out[s, ..., j] = to_snorm8((n[0] * m[j, 0] + n[1] * m[j, 1]) + n[2] * m[j, 2])
        out[s, ..., 3] = 127
    return out


# ---- stage 3: CSGenerateQ2 -------------------------------------------------------------------------------------------------------------------
def _obscurance(n, d, falloff, c):
    """CalculatePixelObscurance (:623-631)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        length_sq = dot3(d, d)
        n_dot_d = dot3(n, d) / np.sqrt(length_sq)
        falloff_mult = max0(length_sq * falloff + F(1.0))
        return max0(n_dot_d - c.EffectHorizonAngleThreshold) * falloff_mult


def generate_pixels(depths, normals, c, xs, ys):
    """GenerateSSAOShadowsInternal(qualityLevel 2, adaptiveBase false) for the pixels (xs, ys) of pass c.PassIndex -> (occlusion, packed edges) as floats, the mip
    each of the 24 taps selected [n, 12] and the four edge weights"""
    p = c.PassIndex
    d0 = depths[0][p].astype(F)
    hh, hw = d0.shape
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    sx, sy = xs.astype(F), ys.astype(F)
    inv_d, inv_s = c.DeinterleavedDepthBufferInverseDimensions, c.SSAOBufferInverseDimensions
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        uvx = (sx + F(0.5)) * inv_d[0] + c.DeinterleavedDepthBufferNormalisedOffset[0]
        uvy = (sy + F(0.5)) * inv_d[1] + c.DeinterleavedDepthBufferNormalisedOffset[1]
        gx, _ = fixed8(uvx * F(hw) - F(0.5))                                      # the footprint of GatherRed(uv); offset (-1, -1) moves it
        gy, _ = fixed8(uvy * F(hh) - F(0.5))
        at = lambda ax, ay: d0[mirror(ay, hh), mirror(ax, hw)]
        pix_z, pix_l, pix_t = at(gx, gy), at(gx - 1, gy), at(gx, gy - 1)          # valuesUL .y .x .z
        pix_r, pix_b = at(gx + 1, gy), at(gx, gy + 1)                             # valuesBR .z .x
        nspx, nspy = (sx + F(0.5)) * inv_s[0], (sy + F(0.5)) * inv_s[1]
        pc = [(c.NDCToViewMul[0] * nspx + c.NDCToViewAdd[0]) * pix_z, (c.NDCToViewMul[1] * nspy + c.NDCToViewAdd[1]) * pix_z, pix_z]
        nrm = from_snorm8(normals[p][ys, xs, :3])
        n = [nrm[:, 0], nrm[:, 1], nrm[:, 2]]
        dir_rb = [pc[2] * c.NDCToViewMul[0] * inv_s[0], pc[2] * c.NDCToViewMul[1] * inv_s[1]]
        # CalculateRadiusParameters (:588-605)
        too_close = sat(np.sqrt(dot3(pc, pc)) * c.EffectSamplingRadiusNearLimitRec) * D(0.8) + D(0.2)
        radius = c.EffectRadius * too_close
        lookup = (D(0.85) * radius) / dir_rb[0]
        falloff = F(-1.0) / (radius * radius)
        rs = c.PatternRotScaleMatrices[_trunc_u(sy * F(2.0) + sx) % 5]
        rot = [rs[:, k] * lookup for k in range(4)]
        pc = [v * c.DepthPrecisionOffsetMod for v in pc]
        # CalculateEdges (:213-219)
        e = [pix_l - pix_z, pix_r - pix_z, pix_t - pix_z, pix_b - pix_z]
        adj = [e[0] + e[1], e[1] + e[0], e[2] + e[3], e[3] + e[2]]
        e = [min_(np.abs(a), np.abs(b)) for a, b in zip(e, adj)]
        edges = [sat(D(1.3) - a / (pix_z * D(0.040))) for a in e]
        # detail AO (:877-905)
        vdz = [pc[0] / pc[2], pc[1] / pc[2], np.ones_like(pc[2])]
        zero = np.zeros_like(pc[2])
        deltas = []
        for z, base in ((pix_l, [-dir_rb[0], zero, zero]), (pix_r, [dir_rb[0], zero, zero]), (pix_t, [zero, -dir_rb[1], zero]), (pix_b, [zero, dir_rb[1], zero])):
            dz = z - pc[2]
            deltas.append([base[k] + vdz[k] * dz for k in range(3)])
        mod_falloff = F(4.0) * falloff
        add_obs = [_obscurance(n, d, mod_falloff, c) for d in deltas]
        obs_sum = (F(0.0) + c.DetailAOStrength * dot4(add_obs, edges)).astype(F)
        weight_sum = np.zeros_like(obs_sum)
        # normal-based edges (:908-935): a Load outside the slice returns 0
        np_ = normals[p]
        for k, (dx, dy) in enumerate(((-1, 0), (1, 0), (0, -1), (0, 1))):
            ax, ay = xs + dx, ys + dy
            ok = (ax >= 0) & (ax < hw) & (ay >= 0) & (ay < hh)
            nb = np.where(ok[:, None], from_snorm8(np_[np.clip(ay, 0, hh - 1), np.clip(ax, 0, hw - 1), :3]), F(0))
            edges[k] = edges[k] * sat(dot3(n, [nb[:, 0], nb[:, 1], nb[:, 2]]) + D(0.5))
        mip_offset = log2_(lookup) + MIP_GLOBAL_OFFSET
        mips = np.zeros((len(xs), NUM_TAPS), np.int64)
        for i in range(NUM_TAPS):
            s = SAMPLE_PATTERN[i]
            ox = np.rint(rot[0] * s[0] + rot[1] * s[1]).astype(F)
            oy = np.rint(rot[2] * s[0] + rot[3] * s[1]).astype(F)
            lod = s[3] + mip_offset
            level = np.clip(_floor_i(lod + F(0.5)), 0, 3)                           # NaN -> 0
            mips[:, i] = level
            weight_mod = F(1.0) * s[2]
            for sign in (F(1.0), F(-1.0)):
                tx, ty = (sign * ox) * inv_d[0] + uvx, (sign * oy) * inv_d[1] + uvy
                z = np.zeros_like(pix_z)
                for k in range(4):
                    mw, mh = mip_dims(hw, hh, k)
                    sel = level == k
                    if sel.any():
                        z[sel] = depths[k][p][np.clip(_floor_i(ty[sel] * F(mh)), 0, mh - 1), np.clip(_floor_i(tx[sel] * F(mw)), 0, mw - 1)].astype(F)
                hit = [(c.DepthBufferUVToViewMul[0] * tx + c.DepthBufferUVToViewAdd[0]) * z, (c.DepthBufferUVToViewMul[1] * ty + c.DepthBufferUVToViewAdd[1]) * z, z]
                delta = [hit[k] - pc[k] for k in range(3)]
                obs = _obscurance(n, delta, falloff, c)
                reduct = sat(max0(-delta[2]) * c.NegRecEffectRadius + F(2.0))
                weight = (D(0.6) * reduct + LIT_0_4) * weight_mod
                obs_sum = obs_sum + obs * weight
                weight_sum = weight_sum + weight
        obscurance = obs_sum / weight_sum
        fade = sat(pc[2] * c.EffectFadeOutMul + c.EffectFadeOutAdd)
        edge_fade = sat((F(1.0) - edges[0] - edges[1]) * D(0.35)) + sat((F(1.0) - edges[2] - edges[3]) * D(0.35))
        fade = fade * sat(F(1.0) - edge_fade)
        obscurance = min_(c.EffectShadowStrength * obscurance, c.EffectShadowClamp) * fade
        occlusion = exp2_(c.EffectShadowPow * log2_(sat(F(1.0) - obscurance)))
    return occlusion.astype(F), pack_edges(edges).astype(F), mips, edges


def generate(depths, normals, per_pass, pixels=None):
    """The four CSGenerateQ2 dispatches -> (ping uint8 [4, hh, hw, 2] (R8G8_UNORM), stats). pixels: None = all, or per pass a pair (xs, ys) — only those texels of
    ping are written (the rest 0). stats: `mip_histogram` int64 [4] over the 12 mip selections of every evaluated pixel (each serves two taps), `edge_share` = the share
    of evaluated pixels with any edge weight below 1, `packed_edge_share` = the share whose stored edge byte is not 255."""
    hh, hw = depths[0].shape[1:]
    ping = np.zeros((4, hh, hw, 2), np.uint8)
    hist, n_edge, n_packed, n_px = np.zeros(4, np.int64), 0, 0, 0
    for p in range(4):
        c = per_pass[p] if isinstance(per_pass[p], Consts) else Consts(per_pass[p])
        if pixels is None:
            ys, xs = (a.ravel() for a in np.mgrid[0:hh, 0:hw])
        else:
            xs, ys = (np.asarray(a, np.int64) for a in pixels[p])
        occ, packed, mips, edges = generate_pixels(depths, normals, c, xs, ys)
        ping[p, ys, xs, 0], ping[p, ys, xs, 1] = to_unorm8(occ), to_unorm8(packed)
        hist += np.bincount(mips.ravel(), minlength=4)
        n_edge += int((np.minimum(np.minimum(edges[0], edges[1]), np.minimum(edges[2], edges[3])) < 1).sum())
        n_packed += int((ping[p, ys, xs, 1] != 255).sum())
        n_px += len(xs)
    return ping, {"mip_histogram": hist, "edge_share": n_edge / max(n_px, 1), "packed_edge_share": n_packed / max(n_px, 1), "pixels": n_px}


# ---- stage 4: CSEdgeSensitiveBlur<p> ------------------------------------------------------------------------------------------------------------
def blur(ping, per_pass, passes):
    """LDSEdgeSensitiveBlur(passes) on every slice, each with its own pass's constants (per_pass: four blocks): ping uint8 [4, hh, hw, 2] -> pong. Groups of 16 x 16 threads load a 64 x 48 tile (point MIRROR) whose origin is
    gid * (64 - 2p, 48 - 2p) - p, keep the occlusion as binary16, run p iterations of the 5-point edge-weighted average (every result rounded to binary16 again)
    and write the inner (64 - 2p) x (48 - 2p) texels with their unchanged edge bytes. Group-shared texels outside the tile are never written by the source; they
    only reach texels that are not stored, and read 0 here."""
    if passes == 0:
        raise ValueError("blurPassCount 0 skips the stage: apply reads ping")
    ping = np.asarray(ping, np.uint8)
    return np.concatenate([_blur_slice(ping[s:s + 1], per_pass[s] if isinstance(per_pass[s], Consts) else Consts(per_pass[s]), passes) for s in range(4)])


def _blur_slice(ping, c, passes):
    _, hh, hw, _ = ping.shape
    sw, sh = BLUR_TILE_W - 2 * passes, BLUR_TILE_H - 2 * passes
    gx, gy = (hw + sw - 1) // sw, (hh + sh - 1) // sh
    u = ((np.arange(gx)[:, None] * sw - passes + np.arange(BLUR_TILE_W)[None, :]).astype(F) + F(0.5)) * c.SSAOBufferInverseDimensions[0]      # [gx, 64]
    v = ((np.arange(gy)[:, None] * sh - passes + np.arange(BLUR_TILE_H)[None, :]).astype(F) + F(0.5)) * c.SSAOBufferInverseDimensions[1]      # [gy, 48]
    cx, cy = mirror(_floor_i(u * F(hw)), hw), mirror(_floor_i(v * F(hh)), hh)
    tile = ping[:, cy[:, None, :, None], cx[None, :, None, :], :]                                  # [4, gy, gx, 48, 64, 2]
    val = f16r(from_unorm8(tile[..., 0]))
    el, er, et, eb = unpack_edges(from_unorm8(tile[..., 1]), c.InvSharpness)
    for _ in range(passes):
        pad = np.zeros(val.shape[:3] + (BLUR_TILE_H + 2, BLUR_TILE_W + 2), F)
        pad[..., 1:-1, 1:-1] = val
        left, right, top, bottom = pad[..., 1:-1, :-2], pad[..., 1:-1, 2:], pad[..., :-2, 1:-1], pad[..., 2:, 1:-1]
        s = val * F(0.5)
        wsum = np.full_like(val, F(0.5))
        for nb, e in ((left, el), (right, er), (top, et), (bottom, eb)):
            s = s + nb * e
            wsum = wsum + e
        val = f16r(s / wsum)
    pong = np.zeros_like(ping)
    ox = np.arange(gx)[:, None] * sw + np.arange(sw)[None, :]                                      # image x of the stored texels [gx, sw]
    oy = np.arange(gy)[:, None] * sh + np.arange(sh)[None, :]
    inner_v = to_unorm8(val[..., passes:BLUR_TILE_H - passes, passes:BLUR_TILE_W - passes])
    inner_e = to_unorm8(from_unorm8(tile[..., passes:BLUR_TILE_H - passes, passes:BLUR_TILE_W - passes, 1]))
    for j in range(gy):
        ys = oy[j][oy[j] < hh]
        for i in range(gx):
            xs = ox[i][ox[i] < hw]
            pong[:, ys[:, None], xs[None, :], 0] = inner_v[:, j, i, :len(ys), :len(xs)]
            pong[:, ys[:, None], xs[None, :], 1] = inner_e[:, j, i, :len(ys), :len(xs)]
    return pong


# ---- stage 5: CSApply ---------------------------------------------------------------------------------------------------------------------------
def _fma_exact64(a, b, c):
    """fma(a, b, c) in binary32 for the blend below: a is a multiple of 2^-16 in [0, 1], b a UNORM8 value / 255 (or 0), c in [0, 1] — the product has at most 41
    significant bits at 2^-47 or above and its sum with c fits binary64 exactly, so one rounding to binary32 remains (tests/test_cacao_cpu.py compares with _fma32)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def _bilinear_clamp(plane, u, v):
    """SampleLevel(g_LinearClampSampler, uv, 0).x of one slice's occlusion bytes [hh, hw]: §3.4 — 8-bit fractions, the blend4 FMA chain"""
    hh, hw = plane.shape
    ix, wx = fixed8(u * F(hw) - F(0.5))
    iy, wy = fixed8(v * F(hh) - F(0.5))
    x0, x1, y0, y1 = np.clip(ix, 0, hw - 1), np.clip(ix + 1, 0, hw - 1), np.clip(iy, 0, hh - 1), np.clip(iy + 1, 0, hh - 1)
    w00, w10, w01, w11 = (F(1) - wx) * (F(1) - wy), wx * (F(1) - wy), (F(1) - wx) * wy, wx * wy
    c00, c10, c01, c11 = (from_unorm8(plane[a, b]) for a, b in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
    return _fma_exact64(w11, c11, _fma_exact64(w01, c01, _fma_exact64(w10, c10, w00 * c00)))


def apply(final, c, width, height):
    """CSApply over width x height: final uint8 [4, hh, hw, 2] (pong, or ping when the blur is skipped) -> the AO plane uint8 [H,W] (R8_UNORM). Evaluated per
    pixel parity (mx, my): the four slice indices are constants of a parity class."""
    final = np.asarray(final, np.uint8)
    out = np.zeros((height, width), np.uint8)
    inv = c.SSAOBufferInverseDimensions
    for my in (0, 1):
        for mx in (0, 1):
            y, x = np.mgrid[my:height:2, mx:width:2]
            if y.size == 0:
                continue
            ic, ih, iv, idg = mx + my * 2, (1 - mx) + my * 2, mx + (1 - my) * 2, (1 - mx) + (1 - my) * 2
            centre = final[ic, y // 2, x // 2]
            ao = from_unorm8(centre[..., 0])
            e = unpack_edges(from_unorm8(centre[..., 1]), c.InvSharpness)
            fx, fy, fmx, fmy = x.astype(F), y.astype(F), F(mx), F(my)
            fmxe, fmye = e[1] - e[0], e[3] - e[2]

            def sample(index, offx, offy):
                return _bilinear_clamp(final[index, ..., 0], (fx + offx) * F(0.5) * inv[0], (fy + offy) * F(0.5) * inv[1])
            ao_h = sample(ih, fmx + fmxe - F(0.5), F(0.5) - fmy)
            ao_v = sample(iv, F(0.5) - fmx, fmy - F(0.5) + fmye)
            ao_d = sample(idg, fmx - F(0.5) + fmxe, fmy - F(0.5) + fmye)
            bw = [np.ones_like(ao), (e[0] + e[1]) * F(0.5), (e[2] + e[3]) * F(0.5)]
            bw.append((bw[1] + bw[2]) * F(0.5))
            total = ((bw[0] + bw[1]) + bw[2]) + bw[3]
            out[my::2, mx::2] = to_unorm8(dot4([ao, ao_h, ao_v, ao_d], bw) / total)
    return out


# ---- the whole call -----------------------------------------------------------------------------------------------------------------------------
def frame(depth, normals, fmt, shared, per_pass, blur_passes=2):
    """vqhip_cacao in full -> dict: depths (4 float16 arrays), normals, ping, pong (None when blur_passes == 0), ao, stats"""
    cs = Consts(shared)
    cp = [Consts(per_pass[i]) for i in range(4)]
    h, w = np.asarray(depth).shape
    depths = prepare_depths(depth, cs)
    nrm = prepare_normals(normals, fmt, cs)
    ping, stats = generate(depths, nrm, cp)
    pong = blur(ping, cp, blur_passes) if blur_passes else None
    ao = apply(pong if blur_passes else ping, cs, w, h)
    return {"depths": depths, "normals": nrm, "ping": ping, "pong": pong, "ao": ao, "stats": stats}
