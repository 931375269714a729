"""CPU-side checks of vqhip_adaptive_cacao (docs/DESIGN_DETAILS.md §7.15), no GPU: the numpy statement (tests/cacao_adaptive_ref.py) against a per-thread scalar
transcription of the five adaptive stages written straight from ffx_cacao.hlsl — its own sample pattern, point / gather / bilinear fetches and store rules —, the
coverage the test frames give (exact numbers, as §7.13 pins its scene), the hand-made cases of §7.15's readings, and the boundary: header, binding, library, work
layout, refusal without a context, the C++ adaptor against tests/cpp/mock_engine/."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import cacao_adaptive_ref as A
from tests import cacao_ref as R
from tests import oracle_lib as O
from tests.depth_ref import _fma32
from tests.ref_cases import to_unorm8
from vqengine_amd import abi, cacao, capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
R10, F32 = abi.FMT_R10G10B10A2_UNORM, abi.FMT_RGBA32F
SIZES = ((37, 23), (64, 48), (125, 93))
NEW_SYMBOLS = {"vqhip_adaptive_cacao", "vqhip_adaptive_cacao_work_bytes", "vqhip_adaptive_cacao_plane_offset_bytes"}


def scaled_radius(w):
    """tests/test_gpu_cacao.py's radius for the noise frame: the sampling discs of 1280 x 720 at the default 1.2, so that every depth mip is selected"""
    return 1.2 * 640.0 / ((w + 1) // 2)


@functools.lru_cache(maxsize=None)
def case(kind, w, h, limit=0.45):
    f = synth.cacao_room(w, h) if kind == "room" else synth.cacao_noise(w, h)
    over = {"adaptiveQualityLimit": limit}
    if kind == "noise":
        over["radius"] = scaled_radius(w)
    sh, pp = cacao.constants(w, h, f["proj"], f["normals_to_view"], cacao.settings(**over))
    return f, sh, pp, A.frame(f["depth"], f["packed"], R10, sh, pp, 0)


# ---- the scalar transcription: one thread at a time, every operation rounded to binary32 by numpy's float32 scalars -------------------------------
PATTERN = [tuple(F(v) for v in row) for row in (
    (0.78488064, 0.56661671, 1.500000, -0.126083), (0.26022232, -0.29575172, 1.500000, -1.064030), (0.10459357, 0.08372527, 1.110000, -2.730563),
    (-0.68286800, 0.04963045, 1.090000, -0.498827), (-0.13570161, -0.64190155, 1.250000, -0.532765), (-0.26193795, -0.08205118, 0.670000, -1.783245),
    (-0.61177456, 0.66664219, 0.710000, -0.044234), (0.43675563, 0.25119025, 0.610000, -1.167283), (0.07884444, 0.86618668, 0.640000, -0.459002),
    (-0.12790935, -0.29869005, 0.600000, -1.729424), (-0.04031125, 0.02413622, 0.600000, -4.792042), (0.16201244, -0.52851415, 0.790000, -1.067055),
    (-0.70991218, 0.47301072, 0.640000, -0.335236), (0.03277707, -0.22349690, 0.600000, -1.982384), (0.68921727, 0.36800742, 0.630000, -0.266718),
    (0.29251814, 0.37775412, 0.610000, -1.422520), (-0.12224089, 0.96582592, 0.600000, -0.426142), (0.11071457, -0.16131058, 0.600000, -2.165947),
    (0.46562141, -0.59747696, 0.600000, -0.189760), (-0.51548797, 0.11804193, 0.600000, -1.246800), (0.89141309, -0.42090443, 0.600000, 0.028192),
    (-0.32402530, -0.01591529, 0.600000, -1.543018), (0.60771245, 0.41635221, 0.600000, -0.605411), (0.02379565, -0.08239821, 0.600000, -3.809046),
    (0.48951152, -0.23657045, 0.600000, -1.189011), (-0.17611565, -0.81696892, 0.600000, -0.513724), (-0.33930185, -0.20732205, 0.600000, -1.698047),
    (-0.91974425, 0.05403209, 0.600000, 0.062246), (-0.15064627, -0.14949332, 0.600000, -1.896062), (0.53180975, -0.35210401, 0.600000, -0.758838),
    (0.41487166, 0.81442589, 0.600000, -0.505648), (-0.24106961, -0.32721516, 0.600000, -1.665244))]
ZERO, HALF, ONE, TWO = F(0.0), F(0.5), F(1.0), F(2.0)
L_0_8, L_0_2, L_0_85, L_0_6, L_0_4, L_1_3, L_0_04, L_0_35, L_M4_3 = (F(np.float64(v)) for v in (0.8, 0.2, 0.85, 0.6, 1.0 - 0.6, 1.3, 0.040, 0.35, -4.3))
L_3_05, L_20, L_5_32, L_255 = F(np.float64(3.05)), F(np.float64(5 * 4.0)), F(np.float64(5 / 32.0)), F(255.0)
PACK_W = [F(np.float64(v) / 255.0) for v in (64.0, 16.0, 4.0, 1.0)]


def _log2(x):
    return O.math_array(0, np.array([x], F))[0]


def _exp2(x):
    return O.math_array(1, np.array([x], F))[0]


def _pow(x, y):
    return _exp2(y * _log2(x))


def _sat(x):
    return ZERO if not x > 0 else (x if x < 1 else ONE)


def _max0(x):
    return x if x > 0 else ZERO


def _fix8(x):
    v = int(np.floor(x * F(256.0) + HALF))
    return v >> 8, F(v & 255) * F(0.00390625)


def _unorm8(x):
    return int(_sat(F(x)) * L_255 + HALF)


def _clamp(i, n):
    return min(max(i, 0), n - 1)


def _mirror(i, n):
    t = i % (2 * n)
    return t if t < n else 2 * n - 1 - t


def _floor_texel(u, n):
    return 0 if np.isnan(u) else _clamp(int(np.floor(min(max(u * F(n), F(-1e9)), F(1e9)))), n)


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _bilinear(plane, u, v):
    """g_LinearClampSampler on an R8_UNORM plane: 8-bit fractions, the products summed as the FMA chain of §3.4"""
    rows, cols = plane.shape
    ix, wx = _fix8(u * F(cols) - HALF)
    iy, wy = _fix8(v * F(rows) - HALF)
    tex = lambda y, x: F(plane[_clamp(y, rows), _clamp(x, cols)]) / L_255
    r = ((ONE - wx) * (ONE - wy)) * tex(iy, ix)
    for wt, cv in ((wx * (ONE - wy), tex(iy, ix + 1)), ((ONE - wx) * wy, tex(iy + 1, ix)), (wx * wy, tex(iy + 1, ix + 1))):
        r = _fma32(np.array([wt], F), np.array([cv], F), np.array([r], F))[0]
    return r


class _Thread:
    """What GenerateSSAOShadowsInternal computes before its taps for SVPos = (x, y) of pass c.PassIndex"""

    def __init__(self, depths, normals, c, x, y):
        self.c, self.depths, self.p = c, depths, c.PassIndex
        p = self.p
        hh, hw = depths[0].shape[1:]
        self.hw, self.hh = hw, hh
        inv_d, inv_s = c.DeinterleavedDepthBufferInverseDimensions, c.SSAOBufferInverseDimensions
        sx, sy = F(x), F(y)
        self.uv = ((sx + HALF) * inv_d[0] + c.DeinterleavedDepthBufferNormalisedOffset[0], (sy + HALF) * inv_d[1] + c.DeinterleavedDepthBufferNormalisedOffset[1])
        gx, _ = _fix8(self.uv[0] * F(hw) - HALF)
        gy, _ = _fix8(self.uv[1] * F(hh) - HALF)
        at = lambda ax, ay: F(depths[0][p, _mirror(ay, hh), _mirror(ax, hw)])
        # GatherRed with offset (-1, -1): .x = (g - 1, g), .y = (g, g), .z = (g, g - 1); without: .x = (g, g + 1), .z = (g + 1, g)
        self.pix_l, self.pix_z, self.pix_t, self.pix_b, self.pix_r = at(gx - 1, gy), at(gx, gy), at(gx, gy - 1), at(gx, gy + 1), at(gx + 1, gy)
        self.nsp = ((sx + HALF) * inv_s[0], (sy + HALF) * inv_s[1])
        pc = [(c.NDCToViewMul[0] * self.nsp[0] + c.NDCToViewAdd[0]) * self.pix_z, (c.NDCToViewMul[1] * self.nsp[1] + c.NDCToViewAdd[1]) * self.pix_z, self.pix_z]
        self.n = self.normal(normals, x, y)
        self.dir_rb = (pc[2] * c.NDCToViewMul[0] * inv_s[0], pc[2] * c.NDCToViewMul[1] * inv_s[1])
        too_close = _sat(np.sqrt(_dot3(pc, pc)) * c.EffectSamplingRadiusNearLimitRec) * L_0_8 + L_0_2
        radius = c.EffectRadius * too_close
        self.lookup = (L_0_85 * radius) / self.dir_rb[0]
        self.falloff = F(-1.0) / (radius * radius)
        rs = c.PatternRotScaleMatrices[int(sy * TWO + sx) % 5]
        self.rot = [rs[k] * self.lookup for k in range(4)]
        self.pc = [v * c.DepthPrecisionOffsetMod for v in pc]
        self.mip_offset = _log2(self.lookup) + L_M4_3

    def normal(self, normals, x, y):
        if not (0 <= x < self.hw and 0 <= y < self.hh):
            return [ZERO] * 3                                                          # a Load outside the resource
        return [F(max(int(normals[self.p, y, x, k]), -127)) / F(127.0) for k in range(3)]

    def obscurance(self, d, falloff):
        length_sq = _dot3(d, d)
        n_dot_d = _dot3(self.n, d) / np.sqrt(length_sq)
        return _max0(n_dot_d - self.c.EffectHorizonAngleThreshold) * _max0(length_sq * falloff + ONE)

    def rounded_offset(self, i):
        s = PATTERN[i]
        return F(np.rint(self.rot[0] * s[0] + self.rot[1] * s[1])), F(np.rint(self.rot[2] * s[0] + self.rot[3] * s[1]))

    def tap_depth(self, i, u, v):
        lod = PATTERN[i][3] + self.mip_offset
        level = 0 if np.isnan(lod) else int(min(max(np.floor(lod + HALF), 0), 3))
        mw, mh = max(1, self.hw >> level), max(1, self.hh >> level)
        return F(self.depths[level][self.p, _floor_texel(v, mh), _floor_texel(u, mw)])

    def hit(self, u, v, z):
        """-> (obscurance, the haloing-reduction weight) of one hit"""
        c = self.c
        pos = [(c.DepthBufferUVToViewMul[0] * u + c.DepthBufferUVToViewAdd[0]) * z, (c.DepthBufferUVToViewMul[1] * v + c.DepthBufferUVToViewAdd[1]) * z, z]
        delta = [pos[k] - self.pc[k] for k in range(3)]
        reduct = _sat(_max0(-delta[2]) * c.NegRecEffectRadius + TWO)
        return self.obscurance(delta, self.falloff), L_0_6 * reduct + L_0_4


def scalar_base(depths, normals, c):
    """CSGenerateQ3Base: SSAOTap x 5, no edges, no detail AO -> [hh, hw, 2] bytes"""
    hh, hw = depths[0].shape[1:]
    out = np.zeros((hh, hw, 2), np.uint8)
    inv_d = c.DeinterleavedDepthBufferInverseDimensions
    for y in range(hh):
        for x in range(hw):
            t = _Thread(depths, normals, c, x, y)
            obs_sum, weight_sum = ZERO, ZERO
            for i in range(5):
                off = t.rounded_offset(i)
                weight_mod = ONE * PATTERN[i][2]
                for sign in (ONE, -ONE):
                    u, v = (sign * off[0]) * inv_d[0] + t.uv[0], (sign * off[1]) * inv_d[1] + t.uv[1]
                    obs, weight = t.hit(u, v, t.tap_depth(i, u, v))
                    weight = weight * weight_mod
                    obs_sum, weight_sum = obs_sum + obs * weight, weight_sum + weight
            out[y, x] = (_unorm8(obs_sum / weight_sum), _unorm8(weight_sum / L_20))
    return out


def scalar_importance_generate(base, c):
    _, hh, hw, _ = base.shape
    iw, ih = (hw + 1) // 2, (hh + 1) // 2
    out = np.zeros((ih, iw), np.uint8)
    for ty in range(ih):
        for tx in range(iw):
            u, v = (F(2 * tx) + HALF) * c.SSAOBufferInverseDimensions[0], (F(2 * ty) + HALF) * c.SSAOBufferInverseDimensions[1]
            ix, _ = _fix8(u * F(hw) - HALF)
            iy, _ = _fix8(v * F(hh) - HALF)
            min_v, max_v = ONE, ZERO
            for i in range(4):
                for dy, dx in ((1, 0), (1, 1), (0, 1), (0, 0)):                        # GatherRed .x .y .z .w
                    val = F(base[i, _clamp(iy + dy, hh), _clamp(ix + dx, hw), 0]) / L_255
                    val = _pow(_sat(ONE - c.EffectShadowStrength * val), c.EffectShadowPow)
                    max_v, min_v = max(max_v, val), min(min_v, val)
            out[ty, tx] = _unorm8(_pow(_sat((max_v - min_v) * TWO), L_0_8))
    return out


def _scalar_postprocess(src, c, tx, ty, second):
    inv = c.ImportanceMapInverseDimensions
    u, v = (F(tx) + HALF) * inv[0], (F(ty) + HALF) * inv[1]
    centre = _bilinear(src, u, v)
    hx, hy = HALF * inv[0], HALF * inv[1]
    three = F(3.0)
    if not second:
        vals = [_bilinear(src, u + -hx * three, v + -hy), _bilinear(src, u + hx, v + -hy * three), _bilinear(src, u + hx * three, v + hy), _bilinear(src, u + -hx, v + hy * three)]
    else:
        vals = [_bilinear(src, u + -hx, v + -hy * three), _bilinear(src, u + hx * three, v + -hy), _bilinear(src, u + hx, v + hy * three), _bilinear(src, u + -hx * three, v + hy)]
    q = F(0.25)
    avg_val = ((vals[0] * q + vals[1] * q) + vals[2] * q) + vals[3] * q
    max_val = max(centre, max(max(vals[0], vals[2]), max(vals[1], vals[3])))
    return max_val + ONE * (avg_val - max_val)


def scalar_importance_a(importance, c):
    ih, iw = importance.shape
    return np.array([[_unorm8(_scalar_postprocess(importance, c, tx, ty, False)) for tx in range(iw)] for ty in range(ih)], np.uint8)


def scalar_importance_b(pong, c):
    """every thread of the ceil(iw / 8) x ceil(ih / 8) groups runs: the store of a thread outside the map is dropped, its InterlockedAdd is not"""
    ih, iw = pong.shape
    out, counter = np.zeros((ih, iw), np.uint8), 0
    for ty in range((ih + 7) // 8 * 8):
        for tx in range((iw + 7) // 8 * 8):
            val = _scalar_postprocess(pong, c, tx, ty, True)
            if tx < iw and ty < ih:
                out[ty, tx] = _unorm8(val)
            if tx % 3 + ty % 3 == 0:
                counter = (counter + int(_sat(val) * L_255 + HALF)) & 0xFFFFFFFF
    return out, counter


def scalar_adaptive(depths, normals, c, importance_map, base, counter):
    """CSGenerateQ3: the front end of the HIGH pass, the adaptive branch with its pipelined tap loop, the back end -> ([hh, hw, 2] bytes, tap counts [hh, hw])"""
    hh, hw = depths[0].shape[1:]
    out, taps = np.zeros((hh, hw, 2), np.uint8), np.zeros((hh, hw), np.int64)
    inv_d = c.DeinterleavedDepthBufferInverseDimensions
    avg_importance = F(np.uint32(counter)) * c.LoadCounterAvgDiv
    for y in range(hh):
        for x in range(hw):
            t = _Thread(depths, normals, c, x, y)
            z = t.pix_z
            e = [t.pix_l - z, t.pix_r - z, t.pix_t - z, t.pix_b - z]
            adj = [e[0] + e[1], e[1] + e[0], e[2] + e[3], e[3] + e[2]]
            edges = [_sat(L_1_3 - min(abs(a), abs(b)) / (z * L_0_04)) for a, b in zip(e, adj)]
            pc = t.pc
            vdz = [pc[0] / pc[2], pc[1] / pc[2], ONE]
            add_obs = []
            for nz, b in ((t.pix_l, [-t.dir_rb[0], ZERO, ZERO]), (t.pix_r, [t.dir_rb[0], ZERO, ZERO]), (t.pix_t, [ZERO, -t.dir_rb[1], ZERO]), (t.pix_b, [ZERO, t.dir_rb[1], ZERO])):
                dz = nz - pc[2]
                add_obs.append(t.obscurance([b[k] + vdz[k] * dz for k in range(3)], F(4.0) * t.falloff))
            obs_sum = ZERO + c.DetailAOStrength * (((add_obs[0] * edges[0] + add_obs[1] * edges[1]) + add_obs[2] * edges[2]) + add_obs[3] * edges[3])
            weight_sum = ZERO
            for k, (dx, dy) in enumerate(((-1, 0), (1, 0), (0, -1), (0, 1))):
                edges[k] = edges[k] * _sat(_dot3(t.n, t.normal(normals, x + dx, y + dy)) + HALF)
            importance = _bilinear(importance_map, t.nsp[0] + c.PerPassFullResUVOffset[0], t.nsp[1] + c.PerPassFullResUVOffset[1])
            obs_sum = obs_sum * (L_5_32 + importance * F(27.0) / F(32.0))
            weight_sum = weight_sum + (F(base[c.PassIndex, y, x, 1]) / L_255) * L_20
            obs_sum = obs_sum + (F(base[c.PassIndex, y, x, 0]) / L_255) * weight_sum
            importance = importance * _sat(c.AdaptiveSampleCountLimit / avg_importance)
            count = F(27.0) * importance
            count = count + F(1.5)
            to = min(32, (0 if np.isnan(count) else int(count)) + 5)

            def get_hits(i):
                off = t.rounded_offset(i)
                off = (off[0] * inv_d[0], off[1] * inv_d[1])
                hits = []
                for u, v in ((t.uv[0] + off[0], t.uv[1] + off[1]), (t.uv[0] - off[0], t.uv[1] - off[1])):
                    hits.append((u, v, t.tap_depth(i, u, v)))
                return hits

            def add_hits(hits, obs_sum, weight_sum):
                for u, v, hz in hits:
                    obs, weight = t.hit(u, v, hz)                                       # the weight is overwritten per hit: weightMod does not enter
                    obs_sum, weight_sum = obs_sum + obs * weight, weight_sum + weight
                return obs_sum, weight_sum
            hits = get_hits(5)
            i = 5
            while i < to - 1:
                next_hits = get_hits(i + 1)
                obs_sum, weight_sum = add_hits(hits, obs_sum, weight_sum)
                hits = next_hits
                i += 1
            obs_sum, weight_sum = add_hits(hits, obs_sum, weight_sum)
            obsc = obs_sum / weight_sum
            fade = _sat(pc[2] * c.EffectFadeOutMul + c.EffectFadeOutAdd)
            edge_fade = _sat((ONE - edges[0] - edges[1]) * L_0_35) + _sat((ONE - edges[2] - edges[3]) * L_0_35)
            fade = fade * _sat(ONE - edge_fade)
            obsc = c.EffectShadowStrength * obsc
            obsc = (c.EffectShadowClamp if (np.isnan(obsc) or c.EffectShadowClamp < obsc) else obsc) * fade
            occlusion = _pow(_sat(ONE - obsc), c.EffectShadowPow)
            r = [F(np.rint(_sat(v) * L_3_05)) for v in edges]
            packed = ((r[0] * PACK_W[0] + r[1] * PACK_W[1]) + r[2] * PACK_W[2]) + r[3] * PACK_W[3]
            out[y, x] = (_unorm8(occlusion), _unorm8(packed))
            taps[y, x] = to
    return out, taps


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ("room", "noise"))
def test_statement_equals_the_scalar_transcription(kind, size):
    """Every adaptive stage, every plane and the counter. The prepare passes, the blur and the apply pass are tests/cacao_ref.py's, transcribed in
    tests/test_cacao_cpu.py."""
    w, h = size
    f, sh, pp, ref = case(kind, w, h)
    cs, cp = R.Consts(sh), [R.Consts(pp[i]) for i in range(4)]
    with np.errstate(all="ignore"):
        base = np.stack([scalar_base(ref["depths"], ref["normals"], cp[p]) for p in range(4)])
        assert np.array_equal(base, ref["base"]), ("base", np.argwhere(base != ref["base"])[:4])
        generated = scalar_importance_generate(base, cs)
        assert np.array_equal(generated, ref["importance_generated"]), "CSGenerateImportanceMap"
        pong = scalar_importance_a(generated, cs)
        assert np.array_equal(pong, ref["importance_pong"]), "CSPostprocessImportanceMapA"
        importance, counter = scalar_importance_b(pong, cs)
        assert np.array_equal(importance, ref["importance"]), "CSPostprocessImportanceMapB"
        assert counter == ref["counter"], "the load counter"
        for p in range(4):
            ping, taps = scalar_adaptive(ref["depths"], ref["normals"], cp[p], importance, base, counter)
            assert np.array_equal(ping, ref["ping"][p]), (p, np.argwhere(ping != ref["ping"][p])[:4])
            assert np.array_equal(taps, ref["stats"]["taps"][p]), p
    assert np.array_equal(ref["ao"], R.apply(ref["ping"], cs, w, h)) and ref["pong"] is None


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------------
def test_coverage_of_the_test_set():
    """What the frames of tests/test_gpu_cacao_adaptive.py exercise, from the statement alone: the three sizes x two scenes at the default limit 0.45, and 125 x 93
    at adaptiveQualityLimit 0 and 1. The exact numbers pin the scenes and the statement."""
    hist = np.zeros(33, np.int64)
    limiters, divergent = [], 0
    configs = [(k, w, h, 0.45) for (w, h) in SIZES for k in ("room", "noise")] + [(k, 125, 93, lim) for k in ("room", "noise") for lim in (0.0, 1.0)]
    for kind, w, h, limit in configs:
        st = case(kind, w, h, limit)[3]["stats"]
        hist += st["tap_histogram"]
        limiters.append(st["limiter"])
        tmin = np.array([st["taps"][p, y:y + 8, x:x + 8].min() for p in range(4) for y in range(0, (h + 1) // 2, 8) for x in range(0, (w + 1) // 2, 8)])
        divergent += int((st["wave_max"] != tmin).sum())
    assert hist[:6].sum() == 0 and hist[6] >= 32 and hist[32] >= 32 and int((hist[7:32] > 0).sum()) >= 8
    assert 1.0 in limiters and any(0.0 < v < 1.0 for v in limiters) and 0.0 in limiters
    assert divergent >= 1
    assert hist.tolist() == COVERAGE_HISTOGRAM and divergent == COVERAGE_DIVERGENT_WAVES
    assert [case(k, w, h)[3]["counter"] for (w, h) in SIZES for k in ("room", "noise")] == COVERAGE_COUNTERS


COVERAGE_HISTOGRAM = [0, 0, 0, 0, 0, 0, 29383, 7667, 2784, 1851, 2117, 2379, 1605, 4308, 1094, 760, 557, 637, 12046, 0, 0, 0, 0, 0, 0, 0, 0, 0, 9, 36, 48, 145, 11606]
COVERAGE_DIVERGENT_WAVES = 421
COVERAGE_COUNTERS = [1132, 4563, 1342, 9174, 2146, 22412]


# ---- hand-made cases ---------------------------------------------------------------------------------------------------------------------------
def _constant_frame(limit):
    """constant depth, a constant normal facing the camera: every obscurance is 0"""
    w = h = 8
    f = synth.cacao_room(w, h)
    m = np.asarray(f["normals_to_view"], np.float64)[:3, :3]
    n01 = np.ones((h, w, 4), F)
    n01[..., :3] = ((m.T @ np.array([0.0, 0.0, -1.0]) + 1.0) / 2.0).astype(F)
    sh, pp = cacao.constants(w, h, f["proj"], f["normals_to_view"], cacao.settings(adaptiveQualityLimit=limit))
    return A.frame(np.full((h, w), 0.5, F), n01, F32, sh, pp, 0), R.Consts(pp[0])


def test_constant_frame_takes_the_infinite_and_the_nan_quotient():
    r, c = _constant_frame(0.45)
    assert not r["importance"].any() and not r["importance_pong"].any() and r["counter"] == 0
    with np.errstate(all="ignore"):
        assert np.isposinf(c.AdaptiveSampleCountLimit / (F(0.0) * c.LoadCounterAvgDiv))
    assert r["stats"]["limiter"] == 1.0 and r["stats"]["tap_histogram"][6] == 4 * 4 * 4
    r0, c0 = _constant_frame(0.0)
    with np.errstate(all="ignore"):
        assert np.isnan(c0.AdaptiveSampleCountLimit / (F(0.0) * c0.LoadCounterAvgDiv))
    assert r0["counter"] == 0 and r0["stats"]["limiter"] == 0.0 and r0["stats"]["tap_histogram"][6] == 64
    assert np.array_equal(r0["ping"], r["ping"]) and np.array_equal(r0["ao"], r["ao"])         # importance is 0 either way


def test_counter_includes_the_threads_outside_the_map():
    """37 x 23: the map is 10 x 6 inside B's 16 x 8 threads. As written the threads outside add too (their InterlockedAdd targets element 0), while LoadCounterAvgDiv
    divides by 10 * 6: the statement is the source as written, and the other reading gives another counter."""
    f, sh, pp, ref = case("room", 37, 23)
    cs = R.Consts(sh)
    assert ref["importance"].shape == (6, 10) and cs.LoadCounterAvgDiv == F(F(9.0) / F(10 * 6 * 255.0))
    _, written = A.importance_b(ref["importance_pong"], cs)
    _, inside = A.importance_b(ref["importance_pong"], cs, count_threads_outside_the_map=False)
    assert written == ref["counter"] == 1132 and inside == COUNTER_37x23_MAP_ONLY and inside < written
    # 16 x 8 threads, every third in x and y: 6 x 3 add as written, 4 x 2 of them lie inside the map
    assert A.importance_limiter(written, cs) != A.importance_limiter(inside, cs)


COUNTER_37x23_MAP_ONLY = 483


def test_lerp_with_weight_one_is_not_its_second_argument():
    """lerp(maxVal, avgVal, 1.0) = maxVal + 1.0 * (avgVal - maxVal): the difference is rounded before it is added back"""
    max_val, avg_val = F(1.0), F(np.float64(2.0 ** -25 + 2.0 ** -30))
    assert F(max_val + F(1.0) * F(avg_val - max_val)) != avg_val
    # and on the map itself: a pong whose four taps and centre give such a pair is found among all byte pairs of a two-texel map
    found = 0
    c = R.Consts(cacao.constants(4, 4, np.eye(4, dtype=F), np.eye(4, dtype=F), cacao.settings())[0])
    c.ImportanceMapInverseDimensions = np.array([0.5, 1.0], F)
    for a in range(0, 256, 5):
        for b in range(1, 256, 7):
            src = np.array([[a, b]], np.uint8)
            got = A._postprocess(src, c, False, 1, 2)
            inv = c.ImportanceMapInverseDimensions
            for tx in range(2):
                u, v = (F(tx) + F(0.5)) * inv[0], F(0.5) * inv[1]
                hx, hy = F(0.5) * inv[0], F(0.5) * inv[1]
                vals = [A.bilinear_r8(src, u + a_, v + b_) for a_, b_ in ((-hx * F(3.0), -hy), (hx, -hy * F(3.0)), (hx * F(3.0), hy), (-hx, hy * F(3.0)))]
                avg = F(F(F(vals[0] * F(0.25) + vals[1] * F(0.25)) + vals[2] * F(0.25)) + vals[3] * F(0.25))
                found += int(got[0, tx] != avg)
    assert found > 0, "no byte pair separates the contract's lerp from avgVal"


def test_base_weight_byte_round_trip_and_range():
    """The R8G8_UNORM store of weightSum / 20 saturates; the adaptive pass reads byte / 255 * 20. Every code survives the round trip, and the base pass cannot reach
    the clamp: ten hits of weight (0.6 * reduct + 0.4) * newSample.z <= newSample.z, the five z summing to 6.45 of 10 per hit pair."""
    b = np.arange(256, dtype=np.uint8)
    weight = R.from_unorm8(b) * A.LIT_BASE_WEIGHT
    assert np.array_equal(to_unorm8(weight / A.LIT_BASE_WEIGHT), b)
    assert A.LIT_BASE_WEIGHT == F(20.0) and A.LIT_BASE_SHARE == F(0.15625) and A.LIT_0_8 == F(np.float64(0.8))
    largest = F(0.0)
    for i in range(A.BASE_TAPS):
        largest = F(largest + A.SAMPLE_PATTERN[i][2]) + A.SAMPLE_PATTERN[i][2]
    assert largest < F(20.0) and to_unorm8(np.array([largest / F(20.0)], F))[0] < 255
    for kind, (w, h) in (("room", SIZES[2]), ("noise", SIZES[2])):
        assert case(kind, w, h)[3]["base"][..., 1].max() < 255


def test_sample_pattern_is_read_inside_its_32_rows():
    """g_samplePatternMain[i + 2] at i = 30 is one row past the array and feeds nothing: a texel at 32 taps evaluates rows 5 .. 31 and no other"""
    assert A.SAMPLE_PATTERN.shape == (32, 4) and len(PATTERN) == 32
    assert np.array_equal(np.array(PATTERN, F), A.SAMPLE_PATTERN)
    st = case("noise", 125, 93, 1.0)[3]["stats"]
    assert st["tap_histogram"][32] > 0 and st["taps"].max() == 32


# ---- boundary ------------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    src = open(os.path.join(ROOT, "include", "vqhip.h")).read()
    declared = set(re.findall(r"VQHIP_API\s+[\w\s\*]+?\b(vqhip_adaptive_cacao\w*)\s*\(", src))
    assert declared == NEW_SYMBOLS
    lib = capi.load_library()
    for s in declared:
        assert s in capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert lib.vqhip_abi_version() == abi.ABI_VERSION == 3
    for name in ("PLANE_IMPORTANCE", "PLANE_IMPORTANCE_PONG", "PLANE_LOAD_COUNTER"):
        m = re.search(rf"VQHIP_CACAO_{name}\s*=\s*(\d+)", src)
        assert m and int(m.group(1)) == getattr(abi, "CACAO_" + name), name
    assert (abi.CACAO_PLANE_IMPORTANCE, abi.CACAO_PLANE_IMPORTANCE_PONG, abi.CACAO_PLANE_LOAD_COUNTER) == (4, 5, 6)
    # the new declarations follow vqhip_cacao's: what tests/test_cacao_cpu.py finds first stays where it was
    assert src.index("vqhip_adaptive_cacao_work_bytes(int") > src.index("VQHIP_API int vqhip_cacao(")


def test_work_buffer_layout():
    lib = capi.load_library()
    off = lib.vqhip_adaptive_cacao_plane_offset_bytes
    for (w, h) in ((37, 23), (64, 48), (125, 93), (1280, 720), (3840, 2160), (1, 1)):
        hw, hh = abi.cacao_half_dims(w, h)
        iw, ih = abi.cacao_half_dims(hw, hh)
        spans = []
        for k in range(4):
            for s in range(4):
                assert off(w, h, abi.CACAO_PLANE_DEPTHS, s, k) == lib.vqhip_cacao_plane_offset_bytes(w, h, abi.CACAO_PLANE_DEPTHS, s, k)      # HIGH's layout is the prefix
                spans.append((off(w, h, abi.CACAO_PLANE_DEPTHS, s, k), abi.mip_dim(hw, k) * abi.mip_dim(hh, k) * 2))
        for plane, px in ((abi.CACAO_PLANE_NORMALS, 4), (abi.CACAO_PLANE_PING, 2), (abi.CACAO_PLANE_PONG, 2)):
            for s in range(4):
                assert off(w, h, plane, s, 0) == lib.vqhip_cacao_plane_offset_bytes(w, h, plane, s, 0)
                spans.append((off(w, h, plane, s, 0), hw * hh * px))
        new = [(off(w, h, abi.CACAO_PLANE_IMPORTANCE, 0, 0), iw * ih), (off(w, h, abi.CACAO_PLANE_IMPORTANCE_PONG, 0, 0), iw * ih),
               (off(w, h, abi.CACAO_PLANE_LOAD_COUNTER, 0, 0), 4)]
        for o, _ in new:
            assert o % 256 == 0 and o >= lib.vqhip_cacao_work_bytes(w, h)
        spans = sorted(spans + new)
        assert spans[0][0] == 0
        for (a, n), (b, _) in zip(spans, spans[1:]):
            assert a + n <= b, "planes overlap"
        assert spans[-1][0] + spans[-1][1] <= lib.vqhip_adaptive_cacao_work_bytes(w, h)
        assert capi.adaptive_cacao_work_bytes(w, h) == lib.vqhip_adaptive_cacao_work_bytes(w, h)
    assert lib.vqhip_adaptive_cacao_work_bytes(0, 4) == 0 and lib.vqhip_adaptive_cacao_work_bytes(abi.CACAO_MAX_DIM + 1, 4) == 0
    assert off(64, 48, abi.CACAO_PLANE_PING, 4, 0) == 0 and off(64, 48, abi.CACAO_PLANE_PING, 0, 1) == 0
    assert off(64, 48, abi.CACAO_PLANE_IMPORTANCE, 1, 0) == 0 and off(64, 48, abi.CACAO_PLANE_LOAD_COUNTER, 0, 1) == 0 and off(64, 48, 7, 0, 0) == 0 and off(0, 48, 4, 0, 0) == 0
    # the views of a host buffer: HIGH's planes where cacao_work_planes has them, the three new ones with their shapes
    w, h = 37, 23
    buf = np.arange(capi.adaptive_cacao_work_bytes(w, h), dtype=np.uint32).astype(np.uint8)
    v, high = capi.adaptive_cacao_work_planes(buf, w, h), capi.cacao_work_planes(buf, w, h)
    assert all(np.array_equal(v[k], high[k]) for k in ("normals", "ping", "pong")) and v["importance"].shape == v["importance_pong"].shape == (6, 10)
    assert v["counter"].dtype == np.uint32 and v["counter"].shape == (1,)


def test_call_without_a_context_is_refused():
    lib = capi.load_library()
    sh, pp = cacao.constants(8, 8, np.eye(4, dtype=F), np.eye(4, dtype=F), cacao.settings())
    buf = (C.c_uint8 * 4096)()
    rc = lib.vqhip_adaptive_cacao(None, None, buf, 32, buf, R10, 32, C.byref(sh), pp, 2, buf, 4096, buf, 8, 8, 8)
    assert rc == abi.VQHIP_ERR_INVALID_ARG and b"ctx is NULL" in lib.vqhip_last_error(None)


def test_constants_carry_the_adaptive_fields():
    """cacao.constants with settings() — HIGHEST, the reference's default — fills what the adaptive pass reads (tests/test_cacao_cpu.py pins the bits to the golden)"""
    sh, pp = cacao.constants(125, 93, np.eye(4, dtype=F), np.eye(4, dtype=F), cacao.settings())
    for c in [sh] + [pp[i] for i in range(4)]:
        assert tuple(c.ImportanceMapDimensions) == (32.0, 24.0) and F(c.AdaptiveSampleCountLimit) == F(0.45)
        assert F(c.LoadCounterAvgDiv) == F(F(9.0) / F(32 * 24 * 255.0))
    assert [tuple(pp[i].PerPassFullResUVOffset) for i in range(4)] == [(0.0, 0.0), (float(F(1) / F(63)), 0.0), (0.0, float(F(1) / F(47))), (float(F(1) / F(63)), float(F(1) / F(47)))]


def test_cpp_adaptor_forwards_its_arguments_and_refuses_null(tmp_path):
    """tests/cpp/test_passes_adaptive_cacao.cpp against tests/cpp/mock_engine/, with the command line tests/cpp/Makefile uses for test_passes_engine"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = tmp_path / "test_passes_adaptive_cacao"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    lib = os.path.join(ROOT, "vqengine_amd", "lib")
    r = subprocess.run([hipcc, "-std=c++17", "-O2", "-Wall", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I.", "-I../../include", "-I/opt/rocm/include",
                        "test_passes_adaptive_cacao.cpp", "-o", str(exe), "-L../../vqengine_amd/lib", "-lvqhip", "-L/opt/rocm/lib", "-lamdhip64",
                        f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], cwd=cpp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "adaptive cacao adaptor OK" in r.stdout, (r.returncode, r.stdout, r.stderr)
