"""CPU checks of the statement of vqhip_ssr_reproject (tests/ssr_reproject_ref.py, docs/DESIGN_DETAILS.md §7.13): the vectorised statement against an independent
scalar per-pixel transcription of Reproject.hlsl + ffx_denoiser_reflections_reproject.h (its own constants, its own bilinear fetch, its own fma and R11G11B10
encode), bit for bit; the branch population of the committed frames; hand-made cases for the downsample, the guard, the 0.9 threshold, the in-loop update of
reprojection_uv and the R11G11B10 encode; the binding; the C++ adaptor compiled against the stand-in of the engine's RenderPass.h."""
import ctypes
import itertools
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import oracle_lib as O
from tests import ssr_denoise_ref as D
from tests import ssr_reproject_ref as P
from vqengine_amd import abi, capi, synth

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, F32, N10, R11, M16, M32 = abi.FMT_RGBA16F, abi.FMT_RGBA32F, abi.FMT_R10G10B10A2_UNORM, abi.FMT_R11G11B10_FLOAT, abi.FMT_RG16F, abi.FMT_RG32F
FORMATS = dict(normal_fmt=N10, hist_normal_fmt=N10, rad_fmt=F16, hist_fmt=F16, motion_fmt=M16, out_fmt=F16, avg_fmt=R11)
SENTINEL, AVG_SENTINEL = -7.0, 0x80000000


def all_tiles(w, h):
    return np.array([((y * 8) << 16) | (x * 8) for y in range((h + 7) // 8) for x in range((w + 7) // 8)], np.uint32)


def host_inputs(f, fm):
    cast = lambda a, half: np.ascontiguousarray(a.astype(np.float16 if half else np.float32))                        # noqa: E731
    with np.errstate(over="ignore"):
        return dict(depth=f["depth"], normals=f["packed"] if fm["normal_fmt"] == N10 else f["n01"], roughness8=f["roughness8"], depth_hist=f["depth_hist"],
                    normal_hist=f["packed_hist"] if fm["hist_normal_fmt"] == N10 else f["n01_hist"], roughness8_hist=f["roughness8_hist"],
                    radiance=cast(f["radiance"], fm["rad_fmt"] == F16), radiance_hist=cast(f["radiance_hist"], fm["hist_fmt"] == F16),
                    motion=cast(f["motion"], fm["motion_fmt"] == M16), variance_hist=f["variance_hist"], sample_count_hist=f["sample_count_hist"])


def host_outputs(w, h, fm):
    h8, w8 = (h + 7) // 8, (w + 7) // 8
    avg = np.full((h8, w8), AVG_SENTINEL, np.uint32) if fm["avg_fmt"] == R11 else np.full((h8, w8, 4), SENTINEL, np.float32)
    return (np.full((h, w, 4), SENTINEL, np.float16 if fm["out_fmt"] == F16 else np.float32), avg, np.full((h, w), SENTINEL, np.float16), np.full((h, w), SENTINEL, np.float16))


def statement(f, tiles, count, fm, dxc=False, stats=None, hi=None, outs=None):
    w, h = int(f["cb"].bufferDimensions[0]), int(f["cb"].bufferDimensions[1])
    hi = host_inputs(f, fm) if hi is None else hi
    outs = host_outputs(w, h, fm) if outs is None else outs
    return P.reproject(tiles, count, hi["depth"], hi["normals"], fm["normal_fmt"], hi["roughness8"], hi["depth_hist"], hi["normal_hist"], fm["hist_normal_fmt"],
                       hi["roughness8_hist"], hi["radiance"], hi["radiance_hist"], hi["motion"], hi["variance_hist"], hi["sample_count_hist"], f["cb"],
                       outs[0], outs[1], fm["avg_fmt"], outs[2], outs[3], dxc=dxc, stats=stats)


# ---- the scalar transcription: numpy float32 SCALARS, one pixel at a time ------------------------------------------------------------------------
S_LOG2E = F(1.44269502)
S_THRESHOLD = F(0.9)


def to_f32(q):
    """a non-zero Fraction rounded ONCE to binary32, ties to even (Python rounds a Fraction half to even)"""
    sign, q = (-1.0, -q) if q < 0 else (1.0, q)
    e = max(q.numerator.bit_length() - q.denominator.bit_length() - 24, -149)
    while q / Fraction(2) ** e >= 1 << 24:
        e += 1
    while e > -149 and q / Fraction(2) ** e < 1 << 23:
        e -= 1
    return F(sign * float(round(q / Fraction(2) ** e)) * 2.0 ** e)


def s_fma(a, b, c):
    with np.errstate(all="ignore"):
        if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
            return F(np.float64(a) * np.float64(b) + np.float64(c))      # an inf / NaN operand: no rounding question is left
        q = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
        if q == 0:
            return F(np.float64(a) * np.float64(b) + np.float64(c))      # the sign of an exact zero: IEEE's rule, which binary64 follows (the product is exact there)
        return to_f32(q)


def s_exp(x):
    with np.errstate(all="ignore"):
        return O.math_array(1, np.array([F(x) * S_LOG2E], F))[0]


def s_max(a, b):
    return b if (b > a or a != a) else a


def s_min(a, b):
    return b if (b < a or a != a) else a


def s_dot(a, b, dxc):
    if dxc:
        return s_fma(a[2], b[2], s_fma(a[1], b[1], a[0] * b[0]))
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def s_normalize(v, dxc):
    if dxc:
        r = F(1.0 / np.sqrt(np.float64(s_fma(v[2], v[2], s_fma(v[1], v[1], v[0] * v[0])))))
        return tuple(c * r for c in v)
    ln = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    return tuple(c / ln for c in v)


def s_half(x):
    return F(np.float16(x))


def s_floor_int(x):
    if x != x:
        return 0
    return int(min(max(np.floor(np.float64(x)), -2147483648.0), 2147483647.0))


def s_trunc_int(x):
    if x != x:
        return 0
    return int(min(max(np.trunc(np.float64(x)), -2147483648.0), 2147483647.0))


def s_luminance(c, dxc):
    return s_max(s_dot(c, (F(0.299), F(0.587), F(0.114)), dxc), F(0.001))


def s_encode_field(x, mb):
    """nearest representable value of a 5-bit-exponent / mb-bit-mantissa unsigned float by exact comparison against the two neighbouring codes; inf counts as the
    code after the largest finite one (value 65536) so that overflow and its tie follow round-to-nearest-even"""
    if x != x:
        return (31 << mb) | (1 << (mb - 1))
    if np.signbit(x) or x == 0:
        return 0
    top = 31 << mb

    def value(code):
        e, m = code >> mb, code & ((1 << mb) - 1)
        return Fraction(m, 1 << mb) * Fraction(2) ** -14 if e == 0 else (1 + Fraction(m, 1 << mb)) * Fraction(2) ** (e - 15)
    if np.isinf(x):
        return top
    q = Fraction(float(x))
    lo, hi = 0, top                                                   # value(lo) <= q, bisect on the monotone code -> value map
    if q >= value(top):
        return top
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if value(mid) <= q:
            lo = mid
        else:
            hi = mid
    dl, dh = q - value(lo), value(hi) - q
    return lo if dl < dh or (dl == dh and lo % 2 == 0) else hi


class Scalar:
    def __init__(self, f, fm, dxc):
        self.f, self.fm, self.dxc = f, fm, dxc
        cb = f["cb"]
        self.w, self.h = int(cb.bufferDimensions[0]), int(cb.bufferDimensions[1])
        self.hi = host_inputs(f, fm)
        mat = lambda m: [[F(m.m[i][j]) for j in range(4)] for i in range(4)]                                      # noqa: E731
        self.inv_proj, self.inv_view, self.prev_vp = mat(cb.invProjection), mat(cb.invView), mat(cb.prevViewProjection)
        self.thr = F(cb.roughnessThreshold)
        self.kw = {i: s_exp(-F(3.0) * (F(i) * F(i)) / ((F(4) + F(1.0)) * (F(4) + F(1.0)))) for i in range(-4, 5)}
        self.count = dict(glossy=0, hit=0, surface=0, discard=0, early_out=0, search=0, slow=0, uv_outside=0, kept=0)

    # ---- texels
    def inside(self, x, y):
        return 0 <= x < self.w and 0 <= y < self.h

    def n01(self, plane, fmt, x, y):
        if fmt == N10:
            q = int(plane[y, x])
            return tuple(F(c) / F(1023.0) for c in (q & 1023, (q >> 10) & 1023, (q >> 20) & 1023))
        return tuple(F(c) for c in plane[y, x, :3])

    def world_normal(self, n01):
        return s_normalize(tuple(F(2.0) * c - F(1.0) for c in n01), self.dxc)

    def load_normal(self, x, y):
        return self.world_normal(self.n01(self.hi["normals"], self.fm["normal_fmt"], x, y) if self.inside(x, y) else (F(0), F(0), F(0)))

    def load_normal_history(self, x, y):
        return self.world_normal(self.n01(self.hi["normal_hist"], self.fm["hist_normal_fmt"], x, y) if self.inside(x, y) else (F(0), F(0), F(0)))

    def load_radiance_history(self, x, y):
        return tuple(F(c) for c in self.hi["radiance_hist"][y, x, :3]) if self.inside(x, y) else (F(0), F(0), F(0))

    def load_depth_history(self, x, y):
        return F(self.hi["depth_hist"][y, x]) if self.inside(x, y) else F(0)

    # ---- the sampler: CLAMP, 8-bit fractions, the FMA chain
    def sample(self, fetch, u, v):
        """fetch(x, y) -> tuple of binary32 channels of an IN-RANGE texel"""
        def axis(t, n):
            k = s_floor_int((t * F(n) - F(0.5)) * F(256.0) + F(0.5))
            i, wgt = k >> 8, F(k & 255) * F(1.0 / 256.0)
            return min(max(i, 0), n - 1), min(max(i + 1, 0), n - 1), wgt
        x0, x1, wx = axis(u, self.w)
        y0, y1, wy = axis(v, self.h)
        c00, c10, c01, c11 = fetch(x0, y0), fetch(x1, y0), fetch(x0, y1), fetch(x1, y1)
        w00, w10, w01, w11 = (F(1) - wx) * (F(1) - wy), wx * (F(1) - wy), (F(1) - wx) * wy, wx * wy
        return tuple(s_fma(w11, c11[k], s_fma(w01, c01[k], s_fma(w10, c10[k], w00 * c00[k]))) for k in range(len(c00)))

    def sample_normal_history(self, u, v):
        return self.world_normal(self.sample(lambda x, y: self.n01(self.hi["normal_hist"], self.fm["hist_normal_fmt"], x, y), u, v))

    def sample_radiance_history(self, u, v):
        return self.sample(lambda x, y: tuple(F(c) for c in self.hi["radiance_hist"][y, x, :3]), u, v)

    def sample_depth_history(self, u, v):
        return self.sample(lambda x, y: (F(self.hi["depth_hist"][y, x]),), u, v)[0]

    def sample_roughness_history(self, u, v):
        return self.sample(lambda x, y: (F(self.hi["roughness8_hist"][y, x]) / F(255.0),), u, v)[0]

    def sample_r16f(self, plane, u, v):
        return self.sample(lambda x, y: (F(plane[y, x]),), u, v)[0]

    # ---- geometry
    def mul(self, M, p):
        return tuple(((p[0] * M[0][j] + p[1] * M[1][j]) + p[2] * M[2][j]) + F(1.0) * M[3][j] for j in range(4))

    def linear_depth(self, u, v, z):
        cy = F(1.0) - v
        q = (F(2.0) * u - F(1.0), F(2.0) * cy - F(1.0), z)
        M = self.inv_proj
        pz = ((q[0] * M[0][2] + q[1] * M[1][2]) + q[2] * M[2][2]) + F(1.0) * M[3][2]
        pw = ((q[0] * M[0][3] + q[1] * M[1][3]) + q[2] * M[2][3]) + F(1.0) * M[3][3]
        return abs(pz / pw)

    def disocclusion(self, n, hn, ld, hld):
        return (F(1.0) * s_exp(-abs(F(1.0) - s_max(F(0.0), s_dot(n, hn, self.dxc))) * F(1.4))) * s_exp(-abs(hld - ld) / ld * F(1.0))

    # ---- FFX_DNSR_Reflections_PickReprojection: (disocclusion_factor, reprojection_uv | None, reprojection | None)
    def pick(self, px, py, lds, gx, gy, roughness, ray_length):
        dxc = self.dxc
        mean, var, acc = [F(0)] * 3, [F(0)] * 3, F(0)
        for j in range(-4, 5):
            for i in range(-4, 5):
                r = lds[gy + j][gx + i]
                wgt = self.kw[i] * self.kw[j]
                acc = acc + wgt
                mean = [mean[k] + r[k] * wgt for k in range(3)]
                var = [var[k] + r[k] * r[k] * wgt for k in range(3)]
        mean = [m / acc for m in mean]
        var = [v / acc for v in var]
        var = [abs(var[k] - mean[k] * mean[k]) for k in range(3)]
        u, v = (F(px) + F(0.5)) / F(self.w), (F(py) + F(0.5)) / F(self.h)
        normal = self.load_normal(px, py)
        mv = self.hi["motion"][py, px] if self.inside(px, py) else (0.0, 0.0)
        motion = (F(mv[0]) * F(0.5), F(mv[1]) * F(-0.5))
        s_uv = (u - motion[0], v - motion[1])
        z = F(self.hi["depth"][py, px]) if self.inside(px, py) else F(0)
        cy = F(1.0) - v
        p4 = self.mul(self.inv_proj, (F(2.0) * u - F(1.0), F(2.0) * cy - F(1.0), z))
        ray = [p4[k] / p4[3] for k in range(3)]
        surface_depth = np.sqrt(s_dot(ray, ray, dxc))
        length = surface_depth + ray_length
        ray = [c / surface_depth for c in ray]
        ray = [c * length for c in ray]
        world = self.mul(self.inv_view, ray)[:3]
        q4 = self.mul(self.prev_vp, world)
        prj = [q4[k] / q4[3] for k in range(3)]
        h_uv = (F(0.5) * prj[0] + F(0.5), F(1) - (F(0.5) * prj[1] + F(0.5)))
        s_n, h_n = self.sample_normal_history(*s_uv), self.sample_normal_history(*h_uv)
        s_hist, h_hist = self.sample_radiance_history(*s_uv), self.sample_radiance_history(*h_uv)
        nn = s_normalize(normal, dxc)
        h_sim, s_sim = s_dot(s_normalize(h_n, dxc), nn, dxc), s_dot(s_normalize(s_n, dxc), nn, dxc)
        h_r, s_r = self.sample_roughness_history(*h_uv), self.sample_roughness_history(*s_uv)
        if h_sim > F(0.9999) and h_sim + F(1.0e-3) > s_sim and abs(h_r - roughness) < abs(s_r - roughness) + F(1.0e-3):
            self.count["hit"] += self.on
            hist_n, r_uv, rep = h_n, h_uv, h_hist
        else:
            d = [s_hist[k] - mean[k] for k in range(3)]
            if s_dot(d, d, dxc) < F(1.5) * np.sqrt(s_dot(var, var, dxc)):
                self.count["surface"] += self.on
                hist_n, r_uv, rep = s_n, s_uv, s_hist
            else:
                self.count["discard"] += self.on
                return F(0.0), None, None
        hld = self.linear_depth(r_uv[0], r_uv[1], self.sample_depth_history(*r_uv))
        ld = self.linear_depth(u, v, z)
        df = self.disocclusion(normal, hist_n, ld, hld)
        if df > S_THRESHOLD:
            self.count["early_out"] += self.on
            return df, r_uv, rep
        if df < S_THRESHOLD:
            self.count["search"] += self.on
            dudv = (F(1.0) / F(self.w), F(1.0) / F(self.h))
            for y in (-1, 0, 1):
                for x in (-1, 0, 1):
                    t = (r_uv[0] + F(x) * dudv[0], r_uv[1] + F(y) * dudv[1])
                    wgt = self.disocclusion(normal, self.sample_normal_history(*t), ld, self.linear_depth(t[0], t[1], self.sample_depth_history(*t)))
                    if wgt > df:
                        df, r_uv = wgt, t
            rep = self.sample_radiance_history(*r_uv)
        if df < S_THRESHOLD:
            self.count["slow"] += self.on
            fx, fy = F(self.w) * r_uv[0] + F(0.5), F(self.h) * r_uv[1] + F(0.5)
            uvx, uvy = fx - np.floor(fx), fy - np.floor(fy)
            tx, ty = s_trunc_int(F(self.w) * r_uv[0] - F(0.5)), s_trunc_int(F(self.h) * r_uv[1] - F(0.5))
            at = [(tx, ty), (tx + 1, ty), (tx, ty + 1), (tx + 1, ty + 1)]
            rr = [self.load_radiance_history(*c) for c in at]
            ns = [self.load_normal_history(*c) for c in at]
            ds = [self.linear_depth(r_uv[0], r_uv[1], self.load_depth_history(*c)) for c in at]
            wq = [F(1.0) if self.disocclusion(normal, ns[k], ld, ds[k]) > S_THRESHOLD / F(2.0) else F(0.0) for k in range(4)]
            wq = [wq[0] * (F(1.0) - uvx) * (F(1.0) - uvy), wq[1] * uvx * (F(1.0) - uvy), wq[2] * (F(1.0) - uvx) * uvy, wq[3] * uvx * uvy]
            ws = s_max(wq[0] + wq[1] + wq[2] + wq[3], F(1.0e-3))
            wq = [c / ws for c in wq]
            rep = tuple(rr[0][k] * wq[0] + rr[1][k] * wq[1] + rr[2][k] * wq[2] + rr[3][k] * wq[3] for k in range(3))
            hld = ds[0] * wq[0] + ds[1] * wq[1] + ds[2] * wq[2] + ds[3] * wq[3]
            hn = tuple(ns[0][k] * wq[0] + ns[1][k] * wq[1] + ns[2][k] * wq[2] + ns[3][k] * wq[3] for k in range(3))
            df = self.disocclusion(normal, hn, ld, hld)
        df = F(0.0) if df < S_THRESHOLD else df
        return df, r_uv, rep

    # ---- FFX_DNSR_Reflections_Reproject for one tile
    def tile(self, x0, y0, outs):
        o_rep, o_avg, o_var, o_cnt = outs
        dxc = self.dxc
        rad_img = self.hi["radiance"]
        lds = [[tuple(s_half(F(rad_img[y0 - 4 + j, x0 - 4 + i, k])) for k in range(3)) if self.inside(x0 - 4 + i, y0 - 4 + j) else (F(0), F(0), F(0))
                for i in range(16)] for j in range(16)]
        shared = [[None] * 8 for _ in range(8)]
        for gy in range(8):
            for gx in range(8):
                px, py = x0 + gx, y0 + gy
                on = self.inside(px, py)
                roughness = F(self.hi["roughness8"][py, px]) / F(255.0) if on else F(0)
                radiance = [F(c) for c in rad_img[py, px, :3]] if on else [F(0)] * 3
                ray_length = F(rad_img[py, px, 3]) if on else F(0)
                if roughness < self.thr:
                    self.on = int(on)                        # the branch counters cover pixels of the frame only
                    df, r_uv, rep = self.pick(px, py, lds, gx + 4, gy + 4, roughness, ray_length)
                    store = ((F(0), F(0), F(0)), F(1.0), F(1.0))
                    if on:
                        self.count["glossy"] += 1
                    if r_uv is not None:                      # the discard branch: defined as the store of (0, 0, 0) / 1 / 1, the radiance is not mixed
                        if r_uv[0] > 0 and r_uv[1] > 0 and r_uv[0] < F(1.0) and r_uv[1] < F(1.0):
                            prev_var = self.sample_r16f(self.hi["variance_hist"], *r_uv)
                            num = self.sample_r16f(self.hi["sample_count_hist"], *r_uv) * df
                            s_max_samples = s_max(F(8.0), F(32) * (F(1.0) - s_exp(-roughness * F(100.0))))
                            num = s_min(s_max_samples, num + F(1))
                            hl, lum = s_luminance(radiance, dxc), s_luminance(rep, dxc)      # ComputeTemporalVariance(radiance, reprojection)
                            diff = abs(hl - lum) / s_max(s_max(hl, lum), F(0.5))
                            new_var = diff * diff
                            if not df < S_THRESHOLD:
                                store = (rep, new_var + (F(1.0) / num) * (prev_var - new_var), num)
                                radiance = [radiance[k] + F(0.3) * (rep[k] - radiance[k]) for k in range(3)]
                                self.count["kept"] += on
                        else:
                            self.count["uv_outside"] += on
                    if on:
                        o_rep[py, px] = np.array(list(store[0]) + [F(0)], F).astype(o_rep.dtype)
                        o_var[py, px], o_cnt[py, px] = np.float16(store[1]), np.float16(store[2])
                weight = s_max(s_exp(-s_luminance(radiance, dxc) * F(0.3)), F(1.0e-2))
                radiance = [c * weight for c in radiance]
                if px >= self.w or py >= self.h or any(np.isinf(c) for c in radiance) or any(np.isnan(c) for c in radiance) or weight > F(1.0e3):
                    radiance, weight = [F(0)] * 3, F(0)
                shared[gy][gx] = [s_half(c) for c in radiance + [weight]]
        i = 2
        while i <= 8:
            for gy in range(8):
                for gx in range(8):
                    ox, oy, ix, iy = gx * i, gy * i, gx * i + i // 2, gy * i + i // 2
                    if ix < 8 and iy < 8:
                        w00, w10, w01, w11 = shared[oy][ox], shared[iy][ox], shared[oy][ix], shared[iy][ix]      # the source's names: 10 = (ox, iy), 01 = (ix, oy)
                        shared[oy][ox] = [s_half(w00[k] + w01[k] + w10[k] + w11[k]) for k in range(4)]
            i *= 2
        total = shared[0][0]
        wacc = s_max(total[3], F(1.0e-3))
        avg = [total[k] / wacc for k in range(3)]
        if self.fm["avg_fmt"] == R11:
            o_avg[y0 // 8, x0 // 8] = s_encode_field(avg[0], 6) | (s_encode_field(avg[1], 6) << 11) | (s_encode_field(avg[2], 5) << 22)
        else:
            o_avg[y0 // 8, x0 // 8] = avg + [F(0)]

    def run(self, tiles):
        outs = host_outputs(self.w, self.h, self.fm)
        with np.errstate(all="ignore"):
            for e in sorted(set(int(t) for t in tiles)):
                self.tile(((e & 0xFFFF) >> 3) * 8, ((e >> 16) >> 3) * 8, outs)
        return outs


def check_against_scalar(f, fm, dxc, what):
    w, h = int(f["cb"].bufferDimensions[0]), int(f["cb"].bufferDimensions[1])
    tiles = all_tiles(w, h)
    st = {}
    ref = statement(f, tiles, tiles.size, fm, dxc=dxc, stats=st)
    sc = Scalar(f, fm, dxc)
    got = sc.run(tiles)
    for k, name in enumerate(("reprojected radiance", "average radiance", "variance", "sample count")):
        n, idx = O.bits_equal(got[k], ref[k])
        assert n == 0, f"{what}: {name}: {n} mismatching elements, first {idx.tolist()}"
    for k, v in sc.count.items():
        assert int(st[k].sum()) == v, (what, k)
    return st


@pytest.mark.parametrize("dxc", [False, True])
@pytest.mark.parametrize("nf,hnf,rf,hf,mf", list(itertools.product([N10, F32], [N10, F32], [F16, F32], [F16, F32], [M16, M32])))
def test_statement_equals_the_scalar_transcription_8x8_every_format(nf, hnf, rf, hf, mf, dxc):
    """all 128 format combinations in both readings: one case per input-format set, each with the four output-format pairs"""
    f = synth.ssr_reproject_frames(8, 8, seed=0xF08)
    f["roughness8"][:] = np.where(np.arange(8)[None, :] < 5, 25, 200)
    for of, af in itertools.product([F16, F32], [R11, F32]):
        fm = dict(normal_fmt=nf, hist_normal_fmt=hnf, rad_fmt=rf, hist_fmt=hf, motion_fmt=mf, out_fmt=of, avg_fmt=af)
        check_against_scalar(f, fm, dxc, f"8 x 8 dxc {dxc} {fm}")


@pytest.mark.parametrize("dxc", [False, True])
@pytest.mark.parametrize("W,H", [(16, 16), (19, 13)])
def test_statement_equals_the_scalar_transcription(W, H, dxc):
    check_against_scalar(synth.ssr_reproject_frames(W, H, seed=0x1600 + W), FORMATS, dxc, f"{W} x {H} dxc {dxc}")


# the pixels per branch of synth.ssr_reproject_frames(67, 45) (seed 0x4E90), literal reading: a CONDITION of the frames (each >= 32), committed as numbers
BRANCHES_67x45 = dict(hit=959, surface=1318, discard=198, early_out=1725, search=552, slow=514, uv_outside=391, kept=1722, not_glossy=540)


def test_statement_equals_the_scalar_transcription_67x45_and_branch_coverage():
    st = check_against_scalar(synth.ssr_reproject_frames(67, 45), FORMATS, False, "67 x 45")
    counts = {k: int(v.sum()) for k, v in st.items()}
    counts["not_glossy"] = 67 * 45 - counts.pop("glossy")
    for k in ("hit", "surface", "discard", "early_out", "search", "slow", "uv_outside", "not_glossy"):
        assert counts[k] >= 32, (k, counts)
    assert counts == BRANCHES_67x45, counts


# ---- hand-made cases ----------------------------------------------------------------------------------------------------------------------------------
def test_downsample_order_and_binary16_round_trips_are_observable():
    rng = np.random.default_rng(0xD0)
    rw = ((1.0 + rng.random((64, 8, 8, 4))) * np.exp2(rng.integers(-12, 13, (64, 8, 8, 4)))).astype(F)
    # tile 0, the order: ((4096 + 2) + 2^-12) + 2^-12 = 4098 in binary32 (two ties to even), which binary16 rounds to 4096 (a tie to even again); summed as
    # (4096 + 2) + (2^-12 + 2^-12) = 4098 + 2^-11, which binary16 rounds to 4100
    rw[0] = 0
    rw[0, 0, 0], rw[0, 0, 1], rw[0, 1, 0], rw[0, 1, 1] = 4096.0, 2.0, 2.0 ** -12, 2.0 ** -12
    # tile 1, the per-level store: three 2 x 2 blocks of 1 + 2^-11 each store 1 (a binary16 tie to even), their sum is 3; kept in binary32 the sum 3 + 3 * 2^-11 stores as 3 + 2^-9
    rw[1] = 0
    for y, x in ((0, 0), (0, 2), (2, 0)):
        rw[1, y, x], rw[1, y, x + 1] = 1.0, 2.0 ** -11
    want = P.downsample(rw)
    assert (want[0] == 4096.0).all() and (want[1] == 3.0).all()
    p = P.f16r(rw)
    for t in range(rw.shape[0]):                                          # the loops as written
        s = [[[F(c) for c in p[t, y, x]] for x in range(8)] for y in range(8)]
        for i in (2, 4, 8):
            for gy in range(8):
                for gx in range(8):
                    ox, oy, ix, iy = gx * i, gy * i, gx * i + i // 2, gy * i + i // 2
                    if ix < 8 and iy < 8:
                        s[oy][ox] = [s_half(((s[oy][ox][k] + s[oy][ix][k]) + s[iy][ox][k]) + s[iy][ix][k]) for k in range(4)]
        assert O.bits_equal(np.array(s[0][0], F), want[t])[0] == 0
    q = p
    for _ in range(3):                                                    # NOT the contract: the two rows summed separately
        q = P.f16r((q[:, 0::2, 0::2] + q[:, 0::2, 1::2]) + (q[:, 1::2, 0::2] + q[:, 1::2, 1::2]))
    assert (q[0, 0, 0] == 4100.0).all(), "another summation order changes bits"
    q = p
    for _ in range(3):                                                    # NOT the contract: no binary16 store between the levels
        q = ((q[:, 0::2, 0::2] + q[:, 0::2, 1::2]) + q[:, 1::2, 0::2]) + q[:, 1::2, 1::2]
    assert (P.f16r(q[1, 0, 0]) == F(3.0 + 2.0 ** -9)).all(), "the per-level binary16 round trip changes bits"
    assert O.bits_equal(P.downsample(rw), P.downsample(p))[0] == 0, "the first store is a binary16 round trip as well"


def flat_frames(w=16, h=16, rgb=(1.0, 0.5, 0.25)):
    """rough everywhere (no reprojection): the average is the luminance-weighted mean of the traced radiance alone"""
    f = synth.ssr_reproject_frames(w, h, seed=0xF1A7)
    f["roughness8"][:] = 255
    f["radiance"][..., :3] = rgb
    return f


def test_guard_keeps_inf_nan_and_pixels_beyond_the_screen_out_of_the_average():
    fm = dict(FORMATS, rad_fmt=F32, avg_fmt=F32)
    f = flat_frames(12, 12)                                               # tiles (8, 0), (0, 8), (8, 8) are partial
    base = statement(f, all_tiles(12, 12), 4, fm)[1]
    assert O.bits_equal(base[0, 0], base[1, 1])[0] == 0, "a partial tile of the same colour averages to the same value: pixels beyond the screen carry weight 0"
    # weight = exp(-lum * 0.3) with lum = 0.299 + 0.587 * 0.5 + 0.114 * 0.25; 64 equal terms: sum(rad * w) / sum(w) up to the binary16 steps
    assert np.allclose(base[0, 0, :3], (1.0, 0.5, 0.25), rtol=2e-3) and base[0, 0, 3] == 0
    g = flat_frames(12, 12)
    g["radiance"][0, 0, 0], g["radiance"][1, 1, 1], g["radiance"][2, 2, 2] = np.inf, np.nan, -np.inf
    g["radiance"][3, 3, :3] = 3e38                                        # finite in binary32, finite * weight as well: NOT guarded, overflows binary16 in the store
    out = statement(g, all_tiles(12, 12), 4, fm)[1]
    assert np.isinf(out[0, 0, :3]).all() or np.isnan(out[0, 0, :3]).any(), "a finite value that overflows binary16 is not what the guard tests"
    g["radiance"][3, 3, :3] = (1.0, 0.5, 0.25)
    out = statement(g, all_tiles(12, 12), 4, fm)[1]
    assert np.isfinite(out).all() and np.allclose(out[0, 0, :3], (1.0, 0.5, 0.25), rtol=2e-3), "inf / NaN pixels are dropped with their weight"
    assert O.bits_equal(out[1:], base[1:])[0] == 0


@pytest.mark.parametrize("dxc", [False, True])
def test_disocclusion_factor_exactly_at_the_threshold_takes_neither_branch(dxc):
    """synth.ssr_reproject_threshold_frames: constructed pixels whose factor is the word of 0.9f, through the statement AND the scalar transcription"""
    f = synth.ssr_reproject_threshold_frames()
    fm = dict(FORMATS, normal_fmt=F32, hist_normal_fmt=F32)
    n = tuple(np.array([c], F) for c in (0.0, 1.0, 0.0))
    hn = P._norm3(f["n01_hist"][:1, :1, :3].reshape(1, 3), dxc)
    factor = P.disocclusion_factor(n, hn, np.array([12.5], F), np.array([12.5], F), dxc)
    assert factor.astype(F).view(np.uint32)[0] == 0x3F666666, "the constructed normals give exactly 0.9"
    st = check_against_scalar(f, fm, dxc, f"threshold dxc {dxc}")
    assert st["glossy"].sum() == 64 and st["surface"].sum() == 64, "every glossy pixel takes the surface reprojection"
    assert st["early_out"].sum() == 0 and st["search"].sum() == 0 and st["slow"].sum() == 0, "0.9 is neither > 0.9 nor < 0.9"
    assert st["kept"].sum() == 64 and st["uv_outside"].sum() == 0, "0.9 is not < 0.9: the history is kept"
    rep, _, _, cnt = statement(f, all_tiles(16, 16), 4, fm, dxc=dxc)
    assert (rep[4:12, 4:12, :3] == np.float16(1.0)).all()
    smax = F(32.0) * (F(1.0) - P.exp_(np.array([-(F(25) / F(255.0)) * F(100.0)], F))[0])
    want = np.minimum(smax, f["sample_count_hist"][4:12, 4:12].astype(F) * F(0.9) + F(1.0)).astype(np.float16)
    assert (cnt[4:12, 4:12] == want).all(), "num_samples = min(s_max, history * 0.9 + 1)"


def test_search_offsets_from_the_updated_reprojection_uv():
    """One constructed pixel at (8, 8) of a 16 x 16 frame. Its history normal is perpendicular to its own (factor exp(-1.4)); the history texel at (7, 7) — the search's
    FIRST tap — is better (dot 0.8), so reprojection_uv moves there inside the loop; the texel at (6, 8) matches exactly and is a tap of the 3 x 3 around (7, 7) only (it is
    two columns away from the pixel). Only with the in-loop update is it ever sampled: the pixel then reprojects that texel's radiance and keeps it."""
    w = h = 16
    f = synth.ssr_reproject_frames(w, h, seed=0x5EA)
    rng = np.random.default_rng(0x5EA)
    f["cb"].prevViewProjection = synth.ssr_constants(w, h, 1).prevViewProjection                    # the camera did not move
    f["roughness8"][:] = 255
    f["roughness8"][8, 8] = 25
    f["roughness8_hist"][:] = 25
    f["motion"][:] = 0
    f["depth"][:] = 0.99
    f["depth_hist"][:] = 0.99
    f["radiance"][..., :3] = 1.0 + 0.6 * (rng.random((h, w, 3), dtype=np.float32) - 0.5)
    f["radiance"][..., 3] = 0.0
    f["radiance_hist"][..., :3] = 1.0
    f["radiance_hist"][8, 6, :3] = 1.25
    own, perpendicular = np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0])
    better = 0.8 * own + 0.6 * perpendicular
    f["n01"][..., :3] = own * 0.5 + 0.5
    f["n01_hist"][..., :3] = perpendicular * 0.5 + 0.5
    f["n01_hist"][7, 7, :3] = better * 0.5 + 0.5
    f["n01_hist"][8, 6, :3] = own * 0.5 + 0.5
    fm = dict(FORMATS, normal_fmt=F32, hist_normal_fmt=F32)
    st = {}
    rep, _, _, cnt = statement(f, all_tiles(w, h), 4, fm, stats=st)
    assert st["surface"].sum() == 1 and st["search"].sum() == 1 and st["slow"].sum() == 0 and st["kept"].sum() == 1
    assert (rep[8, 8, :3] == np.float16(1.25)).all() and rep[8, 8, 3] == 0
    assert (rep[..., 0] != SENTINEL).sum() == 1
    sc = Scalar(f, fm, False)
    got = sc.run(all_tiles(w, h))
    assert O.bits_equal(got[0], rep)[0] == 0 and O.bits_equal(got[3], cnt)[0] == 0


def test_r11g11b10_encode_over_every_field_value():
    codes6, codes5 = np.arange(1 << 11, dtype=np.uint32), np.arange(1 << 10, dtype=np.uint32)
    words = np.concatenate([codes6, codes6 << 11, codes5 << 22]).astype(np.uint32)
    values = D.decode_r11g11b10(words)
    again = P.encode_r11g11b10(values)
    nan = np.isnan(values).any(-1)
    assert (again[~nan] == words[~nan]).all(), "every representable value round-trips"
    canon = np.concatenate([np.full(1 << 11, (31 << 6) | 32), np.full(1 << 11, ((31 << 6) | 32) << 11), np.full(1 << 10, ((31 << 5) | 16) << 22)]).astype(np.uint32)
    assert (again[nan] == canon[nan]).all(), "NaN: exponent 31 with a non-zero mantissa"
    assert np.isnan(D.decode_r11g11b10(again[nan])).any(-1).all()
    # ties and their neighbours, per channel, against the exact-comparison encoder
    for ch, mb in ((0, 6), (1, 6), (2, 5)):
        shift = (0, 11, 22)[ch]
        finite = np.arange(31 << mb, dtype=np.uint32)
        v = D.decode_r11g11b10(finite << shift)[:, ch].astype(np.float64)
        nxt = np.append(v[1:], 65536.0)
        mid = ((v + nxt) / 2).astype(F)                                   # exact: one more mantissa bit
        assert ((v + nxt) / 2 == mid).all()
        probe = np.concatenate([mid, np.nextafter(mid, F(0)), np.nextafter(mid, F(np.inf)), np.array([65504.0, 65535.9, 65536.0, 1e30, np.inf, 3e-8, 1e-45, 0.0], F)])
        rgb = np.zeros((probe.size, 3), F)
        rgb[:, ch] = probe
        got = (P.encode_r11g11b10(rgb) >> shift) & ((1 << (5 + mb)) - 1)
        want = np.array([s_encode_field(x, mb) for x in probe], np.uint32)
        assert (got == want).all(), (ch, probe[got != want][:5])
        tie = got[:mid.size]
        assert (tie % 2 == 0).all(), "a tie goes to the even code (at the top: to inf)"
    neg = np.array([[-1.0, -0.0, -np.inf], [-1e-30, -65504.0, -3e38]], F)
    assert (P.encode_r11g11b10(neg) == 0).all(), "negative values and -0 encode as 0"
    rng = np.random.default_rng(0x11B)
    x = np.exp(rng.uniform(np.log(1e-8), np.log(2e5), (4000, 3))).astype(F)
    want = np.array([s_encode_field(a, 6) | (s_encode_field(b, 6) << 11) | (s_encode_field(c, 5) << 22) for a, b, c in x], np.uint32)
    assert (P.encode_r11g11b10(x) == want).all()
    assert (synth.encode_r11g11b10(x) != want).any(), "the input maker double-rounds through binary16: a different encoder, kept as it is"


def test_bindings_are_present():
    lib = capi.load_library()
    assert "vqhip_ssr_reproject" in capi.EXPORTED_SYMBOLS and hasattr(lib, "vqhip_ssr_reproject") and hasattr(capi.Context, "ssr_reproject")
    header = open(os.path.join(ROOT, "include", "vqhip.h")).read()
    assert "vqhip_ssr_reproject(vqhip_ctx* ctx, void* stream, const vqhip_ssr_reproject_surfaces* io, const VQ_SSSRConstants* cb)" in header
    assert abi.ABI_VERSION == 3


def test_surfaces_struct_layout_matches_the_header(tmp_path):
    fields = [n for n, _ in abi.SSRReprojectSurfaces._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vqhip.h"\nint main(void){printf("%zu", sizeof(vqhip_ssr_reproject_surfaces));\n'
                   + "".join(f'printf(" %zu", offsetof(vqhip_ssr_reproject_surfaces, {n}));\n' for n in fields) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(abi.SSRReprojectSurfaces)] + [getattr(abi.SSRReprojectSurfaces, n).offset for n in fields]


def test_cpp_adaptor_forwards_its_planes_and_refuses_null(tmp_path):
    """tests/cpp/test_passes_reproject.cpp against tests/cpp/mock_engine/, with the command line tests/cpp/Makefile uses for test_passes_engine"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = tmp_path / "test_passes_reproject"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    lib = os.path.join(ROOT, "vqengine_amd", "lib")
    r = subprocess.run([hipcc, "-std=c++17", "-O2", "-Wall", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I.", "-I../../include", "-I/opt/rocm/include", "test_passes_reproject.cpp",
                        "-o", str(exe), "-L../../vqengine_amd/lib", "-lvqhip", "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"],
                       cwd=cpp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "reproject adaptor OK" in r.stdout, (r.returncode, r.stdout, r.stderr)
