"""docs/DESIGN_DETAILS.md §7.19 (the contract M1 .. M5 of vqhip_scene_masked_depth and vqhip_shadow_masked_depth) stated in numpy, on top of tests/scene_depth_ref.py,
tests/shadow_raster_ref.py and tests/scene_interp_ref.py: setup, clipping, coverage, depth and the minimum are theirs (M5); this file adds the alpha test of the
"_AlphaMasked" pixel shaders in front of the minimum.

  M1  the test runs once per (primitive, pixel) at the pixel centre; a discard removes all of the primitive's samples in the pixel. Shadow maps: pixel = texel.
  M2  uv at the pixel centre: scene_interp_ref's I2 weights (binary64, from the unclipped triangle's binary32 clip x, y, w) and I3 blend (binary64, one rounding).
  M3  scene depth: uv * scale + offset in binary32, the isotropic trilinear WRAP fetch of an RGBA8 mip chain with derivatives from HELPER LANES — the same primitive
      evaluated by M2 at (i ^ 1, j) and (i, j ^ 1) — own - neighbour on the odd lane, neighbour - own on the even one; discard iff HasDiffuseMap && a < 0.01.
  M4  shadow: the raw uv, the bilinear WRAP fetch of level 0, discard iff a < 0.01 (no HasDiffuseMap test).

The sampler is the arithmetic of vqengine_amd/csrc/vq_tex8.h: 8-bit fixed-point fractions, exact bilinear weights, fma(f, hi, (1 - f) lo) between levels, the
contract's log2 (tests/cacao_ref.log2_). An FMA is evaluated in binary64 and rounded once to binary32: exact for the blends (their operands have few bits), and
for the squared derivative lengths of the LOD as long as the two squares are within 2^5 of each other in magnitude or the sum is no rounding tie.
tests/test_masked_depth_cpu.py pins every decision of the cases to the oracle's sampler.

A scene is scene_depth_ref's dict whose draws may carry `mask`: None (opaque) or dict(tex = dict(chain uint8 [px, 4] | None, w, h, mips), scale_offset = 4 floats,
texture_config float) with positions float32 [V, >= 11] (uv at columns 9, 10). A view is shadow_raster_ref's dict whose draws may carry `mask` = dict(tex = ...)."""
import numpy as np

from tests import scene_depth_ref as V
from tests import scene_interp_ref as I
from tests import shadow_raster_ref as R
from tests.cacao_ref import _floor_i, fixed8, log2_

F, F64, I64, U32 = np.float32, np.float64, np.int64, np.uint32
RCP255 = F(0.0039215688593685627)
ALPHA_CUT = F(0.01)


def fma(a, b, c):
    return (np.asarray(a, F).astype(F64) * np.asarray(b, F).astype(F64) + np.asarray(c, F).astype(F64)).astype(F)


def has_diffuse_map(texture_config):
    """HasDiffuseMap(int(textureConfig)): bit 0 of the truncated value (NaN -> 0)"""
    t = F(texture_config)
    return bool(0 if np.isnan(t) else int(np.clip(t, F(-2147483520.0), F(2147483520.0))) & 1)


# ---- the RGBA8 fetch (alpha channel) -------------------------------------------------------------------------------------------------------------------------
def mip_dim(d, level):
    return max(d >> level, 1)


def level_offset(w, h, level):
    return sum(mip_dim(w, k) * mip_dim(h, k) for k in range(level))


def level_alpha(tex, level, u, v):
    """bilinear WRAP fetch of one level, in byte units (exact in binary32): level int array, u / v float32 arrays of one shape"""
    level = np.asarray(level, I64)
    out = np.zeros(u.shape, F)
    alpha = tex["chain"][:, 3].astype(F)
    for lv in np.unique(level):
        m = level == lv
        W, H = mip_dim(tex["w"], int(lv)), mip_dim(tex["h"], int(lv))
        ix, wx = fixed8(u[m] * F(W) - F(0.5))
        iy, wy = fixed8(v[m] * F(H) - F(0.5))
        x0, x1, y0, y1 = np.mod(ix, W), np.mod(ix + 1, W), np.mod(iy, H), np.mod(iy + 1, H)
        base = level_offset(tex["w"], tex["h"], int(lv))
        c00, c10, c01, c11 = alpha[base + y0 * W + x0], alpha[base + y0 * W + x1], alpha[base + y1 * W + x0], alpha[base + y1 * W + x1]
        one = F(1.0)
        w00, w10, w01, w11 = (one - wx) * (one - wy), wx * (one - wy), (one - wx) * wy, wx * wy
        out[m] = fma(w11, c11, fma(w01, c01, fma(w10, c10, w00 * c00)))
    return out


def sample_alpha(tex, u, v, ddx, ddy):
    """Texture2D.Sample(AnisoSampler, uv).a as the library restates it: isotropic trilinear WRAP, bias 0. u, v float32 arrays; ddx, ddy = (du, dv) pairs."""
    u, v = np.asarray(u, F), np.asarray(v, F)
    if tex is None or tex["chain"] is None:
        return np.zeros(u.shape, F)
    with np.errstate(all="ignore"):
        W, H, mips = F(tex["w"]), F(tex["h"]), int(tex["mips"])
        dXx, dXy, dYx, dYy = ddx[0] * W, ddx[1] * H, ddy[0] * W, ddy[1] * H
        rx, ry = fma(dXy, dXy, dXx * dXx), fma(dYy, dYy, dYx * dYx)
        lod = F(0.5) * log2_(np.fmax(rx, ry)) + F(0.0)
        maxl = F(mips - 1)
        lvl = np.where(lod > 0, np.where(lod < maxl, lod, maxl), F(0)).astype(F)
        fl = _floor_i(lvl * F(256.0) + F(0.5))
        lo, f = fl >> 8, (fl & 255).astype(F) * F(0.00390625)
        last = lo >= mips - 1
        lo, f = np.where(last, mips - 1, lo), np.where(last, F(0), f).astype(F)
        a0 = level_alpha(tex, lo, u, v)
        a1 = level_alpha(tex, np.minimum(lo + 1, mips - 1), u, v)
        r = np.where(f != 0, fma(f, a1, (F(1.0) - f) * a0), a0).astype(F)
        return (r * RCP255).astype(F)


def sample_alpha_level0(tex, u, v):
    """SampleLevel(LinearSampler, uv, 0).a: the bilinear WRAP fetch of level 0"""
    u, v = np.asarray(u, F), np.asarray(v, F)
    if tex is None or tex["chain"] is None:
        return np.zeros(u.shape, F)
    with np.errstate(all="ignore"):
        return (level_alpha(tex, np.zeros(u.shape, I64), u, v) * RCP255).astype(F)


# ---- M2 --------------------------------------------------------------------------------------------------------------------------------------------------------
def uv_at(clip_xyw, uv, i, j, W, H):
    """clip_xyw float32 [3, 3] (x, y, w per vertex), uv float32 [3, 2]; i, j int arrays (any integers) -> (u, v) float32 arrays: I2 + I3 at the pixel centres"""
    c = clip_xyw.astype(F64)
    X = (2.0 * np.asarray(i, F64) + 1.0) / F64(W) - 1.0
    Y = 1.0 - (2.0 * np.asarray(j, F64) + 1.0) / F64(H)
    with np.errstate(all="ignore"):
        k0, k1, k2 = I.det(X, Y, c[1], c[2]), I.det(X, Y, c[2], c[0]), I.det(X, Y, c[0], c[1])
        den = (k0 + k1) + k2
        l1, l2 = k1 / den, k2 / den
        a = uv.astype(F64)
        return tuple(((a[0, k] + l1 * (a[1, k] - a[0, k])) + l2 * (a[2, k] - a[0, k])).astype(F) for k in range(2))


def scene_discard(mask, clip_xyw, uv, i, j, W, H, probes=None):
    """M3 for the pixels (i, j) (int arrays of one shape) of one primitive: bool array, True = discard"""
    if not has_diffuse_map(mask["texture_config"]):
        return np.zeros(np.shape(i), bool)
    sx, sy, ox, oy = (F(x) for x in mask["scale_offset"])
    with np.errstate(all="ignore"):
        own, hor, ver = uv_at(clip_xyw, uv, i, j, W, H), uv_at(clip_xyw, uv, i ^ 1, j, W, H), uv_at(clip_xyw, uv, i, j ^ 1, W, H)
        t = lambda p: ((p[0] * sx + ox).astype(F), (p[1] * sy + oy).astype(F))      # noqa: E731
        o, h, v = t(own), t(hor), t(ver)
        odd_x, odd_y = (i & 1) == 1, (j & 1) == 1
        ddx = tuple(np.where(odd_x, o[k] - h[k], h[k] - o[k]).astype(F) for k in range(2))
        ddy = tuple(np.where(odd_y, o[k] - v[k], v[k] - o[k]).astype(F) for k in range(2))
        out = sample_alpha(mask["tex"], o[0], o[1], ddx, ddy) < ALPHA_CUT
    if probes is not None:
        probes.append({"mask": mask, "i": np.array(i), "j": np.array(j), "own": own, "hor": hor, "ver": ver, "discard": out.copy()})
    return out


def shadow_discard(mask, clip_xyw, uv, i, j, dim, probes=None):
    """M4 for the texels (i, j) of one primitive"""
    u, v = uv_at(clip_xyw, uv, i, j, dim, dim)
    out = sample_alpha_level0(mask["tex"], u, v) < ALPHA_CUT
    if probes is not None:
        probes.append({"mask": mask, "i": np.array(i), "j": np.array(j), "own": (u, v), "discard": out.copy()})
    return out


def new_stats():
    return {"masked_records": 0, "candidates": 0, "discarded": 0}


def _vertex_clip(draw, inst):
    """V1 / R1 of every vertex of a draw under one instance: float32 [V, 4]"""
    P = R.f32(draw["positions"])[:, :3].copy()
    P[:, 1] = P[:, 1] + R.ZERO
    with np.errstate(all="ignore"):
        return R.mul_point(P, R.f32(draw["wvp"])[inst]).astype(F)


def _triangle(draw, inst, tri, cache):
    """(clip x, y, w float32 [3, 3], uv float32 [3, 2]) of the unclipped triangle"""
    key = (id(draw), inst)
    if key not in cache:
        cache[key] = _vertex_clip(draw, inst)
    idx = np.asarray(draw["indices"], dtype=I64).reshape(-1, 3)[tri]
    return cache[key][idx][:, [0, 1, 3]], R.f32(draw["positions"])[idx][:, 9:11]


# ---- vqhip_scene_masked_depth ----------------------------------------------------------------------------------------------------------------------------------------
def owner_of(scene, q):
    """q -> (draw, instance, triangle)"""
    first = 0
    for d in scene["draws"]:
        nt, ni = len(d["indices"]) // 3, np.asarray(d["wvp"]).shape[0]
        if first <= q < first + nt * ni:
            return d, (q - first) // nt, (q - first) % nt
        first += nt * ni
    raise ValueError(q)


def fill_scene(records, scene, stats=None, probes=None):
    """scene_depth_ref.fill with M1 .. M4 in front of the minimum: (depth float32 [H, W, S], primitive uint32 [H, W, S])"""
    W, H, S = int(scene["width"]), int(scene["height"]), int(scene["samples"])
    st = stats if stats is not None else new_stats()
    depth = np.ones((H, W, S), dtype=F)
    prim = np.full((H, W, S), V.NO_PRIMITIVE, dtype=U32)
    ox = np.array(V.SAMPLE_X[S], dtype=I64)[None, None, :]
    oy = np.array(V.SAMPLE_Y[S], dtype=I64)[None, None, :]
    cache, decided = {}, {}
    with np.errstate(all="ignore"):
        for r in range(records["xy"].shape[0]):
            (x0, y0), (x1, y1), (x2, y2) = (int(a) for a in records["xy"][r, 0]), (int(a) for a in records["xy"][r, 1]), (int(a) for a in records["xy"][r, 2])
            i0, i1, j0, j1 = (int(a) for a in records["box"][r])
            px = (256 * np.arange(i0, i1 + 1, dtype=I64))[None, :, None] + ox
            py = (256 * np.arange(j0, j1 + 1, dtype=I64))[:, None, None] + oy
            A = V.edge(x1, y1, x2, y2, x0, y0)
            s = 1 if A > 0 else -1
            E = (V.edge(x1, y1, x2, y2, px, py), V.edge(x2, y2, x0, y0, px, py), V.edge(x0, y0, x1, y1, px, py))
            ends = (((x1, y1), (x2, y2)), ((x2, y2), (x0, y0)), ((x0, y0), (x1, y1)))
            inside = np.ones(E[0].shape, dtype=bool)
            for e, ((xa, ya), (xb, yb)) in zip(E, ends):
                dx, dy = s * (xb - xa), s * (yb - ya)
                top_left = dy < 0 or (dy == 0 and dx > 0)
                inside &= (s * e > 0) | ((e == 0) & top_left)
            if not inside.any():
                continue
            fA = F(A)
            b1, b2 = E[1].astype(F) / fA, E[2].astype(F) / fA
            zw = records["clip_zw"][r]
            z0, z1, z2 = zw[0, 0] / zw[0, 1], zw[1, 0] / zw[1, 1], zw[2, 0] / zw[2, 1]
            d = V.saturate((z0 + b1 * (z1 - z0)) + b2 * (z2 - z0)).astype(F)
            q = int(records["q"][r])
            live = inside & (d < F(1))
            draw, inst, tri = owner_of(scene, q)
            if draw.get("mask") is not None and live.any():
                st["masked_records"] += 1
                pix = live.any(axis=2)                                  # M1: the pixels with a candidate sample
                jj, ii = np.nonzero(pix)
                jj, ii = jj + j0, ii + i0
                # the decision is a function of (q, pixel): fan pieces of one clipped triangle that meet in a pixel reuse it (and must, for the statistics)
                new = [k for k in range(len(ii)) if (q, int(ii[k]), int(jj[k])) not in decided]
                if new:
                    clip_xyw, uv = _triangle(draw, inst, tri, cache)
                    out = scene_discard(draw["mask"], clip_xyw, uv, ii[new], jj[new], W, H, probes)
                    for k, o in zip(new, out):
                        decided[(q, int(ii[k]), int(jj[k]))] = bool(o)
                    st["candidates"] += len(new)
                    st["discarded"] += int(out.sum())
                gone = np.zeros(pix.shape, bool)
                gone[jj - j0, ii - i0] = [decided[(q, int(a), int(b))] for a, b in zip(ii, jj)]
                live &= ~gone[:, :, None]
            sub_d, sub_q = depth[j0:j1 + 1, i0:i1 + 1], prim[j0:j1 + 1, i0:i1 + 1]
            win = live & ((d < sub_d) | ((d == sub_d) & (U32(q) < sub_q)))
            depth[j0:j1 + 1, i0:i1 + 1] = np.where(win, d, sub_d)
            prim[j0:j1 + 1, i0:i1 + 1] = np.where(win, U32(q), sub_q)
    return depth, prim


def rasterize_scene(scene, stats=None, layers=None, probes=None):
    """vqhip_scene_masked_depth: the dict of scene_depth_ref.rasterize"""
    depth, prim = fill_scene(V.setup(scene), scene, stats, probes)
    if int(scene["samples"]) == 1:
        return {"depth": depth[:, :, 0].copy(), "primitive": prim[:, :, 0].copy()}
    cov, lp = V.layers_of(prim, 4 if layers is None else layers)
    return {"depth": depth, "primitive": prim, "coverage": cov, "layer_primitive": lp}


# ---- vqhip_shadow_masked_depth ---------------------------------------------------------------------------------------------------------------------------------------
def setup_shadow_view(view):
    """shadow_raster_ref.setup_view, one (draw, instance, triangle) at a time so that every record knows its primitive: (records, owner list of (draw, inst, tri))"""
    parts, owners = [], []
    for draw in view["draws"]:
        idx = np.asarray(draw["indices"], dtype=I64).reshape(-1, 3)
        wvp = R.f32(draw["wvp"])
        for inst in range(wvp.shape[0]):
            for t in range(idx.shape[0]):
                one = dict(draw, indices=idx[t], wvp=wvp[inst:inst + 1], world=(R.f32(draw["world"])[inst:inst + 1] if draw.get("world") is not None else None))
                rec = R.setup_view(dict(view, draws=[one]))
                parts.append(rec)
                owners += [(draw, inst, t)] * rec["xy"].shape[0]
    keys = ("xy", "clip_zw", "world", "box")
    if not parts:
        return R.setup_view(dict(view, draws=[])), owners
    return {k: np.concatenate([p[k] for p in parts], axis=0) for k in keys}, owners


def fill_shadow_view(records, owners, view, stats=None, probes=None):
    """shadow_raster_ref.fill_view with M1, M2, M4 in front of the minimum"""
    dim, lin = int(view["dim"]), bool(view["linear"])
    st = stats if stats is not None else new_stats()
    depth = np.ones((dim, dim), dtype=F)
    cam = np.asarray(view.get("camera", (0, 0, 0)), dtype=F)
    far = F(view.get("far", 1.0))
    cache, decided = {}, {}
    with np.errstate(all="ignore"):
        for r in range(records["xy"].shape[0]):
            (x0, y0), (x1, y1), (x2, y2) = (int(a) for a in records["xy"][r, 0]), (int(a) for a in records["xy"][r, 1]), (int(a) for a in records["xy"][r, 2])
            i0, i1, j0, j1 = (int(a) for a in records["box"][r])
            px = (256 * np.arange(i0, i1 + 1, dtype=I64) + 128)[None, :]
            py = (256 * np.arange(j0, j1 + 1, dtype=I64) + 128)[:, None]
            A = R.edge(x1, y1, x2, y2, x0, y0)
            s = 1 if A > 0 else -1
            E = (R.edge(x1, y1, x2, y2, px, py), R.edge(x2, y2, x0, y0, px, py), R.edge(x0, y0, x1, y1, px, py))
            ends = (((x1, y1), (x2, y2)), ((x2, y2), (x0, y0)), ((x0, y0), (x1, y1)))
            inside = np.ones(E[0].shape, dtype=bool)
            for e, ((xa, ya), (xb, yb)) in zip(E, ends):
                dx, dy = s * (xb - xa), s * (yb - ya)
                top_left = dy < 0 or (dy == 0 and dx > 0)
                inside &= (s * e > 0) | ((e == 0) & top_left)
            if not inside.any():
                continue
            draw, inst, tri = owners[r]
            if draw.get("mask") is not None:
                st["masked_records"] += 1
                jj, ii = np.nonzero(inside)
                jj, ii = jj + j0, ii + i0
                key = (id(draw), inst, tri)
                new = [k for k in range(len(ii)) if (key, int(ii[k]), int(jj[k])) not in decided]
                if new:
                    clip_xyw, uv = _triangle(draw, inst, tri, cache)
                    out = shadow_discard(draw["mask"], clip_xyw, uv, ii[new], jj[new], dim, probes)
                    for k, o in zip(new, out):
                        decided[(key, int(ii[k]), int(jj[k]))] = bool(o)
                    st["candidates"] += len(new)
                    st["discarded"] += int(out.sum())
                gone = np.zeros(inside.shape, bool)
                gone[jj - j0, ii - i0] = [decided[(key, int(a), int(b))] for a, b in zip(ii, jj)]
                inside &= ~gone
            fA = F(A)
            b0, b1, b2 = E[0].astype(F) / fA, E[1].astype(F) / fA, E[2].astype(F) / fA
            zw = records["clip_zw"][r]
            if not lin:
                z0, z1, z2 = zw[0, 0] / zw[0, 1], zw[1, 0] / zw[1, 1], zw[2, 0] / zw[2, 1]
                d = (z0 + b1 * (z1 - z0)) + b2 * (z2 - z0)
            else:
                rw0, rw1, rw2 = F(1) / zw[0, 1], F(1) / zw[1, 1], F(1) / zw[2, 1]
                k0, k1, k2 = b0 * rw0, b1 * rw1, b2 * rw2
                den = (k0 + k1) + k2
                Pw = records["world"][r]
                c = [((k0 * Pw[0, a] + k1 * Pw[1, a]) + k2 * Pw[2, a]) / den for a in range(3)]
                e = [cam[a] - c[a] for a in range(3)]
                d = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) / far
            d = R.saturate(d).astype(F)
            sub = depth[j0:j1 + 1, i0:i1 + 1]
            depth[j0:j1 + 1, i0:i1 + 1] = np.where(inside & (d < sub), d, sub)
    return depth


def rasterize_shadow(views, stats=None, probes=None):
    """vqhip_shadow_masked_depth: the maps of all views (float32 [dim, dim] each)"""
    out = []
    for v in views:
        rec, owners = setup_shadow_view(v)
        out.append(fill_shadow_view(rec, owners, v, stats, probes))
    return out
