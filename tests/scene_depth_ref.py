"""docs/DESIGN_DETAILS.md §7.17 (the contract V1 .. V5 of vqhip_scene_depth, and its layer rule) stated in numpy: binary32 arithmetic with every operation rounded,
int64 edge functions, one unsigned 64-bit minimum per sample. Vectorised over vertices and over the samples of a record's box; the clipper runs per triangle,
and only for triangles that leave a plane. What §7.17 takes over from §7.16 unchanged is imported from tests/shadow_raster_ref.py (the vertex stage's product,
saturate, the edge function, the new vertex of a cut edge). tests/test_scene_depth_cpu.py pins this file with a per-triangle, per-sample scalar transcription.

A scene is a dict: width, height, samples (1 | 4), draws = [dict(positions float32 [V, >= 3], indices int [3 T], wvp float32 [n, 4, 4], cull 0 | 1 | 2)]."""
import numpy as np

from tests.shadow_raster_ref import CULL_BACK, CULL_FRONT, CULL_NONE, F, I64, ONE, SNAP_LIMIT, W_MIN, ZERO, clip_vertex, edge, f32, mul_point, saturate  # noqa: F401

U32, U64 = np.uint32, np.uint64
MAX_POLY = 10                                  # 3 + 7 planes
FAN_MAX = 8
NO_PRIMITIVE = 0xFFFFFFFF
CLEAR_KEY = (0x3F800000 << 32) | NO_PRIMITIVE
SAMPLE_X = {1: (128,), 4: (96, 224, 32, 160)}    # 1/256 of a pixel from the pixel's corner: D3D's standard 4x pattern (-2, -6), (6, -2), (-6, 2), (2, 6) sixteenths
SAMPLE_Y = {1: (128,), 4: (32, 96, 160, 224)}


def plane_dist(v, plane):
    """V2: the seven signed distances, in order. v [..., 4] = clip xyzw."""
    x, y, z, w = v[..., 0], v[..., 1], v[..., 2], v[..., 3]
    return (w - W_MIN, w + x, w - x, w + y, w - y, z, w - z)[plane]


def clip_polygon(tri):
    """Sutherland-Hodgman of one triangle [3, 4] against the seven planes in order. Returns (polygon [n, 4] with n in {0, 3 .. 10}, the planes that cut it)."""
    poly = [tri[0], tri[1], tri[2]]
    cut = []
    for plane in range(7):
        d = [plane_dist(v, plane) for v in poly]
        inside = [bool(x >= ZERO) for x in d]
        if all(inside):
            continue
        if not any(inside):
            return np.zeros((0, 4), dtype=F), cut
        cut.append(plane)
        out = []
        n = len(poly)
        for i in range(n):
            j = (i + 1) % n
            if inside[i]:
                out.append(poly[i])
                if not inside[j]:
                    out.append(clip_vertex(poly[i], poly[j], d[i], d[j]))
            elif inside[j]:
                out.append(clip_vertex(poly[j], poly[i], d[j], d[i]))
        poly = out[:MAX_POLY]                      # vertices beyond the tenth are discarded (rounding can break convexity)
    if len(poly) < 3:
        return np.zeros((0, 4), dtype=F), cut
    return np.stack(poly).astype(F), cut


def snap(clip_xyw, width, height):
    """V3: viewport {0, 0, W, H} and the 16.8 snap of R3. Returns (xy int64 [..., 2], ok [...])."""
    half_w, half_h = F(0.5) * F(width), F(0.5) * F(height)
    nx = clip_xyw[..., 0] / clip_xyw[..., 2]
    ny = clip_xyw[..., 1] / clip_xyw[..., 2]
    fx = ((nx + ONE) * half_w) * F(256.0)
    fy = ((ONE - ny) * half_h) * F(256.0)
    ok = (np.abs(fx) <= SNAP_LIMIT) & (np.abs(fy) <= SNAP_LIMIT)
    sx = np.where(ok, np.rint(fx), ZERO).astype(I64)
    sy = np.where(ok, np.rint(fy), ZERO).astype(I64)
    return np.stack([sx, sy], axis=-1), ok


def pixel_range(lo, hi, samples, size):
    """the pixels of one axis that hold a sample coordinate in [lo, hi], clamped to the target (both axes use the offsets {128} or {32 .. 224})"""
    first, last = (128, 128) if samples == 1 else (224, 32)
    return max(-((first - lo) // 256), 0), min((hi - last) // 256, size - 1)


def new_stats():
    return {"triangles": 0, "untouched": 0, "clipped": [0] * 8, "cut_by_plane": [0] * 7, "clipped_away": 0, "nonfinite": 0, "bad_index": 0, "culled": 0,
            "zero_area": 0, "unsnappable": 0, "no_sample": 0, "records": 0, "max_fan": 0}


def instanced_triangles(scene):
    return sum((len(d["indices"]) // 3) * np.asarray(d["wvp"]).shape[0] for d in scene["draws"])


def setup(scene, stats=None):
    """V1 .. V4's setup of every draw. Returns the records: xy int64 [R, 3, 2], clip_zw float32 [R, 3, 2], q uint32 [R], box int64 [R, 4] = i0, i1, j0, j1."""
    W, H, S = int(scene["width"]), int(scene["height"]), int(scene["samples"])
    st = stats if stats is not None else new_stats()
    out_xy, out_zw, out_q, out_box = [], [], [], []
    first = 0
    with np.errstate(all="ignore"):
        for draw in scene["draws"]:
            pos = f32(draw["positions"])[:, :3]
            idx = np.asarray(draw["indices"], dtype=I64).reshape(-1, 3)
            wvp = f32(draw["wvp"])
            cull = int(draw["cull"])
            P = pos.copy()
            P[:, 1] = P[:, 1] + ZERO                                   # the null heightmap
            for inst in range(wvp.shape[0]):
                clip = mul_point(P, wvp[inst]).astype(F)
                st["triangles"] += idx.shape[0]
                index_ok = np.all((idx >= 0) & (idx < P.shape[0]), axis=1)
                st["bad_index"] += int(np.sum(~index_ok))
                tri = clip[np.where(index_ok[:, None], idx, 0)]        # [T, 3, 4]
                finite = np.all(np.isfinite(tri), axis=(1, 2)) & index_ok
                st["nonfinite"] += int(np.sum(index_ok & ~finite))
                dists = np.stack([plane_dist(tri, p) for p in range(7)], axis=-1)          # [T, 3, 7]
                inside_all = np.all(dists >= ZERO, axis=(1, 2)) & finite
                for t in np.nonzero(finite)[0]:
                    if inside_all[t]:
                        st["untouched"] += 1
                        poly = tri[t]
                    else:
                        poly, cut = clip_polygon(tri[t])
                        for p in cut:
                            st["cut_by_plane"][p] += 1
                        if poly.shape[0] == 0:
                            st["clipped_away"] += 1
                            continue
                        st["clipped"][len(cut)] += 1
                    q = first + inst * idx.shape[0] + int(t)
                    xy, ok = snap(poly[:, [0, 1, 3]], W, H)
                    st["max_fan"] = max(st["max_fan"], poly.shape[0] - 2)
                    for k in range(poly.shape[0] - 2):
                        sel = [0, k + 1, k + 2]
                        if not (ok[0] and ok[k + 1] and ok[k + 2]):
                            st["unsnappable"] += 1
                            continue
                        (x0, y0), (x1, y1), (x2, y2) = (int(a) for a in xy[0]), (int(a) for a in xy[k + 1]), (int(a) for a in xy[k + 2])
                        A = edge(x1, y1, x2, y2, x0, y0)
                        if A == 0:
                            st["zero_area"] += 1
                            continue
                        if (A > 0 and cull == CULL_FRONT) or (A < 0 and cull == CULL_BACK):
                            st["culled"] += 1
                            continue
                        i0, i1 = pixel_range(min(x0, x1, x2), max(x0, x1, x2), S, W)
                        j0, j1 = pixel_range(min(y0, y1, y2), max(y0, y1, y2), S, H)
                        if i0 > i1 or j0 > j1:
                            st["no_sample"] += 1
                            continue
                        st["records"] += 1
                        out_xy.append(xy[sel])
                        out_zw.append(poly[sel][:, [2, 3]])
                        out_q.append(q)
                        out_box.append((i0, i1, j0, j1))
            first += idx.shape[0] * wvp.shape[0]
    n = len(out_xy)
    return {"xy": np.array(out_xy, dtype=I64).reshape(n, 3, 2), "clip_zw": np.array(out_zw, dtype=F).reshape(n, 3, 2), "q": np.array(out_q, dtype=U32),
            "box": np.array(out_box, dtype=I64).reshape(n, 4)}


def fill(records, scene, coverage_count=False, dtype=F):
    """V4, V5 over the records. Returns (depth [H, W, S] of `dtype`, primitive uint32 [H, W, S]), or with coverage_count the fragments per sample (int32 [H, W, S],
    fragments at depth 1.0 included: coverage is V4's alone). dtype = np.float64 evaluates V5 in binary64 on the same snapped vertices: the depth test is then
    (depth, q) in lexicographic order on the binary64 values."""
    W, H, S = int(scene["width"]), int(scene["height"]), int(scene["samples"])
    T = dtype
    depth = np.ones((H, W, S), dtype=T)
    prim = np.full((H, W, S), NO_PRIMITIVE, dtype=U32)
    count = np.zeros((H, W, S), dtype=np.int32)
    ox = np.array(SAMPLE_X[S], dtype=I64)[None, None, :]
    oy = np.array(SAMPLE_Y[S], dtype=I64)[None, None, :]
    with np.errstate(all="ignore"):
        for r in range(records["xy"].shape[0]):
            (x0, y0), (x1, y1), (x2, y2) = (int(a) for a in records["xy"][r, 0]), (int(a) for a in records["xy"][r, 1]), (int(a) for a in records["xy"][r, 2])
            i0, i1, j0, j1 = (int(a) for a in records["box"][r])
            px = (256 * np.arange(i0, i1 + 1, dtype=I64))[None, :, None] + ox
            py = (256 * np.arange(j0, j1 + 1, dtype=I64))[:, None, None] + oy
            A = edge(x1, y1, x2, y2, x0, y0)
            s = 1 if A > 0 else -1
            E = (edge(x1, y1, x2, y2, px, py), edge(x2, y2, x0, y0, px, py), edge(x0, y0, x1, y1, px, py))
            ends = (((x1, y1), (x2, y2)), ((x2, y2), (x0, y0)), ((x0, y0), (x1, y1)))
            inside = np.ones(E[0].shape, dtype=bool)
            for e, ((xa, ya), (xb, yb)) in zip(E, ends):
                dx, dy = s * (xb - xa), s * (yb - ya)
                top_left = dy < 0 or (dy == 0 and dx > 0)
                inside &= (s * e > 0) | ((e == 0) & top_left)
            if not inside.any():
                continue
            if coverage_count:
                count[j0:j1 + 1, i0:i1 + 1] += inside
                continue
            fA = T(F(A)) if T is F else T(A)
            conv = (lambda e: e.astype(F)) if T is F else (lambda e: e.astype(np.float64))
            b1, b2 = conv(E[1]) / fA, conv(E[2]) / fA
            zw = records["clip_zw"][r].astype(T)
            z0, z1, z2 = zw[0, 0] / zw[0, 1], zw[1, 0] / zw[1, 1], zw[2, 0] / zw[2, 1]
            d = saturate((z0 + b1 * (z1 - z0)) + b2 * (z2 - z0)).astype(T)
            q = U32(records["q"][r])
            sub_d, sub_q = depth[j0:j1 + 1, i0:i1 + 1], prim[j0:j1 + 1, i0:i1 + 1]
            # one minimum over (depth, q): for d >= +0 the order of the bits is the order of the values, and a fragment at 1.0 never beats the clear key
            win = inside & (d < T(1)) & ((d < sub_d) | ((d == sub_d) & (q < sub_q)))
            depth[j0:j1 + 1, i0:i1 + 1] = np.where(win, d, sub_d)
            prim[j0:j1 + 1, i0:i1 + 1] = np.where(win, q, sub_q)
    return count if coverage_count else (depth, prim)


def layers_of(prim, layers=4):
    """the layer rule: (coverage uint8 [layers, H, W], layerPrimitive uint32 [layers, H, W]) from primitive uint32 [H, W, 4]"""
    H, W, _ = prim.shape
    lp = np.full((4, H, W), NO_PRIMITIVE, dtype=U32)
    mask = np.zeros((4, H, W), dtype=np.uint8)
    opened = np.zeros((H, W), dtype=np.int64)
    for s in range(4):
        o = prim[:, :, s]
        owned = o != NO_PRIMITIVE
        placed = np.zeros((H, W), dtype=bool)
        for k in range(4):
            hit = owned & ~placed & (k < opened) & (lp[k] == o)
            mask[k] |= np.where(hit, np.uint8(1 << s), np.uint8(0))
            placed |= hit
        fresh = owned & ~placed
        for k in range(4):
            here = fresh & (opened == k)
            lp[k] = np.where(here, o, lp[k])
            mask[k] |= np.where(here, np.uint8(1 << s), np.uint8(0))
        opened = opened + fresh
    return mask[:layers].copy(), lp[:layers].copy()


def rasterize(scene, stats=None, layers=None, dtype=F):
    """vqhip_scene_depth: dict(depth float32 [H, W] | [H, W, 4], primitive uint32 of that shape, and at 4 samples coverage uint8 [L, H, W] and layer_primitive
    uint32 [L, H, W] for L = layers (default 4))"""
    depth, prim = fill(setup(scene, stats), scene, dtype=dtype)
    if int(scene["samples"]) == 1:
        return {"depth": depth[:, :, 0].copy(), "primitive": prim[:, :, 0].copy()}
    cov, lp = layers_of(prim, 4 if layers is None else layers)
    return {"depth": depth, "primitive": prim, "coverage": cov, "layer_primitive": lp}
