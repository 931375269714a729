"""docs/DESIGN_DETAILS.md §7.16 (the rasterisation contract R1 .. R6 of vqhip_shadow_depth) stated in numpy: binary32 arithmetic with every operation rounded,
int64 edge functions. Vectorised over vertices and over the texels of a record's box; the clipper runs per triangle, and only for triangles that leave a plane.
tests/test_shadow_raster_cpu.py pins it with a per-triangle, per-texel scalar transcription.

A view is a dict: dim, linear (bool), camera (3 floats), far, draws = [dict(positions float32 [V, >= 3], indices int [3 T], wvp float32 [n, 4, 4],
world float32 [n, 4, 4] | None, cull 0 | 1 | 2)]."""
import numpy as np

F = np.float32
I64 = np.int64
CULL_NONE, CULL_FRONT, CULL_BACK = 0, 1, 2
W_MIN = F(2.0 ** -24)
SNAP_LIMIT = F(2.0 ** 24)
MAX_POLY = 8
ONE, ZERO = F(1.0), F(0.0)


def f32(x):
    return np.asarray(x, dtype=F)


def mul_point(P, M):
    """R1: HLSL mul(M, float4(P, 1)) == row vector [P, 1] * M_cpu, the four terms summed left to right. P [..., 3], M [4, 4] -> [..., 4]."""
    x, y, z = P[..., 0:1], P[..., 1:2], P[..., 2:3]
    return ((x * M[0] + y * M[1]) + z * M[2]) + ONE * M[3]


def saturate(x):
    """the contract's saturate: NaN -> 0, -0 -> +0"""
    x = np.asarray(x)
    one, zero = x.dtype.type(1), x.dtype.type(0)
    return np.where(x > zero, np.where(x < one, x, one), zero)


def plane_dist(v, plane):
    """R2: the signed distance whose sign is the inside test (>= 0) and whose values weight the new vertex. v [..., 7] = clip xyzw, world xyz."""
    x, y, w = v[..., 0], v[..., 1], v[..., 3]
    return (w - W_MIN, w + x, w - x, w + y, w - y)[plane]


def clip_vertex(I, O, dI, dO):
    """from the inside endpoint I towards the outside endpoint O (all seven components)"""
    t = dI / (dI - dO)
    return I + t * (O - I)


def clip_polygon(tri):
    """Sutherland-Hodgman of one triangle [3, 7] against the five planes in order. Returns (polygon [n, 7] with n in {0, 3 .. 8}, planes that cut it)."""
    poly = [tri[0], tri[1], tri[2]]
    cut = 0
    for plane in range(5):
        d = [plane_dist(v, plane) for v in poly]
        inside = [bool(x >= ZERO) for x in d]
        if all(inside):
            continue
        if not any(inside):
            return np.zeros((0, 7), dtype=F), cut
        cut += 1
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
        poly = out[:MAX_POLY]                      # vertices beyond the eighth are discarded (rounding can break convexity)
    if len(poly) < 3:
        return np.zeros((0, 7), dtype=F), cut
    return np.stack(poly).astype(F), cut


def snap(clip_xyw, dim):
    """R3: viewport {0, 0, dim, dim} and the 16.8 snap. Returns (xy int64 [..., 2], ok [...]): ok is False where p * 256 is NaN or beyond 2^24 in magnitude."""
    half = F(0.5) * F(dim)
    nx = clip_xyw[..., 0] / clip_xyw[..., 2]
    ny = clip_xyw[..., 1] / clip_xyw[..., 2]
    fx = ((nx + ONE) * half) * F(256.0)
    fy = ((ONE - ny) * half) * F(256.0)
    ok = (np.abs(fx) <= SNAP_LIMIT) & (np.abs(fy) <= SNAP_LIMIT)
    sx = np.where(ok, np.rint(fx), ZERO).astype(I64)
    sy = np.where(ok, np.rint(fy), ZERO).astype(I64)
    return np.stack([sx, sy], axis=-1), ok


def edge(xj, yj, xk, yk, px, py):
    return (xj - px) * (yk - py) - (xk - px) * (yj - py)


def new_stats():
    return {"triangles": 0, "untouched": 0, "clipped": [0, 0, 0, 0, 0, 0], "clipped_away": 0, "nonfinite": 0, "bad_index": 0,
            "culled": 0, "zero_area": 0, "unsnappable": 0, "no_sample": 0, "records": 0}


def setup_view(view, stats=None):
    """R1 .. R4's setup of every draw of a view. Returns the records as a dict of arrays: xy int64 [R, 3, 2], clip_zw float32 [R, 3, 2], world float32 [R, 3, 3],
    box int64 [R, 4] = i0, i1, j0, j1 (texels, inclusive, clamped to the map)."""
    dim, lin = int(view["dim"]), bool(view["linear"])
    st = stats if stats is not None else new_stats()
    out_xy, out_zw, out_world, out_box = [], [], [], []
    with np.errstate(all="ignore"):
        for draw in view["draws"]:
            pos = f32(draw["positions"])[:, :3]
            idx = np.asarray(draw["indices"], dtype=I64).reshape(-1, 3)
            wvp, world = f32(draw["wvp"]), (f32(draw["world"]) if draw.get("world") is not None else None)
            cull = int(draw["cull"])
            P = pos.copy()
            P[:, 1] = P[:, 1] + ZERO                                   # the null heightmap
            for inst in range(wvp.shape[0]):
                clip = mul_point(P, wvp[inst])
                wpos = mul_point(P, world[inst])[:, :3] if lin else np.zeros((P.shape[0], 3), dtype=F)
                verts = np.concatenate([clip, wpos], axis=1).astype(F)
                st["triangles"] += idx.shape[0]
                index_ok = np.all((idx >= 0) & (idx < P.shape[0]), axis=1)
                st["bad_index"] += int(np.sum(~index_ok))
                tri = verts[np.where(index_ok[:, None], idx, 0)]       # [T, 3, 7]
                finite = np.all(np.isfinite(tri[:, :, :4]), axis=(1, 2)) & index_ok
                st["nonfinite"] += int(np.sum(index_ok & ~finite))
                dists = np.stack([plane_dist(tri, p) for p in range(5)], axis=-1)          # [T, 3, 5]
                inside_all = np.all(dists >= ZERO, axis=(1, 2)) & finite
                polys = []
                for t in np.nonzero(finite)[0]:
                    if inside_all[t]:
                        st["untouched"] += 1
                        polys.append(tri[t])
                        continue
                    poly, cut = clip_polygon(tri[t])
                    if poly.shape[0] == 0:
                        st["clipped_away"] += 1
                        continue
                    st["clipped"][cut] += 1
                    polys.append(poly)
                for poly in polys:
                    xy, ok = snap(poly[:, [0, 1, 3]], dim)
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
                        xs, ys = (x0, x1, x2), (y0, y1, y2)
                        i0, i1 = max(-((128 - min(xs)) // 256), 0), min((max(xs) - 128) // 256, dim - 1)      # ceil((min - 128) / 256), floor((max - 128) / 256)
                        j0, j1 = max(-((128 - min(ys)) // 256), 0), min((max(ys) - 128) // 256, dim - 1)
                        if i0 > i1 or j0 > j1:
                            st["no_sample"] += 1
                            continue
                        st["records"] += 1
                        out_xy.append(xy[sel])
                        out_zw.append(poly[sel][:, [2, 3]])
                        out_world.append(poly[sel][:, 4:7])
                        out_box.append((i0, i1, j0, j1))
    n = len(out_xy)
    return {"xy": np.array(out_xy, dtype=I64).reshape(n, 3, 2), "clip_zw": np.array(out_zw, dtype=F).reshape(n, 3, 2),
            "world": np.array(out_world, dtype=F).reshape(n, 3, 3), "box": np.array(out_box, dtype=I64).reshape(n, 4)}


def fill_view(records, view, coverage_count=False, dtype=F):
    """R4 .. R6 over the records of a view: the dim x dim map (float32; `dtype` = np.float64 evaluates R5 / R6 in binary64 on the same snapped vertices and
    returns float64), or with coverage_count the number of fragments per texel (int32)."""
    dim, lin = int(view["dim"]), bool(view["linear"])
    T = dtype
    depth = np.ones((dim, dim), dtype=T)
    count = np.zeros((dim, dim), dtype=np.int32)
    cam = np.asarray(view.get("camera", (0, 0, 0)), dtype=F).astype(T)
    far = T(F(view.get("far", 1.0)))
    with np.errstate(all="ignore"):
        for r in range(records["xy"].shape[0]):
            (x0, y0), (x1, y1), (x2, y2) = (int(a) for a in records["xy"][r, 0]), (int(a) for a in records["xy"][r, 1]), (int(a) for a in records["xy"][r, 2])
            i0, i1, j0, j1 = (int(a) for a in records["box"][r])
            px = (256 * np.arange(i0, i1 + 1, dtype=I64) + 128)[None, :]
            py = (256 * np.arange(j0, j1 + 1, dtype=I64) + 128)[:, None]
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
            b0, b1, b2 = conv(E[0]) / fA, conv(E[1]) / fA, conv(E[2]) / fA
            zw = records["clip_zw"][r].astype(T)
            if not lin:
                z0, z1, z2 = zw[0, 0] / zw[0, 1], zw[1, 0] / zw[1, 1], zw[2, 0] / zw[2, 1]
                d = (z0 + b1 * (z1 - z0)) + b2 * (z2 - z0)
            else:
                rw0, rw1, rw2 = T(1) / zw[0, 1], T(1) / zw[1, 1], T(1) / zw[2, 1]
                k0, k1, k2 = b0 * rw0, b1 * rw1, b2 * rw2
                den = (k0 + k1) + k2
                Pw = records["world"][r].astype(T)
                c = [((k0 * Pw[0, a] + k1 * Pw[1, a]) + k2 * Pw[2, a]) / den for a in range(3)]
                e = [cam[a] - c[a] for a in range(3)]
                d = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) / far
            d = saturate(d).astype(T)
            sub = depth[j0:j1 + 1, i0:i1 + 1]
            depth[j0:j1 + 1, i0:i1 + 1] = np.where(inside & (d < sub), d, sub)
    return count if coverage_count else depth


def rasterize_view(view, coverage_count=False, stats=None, dtype=F):
    return fill_view(setup_view(view, stats), view, coverage_count, dtype)


def rasterize(views, stats=None):
    """vqhip_shadow_depth: the maps of all views (float32 [dim, dim] each)"""
    return [rasterize_view(v, stats=stats) for v in views]


def instanced_triangles(views):
    return sum((len(d["indices"]) // 3) * np.asarray(d["wvp"]).shape[0] for v in views for d in v["draws"])
