"""docs/DESIGN_DETAILS.md §7.24 (the contract L1 .. L8 of vqhip_line_draws) stated in numpy on top of tests/scene_depth_ref.py and tests/unlit_ref.py: the
wireframe's vertex stage is U1's (L1: tests/shadow_raster_ref.mul_point on (x, y + 0.0f, z)), the planes, the new vertex of a cut, the viewport and the snap are
§7.17's (L4: plane_dist, clip_vertex, snap — called, not restated), the stored colour is U5's (L7: tests/unlit_ref.opaque_halfs). What this file adds: the lines of
a triangle (L2), VertexDebug.hlsl's three axes per point (L3), the clip of a SEGMENT (L4), the diamond-exit rule as an integer walk over the major axis (L5: python
integers, no floating point), the depth along the major axis (L6) and the largest-q rule (L7, L8). tests/test_line_draws_cpu.py pins the walk with an independent
exact restatement of the diamond as a point set, and L3 with a scalar one-operation-per-line restatement.

A scene is a dict: width, height, depth float32 [H, W] (the scene's depth), draws = a list in submission order of
  dict(kind="wireframe", vertices float32 [V, >= 3], indices int [3 T], matrices float32 [n, 4, 4], color float32 [4])
  dict(kind="axes", vertices float32 [V, >= 9] (position, normal, tangent), indices int [n], cb float32 [52] = one VQ_VertexAxesData)."""
import numpy as np

from tests import scene_depth_ref as V
from tests import unlit_ref as R
from tests.shadow_raster_ref import F, I64, ZERO, clip_vertex, f32, mul_point, saturate

U16, U32 = np.uint16, np.uint32
NO_WRITER = R.NO_WRITER
CB_WORLD, CB_NORMAL, CB_VIEW_PROJ, CB_SIZE = 0, 16, 32, 48          # float offsets into VQ_VertexAxesData
AXIS_COLOURS = ((0.6, 0.0, 0.0, 1.0), (0.0, 0.0, 0.6, 1.0), (0.0, 0.6, 0.0, 1.0))    # L3: emission order — tangent red, cross(N, T) BLUE, normal green
HALF_DIAGONAL = 128


# ---- L5 ------------------------------------------------------------------------------------------------------------------------------------------------------------
def in_diamond(px, py, cx, cy, y_major):
    """is the point in the diamond set of the pixel centred at (cx, cy): the open diamond, its two lower edges and its bottom corner (y grows downwards), and for
    a y-major line its right corner"""
    dx, dy = px - cx, py - cy
    a = abs(dx) + abs(dy)
    return a < HALF_DIAGONAL or (a == HALF_DIAGONAL and (dy > 0 or (y_major and dx == HALF_DIAGONAL)))


def is_y_major(x0, y0, x1, y1):
    return abs(x1 - x0) < abs(y1 - y0)              # a slope of exactly +-1 is x-major


def walk(x0, y0, x1, y1, width=None, height=None):
    """L5 as an integer walk: the pixels the line from (x0, y0) to (x1, y1) (1/256 of a pixel) covers, as (i, j, c) in the order of the steps along the major
    axis, c = the pixel centre on the major axis. One candidate per step: the pixel whose diamond's diagonal across the major axis the extended line crosses,
    256 k < crossing <= 256 k + 256 (the tie goes to the included corner); it is covered iff the closed segment meets its diamond set — the crossing lies on
    the segment, or an end lies in the set — and the END point is not in the set. width, height: clamp to a target."""
    x0, y0, x1, y1 = int(x0), int(y0), int(x1), int(y1)
    if x0 == x1 and y0 == y1:
        return []
    ym = is_y_major(x0, y0, x1, y1)
    m0, n0, m1, n1 = (y0, x0, y1, x1) if ym else (x0, y0, x1, y1)
    size_m, size_n = (height, width) if ym else (width, height)
    s_lo, s_hi = (min(m0, m1) + 255) // 256 - 1, max(m0, m1) // 256      # the steps whose closed diamond [256 s, 256 s + 256] meets the extent
    if size_m is not None:
        s_lo, s_hi = max(s_lo, 0), min(s_hi, size_m - 1)
    dm, dn = m1 - m0, n1 - n0
    out = []
    for s in range(s_lo, s_hi + 1):
        cm = 256 * s + 128
        num, den = n0 * dm + (cm - m0) * dn, dm * 256                     # the extended line at cm: the minor coordinate num / dm
        if den < 0:
            num, den = -num, -den
        k = -((-num) // den) - 1                                          # ceil(num / den) - 1
        if size_n is not None and not 0 <= k < size_n:
            continue
        cn = 256 * k + 128
        cx, cy = (cn, cm) if ym else (cm, cn)
        on_segment = min(m0, m1) <= cm <= max(m0, m1)
        if in_diamond(x1, y1, cx, cy, ym) or not (on_segment or in_diamond(x0, y0, cx, cy, ym)):
            continue
        out.append((cx >> 8, cy >> 8, cm))
    return out


# ---- L1 .. L3: the vertex stages --------------------------------------------------------------------------------------------------------------------------------------
def normalize_lit(v):
    """the contract's normalize as written: one IEEE quotient per component by sqrt((x x + y y) + z z); [..., 3]"""
    v = f32(v)
    with np.errstate(all="ignore"):                                        # a zero vector normalises to NaN: L3 drops its line
        dd = ((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]).astype(F)
        return (v / np.sqrt(dd)[..., None]).astype(F)


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]],
                    axis=-1).astype(F)


def mul_direction(v, M):
    """mul(M, float4(v, 0)).xyz in mulPoint's association"""
    x, y, z = v[..., 0:1], v[..., 1:2], v[..., 2:3]
    return (((x * M[0] + y * M[1]) + z * M[2]) + ZERO * M[3]).astype(F)[..., :3]


def wireframe_ends(draw):
    """L1, L2: (clip float32 [L, 2, 4], live bool [L]) of the draw's lines in q order: instance, triangle, edge; live = the triangle's indices are in range"""
    pos = f32(draw["vertices"])[:, :3]
    idx = np.asarray(draw["indices"], dtype=I64).reshape(-1, 3)
    mats = f32(draw["matrices"]).reshape(-1, 4, 4)
    P = pos.copy()
    P[:, 1] = P[:, 1] + ZERO                                               # the null heightmap
    index_ok = np.all((idx >= 0) & (idx < P.shape[0]), axis=1)
    safe = np.where(index_ok[:, None], idx, 0)
    ends = np.empty((mats.shape[0], idx.shape[0], 3, 2, 4), dtype=F)
    for inst in range(mats.shape[0]):
        clip = mul_point(P, mats[inst]).astype(F) if P.shape[0] else np.zeros((1, 4), dtype=F)
        tri = clip[safe] if P.shape[0] else np.zeros((idx.shape[0], 3, 4), dtype=F)
        for e in range(3):
            ends[inst, :, e, 0], ends[inst, :, e, 1] = tri[:, e], tri[:, (e + 1) % 3]
    live = np.broadcast_to(index_ok[None, :, None], ends.shape[:3])
    return ends.reshape(-1, 2, 4), live.reshape(-1).copy()


def axes_ends(draw):
    """L3: (clip float32 [L, 2, 4], live bool [L]) of the draw's lines in q order: point (one per INDEX), axis"""
    v = f32(draw["vertices"])
    idx = np.asarray(draw["indices"], dtype=I64).reshape(-1)
    cb = f32(draw["cb"]).reshape(-1)
    world, normal, vp = (cb[o:o + 16].reshape(4, 4) for o in (CB_WORLD, CB_NORMAL, CB_VIEW_PROJ))
    size = cb[CB_SIZE]
    ok = (idx >= 0) & (idx < v.shape[0])
    if not v.shape[0]:
        return np.zeros((3 * idx.shape[0], 2, 4), dtype=F), np.zeros(3 * idx.shape[0], dtype=bool)
    pts = v[np.where(ok, idx, 0)]
    p, N, T = pts[:, 0:3], pts[:, 3:6], pts[:, 6:9]
    tbn = (normalize_lit(T), normalize_lit(cross(N, T)), normalize_lit(N))
    P = mul_point(p, world).astype(F)[:, :3]
    start = mul_point(P, vp).astype(F)
    ends = np.empty((idx.shape[0], 3, 2, 4), dtype=F)
    for k in range(3):
        O = (normalize_lit(mul_direction(tbn[k], normal)) * size).astype(F)
        ends[:, k, 0] = start
        ends[:, k, 1] = mul_point((P + O).astype(F), vp).astype(F)
    return ends.reshape(-1, 2, 4), np.repeat(ok, 3)


def clip_segment(a, b, cut=None):
    """L4: the segment against V2's seven planes in order, from the inside end towards the outside end, the direction kept. None: nothing is left.
    cut: a list that receives the planes that cut."""
    for plane in range(7):
        da, db = V.plane_dist(a, plane), V.plane_dist(b, plane)
        ina, inb = bool(da >= ZERO), bool(db >= ZERO)
        if ina and inb:
            continue
        if cut is not None:
            cut.append(plane)
        if not ina and not inb:
            return None
        if ina:
            b = clip_vertex(a, b, da, db).astype(F)
        else:
            a = clip_vertex(b, a, db, da).astype(F)
    return a, b


def new_stats():
    return {"lines": 0, "bad_index": 0, "nonfinite": 0, "cut_by_plane": [0] * 7, "clipped_away": 0, "unsnappable": 0, "zero_length": 0, "records": 0, "fragments": None}


def lines(scene, stats=None):
    """L1 .. L4, L7's numbering. Returns a dict of arrays over the lines that reach the fill: q uint32, draw int64, colour int64 (0 .. 2 within the draw),
    xy int64 [R, 2, 2] (the snapped ends), z float32 [R, 2] (z / w)."""
    W, H = int(scene["width"]), int(scene["height"])
    st = stats if stats is not None else new_stats()
    out = {"q": [], "draw": [], "colour": [], "xy": [], "z": []}
    first = 0
    with np.errstate(all="ignore"):
        for d, draw in enumerate(scene["draws"]):
            axes = draw["kind"] == "axes"
            ends, live = axes_ends(draw) if axes else wireframe_ends(draw)
            L = ends.shape[0]
            st["lines"] += L
            st["bad_index"] += int(np.sum(~live))
            finite = np.all(np.isfinite(ends), axis=(1, 2)) & live
            st["nonfinite"] += int(np.sum(live & ~finite))
            dists = np.stack([V.plane_dist(ends, p) for p in range(7)], axis=-1) if L else np.zeros((0, 2, 7), dtype=F)
            inside = np.all(dists >= ZERO, axis=(1, 2))
            keep = []
            for l in np.nonzero(finite)[0]:
                if not inside[l]:
                    cut = []
                    seg = clip_segment(ends[l, 0], ends[l, 1], cut)
                    for p in cut:
                        st["cut_by_plane"][p] += 1
                    if seg is None:
                        st["clipped_away"] += 1
                        continue
                    ends[l, 0], ends[l, 1] = seg
                keep.append(int(l))
            if keep:
                keep = np.array(keep, dtype=I64)
                e = ends[keep]
                xy, ok = V.snap(e[..., [0, 1, 3]], W, H)
                z = (e[..., 2] / e[..., 3]).astype(F)
                ok = ok.all(axis=1)
                st["unsnappable"] += int(np.sum(~ok))
                zero = ok & np.all(xy[:, 0] == xy[:, 1], axis=1)
                st["zero_length"] += int(np.sum(zero))
                sel = ok & ~zero
                out["q"].append((first + keep[sel]).astype(U32))
                out["draw"].append(np.full(int(sel.sum()), d, dtype=I64))
                out["colour"].append((keep[sel] % 3) if axes else np.zeros(int(sel.sum()), dtype=I64))
                out["xy"].append(xy[sel])
                out["z"].append(z[sel])
            first += L
    cat = lambda k, shape, dt: np.concatenate(out[k]).astype(dt) if out[k] else np.zeros(shape, dtype=dt)
    rec = {"q": cat("q", (0,), U32), "draw": cat("draw", (0,), I64), "colour": cat("colour", (0,), I64), "xy": cat("xy", (0, 2, 2), I64), "z": cat("z", (0, 2), F)}
    st["records"] = int(rec["q"].shape[0])
    rec["total"] = first
    return rec


def total_lines(scene):
    return sum(3 * len(d["indices"]) if d["kind"] == "axes" else len(d["indices"]) * np.asarray(d["matrices"]).reshape(-1, 4, 4).shape[0] for d in scene["draws"])


def draw_colours(draw):
    """L7: the half bits of the draw's colours, uint16 [3, 4] (a wireframe draw uses entry 0)"""
    if draw["kind"] == "axes":
        return np.stack([R.opaque_halfs(c) for c in AXIS_COLOURS])
    return np.stack([R.opaque_halfs(draw["color"])] * 3)


def fragment_depth(c, m0, m1, z0, z1):
    """L6: t = saturate((float)(c - m0) / (float)(m1 - m0)), d = saturate(z0 + t (z1 - z0)); binary32, every operation rounded"""
    with np.errstate(all="ignore"):
        t = saturate(F(F(c - m0) / F(m1 - m0)))
        return F(saturate(F(F(z0) + F(t * F(F(z1) - F(z0))))))


def line_draws(scene, scene_color, stats=None):
    """vqhip_line_draws: dict(scene_color uint16 [H, W, 4] — the half bits of `scene_color` with the covered, passing pixels replaced —, writer uint32 [H, W])"""
    W, H = int(scene["width"]), int(scene["height"])
    depth = f32(scene["depth"]).reshape(H, W)
    st = stats if stats is not None else new_stats()
    rec = lines(scene, st)
    out = np.array(np.ascontiguousarray(scene_color).view(U16), copy=True).reshape(H, W, 4)
    writer = np.full((H, W), NO_WRITER, dtype=U32)
    best = np.full((H, W), -1, dtype=I64)
    count = np.zeros((H, W), dtype=np.int32)
    colours = [draw_colours(d) for d in scene["draws"]]
    for r in range(rec["q"].shape[0]):
        (x0, y0), (x1, y1) = (int(a) for a in rec["xy"][r, 0]), (int(a) for a in rec["xy"][r, 1])
        ym = is_y_major(x0, y0, x1, y1)
        m0, m1 = (y0, y1) if ym else (x0, x1)
        q, d = int(rec["q"][r]), int(rec["draw"][r])
        for (i, j, c) in walk(x0, y0, x1, y1, W, H):
            z = fragment_depth(c, m0, m1, rec["z"][r, 0], rec["z"][r, 1])
            if not z < depth[j, i]:                                        # strictly below, binary32; a NaN in the plane passes nothing
                continue
            count[j, i] += 1
            if q > best[j, i]:                                             # L7: the largest q
                best[j, i] = q
                out[j, i] = colours[d][int(rec["colour"][r])]
                writer[j, i] = d
    st["fragments"] = count
    return {"scene_color": out, "writer": writer}
