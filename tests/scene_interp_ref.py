"""docs/DESIGN_DETAILS.md §7.18 (the contract I0 .. I3 of vqhip_scene_interpolants) stated in numpy: binary32 for the vertex stage (I1), binary64 for the weights
at the pixel centre (I2) and the attributes (I3), every operation rounded once. Vectorised per pixel; the vertex stage runs per (draw, instance) over all vertices.

A scene is scene_depth_ref's dict with more per draw: draws = [dict(positions float32 [V, >= 11] (position 3, normal 3, tangent 3, uv 2), indices int [3 T],
wvp / world / normal / wvp_prev float32 [n, 4, 4], material int)]. The owner plane is uint32 [H, W]: scene_depth_ref's `primitive` at 1 sample, one
`layer_primitive[k]` at 4."""
import numpy as np

from tests.shadow_raster_ref import F, ONE, ZERO, f32, mul_point

U32, F64 = np.uint32, np.float64
NO_PRIMITIVE = 0xFFFFFFFF
CANONICAL_NAN = 0x7FC00000
N_ATTR = 19                                      # world 3, N 3, T 3, uv 2, clip 4, prev 4
CLIP = 11                                        # where clip starts among them


def mul_dir(n, M):
    """I1: mul((float4x3)M, n).xyz under the VQ_matrix convention: (n.x M[0][j] + n.y M[1][j]) + n.z M[2][j], j < 3"""
    x, y, z = n[..., 0:1], n[..., 1:2], n[..., 2:3]
    return ((x * M[0, :3] + y * M[1, :3]) + z * M[2, :3]).astype(F)


def vertex_stage(draw, inst):
    """I1 for every vertex of `draw` under instance `inst`: float32 [V, 19]"""
    v = f32(draw["positions"])
    P = (v[:, 0:3] + ZERO).astype(F)             # the null heightmap: a float3 add, every component loses a -0
    wvp, world, nrm = f32(draw["wvp"])[inst], f32(draw["world"])[inst], f32(draw["normal"])[inst]
    prev = f32(draw["wvp_prev"])[inst] if draw.get("wvp_prev") is not None else np.zeros((4, 4), dtype=F)
    with np.errstate(all="ignore"):
        return np.concatenate([mul_point(P, world)[:, :3], mul_dir(v[:, 3:6], nrm), mul_dir(v[:, 6:9], nrm), v[:, 9:11], mul_point(P, wvp), mul_point(P, prev)],
                              axis=1).astype(F)


def total_triangles(scene):
    return sum((len(d["indices"]) // 3) * np.asarray(d["wvp"]).shape[0] for d in scene["draws"])


def lookup(scene, owner):
    """I0: per pixel (has_owner bool, draw, instance, triangle int64) of the owner plane uint32 [H, W]; index validity included"""
    q = np.asarray(owner).astype(np.int64) & 0xFFFFFFFF
    total = total_triangles(scene)
    has = (q != NO_PRIMITIVE) & (q < total)
    di = np.zeros(q.shape, dtype=np.int64)
    inst = np.zeros(q.shape, dtype=np.int64)
    tri = np.zeros(q.shape, dtype=np.int64)
    first = 0
    for k, d in enumerate(scene["draws"]):
        nt, ni = len(d["indices"]) // 3, np.asarray(d["wvp"]).shape[0]
        if nt == 0:
            continue                             # a draw with no indices owns nothing
        m = has & (q >= first) & (q < first + nt * ni)
        r = np.where(m, q - first, 0)
        di, inst, tri = np.where(m, k, di), np.where(m, r // nt, inst), np.where(m, r % nt, tri)
        idx = np.asarray(d["indices"], dtype=np.int64).reshape(-1, 3)[r % nt]
        bad = m & np.any((idx < 0) | (idx >= np.asarray(d["positions"]).shape[0]), axis=-1)
        has = has & ~bad
        first += nt * ni
    return has, di, inst, tri


def gather(scene, owner):
    """(has_owner [H, W], attrs float32 [H, W, 3, 19] of the owner's three vertices, material int32 [H, W], draw, instance, triangle)"""
    has, di, inst, tri = lookup(scene, owner)
    H, W = has.shape
    attrs = np.zeros((H, W, 3, N_ATTR), dtype=F)
    mat = np.full((H, W), -1, dtype=np.int32)
    for k, d in enumerate(scene["draws"]):
        idx = np.asarray(d["indices"], dtype=np.int64).reshape(-1, 3)
        for i in range(np.asarray(d["wvp"]).shape[0]):
            m = has & (di == k) & (inst == i)
            if not m.any():
                continue
            attrs[m] = vertex_stage(d, i)[idx[tri[m]]]
            mat[m] = int(d["material"])
    return has, attrs, mat, di, inst, tri


def pixel_centres(W, H):
    """I2: X [1, W], Y [H, 1] in binary64: (2 i + 1) / W - 1 and 1 - (2 j + 1) / H, each operation rounded once"""
    X = (2.0 * np.arange(W, dtype=F64) + 1.0) / F64(W) - 1.0
    Y = 1.0 - (2.0 * np.arange(H, dtype=F64) + 1.0) / F64(H)
    return X[None, :], Y[:, None]


def det(X, Y, a, b):
    """I2: D(a, b) with a, b = (x, y, w) [..., 3] in binary64"""
    xa, ya, wa, xb, yb, wb = a[..., 0], a[..., 1], a[..., 2], b[..., 0], b[..., 1], b[..., 2]
    return (X * (ya * wb - wa * yb) - Y * (xa * wb - wa * xb)) + (xa * yb - ya * xb)


def weights(attrs, W, H):
    """I2: (lambda_1, lambda_2, k [3], den) per pixel, binary64"""
    c = attrs[..., [CLIP, CLIP + 1, CLIP + 3]].astype(F64)            # [H, W, 3 vertices, (x, y, w)]
    X, Y = pixel_centres(W, H)
    with np.errstate(all="ignore"):
        k0, k1, k2 = det(X, Y, c[..., 1, :], c[..., 2, :]), det(X, Y, c[..., 2, :], c[..., 0, :]), det(X, Y, c[..., 0, :], c[..., 1, :])
        den = (k0 + k1) + k2
        return k1 / den, k2 / den, (k0, k1, k2), den


def blend(attrs, l1, l2):
    """I3: float32 [..., 19] as uint32 bits, NaN canonical"""
    a = attrs.astype(F64)
    with np.errstate(all="ignore"):
        v = ((a[..., 0, :] + l1[..., None] * (a[..., 1, :] - a[..., 0, :])) + l2[..., None] * (a[..., 2, :] - a[..., 0, :])).astype(F)
    bits = v.view(U32).copy()
    bits[np.isnan(v)] = CANONICAL_NAN
    return bits


def interpolate(scene, owner, stats=None):
    """vqhip_scene_interpolants: dict(ip0, ip1, ip2, sv_curr, sv_prev: uint32 bits [H, W, 4]). stats (a dict) receives the pixel classes of the call."""
    W, H = int(scene["width"]), int(scene["height"])
    has, attrs, mat, di, inst, _ = gather(scene, owner)
    l1, l2, k, den = weights(attrs, W, H)
    b = blend(attrs, l1, l2)
    out = {key: np.zeros((H, W, 4), dtype=U32) for key in ("ip0", "ip1", "ip2", "sv_curr", "sv_prev")}
    out["ip0"][..., :3], out["ip0"][..., 3] = b[..., 0:3], b[..., 9]
    out["ip1"][..., :3], out["ip1"][..., 3] = b[..., 3:6], b[..., 10]
    out["ip2"][..., :3], out["ip2"][..., 3] = b[..., 6:9], mat.view(U32)
    out["sv_curr"][...], out["sv_prev"][...] = b[..., 11:15], b[..., 15:19]
    none = ~has
    for key in ("ip0", "ip1", "ip2"):
        out[key][none] = 0
    out["ip2"][none, 3] = 0xFFFFFFFF
    for key in ("sv_curr", "sv_prev"):
        out[key][none] = (0, 0, 0, 0x3F800000)
    if stats is not None:
        w = attrs[..., CLIP + 3]
        with np.errstate(all="ignore"):
            l0 = k[0] / den
            outside = has & np.all(w > ZERO, axis=-1) & ((l0 < 0) | (l1 < 0) | (l2 < 0))
        stats.update(no_owner=int(none.sum()), owned=int(has.sum()), behind=int((has & np.any(w <= ZERO, axis=-1)).sum()), outside=int(outside.sum()),
                     later_instance=int((has & (inst > 0)).sum()), later_draw=int((has & (di > 0)).sum()), zero_den=int((has & (den == 0)).sum()),
                     masks={"has": has, "behind": has & np.any(w <= ZERO, axis=-1), "outside": outside, "later_instance": has & (inst > 0),
                            "later_draw": has & (di > 0)})
    return out
