"""docs/DESIGN_DETAILS.md §7.20 (helper-lane uv derivatives for the lit draw) stated in numpy, on top of tests/scene_interp_ref.py (the five planes, §7.18),
tests/masked_depth_ref.py (uv_at: I2 / I3 at any pixel centre, §7.19 M2) and the unchanged oracle of the surface producers (tests/oracle_lib.py).

  Q1  quad_uv(scene, owner): for an owned pixel (i, j) the owner triangle's vertex uv at the centres of (i ^ 1, j) and (i, j ^ 1) — value for value
      masked_depth_ref.uv_at; (0, 0, 0, 0) without an owner; a NaN is 0x7FC00000.
  Q2  the _quad producers = the oracle on an EXPLODED image. A W x H frame becomes 2W x 2H: pixel (i, j) with b = (i & 1, j & 1) sits at (2i + b.x, 2j + b.y)
      with its own record; its horizontal partner in that aligned quad holds the same record with uv (u_h, v_h), its vertical partner the same record with uv
      (u_v, v_v), the diagonal partner index -1; a pixel with no owner contributes four -1 records. The oracle's neighbour rule on that image IS the helper rule
      on the frame: every partner belongs to the own material and lies inside the image. The own positions are read back, the own ip2.w (the discard's -1)
      included. SSAO depends on the pixel position (§7.1: texel (x + 1, y + 1), wrapping): the exploded SSAO plane is built so that the own position fetches
      the texel the original pixel would.
tests/test_quad_interp_cpu.py proves the construction on frames whose every aligned quad has one owner before anything rests on it."""
import numpy as np

from tests import masked_depth_ref as M
from tests import oracle_lib as O
from tests import scene_interp_ref as I

F, U32, I32 = np.float32, np.uint32, np.int32
MINUS_ONE = np.array([-1], dtype=I32).view(F)[0]


# ---- Q1 ----------------------------------------------------------------------------------------------------------------------------------------------------------------
def quad_uv(scene, owner):
    """uint32 bits [H, W, 4] = (u_h, v_h, u_v, v_v): one masked_depth_ref.uv_at call per owner primitive and helper lane, over that primitive's pixels"""
    W, H = int(scene["width"]), int(scene["height"])
    has, attrs, *_ = I.gather(scene, owner)
    out = np.zeros((H, W, 4), dtype=F)
    q = np.asarray(owner).astype(np.int64) & 0xFFFFFFFF
    for prim in np.unique(q[has]):
        m = has & (q == prim)
        jj, ii = np.nonzero(m)
        a = attrs[jj[0], ii[0]]                                     # the owner's three vertices: [3, 19]
        clip_xyw, uv = a[:, [I.CLIP, I.CLIP + 1, I.CLIP + 3]], a[:, 9:11]
        with np.errstate(all="ignore"):
            uh, vh = M.uv_at(clip_xyw, uv, ii ^ 1, jj, W, H)
            uv_, vv = M.uv_at(clip_xyw, uv, ii, jj ^ 1, W, H)
        out[jj, ii] = np.stack([uh, vh, uv_, vv], axis=-1)
    bits = out.view(U32).copy()
    bits[np.isnan(out)] = I.CANONICAL_NAN
    return bits


def interpolate(scene, owner, stats=None):
    """vqhip_scene_quad_interpolants: scene_interp_ref.interpolate's dict + quad_uv. stats also receives the partner classes of the owner plane (classify)."""
    out = I.interpolate(scene, owner, stats=stats)
    out["quad_uv"] = quad_uv(scene, owner)
    if stats is not None:
        stats.update(classify(scene, owner))
    return out


def classify(scene, owner):
    """the classes of quad partners §7.20 distinguishes, as pixel counts over the owned pixels of one owner plane: (a) `same_material`: the horizontal partner has
    another owner of the same material; (b) `other_material`; (c) `partner_unowned`; (d) `outside_x` / `outside_y`: the partner lies outside the image"""
    has, _, mat, *_ = I.gather(scene, owner)
    H, W = has.shape
    q = np.asarray(owner).astype(np.int64) & 0xFFFFFFFF
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ih = ii ^ 1
    inx = ih < W
    ihc = np.minimum(ih, W - 1)
    ph, pq, pm = has[jj, ihc], q[jj, ihc], mat[jj, ihc]
    iny = (jj ^ 1) < H
    return {"same_material": int((has & inx & ph & (pq != q) & (pm == mat)).sum()), "other_material": int((has & inx & ph & (pm != mat)).sum()),
            "partner_unowned": int((has & inx & ~ph).sum()), "outside_x": int((has & ~inx).sum()), "outside_y": int((has & ~iny).sum())}


def neighbour_quad_uv(ip0, ip1):
    """what the neighbour rule reads: the quad partners' stored uv, as bits [H, W, 4] in quad_uv's layout, and the mask of pixels whose two partners lie inside
    the image"""
    u, v = np.ascontiguousarray(ip0[..., 3]).view(U32), np.ascontiguousarray(ip1[..., 3]).view(U32)
    H, W = u.shape
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ok = ((ii ^ 1) < W) & ((jj ^ 1) < H)
    ih, jv = np.minimum(ii ^ 1, W - 1), np.minimum(jj ^ 1, H - 1)
    return np.stack([u[jj, ih], v[jj, ih], u[jv, ii], v[jv, ii]], axis=-1), ok


# ---- Q2 ----------------------------------------------------------------------------------------------------------------------------------------------------------------
def _own(H, W):
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return 2 * jj + (jj & 1), 2 * ii + (ii & 1)


def explode(ip, quv):
    """ip: three float32 [H, W, 4] planes (bits kept); quv: quad_uv as uint32 bits or float32 [H, W, 4] -> three float32 [2H, 2W, 4] planes"""
    ip = [np.ascontiguousarray(p).view(F) if p.dtype != F else np.ascontiguousarray(p) for p in ip]
    quv = np.ascontiguousarray(quv).view(F)
    H, W = ip[0].shape[:2]
    big = [np.zeros((2 * H, 2 * W, 4), dtype=F) for _ in range(3)]
    big[2][..., 3] = MINUS_ONE
    idx = ip[2][..., 3].view(I32)
    owned = idx >= 0
    r, c = _own(H, W)
    for rr, cc, uv in ((r, c, None), (r, c ^ 1, (quv[..., 0], quv[..., 1])), (r ^ 1, c, (quv[..., 2], quv[..., 3]))):
        for k in range(3):
            big[k][rr[owned], cc[owned]] = ip[k][owned]
        if uv is not None:
            big[0][rr[owned], cc[owned], 3] = uv[0][owned]
            big[1][rr[owned], cc[owned], 3] = uv[1][owned]
    return big


def explode_ssao(ssao):
    """uint8 [H, W] -> uint8 [2H, 2W]: ssao'[(2j + b.y + 1) % 2H][(2i + b.x + 1) % 2W] = ssao[(j + 1) % H][(i + 1) % W]; distinct pixels never collide"""
    ssao = np.ascontiguousarray(ssao, dtype=np.uint8)
    H, W = ssao.shape
    r, c = _own(H, W)
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    big = np.zeros((2 * H, 2 * W), dtype=np.uint8)
    big[(r + 1) % (2 * H), (c + 1) % (2 * W)] = ssao[(jj + 1) % H, (ii + 1) % W]
    return big


def gbuffer_from_materials_quad(ip, quv, materials, ambient, ssao=None):
    """vqhip_gbuffer_from_materials_quad: (four float32 [H, W, 4] planes, ip2.w after the call as int32 [H, W] — -1 where the fragment was discarded)"""
    H, W = ip[0].shape[:2]
    big = explode(ip, quv)
    with np.errstate(all="ignore"):
        gb = O.gbuffer_from_materials(big, materials, ambient, explode_ssao(ssao) if ssao is not None else None)
    r, c = _own(H, W)
    return [np.ascontiguousarray(g[r, c]) for g in gb], np.ascontiguousarray(big[2][r, c, 3]).view(I32)


def scene_normals_from_materials_quad(ip, quv, materials, out_fmt):
    """vqhip_scene_normals_from_materials_quad: uint32 [H, W] or float32 [H, W, 4]"""
    H, W = ip[0].shape[:2]
    with np.errstate(all="ignore"):
        out = O.scene_normals_from_materials(explode(ip, quv), materials, out_fmt)
    r, c = _own(H, W)
    return np.ascontiguousarray(out[r, c])
