"""docs/DESIGN_DETAILS.md §7.21 (the contract O1 .. O6 of vqhip_outline) stated in numpy on top of tests/scene_depth_ref.py and tests/shadow_raster_ref.py: the two
vertex stages (O1, O2) in binary32 with every operation rounded, then — unchanged and therefore imported — §7.17's clipper against seven planes, viewport and
snap, int64 edge functions with the top-left rule and V5's depth (O3); the mark (O4), the last-writer rule and the colour (O5, O6). The contract's as-written
normalize, its pow and the half conversion are the CPU checker's (oracle/: vqo_normalize_lit_array, vqo_pow, vqo_f32_to_f16).
tests/test_outline_cpu.py pins this file with a per-triangle, per-pixel scalar transcription.

A scene is a dict: width, height, draws = [dict(vertices float32 [V, >= 6] (position 3, normal 3), indices int [3 T], cb float32 [92] = one VQ_OutlineData)]."""
import ctypes as C

import numpy as np

from tests import oracle_lib as O
from tests import scene_depth_ref as V
from tests.shadow_raster_ref import F, I64, ZERO, f32, mul_point

U32 = np.uint32
NO_WRITER = 0xFFFFFFFF
HALF = F(0.5)
CB_WORLD_VIEW, CB_NORMAL_VIEW, CB_PROJ, CB_COLOR = 16, 32, 48, 80           # float offsets into VQ_OutlineData


def _lib():
    lib = O.load()
    lib.vqo_normalize_lit_array.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.vqo_normalize_lit_array.restype = None
    lib.vqo_pow.restype = C.c_float
    lib.vqo_pow.argtypes = [C.c_float, C.c_float]
    return lib


def normalize_lit(v):
    """the contract's normalize as written (one IEEE quotient per component by sqrt of the as-written dot), [n, 3] -> [n, 3]"""
    v = np.ascontiguousarray(v, dtype=F).reshape(-1, 3)
    out = np.empty_like(v)
    if v.shape[0]:
        _lib().vqo_normalize_lit_array(v.ctypes.data, out.ctypes.data, v.shape[0])
    return out


def matmul32(A, B):
    """O1: the product of two matrices, (((a0 b0 + a1 b1) + a2 b2) + a3 b3) per element, every operation rounded in binary32"""
    A, B = f32(A).reshape(4, 4), f32(B).reshape(4, 4)
    return (((A[:, 0:1] * B[0] + A[:, 1:2] * B[1]) + A[:, 2:3] * B[2]) + A[:, 3:4] * B[3]).astype(F)


def matrices(cb):
    cb = f32(cb).reshape(-1)
    return (cb[CB_WORLD_VIEW:CB_WORLD_VIEW + 16].reshape(4, 4), cb[CB_NORMAL_VIEW:CB_NORMAL_VIEW + 16].reshape(4, 4), cb[CB_PROJ:CB_PROJ + 16].reshape(4, 4))


def vertex_stages(draw):
    """(clip0 [V, 4], clip1 [V, 4]): O1 and O2 of every vertex of the draw"""
    v = f32(draw["vertices"])
    WV, NV, Pr = matrices(draw["cb"])
    with np.errstate(all="ignore"):
        P = v[:, :3].copy()
        P[:, 1] = P[:, 1] + ZERO                                                  # the null heightmap
        clip0 = mul_point(P, matmul32(WV, Pr)).astype(F)
        view = mul_point(P, WV).astype(F)[:, :3]
        N = v[:, 3:6]
        n = (((N[:, 0:1] * NV[0] + N[:, 1:2] * NV[1]) + N[:, 2:3] * NV[2]) + ZERO * NV[3]).astype(F)
        vn = normalize_lit(np.stack([n[:, 0], n[:, 1], n[:, 0]], axis=1))         # the reference's .xyx
        E = (view + vn * HALF).astype(F)
        clip1 = mul_point(E, Pr).astype(F)
    return clip0, clip1


def records_from_clip(clip, indices, W, H):
    """O3's setup of one draw's triangles whose clip-space vertices are given: V2, V3 and the fan of §7.17 at cull NONE and one sample, in the record form
    tests/scene_depth_ref.fill reads (q = the triangle's number)"""
    idx = np.asarray(indices, dtype=I64).reshape(-1, 3)
    out_xy, out_zw, out_q, out_box = [], [], [], []
    with np.errstate(all="ignore"):
        for t, tri_idx in enumerate(idx):
            if not np.all((tri_idx >= 0) & (tri_idx < clip.shape[0])):
                continue
            tri = clip[tri_idx]
            if not np.all(np.isfinite(tri)):
                continue
            poly, _ = V.clip_polygon(tri)
            if poly.shape[0] == 0:
                continue
            xy, ok = V.snap(poly[:, [0, 1, 3]], W, H)
            for k in range(poly.shape[0] - 2):
                sel = [0, k + 1, k + 2]
                if not (ok[0] and ok[k + 1] and ok[k + 2]):
                    continue
                (x0, y0), (x1, y1), (x2, y2) = (int(a) for a in xy[0]), (int(a) for a in xy[k + 1]), (int(a) for a in xy[k + 2])
                if V.edge(x1, y1, x2, y2, x0, y0) == 0:
                    continue
                i0, i1 = V.pixel_range(min(x0, x1, x2), max(x0, x1, x2), 1, W)
                j0, j1 = V.pixel_range(min(y0, y1, y2), max(y0, y1, y2), 1, H)
                if i0 > i1 or j0 > j1:
                    continue
                out_xy.append(xy[sel]); out_zw.append(poly[sel][:, [2, 3]]); out_q.append(t); out_box.append((i0, i1, j0, j1))
    n = len(out_xy)
    return {"xy": np.array(out_xy, dtype=I64).reshape(n, 3, 2), "clip_zw": np.array(out_zw, dtype=F).reshape(n, 3, 2), "q": np.array(out_q, dtype=U32),
            "box": np.array(out_box, dtype=I64).reshape(n, 4)}


def colour_halfs(color):
    """O5: pow_(c, 2.2f) per channel, each stored round-to-nearest-even as a half (uint16 [4]); a NaN is 0x7E00 with its sign"""
    lib = _lib()
    p = np.array([lib.vqo_pow(float(F(c)), float(F(2.2))) for c in f32(color).reshape(4)], dtype=F)
    out = np.empty(4, dtype=np.uint16)
    lib.vqo_f32_to_f16(p.ctypes.data, out.ctypes.data, 4)
    return out


def planes(scene):
    """(marked bool [H, W] — O4 —, covered bool [D, H, W]: the pass-1 coverage of each draw)"""
    W, H = int(scene["width"]), int(scene["height"])
    one = {"width": W, "height": H, "samples": 1}
    marked = np.zeros((H, W), dtype=bool)
    covered = np.zeros((len(scene["draws"]), H, W), dtype=bool)
    for d, draw in enumerate(scene["draws"]):
        clip0, clip1 = vertex_stages(draw)
        _, prim = V.fill(records_from_clip(clip0, draw["indices"], W, H), one)        # a fragment below 1.0 takes the sample from the clear key
        marked |= prim[:, :, 0] != V.NO_PRIMITIVE
        covered[d] = V.fill(records_from_clip(clip1, draw["indices"], W, H), one, coverage_count=True)[:, :, 0] > 0
    return marked, covered


def outline(scene, scene_color):
    """vqhip_outline: dict(scene_color uint16 [H, W, 4] — the half bits of `scene_color` with the written pixels replaced —, selection uint8 [H, W],
    writer uint32 [H, W])"""
    marked, covered = planes(scene)
    out = np.array(np.ascontiguousarray(scene_color).view(np.uint16), copy=True)
    writer = np.full(marked.shape, NO_WRITER, dtype=U32)
    for d, draw in enumerate(scene["draws"]):                                       # submission order: the last covering draw wins
        hit = covered[d] & ~marked
        writer[hit] = d
        out[hit] = colour_halfs(f32(draw["cb"]).reshape(-1)[CB_COLOR:CB_COLOR + 4])
    return {"scene_color": out, "selection": marked.astype(np.uint8), "writer": writer}
