"""docs/DESIGN_DETAILS.md §7.23 (the contract U1 .. U7 of vqhip_unlit_draws) stated in numpy on top of tests/scene_depth_ref.py: the vertex stage, the clipper
against seven planes, viewport and snap, the cull mode and the fan are §7.17's setup, unchanged and therefore called (U1, U2, U4: a draw is one instance whose
matrix is the cbuffer's matModelViewProj); what this file adds is the fill: int64 edge functions with the top-left rule and V5's depth exactly as
tests/scene_depth_ref.fill writes them, U3's test against a depth plane that is never written, and — per pixel, over the records IN SUBMISSION ORDER — U5's
overwrite or U6's fold, every operation rounded in binary32 and the result rounded to half after every fragment. tests/test_unlit_draws_cpu.py pins the fold
with an independent binary64-then-round restatement and the half conversion with the CPU checker's (oracle/: vqo_f32_to_f16).

A scene is a dict: width, height, depth float32 [H, W] (the scene's depth), draws = [dict(vertices float32 [V, >= 3], indices int [3 T], cb float32 [20] = one
VQ_UnlitData, cull 0 | 1 | 2)]."""
import numpy as np

from tests import scene_depth_ref as V
from tests.shadow_raster_ref import F, I64, edge, f32, saturate

U16, U32 = np.uint16, np.uint32
NO_WRITER = 0xFFFFFFFF
ONE = F(1.0)
CB_COLOR = 16                                   # float offset of VQ_UnlitData.color
NAN_HALF = 0x7E00


def depth_scene(scene):
    """the scene in the form tests/scene_depth_ref.setup reads: one instance per draw, the cbuffer's matrix"""
    return {"width": scene["width"], "height": scene["height"], "samples": 1,
            "draws": [{"positions": f32(d["vertices"])[:, :3], "indices": d["indices"], "wvp": f32(d["cb"]).reshape(-1)[:16].reshape(1, 4, 4), "cull": int(d["cull"])}
                      for d in scene["draws"]]}


def records(scene):
    """U1, U2, U4: §7.17's records of the scene in submission order (q ascending, a triangle's fan pieces in fan order), and the draw of each record"""
    rec = V.setup(depth_scene(scene))
    first = np.cumsum([0] + [len(d["indices"]) // 3 for d in scene["draws"]])
    rec["draw"] = (np.searchsorted(first, rec["q"].astype(I64), side="right") - 1).astype(I64)
    assert np.all(np.diff(rec["q"].astype(I64)) >= 0), "the records are in submission order"
    return rec


def to_half(x):
    """RN16 of binary32 values: round to nearest even, denormals kept, overflow to inf; uint16 bits (a NaN's bits are the caller's business)"""
    with np.errstate(all="ignore"):
        return f32(x).astype(np.float16).view(U16)


def opaque_halfs(color):
    """U5 = O5's conversion of the four channels: a NaN is 0x7E00 with its sign"""
    c = f32(color).reshape(4)
    h = to_half(c)
    nan = np.isnan(c)
    return np.where(nan, ((c.view(U32) >> 16) & 0x8000).astype(U16) | U16(NAN_HALF), h).astype(U16)


def blend_step(dst, src):
    """U6, one fragment: dst float32 [..., 4] (values that are halfs exactly, or NaN), src float32 [4] -> the new dst, again halfs held as binary32"""
    with np.errstate(all="ignore"):
        a = F(src[3])
        ia = F(ONE - a)
        out = np.empty_like(dst)
        for c in range(3):
            out[..., c] = ((F(src[c]) * a).astype(F) + (dst[..., c] * ia).astype(F)).astype(F).astype(np.float16).astype(F)
        out[..., 3] = F(a).astype(np.float16).astype(F)
    return out


def store_blend(values):
    """U6's stored bits of the folded values: exact (they are halfs), a NaN as 0x7E00 with the sign cleared"""
    return np.where(np.isnan(values), U16(NAN_HALF), to_half(values)).astype(U16)


def fragments(rec, r, depth):
    """record r over its box: (j0, j1, i0, i1, passing bool [rows, cols]) — R4's coverage at the pixel centre, V5's depth, U3's test against `depth`"""
    (x0, y0), (x1, y1), (x2, y2) = (int(a) for a in rec["xy"][r, 0]), (int(a) for a in rec["xy"][r, 1]), (int(a) for a in rec["xy"][r, 2])
    i0, i1, j0, j1 = (int(a) for a in rec["box"][r])
    px = (256 * np.arange(i0, i1 + 1, dtype=I64))[None, :] + 128
    py = (256 * np.arange(j0, j1 + 1, dtype=I64))[:, None] + 128
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
        return j0, j1, i0, i1, inside
    with np.errstate(all="ignore"):
        fA = F(A)
        b1, b2 = E[1].astype(F) / fA, E[2].astype(F) / fA
        zw = rec["clip_zw"][r].astype(F)
        z0, z1, z2 = zw[0, 0] / zw[0, 1], zw[1, 0] / zw[1, 1], zw[2, 0] / zw[2, 1]
        d = saturate((z0 + b1 * (z1 - z0)) + b2 * (z2 - z0)).astype(F)
        passing = inside & (d < depth[j0:j1 + 1, i0:i1 + 1])                      # U3: strictly below, binary32; a NaN in the plane passes nothing
    return j0, j1, i0, i1, passing


def unlit_draws(scene, scene_color, blend, stats=None):
    """vqhip_unlit_draws: dict(scene_color uint16 [H, W, 4] — the half bits of `scene_color` with the touched pixels replaced —, writer uint32 [H, W]).
    stats: a dict that receives `fragments` int32 [H, W], the passing fragments per pixel, and `records`, the number of records."""
    W, H = int(scene["width"]), int(scene["height"])
    depth = f32(scene["depth"]).reshape(H, W)
    rec = records(scene)
    out = np.array(np.ascontiguousarray(scene_color).view(U16), copy=True).reshape(H, W, 4)
    writer = np.full((H, W), NO_WRITER, dtype=U32)
    count = np.zeros((H, W), dtype=np.int32)
    with np.errstate(all="ignore"):
        values = out.view(np.float16).astype(F)                                   # U6: the stored halfs, decoded exactly
    colours = [f32(d["cb"]).reshape(-1)[CB_COLOR:CB_COLOR + 4] for d in scene["draws"]]
    for r in range(rec["xy"].shape[0]):                                            # submission order
        j0, j1, i0, i1, passing = fragments(rec, r, depth)
        if not passing.any():
            continue
        d = int(rec["draw"][r])
        box = (slice(j0, j1 + 1), slice(i0, i1 + 1))
        writer[box] = np.where(passing, U32(d), writer[box])
        count[box] += passing
        if blend:
            values[box] = np.where(passing[..., None], blend_step(values[box], colours[d]), values[box])
        else:
            out[box] = np.where(passing[..., None], opaque_halfs(colours[d]), out[box])
    if blend:
        touched = writer != NO_WRITER
        out[touched] = store_blend(values[touched])
    if stats is not None:
        stats["fragments"], stats["records"] = count, int(rec["xy"].shape[0])
    return {"scene_color": out, "writer": writer}
