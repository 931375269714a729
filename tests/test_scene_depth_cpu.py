"""CPU side of vqhip_scene_depth (docs/DESIGN_DETAILS.md §7.17): the boundary (symbols, struct layout, work size, refusal without a context); the numpy statement
(tests/scene_depth_ref.py) pinned against §7.16's statement where the two contracts coincide, by a per-triangle, per-sample scalar transcription, and by properties
that need no second implementation (watertight grids at 1x and 4x, the sample positions on hand-made edges, the z planes, equal depths, the clear value, the layer
rule); a binary64 cross-check of V5; and the C++ adaptor."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import scene_depth_cases as SC
from tests import scene_depth_ref as V
from tests import shadow_raster_cases as K
from tests import shadow_raster_ref as R
from vqengine_amd import abi, capi
from vqengine_amd import shadow_scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW_SYMBOLS = {"vqhip_scene_depth", "vqhip_scene_depth_work_bytes"}
NONE = V.NO_PRIMITIVE


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ---- the scalar transcription: one triangle, one sample, one binary32 operation at a time ----------------------------------------------------------------------
def _vertex(p, M):
    x, y, z = F(p[0]), F(p[1]) + F(0.0), F(p[2])
    return [((x * M[0][j] + y * M[1][j]) + z * M[2][j]) + F(1.0) * M[3][j] for j in range(4)]


def _dist(v, plane):
    if plane == 0:
        return v[3] - F(2.0 ** -24)
    if plane == 1:
        return v[3] + v[0]
    if plane == 2:
        return v[3] - v[0]
    if plane == 3:
        return v[3] + v[1]
    if plane == 4:
        return v[3] - v[1]
    if plane == 5:
        return v[2]
    return v[3] - v[2]


def _cut(inside_v, outside_v, d_in, d_out):
    t = d_in / (d_in - d_out)
    return [inside_v[c] + t * (outside_v[c] - inside_v[c]) for c in range(4)]


def _clip(poly):
    for plane in range(7):
        out = []
        n = len(poly)
        for i in range(n):
            a, b = poly[i], poly[(i + 1) % n]
            da, db = _dist(a, plane), _dist(b, plane)
            if da >= 0:
                if len(out) < 10:
                    out.append(a)
                if not db >= 0 and len(out) < 10:
                    out.append(_cut(a, b, da, db))
            elif db >= 0 and len(out) < 10:
                out.append(_cut(b, a, db, da))
        poly = out
    return poly if len(poly) >= 3 else []


def _snap(v, w, h):
    fx = ((v[0] / v[3] + F(1.0)) * (F(0.5) * F(w))) * F(256.0)
    fy = ((F(1.0) - v[1] / v[3]) * (F(0.5) * F(h))) * F(256.0)
    if not (abs(fx) <= F(2.0 ** 24) and abs(fy) <= F(2.0 ** 24)):
        return None
    return int(np.rint(fx)), int(np.rint(fy))


def _sat(x):
    if x > 0:
        return x if x < 1 else F(1.0)
    return F(0.0)


def scalar_scene(scene, coverage_count=False):
    """(depth float32 [H, W, S], primitive uint32 [H, W, S]) by the 64-bit minimum over keys, or the fragments per sample"""
    W, H, S_ = scene["width"], scene["height"], scene["samples"]
    offs = [(128, 128)] if S_ == 1 else [(96, 32), (224, 96), (32, 160), (160, 224)]
    keys = [[[V.CLEAR_KEY] * S_ for _ in range(W)] for _ in range(H)]
    count = np.zeros((H, W, S_), dtype=np.int32)
    first = 0
    with np.errstate(all="ignore"):
        for d in scene["draws"]:
            pos, idx = d["positions"], d["indices"].reshape(-1, 3)
            for inst in range(d["wvp"].shape[0]):
                M = d["wvp"][inst]
                for t, tri in enumerate(idx):
                    q = first + inst * idx.shape[0] + t
                    if any(i >= pos.shape[0] for i in tri):
                        continue
                    poly = [_vertex(pos[i], M) for i in tri]
                    if not all(np.isfinite(c) for v in poly for c in v):
                        continue
                    poly = _clip(poly)
                    snapped = [_snap(v, W, H) for v in poly]
                    for k in range(len(poly) - 2):
                        tri_v = (0, k + 1, k + 2)
                        if any(snapped[i] is None for i in tri_v):
                            continue
                        (x0, y0), (x1, y1), (x2, y2) = (snapped[i] for i in tri_v)
                        A = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
                        if A == 0 or (A > 0 and d["cull"] == V.CULL_FRONT) or (A < 0 and d["cull"] == V.CULL_BACK):
                            continue
                        s = 1 if A > 0 else -1
                        edges = (((x1, y1), (x2, y2)), ((x2, y2), (x0, y0)), ((x0, y0), (x1, y1)))
                        tl = [s * (b[1] - a[1]) < 0 or (b[1] == a[1] and s * (b[0] - a[0]) > 0) for a, b in edges]
                        v0, v1, v2 = (poly[i] for i in tri_v)
                        z0, z1, z2 = v0[2] / v0[3], v1[2] / v1[3], v2[2] / v2[3]
                        fA = F(A)
                        for j in range(max(0, min(y0, y1, y2) // 256 - 1), min(H - 1, max(y0, y1, y2) // 256 + 1) + 1):       # a generous box: every pixel near the bounds
                            for i in range(max(0, min(x0, x1, x2) // 256 - 1), min(W - 1, max(x0, x1, x2) // 256 + 1) + 1):
                                for smp, (ox, oy) in enumerate(offs):
                                    px, py = 256 * i + ox, 256 * j + oy
                                    E = [(a[0] - px) * (b[1] - py) - (b[0] - px) * (a[1] - py) for a, b in edges]
                                    if not all(s * e > 0 or (e == 0 and t_) for e, t_ in zip(E, tl)):
                                        continue
                                    if coverage_count:
                                        count[j, i, smp] += 1
                                        continue
                                    b1, b2 = F(E[1]) / fA, F(E[2]) / fA
                                    val = _sat((z0 + b1 * (z1 - z0)) + b2 * (z2 - z0))
                                    if val >= 1:
                                        continue
                                    key = (int(np.float32(val).view(np.uint32)) << 32) | q
                                    if key < keys[j][i][smp]:
                                        keys[j][i][smp] = key
            first += idx.shape[0] * d["wvp"].shape[0]
    if coverage_count:
        return count
    k = np.array(keys, dtype=np.uint64).reshape(H, W, S_)
    return (k >> np.uint64(32)).astype(np.uint32).view(F), (k & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def scalar_layers(prim):
    H, W, _ = prim.shape
    mask, lp = np.zeros((4, H, W), dtype=np.uint8), np.full((4, H, W), NONE, dtype=np.uint32)
    for j in range(H):
        for i in range(W):
            opened = []
            for s in range(4):
                o = int(prim[j, i, s])
                if o == NONE:
                    continue
                if o not in opened:
                    opened.append(o)
                    lp[len(opened) - 1, j, i] = o
                mask[opened.index(o), j, i] |= 1 << s
    return mask, lp


# ---- boundary ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    src = open(os.path.join(ROOT, "include", "vqhip.h")).read()
    declared = set(re.findall(r"VQHIP_API\s+[\w\s\*]+?\b(vqhip_scene_depth\w*)\s*\(", src))
    assert declared == NEW_SYMBOLS
    lib = capi.load_library()
    for s in declared:
        assert s in capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert lib.vqhip_abi_version() == abi.ABI_VERSION == 3                     # additions only
    for name in ("SCENE_DEPTH_MAX_DIM", "SCENE_DEPTH_MAX_INSTANCES", "SCENE_DEPTH_MAX_LAYERS"):
        m = re.search(rf"#define VQHIP_{name}\s+(\d+)", src)
        assert m and int(m.group(1)) == getattr(abi, name)
    assert (abi.SCENE_DEPTH_MAX_DIM, abi.SCENE_DEPTH_MAX_INSTANCES) == (8192, 64)
    section = src[src.index("Main-view depth pre-pass"):]
    for word in ("ENABLE_ALPHA_MASK", "tessellation", "heightmap", "wireframe", "normals target", "interpolant planes", "UNPINNED", "DROPPED FROM THE LAYER PLANES ONLY"):
        assert word in section, f"{word} is not stated in the header section"
    # the sample pattern is the one the MSAA consumers use
    assert list(zip(V.SAMPLE_X[4], V.SAMPLE_Y[4])) == [(128 + 16 * int(x), 128 + 16 * int(y)) for x, y in abi.MSAA_SAMPLE_POSITIONS]      # sixteenths from the centre


def test_struct_layout_equals_the_c_header(tmp_path):
    structs = (("vqhip_scene_depth_draw", abi.SceneDepthDraw), ("vqhip_scene_depth_targets", abi.SceneDepthTargets))
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "vqhip.h"\nint main(void){\n'
    for cname, t in structs:
        prog += f'printf("%zu", sizeof({cname}));\n' + "".join(f'printf(" %zu", offsetof({cname}, {n}));\n' for n, _ in t._fields_) + 'printf("\\n");\n'
    prog += "return 0;}\n"
    (tmp_path / "t.c").write_text(prog)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    lines = subprocess.check_output([str(tmp_path / "t")]).decode().strip().split("\n")
    for (cname, t), line in zip(structs, lines):
        assert [int(v) for v in line.split()] == [C.sizeof(t)] + [getattr(t, n).offset for n, _ in t._fields_], cname
    assert (C.sizeof(abi.SceneDepthDraw), C.sizeof(abi.SceneDepthTargets)) == (48, 96)


def test_work_size_function():
    f = capi.load_library().vqhip_scene_depth_work_bytes
    assert f(0) == 256                                                          # the counter alone
    counts = (1, 2, 3, 100, 2000, 10 ** 6, 2 ** 29 - 1)
    sizes = [f(n) for n in counts]
    assert all(s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)       # monotone in the triangle count
    for n, s in zip(counts, sizes):
        assert 256 + 8 * n * 56 <= s <= 256 + 8 * n * 56 + 512                   # eight records of 8 + 48 bytes per instanced triangle
    assert f(2 ** 29) == 0 and f(2 ** 32 - 1) == 0 and f(2 ** 63) == 0
    assert capi.scene_depth_work_bytes(2000) == f(2000)


def test_call_without_a_context_is_refused():
    lib = capi.load_library()
    tg = abi.SceneDepthTargets()
    buf = (C.c_uint8 * 4096)()
    rc = lib.vqhip_scene_depth(None, None, None, 0, 16, 16, 1, C.byref(tg), buf, 4096)
    assert rc == abi.VQHIP_ERR_INVALID_ARG and b"ctx is NULL" in lib.vqhip_last_error(None)


# ---- pinned against §7.16's statement where the contracts coincide -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,view", [("rules_16", K.rules_view(16)), ("rules_64_back", K.rules_view(64, K.BACK)), ("boxes_64", K.boxes_view(64)),
                                       ("boxes_129_front", K.boxes_view(129, False, K.FRONT, 32, 12)), ("sphere_64", K.sphere_view(64)),
                                       ("sphere_129_none", K.sphere_view(129, False, K.NONE)), ("spot_room_64", K.spot_room_view(64)), ("spot_room_129", K.spot_room_view(129))])
def test_one_sample_square_target_equals_the_shadow_statement(name, view):
    """samples 1, W == H == dim, no polygon reaches a z plane, every depth below 1.0: the same bits as shadow_raster_ref.rasterize_view (linear False) over the
    WHOLE map — the preconditions are asserted, no texel is excluded"""
    dim = view["dim"]
    scene = SC.scene(dim, dim, 1, view["draws"])
    st = V.new_stats()
    got = V.rasterize(scene, stats=st)
    assert st["cut_by_plane"][5] == 0 and st["cut_by_plane"][6] == 0, "a z plane cuts this case: it is not a pin case"
    shadow = R.rasterize_view(dict(view, linear=False))
    covered = R.rasterize_view(dict(view, linear=False), coverage_count=True) > 0
    assert (shadow[covered] < 1.0).all() and covered.sum() > 0, "a fragment at 1.0: it is not a pin case"
    assert (bits(got["depth"]) == bits(shadow)).all()
    assert ((got["primitive"] != NONE) == covered).all()


# ---- the statement against its scalar transcription, on the GPU test set ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SC.cases()))
def test_statement_equals_the_scalar_transcription(name):
    scene, e = SC.cases()[name], SC.expected(name)
    depth, prim = scalar_scene(scene)
    if scene["samples"] == 1:
        depth, prim = depth[:, :, 0], prim[:, :, 0]
    bad = np.argwhere((bits(depth) != bits(e["depth"])) | (prim != e["primitive"]))
    assert bad.shape[0] == 0, f"{name}: {bad.shape[0]} samples differ, first at {bad[0].tolist()}"
    if scene["samples"] == 4:
        mask, lp = scalar_layers(prim)
        assert np.array_equal(mask, e["coverage"]) and np.array_equal(lp, e["layer_primitive"]), name


def test_coverage_counts_agree_too():
    for name in ("rules_16x16_s4", "soup_16x16_s4", "boxes_64x40_s1"):
        scene = SC.cases()[name]
        assert np.array_equal(scalar_scene(scene, coverage_count=True), V.fill(V.setup(scene), scene, coverage_count=True)), name


def test_the_test_set_meets_every_plane_and_every_layer_count():
    for w, h in SC.SIZES:
        for s in (1, 4):
            st = SC.expected(f"soup_{w}x{h}_s{s}")["stats"]
            assert all(c > 0 for c in st["cut_by_plane"]), f"soup {w}x{h}: a plane cuts nothing: {st['cut_by_plane']}"
            assert st["max_fan"] <= V.FAN_MAX and st["nonfinite"] == 0 and st["bad_index"] == 0
            assert sum(SC.expected(f"boxes_{w}x{h}_s{s}")["stats"]["cut_by_plane"][1:5]) > 0, "no box crosses a side plane"
        e = SC.expected(f"soup_{w}x{h}_s4")
        assert all((e["coverage"][k] != 0).any() for k in range(4)), "no pixel of the soup has four owners"


# ---- properties that need no second implementation ----------------------------------------------------------------------------------------------------------------
def _grid_on_the_target(w, h, samples, n=7, seed=3):
    p, idx = S.grid(n, 2.0, 0.35, seed)
    m = np.zeros((4, 4), dtype=F)
    m[0, 0], m[2, 1], m[3, 2], m[3, 3] = 1.0, 1.0, 0.5, 1.0
    return SC.scene(w, h, samples, [SC.draw(p, idx, m[None], None, V.CULL_NONE)])


@pytest.mark.parametrize("w,h", [(64, 40), (129, 67)])
@pytest.mark.parametrize("samples", [1, 4])
def test_watertight_grid_covers_every_sample_once(w, h, samples):
    scene = _grid_on_the_target(w, h, samples)
    count = V.fill(V.setup(scene), scene, coverage_count=True)
    assert count.shape == (h, w, samples) and (count == 1).all(), f"{int((count != 1).sum())} samples are not covered exactly once"
    out = V.rasterize(scene)
    assert (bits(out["depth"]) == bits(F(0.5))).all() and (out["primitive"] != NONE).all()


def _px_scene(w, h, samples, tris, z, cull=V.CULL_NONE):
    pos, idx = SC.px_triangles(w, h, tris, z)
    return SC.scene(w, h, samples, [SC.draw(pos, idx, K.IDENTITY, None, cull)])


def _quad(x0, x1, y0=2.0, y1=14.0):
    return [((x0, y0), (x1, y0), (x1, y1)), ((x0, y0), (x1, y1), (x0, y1))]


def _owned(out):
    """bit s: sample s of the pixel has an owner (the union of the layer masks; a quad is two primitives, so its pixels on the diagonal have two layers)"""
    return sum(((out["primitive"][:, :, s] != NONE).astype(np.int64) << s) for s in range(4))


def test_sample_positions_on_hand_made_edges():
    # a quad whose left edge is the pixel centre line of column 10: samples 1 and 3 (x = 10.875, 10.625) are right of it, samples 0 and 2 (10.375, 10.125) left
    out = V.rasterize(_px_scene(16, 16, 4, _quad(10.5, 14.0), [0.5, 0.5]))
    assert (_owned(out)[3:13, 10] == 0b1010).all() and (_owned(out)[3:13, 11:14] == 0b1111).all() and (_owned(out)[:, :10] == 0).all()
    # an edge exactly through sample 0 (x = 10 + 96 / 256): a left edge owns the sample, a right edge does not
    left = V.rasterize(_px_scene(16, 16, 4, _quad(10.375, 14.0), [0.5, 0.5]))
    right = V.rasterize(_px_scene(16, 16, 4, _quad(2.0, 10.375), [0.5, 0.5]))
    assert (_owned(left)[3:13, 10] == 0b1011).all()                      # samples 0, 1, 3: only sample 2 (x = 10.125) is left of the edge
    assert (_owned(right)[3:13, 10] == 0b0100).all()                     # sample 2 alone; sample 0 sits on the right edge and is not owned
    both = _px_scene(16, 16, 4, _quad(2.0, 10.375) + _quad(10.375, 14.0), [0.5] * 4)
    assert V.fill(V.setup(both), both, coverage_count=True)[3:13, 2:14].min() == 1 and V.fill(V.setup(both), both, coverage_count=True).max() == 1
    # the same edges at one sample per pixel: the centre (10.5) is right of 10.375
    assert (V.rasterize(_px_scene(16, 16, 1, _quad(10.375, 14.0), [0.5, 0.5]))["primitive"][3:13, 10] != NONE).all()
    assert (V.rasterize(_px_scene(16, 16, 1, _quad(10.5, 14.0), [0.5, 0.5]))["primitive"][3:13, 10] != NONE).all()      # the centre on a left edge: owned
    assert (V.rasterize(_px_scene(16, 16, 1, _quad(2.0, 10.5), [0.5, 0.5]))["primitive"][3:13, 10] == NONE).all()       # on a right edge: not owned


def _tilted_quad(samples, z_left, z_right):
    """the whole 16 x 16 target as two triangles that share the diagonal; z runs linearly from z_left at x = 0 to z_right at x = 16 (w = 1)"""
    corners = {(0, 0): z_left, (16, 0): z_right, (16, 16): z_right, (0, 16): z_left}
    pos, idx = [], []
    for tri in (((0, 0), (16, 0), (16, 16)), ((0, 0), (16, 16), (0, 16))):
        for (x, y) in tri:
            idx.append(len(pos))
            pos.append((x / 8.0 - 1.0, 1.0 - y / 8.0, corners[(x, y)]))
    return SC.scene(16, 16, samples, [SC.draw(np.array(pos, dtype=F), np.array(idx), K.IDENTITY, None, V.CULL_NONE)])


@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("plane,z_left,z_right,keep_right", [(5, -0.5, 0.5, True), (6, 0.5, 1.5, False)])
def test_z_planes_remove_exactly_what_lies_outside(samples, plane, z_left, z_right, keep_right):
    """z crosses the plane at x = 8 exactly (t = 1/2): the kept half is covered exactly once — the diagonal stays watertight because both triangles compute the
    same new vertex on it —, the other half not at all"""
    scene = _tilted_quad(samples, z_left, z_right)
    st = V.new_stats()
    count = V.fill(V.setup(scene, st), scene, coverage_count=True)
    assert st["cut_by_plane"][plane] == 2 and sum(st["cut_by_plane"]) == 2
    kept = np.zeros((16, 16, samples), dtype=bool)
    kept[:, 8:, :] = True
    if not keep_right:
        kept = ~kept
    assert np.array_equal(count, kept.astype(np.int32))
    out = V.rasterize(scene)
    owned = out["primitive"] != NONE
    assert np.array_equal(owned.reshape(16, 16, samples), kept) and (out["depth"][owned] < 1.0).all() and (out["depth"][owned] >= 0.0).all()
    # the two triangles share the edge (0, 0) .. (16, 16): the vertices the clipper creates on it are the same bits
    d = scene["draws"][0]
    tris = R.mul_point(d["positions"][:, :3], d["wvp"][0]).astype(F)[d["indices"].reshape(-1, 3)]
    polys = [V.clip_polygon(t)[0] for t in tris]
    new = [{tuple(bits(v).tolist()) for v in p if not any((bits(v) == bits(o)).all() for o in t)} for p, t in zip(polys, tris)]
    assert len(new[0] & new[1]) == 1 and len(new[0]) == 2 and len(new[1]) == 2


@pytest.mark.parametrize("samples", [1, 4])
def test_equal_depth_goes_to_the_first_submitted(samples):
    ab, ba = SC.expected(f"pair_ab_64x40_s{samples}"), SC.expected(f"pair_ba_64x40_s{samples}")
    shared = ab["primitive"] == 0                                              # q(A) = 0 in the order A, B; B's copy would be 2
    assert shared.sum() > 100 and (ba["primitive"][shared] == 1).all()         # q(B's copy) = 1 in the order B, A; A's copy would be 2
    assert not (ab["primitive"] == 2).any() and not (ba["primitive"] == 2).any()
    assert np.array_equal(bits(ab["depth"]), bits(ba["depth"]))


@pytest.mark.parametrize("samples", [1, 4])
def test_a_fragment_at_exactly_one_is_not_written(samples):
    scene = _px_scene(16, 16, samples, _quad(2.0, 14.0), [1.0, 1.0])
    assert V.fill(V.setup(scene), scene, coverage_count=True).sum() == 12 * 12 * samples
    out = V.rasterize(scene)
    assert (out["primitive"] == NONE).all() and (bits(out["depth"]) == 0x3F800000).all()
    behind = _px_scene(16, 16, samples, _quad(2.0, 14.0) + _quad(4.0, 10.0), [1.0, 1.0, 0.75, 0.75])       # a nearer quad in front of it is written as usual
    out = V.rasterize(behind)
    assert set(np.unique(out["primitive"]).tolist()) == {2, 3, NONE}


# ---- the layer rule --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soup_64x40_s4", "room_129x67_s4", "boxes_16x16_s4"])
def test_layers(name):
    e = SC.expected(name)
    prim, cov, lp = e["primitive"], e["coverage"].astype(np.int64), e["layer_primitive"]
    assert all(((cov[a] & cov[b]) == 0).all() for a in range(4) for b in range(a + 1, 4)), "the masks are not disjoint"
    owned = sum(((prim[:, :, s] != NONE).astype(np.int64) << s) for s in range(4))
    assert np.array_equal(cov[0] | cov[1] | cov[2] | cov[3], owned) and (cov < 16).all()
    for k in range(4):
        assert ((cov[k] == 0) == (lp[k] == NONE)).all(), "an unused layer is not empty, or a used one has no primitive"
        for s in range(4):
            has = (cov[k] >> s) & 1 == 1
            assert (prim[:, :, s][has] == lp[k][has]).all()
    low = [np.where(cov[k] != 0, (cov[k] & -cov[k]), 1 << 8) for k in range(4)]            # the first owning sample of each layer, 256 for an unused one
    assert all((low[k] < low[k + 1]).all() or ((low[k] < low[k + 1]) | (low[k + 1] == 256)).all() for k in range(3)), "layer order does not follow the first owning sample"
    # fewer layers than a pixel needs: the first planes of the four, the rest dropped; depth and primitive are not touched by the choice
    three = (cov[2] != 0) & (cov[3] == 0)
    if name.startswith("soup"):
        assert three.sum() > 0
    c2, l2 = V.layers_of(np.asarray(prim), 2)
    assert np.array_equal(c2, e["coverage"][:2]) and np.array_equal(l2, lp[:2])


# ---- binary64 cross-check of V5 ---------------------------------------------------------------------------------------------------------------------------------------
def test_float64_cross_check():
    """The same snapped vertices with V5 evaluated in binary64: coverage is identical (integer arithmetic decides it); `primitive` is identical apart from samples
    where two depths tie differently in the two precisions (their number is recorded); the largest depth difference over the samples with the same owner, in
    binary32 ulps at the value, is the figure recorded in §7.17 — a record, not a tolerance. Seeded scenes and correctly rounded arithmetic: asserted exactly."""
    worst, where, differs = 0.0, None, 0
    for name, scene in SC.cases().items():
        e = SC.expected(name)
        rec = V.setup(scene)
        d64, p64 = V.fill(rec, scene, dtype=np.float64)
        d32, p32 = np.asarray(e["depth"]).reshape(d64.shape), np.asarray(e["primitive"]).reshape(p64.shape)
        same = p32 == p64
        differs += int((~same).sum())
        ref = d64.astype(F)
        ulp = np.spacing(np.maximum(np.abs(ref), F(2.0 ** -126))).astype(np.float64)
        u = np.where(same, np.abs(d32.astype(np.float64) - d64) / ulp, 0.0)
        if u.max() > worst:
            worst, where = float(u.max()), (name, tuple(int(a) for a in np.unravel_index(u.argmax(), u.shape)))
    print(f"V5 binary64 cross-check: max {worst!r} ulps at {where}; owner differs at {differs} samples")
    doc = open(os.path.join(ROOT, "docs", "DESIGN_DETAILS.md")).read()
    section = doc[doc.index("### 7.17"):]
    assert repr(worst) in section and where[0] in section and f"{differs} samples" in section, "§7.17 does not carry the measured figures"


# ---- the host-side producers and the adaptor ------------------------------------------------------------------------------------------------------------------------
def test_camera_matrix_is_left_handed_with_depth_zero_to_one():
    vp = S.camera_view_proj((1.0, 2.0, -3.0), (1.0, 2.0, 5.0), np.radians(60.0), 16.0 / 9.0, 0.5, 100.0)
    for z, depth in ((-3.0 + 0.5, 0.0), (-3.0 + 100.0, 1.0)):
        clip = np.array([1.0, 2.0, z, 1.0]) @ vp
        assert abs(clip[2] / clip[3] - depth) < 1e-12 and clip[3] > 0            # +z is forward; near -> 0, far -> 1
    right, up = np.array([2.0, 2.0, 0.0, 1.0]) @ vp, np.array([1.0, 3.0, 0.0, 1.0]) @ vp
    assert right[0] > 0 and abs(right[1]) < 1e-12 and up[1] > 0 and abs(up[0]) < 1e-12
    assert abs(up[1] / up[3] / (right[0] / right[3]) - 16.0 / 9.0) < 1e-12      # x is narrowed by the aspect


def test_cpp_adaptor_builds_the_call_from_the_pre_pass(tmp_path):
    """tests/cpp/test_passes_scene_depth.cpp against tests/cpp/mock_engine/, with the command line tests/test_shadow_raster_cpu.py uses"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = tmp_path / "test_passes_scene_depth"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    lib = os.path.join(ROOT, "vqengine_amd", "lib")
    r = subprocess.run([hipcc, "-std=c++17", "-O2", "-Wall", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I.", "-I../../include", "-I/opt/rocm/include",
                        "test_passes_scene_depth.cpp", "-o", str(exe), "-L../../vqengine_amd/lib", "-lvqhip", "-L/opt/rocm/lib", "-lamdhip64",
                        f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], cwd=cpp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "scene depth adaptor OK" in r.stdout, (r.returncode, r.stdout, r.stderr)
