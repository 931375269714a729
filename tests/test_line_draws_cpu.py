"""CPU side of vqhip_line_draws (docs/DESIGN_DETAILS.md §7.24 L1 .. L8): the integer walk of the numpy statement the GPU tests compare against
(tests/line_ref.py) pinned, pixel for pixel, by an independent exact restatement of L5 with fractions.Fraction — the segment intersected with the diamond as a
point set, the included edges and corners spelt out —; L3 pinned by a scalar, one-operation-per-line numpy.float32 restatement; the emission order and colours;
and the boundary: symbols, struct layouts against gcc, the work-size function, the refusal without a context, the host mirror of the three producers, the
documents, the C++ adaptor against tests/cpp/mock_engine/."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np

from tests import line_cases as LC
from tests import line_ref as L
from tests import outline_ref as OR
from tests import unlit_cases as UC
from vqengine_amd import abi, capi
from vqengine_amd import line_scene as LS
from vqengine_amd import shadow_scene as S
from vqengine_amd import unlit_scene as US

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW_SYMBOLS = {"vqhip_line_draws", "vqhip_line_draws_work_bytes"}
INCLUDED = {"interior", "lower_left", "lower_right", "bottom"}          # and "right" for y-major lines


# ---- L5 restated: the diamond as a point set ----------------------------------------------------------------------------------------------------------------------------
def classify(px, py, cx, cy):
    """where the point lies relative to the diamond of the pixel centred at (cx, cy): interior, outside, or the name of the edge or corner it is on"""
    dx, dy = Fraction(px) - cx, Fraction(py) - cy
    a = abs(dx) + abs(dy)
    if a != 128:
        return "interior" if a < 128 else "outside"
    if dx == 0:
        return "bottom" if dy > 0 else "top"
    if dy == 0:
        return "right" if dx > 0 else "left"
    return ("lower_" if dy > 0 else "upper_") + ("right" if dx > 0 else "left")


def in_set(cls, y_major):
    return cls in INCLUDED or (y_major and cls == "right")


def exact_cover(x0, y0, x1, y1, i, j, decided=None):
    """L5 for one pixel, from the definition: the closed segment meets the diamond set and the segment's end point is not in it. The distance
    |x - cx| + |y - cy| is convex and piecewise linear along the segment: its minimum is at an end or where the segment crosses one of the pixel's two axes; a
    minimum of exactly 128 is a touch — at a point, or along an edge (then the midpoint of the stretch stands for its interior). decided: a set that receives
    the names of the edges and corners the decision depended on."""
    if (x0, y0) == (x1, y1):
        return False
    cx, cy = 256 * i + 128, 256 * j + 128
    y_major = abs(x1 - x0) < abs(y1 - y0)
    ts = {Fraction(0), Fraction(1)}
    if x1 != x0 and 0 <= Fraction(cx - x0, x1 - x0) <= 1:
        ts.add(Fraction(cx - x0, x1 - x0))
    if y1 != y0 and 0 <= Fraction(cy - y0, y1 - y0) <= 1:
        ts.add(Fraction(cy - y0, y1 - y0))
    ts = sorted(ts)
    at = lambda t: (x0 + t * (x1 - x0), y0 + t * (y1 - y0))
    dist = lambda p: abs(p[0] - cx) + abs(p[1] - cy)
    lowest = min(dist(at(t)) for t in ts)
    if lowest > 128:
        return False
    if lowest < 128:
        meets = True
    else:
        touch = [t for t in ts if dist(at(t)) == 128]
        touch += [(a + b) / 2 for a, b in zip(touch, touch[1:])]           # the stretch between two touching breakpoints runs along one edge
        names = {classify(*at(t), cx, cy) for t in touch}
        meets = any(in_set(n, y_major) for n in names)
        if decided is not None:
            decided.update((n, y_major) for n in names)
    end = classify(x1, y1, cx, cy)
    if decided is not None and meets and end not in ("interior", "outside"):
        decided.add((end, y_major))
    return meets and not in_set(end, y_major)


def exact_pixels(x0, y0, x1, y1, decided=None):
    """every covered pixel of the neighbourhood of the line's extent (one pixel beyond it on every side)"""
    i0, i1 = min(x0, x1) // 256 - 1, max(x0, x1) // 256 + 1
    j0, j1 = min(y0, y1) // 256 - 1, max(y0, y1) // 256 + 1
    return {(i, j) for j in range(j0, j1 + 1) for i in range(i0, i1 + 1) if exact_cover(x0, y0, x1, y1, i, j, decided)}


def test_walk_equals_the_exact_restatement_of_the_diamond_rule():
    """total agreement on the adversarial list and the seeded set; every included or excluded edge and corner decides at least one pixel; reversing a line changes
    the result exactly at end pixels, and does so; at most one pixel per major step"""
    lines = LC.adversarial_lines()
    decided = set()
    covered = {}
    for l in lines:
        want = exact_pixels(*l, decided)
        got = L.walk(*l)
        assert {(i, j) for i, j, _ in got} == want and len(got) == len(want), (l, sorted(want), got)
        covered[l] = want
        y_major = L.is_y_major(*l)
        steps = [j if y_major else i for i, j in want]
        assert len(steps) == len(set(steps)), f"{l}: two pixels in one step of the major axis"
        assert all(c == 256 * (j if y_major else i) + 128 for i, j, c in got)
    assert sum(len(v) for v in covered.values()) > 1500 and sum(1 for v in covered.values() if not v) >= 8
    for name in ("top", "bottom", "left", "right", "upper_left", "upper_right", "lower_left", "lower_right"):
        for y_major in (False, True):
            if name in ("upper_left", "upper_right", "lower_left", "lower_right") and y_major:
                continue                                                   # a y-major segment cannot run along an edge; its ends on edges are counted below
            assert (name, y_major) in decided, f"no pixel of the set is decided by the {name} of a diamond ({'y' if y_major else 'x'}-major)"
    assert {(n, True) for n in ("upper_left", "upper_right", "lower_left", "lower_right")} <= decided
    changed = 0
    for (x0, y0, x1, y1), fwd in covered.items():
        back = covered[(x1, y1, x0, y0)]
        ends = {(x0 // 256 + a, y0 // 256 + b) for a in (-1, 0) for b in (-1, 0)} | {(x1 // 256 + a, y1 // 256 + b) for a in (-1, 0) for b in (-1, 0)}
        assert (fwd ^ back) <= ends, ((x0, y0, x1, y1), fwd ^ back)
        changed += bool(fwd ^ back)
    assert changed > 50, "the direction decides nothing in this set"
    # the slope-1 case is x-major; the right corner belongs to y-major lines alone
    assert not L.is_y_major(0, 0, 300, 300) and not L.is_y_major(0, 0, 300, -300) and L.is_y_major(0, 0, 299, 300)
    assert L.in_diamond(128 + 128, 128, 128, 128, True) and not L.in_diamond(128 + 128, 128, 128, 128, False)


def test_clamped_walk_is_the_walk_inside_the_target():
    for l in LC.adversarial_lines()[::7]:
        full = L.walk(*l)
        assert L.walk(*l, 6, 5) == [(i, j, c) for i, j, c in full if 0 <= i < 6 and 0 <= j < 5]


# ---- L3 against a scalar restatement ------------------------------------------------------------------------------------------------------------------------------------
def _normalize(v):
    xx = F(v[0] * v[0])
    yy = F(v[1] * v[1])
    s = F(xx + yy)
    zz = F(v[2] * v[2])
    dd = F(s + zz)
    l = F(np.sqrt(dd))
    return [F(v[0] / l), F(v[1] / l), F(v[2] / l)]


def _mul(v, w, M):
    out = []
    for j in range(4):
        a = F(v[0] * M[0][j])
        b = F(v[1] * M[1][j])
        s = F(a + b)
        c = F(v[2] * M[2][j])
        s = F(s + c)
        d = F(w * M[3][j])
        out.append(F(s + d))
    return out


def scalar_axes(vertex, cb):
    """VertexDebug.hlsl:54-107 for one point, one binary32 operation per line: the three lines' clip-space ends, [3][2][4]"""
    world, normal, vp = (cb[o:o + 16].reshape(4, 4) for o in (0, 16, 32))
    size = cb[48]
    p, N, T = vertex[0:3], vertex[3:6], vertex[6:9]
    c0 = F(F(N[1] * T[2]) - F(N[2] * T[1]))
    c1 = F(F(N[2] * T[0]) - F(N[0] * T[2]))
    c2 = F(F(N[0] * T[1]) - F(N[1] * T[0]))
    tbn = (_normalize(T), _normalize([c0, c1, c2]), _normalize(N))
    P = _mul(p, F(1.0), world)[:3]
    start = _mul(P, F(1.0), vp)
    out = []
    for k in range(3):
        o = _normalize(_mul(tbn[k], F(0.0), normal)[:3])
        e = [F(P[0] + F(o[0] * size)), F(P[1] + F(o[1] * size)), F(P[2] + F(o[2] * size))]
        out.append([start, _mul(e, F(1.0), vp)])
    return np.array(out, dtype=F)


def test_axes_vertex_stage_equals_the_scalar_restatement():
    """bit-equal, NaNs included: the sphere of the axes case under a non-uniform matNormal, with its zero normal, zero tangent and normal parallel to the tangent"""
    draw = LC.case("axes_mesh_64x40")["draws"][0]
    with np.errstate(all="ignore"):
        ends, live = L.axes_ends(draw)
        ends = ends.reshape(-1, 3, 2, 4)
        v, cb = draw["vertices"], draw["cb"]
        assert not np.allclose(cb[16:32].reshape(4, 4)[:3, :3], np.eye(3) * cb[16]), "matNormal is non-uniform"
        seen_nan = 0
        for n, vi in enumerate(draw["indices"]):
            if not 0 <= vi < len(v):
                assert not live[3 * n:3 * n + 3].any()
                continue
            want = scalar_axes(v[vi], cb)
            assert np.array_equal(ends[n].view(np.uint32), want.view(np.uint32)), f"point {n} (vertex {vi})"
            seen_nan += int(np.isnan(want).any())
    assert seen_nan >= 3
    # a zero normal: the normal and the cross axis vanish, the tangent axis stays; a zero tangent: the normal axis alone stays; parallel: the cross axis vanishes
    fin = np.isfinite(ends).all(axis=(2, 3))
    assert fin[3].tolist() == [True, False, False] and fin[5].tolist() == [False, False, True] and fin[7].tolist() == [True, False, True]
    assert np.array_equal(L.normalize_lit(v[:, 3:6]).view(np.uint32), OR.normalize_lit(v[:, 3:6]).view(np.uint32)), "the contract's normalize, as O2 uses it"


def test_emission_order_and_colours():
    assert L.AXIS_COLOURS == ((0.6, 0.0, 0.0, 1.0), (0.0, 0.0, 0.6, 1.0), (0.0, 0.6, 0.0, 1.0))        # tangent red, cross(N, T) BLUE, normal green
    h06, one = int(np.float16(F(0.6)).view(np.uint16)), 0x3C00
    assert L.draw_colours({"kind": "axes"}).tolist() == [[h06, 0, 0, one], [0, 0, h06, one], [0, h06, 0, one]]
    # one point with orthogonal axes of its own on a cleared frame: three lines from the centre, right (tangent), up on screen (cross) and none along the view (normal)
    w, h = 16, 16
    v = np.array([[0.0, 0.0, 0.5, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0]], dtype=F)
    sc = LC.scene(w, h, [LC.axes(v, [0], np.eye(4), np.eye(4), np.eye(4), 0.5)])
    rec = L.lines(sc)
    assert rec["q"].tolist() == [0, 1] and rec["colour"].tolist() == [0, 1]                             # the normal's line has no length on screen
    out = L.line_draws(sc, np.zeros((h, w, 4), dtype=np.uint16))
    # the point snaps to the corner shared by four pixels: the tangent's line runs right through the bottom corners of row 7, the cross's line — cross((0, 0, 1),
    # (1, 0, 0)) = +y, up the screen — through the right corners of column 7
    assert out["scene_color"][7, 9].tolist() == [h06, 0, 0, one] and out["scene_color"][6, 7].tolist() == [0, 0, h06, one]
    assert (out["writer"] == 0).sum() == 8 and not out["scene_color"][8:, :].any() and not out["scene_color"][:, :7].any()
    # wireframe q numbering: three lines per triangle, instance-major
    tri = (np.array([LC.ndc(300, 300, w, h), LC.ndc(3000, 500, w, h), LC.ndc(800, 3000, w, h)], dtype=F), [0, 1, 2])
    rec = L.lines(LC.scene(w, h, [LC.wire(tri, [np.eye(4)] * 2, LC.RED), LC.wire(tri, [np.eye(4)], LC.TEAL)]))
    assert rec["q"].tolist() == list(range(9)) and rec["draw"].tolist() == [0] * 6 + [1] * 3
    assert rec["xy"][0].tolist() == [[300, 300], [3000, 500]] and rec["xy"][1].tolist() == [[3000, 500], [800, 3000]] and rec["xy"][2].tolist() == [[800, 3000], [300, 300]]


def test_what_the_cases_are_there_for():
    for (w, h) in LC.SIZES:
        st = LC.expected(f"clip_planes_{w}x{h}")["stats"]
        assert all(c > 0 for c in st["cut_by_plane"]) and st["nonfinite"] > 0 and st["bad_index"] > 0 and st["clipped_away"] > 0
        st = LC.expected(f"soup_{w}x{h}")["stats"]
        assert st["records"] > 256 * 9 and st["lines"] == L.total_lines(LC.case(f"soup_{w}x{h}"))
        rec = L.lines(LC.case(f"soup_{w}x{h}"))
        assert rec["xy"].max() < 32 * 256, "every line lies inside the first 32 x 32 tile"
        assert LC.case(f"cube_instances_{w}x{h}")["draws"][0]["matrices"].shape == (512, 4, 4)
        ab, ba = LC.expected(f"crossing_ab_{w}x{h}"), LC.expected(f"crossing_ba_{w}x{h}")
        shared = (ab["writer"] == 1) & (ba["writer"] == 1)
        assert shared.sum() >= 4 and np.array_equal((ab["scene_color"] != ba["scene_color"]).any(axis=-1), shared)
        # the depth producer's own box as wire: its silhouette lines lie ON its own depth and never strictly below it everywhere; NaN and 0.0 pass nothing
        dp, sc = LC.expected(f"depth_plane_{w}x{h}"), LC.case(f"depth_plane_{w}x{h}")
        blocked = np.isnan(sc["depth"]) | (sc["depth"] == 0.0)
        assert blocked.sum() > 5 and (dp["writer"][blocked] == L.NO_WRITER).all()
        ax = LC.expected(f"axes_mesh_{w}x{h}")
        assert (ax["writer"] == 1).sum() == 0 and (ax["writer"] == 0).sum() > 10, "LocalAxisSize 0 draws nothing"
        se = LC.expected(f"shared_edge_{w}x{h}")["stats"]["fragments"]
        assert se.max() >= 4, "the shared edge is drawn by both triangles of the first draw and by both later draws"
    # every placed adversarial line snaps to the grid point it was built for
    for (w, h) in LC.SIZES:
        layers = LC.placed_lines(w, h)
        sc = LC.case(f"adversarial_wire_{w}x{h}")
        for layer, d in zip(layers, sc["draws"]):
            rec = L.lines(LC.scene(w, h, [d]))
            want = [l for l in layer if (l[0], l[1]) != (l[2], l[3])]
            assert rec["xy"].reshape(-1, 4).tolist() == [list(l) for l in want]


# ---- boundary -----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    src = open(os.path.join(ROOT, "include", "vqhip.h")).read()
    declared = set(re.findall(r"VQHIP_API\s+[\w\s\*]+?\b(vqhip_line_draws\w*)\s*\(", src))
    assert declared == NEW_SYMBOLS
    lib = capi.load_library()
    for s in declared:
        assert s in capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert lib.vqhip_abi_version() == abi.ABI_VERSION == 3                          # additions only
    section = src[src.index("---- Line draws:"):]
    for word in ("L1", "L2", "L3", "L4", "L5", "L6", "L7", "L8", "UNPINNED", "IN PLACE", "WITHOUT depth writes", "largest q", "0x7E00", "BLUE", "k_lines_setup", "k_lines_fill",
                 "4x MSAA", "2^31", "VQHIP_LINES_MAX_INSTANCES", "sizeof(VQ_VertexAxesData) == 208", "sizeof(vqhip_line_draw) == 64", "vqhip_unlit_targets"):
        assert word in section, f"{word} is not stated in the header section"
    unlit = src[src.index("---- Unlit draws: the light gizmo meshes"):src.index("---- Line draws:")]
    assert "vqhip_line_draws" in unlit, "the unlit section's out-of-scope sentence points at the new call"
    assert int(re.search(r"#define\s+VQHIP_LINES_MAX_INSTANCES\s+(\d+)", src).group(1)) == abi.LINES_MAX_INSTANCES == 512
    assert (abi.LINES_WIREFRAME, abi.LINES_VERTEX_AXES) == (0, 1) and "VQHIP_LINES_WIREFRAME = 0, VQHIP_LINES_VERTEX_AXES = 1" in src


def test_struct_layout_equals_the_c_header(tmp_path):
    structs = (("VQ_VertexAxesData", abi.VertexAxesData), ("vqhip_line_draw", abi.LineDraw), ("vqhip_unlit_targets", abi.UnlitTargets))
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "vqhip.h"\nint main(void){\n'
    for cname, t in structs:
        prog += f'printf("%zu", sizeof({cname}));\n' + "".join(f'printf(" %zu", offsetof({cname}, {n}));\n' for n, _ in t._fields_) + 'printf("\\n");\n'
    prog += "return 0;}\n"
    (tmp_path / "t.c").write_text(prog)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    out = subprocess.check_output([str(tmp_path / "t")]).decode().strip().split("\n")
    for (cname, t), line in zip(structs, out):
        assert [int(v) for v in line.split()] == [C.sizeof(t)] + [getattr(t, n).offset for n, _ in t._fields_], cname
    assert (C.sizeof(abi.VertexAxesData), C.sizeof(abi.LineDraw)) == (abi.VERTEX_AXES_DATA_BYTES, 64) and abi.VERTEX_AXES_DATA_BYTES == 208
    assert abi.VertexAxesData.LocalAxisSize.offset == 4 * L.CB_SIZE and abi.VertexAxesData.matViewProj.offset == 4 * L.CB_VIEW_PROJ


def test_work_size_function():
    f = capi.load_library().vqhip_line_draws_work_bytes
    assert f(0) == 256 and f(1) == 256 + 256 + 256                                  # four colour entries | one box | one record
    counts = (1, 36, 2304, 18432, 10 ** 6, 2 ** 31 - 1)
    sizes = [f(n) for n in counts]
    assert all(s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    for n, s in zip(counts, sizes):
        lo = 64 * min(n, 20000) + abi.LINE_BYTES * n
        assert lo <= s < lo + 3 * 256
    assert f(2 ** 31 - 1) > 0 and f(2 ** 31) == 0 and f(2 ** 40) == 0
    assert capi.line_draws_work_bytes(18432) == f(18432)


def test_call_without_a_context_is_refused():
    lib = capi.load_library()
    tg = abi.UnlitTargets()
    buf = (C.c_uint8 * 4096)()
    rc = lib.vqhip_line_draws(None, None, None, 0, 16, 16, C.byref(tg), buf, 4096)
    assert rc == abi.VQHIP_ERR_INVALID_ARG and b"ctx is NULL" in lib.vqhip_last_error(None)


def test_mirrors_matrices_colours_and_batching():
    vp = UC.view_proj(64, 40)
    rng = np.random.default_rng(2)
    lo = rng.random((513, 3)) * 4.0 - 2.0
    boxes = [(a, a + rng.random(3) + 0.1) for a in lo]
    draws = LS.bounding_box_draws(boxes, vp)
    assert [d["matrices"].shape[0] for d in draws] == [512, 1] and all(len(d["indices"]) == 36 and d["matrices"].dtype == F for d in draws)
    assert draws[0]["color"].tolist() == [0.0, F(0.8), F(0.2), 0.75] and LS.GAME_OBJECT_BOX_COLOR == (0.0, 0.2, 0.8, 0.75)
    a, b = (np.asarray(v, dtype=F) for v in boxes[512])
    world = S.scaling(((b - a) * F(0.5)).astype(np.float64)) @ S.translation(((b + a) * F(0.5)).astype(np.float64))
    assert np.array_equal(draws[1]["matrices"][0], (world @ vp).astype(F))
    corners = np.asarray(LS.CUBE[0], dtype=np.float64)[:, :3]
    moved = np.concatenate([corners, np.ones((8, 1))], axis=1) @ world
    assert np.allclose(moved[:, :3].min(axis=0), a, atol=1e-6) and np.allclose(moved[:, :3].max(axis=0), b, atol=1e-6), "the cube's corners land on the box's"
    assert LS.bounding_box_draws([], vp) == [] and LS.bounding_box_draws(boxes[:3], vp, LS.GAME_OBJECT_BOX_COLOR)[0]["color"][2] == F(0.8)
    # the wire half of the light bounds: the solid half's meshes and matrices, alpha 0.45 — not 0.0045
    point = {"type": "point", "position": (4.0, 6.0, 9.0), "color": (0.5, 0.0, 2.0), "brightness": 300.0, "range": 7.0}
    spot = {"type": "spot", "position": (0.0, 5.0, 0.0), "color": (1.0, 1.0, 1.0), "brightness": 50.0, "range": 4.0, "outer_cone_degrees": 30.0}
    sun = {"type": "directional", "position": (0.0, 99.0, 0.0), "color": (1.0, 1.0, 1.0), "brightness": 5.0, "range": 1.0}
    sphere = S.uv_sphere(1.0, 8, 6)
    wire = LS.light_bounds_wire_draws([point, sun, dict(point, enabled=False), spot], vp, sphere, cone=sphere)
    solid = US.light_bounds_draws([point, sun, dict(point, enabled=False), spot], vp, sphere, cone=sphere, blended=True)
    assert [d["light"] for d in wire] == [d["light"] for d in solid] == [0, 3]
    for wd, sd in zip(wire, solid):
        assert np.array_equal(wd["matrices"][0], sd["cb"][:16].reshape(4, 4)) and wd["vertices"] is sd["vertices"] and wd["indices"] is sd["indices"]
        assert wd["color"][3] == F(0.45) and sd["cb"][19] == F(F(0.45) * F(0.01)) and np.array_equal(wd["color"][:3], sd["cb"][16:19])
    assert LS.light_bounds_wire_draws([point, spot], vp, sphere) and len(LS.light_bounds_wire_draws([point, spot], vp, sphere)) == 1        # no cone mesh: the spot is skipped
    # the vertex axes: matWorld, matNormal = the inverse transpose, matViewProj, LocalAxisSize; one draw per mesh
    world = S.scaling((1.0, 2.0, 0.5)) @ S.rotation_y(0.3) @ S.translation((1.0, 2.0, 3.0))
    v = np.zeros((4, 9), dtype=F)
    ax = LS.vertex_axes_draws([(v, np.arange(4), world), (v, np.arange(2), np.eye(4))], vp, 0.25)
    assert len(ax) == 2 and ax[0]["cb"].shape == (52,) and ax[0]["cb"].dtype == F and ax[0]["cb"][48] == F(0.25) and not ax[0]["cb"][49:].any()
    st = LS.as_struct(ax[0]["cb"])
    assert np.array_equal(np.array(st.matWorld.m, dtype=F), world.astype(F)) and np.array_equal(np.array(st.matViewProj.m, dtype=F), vp.astype(F))
    nm = np.array(st.matNormal.m, dtype=np.float64)
    assert np.allclose(nm[:3, :3] @ world[:3, :3].T, np.eye(3), atol=1e-6) and nm[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert st.LocalAxisSize == F(0.25)


def test_documents_state_the_pass():
    doc = open(os.path.join(ROOT, "docs", "DESIGN_DETAILS.md")).read()
    assert doc.index("### 7.23") < doc.index("### 7.24")
    section = doc[doc.index("### 7.24"):]
    for word in ("**L1", "**L2", "**L3", "**L4", "**L5", "**L6", "**L7", "**L8", "k_lines_setup", "k_lines_fill", "atomicMax", "-ffp-contract=off", "tests/line_ref.py",
                 "Unpinned", "D3D11.3", "4x MSAA", "FillMode", "ntialiased", "LDS", "VGPR", "profiles/r27a_line_draws.md", "vqhip_line_draws"):
        assert word in section, f"{word} is not stated in §7.24"
    for earlier in ("### 7.16", "### 7.17", "### 7.23"):
        nxt = re.search(r"\n### 7\.\d+", doc[doc.index(earlier) + 8:])
        body = doc[doc.index(earlier):doc.index(earlier) + 8 + nxt.start()]
        assert "vqhip_line_draws" in body, f"{earlier} does not point at the new call"
    calib = open(os.path.join(ROOT, "docs", "WARP_CALIBRATION.md")).read()
    for rule in ("L2", "L5", "L6"):
        assert re.search(rf"§7\.24[^\n]*{rule}|{rule}[^\n]*§7\.24", calib), f"docs/WARP_CALIBRATION.md §5 has no row for {rule}"
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "vqhip_line_draws" in design and "vqhip_line_draws" in readme and "raster_lines.hip" in readme and "line_scene.py" in readme
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for word in ("RenderBoundingBoxes", "RenderLightBounds", "RenderDebugVertexAxes", "WireframePass", "VertexAxesPass"):
        assert word in integ, word
    assert os.path.exists(os.path.join(ROOT, "profiles", "r27a_line_draws.md")) and os.path.exists(os.path.join(ROOT, "scripts", "line_draws_bench.py"))


def test_cpp_adaptor_builds_the_calls_from_the_three_fronts(tmp_path):
    """tests/cpp/test_passes_lines.cpp (vqhip::WireframePass, vqhip::VertexAxesPass) against tests/cpp/mock_engine/, with the command line
    tests/test_unlit_draws_cpu.py uses"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = tmp_path / "test_passes_lines"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    lib = os.path.join(ROOT, "vqengine_amd", "lib")
    r = subprocess.run([hipcc, "-std=c++17", "-O2", "-Wall", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I.", "-I../../include", "-I/opt/rocm/include",
                        "test_passes_lines.cpp", "-o", str(exe), "-L../../vqengine_amd/lib", "-lvqhip", "-L/opt/rocm/lib", "-lamdhip64",
                        f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], cwd=cpp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "line draws adaptor OK" in r.stdout, (r.returncode, r.stdout, r.stderr)
