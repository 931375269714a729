"""CPU side of vqhip_outline (docs/DESIGN_DETAILS.md §7.21 O1 .. O6): the numpy statement the GPU tests compare against (tests/outline_ref.py) pinned by a
per-triangle, per-pixel scalar transcription; the vertex stages against a binary64 cross-check; the properties the rules promise (the .xyx swizzle, mark =
silhouette, the outline ring, selections, last writer, depth 1.0, the z planes, the colour bits); and the boundary: symbols, struct layouts against gcc, the
work-size function, the refusal without a context, the host-side producer, the documents, the C++ adaptor against tests/cpp/mock_engine/."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import outline_cases as OC
from tests import outline_ref as R
from tests import scene_depth_ref as V
from tests.test_scene_depth_cpu import _clip, _sat, _snap, _vertex
from vqengine_amd import abi, capi
from vqengine_amd import outline_scene as OS
from vqengine_amd import shadow_scene as S
from vqengine_amd import surface_scene as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, F64 = np.float32, np.float64
NEW_SYMBOLS = {"vqhip_outline", "vqhip_outline_work_bytes"}
EPS = 2.0 ** -24                                  # half an ulp of a binary32 in [1, 2): the relative error of one rounded operation
IDENT = np.eye(4)


# ---- the scalar transcription: one triangle, one pixel, one binary32 operation at a time -------------------------------------------------------------------------
def _matmul(A, B):
    return [[((A[r][0] * B[0][c] + A[r][1] * B[1][c]) + A[r][2] * B[2][c]) + A[r][3] * B[3][c] for c in range(4)] for r in range(4)]


def _extruded(v, WV, NV, Pr):
    """O2 of one vertex (position 3, normal 3): the clip-space position"""
    x, y, z = F(v[0]), F(v[1]) + F(0.0), F(v[2])
    view = [((x * WV[0][j] + y * WV[1][j]) + z * WV[2][j]) + F(1.0) * WV[3][j] for j in range(3)]
    n = [((F(v[3]) * NV[0][j] + F(v[4]) * NV[1][j]) + F(v[5]) * NV[2][j]) + F(0.0) * NV[3][j] for j in range(3)]
    s = (n[0], n[1], n[0])
    length = np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
    e = [view[j] + (s[j] / length) * F(0.5) for j in range(3)]
    return [((e[0] * Pr[0][j] + e[1] * Pr[1][j]) + e[2] * Pr[2][j]) + F(1.0) * Pr[3][j] for j in range(4)]


def _fragments(poly, W, H):
    """(i, j, saturated depth) of every fragment of a clip-space triangle: V2, V3, R4, V5 as tests/test_scene_depth_cpu.py transcribes them, cull NONE"""
    if not all(np.isfinite(c) for v in poly for c in v):
        return
    poly = _clip(poly)
    snapped = [_snap(v, W, H) for v in poly]
    for k in range(len(poly) - 2):
        tri_v = (0, k + 1, k + 2)
        if any(snapped[i] is None for i in tri_v):
            continue
        (x0, y0), (x1, y1), (x2, y2) = (snapped[i] for i in tri_v)
        A = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
        if A == 0:
            continue
        s = 1 if A > 0 else -1
        edges = (((x1, y1), (x2, y2)), ((x2, y2), (x0, y0)), ((x0, y0), (x1, y1)))
        tl = [s * (b[1] - a[1]) < 0 or (b[1] == a[1] and s * (b[0] - a[0]) > 0) for a, b in edges]
        v0, v1, v2 = (poly[i] for i in tri_v)
        z0, z1, z2 = v0[2] / v0[3], v1[2] / v1[3], v2[2] / v2[3]
        for j in range(max(0, min(y0, y1, y2) // 256 - 1), min(H - 1, max(y0, y1, y2) // 256 + 1) + 1):
            for i in range(max(0, min(x0, x1, x2) // 256 - 1), min(W - 1, max(x0, x1, x2) // 256 + 1) + 1):
                px, py = 256 * i + 128, 256 * j + 128
                E = [(a[0] - px) * (b[1] - py) - (b[0] - px) * (a[1] - py) for a, b in edges]
                if all(s * e > 0 or (e == 0 and t_) for e, t_ in zip(E, tl)):
                    b1, b2 = F(E[1]) / F(A), F(E[2]) / F(A)
                    yield i, j, _sat((z0 + b1 * (z1 - z0)) + b2 * (z2 - z0))


def scalar_outline(scene, scene_color):
    W, H = scene["width"], scene["height"]
    marked = np.zeros((H, W), dtype=bool)
    last = np.full((H, W), -1, dtype=np.int64)
    with np.errstate(all="ignore"):
        for d, draw in enumerate(scene["draws"]):
            WV, NV, Pr = R.matrices(draw["cb"])
            WVP = _matmul(WV, Pr)
            v = draw["vertices"]
            for tri in np.asarray(draw["indices"]).reshape(-1, 3):
                if any(i >= v.shape[0] for i in tri):
                    continue
                for i, j, depth in _fragments([_vertex(v[k], WVP) for k in tri], W, H):
                    if depth < 1:
                        marked[j, i] = True
                for i, j, _ in _fragments([_extruded(v[k], WV, NV, Pr) for k in tri], W, H):
                    last[j, i] = d
    out = np.array(scene_color, copy=True)
    writer = np.full((H, W), R.NO_WRITER, dtype=np.uint32)
    for j in range(H):
        for i in range(W):
            if last[j, i] >= 0 and not marked[j, i]:
                writer[j, i] = last[j, i]
                out[j, i] = R.colour_halfs(scene["draws"][last[j, i]]["cb"][R.CB_COLOR:R.CB_COLOR + 4])
    return {"scene_color": out, "selection": marked.astype(np.uint8), "writer": writer}


@pytest.mark.parametrize("name", ["sphere_16x16", "two_boxes_16x16", "two_colours_ab_16x16", "two_colours_ba_64x40", "soup_small"])
def test_statement_equals_the_scalar_transcription(name):
    scene = OC.soup(33, 17, n=300, seed=5) if name == "soup_small" else OC.cases()[name]
    pre = OC.prefill(scene["width"], scene["height"])
    a, b = R.outline(scene, pre), scalar_outline(scene, pre)
    for k in ("scene_color", "selection", "writer"):
        assert np.array_equal(a[k], b[k]), (name, k)
    assert a["selection"].any() and (a["writer"] != R.NO_WRITER).any()


# ---- O1 / O2 against binary64 ------------------------------------------------------------------------------------------------------------------------------------------
def test_vertex_stages_against_a_float64_cross_check():
    """each rounded operation contributes at most 2^-24 of the magnitude it rounds; the bound below sums the magnitudes of all terms of a component (every operand
    taken by absolute value) times the number of operations on its longest path: O1 7 (product) + 7 (mulPoint) = 14; O2 7 (view) + 7 (normal) + 8 (normalize:
    dot 5, root, quotient, with the root's error halved — counted whole) + 2 (E) + 7 (mulPoint) = 31"""
    worst0 = worst1 = 0.0
    for name in ("sphere_64x40", "two_boxes_64x40", "soup_64x40"):
        for draw in OC.cases()[name]["draws"]:
            v = draw["vertices"].astype(F64)
            WV, NV, Pr = (m.astype(F64) for m in R.matrices(draw["cb"]))
            P1 = np.concatenate([v[:, :3], np.ones((len(v), 1))], axis=1)
            clip0, clip1 = R.vertex_stages(draw)
            exact0 = P1 @ (WV @ Pr)
            mag0 = np.abs(P1) @ (np.abs(WV) @ np.abs(Pr))
            n = v[:, 3:6] @ NV[:3, :3]
            s = np.stack([n[:, 0], n[:, 1], n[:, 0]], axis=1)
            length = np.linalg.norm(s, axis=1, keepdims=True)
            ok = length[:, 0] > 1e-3                                                # away from the degenerate normal, where the quotient amplifies without bound
            E1 = np.concatenate([(P1 @ WV)[:, :3] + 0.5 * s / np.where(ok[:, None], length, 1.0), np.ones((len(v), 1))], axis=1)
            exact1 = E1 @ Pr
            mag1 = (np.concatenate([(np.abs(P1) @ np.abs(WV))[:, :3] + 0.5, np.ones((len(v), 1))], axis=1)) @ np.abs(Pr)
            with np.errstate(all="ignore"):
                r0 = np.abs(clip0.astype(F64) - exact0) / (mag0 * EPS)
                r1 = np.abs(clip1.astype(F64) - exact1)[ok] / (mag1[ok] * EPS)
            worst0, worst1 = max(worst0, float(np.nanmax(r0))), max(worst1, float(np.nanmax(r1)))
    print(f"O1: worst error {worst0:.2f} x 2^-24 of the term magnitudes (bound 14); O2: {worst1:.2f} (bound 31)")
    assert worst0 <= 14 and worst1 <= 31


def test_matrix_product_is_the_rounded_product():
    rng = np.random.default_rng(4)
    A, B = rng.normal(size=(4, 4)).astype(F), rng.normal(size=(4, 4)).astype(F)
    got = R.matmul32(A, B)
    want = np.array(_matmul(A, B), dtype=F)
    assert got.dtype == F and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.abs(got.astype(F64) - A.astype(F64) @ B.astype(F64)).max() <= 7 * EPS * (np.abs(A).astype(F64) @ np.abs(B).astype(F64)).max()


# ---- the rules' properties ------------------------------------------------------------------------------------------------------------------------------------------------
def _ident_scene(w, h, vertices, indices, color=OC.ORANGE, normal=None):
    return OC.scene(w, h, [OC.draw(np.asarray(vertices, dtype=F), indices, IDENT, IDENT, IDENT, color, normal=IDENT if normal is None else normal)])


def test_the_xyx_rule():
    """view-space normals (0, 0, +-1): n.xyx = 0, normalize gives NaN, every triangle is dropped and nothing is painted (the mark is there all the same); the same
    mesh under a matNormalView that rotates the normals to x paints"""
    quad = [(-0.5, -0.5, 0.5, 0, 0, -1), (-0.5, 0.5, 0.5, 0, 0, 1), (0.5, 0.5, 0.5, 0, 0, -1), (0.5, -0.5, 0.5, 0, 0, 1)]
    idx = [0, 1, 2, 0, 2, 3]
    sc = _ident_scene(16, 16, quad, idx)
    out = R.outline(sc, OC.prefill(16, 16))
    assert out["selection"].sum() == 64 and (out["writer"] == R.NO_WRITER).all() and np.array_equal(out["scene_color"], OC.prefill(16, 16))
    assert np.isnan(R.vertex_stages(sc["draws"][0])[1]).all()
    turned = _ident_scene(16, 16, quad, idx, normal=S.rotation_y(0.5 * np.pi))      # z -> x (either sign: rows 0 and 2 move by +-0.354 in x and z, apart)
    out = R.outline(turned, OC.prefill(16, 16))
    assert out["selection"].sum() == 64 and (out["writer"] == 0).sum() > 8


def test_sphere_mark_is_the_silhouette_and_the_outline_is_a_ring_around_it():
    for (w, h) in ((64, 40), (129, 67)):
        sc = OC.cases()[f"sphere_{w}x{h}"]
        out = OC.expected(f"sphere_{w}x{h}")
        d = sc["draws"][0]
        WV, _, Pr = R.matrices(d["cb"])
        owner = V.rasterize({"width": w, "height": h, "samples": 1,
                             "draws": [{"positions": d["vertices"], "indices": d["indices"], "wvp": R.matmul32(WV, Pr)[None], "cull": V.CULL_NONE}]})["primitive"]
        marked = out["selection"] == 1
        assert np.array_equal(marked, owner != V.NO_PRIMITIVE) and marked.sum() > 100
        written = out["writer"] != R.NO_WRITER
        assert written.any() and not (written & marked).any()
        # the extrusion moves a vertex by 0.5 in view space; the nearest one is at view z >= 6 - 1.5 - 0.5 = 4
        reach = int(np.ceil(0.5 * max(Pr[0][0] * w / 2, Pr[1][1] * h / 2) / 4.0)) + 1
        jj, ii = np.nonzero(written)
        for j, i in zip(jj, ii):
            assert marked[max(0, j - reach):j + reach + 1, max(0, i - reach):i + reach + 1].any(), (i, j, reach)
        ring = np.zeros_like(marked)                                                # ... and it surrounds the silhouette: every side has written pixels
        cy, cx = (int(round(c)) for c in np.argwhere(marked).mean(axis=0))
        assert written[:cy, cx].any() and written[cy:, cx].any() and written[cy, :cx].any() and written[cy, cx:].any() and not ring.any()


def test_selections():
    for (w, h) in ((64, 40), (129, 67)):
        out = OC.expected(f"two_boxes_{w}x{h}")
        marked = out["selection"] == 1
        assert (out["writer"][marked] == R.NO_WRITER).all() and np.array_equal(out["scene_color"][marked], OC.prefill(w, h)[marked])
        each = [R.planes(OC.scene(w, h, [d]))[0] for d in OC.cases()[f"two_boxes_{w}x{h}"]["draws"]]
        assert np.array_equal(marked, each[0] | each[1]) and (each[0] & each[1]).sum() > 20      # the union; the boxes overlap on screen
        assert {0, 1} <= set(out["writer"].reshape(-1).tolist())
        # two colours: where both extrusions cover an unmarked pixel the later draw's colour lands, in both submission orders
        ab, ba = OC.cases()[f"two_colours_ab_{w}x{h}"], OC.cases()[f"two_colours_ba_{w}x{h}"]
        m, cov = R.planes(ab)
        both = cov[0] & cov[1] & ~m
        assert both.sum() >= 4
        blue, green = R.colour_halfs(OC.BLUE), R.colour_halfs(OC.GREEN)
        oab, oba = OC.expected(f"two_colours_ab_{w}x{h}"), OC.expected(f"two_colours_ba_{w}x{h}")
        assert (oab["writer"][both] == 1).all() and (oab["scene_color"][both] == green).all()        # a = blue first, b = green last
        assert (oba["writer"][both] == 1).all() and (oba["scene_color"][both] == blue).all()         # b first, a last
        assert np.array_equal(oab["selection"], oba["selection"]) and np.array_equal(oab["writer"] != R.NO_WRITER, oba["writer"] != R.NO_WRITER)


def test_a_pass_0_triangle_at_exactly_one_marks_nothing_and_the_paint_behind_it_lands():
    tri = [(-0.8, -0.8, 1.0, -1, 0, 0), (0.0, 0.8, 1.0, -1, 0, 0), (0.8, -0.8, 1.0, -1, 0, 0)]
    out = R.outline(_ident_scene(16, 16, tri, [0, 1, 2]), OC.prefill(16, 16))
    alone = int((out["writer"] == 0).sum())
    assert out["selection"].sum() == 0 and alone > 30                               # moved by (-0.354, 0, -0.354): depth 0.646, inside the frustum
    nearer = [(x, y, 0.999, a, b, c) for (x, y, _, a, b, c) in tri]
    out = R.outline(_ident_scene(16, 16, nearer, [0, 1, 2]), OC.prefill(16, 16))
    assert out["selection"].sum() > 30 and 0 < (out["writer"] == 0).sum() < alone   # the mark now hides most of it: a crescent on the left is what remains


def test_a_triangle_across_both_z_planes_is_cut_in_both_passes():
    """identity matrices, z runs from -1 at the left edge to 2 at the right: the mark keeps the columns where 0 <= z < 1, a third of the width; the paint (normal
    -x: moved left by 0.354 in x and z) keeps the columns where the moved z is in [0, 1]"""
    w, h = 48, 16
    quad = [(-1, -1, -1.0, -1, 0, 0), (-1, 1, -1.0, -1, 0, 0), (1, 1, 2.0, -1, 0, 0), (1, -1, 2.0, -1, 0, 0)]
    sc = _ident_scene(w, h, quad, [0, 1, 2, 0, 2, 3])
    marked, cov = R.planes(sc)
    cols = np.nonzero(marked.any(axis=0))[0]
    assert marked.all(axis=0)[cols].all() and cols.min() == 16 and cols.max() == 31           # z = -1 + 3 (i + 0.5) / 48 in [0, 1)
    pcols = np.nonzero(cov[0].any(axis=0))[0]
    shift = 0.5 / np.sqrt(2.0)                                                                 # x' = x - shift, z' = z - shift; z' = -1 - shift + 3 (x' + shift + 1) / 2
    x_lo, x_hi = (shift + 1.0) * 2 / 3 - shift - 1, (shift + 2.0) * 2 / 3 - shift - 1
    lo_px, hi_px = (x_lo + 1) * 24, (x_hi + 1) * 24                                             # 13.17 and 29.17: the pixel centres i + 0.5 between them
    assert pcols.min() == int(np.ceil(lo_px - 0.5)) == 13 and pcols.max() == int(np.floor(hi_px - 0.5)) == 28 and cov[0].all(axis=0)[pcols].all()
    out, ref = scalar_outline(sc, OC.prefill(w, h)), R.outline(sc, OC.prefill(w, h))
    assert all(np.array_equal(out[k], ref[k]) for k in out)


def test_colour_bits():
    """0, 1, 0.5, a denormal, a negative component (NaN by the contract), an overflow: vqo_pow, then ONE round-to-nearest-even conversion — numpy's, an independent
    implementation, agrees wherever the value is a number"""
    lib = R._lib()
    for color in ((0.0, 1.0, 0.5, 1e-40), (-0.5, 0.25, 2.0, 70000.0), (0.7, 0.9999, 3.0e-5, 12.0)):
        got = R.colour_halfs(color)
        for c, g in zip(color, got):
            p = F(lib.vqo_pow(float(F(c)), float(F(2.2))))
            with np.errstate(all="ignore"):
                want = int(np.array([p]).astype(np.float16).view(np.uint16)[0])
            if np.isnan(p):
                assert int(g) & 0x7FFF == 0x7E00, (c, hex(g))
            else:
                assert int(g) == want, (c, hex(g), hex(want))
    assert R.colour_halfs((0.0, 1.0, 0.5, -1.0)).tolist()[:3] == [0x0000, 0x3C00, int(np.float16(0.5 ** 2.2).view(np.uint16))]
    assert R.colour_halfs((1e-40, 70000.0, 2.0, 0.25)).tolist()[:2] == [0x0000, 0x7C00]
    # the statement writes exactly these bits, all four channels, and nothing else changes
    sc = OC.cases()["sphere_16x16"]
    out = OC.expected("sphere_16x16")
    w = out["writer"] == 0
    assert (out["scene_color"][w] == R.colour_halfs(OC.ORANGE)).all() and np.array_equal(out["scene_color"][~w], OC.prefill(16, 16)[~w]) and sc["draws"][0]["cb"][80] == 1.0


# ---- boundary -----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    src = open(os.path.join(ROOT, "include", "vqhip.h")).read()
    declared = set(re.findall(r"VQHIP_API\s+[\w\s\*]+?\b(vqhip_outline\w*)\s*\(", src))
    assert declared == NEW_SYMBOLS
    lib = capi.load_library()
    for s in declared:
        assert s in capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert lib.vqhip_abi_version() == abi.ABI_VERSION == 3                          # additions only
    section = src[src.index("The Outline pass (selection highlight)"):]
    for word in ("O1", "O2", "O3", "O4", "O5", "O6", ".xyx", "UNPINNED", "SUBMITTED LAST", "IN PLACE", "4x MSAA", "_AlphaMasked", "Magnifier", "2^28"):
        assert word in section, f"{word} is not stated in the header section"


def test_struct_layout_equals_the_c_header(tmp_path):
    structs = (("VQ_OutlineData", abi.OutlineData), ("vqhip_outline_draw", abi.OutlineDraw), ("vqhip_outline_targets", abi.OutlineTargets))
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "vqhip.h"\nint main(void){\n'
    for cname, t in structs:
        prog += f'printf("%zu", sizeof({cname}));\n' + "".join(f'printf(" %zu", offsetof({cname}, {n}));\n' for n, _ in t._fields_) + 'printf("\\n");\n'
    prog += "return 0;}\n"
    (tmp_path / "t.c").write_text(prog)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    lines = subprocess.check_output([str(tmp_path / "t")]).decode().strip().split("\n")
    for (cname, t), line in zip(structs, lines):
        assert [int(v) for v in line.split()] == [C.sizeof(t)] + [getattr(t, n).offset for n, _ in t._fields_], cname
    assert (C.sizeof(abi.OutlineData), C.sizeof(abi.OutlineDraw), C.sizeof(abi.OutlineTargets)) == (abi.OUTLINE_DATA_BYTES, 40, 40) and abi.OUTLINE_DATA_BYTES == 368
    assert (abi.OutlineData.Color.offset, abi.OutlineData.matProj.offset) == (4 * R.CB_COLOR, 4 * R.CB_PROJ)


def test_work_size_function():
    f = capi.load_library().vqhip_outline_work_bytes
    assert f(0) == 512 and f(1) == 512 + 256 + 768                                  # counter | one colour entry | 16 boxes | 16 records
    counts = (1, 12, 240, 2000, 10 ** 6)
    sizes = [f(n) for n in counts]
    assert all(s % 256 == 0 for s in sizes) and sizes == sorted(sizes)
    per = abi.OUTLINE_RECORDS_PER_TRIANGLE * (8 + 48)
    for n, s in zip(counts, sizes):
        lo = 256 + 16 * min(n, 20000) + per * n
        assert lo <= s < lo + 4 * 256
    assert f(2 ** 28 - 1) > 0 and f(2 ** 28) == 0 and f(2 ** 40) == 0
    assert capi.outline_work_bytes(2000) == f(2000)


def test_call_without_a_context_is_refused():
    lib = capi.load_library()
    tg = abi.OutlineTargets()
    buf = (C.c_uint8 * 4096)()
    rc = lib.vqhip_outline(None, None, None, 0, 16, 16, C.byref(tg), buf, 4096)
    assert rc == abi.VQHIP_ERR_INVALID_ARG and b"ctx is NULL" in lib.vqhip_last_error(None)


def test_outline_data_producer():
    world = S.scaling((2.0, 0.5, 3.0)) @ S.rotation_y(0.7) @ S.rotation_x(-0.4) @ S.translation((1.0, 2.0, 3.0))
    view = S.look_at_lh((0.5, 1.0, -4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    proj = S.perspective_fov_lh(1.0, 1.5, 0.1, 10.0)
    cb = OS.outline_data(world, view, proj, (0.1, 0.2, 0.3, 0.4), (2.0, 3.0, 0.5, 0.25), 0.75)
    assert cb.dtype == F and cb.shape == (92,)
    s = OS.as_struct(cb)
    m = lambda x: np.array(x.m, dtype=F)                                            # noqa: E731
    assert np.array_equal(m(s.matWorld), world.astype(F)) and np.array_equal(m(s.matWorldView), (world @ view).astype(F)) and np.array_equal(m(s.matProj), proj.astype(F))
    rot = S.rotation_y(0.7) @ S.rotation_x(-0.4)
    assert np.allclose(m(s.matNormalView), rot @ view, atol=1e-6)                   # normal x view: the rotation alone, no scale, no translation of the object
    assert np.allclose(m(s.matViewInverse).astype(F64) @ view, np.eye(4), atol=1e-5)
    assert (s.Color.x, s.Color.w, s.uvScaleBias.y, s.uvScaleBias.w, s.Scale, s.HeightDisplacement) == (F(0.1), F(0.4), 3.0, 0.25, 1.0, 0.75)
    assert np.array_equal(R.matrices(cb)[0], (world @ view).astype(F)) and np.array_equal(R.matrices(cb)[2], proj.astype(F))
    v, i = SS.uv_sphere(1.5, 12, 10)
    assert v.shape[1] >= 6 and np.allclose(np.linalg.norm(v[:, 3:6], axis=1), 1, atol=1e-6)      # position @0, normal @12


def test_documents_state_the_pass():
    doc = open(os.path.join(ROOT, "docs", "DESIGN_DETAILS.md")).read()
    section = doc[doc.index("### 7.21"):]
    for word in ("**O1", "**O2", "**O3", "**O4", "**O5", "**O6", "`.xyx`", "k_outline_setup", "k_outline_fill", "atomicMax", "atomicOr", "4x MSAA", "tests/outline_ref.py",
                 "Unpinned"):
        assert word in section, f"{word} is not stated in §7.21"
    calib = open(os.path.join(ROOT, "docs", "WARP_CALIBRATION.md")).read()
    for word in ("O1", "O4", "O6"):
        assert re.search(rf"§7\.21[^\n]*{word}|{word}[^\n]*§7\.21", calib), f"docs/WARP_CALIBRATION.md §5 has no row for {word}"
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "vqhip_outline" in design and "vqhip_outline" in open(os.path.join(ROOT, "README.md")).read()
    assert "RenderOutline" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_cpp_adaptor_builds_the_call_from_the_pass(tmp_path):
    """tests/cpp/test_passes_outline.cpp (vqhip::OutlinePass) against tests/cpp/mock_engine/, with the command line tests/test_masked_depth_cpu.py uses"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = tmp_path / "test_passes_outline"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    lib = os.path.join(ROOT, "vqengine_amd", "lib")
    r = subprocess.run([hipcc, "-std=c++17", "-O2", "-Wall", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I.", "-I../../include", "-I/opt/rocm/include",
                        "test_passes_outline.cpp", "-o", str(exe), "-L../../vqengine_amd/lib", "-lvqhip", "-L/opt/rocm/lib", "-lamdhip64",
                        f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], cwd=cpp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "outline adaptor OK" in r.stdout, (r.returncode, r.stdout, r.stderr)
