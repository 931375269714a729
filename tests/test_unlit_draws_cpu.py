"""CPU side of vqhip_unlit_draws (docs/DESIGN_DETAILS.md §7.23 U1 .. U7): the fold of the numpy statement the GPU tests compare against (tests/unlit_ref.py) pinned
by an independent binary64-then-round restatement wherever no double rounding can occur; the properties the cases are there for (submission order changes the
bits, two fragments of one draw, the depth producer's own mesh writes nothing, the soup overflows the fill's queue, the special values); the half conversion
against the CPU checker's; Unlit.hlsl's PSMain through the reference shim; and the boundary: symbols, struct layouts against gcc, the work-size function, the
refusal without a context, the host mirror of the two producers, the documents, the C++ adaptor against tests/cpp/mock_engine/."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import oracle_lib as O
from tests import ref_lib as RL
from tests import scene_depth_ref as V
from tests import unlit_cases as UC
from tests import unlit_ref as R
from vqengine_amd import abi, capi
from vqengine_amd import shadow_scene as S
from vqengine_amd import unlit_scene as US

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, F64 = np.float32, np.float64
NEW_SYMBOLS = {"vqhip_unlit_draws", "vqhip_unlit_draws_work_bytes"}
FOLD_CASES = ("sphere_and_box", "two_spheres_ab", "two_spheres_ba", "sphere_cull_none", "crossing_triangle", "veil")      # at most two fragments per pixel


# ---- the fold against binary64 ---------------------------------------------------------------------------------------------------------------------------------------
def _round_half64(x):
    """binary64 -> half bits, one rounding (numpy converts binary64 to binary16 directly, round to nearest even)"""
    with np.errstate(all="ignore"):
        return np.asarray(x, dtype=F64).astype(np.float16).view(np.uint16)


def fold64(scene, prefill):
    """U6 restated independently: per pixel and fragment, the exact products (a binary32 product is exact in binary64), their binary64 sum, ONE rounding to half.
    Agrees with the binary32 path unless the sum lies within that path's rounding error of a boundary between two halfs; `unsafe` marks the pixels where some
    fragment might. Returns (half bits uint16 [H, W, 4], unsafe bool [H, W], fragments int [H, W])."""
    W, H = scene["width"], scene["height"]
    rec = R.records(scene)
    depth = np.asarray(scene["depth"], dtype=F)
    with np.errstate(all="ignore"):
        val = np.array(prefill, copy=True).view(np.float16).astype(F64)
    unsafe = np.zeros((H, W), dtype=bool)
    count = np.zeros((H, W), dtype=np.int64)
    colours = [np.asarray(d["cb"], dtype=F).reshape(-1)[R.CB_COLOR:R.CB_COLOR + 4].astype(F64) for d in scene["draws"]]
    for r in range(rec["xy"].shape[0]):
        j0, j1, i0, i1, passing = R.fragments(rec, r, depth)
        if not passing.any():
            continue
        s = colours[int(rec["draw"][r])]
        a = s[3]
        ia = F64(F(F(1.0) - F(a)))                                 # 1.0f - a is one binary32 operation in both statements
        box = (slice(j0, j1 + 1), slice(i0, i1 + 1))
        with np.errstate(all="ignore"):
            d = val[box]
            new = d.copy()
            risky = np.zeros(passing.shape, dtype=bool)
            for c in range(3):
                p1, p2 = s[c] * a, d[..., c] * ia
                v = p1 + p2
                # how far the binary32 path can be from v: what its three roundings discard (nothing where they are exact — a half times 0.5 plus a
                # short constant lands exactly ON a boundary between two halfs as often as not, and both paths then break the tie alike)
                r1, r2 = np.asarray(p1, dtype=F64).astype(F).astype(F64), np.asarray(p2, dtype=F64).astype(F).astype(F64)
                t = r1 + r2
                err = np.abs(r1 - p1) + np.abs(r2 - p2) + np.abs(t.astype(F).astype(F64) - t)
                lo, hi = _round_half64(v - err), _round_half64(v + err)
                risky |= (lo != hi) & np.isfinite(v)
                new[..., c] = _round_half64(v).view(np.float16).astype(F64)
            new[..., 3] = _round_half64(a).view(np.float16).astype(F64)
        val[box] = np.where(passing[..., None], new, d)
        unsafe[box] |= passing & risky
        count[box] += passing
    with np.errstate(all="ignore"):
        bits = np.where(np.isnan(val), np.uint16(R.NAN_HALF), val.astype(np.float16).view(np.uint16)).astype(np.uint16)
    return bits, unsafe, count


def test_fold_equals_the_binary64_restatement():
    """every pixel the blend touches, in the cases with at most two fragments per pixel at every size, except those where a fragment's sum lies within the
    binary32 path's error of a half boundary (double rounding possible): at most 1 % of the touched pixels are left out"""
    touched_all = left_out = 0
    for name in (f"{b}_{w}x{h}" for (w, h) in UC.SIZES for b in FOLD_CASES):
        sc = UC.cases()[name]
        ref = UC.expected(name, True)
        bits, unsafe, count = fold64(sc, UC.prefill(sc["width"], sc["height"]))
        touched = ref["writer"] != R.NO_WRITER
        assert np.array_equal(count, ref["stats"]["fragments"]) and np.array_equal(count > 0, touched), name
        check = touched & ~unsafe
        assert np.array_equal(bits[check], ref["scene_color"][check]), name
        touched_all += int(touched.sum())
        left_out += int((touched & unsafe).sum())
    share = left_out / touched_all
    print(f"fold vs binary64: {touched_all} touched pixels, {left_out} left out ({100 * share:.3f} %)")
    assert touched_all > 20000 and share <= 0.01


def test_half_conversion_equals_the_checkers():
    """tests/unlit_ref.to_half (numpy's conversion) against oracle/'s vqo_f32_to_f16 on every special value the cases use and a seeded sweep across the half range"""
    lib = O.load()
    rng = np.random.default_rng(5)
    x = np.concatenate([np.array([0.0, -0.0, 1e-8, 6e-8, 5.9e-8, 2.98e-8, 2.99e-8, -1e-40, 3.0e-5, 65504.0, 65519.0, 65520.0, 70000.0, -70000.0, np.inf, -np.inf, 1.0, 0.0045], dtype=F),
                        (rng.standard_normal(4000) * np.exp2(rng.integers(-26, 17, 4000))).astype(F)])
    want = np.empty(x.shape, dtype=np.uint16)
    lib.vqo_f32_to_f16(x.ctypes.data, want.ctypes.data, x.size)
    assert np.array_equal(R.to_half(x), want)
    nan = np.array([np.nan, -np.nan], dtype=F)
    assert [int(v) & 0x7FFF for v in R.opaque_halfs([nan[0], nan[1], 1.0, 2.0])[:2]] == [0x7E00, 0x7E00]
    assert R.opaque_halfs(np.array([0x7FC00000, 0xFFC00001, 0x3F800000, 0xBF800000], dtype=np.uint32).view(F)).tolist() == [0x7E00, 0xFE00, 0x3C00, 0xBC00]   # U5 keeps the sign
    assert R.store_blend(np.array([np.nan, -np.nan, 1.0, np.inf], dtype=F)).tolist() == [0x7E00, 0x7E00, 0x3C00, 0x7C00]                                     # U6 clears it


# ---- what the cases are there for ----------------------------------------------------------------------------------------------------------------------------------
def test_submission_order_changes_the_blend_and_the_writer():
    for (w, h) in UC.SIZES:
        ab, ba = UC.expected(f"two_spheres_ab_{w}x{h}", True), UC.expected(f"two_spheres_ba_{w}x{h}", True)
        both = ab["stats"]["fragments"] == 2
        assert np.array_equal(ab["stats"]["fragments"], ba["stats"]["fragments"]) and both.sum() > 10
        differ = (ab["scene_color"] != ba["scene_color"]).any(axis=-1)
        assert differ[both].mean() > 0.9 and not differ[~both].any(), "the fold must depend on the order exactly where two fragments meet"
        assert ((ab["writer"] == 1) & both).sum() == both.sum() and ((ba["writer"] == 1) & both).sum() == both.sum()       # the later draw, whichever sphere it is
        oa, ob = UC.expected(f"two_spheres_ab_{w}x{h}", False), UC.expected(f"two_spheres_ba_{w}x{h}", False)
        assert (oa["scene_color"][both] != ob["scene_color"][both]).any(axis=-1).all()                                     # U5: the largest q wins


def test_cull_none_sphere_blends_twice():
    for (w, h) in UC.SIZES:
        name = f"sphere_cull_none_{w}x{h}"
        frag = UC.expected(name, True)["stats"]["fragments"]
        assert frag.max() == 2 and (frag == 2).sum() > 0.9 * (frag > 0).sum() > 30
        once = dict(UC.cases()[name], draws=[dict(UC.cases()[name]["draws"][0], cull=abi.CULL_BACK)])
        one = R.unlit_draws(once, UC.prefill(w, h), True)
        two = frag == 2
        assert (one["scene_color"][two] != UC.expected(name, True)["scene_color"][two]).any(axis=-1).mean() > 0.6      # the prefill's NaN and inf pixels stay what they are


def test_own_mesh_writes_nothing_where_it_is_the_visible_surface():
    for (w, h) in UC.SIZES:
        name = f"own_mesh_{w}x{h}"
        sc = UC.cases()[name]
        prim = V.rasterize(R.depth_scene({"width": w, "height": h, "draws": [sc["producer"]]}))["primitive"]
        own = prim != V.NO_PRIMITIVE
        assert own.sum() > 1 and sc["draws"][0]["cull"] == abi.CULL_NONE and np.array_equal(sc["draws"][0]["cb"], sc["producer"]["cb"])
        for blend in (False, True):
            out = UC.expected(name, blend)
            assert (out["writer"][own] == R.NO_WRITER).all() and np.array_equal(out["scene_color"][own], UC.prefill(w, h)[own])
        # the coverage is there: against a cleared depth the same draw writes every one of those pixels
        free = R.unlit_draws(dict(sc, depth=UC.clear_depth(w, h)), UC.prefill(w, h), False)
        assert (free["writer"][own] == 0).all()


def test_soup_overflows_the_queue_inside_one_tile():
    for (w, h) in UC.SIZES:
        name = f"soup_{w}x{h}"
        sc = UC.cases()[name]
        assert UC.triangles(sc) >= 3000 and len(sc["draws"]) == 7
        assert {float(F(d["cb"][R.CB_COLOR + 3])) for d in sc["draws"]} == {float(F(a)) for a in (0.0, 0.0045, 0.5, 1.0, 1.5, -0.25)}
        rec = R.records(sc)
        assert rec["box"][:, 1].max() < 32 and rec["box"][:, 3].max() < 32, "every record lies inside the first 32 x 32 tile"
        assert rec["xy"].shape[0] > abi.UNLIT_QUEUE_CAPACITY * 8
        frag = UC.expected(name, True)["stats"]["fragments"]
        assert frag.max() >= 20 and len(np.unique(UC.expected(name, True)["writer"])) >= 4                                 # several draws are some pixel's last writer
    src = open(os.path.join(ROOT, "include", "vqhip.h")).read()
    assert int(re.search(r"#define\s+VQHIP_UNLIT_QUEUE_CAPACITY\s+(\d+)", src).group(1)) == abi.UNLIT_QUEUE_CAPACITY


def test_crossing_triangle_is_clipped_by_w_and_both_z_planes():
    sc = UC.cases()["crossing_triangle_64x40"]
    d = R.depth_scene(sc)["draws"][0]
    clip = R.f32(d["positions"]) @ d["wvp"][0][:3] + d["wvp"][0][3]
    assert (clip[:, 3] < 0).any() and (clip[:, 2] < 0).any() and (clip[:, 2] > clip[:, 3]).any()
    out = UC.expected("crossing_triangle_64x40", True)
    assert (out["writer"] == 0).sum() > 100 and (out["stats"]["fragments"] == 2).sum() > 10


def test_special_colours_and_prefill():
    for (w, h) in UC.SIZES:
        o = UC.expected(f"special_colours_{w}x{h}", False)
        assert (o["writer"] != R.NO_WRITER).all()
        for k, c in enumerate(UC.SPECIAL_COLOURS):
            px = o["scene_color"][o["writer"] == k]
            assert len(px) and (px == R.opaque_halfs(c)).all()
        assert R.opaque_halfs(UC.SPECIAL_COLOURS[0]).tolist() == [0x7C00, 0xFC00, 0x7E00, 0x8000]
        assert R.opaque_halfs(UC.SPECIAL_COLOURS[1]).tolist() == [0x7C00, 0xFC00, 0x7C00, 0x7BFF]
        b = UC.expected(f"special_colours_{w}x{h}", True)["scene_color"]
        assert ((b & 0x7FFF) > 0x7C00).any() and not (((b & 0x7FFF) > 0x7C00) & (b != R.NAN_HALF)).any(), "a blended NaN is 0x7E00, sign cleared"
        pre = UC.prefill(w, h)
        if w * h >= 19 * 13:
            for word in (0x0001, 0x83FF, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7C01):
                assert (pre == word).any(), hex(word)
        v = UC.expected(f"veil_{w}x{h}", True)
        assert (v["writer"] != R.NO_WRITER).all() and (v["scene_color"][..., 3] == R.to_half(F(0.5))).sum() + (v["scene_color"][..., 3] == R.to_half(F(0.0045))).sum() == w * h


@pytest.mark.skipif(not RL.available("shaders"), reason="oracle/_ref is built only where the reference tree exists")
def test_reference_unlit_psmain_returns_the_constant():
    """Unlit.hlsl:PSMain through the shim of oracle/_ref: the colour a fragment writes is the cbuffer's, bit for bit — what U5 stores and U6 folds"""
    lib = RL.load()
    for c in UC.SPECIAL_COLOURS[1:3] + (UC.RED, UC.TEAL):
        a, o = np.asarray(c, F), np.zeros(4, F)
        lib.vqref_unlit_color(a.ctypes.data, o.ctypes.data)
        assert np.array_equal(a.view(np.uint32), o.view(np.uint32))


# ---- boundary -----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    src = open(os.path.join(ROOT, "include", "vqhip.h")).read()
    declared = set(re.findall(r"VQHIP_API\s+[\w\s\*]+?\b(vqhip_unlit_draws\w*)\s*\(", src))
    assert declared == NEW_SYMBOLS
    lib = capi.load_library()
    for s in declared:
        assert s in capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert lib.vqhip_abi_version() == abi.ABI_VERSION == 3                          # additions only
    section = src[src.index("---- Unlit draws: the light gizmo meshes"):]
    for word in ("U1", "U2", "U3", "U4", "U5", "U6", "U7", "UNPINNED", "IN PLACE", "WITHOUT depth writes", "ascending q", "0x7E00", "WIREFRAME", "RenderDebugVertexAxes",
                 "4x MSAA", "instanced cbuffer", "2^28", "VQHIP_UNLIT_QUEUE_CAPACITY", 'sizeof(VQ_UnlitData) == 80', 'sizeof(vqhip_unlit_draw) == 48',
                 'sizeof(vqhip_unlit_targets) == 40'):
        assert word in section, f"{word} is not stated in the header section"
    assert "vqhip_unlit_draws" in src[src.index("Light gizmo meshes"):src.index("VQHIP_API int vqhip_unlit_composite")]
    assert "vqhip_unlit_draws" in src[src.index("Replaces VQRenderer::CompositeReflections"):src.index("VQHIP_API int vqhip_composite_reflections")]


def test_struct_layout_equals_the_c_header(tmp_path):
    structs = (("VQ_UnlitData", abi.UnlitData), ("vqhip_unlit_draw", abi.UnlitDraw), ("vqhip_unlit_targets", abi.UnlitTargets))
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "vqhip.h"\nint main(void){\n'
    for cname, t in structs:
        prog += f'printf("%zu", sizeof({cname}));\n' + "".join(f'printf(" %zu", offsetof({cname}, {n}));\n' for n, _ in t._fields_) + 'printf("\\n");\n'
    prog += "return 0;}\n"
    (tmp_path / "t.c").write_text(prog)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    lines = subprocess.check_output([str(tmp_path / "t")]).decode().strip().split("\n")
    for (cname, t), line in zip(structs, lines):
        assert [int(v) for v in line.split()] == [C.sizeof(t)] + [getattr(t, n).offset for n, _ in t._fields_], cname
    assert (C.sizeof(abi.UnlitData), C.sizeof(abi.UnlitDraw), C.sizeof(abi.UnlitTargets)) == (abi.UNLIT_DATA_BYTES, 48, 40) and abi.UNLIT_DATA_BYTES == 80
    assert abi.UnlitData.color.offset == 4 * R.CB_COLOR


def test_work_size_function():
    f = capi.load_library().vqhip_unlit_draws_work_bytes
    assert f(0) == 256 and f(1) == 256 + 256 + 256 + 512                            # one colour entry | one triangle box | 8 boxes | 8 records
    counts = (1, 12, 240, 3080, 10 ** 6)
    sizes = [f(n) for n in counts]
    assert all(s % 256 == 0 for s in sizes) and sizes == sorted(sizes)
    per = abi.UNLIT_SLOTS_PER_TRIANGLE * (8 + 48) + 8
    for n, s in zip(counts, sizes):
        lo = 32 * min(n, 20000) + per * n
        assert lo <= s < lo + 4 * 256
    assert f(2 ** 28 - 1) > 0 and f(2 ** 28) == 0 and f(2 ** 40) == 0
    assert capi.unlit_draws_work_bytes(3080) == f(3080)


def test_call_without_a_context_is_refused():
    lib = capi.load_library()
    tg = abi.UnlitTargets()
    buf = (C.c_uint8 * 4096)()
    rc = lib.vqhip_unlit_draws(None, None, None, 0, 16, 16, 0, C.byref(tg), buf, 4096)
    assert rc == abi.VQHIP_ERR_INVALID_ARG and b"ctx is NULL" in lib.vqhip_last_error(None)


def test_light_mirror_colours_and_matrices():
    cam = (1.0, 2.0, -3.0)
    point = {"type": "point", "position": (4.0, 6.0, 9.0), "color": (0.5, 0.0, 2.0), "brightness": 300.0, "range": 7.0}
    spot = {"type": "spot", "position": (0.0, 5.0, 0.0), "color": (1.0, 1.0, 1.0), "brightness": 50.0, "range": 4.0, "outer_cone_degrees": 30.0}
    sun = {"type": "directional", "position": (0.0, 99.0, 0.0), "color": (1.0, 1.0, 1.0), "brightness": 5.0, "range": 1.0}
    off = dict(point, enabled=False)
    dist_sq = F(F(F(9.0) + F(16.0)) + F(144.0))
    ab = F(F(300.0) * F(F(1.0) / dist_sq))
    # the precedence case: `Color.x * bAttenuateLight ? attenuatedBrightness : 1.0f` SELECTS; a zero channel selects 1.0f, a non-zero one the brightness
    assert US.light_mesh_color(point, cam).tolist() == [ab, F(1.0), ab, F(1.0)]
    assert US.light_mesh_color(point, cam, attenuate=False).tolist() == [1.0, 1.0, 1.0, 1.0]
    assert US.light_mesh_color(dict(point, color=(-0.0, np.nan, 1e-45)), cam).tolist() == [1.0, ab, ab, 1.0]               # -0 is zero, NaN and a denormal are not
    vp = UC.view_proj(64, 40)
    sphere = S.uv_sphere(1.0, 8, 6)
    draws = US.light_mesh_draws([point, sun, off, spot], cam, vp, sphere)
    assert [d["light"] for d in draws] == [0, 3] and all(d["cb"].shape == (20,) and d["cb"].dtype == F for d in draws)
    world = S.scaling((0.1,) * 3) @ S.translation(point["position"])
    assert np.array_equal(draws[0]["cb"][:16].reshape(4, 4), (world @ vp).astype(F)) and draws[0]["cb"][16:].tolist() == [ab, F(1.0), ab, F(1.0)]
    st = US.as_struct(draws[0]["cb"])
    assert (st.color.x, st.color.w) == (ab, 1.0) and np.array_equal(np.array(st.matModelViewProj.m, dtype=F), (world @ vp).astype(F))
    # the bounds: the light's colour with alpha 0.45, the sphere scaled by Range; color.w *= 0.01f on the blended path only
    assert US.light_bounds_color(point, False).tolist() == [0.5, 0.0, 2.0, F(0.45)]
    assert US.light_bounds_color(point, True).tolist() == [0.5, 0.0, 2.0, F(F(0.45) * F(0.01))]
    b = US.light_bounds_draws([point, sun, off, spot], vp, sphere, cone=None, blended=True)
    assert [d["light"] for d in b] == [0]                                                                                   # no cone mesh: the spot is skipped
    assert np.array_equal(b[0]["cb"][:16].reshape(4, 4), (S.scaling((7.0,) * 3) @ S.translation(point["position"]) @ vp).astype(F))
    b = US.light_bounds_draws([point, sun, off, spot], vp, sphere, cone=sphere)
    assert [d["light"] for d in b] == [0, 3] and b[1]["cb"][19] == F(0.45)
    cw = US.light_bounds_world(spot)
    base = np.tan(np.radians(30.0)) * 4.0
    tip, rim = np.array([0.0, 1.0, 0.0, 1.0]) @ cw, np.array([1.0, 0.0, 0.0, 1.0]) @ cw                                     # the unit cone: tip at y = 1, base circle at y = 0
    assert np.allclose(tip[:3], spot["position"], atol=1e-5)                                                                # the tip sits at the light
    assert np.isclose(np.linalg.norm(rim[:3] - np.array(spot["position"])), np.hypot(4.0, base), rtol=1e-5)                 # the rim lies Range along the axis, base radius off it
    assert US.light_bounds_world(sun) is None


def test_documents_state_the_pass():
    doc = open(os.path.join(ROOT, "docs", "DESIGN_DETAILS.md")).read()
    section = doc[doc.index("### 7.23"):]
    for word in ("**U1", "**U2", "**U3", "**U4", "**U5", "**U6", "**U7", "k_unlit_setup", "k_unlit_fill", "8 q + k", "VQHIP_UNLIT_QUEUE_CAPACITY", "-ffp-contract=off",
                 "tests/unlit_ref.py", "Unpinned", "WIREFRAME", "RenderDebugVertexAxes", "4x MSAA", "instanced cbuffer", "LDS", "VGPR", "profiles/r25a_unlit_draws.md"):
        assert word in section, f"{word} is not stated in §7.23"
    calib = open(os.path.join(ROOT, "docs", "WARP_CALIBRATION.md")).read()
    assert re.search(r"§7\.23[^\n]*U6|U6[^\n]*§7\.23", calib), "docs/WARP_CALIBRATION.md §5 has no row for U6"
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "vqhip_unlit_draws" in design and "vqhip_unlit_draws" in open(os.path.join(ROOT, "README.md")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "RenderLightBounds" in integ and "UnlitDrawsPass" in integ
    assert os.path.exists(os.path.join(ROOT, "profiles", "r25a_unlit_draws.md"))


def test_cpp_adaptor_builds_the_calls_from_the_two_fronts(tmp_path):
    """tests/cpp/test_passes_unlit.cpp (vqhip::UnlitDrawsPass) against tests/cpp/mock_engine/, with the command line tests/test_displace_cpu.py uses"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = tmp_path / "test_passes_unlit"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    lib = os.path.join(ROOT, "vqengine_amd", "lib")
    r = subprocess.run([hipcc, "-std=c++17", "-O2", "-Wall", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I.", "-I../../include", "-I/opt/rocm/include",
                        "test_passes_unlit.cpp", "-o", str(exe), "-L../../vqengine_amd/lib", "-lvqhip", "-L/opt/rocm/lib", "-lamdhip64",
                        f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], cwd=cpp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "unlit draws adaptor OK" in r.stdout, (r.returncode, r.stdout, r.stderr)
