"""docs/DESIGN_DETAILS.md §7.20 without a GPU: the boundary (symbols, struct layout against gcc, refusals that need no context, the C++ adaptors against the mock
engine), the validation of the exploded-image construction tests/quad_interp_ref.py rests on, the non-vacuity of the case sets, the inconsistency between the
pre-pass and the lit draw that motivates the work — shown on the oracle — and the identity case."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import masked_depth_ref as M
from tests import oracle_lib as O
from tests import quad_interp_cases as QC
from tests import quad_interp_ref as Q
from tests import scene_interp_ref as I
from vqengine_amd import abi, capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U32 = np.float32, np.uint32
NEW_SYMBOLS = {"vqhip_scene_quad_interpolants", "vqhip_gbuffer_from_materials_quad", "vqhip_forward_lighting_from_materials_quad",
               "vqhip_scene_normals_from_materials_quad"}
RESOLVE_SET = tuple(sorted(QC.cases()))
PRODUCER_SET = QC.PRODUCER_NAMES + tuple(f"cards_{n}" for n in QC.CARD_NAMES)


# ---- the boundary -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    src = open(os.path.join(ROOT, "include", "vqhip.h")).read()
    declared = set(re.findall(r"VQHIP_API\s+[\w\s\*]+?\b(vqhip_\w*_quad\w*)\s*\(", src))
    assert declared == NEW_SYMBOLS
    lib = capi.load_library()
    for s in declared:
        assert s in capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert lib.vqhip_abi_version() == abi.ABI_VERSION == 3                     # additions only
    section = src[src.index("Helper-lane uv derivatives for the lit draw"):]
    for word in ("UNPINNED", "(i ^ 1, j)", "0x7FC00000", "helper", "no image-bounds test", "neighbour rule"):
        assert word in section, f"{word} is not stated in the header section"
    assert src.index("Helper-lane uv derivatives for the lit draw") > src.index("Alpha-tested geometry in the depth pre-pass")
    for m in ("scene_quad_interpolants", "scene_quad_interpolants_prepared", "gbuffer_from_materials_quad", "forward_lighting_from_materials_quad",
              "scene_normals_from_materials_quad"):
        assert callable(getattr(capi.Context, m)), m


def test_struct_layout_equals_the_c_header(tmp_path):
    cname, t = "vqhip_scene_quad_targets", abi.SceneQuadTargets
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "vqhip.h"\nint main(void){\n'
    prog += f'printf("%zu", sizeof({cname}));\n' + "".join(f'printf(" %zu", offsetof({cname}, {n}));\n' for n, _ in t._fields_) + 'printf("\\n");\nreturn 0;}\n'
    (tmp_path / "t.c").write_text(prog)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    line = subprocess.check_output([str(tmp_path / "t")]).decode().strip()
    assert [int(v) for v in line.split()] == [C.sizeof(t)] + [getattr(t, n).offset for n, _ in t._fields_]
    assert C.sizeof(t) == 64 and t.planes.offset == 0 and C.sizeof(abi.SceneInterpolantTargets) == 48


def test_calls_without_a_context_are_refused():
    lib = capi.load_library()
    tg = abi.SceneQuadTargets()
    buf = (C.c_uint8 * 4096)()
    inter, gb = abi.Interpolants(), abi.GBuffer()
    pf, pv = abi.PerFrameData(), abi.PerViewLightingData()
    calls = (lambda: lib.vqhip_scene_quad_interpolants(None, None, None, 0, 16, 16, buf, 0, C.byref(tg), buf, 4096),
             lambda: lib.vqhip_gbuffer_from_materials_quad(None, None, C.byref(inter), None, 0, 0.0, None, C.byref(gb), buf, 0),
             lambda: lib.vqhip_forward_lighting_from_materials_quad(None, None, C.byref(inter), None, 0, None, C.byref(pf), C.byref(pv), None, 0, None, None, buf, 16,
                                                                    abi.FMT_RGBA16F, None, buf, 0),
             lambda: lib.vqhip_scene_normals_from_materials_quad(None, None, C.byref(inter), None, 0, buf, abi.FMT_RGBA32F, 0, buf, 0))
    for call in calls:
        assert call() == abi.VQHIP_ERR_INVALID_ARG and b"ctx is NULL" in lib.vqhip_last_error(None)


def test_cpp_adaptors_build_the_calls_from_the_passes(tmp_path):
    """tests/cpp/test_passes_quad.cpp (vqhip::QuadInterpolantsPass and the lit-draw adaptor it hands quadUV to) against tests/cpp/mock_engine/, with the command
    line tests/test_masked_depth_cpu.py uses"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = tmp_path / "test_passes_quad"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    lib = os.path.join(ROOT, "vqengine_amd", "lib")
    r = subprocess.run([hipcc, "-std=c++17", "-O2", "-Wall", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I.", "-I../../include", "-I/opt/rocm/include",
                        "test_passes_quad.cpp", "-o", str(exe), "-L../../vqengine_amd/lib", "-lvqhip", "-L/opt/rocm/lib", "-lamdhip64",
                        f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], cwd=cpp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "quad adaptors OK" in r.stdout, (r.returncode, r.stdout, r.stderr)


# ---- the construction, proved before anything rests on it --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ssao", [False, True])
def test_the_explosion_returns_the_plain_oracle_on_single_owner_quads(ssao):
    """on frames whose every aligned quad has one owner, exploding the TRUE neighbours' uv returns the plain oracle's output bit for bit — G-buffer, the discard's
    -1 in ip2.w, the pre-pass normals, SSAO included"""
    w, h = 48, 26
    datas, chains = QC.scene_material_inputs()
    mats = O.host_materials(datas, [{slot: (c, ww, hh, n) for slot, (c, n, ww, hh) in cs.items()} for cs in chains])
    mats[1].texDiffuse.reserved = abi.MATERIAL_ALPHA_MASKED                      # a material that discards where its diffuse alpha is low
    ip = QC.single_owner_frame(w, h, 4, 0x720)
    idx = np.ascontiguousarray(ip[2][..., 3]).view(np.int32)
    assert len(np.unique(idx)) >= 4 and (idx < 0).any(), "several materials and pixels without geometry"
    s = QC.ssao_plane(w, h) if ssao else None
    quv, ok = Q.neighbour_quad_uv(ip[0], ip[1])
    assert ok.all()
    plain_ip = [p.copy() for p in ip]
    with np.errstate(all="ignore"):
        want = O.gbuffer_from_materials(plain_ip, mats, 0.055, s)
        want_n = O.scene_normals_from_materials([p.copy() for p in ip], mats, abi.FMT_RGBA32F)
    got, got_idx = Q.gbuffer_from_materials_quad([p.copy() for p in ip], quv, mats, 0.055, s)
    for k in range(4):
        assert O.bits_equal(got[k], want[k])[0] == 0, f"gb{k}"
    assert np.array_equal(got_idx, np.ascontiguousarray(plain_ip[2][..., 3]).view(np.int32))
    assert O.bits_equal(Q.scene_normals_from_materials_quad([p.copy() for p in ip], quv, mats, abi.FMT_RGBA32F), want_n)[0] == 0
    if ssao:
        assert O.bits_equal(got[0], O.gbuffer_from_materials([p.copy() for p in ip], mats, 0.055, None)[0])[0] > 0, "SSAO reaches the record"


def test_quad_uv_is_uv_at_value_for_value():
    """the statement's plane against a direct evaluation, pixel by pixel, on a case with partners outside the image and centres outside the owner"""
    name = "boxes_129x67_s4"
    sc = QC.cases()[name]
    out, _ = QC.expected(name)[1]
    has, attrs, *_ = I.gather(sc, QC.owners(name)[0][1])
    rng = np.random.default_rng(0x720)
    cand = np.argwhere(has)
    picks = [tuple(p) for p in cand[rng.permutation(len(cand))[:200]]] + [tuple(p) for p in cand if p[1] == 128 or p[0] == 66]
    assert any(i == 128 for _, i in picks) and any(j == 66 for j, _ in picks)
    for j, i in picks:
        a = attrs[j, i]
        with np.errstate(all="ignore"):
            h = M.uv_at(a[:, [11, 12, 14]], a[:, 9:11], np.array(i ^ 1), np.array(j), 129, 67)
            v = M.uv_at(a[:, [11, 12, 14]], a[:, 9:11], np.array(i), np.array(j ^ 1), 129, 67)
        want = np.array([h[0], h[1], v[0], v[1]], dtype=F).view(U32)
        assert np.array_equal(out["quad_uv"][j, i], want), (j, i)
    assert not out["quad_uv"][~has].any()
    for k in I.interpolate(sc, QC.owners(name)[0][1]):
        assert np.array_equal(out[k], I.interpolate(sc, QC.owners(name)[0][1])[k])


# ---- non-vacuity ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _lod_moves(name, layer):
    """pixels whose stored G-buffer differs between the two rules while the LOD of the material's diffuse map differs and is above 0 under one of them"""
    sc = QC.cases()[name]
    out, _ = QC.expected(name)[layer]
    gbn, _ = QC.neighbour_gbuffer(name, layer, False)
    gbh, _ = QC.expected_gbuffer(name, layer, False)
    differs = np.zeros(out["ip0"].shape[:2], bool)
    for a, b in zip(gbn, gbh):
        differs |= (a.view(U32) != b.view(U32)).any(axis=-1)
    datas, chains, _ = QC.material_inputs(name)
    idx = np.ascontiguousarray(out["ip2"][..., 3]).view(np.int32)
    u, v = np.ascontiguousarray(out["ip0"][..., 3]).view(F).astype(np.float64), np.ascontiguousarray(out["ip1"][..., 3]).view(F).astype(np.float64)
    nq, ok = Q.neighbour_quad_uv(out["ip0"], out["ip1"])
    H, W = idx.shape
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    same_h = ok & (idx[jj, np.minimum(ii ^ 1, W - 1)] == idx)
    same_v = ok & (idx[np.minimum(jj ^ 1, H - 1), ii] == idx)
    moved = np.zeros_like(differs)
    for k, (d, cs) in enumerate(zip(datas, chains)):
        if "texDiffuse" not in cs or cs["texDiffuse"][1] < 2:
            continue
        _, _, tw, th = cs["texDiffuse"]
        sx, sy = d.uvScaleOffset.x, d.uvScaleOffset.y

        def lod(q, mh, mv):
            q = np.ascontiguousarray(q).view(F).astype(np.float64)
            with np.errstate(all="ignore"):
                dx = np.where(mh, np.hypot((q[..., 0] - u) * sx * tw, (q[..., 1] - v) * sy * th), 0.0)
                dy = np.where(mv, np.hypot((q[..., 2] - u) * sx * tw, (q[..., 3] - v) * sy * th), 0.0)
                return np.log2(np.maximum(np.maximum(dx, dy), 1e-30))
        with np.errstate(all="ignore"):
            ln, lh = lod(nq, same_h, same_v), lod(out["quad_uv"], True, True)
        moved |= (idx == k) & (np.abs(ln - lh) > 1.0 / 256) & (np.maximum(ln, lh) > 0)
    return int((differs & moved).sum())


@pytest.mark.parametrize("which", ["resolve", "producers"])
def test_each_gpu_case_set_holds_every_class_of_pixel(which):
    names = RESOLVE_SET if which == "resolve" else PRODUCER_SET
    total = dict.fromkeys(("same_material", "other_material", "partner_unowned", "outside_x", "outside_y"), 0)
    outside_upper = lod = 0
    for name in names:
        for layer, (_, st) in enumerate(QC.expected(name)):
            for c in total:
                total[c] += st[c]
            if QC.cases()[name]["samples"] == 4 and layer >= 1:
                outside_upper += st["outside"]
    for name in (("room_129x67_s1", "boxes_64x40_s1", "cards_minified_64x48_s1") if which == "producers" else ("room_64x40_s1",)):      # the room's materials bind a mip-chained diffuse map
        lod += _lod_moves(name, 0)
    print(f"{which} set: (a) {total['same_material']}, (b) {total['other_material']}, (c) {total['partner_unowned']}, (d) x {total['outside_x']} y {total['outside_y']}, "
          f"(e) {lod} pixels whose record moves with the LOD, (f) {outside_upper} layer 1..3 pixels with the centre outside the owner")
    assert all(n > 0 for n in total.values()), total
    assert outside_upper > 0 and lod > 0


# ---- the inconsistency that motivates the work ---------------------------------------------------------------------------------------------------------------------------
def test_the_neighbour_rule_disagrees_with_the_pre_pass_and_the_helper_rule_does_not():
    """the minified T O O T card (tests/masked_depth_cases.py: the ground card running away from the camera): at its silhouette the quad partner belongs to the
    wall, the neighbour rule takes a zero derivative there, samples level 0 between two transparent columns and discards a pixel the pre-pass kept"""
    for name, layers in QC.INCONSISTENT.items():
        for layer in layers:
            n, h = QC.disagreements(name, layer)
            print(f"{name} layer {layer}: the neighbour rule discards {n} pixels that own their depth, the helper rule {h}")
            assert n >= 1 and h == 0
    for name in ("cards_magnified_64x48_s1", "cards_magnified_t12_64x48_s1", "cards_magnified_33x17_s4"):       # the helper rule agrees everywhere else too
        for layer in range(len(QC.owners(name)[0])):
            assert QC.disagreements(name, layer)[1] == 0
    doc = open(os.path.join(ROOT, "docs", "DESIGN_DETAILS.md")).read()
    section = doc[doc.index("### 7.20"):]
    assert "minified_64x48" in section and f"**{QC.disagreements('cards_minified_64x48_s1', 0)[0]}**" in section


# ---- the identity case -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_on_single_owner_quads_inside_the_image_the_two_rules_are_one():
    checked = 0
    for name in ("room_64x40_s1", "grid_64x40_s1", "boxes_129x67_s1", "cards_magnified_64x48_s1"):
        out, _ = QC.expected(name)[0]
        q = QC.owners(name)[0][0].astype(np.int64)
        H, W = q.shape
        He, We = H & ~1, W & ~1
        blocks = q[:He, :We].reshape(He // 2, 2, We // 2, 2)
        single = (blocks == blocks[:, :1, :, :1]).all(axis=(1, 3))
        m = np.zeros((H, W), bool)
        m[:He, :We] = np.repeat(np.repeat(single, 2, axis=0), 2, axis=1)
        m &= np.ascontiguousarray(out["ip2"][..., 3]).view(np.int32) >= 0
        nq, ok = Q.neighbour_quad_uv(out["ip0"], out["ip1"])
        assert np.array_equal(out["quad_uv"][m], nq[m]), name
        gbn, _ = QC.neighbour_gbuffer(name, 0, False)
        gbh, _ = QC.expected_gbuffer(name, 0, False)
        for a, b in zip(gbn, gbh):
            assert np.array_equal(a.view(U32)[m], b.view(U32)[m]), name
        checked += int(m.sum())
    assert checked > 5000
