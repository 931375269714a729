"""docs/DESIGN_DETAILS.md §7.19 without a GPU: tests/masked_depth_ref.py (the numpy statement of vqhip_scene_masked_depth / vqhip_shadow_masked_depth) pinned to the
oracle's sampler decision by decision, its equivalence with the opaque statements when nothing is masked, the non-vacuity of the cases, and the host-only pieces
of the C ABI (work sizes, struct layouts)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import masked_depth_cases as MC
from tests import masked_depth_ref as M
from tests import oracle_lib as O
from tests import scene_depth_cases as SC
from tests import scene_depth_ref as V
from tests import shadow_raster_cases as K
from tests import shadow_raster_ref as R
from vqengine_amd import abi, capi

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN_SCENES = ("magnified_64x48_s1", "magnified_64x48_s4", "magnified_33x17_s1", "magnified_33x17_s4", "magnified_t12_64x48_s1", "tilted_64x48_s1", "tilted_64x48_s4",
               "tilted_33x17_s4", "scale_offset_64x48_s1", "scale_offset_64x48_s4", "scale_offset_t12_64x48_s4", "clipped_64x48_s1", "clipped_64x48_s4",
               "clipped_33x17_s4", "equal_depth_64x48_s1", "equal_depth_64x48_s4", "equal_depth_33x17_s4", "minified_64x48_s1", "minified_64x48_s4")
MAIN_SHADOWS = ("spot_48", "point_32")


def oracle_material(mask, shadow_rule):
    """one vqhip_material over the HOST chain of a case's mask; the shadow rule as the issue pins it: identity scale, the diffuse bit set"""
    d = abi.MaterialData()
    so, cfg = ((1.0, 1.0, 0.0, 0.0), 1.0) if shadow_rule else (mask["scale_offset"], mask["texture_config"])
    d.uvScaleOffset = abi.float4(*so)
    d.textureConfig = cfg
    t = mask["tex"]
    mats = O.host_materials([d], [{"texDiffuse": (t["chain"], t["w"], t["h"], t["mips"])} if t["chain"] is not None else {}])
    mats[0].texDiffuse.reserved = abi.MATERIAL_ALPHA_MASKED
    return mats


def oracle_decisions(probe, shadow_rule):
    """the discard decisions of one probe batch from oracle_lib.scene_normals_from_materials: a 2 x 2 interpolant quad per (primitive, pixel), stacked into a
    2N x 2 plane; RGBA32F output, w == 0 = discarded"""
    i, j = probe["i"].astype(np.int64), probe["j"].astype(np.int64)
    n = i.size
    own = probe["own"]
    hor, ver = (own, own) if shadow_rule else (probe["hor"], probe["ver"])
    ip = [np.zeros((2 * n, 2, 4), F) for _ in range(3)]
    ip[1][..., 2] = 1.0                                              # a normal, so that a surviving fragment writes w = 1
    ip[2][..., 3] = np.zeros(1, np.int32).view(F)[0]                 # material 0 everywhere
    row, col = 2 * np.arange(n) + (j & 1), i & 1
    for (u, v), rr, cc in ((own, row, col), (hor, row, col ^ 1), (ver, row ^ 1, col), (own, row ^ 1, col ^ 1)):
        ip[0][rr, cc, 3], ip[1][rr, cc, 3] = u, v
    out = O.scene_normals_from_materials(ip, oracle_material(probe["mask"], shadow_rule), abi.FMT_RGBA32F)
    return out[row, col, 3] == 0.0


@pytest.mark.parametrize("name", sorted(MC.cases()))
def test_scene_decisions_equal_the_oracles(name):
    """M3 pinned: every (masked primitive, candidate pixel) of the case — uv, helper-lane derivatives, LOD, trilinear WRAP fetch, the 0.01 cut"""
    probes = MC.expected(name)["probes"]
    assert probes
    for p in probes:
        got = oracle_decisions(p, False)
        assert np.array_equal(got, p["discard"]), f"{name} ({p['mask']['name']}): {int((got != p['discard']).sum())} of {got.size} decisions differ from the oracle"


@pytest.mark.parametrize("name", sorted(MC.shadow_cases()))
def test_shadow_decisions_equal_the_oracles(name):
    """M4 pinned: four equal uv values (zero derivatives: level 0), identity scale, the diffuse bit set"""
    probes = MC.shadow_expected(name)["probes"]
    assert probes
    for p in probes:
        got = oracle_decisions(p, True)
        assert np.array_equal(got, p["discard"]), f"{name} ({p['mask']['name']}): {int((got != p['discard']).sum())} of {got.size} decisions differ from the oracle"


def test_the_sampler_meets_every_branch_on_the_cases():
    """levels 0, 1 and beyond, fractional blends, WRAP on both sides, both chain kinds — asserted on the inputs, so that the pinning above means something"""
    seen_neg = seen_big = False
    for name in MC.cases():
        for p in MC.expected(name)["probes"]:
            if "hor" not in p or not M.has_diffuse_map(p["mask"]["texture_config"]):
                continue
            sx, sy, ox, oy = (F(x) for x in p["mask"]["scale_offset"])
            u = p["own"][0] * sx + ox
            seen_neg |= bool((u < 0).any())
            seen_big |= bool((u > 1).any())
    assert seen_neg and seen_big
    lods = []
    for p in MC.expected("minified_64x48_s1")["probes"]:
        du = np.abs(p["hor"][0] - p["own"][0]) * 8
        dv = np.abs(p["ver"][1] - p["own"][1]) * 8
        lods.append(np.log2(np.maximum(np.maximum(du, dv), 1e-9)))
    lods = np.concatenate(lods)
    assert (lods < 0).any() and ((lods > 0) & (lods < 1)).any() and (lods > 1).any()


@pytest.mark.parametrize("name", ["rules_64x40_s1", "rules_64x40_s4", "soup_64x40_s1", "soup_64x40_s4", "boxes_64x40_s4", "room_64x40_s1", "room_16x16_s4",
                                  "pair_ab_64x40_s4", "pair_ba_16x16_s1"])
def test_no_mask_scene_equals_the_opaque_statement(name):
    e = SC.expected(name)
    got = M.rasterize_scene(SC.cases()[name])
    for key in got:
        assert O.bits_equal(np.asarray(got[key]), np.asarray(e[key]))[0] == 0, f"{name} {key}"


@pytest.mark.parametrize("name", ["rules_16", "rules_16_back_linear", "quad_w0_64", "soup_16_back", "soup_64_linear", "boxes128_64", "big_64_linear", "sphere_16_linear"])
def test_no_mask_shadow_equals_the_opaque_statement(name):
    got = M.rasterize_shadow(K.cases()[name])
    for a, b in zip(got, K.expected(name)):
        assert O.bits_equal(a, b)[0] == 0, name


def test_masks_removed_equal_the_opaque_statement_on_the_new_scenes():
    for name in ("variety_64x48_s4", "clipped_33x17_s4"):
        sc = MC.opaque(MC.cases()[name])
        a, b = M.rasterize_scene(sc), V.rasterize(sc)
        for key in a:
            assert np.array_equal(a[key], b[key]), f"{name} {key}"
    v = MC.opaque(MC.shadow_cases()["both"])
    for a, b in zip(M.rasterize_shadow(v), R.rasterize(v)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", MAIN_SCENES + MAIN_SHADOWS)
def test_main_cases_discard_between_a_fifth_and_four_fifths(name):
    st = (MC.shadow_expected(name) if name in MAIN_SHADOWS else MC.expected(name))["stats"]
    rate = st["discarded"] / st["candidates"]
    assert st["candidates"] >= 100 and 0.2 <= rate <= 0.8, (name, st)


def test_what_the_special_cases_are_there_for():
    """on the statement: holes show the wall (q of draw 0); the diffuse bit, the null SRV and the 1 x 1 texture; equal depth goes to the later draw in the holes;
    the minified card moves when the LOD is wrong; the tilted card when the uv is affine; 4x pixels evaluated outside their primitive"""
    e, o = MC.expected("magnified_64x48_s1"), V.rasterize(MC.opaque(MC.cases()["magnified_64x48_s1"]))
    holes = (o["primitive"] >= 2) & (e["primitive"] < 2)
    assert holes.sum() > 200 and (e["depth"][holes] > o["depth"][holes]).all() and (e["primitive"][e["primitive"] >= 2].size > 500)
    f = MC.expected("flags_64x48_s1")["primitive"]
    assert ((f == 2) | (f == 3)).sum() > 100 and not np.isin(f, (4, 5, 6, 7)).any()          # bit clear: kept whole; null SRV and clear texel: gone
    q = MC.expected("equal_depth_64x48_s1")["primitive"]
    assert ((q == 2) | (q == 3)).sum() > 200 and ((q == 0) | (q == 1)).sum() > 400
    sc = MC.cases()["minified_64x48_s1"]
    flat = dict(sc, draws=[sc["draws"][0], dict(sc["draws"][1], mask=dict(sc["draws"][1]["mask"], tex=dict(sc["draws"][1]["mask"]["tex"], mips=1)))])
    assert (M.rasterize_scene(flat)["primitive"] != MC.expected("minified_64x48_s1")["primitive"]).any()           # level 0 alone discards more: the result moves with the LOD
    for name in ("magnified_64x48_s4", "tilted_33x17_s4"):
        sc = MC.cases()[name]
        only = dict(sc, draws=[d for d in sc["draws"] if d["mask"] is not None])
        any4 = V.fill(V.setup(only), only, coverage_count=True).sum(axis=2) > 0
        centre = V.fill(V.setup(dict(only, samples=1)), dict(only, samples=1), coverage_count=True)[:, :, 0] > 0
        assert (any4 & ~centre).sum() >= 8, name                       # evaluated at a centre the primitive does not cover
        cov = MC.expected(name)["coverage"]
        assert ((cov[0] != 0) & (cov[1] != 0)).sum() >= 8, name        # pixels shared by two primitives (card over wall, card over hole)


def test_affine_uv_would_discard_other_pixels():
    sc = MC.cases()["tilted_64x48_s1"]
    d = sc["draws"][1]
    probes = MC.expected("tilted_64x48_s1")["probes"]
    w = np.concatenate([M._vertex_clip(d, 0)[:, 3]])
    assert w.max() / w.min() > 3.9, (w.min(), w.max())
    # screen-space (affine) interpolation = the same triangle with every w forced to 1 after the divide
    diff = 0
    for p in probes:
        idx = np.asarray(d["indices"]).reshape(-1, 3)
        for tri in idx:
            clip = M._vertex_clip(d, 0)[tri]
            ndc = np.stack([clip[:, 0] / clip[:, 3], clip[:, 1] / clip[:, 3], np.ones(3, F)], axis=1).astype(F)
            u_aff, _ = M.uv_at(ndc, d["positions"][tri][:, 9:11], p["i"], p["j"], 64, 48)
            u_per, _ = M.uv_at(clip[:, [0, 1, 3]], d["positions"][tri][:, 9:11], p["i"], p["j"], 64, 48)
            diff = max(diff, float(np.nanmax(np.abs(u_aff - u_per))))
    assert diff > 0.125                      # more than a texel of the 8 x 8 texture


def test_work_sizes_and_layouts():
    lib = capi.load_library()
    base = capi.scene_depth_work_bytes(1000)
    assert capi.scene_masked_depth_work_bytes(1000, 0, 0) == base + 256
    assert capi.scene_masked_depth_work_bytes(1000, 10, 7) == base + 512 + 768
    assert capi.scene_masked_depth_work_bytes(1000, 1001, 7) == 0 and capi.scene_masked_depth_work_bytes(1000, 10, -1) == 0
    assert capi.scene_masked_depth_work_bytes(1 << 29, 0, 1) == 0
    sb = capi.shadow_depth_work_bytes(1000, 3)
    assert capi.shadow_masked_depth_work_bytes(1000, 1000, 3, 6) == sb + 512 + 64000
    assert capi.shadow_masked_depth_work_bytes(1000, 10, 65, 6) == 0 and capi.shadow_masked_depth_work_bytes(10, 11, 1, 1) == 0
    assert abi.MASK_TABLE_ENTRY_BYTES == 48 and abi.MASK_SIDE_RECORD_BYTES == 64
    assert C.sizeof(abi.SceneDepthMaskedDraw) == 56 and C.sizeof(abi.ShadowMaskedDraw) == 64 and C.sizeof(abi.ShadowMaskedView) == C.sizeof(abi.ShadowView)
    assert lib.vqhip_scene_masked_depth and lib.vqhip_shadow_masked_depth


def test_refusals_that_need_no_gpu():
    """ctx NULL is refused before anything else, by both entry points"""
    lib = capi.load_library()
    assert lib.vqhip_scene_masked_depth(None, None, None, 0, 8, 8, 1, None, None, 0) == abi.VQHIP_ERR_INVALID_ARG
    assert lib.vqhip_shadow_masked_depth(None, None, None, 1, None, 0) == abi.VQHIP_ERR_INVALID_ARG


def test_cpp_adaptors_build_the_calls_from_the_passes(tmp_path):
    """tests/cpp/test_passes_masked_depth.cpp (vqhip::MaskedDepthPrePass, vqhip::MaskedShadowDepthPass) against tests/cpp/mock_engine/, with the command line
    tests/test_scene_depth_cpu.py uses"""
    import subprocess
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = tmp_path / "test_passes_masked_depth"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    lib = os.path.join(ROOT, "vqengine_amd", "lib")
    r = subprocess.run([hipcc, "-std=c++17", "-O2", "-Wall", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I.", "-I../../include", "-I/opt/rocm/include",
                        "test_passes_masked_depth.cpp", "-o", str(exe), "-L../../vqengine_amd/lib", "-lvqhip", "-L/opt/rocm/lib", "-lamdhip64",
                        f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], cwd=cpp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "masked depth adaptors OK" in r.stdout, (r.returncode, r.stdout, r.stderr)
