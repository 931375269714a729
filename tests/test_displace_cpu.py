"""CPU side of vqhip_displace_meshes (docs/DESIGN_DETAILS.md §7.22): tests/displace_ref.py — the numpy statement the GPU tests compare against — pinned to the
oracle's sampler decision by decision, the landing places of the cases' uvs, the non-vacuity of the chain scene, H4's sign of zero, and the host-only pieces
(struct layout against the header, the exported symbol, the documents)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import displace_cases as DC
from tests import displace_ref as D
from tests import masked_depth_ref as M
from tests import oracle_lib as O
from vqengine_amd import abi, capi

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METALNESS_MAP = 1 << 5                                   # HasMetallicMap: metalness *= texMetalness.Sample(..).r (ForwardLighting.hlsl:271)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def oracle_red_samples(jb):
    """the pre-displacement sample of every vertex of a job from the ORACLE's sampler: the height map bound as the metalness map of a material whose metalness
    constant is 1.0 (the product 1.0f * s is exact), the job's uvScaleOffset as the material's (the oracle applies H1's statement), a 2 x 2 quad of equal uv per
    vertex (zero derivatives: LOD 0), read back from the G-buffer's metalness channel (gb2.w)"""
    v = np.asarray(jb["vertices"], F)
    n = v.shape[0]
    ip = [np.zeros((2 * n, 2, 4), F) for _ in range(3)]
    ip[0][..., 3] = np.repeat(v[:, 9], 2)[:, None]
    ip[1][..., 3] = np.repeat(v[:, 10], 2)[:, None]
    ip[1][..., 1], ip[2][..., 0] = 1.0, 1.0               # a normal and a tangent
    ip[2][..., 3] = np.zeros(1, np.int32).view(F)[0]       # material 0 everywhere
    d = abi.MaterialData()
    d.uvScaleOffset = abi.float4(*jb["scale_offset"])
    d.metalness, d.roughness, d.textureConfig = 1.0, 0.5, float(METALNESS_MAP)
    t = jb["heightmap"]
    mats = O.host_materials([d], [{"texMetalness": (t["chain"], t["w"], t["h"], t["mips"])} if t["chain"] is not None else {}])
    with np.errstate(all="ignore"):
        gb = O.gbuffer_from_materials(ip, mats, 1.0)
    return np.ascontiguousarray(gb[2][0::2, 0, 3])


@pytest.mark.parametrize("name", sorted(DC.stream_jobs()))
def test_red_fetch_equals_the_oracles(name):
    """H1 + H2 pinned: uv transform, fixed-point fractions, WRAP, both level_taps forms, the FMA chain, * RN(1/255), level 0 whatever `mips` says, the null SRV"""
    jb = DC.stream_jobs()[name]
    u, v = D.transformed_uv(jb["vertices"], jb["scale_offset"])
    ours = D.sample_level0(jb["heightmap"], u, v)
    assert np.array_equal(bits(ours), bits(oracle_red_samples(jb))), f"{name}: the red-channel level-0 fetch differs from the oracle's sampler"


def test_a_wrong_channel_or_level_would_show():
    jb = DC.stream_jobs()["wrap_8x8_grid9"]
    u, v = D.transformed_uv(jb["vertices"], jb["scale_offset"])
    red = D.sample_level0(jb["heightmap"], u, v)
    for ch in (D.GREEN, D.BLUE, D.ALPHA):
        assert (bits(red) != bits(D.sample_level0(jb["heightmap"], u, v, ch))).mean() > 0.9
    assert np.array_equal(bits(D.sample_level0(jb["heightmap"], u, v, D.ALPHA)), bits(M.sample_alpha_level0(jb["heightmap"], u, v))), "the generalised fetch is M4's on alpha"
    two = DC.stream_jobs()["level0_only_grid9"]
    u, v = D.transformed_uv(two["vertices"], two["scale_offset"])
    lv1 = (D.level_channel(two["heightmap"], 1, u, v, D.RED) * M.RCP255).astype(F)
    assert (bits(D.sample_level0(two["heightmap"], u, v)) != bits(lv1)).mean() > 0.9, "level 1 of the two-level map is nothing like level 0"


def test_uvs_land_where_the_cases_say():
    j = DC.stream_jobs()
    u, v, wx, wy = DC.footprint(j["centres_4x4_grid5"])
    assert ((wx == 0) & (wy == 0)).any(), "a vertex exactly on a texel centre"
    u, v, wx, wy = DC.footprint(j["fraction255_4x4_grid5_s48"])
    assert ((wx == F(255 / 256)) & (wy == F(255 / 256))).any(), "a vertex at fraction 255/256 on both axes"
    for name in ("wrap_8x8_grid9", "wrap_5x3_grid9_s48"):
        u, v, wx, wy = DC.footprint(j[name])
        assert (u < 0).any() and (v >= 1).any(), name
    u, v, wx, wy = DC.footprint(j["one_texel_axis_1x7_grid5"])
    assert (u >= 1).any() and (u < 0).any() and (v < 0).any() and (v >= 1).any()
    for name in ("special_uv_8x8_grid5", "special_uv_5x3_grid5"):
        uv = j[name]["vertices"][:, 9:11]
        assert np.isnan(uv).any() and np.isposinf(uv).any() and np.isneginf(uv).any()
        assert np.isfinite(j[name]["vertices"][:, 1]).all()
    pot = {n for n, jb in j.items() if jb["heightmap"]["chain"] is not None and (jb["heightmap"]["w"] & (jb["heightmap"]["w"] - 1)) == 0 and (jb["heightmap"]["h"] & (jb["heightmap"]["h"] - 1)) == 0}
    npot = {n for n, jb in j.items() if jb["heightmap"]["chain"] is not None} - pot
    assert pot and npot and any(jb["heightmap"]["chain"] is None for jb in j.values()), "both level_taps instantiations and the null SRV"
    assert {jb["vertices"].shape[0] for jb in j.values()} >= {0, 1, 64, 65, 36, 100, 324} and {jb["vertices"].shape[1] for jb in j.values()} == {11, 12}
    assert {jb["displacement"] for jb in j.values()} >= {100.0, 0.0, -2.5} and any(np.signbit(jb["displacement"]) and jb["displacement"] == 0 for jb in j.values())
    assert j["level0_only_grid9"]["heightmap"]["mips"] == 2


@pytest.mark.parametrize("name", sorted(DC.stream_jobs()))
def test_statement_moves_y_alone(name):
    jb = DC.stream_jobs()[name]
    full, compact = DC.stream_expected(name, False), DC.stream_expected(name, True)
    src = bits(jb["vertices"])
    keep = [c for c in range(src.shape[1]) if c != 1]
    assert np.array_equal(bits(full)[:, keep], src[:, keep]) and np.array_equal(bits(full)[:, :3], bits(compact)) and compact.shape[1:] == (3,)
    if jb["displacement"] != 0 and jb["heightmap"]["chain"] is not None and jb["vertices"].shape[0] > 0 and jb["name"] != "zero4":
        assert (bits(full)[:, 1] != src[:, 1]).mean() > 0.5, "most vertices move"
    else:
        assert np.array_equal(D.consumed_y(full[:, 1]).view(np.uint32), D.consumed_y(jb["vertices"][:, 1]).view(np.uint32))


def test_h4_sign_of_zero_is_the_one_deviation():
    """y = -0, sample 0, displacement -0: h = 0 * -0 = -0, the reference's y + h = -0; the stream stores -0 and every consumer's retained + 0.0f reads +0.
    Any other pairing gives +0 (or a non-zero value) on both sides."""
    jb = DC.stream_jobs()["negative_zero_grid5"]
    h = D.height_offsets(jb)
    assert (h == 0).all() and np.signbit(h).all()
    stored = DC.stream_expected("negative_zero_grid5", False)[:, 1]
    ref = D.reference_stage_y(jb["vertices"][:, 1], h)
    assert np.array_equal(bits(stored), bits(ref)) and np.signbit(ref).all(), "the stream itself holds the reference's -0"
    seen = D.consumed_y(stored)
    assert (seen == 0).all() and not np.signbit(seen).any(), "what a rasteriser computes with is +0"
    assert np.array_equal(seen, ref), "equal as numbers: the deviation is the sign bit alone"
    for y, hh in ((F(-0.0), F(0.0)), (F(0.0), F(-0.0)), (F(0.0), F(0.0)), (F(1.5), F(-1.5)), (F(-2.0), F(0.25))):
        r = D.reference_stage_y(y, hh)
        assert bits(D.consumed_y(r)) == bits(r), "no other sum is changed by the retained + 0.0f"
    for name in DC.stream_jobs():
        if name != "negative_zero_grid5":
            y = DC.stream_expected(name, False)[:, 1]
            assert np.array_equal(bits(D.consumed_y(y)), bits(y)), f"{name}: no stored y of the other cases is -0"


# ---- non-vacuity of the chain scene, on the references alone ---------------------------------------------------------------------------------------------------------
def test_the_hill_changes_the_depth_of_a_quarter_of_the_covered_pixels():
    for (w, h, s, layers) in ((64, 48, 1, None), (32, 32, 4, 2)):
        a, b = DC.depth_expected(w, h, s, layers), DC.depth_expected(w, h, s, layers, displaced=False)
        assert DC.changed_fraction(a["depth"], b["depth"]) >= 0.25, (w, h, s)
    a, b = DC.masked_expected(64, 48), DC.masked_expected(64, 48, displaced=False)
    assert DC.changed_fraction(a["depth"], b["depth"]) >= 0.25
    for k, (x, y) in enumerate(zip(DC.shadow_expected(48), DC.shadow_expected(48, displaced=False))):
        assert DC.changed_fraction(x, y) >= 0.25, f"shadow view {k}"


def test_the_hill_hides_part_of_the_card():
    a, b = DC.masked_expected(64, 48), DC.masked_expected(64, 48, displaced=False)
    hill_tris = len(DC.hill_job()["indices"]) // 3
    card_flat = b["primitive"] >= hill_tris
    card_flat &= b["primitive"] != V_NO
    taken = card_flat & (a["primitive"] < hill_tris)
    assert card_flat.sum() > 50 and taken.sum() >= 1, "the hill owns pixels the card owned over the flat grid"
    assert ((a["primitive"] >= hill_tris) & (a["primitive"] != V_NO)).sum() > 20, "the card is still on screen"
    holes = DC.depth_expected(64, 48, 1, None)["primitive"] != a["primitive"]
    assert holes.sum() > 10, "the alpha test removes fragments of the card"


V_NO = np.uint32(0xFFFFFFFF)


def test_the_selected_hill_outlines_differently():
    a, b = DC.outline_expected(64, 48), DC.outline_expected(64, 48, displaced=False)
    assert (a["selection"] != b["selection"]).sum() > 100 and a["selection"].sum() > 200 and (a["writer"] != 0xFFFFFFFF).sum() > 20


def test_ids_and_interpolants_see_both_draws():
    draws, ids = DC.ids_expected(64, 48)
    assert {draws[0]["mesh_id"], draws[1]["mesh_id"]} <= set(np.unique(ids[..., 1]).tolist())
    ip, qp = DC.interp_expected(64, 48)
    mat = ip["ip2"][..., 3].view(np.int32)
    assert {0, 1} <= set(np.unique(mat).tolist()) and np.array_equal(ip["ip0"], qp["ip0"]) and qp["quad_uv"].any()


# ---- host-only pieces -------------------------------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_the_header():
    src = open(os.path.join(ROOT, "include", "vqhip.h")).read()
    body = re.search(r"typedef struct vqhip_displace_job \{(.*?)\} vqhip_displace_job;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [m.group(1) for m in re.finditer(r"(\w+)\s*;", body)]
    assert names == [f[0] for f in abi.DisplaceJob._fields_]
    assert C.sizeof(abi.DisplaceJob) == 80
    for field, off in (("strideBytes", 8), ("numVertices", 12), ("out", 16), ("outStrideBytes", 24), ("reserved", 28), ("heightmap", 32), ("uvScaleOffset", 56),
                       ("displacement", 72)):
        assert getattr(abi.DisplaceJob, field).offset == off and f"offsetof(vqhip_displace_job, {field}) == {off}" in src, field
    assert "sizeof(vqhip_displace_job) == 80" in src
    assert int(re.search(r"#define VQHIP_DISPLACE_MAX_JOBS (\d+)", src).group(1)) == abi.DISPLACE_MAX_JOBS
    assert re.search(r"#define VQHIP_ABI_VERSION 3\b", src) and abi.ABI_VERSION == 3
    declared = set(re.findall(r"VQHIP_API\s+[\w\s\*]+?\b(vqhip_displace\w*)\s*\(", src))
    assert declared == {"vqhip_displace_meshes"} and declared <= set(capi.EXPORTED_SYMBOLS)


def test_refusals_that_need_no_gpu():
    lib = capi.load_library()
    assert lib.vqhip_displace_meshes(None, None, None, 0) == abi.VQHIP_ERR_INVALID_ARG
    assert b"ctx is NULL" in lib.vqhip_last_error(None)


def test_cpp_adaptor_builds_the_call_from_the_pass(tmp_path):
    """tests/cpp/test_passes_displace.cpp (vqhip::HeightmapDisplacementPass) against tests/cpp/mock_engine/, with the command line tests/test_masked_depth_cpu.py uses"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = tmp_path / "test_passes_displace"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    lib = os.path.join(ROOT, "vqengine_amd", "lib")
    r = subprocess.run([hipcc, "-std=c++17", "-O2", "-Wall", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I.", "-I../../include", "-I/opt/rocm/include",
                        "test_passes_displace.cpp", "-o", str(exe), "-L../../vqengine_amd/lib", "-lvqhip", "-L/opt/rocm/lib", "-lamdhip64",
                        f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], cwd=cpp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "heightmap displacement adaptor OK" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_documents_state_the_contract():
    details = open(os.path.join(ROOT, "docs", "DESIGN_DETAILS.md")).read()
    sec = details[details.index("### 7.22"):]
    for word in ("**H1 —", "**H2 —", "**H3 —", "**H4 —", "vqhip_displace_meshes", "tests/displace_ref.py", "LinearSamplerTess", "CalcHeightOffset"):
        assert word in sec, word
    for doc, word in (("README.md", "vqhip_displace_meshes"), ("DESIGN.md", "vqhip_displace_meshes"), ("INTEGRATION.md", "vqhip_displace_meshes"),
                      (os.path.join("docs", "WARP_CALIBRATION.md"), "H2")):
        assert word in open(os.path.join(ROOT, doc)).read(), doc
    for doc in ("DESIGN.md", os.path.join("docs", "DESIGN_DETAILS.md"), os.path.join("include", "vqhip.h")):
        assert "tessellation and heightmap variants" not in open(os.path.join(ROOT, doc)).read(), doc
