"""CPU side of vqhip_ssr_classify / vqhip_ssr_intersect (docs/DESIGN_DETAILS.md §7.11): the boundary declares and exports both symbols; the numpy statement
(tests/ssr_trace_ref.py) against a per-lane transcription of ClassifyTiles on hand-made 16 x 16 frames, PackRayCoords, hand-made marches, and the coverage
floors of synth.ssr_room at 1280 x 720 as exact numbers. The GPU side: tests/test_gpu_ssr_trace.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import depth_ref
from tests import oracle_lib as O
from tests import ref_cases
from tests import ssr_trace_ref as R
from vqengine_amd import abi, capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---- the boundary -------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_have_both_entry_points():
    header = open(os.path.join(ROOT, "include", "vqhip.h")).read()
    lib = capi.load_library()
    for s in ("vqhip_ssr_classify", "vqhip_ssr_intersect"):
        assert re.search(r"VQHIP_API\s+int\s+" + s + r"\s*\(vqhip_ctx\* ctx, void\* stream,", header), s
        assert s in capi.EXPORTED_SYMBOLS and hasattr(lib, s)
        assert getattr(lib, s).argtypes is not None and getattr(lib, s).restype is C.c_int
    assert hasattr(capi.Context, "ssr_classify") and hasattr(capi.Context, "ssr_intersect")
    assert lib.vqhip_abi_version() == 3
    # the two comments that called the traced rays out of scope now name only the denoiser
    assert "the traced rays are FidelityFX SSSR: out of scope" not in header and "FidelityFX SSSR + denoiser, is out of scope" not in header


def test_calls_without_a_context_are_refused():
    lib = capi.load_library()
    cb = synth.ssr_constants(16, 16, 1)
    assert lib.vqhip_ssr_classify(None, None, None, abi.FMT_RGBA16F, 0, None, 0, None, 0, cb, None, None, None) == abi.VQHIP_ERR_INVALID_ARG
    assert b"ctx is NULL" in lib.vqhip_last_error(None)
    assert lib.vqhip_ssr_intersect(None, None, None, None, None, abi.FMT_RGBA16F, 0, None, None, abi.FMT_RGBA32F, 0, None, None, cb, None, None, abi.FMT_RGBA16F, 0) \
        == abi.VQHIP_ERR_INVALID_ARG


# ---- PackRayCoords / RemapLane8x8 ---------------------------------------------------------------------------------------------------------------
def test_pack_ray_coords_round_trip_and_lane_remap():
    rng = np.random.default_rng(1)
    for _ in range(200):
        x, y = int(rng.integers(0, 4096)), int(rng.integers(0, 4096))
        fl = tuple(bool(b) for b in rng.integers(0, 2, 3))
        p = abi.pack_ray_coords(x, y, *fl)
        assert 0 <= p < 2 ** 32 and abi.unpack_ray_coords(p) == (x, y) + fl
    assert abi.pack_ray_coords(0x7FFF, 0x3FFF, True, True, True) == 0xFFFFFFFF
    assert abi.pack_ray_coords(5, 3) == (3 << 15) | 5 and abi.pack_ray_coords(0, 0, copy_horizontal=True) == 1 << 29
    assert abi.pack_ray_coords(0, 0, copy_vertical=True) == 1 << 30 and abi.pack_ray_coords(0, 0, copy_diagonal=True) == 1 << 31
    # the table of ffx_denoiser_reflections_common.h:38-47: row 0 = lanes 00 01 08 09 10 11 18 19, row 1 = 02 03 0a 0b 12 13 1a 1b
    grid = np.zeros((8, 8), np.int64)
    for lane in range(64):
        x, y = abi.ssr_remap_lane8x8(lane)
        grid[y, x] = lane
    assert grid[0].tolist() == [0x00, 0x01, 0x08, 0x09, 0x10, 0x11, 0x18, 0x19] and grid[1].tolist() == [0x02, 0x03, 0x0A, 0x0B, 0x12, 0x13, 0x1A, 0x1B]
    assert sorted(grid.ravel().tolist()) == list(range(64))
    for lane in range(0, 64, 4):                                   # four neighbouring lanes are one 2 x 2 quad: l^1 across x, l^2 across y, l^3 diagonal
        x, y = abi.ssr_remap_lane8x8(lane)
        assert x % 2 == 0 and y % 2 == 0
        assert [abi.ssr_remap_lane8x8(lane ^ k) for k in (1, 2, 3)] == [(x + 1, y), (x, y + 1), (x + 1, y + 1)]
    assert np.array_equal(R.LANE_X, [abi.ssr_remap_lane8x8(l)[0] for l in range(64)]) and np.array_equal(R.LANE_Y, [abi.ssr_remap_lane8x8(l)[1] for l in range(64)])


# ---- classification -------------------------------------------------------------------------------------------------------------------------------
def classify_by_lane(scene, depth, cb, variance=None):
    """ClassifyTiles transcribed lane by lane (no numpy tricks): the independent statement the vectorised one is held against"""
    w, h = cb.bufferDimensions[0], cb.bufferDimensions[1]
    spq = cb.samplesPerQuad
    rays, tiles = [], []
    for ty in range((h + 7) // 8):
        for tx in range((w + 7) // 8):
            lanes = []
            for lane in range(64):
                lx, ly = abi.ssr_remap_lane8x8(lane)
                x, y = tx * 8 + lx, ty * 8 + ly
                on = x < w and y < h
                rough = F(scene[y, x, 3]) if on else F(0)
                z = F(depth[y, x]) if on else F(0)
                reflective, glossy = bool(z < F(1.0)), bool(rough < F(cb.roughnessThreshold))
                needs = on and glossy and reflective
                den = needs and not bool(rough < F(0.04))
                base = ((x & 1) | (y & 1)) == 0 if spq == 1 else (x & 1) == (y & 1) if spq == 2 else True
                needs = needs and (not den or base)
                if cb.temporalVarianceGuidedTracingEnabled and den and not needs:
                    var = F(variance[y, x]) if (variance is not None and on) else F(0)
                    needs = needs or bool(var > F(cb.varianceThreshold))
                lanes.append(dict(x=x, y=y, needs=needs, copy=(not needs) and den, base=base, tile=glossy and reflective))
            for lane, L in enumerate(lanes):
                if L["needs"]:
                    rays.append(abi.pack_ray_coords(L["x"], L["y"], spq != 4 and L["base"] and lanes[lane ^ 1]["copy"], spq == 1 and L["base"] and lanes[lane ^ 2]["copy"],
                                                    spq == 1 and L["base"] and lanes[lane ^ 3]["copy"]))
            if any(L["tile"] for L in lanes):
                tiles.append(((ty * 8) << 16) | (tx * 8))
    return np.array(rays, np.uint32), np.array(tiles, np.uint32)


def hand_frame():
    """16 x 16: tile (0,0) glossy 0.1 with a mirror pixel at the non-base position (1, 1), a rough pixel at the base position (4, 4) and a sky pixel at (6, 2); tile
    (1,0) rough (no ray, no tile entry); tile (0,1) mirror; tile (1,1) sky except one glossy pixel at (13, 11)"""
    scene = np.zeros((16, 16, 4), np.float16)
    depth = np.full((16, 16), 0.5, F)
    scene[:8, :8, 3], scene[:8, 8:, 3], scene[8:, :8, 3] = 0.1, 0.6, 0.02
    scene[1, 1, 3], scene[4, 4, 3] = 0.02, 0.7
    depth[2, 6] = 1.0
    depth[8:, 8:] = 1.0
    depth[11, 13], scene[11, 13, 3] = 0.25, 0.15
    return scene, depth


@pytest.mark.parametrize("spq", [1, 2, 4])
def test_classification_of_hand_made_frames(spq):
    scene, depth = hand_frame()
    cb = synth.ssr_constants(16, 16, 1)
    cb.samplesPerQuad = spq
    got = R.classify(scene, depth, cb)
    rays, tiles = classify_by_lane(scene, depth, cb)
    assert np.array_equal(got["rays"], rays) and np.array_equal(got["tiles"], tiles) and got["counters"].tolist() == [len(rays), len(tiles)]
    assert tiles.tolist() == [0, 8 << 16, (8 << 16) | 8]                         # tile (1,0) is rough: not listed
    un = [abi.unpack_ray_coords(r) for r in rays]
    by_px = {(x, y): (a, b, c) for x, y, a, b, c in un}
    assert len(by_px) == len(un)                                                 # no pixel twice
    assert [u[:2] for u in un[:4]] == {1: [(0, 0), (1, 1), (0, 2), (2, 0)], 2: [(0, 0), (1, 1), (0, 2), (1, 3)], 4: [(0, 0), (1, 0), (0, 1), (1, 1)]}[spq]   # lanes 0-3, then lane 4 = (0, 2), lane 8 = (2, 0)
    assert (1, 1) in by_px, "a mirror pixel in a non-base position keeps its ray"
    assert all((x, y) in by_px for x in range(8) for y in range(8, 16)), "every mirror pixel traces, whatever samplesPerQuad"
    assert (6, 2) not in by_px and (4, 4) not in by_px
    assert ((13, 11) in by_px) == (spq != 1), "(13, 11) is no base ray of the 1-sample pattern and its base pixel is sky: no ray, but its tile is listed"
    if spq == 1:
        assert by_px[(0, 0)] == (True, True, False), "the mirror neighbour (1, 1) needs no copy"
        assert by_px[(2, 2)] == (True, True, True) and by_px[(6, 6)] == (True, True, True)
        assert by_px[(1, 1)] == (False, False, False)
        assert not any((x, y) in by_px for x in (4, 5) for y in (4, 5)), "the quad of the rough base pixel (4, 4) gets neither rays nor copies"
        assert not any((x, y) in by_px for x in (6, 7) for y in (2, 3)), "nor does the quad of the sky base pixel (6, 2)"
        assert sum(1 for v in by_px.values() if any(v)) == 14                     # the 16 quads of tile (0,0) minus those two
        assert len(by_px) == 14 + 1 + 64                                          # + the mirror pixel (1, 1) and the mirror tile
    if spq == 2:
        assert by_px[(0, 0)] == (True, False, False) and by_px[(1, 1)] == (True, False, False), "the mirror pixel is a base ray of the diagonal pattern: it copies to (0, 1)"
        assert by_px[(5, 5)] == (True, False, False) and (4, 5) not in by_px, "(4, 5) is the copy target of (5, 5)"
        assert (5, 4) not in by_px, "its base partner (4, 4) is rough: neither a ray nor a copy"
        assert by_px[(7, 3)] == (True, False, False) and (7, 2) not in by_px and (6, 2) not in by_px
    if spq == 4:
        assert not any(any(v) for v in by_px.values()) and len(by_px) == 62 + 64 + 1


def test_variance_re_enable():
    scene, depth = hand_frame()
    cb = synth.ssr_constants(16, 16, 1)
    cb.samplesPerQuad, cb.temporalVarianceGuidedTracingEnabled, cb.varianceThreshold = 1, 1, 0.25
    var = np.zeros((16, 16), np.float16)
    var[0, 1], var[3, 3], var[1, 1], var[4, 5] = 0.5, 0.25, 9.0, 9.0          # (3,3): not ABOVE the threshold; (1,1) is mirror: traces anyway; (4,5): copy of a rough base
    got = R.classify(scene, depth, cb, var)
    rays, tiles = classify_by_lane(scene, depth, cb, var)
    assert np.array_equal(got["rays"], rays) and np.array_equal(got["tiles"], tiles)
    by_px = {u[:2]: u[2:] for u in (abi.unpack_ray_coords(r) for r in rays)}
    assert (1, 0) in by_px and by_px[(1, 0)] == (False, False, False), "the re-enabled pixel traces its own ray"
    assert by_px[(0, 0)] == (False, True, False), "and its base ray no longer copies to it"
    assert (3, 3) not in by_px and (5, 4) in by_px
    # a NULL history reads 0: nothing is above a threshold >= 0, the list is the one without the option
    with_null = R.classify(scene, depth, cb, None)["rays"]
    cb.temporalVarianceGuidedTracingEnabled = 0
    plain = R.classify(scene, depth, cb, var)["rays"]
    assert np.array_equal(with_null, plain) and (1, 0) not in {abi.unpack_ray_coords(r)[:2] for r in plain}


def test_edge_tiles_and_order_on_a_frame_that_is_no_multiple_of_8():
    scene, depth, _, _ = synth.ssr_surfaces(21, 13, seed=3)
    cb = synth.ssr_constants(21, 13, 1)
    for spq in (1, 2, 4):
        cb.samplesPerQuad = spq
        got = R.classify(scene.astype(np.float16), depth, cb)
        rays, tiles = classify_by_lane(scene.astype(np.float16), depth, cb)
        assert np.array_equal(got["rays"], rays) and np.array_equal(got["tiles"], tiles)
        assert all(x < 21 and y < 13 for x, y, *_ in (abi.unpack_ray_coords(r) for r in rays))
    assert {(int(t) & 0xFFFF, int(t) >> 16) for t in tiles} >= {(16, 0), (16, 8), (0, 8), (8, 8)}, "lanes beyond the frame load 0: the partial edge tiles are listed (:126 as written)"


# ---- intrinsics -----------------------------------------------------------------------------------------------------------------------------------
def test_pow_half_is_exact_and_normalize_matches_the_oracle():
    mips = np.arange(13)
    want = np.ldexp(F(1.0), -mips).astype(F)
    assert np.array_equal(R.pow_half(mips).view(np.uint32), want.view(np.uint32))
    got = O.math_array(2, np.full(13, 0.5, F), mips.astype(F))                    # the contract's pow = exp2(y * log2 x)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "pow(0.5, mip) must equal 2^-mip exactly for mip 0..12"
    assert all(F(4096.0) * want[m] == 4096 >> m for m in range(13))
    lib = O.load()
    lib.vqo_normalize_lit_array.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    v = np.random.default_rng(5).normal(size=(4096, 3)).astype(F) * F(3.0)
    for dxc in (0, 1):
        out = np.empty_like(v)
        lib.vqo_set_arithmetic(dxc)
        try:
            lib.vqo_normalize_lit_array(v.ctypes.data, out.ctypes.data, len(v))
        finally:
            lib.vqo_set_arithmetic(0)
        assert np.array_equal(np.stack(R._normalize((v[:, 0], v[:, 1], v[:, 2]), bool(dxc)), -1).view(np.uint32), out.view(np.uint32))
    assert float(R.TWO_PI) == 6.2831854820251465 and lib.vqo_unorm8_to_float(128) == float(F(128.0) / F(255.0))
    assert R._ftoi(np.array([-0.5, 0.99, 1.0, -1.0, np.nan, 3e10, -3e10], F)).tolist() == [0, 0, 1, -1, 0, 2147483647, -2147483648]


# ---- hand-made marches ----------------------------------------------------------------------------------------------------------------------------
def _group(n_live=64, **kw):
    """[1, 64] arrays of one 64-ray group; every ray (ox, oy, oz) + t (dx, dy, dz), dz = 0 unless given"""
    a = {k: np.full((1, 64), v, F) for k, v in dict(ox=0.1, oy=0.5, oz=0.5, dx=0.3, dy=0.05, dz=0.0).items()}
    for k, v in kw.items():
        a[k] = np.broadcast_to(np.asarray(v, F), (1, 64)).copy()
    a["live"] = (np.arange(64) < n_live)[None, :]
    return a


def _march(a, levels, w, h, max_iter=128, min_occ=0, mdm=0, mirror=False):
    return R.march(a["ox"], a["oy"], a["oz"], a["dx"], a["dy"], a["dz"], np.full((1, 64), mirror), np.full((1, 64), mdm, np.int64), a["live"], levels, w, h, max_iter, min_occ)


def test_a_ray_over_an_empty_pyramid_leaves_the_screen_with_confidence_0():
    w = h = 64
    levels = depth_ref.hierarchy(np.ones((h, w), F))
    levels[-1][:] = 1.0                                                        # hierarchy() clamps the top of a <= 12-level chain to min(top, 0): an EMPTY pyramid here
    a = _group()
    r = _march(a, levels, w, h)
    assert (r["px"] > 1.0).all() and (r["iterations"] < 128).all() and (r["mip"] < 0).all() and not r["low"].any()
    assert (r["top"] == len(levels) - 1).all(), "it skipped up level by level; the 32-pixel tile of level 5 ends at the screen's edge, and the load at the 1 x 1 level is outside it"
    n01 = np.full((h, w, 3), 0.5, F)
    wray = (np.ones((1, 64), F), np.zeros((1, 64), F), np.zeros((1, 64), F))
    conf, hx, hy = R.validate_hit(r["px"], r["py"], r["pz"], a["ox"], a["oy"], wray, r["iterations"] <= 128, levels, n01, np.eye(4, dtype=F), w, h, 0.015)
    assert (conf == 0).all() and (hx >= w).all()


def test_a_ray_against_a_wall_hits_it():
    w = h = 64
    depth = np.ones((h, w), F)
    depth[:, 40:] = 0.3                                                        # nearer than the ray (z = 0.5): a wall
    levels = depth_ref.hierarchy(depth)
    a = _group()
    r = _march(a, levels, w, h)
    assert (r["mip"] == -1).all() and (r["iterations"] < 40).all() and (r["top"] >= 2).all()
    assert ((r["px"] >= F(40 / 64)) & (r["px"] < F(41 / 64))).all(), "the hit is in the wall's first column"
    assert (r["py"] > a["oy"]).all() and (r["pz"] == F(0.5)).all()
    # in front of it the ray only ever loaded depths it was above of; a ray that starts inside the wall stops at once
    inside = _group(ox=0.8)
    ri = _march(inside, levels, w, h)
    assert (ri["iterations"] == 1).all() and (ri["mip"] == -1).all()


def test_the_last_rays_leave_when_the_count_reaches_min_traversal_occupancy():
    w = h = 256
    depth = np.ones((h, w), F)
    depth[:, 200:] = 0.3
    levels = depth_ref.hierarchy(depth)
    ox = np.full(64, 0.77, F)                                                  # 60 rays start just in front of the wall
    ox[[3, 17, 40, 63]] = 0.01                                                 # 4 rays cross the empty part first
    a = _group(ox=ox)
    long = np.zeros(64, bool)
    long[[3, 17, 40, 63]] = True
    free = _march(a, levels, w, h, min_occ=0)
    assert free["iterations"][0, long].min() > free["iterations"][0, ~long].max() + 3 and not free["low"].any()
    k = int(free["iterations"][0, ~long].max())                                # iterations 0 .. k-1 have more than 4 rays in the loop; at iteration k the count is 4
    r = _march(a, levels, w, h, min_occ=4)
    assert np.array_equal(r["iterations"][0, ~long], free["iterations"][0, ~long]) and not r["low"][0, ~long].any()
    assert (r["iterations"][0, long] == k + 1).all() and r["low"][0, long].all(), "the lane that trips the term still finishes that iteration"
    r3 = _march(a, levels, w, h, min_occ=3)                                    # the four march alike and leave together: the count is never 3
    assert np.array_equal(r3["iterations"], free["iterations"]) and not r3["low"].any()
    # mirror rays are counted but ignore the result
    rm = _march(a, levels, w, h, min_occ=4, mirror=True)
    assert np.array_equal(rm["iterations"], free["iterations"]) and not rm["low"].any()
    # rays beyond the list's end are not in the wave
    few = _group(n_live=3, ox=ox)
    rf = _march(few, levels, w, h, min_occ=4)
    assert (rf["iterations"][0, :3] == 1).all() and rf["low"][0, :3].all() and (rf["iterations"][0, 3:] == 0).all()


def test_a_ray_that_climbs_above_the_top_level_reads_0_and_comes_back_down():
    w = h = 8
    levels = [np.ones((max(1, h >> l), max(1, w >> l)), F) for l in range(4)]
    a = _group(ox=0.05, oy=0.05, dx=0.011, dy=0.007)
    r = _march(a, levels, w, h)
    L = len(levels)
    assert (r["top"] == L).all() and (r["mip"] == -1).all()
    assert (r["iterations"] == L + (L + 1)).all(), "L skips up through the levels, then the load of 0.0 at level L and at every level on the way down"
    assert R.load_depth(levels, np.array([0]), np.array([0]), np.array([L]))[0] == 0.0 and R.load_depth(levels, np.array([8]), np.array([0]), np.array([0]))[0] == 0.0
    # mostDetailedMip 3 of an 8 x 8 frame: the march starts on the 1 x 1 level, whose only tile ends at the screen's edge: the first load is already outside
    r3 = _march(a, levels, w, h, mdm=3)
    assert (r3["top"] == 3).all() and (r3["mip"] == 2).all() and (r3["iterations"] == 1).all() and (r3["px"] > 1.0).all()


# ---- coverage floors: conditions on the reference alone -------------------------------------------------------------------------------------------
def test_room_720p_reaches_every_exit_every_copy_flag_and_enough_hits():
    e = ref_cases.small_env()
    r = synth.ssr_room(1280, 720, e["spec_mips"])
    cb = r["cb"]
    scene = r["scene"].astype(np.float16)
    c = R.classify(scene, r["depth"], cb)
    rays = c["rays"]
    flags = [int(((rays >> np.uint32(b)) & 1).sum()) for b in (29, 30, 31)]
    st = {}
    rad0 = np.zeros((720, 1280, 4), np.float16)
    out = R.intersect(rays, rays.size, scene, depth_ref.hierarchy(r["depth"]), r["packed"], abi.FMT_R10G10B10A2_UNORM,
                      ref_cases.to_unorm8(scene[..., 3].astype(F)), r["noise"], cb, ref_cases.host_env(e), rad0, stats=st)
    exits = np.bincount(st["exit"], minlength=3).tolist()
    hits = int((st["confidence"] > 0).sum())
    print(f"rays {rays.size} tiles {c['tiles'].size} copy flags {flags} exits (cap, mip, occupancy) {exits} confidence > 0: {hits} iterations mean {st['iterations'].mean():.3f}")
    assert min(exits) >= 1, "each of the three loop exits"
    assert min(flags) >= 1, "each copy flag"
    assert hits >= 0.1 * rays.size, "at least 10 % of the rays with confidence > 0"
    # the counts the statement gives, as exact numbers
    assert (rays.size, c["tiles"].size) == (310420, 8705) and flags == [76336, 76270, 76298]
    assert exits == [288, 305937, 4195] and hits == 85857 and int(st["iterations"].max()) == 128 and int(st["top_mip"].max()) == 10
    assert np.isfinite(out.astype(F)).all()
