"""-m gpu: vqhip_ssr_classify and vqhip_ssr_intersect (csrc/ssr_trace.hip, docs/DESIGN_DETAILS.md §7.11) through the C ABI against tests/ssr_trace_ref.py, bit for
bit, no tolerance anywhere: synth.ssr_room at 1280 x 720 in full and at 3840 x 2160 on a seeded sample of 64-ray groups, white-noise frames (maximal divergence),
every samplesPerQuad / mostDetailedMip / minTraversalOccupancy / maxTraversalIntersections of the issue, both arithmetic readings and Fresnel modes, every format
combination, pitched buffers, an empty list, streams, refusals, and the whole chain resolve -> hierarchy -> fallback -> classify -> intersect -> composite.
Each GPU step runs once."""
import itertools

import numpy as np
import pytest
import torch

from tests import depth_ref
from tests import oracle_lib as O
from tests import ref_cases
from tests import ssr_trace_ref as R
from vqengine_amd import abi, capi, synth

pytestmark = pytest.mark.gpu
dev = ref_cases._dev
F16, F32, N10 = abi.FMT_RGBA16F, abi.FMT_RGBA32F, abi.FMT_R10G10B10A2_UNORM
SENTINEL = -7.0                     # radiance alpha is a length (>= 0): a pixel still holding the sentinel was not written


def _np(t):
    return t.cpu().numpy()


def assert_bits(got, ref, what):
    n, idx = O.bits_equal(_np(got) if hasattr(got, "cpu") else got, ref)
    assert n == 0, f"{what}: {n} mismatching elements, first {idx.tolist()}"


@pytest.fixture(scope="module")
def small():
    e = ref_cases.small_env()
    keep = []
    return {"e": e, "henv": ref_cases.host_env(e), "denv": ref_cases.dev_env(e, keep), "keep": keep}


def room(w, h, spec_mips, **kw):
    r = synth.ssr_room(w, h, spec_mips, **kw)
    return {"cb": r["cb"], "scene": r["scene"], "depth": r["depth"], "packed": r["packed"], "n01": r["n01"], "noise": r["noise"]}


def noise_frame(w, h, spec_mips, seed):
    scene, depth, packed, n01 = synth.ssr_surfaces(w, h, seed=seed)
    nz = np.random.default_rng(seed).integers(0, 256, (128, 128, 2), dtype=np.uint8)
    return {"cb": synth.ssr_constants(w, h, spec_mips), "scene": scene, "depth": depth, "packed": packed, "n01": n01, "noise": nz}


def host_side(f, lit_fmt=F16, normal_fmt=N10, true_top=False):
    """what both sides read: the scene colour in its storage format, the extracted roughness, the pyramid, the normals plane"""
    scene = f["scene"].astype(np.float16 if lit_fmt == F16 else np.float32)
    return {"scene": scene, "r8": ref_cases.to_unorm8(scene[..., 3].astype(np.float32)), "levels": depth_ref.hierarchy(f["depth"], true_top=true_top),
            "normals": f["packed"] if normal_fmt == N10 else f["n01"]}


def gpu_classify(ctx, f, hs, lit_fmt=F16, variance=None, stream=None):
    levels = ctx.depth_hierarchy(dev(f["depth"]), stream=stream)
    rays, counters, tiles = ctx.ssr_classify(dev(hs["scene"]), lit_fmt, levels[0], f["cb"], variance=dev(variance) if variance is not None else None, stream=stream)
    return levels, rays, counters, tiles


def check_classify(rays, counters, tiles, want, what):
    c = _np(counters).view(np.uint32)
    assert c.tolist() == want["counters"].tolist(), f"{what}: counters {c.tolist()} != {want['counters'].tolist()}"
    assert np.array_equal(_np(rays).view(np.uint32)[:c[0]], want["rays"]), f"{what}: ray list"
    assert np.array_equal(_np(tiles).view(np.uint32)[:c[1]], want["tiles"]), f"{what}: tile list"


def run_both(ctx, f, env, lit_fmt=F16, normal_fmt=N10, out_fmt=F16, dxc=False, explog=False, groups=None, stats=None, what=""):
    """classify + intersect on the GPU and in numpy over the same inputs; returns (gpu radiance, reference radiance)"""
    hs = host_side(f, lit_fmt, normal_fmt)
    want = R.classify(hs["scene"], f["depth"], f["cb"])
    levels, rays, counters, tiles = gpu_classify(ctx, f, hs, lit_fmt)
    h, w = f["depth"].shape
    odt = np.float16 if out_fmt == F16 else np.float32
    rad0 = np.full((h, w, 4), SENTINEL, odt)
    nrm = dev(hs["normals"].view(np.int32)) if normal_fmt == N10 else dev(hs["normals"])
    got = ctx.ssr_intersect(rays, counters, dev(hs["scene"]), lit_fmt, levels, nrm, normal_fmt, dev(hs["r8"]), dev(f["noise"]), f["cb"], env["denv"], dev(rad0), out_fmt)
    torch.cuda.synchronize()
    check_classify(rays, counters, tiles, want, what)
    ref = R.intersect(want["rays"], want["rays"].size, hs["scene"], hs["levels"], hs["normals"], normal_fmt, hs["r8"], f["noise"], f["cb"], env["henv"], rad0,
                      dxc=dxc, pow5_explog=explog, groups=groups, stats=stats)
    return _np(got), ref


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------------------
def test_room_720p_in_full(ctx, small):
    f = room(1280, 720, small["e"]["spec_mips"])
    st = {}
    got, ref = run_both(ctx, f, small, stats=st, what="room 1280 x 720")
    print(f"room 1280 x 720: {st['iterations'].size} rays, iterations mean {st['iterations'].mean():.2f} max {st['iterations'].max()}, "
          f"exits {np.bincount(st['exit'], minlength=3).tolist()}, confidence > 0: {(st['confidence'] > 0).mean():.3f}")
    assert_bits(got, ref, "room 1280 x 720 radiance")
    assert (ref[..., 3] == SENTINEL).any() and (ref[..., 3] != SENTINEL).mean() > 0.3


def test_room_2160p_on_a_sample_of_groups(ctx, small):
    """the ray list and the tile list in full; the march on 96 seeded 64-ray groups (6144 rays) — the full numpy march of 2.8 M rays takes minutes"""
    f = room(3840, 2160, small["e"]["spec_mips"])
    hs = host_side(f)
    n_groups = (R.classify(hs["scene"], f["depth"], f["cb"])["rays"].size + 63) // 64
    groups = np.random.default_rng(0x2160).choice(n_groups, 96, replace=False)
    got, ref = run_both(ctx, f, small, groups=groups, what="room 3840 x 2160")
    m = ref[..., 3] != SENTINEL
    assert m.sum() >= 96 * 64 - 63
    assert_bits(got[m], ref[m], "room 3840 x 2160 radiance of the sampled groups")


@pytest.mark.parametrize("W,H", [(333, 37), (1280, 720)])
def test_white_noise_frames(ctx, small, W, H):
    f = noise_frame(W, H, small["e"]["spec_mips"], 0x9900 + W)
    got, ref = run_both(ctx, f, small, what=f"noise {W} x {H}")
    assert_bits(got, ref, f"noise {W} x {H} radiance")


# ---- options ------------------------------------------------------------------------------------------------------------------------------------
def _frames(small):
    return [("room", room(320, 180, small["e"]["spec_mips"])), ("noise", noise_frame(333, 37, small["e"]["spec_mips"], 0x77))]


@pytest.mark.parametrize("spq", [1, 2, 4])
def test_samples_per_quad_and_variance(ctx, small, spq):
    for name, f in _frames(small):
        f["cb"].samplesPerQuad = spq
        got, ref = run_both(ctx, f, small, what=f"{name} spq {spq}")
        assert_bits(got, ref, f"{name} spq {spq}")
        # the variance re-enable
        h, w = f["depth"].shape
        var = np.random.default_rng(spq).random((h, w)).astype(np.float16)
        f["cb"].temporalVarianceGuidedTracingEnabled, f["cb"].varianceThreshold = 1, 0.5
        hs = host_side(f)
        want = R.classify(hs["scene"], f["depth"], f["cb"], var)
        _, rays, counters, tiles = gpu_classify(ctx, f, hs, variance=var)
        torch.cuda.synchronize()
        check_classify(rays, counters, tiles, want, f"{name} spq {spq} variance guided")
        f["cb"].temporalVarianceGuidedTracingEnabled = 0


@pytest.mark.parametrize("mdm", [0, 1, 3])
@pytest.mark.parametrize("occ", [0, 4, 32])
def test_most_detailed_mip_and_occupancy(ctx, small, mdm, occ):
    for name, f in _frames(small):
        f["cb"].mostDetailedMip, f["cb"].minTraversalOccupancy = mdm, occ
        got, ref = run_both(ctx, f, small, what=f"{name} mip {mdm} occupancy {occ}")
        assert_bits(got, ref, f"{name} mostDetailedMip {mdm} minTraversalOccupancy {occ}")


@pytest.mark.parametrize("max_it", [0, 1, 128])
def test_max_traversal_intersections(ctx, small, max_it):
    for name, f in _frames(small):
        f["cb"].maxTraversalIntersections = max_it
        got, ref = run_both(ctx, f, small, what=f"{name} max {max_it}")
        assert_bits(got, ref, f"{name} maxTraversalIntersections {max_it}")


@pytest.mark.parametrize("dxc", [False, True])
@pytest.mark.parametrize("explog", [False, True])
def test_arithmetic_readings_and_fresnel_modes(ctx, small, dxc, explog):
    ctx.set_arithmetic(dxc); ctx.set_fresnel_pow(explog)
    try:
        for name, f in _frames(small):
            got, ref = run_both(ctx, f, small, out_fmt=F32, dxc=dxc, explog=explog, what=f"{name} dxc {dxc} explog {explog}")
            assert_bits(got, ref, f"{name} DXC reading {dxc}, exp2-log2 pow {explog}")
    finally:
        ctx.set_arithmetic(False); ctx.set_fresnel_pow(False)


@pytest.mark.parametrize("lit_fmt,normal_fmt,out_fmt", list(itertools.product([F16, F32], [N10, F32], [F16, F32])))
def test_every_format_combination(ctx, small, lit_fmt, normal_fmt, out_fmt):
    name, f = _frames(small)[0]
    got, ref = run_both(ctx, f, small, lit_fmt=lit_fmt, normal_fmt=normal_fmt, out_fmt=out_fmt, what=f"formats {lit_fmt}/{normal_fmt}/{out_fmt}")
    assert_bits(got, ref, f"formats lit {lit_fmt} normals {normal_fmt} radiance {out_fmt}")


def test_hierarchy_flags_do_not_matter_to_the_caller(ctx, small):
    """the march reads whatever pyramid it is given: TRUE_TOP changes the 1 x 1 level, and the reference follows"""
    name, f = _frames(small)[0]
    hs = host_side(f, true_top=True)
    want = R.classify(hs["scene"], f["depth"], f["cb"])
    levels = ctx.depth_hierarchy(dev(f["depth"]), flags=abi.DEPTH_HIERARCHY_TRUE_TOP)
    rays, counters, _ = ctx.ssr_classify(dev(hs["scene"]), F16, levels[0], f["cb"])
    rad0 = np.full(f["depth"].shape + (4,), SENTINEL, np.float16)
    got = ctx.ssr_intersect(rays, counters, dev(hs["scene"]), F16, levels, dev(hs["normals"].view(np.int32)), N10, dev(hs["r8"]), dev(f["noise"]), f["cb"], small["denv"], dev(rad0), F16)
    torch.cuda.synchronize()
    ref = R.intersect(want["rays"], want["rays"].size, hs["scene"], hs["levels"], hs["normals"], N10, hs["r8"], f["noise"], f["cb"], small["henv"], rad0)
    assert_bits(got, ref, "TRUE_TOP pyramid")


def test_pitched_buffers(ctx, small):
    name, f = _frames(small)[0]
    h, w = f["depth"].shape
    P = w + 24
    hs = host_side(f)
    want = R.classify(hs["scene"], f["depth"], f["cb"])
    rad0 = np.full((h, w, 4), SENTINEL, np.float16)
    ref = R.intersect(want["rays"], want["rays"].size, hs["scene"], hs["levels"], hs["normals"], N10, hs["r8"], f["noise"], f["cb"], small["henv"], rad0)

    def pitched(a, fill):
        out = torch.full((h, P) + tuple(a.shape[2:]), fill, dtype=a.dtype, device="cuda")
        out[:, :w] = a
        return out
    sc, dp, nm = pitched(dev(hs["scene"]), 0.01), pitched(dev(f["depth"]), 0.5), pitched(dev(hs["normals"].view(np.int32)), 0)
    var = pitched(torch.zeros((h, w), dtype=torch.float16, device="cuda"), 9.0)
    out = torch.full((h, P, 4), SENTINEL, dtype=torch.float16, device="cuda")
    rays = torch.empty((h * w,), dtype=torch.int32, device="cuda")
    counters = torch.empty((2,), dtype=torch.int32, device="cuda")
    tiles = torch.empty((((w + 7) // 8) * ((h + 7) // 8),), dtype=torch.int32, device="cuda")
    levels = ctx.depth_hierarchy(dp[:, :w])
    lib, p = ctx.lib, lambda t: t.data_ptr()
    rc = lib.vqhip_ssr_classify(ctx._h, None, p(sc), F16, P, p(dp), P, p(var), P, f["cb"], p(rays), p(counters), p(tiles))
    assert rc == 0, lib.vqhip_last_error(ctx._h)
    r8, nz = dev(hs["r8"]), dev(f["noise"])                             # named: the raw pointers below must stay alive until the kernel has run
    rc = lib.vqhip_ssr_intersect(ctx._h, None, p(rays), p(counters), p(sc), F16, P, p(levels[0]), p(nm), N10, P, p(r8), p(nz), f["cb"], small["denv"], p(out), F16, P)
    assert rc == 0, lib.vqhip_last_error(ctx._h)
    torch.cuda.synchronize()
    check_classify(rays, counters, tiles, want, "pitched")
    assert_bits(out[:, :w].contiguous(), ref, "pitched radiance")
    assert (out[:, w:] == SENTINEL).all()


def test_empty_ray_list_writes_nothing(ctx, small):
    name, f = _frames(small)[0]
    f["cb"].roughnessThreshold = 0.0                                  # nothing is glossy
    got, ref = run_both(ctx, f, small, what="empty list")
    assert (ref[..., 3] == SENTINEL).all() and (ref == SENTINEL).all()
    assert_bits(got, ref, "empty list")


def test_two_calls_on_one_stream_and_one_on_a_second(ctx, small):
    name, f = _frames(small)[0]
    _, f2 = _frames(small)[1]
    s2 = torch.cuda.Stream()
    outs = []
    torch.cuda.synchronize()
    for fr, stream in ((f, None), (f2, None), (f, s2)):
        hs = host_side(fr)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            scene, dp, nrm, r8, nz = dev(hs["scene"]), dev(fr["depth"]), dev(hs["normals"].view(np.int32)), dev(hs["r8"]), dev(fr["noise"])
            rad = dev(np.full(fr["depth"].shape + (4,), SENTINEL, np.float16))
            levels = ctx.depth_hierarchy(dp, stream=stream)
            rays, counters, tiles = ctx.ssr_classify(scene, F16, levels[0], fr["cb"], stream=stream)
            outs.append((ctx.ssr_intersect(rays, counters, scene, F16, levels, nrm, N10, r8, nz, fr["cb"], small["denv"], rad, F16, stream=stream), rays, counters, tiles,
                         (scene, dp, nrm, r8, nz, levels)))
    torch.cuda.synchronize()
    for (got, rays, counters, tiles, _), fr in zip(outs, (f, f2, f)):
        hs = host_side(fr)
        want = R.classify(hs["scene"], fr["depth"], fr["cb"])
        check_classify(rays, counters, tiles, want, "streams")
        rad0 = np.full(fr["depth"].shape + (4,), SENTINEL, np.float16)
        ref = R.intersect(want["rays"], want["rays"].size, hs["scene"], hs["levels"], hs["normals"], N10, hs["r8"], fr["noise"], fr["cb"], small["henv"], rad0)
        assert_bits(got, ref, "streams radiance")
    assert_bits(outs[0][0], _np(outs[2][0]), "the same frame on two streams")


def test_argument_refusals(ctx, small):
    name, f = _frames(small)[0]
    h, w = f["depth"].shape
    hs = host_side(f)
    scene, dp, nrm, r8, nz = dev(hs["scene"]), dev(f["depth"]), dev(hs["normals"].view(np.int32)), dev(hs["r8"]), dev(f["noise"])
    levels = ctx.depth_hierarchy(dp)
    rays, counters, tiles = ctx.ssr_classify(scene, F16, levels[0], f["cb"])
    rad = torch.zeros((h, w, 4), dtype=torch.float16, device="cuda")
    lib, p = ctx.lib, lambda t: t.data_ptr() if t is not None else None
    INV, UNS = abi.VQHIP_ERR_INVALID_ARG, abi.VQHIP_ERR_UNSUPPORTED
    err = lambda: lib.vqhip_last_error(ctx._h).decode()

    def cb_with(**kw):
        cb = synth.ssr_constants(w, h, small["e"]["spec_mips"])
        for k, v in kw.items():
            if k == "dims":
                cb.bufferDimensions[0], cb.bufferDimensions[1] = v
            else:
                setattr(cb, k, v)
        return cb

    def classify(scene=scene, fmt=F16, pitch=0, cb=f["cb"], rays=rays, counters=counters):
        return lib.vqhip_ssr_classify(ctx._h, None, p(scene), fmt, pitch, p(dp), 0, None, 0, cb, p(rays), p(counters), p(tiles))
    assert classify() == 0
    assert classify(scene=None) == INV and "NULL" in err()
    assert classify(rays=None) == INV and classify(counters=None) == INV
    assert classify(fmt=abi.FMT_RGBA8_UNORM) == UNS
    assert classify(pitch=w - 1) == INV and "pitch" in err()
    assert classify(cb=cb_with(dims=(4097, 8))) == UNS and "4096" in err()
    assert classify(cb=cb_with(dims=(8, 4097))) == UNS
    assert classify(cb=cb_with(dims=(0, 8))) == INV

    def intersect(cb=f["cb"], lit_fmt=F16, normal_fmt=N10, out_fmt=F16, pitch=0, rays=rays, env=small["denv"], out=rad, noise=nz):
        return lib.vqhip_ssr_intersect(ctx._h, None, p(rays), p(counters), p(scene), lit_fmt, pitch, p(levels[0]), p(nrm), normal_fmt, 0, p(r8), p(noise), cb, env,
                                       p(out), out_fmt, 0)
    assert intersect() == 0
    assert intersect(cb=cb_with(maxTraversalIntersections=257)) == UNS and "256" in err()
    assert intersect(cb=cb_with(maxTraversalIntersections=256)) == 0
    assert intersect(cb=cb_with(mostDetailedMip=6)) == UNS and "mostDetailedMip" in err()
    assert intersect(cb=cb_with(dims=(4097, 8))) == UNS
    assert intersect(rays=None) == INV and intersect(noise=None) == INV and intersect(out=None) == INV
    assert intersect(lit_fmt=abi.FMT_RGBA8_UNORM) == UNS and intersect(out_fmt=N10) == UNS and intersect(normal_fmt=F16) == UNS
    assert intersect(pitch=w - 1) == INV
    assert intersect(out=scene) == INV and "overlaps" in err()
    assert intersect(env=abi.EnvMap(None, 0, None, 0, 0, None, 0)) == INV
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ctx.ssr_classify(scene, F16, levels[0], cb_with(dims=(w + 1, h)))


# ---- the whole chain ----------------------------------------------------------------------------------------------------------------------------
def test_whole_reflection_chain(ctx, small):
    """vqhip_msaa_resolve_surfaces (+ fused hierarchy) -> vqhip_ssr_environment_fallback -> vqhip_ssr_classify -> vqhip_ssr_intersect -> vqhip_composite_reflections
    against the same chain in numpy / the oracle: one layer covering every sample of the room, the four depth samples a hair apart"""
    w, h = 640, 360
    f = room(w, h, small["e"]["spec_mips"])
    cb = f["cb"]
    rng = np.random.default_rng(0xC4A1)
    ms = np.repeat(f["depth"][..., None], 4, -1)
    ms = np.where(ms < 1.0, np.minimum(ms + (rng.random((h, w, 4)) * 2e-6).astype(np.float32), np.nextafter(np.float32(1), np.float32(0))), ms).astype(np.float32)
    cov = [np.full((h, w), 0xF, np.uint8)]
    gb1 = [np.concatenate([np.zeros((h, w, 3), np.float32), f["scene"][..., 3:4]], -1)]
    lit = f["scene"].astype(np.float16)
    lit[..., 3] = 0
    # reference chain
    depth, _ = depth_ref.resolve_depth(ms)
    normals = depth_ref.resolve_normals([f["packed"]], cov, N10, False, N10)
    scene = lit.copy()
    scene[..., 3] = depth_ref.resolve_roughness(ms, cov, gb1, None, F16)
    levels = depth_ref.hierarchy(depth)
    rad, r8 = O.ssr_environment_fallback(scene, F16, depth, normals, N10, cb, small["henv"], F16, extract_roughness=True)
    want = R.classify(scene, depth, cb)
    rad = R.intersect(want["rays"], want["rays"].size, scene, levels, normals, N10, r8, f["noise"], cb, small["henv"], rad)
    final = O.composite_reflections(rad, scene, F16)
    # the library
    dscene = dev(lit)
    res = ctx.msaa_resolve_surfaces(dev(ms), [dev(c) for c in cov], normals=[dev(f["packed"].view(np.int32))], roughness=[dev(g) for g in gb1],
                                    out_normals_fmt=N10, scene_color=dscene, scene_fmt=F16, hierarchy=True)
    glevels = res["hierarchy"]
    grad, g8 = ctx.ssr_environment_fallback(dscene, F16, glevels[0].contiguous(), res["normals"], N10, cb, small["denv"], F16, extract_roughness=True)
    rays, counters, tiles = ctx.ssr_classify(dscene, F16, glevels[0], cb)
    ctx.ssr_intersect(rays, counters, dscene, F16, glevels, res["normals"], N10, g8, dev(f["noise"]), cb, small["denv"], grad, F16)
    traced = _np(grad).copy()
    ctx.composite_reflections(grad, dscene, F16)
    torch.cuda.synchronize()
    check_classify(rays, counters, tiles, want, "chain")
    assert_bits(traced, rad, "chain: radiance")
    assert_bits(dscene, final, "chain: composited scene colour")
    glossy = (scene[..., 3].astype(np.float32) < np.float32(cb.roughnessThreshold)) & (depth < 1)
    assert (rad[glossy][:, :3].astype(np.float32).sum(-1) > 0).mean() > 0.9, "glossy pixels now carry reflections"
