"""-m gpu: vqhip_depth_hierarchy and vqhip_msaa_resolve_surfaces (csrc/depth.hip, docs/DESIGN_DETAILS.md §7.10) bit for bit against tests/depth_ref.py;
the roughness resolve against vqhip_forward_lighting[_msaa]'s own output; the fused call against the two separate ones; the resolved surfaces fed to
vqhip_ssr_environment_fallback against the oracle on the numpy-resolved inputs; the argument checks."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests import depth_ref as R
from tests import oracle_lib as O
from tests import ref_cases
from vqengine_amd import abi, capi, synth

pytestmark = pytest.mark.gpu
dev = ref_cases._dev
F = np.float32
F16, F32, N10 = abi.FMT_RGBA16F, abi.FMT_RGBA32F, abi.FMT_R10G10B10A2_UNORM
TRUE_TOP = abi.DEPTH_HIERARCHY_TRUE_TOP


def _np(t):
    return t.cpu().numpy()


def assert_levels(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for l, (g, w) in enumerate(zip(got, want)):
        g = _np(g)
        assert g.shape == w.shape, (what, l, g.shape, w.shape)
        bad = np.argwhere(g.view(np.uint32) != np.ascontiguousarray(w, F).view(np.uint32))
        assert len(bad) == 0, f"{what}: level {l} ({w.shape[1]} x {w.shape[0]}): {len(bad)} texels differ, first (y, x) = {bad[0].tolist()}: got {g[tuple(bad[0])]!r}, want {w[tuple(bad[0])]!r}"


def _random_depth(w, h, seed):
    r = np.random.default_rng(seed)
    d = (0.001 + 0.998 * r.random((h, w), dtype=F)).astype(F)
    d[r.random((h, w)) < 0.02] = 1.0
    return d


SHAPES = [(1, 1), (2, 1), (64, 1), (64, 64), (65, 65), (333, 37), (1000, 3), (1280, 720), (1920, 1080), (3840, 2160), (4096, 4096)]


# ---- vqhip_depth_hierarchy --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("content", ["random", "ones", "one_texel"])
def test_hierarchy_every_level_both_flags(ctx, w, h, content):
    if content == "random":
        d = _random_depth(w, h, seed=w * 31 + h)
    else:
        d = np.ones((h, w), F)
        if content == "one_texel":
            d[h - 1, w - 1] = 0.5                 # last row and column: a dropped edge tile or a stale level-6 read shows in exactly one texel per level
    dd = dev(d)
    for flags in (0, TRUE_TOP):
        got = ctx.depth_hierarchy(dd, flags=flags)
        torch.cuda.synchronize()
        assert_levels(got, R.hierarchy(d, true_top=bool(flags)), f"{w} x {h} {content} flags {flags}")
    if content == "one_texel" and w * h > 1:
        ones, one = R.hierarchy(np.ones((h, w), F)), R.hierarchy(d)
        assert all(np.count_nonzero(a != b) <= 1 for a, b in zip(ones, one)) and np.count_nonzero(ones[0] != one[0]) == 1


@pytest.mark.parametrize("w,h,pitch", [(333, 37, 340), (1280, 720, 1284), (200, 130, 203)])
def test_hierarchy_pitched_input(ctx, w, h, pitch):
    d = _random_depth(w, h, seed=pitch)
    wide = np.full((h, pitch), np.nan, F)
    wide[:, :w] = d
    dw = dev(wide)
    for flags in (0, TRUE_TOP):
        got = ctx.depth_hierarchy(dw[:, :w], flags=flags)
        assert_levels(got, R.hierarchy(d, true_top=bool(flags)), f"pitched {w} x {h} / {pitch} flags {flags}")


def test_hierarchy_twice_on_one_stream_and_once_on_a_second(ctx):
    """nothing is left behind by a call, and calls on different streams are ordered on the context's tile-minimum buffer: three different inputs (the TRUE_TOP
    call between two default ones, then TRUE_TOP again on a second stream), each result compared. One run of each."""
    w, h = 1280, 720
    a, b, c = (_random_depth(w, h, seed=s) for s in (11, 12, 13))
    da, db, dc = dev(a), dev(b), dev(c)
    torch.cuda.synchronize()
    s2 = torch.cuda.Stream()
    ga = ctx.depth_hierarchy(da)
    gb = ctx.depth_hierarchy(db, flags=TRUE_TOP)
    gc = ctx.depth_hierarchy(dc, stream=s2)
    gd = ctx.depth_hierarchy(da, flags=TRUE_TOP, stream=s2)
    torch.cuda.synchronize()
    assert_levels(ga, R.hierarchy(a), "first call")
    assert_levels(gb, R.hierarchy(b, true_top=True), "second call, same stream")
    assert_levels(gc, R.hierarchy(c), "third call, second stream")
    assert_levels(gd, R.hierarchy(a, true_top=True), "fourth call, second stream, TRUE_TOP")


# ---- vqhip_msaa_resolve_surfaces ----------------------------------------------------------------------------------------------------------------
def _frame(w, h, layers, mode, seed, normals_fmt, scene_fmt, with_bg):
    gbs, cov = synth.gbuffer_msaa(w, h, layers, 0.2, seed=seed, mode=mode)
    ms = synth.depth_msaa(w, h, cov, seed=seed + 1, plant=True)
    words = [synth.packed_unit_normals((h, w), seed=seed + 10 + k) for k in range(layers)]
    if normals_fmt == F32:
        normals = [np.concatenate([R.decode_normals01(x, N10), np.ones((h, w, 1), F)], -1) for x in words]
    else:
        normals = words
    gb1 = [g[1] for g in gbs]
    sdt = np.float16 if scene_fmt == F16 else np.float32
    scene = synth.hdr_image(w, h, seed=seed + 2).astype(sdt)
    bg = synth.hdr_image(w, h, seed=seed + 3).astype(sdt) if with_bg else None
    if bg is not None:
        bg[..., 3] = np.random.default_rng(seed + 4).random((h, w)).astype(sdt)
    return {"cov": cov, "ms": ms, "normals": normals, "gb1": gb1, "scene": scene, "bg": bg, "gbs": gbs}


def _dev_normals(n):
    return dev(n.view(np.int32)) if n.dtype == np.uint32 else dev(n)


def _run_resolve(ctx, f, normals_fmt, out_depth, out_normals_fmt, scene_fmt, with_scene, hierarchy=False, flags=0):
    scene = dev(f["scene"]) if with_scene else None
    res = ctx.msaa_resolve_surfaces(dev(f["ms"]), [dev(c) for c in f["cov"]], normals=[_dev_normals(n) for n in f["normals"]], normals_fmt=normals_fmt,
                                    roughness=[dev(g) for g in f["gb1"]], background=dev(f["bg"]) if f["bg"] is not None else None,
                                    out_depth=out_depth, out_normals_fmt=out_normals_fmt, scene_color=scene, scene_fmt=scene_fmt,
                                    hierarchy=hierarchy, flags=flags)
    torch.cuda.synchronize()
    return res


def _check_resolve(res, f, normals_fmt, out_normals_fmt, scene_fmt, dxc, what):
    if "depth" in res:
        want, _ = R.resolve_depth(f["ms"])
        assert np.array_equal(_np(res["depth"]).view(np.uint32), want.view(np.uint32)), what + ": depth"
    if "normals" in res:
        want = R.resolve_normals(f["normals"], f["cov"], normals_fmt, dxc, out_normals_fmt)
        got = _np(res["normals"])
        got = got.view(np.uint32)
        bad = np.argwhere(got != want.view(np.uint32))
        assert len(bad) == 0, f"{what}: normals: {len(bad)} elements differ, first {bad[0].tolist()}"
    if "scene_color" in res:
        got = _np(res["scene_color"])
        u = np.uint16 if scene_fmt == F16 else np.uint32
        assert np.array_equal(got[..., :3].view(u), f["scene"][..., :3].view(u)), what + ": rgb must not change"
        want = R.resolve_roughness(f["ms"], f["cov"], f["gb1"], f["bg"], scene_fmt)
        assert np.array_equal(np.ascontiguousarray(got[..., 3]).view(u), np.ascontiguousarray(want).view(u)), what + ": alpha"


SUBSETS = [s for s in itertools.product([False, True], repeat=3) if any(s)]        # (depth, normals, roughness): the seven permutations


@pytest.mark.parametrize("layers", [2, 3, 4])
@pytest.mark.parametrize("mode", ["edges", "random"])
def test_resolve_every_output_subset_and_format(ctx, layers, mode):
    w, h = 160, 48
    combos = list(itertools.product([N10, F32], [N10, F32], [F16, F32], [False, True]))
    for ci, (nin, nout, sfmt, with_bg) in enumerate(combos):
        f = _frame(w, h, layers, mode, 0x200 + 16 * layers + ci, nin, sfmt, with_bg)
        for (d, n, r) in SUBSETS:
            res = _run_resolve(ctx, f, nin, d, nout if n else None, sfmt, r)
            assert set(res) == {k for k, on in (("depth", d), ("normals", n), ("scene_color", r)) if on}
            _check_resolve(res, f, nin, nout, sfmt, False, f"{layers} layers {mode} nin {nin} nout {nout} scene {sfmt} bg {with_bg} subset {(d, n, r)}")


@pytest.mark.parametrize("nin,nout", [(N10, N10), (F32, F32), (N10, F32)])
def test_resolve_normals_in_the_dxc_reading(ctx, nin, nout):
    """tests/depth_ref.py restates the DXC reading exactly (the FMA chain through an error-free sum rounded to odd, rsqrt as (float)(1 / sqrt((double)x))): bit-exact"""
    f = _frame(160, 48, 3, "edges", 0x310, nin, F16, False)
    ctx.set_arithmetic(True)
    try:
        res = _run_resolve(ctx, f, nin, False, nout, F16, False)
    finally:
        ctx.set_arithmetic(False)
    _check_resolve(res, f, nin, nout, F16, True, f"DXC reading {nin} -> {nout}")
    lit = R.resolve_normals(f["normals"], f["cov"], nin, False, nout)
    dxc = R.resolve_normals(f["normals"], f["cov"], nin, True, nout)
    print(f"normals resolve, literal vs DXC reading: {np.mean(lit.view(np.uint32) != dxc.view(np.uint32)):.5f} of the stored elements differ")


def test_resolve_zero_sum_and_background_pixels(ctx):
    """(-1, 1, -1) + (1, -1, 1) twice: a zero sum normalises to NaN — the UNORM store writes code 0 in every channel, the RGBA32F store the NaN; alpha is 1.
    Row 1 has no owner at all: four background samples, normalize(-1, -1, -1)."""
    w, h = 64, 2
    normals = [np.full((h, w), np.uint32(0 | (1023 << 10) | (0 << 20) | (3 << 30)), np.uint32), np.full((h, w), np.uint32(1023 | (0 << 10) | (1023 << 20) | (3 << 30)), np.uint32)]
    cov = [np.full((h, w), 0x5, np.uint8), np.full((h, w), 0xA, np.uint8)]
    cov[0][1], cov[1][1] = 0, 0
    ms = np.ones((h, w, 4), F)
    for dxc in (False, True):
        ctx.set_arithmetic(dxc)
        try:
            for out_fmt in (N10, F32):
                res = ctx.msaa_resolve_surfaces(dev(ms), [dev(c) for c in cov], normals=[_dev_normals(n) for n in normals], out_normals_fmt=out_fmt)
                torch.cuda.synchronize()
                got, want = _np(res["normals"]), R.resolve_normals(normals, cov, N10, dxc, out_fmt)
                if out_fmt == N10:
                    assert np.array_equal(got.view(np.uint32), want) and np.all(got.view(np.uint32)[0] == np.uint32(3) << 30)
                else:
                    assert np.all(np.isnan(got[0, :, :3])) and np.all(np.isnan(want[0, :, :3])) and np.all(got[..., 3] == 1.0)
                    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
        finally:
            ctx.set_arithmetic(False)


def test_resolve_1080p_all_outputs(ctx):
    w, h = 1920, 1080
    f = _frame(w, h, 3, "edges", 0x400, N10, F16, True)
    res = _run_resolve(ctx, f, N10, True, N10, F16, True)
    _check_resolve(res, f, N10, N10, F16, False, "1920 x 1080")


# ---- roughness ties the two MSAA entry points together -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [F16, F32])
def test_roughness_on_the_output_of_forward_lighting_msaa(ctx, fmt):
    w, h, layers = 160, 48, 3
    f = _frame(w, h, layers, "edges", 0x500, N10, fmt, True)
    pf, extra = synth.per_frame(points=synth.point_lights(12, seed=5), spots=synth.spot_lights(2, seed=5), directional=synth.directional_light())
    pv = synth.per_view(w, h)
    planes = [[dev(p) for p in g] for g in f["gbs"]]
    covd = [dev(c) for c in f["cov"]]
    bgd = dev(f["bg"])
    lit = ctx.forward_lighting_msaa(planes, covd, pf, pv, background=bgd, out_fmt=fmt, extra_point=extra)
    torch.cuda.synchronize()
    before = _np(lit).copy()
    res = ctx.msaa_resolve_surfaces(dev(f["ms"]), covd, roughness=[p[1] for p in planes], background=bgd, scene_color=lit, scene_fmt=fmt)
    torch.cuda.synchronize()
    after = _np(res["scene_color"])
    u = np.uint16 if fmt == F16 else np.uint32
    assert np.array_equal(after[..., :3].view(u), before[..., :3].view(u))
    want = R.resolve_roughness(f["ms"], f["cov"], f["gb1"], f["bg"], fmt)
    assert np.array_equal(np.ascontiguousarray(after[..., 3]).view(u), np.ascontiguousarray(want).view(u))
    # full coverage by one layer: the image equals vqhip_forward_lighting's, alpha included
    full = torch.full((h, w), 0xF, dtype=torch.uint8, device="cuda")
    one = ctx.forward_lighting_msaa([planes[0]], [full], pf, pv, out_fmt=fmt, extra_point=extra)
    ctx.msaa_resolve_surfaces(dev(f["ms"]), [full], roughness=[planes[0][1]], scene_color=one, scene_fmt=fmt)
    ref = ctx.forward_lighting(planes[0], pf, pv, out_fmt=fmt, extra_point=extra)
    torch.cuda.synchronize()
    assert np.array_equal(_np(one).view(u), _np(ref).view(u))


# ---- fusion ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(333, 37), (1280, 720), (3840, 2160)])
def test_fused_call_equals_resolve_then_hierarchy(ctx, w, h):
    _, cov = synth.gbuffer_msaa(w, h, 2, 0.05, seed=0x600 + w) if w < 2000 else (None, [np.full((h, w), 0xF, np.uint8)])
    ms = synth.depth_msaa(w, h, cov, seed=0x601, plant=True)
    msd = dev(ms)
    for flags in (0, TRUE_TOP):
        fused = ctx.msaa_resolve_surfaces(msd, hierarchy=True, flags=flags)
        sep = ctx.msaa_resolve_surfaces(msd, out_depth=True)
        chain = ctx.depth_hierarchy(sep["depth"], flags=flags)
        torch.cuda.synchronize()
        assert set(fused) == {"hierarchy"}
        assert_levels(fused["hierarchy"], [_np(c) for c in chain], f"fused vs separate {w} x {h} flags {flags}")
        assert_levels(fused["hierarchy"], R.hierarchy(R.resolve_depth(ms)[0], true_top=bool(flags)), f"fused vs contract {w} x {h} flags {flags}")
    both = ctx.msaa_resolve_surfaces(msd, out_depth=True, hierarchy=True)
    torch.cuda.synchronize()
    assert np.array_equal(_np(both["depth"]).view(np.uint32), _np(both["hierarchy"][0]).view(np.uint32))


# ---- end to end: the resolved surfaces are what the SSR fallback takes ----------------------------------------------------------------------------
def test_resolved_surfaces_feed_the_ssr_fallback(ctx):
    w, h, layers = 200, 40, 3
    e = ref_cases.small_env()
    keep = []
    denv, henv = ref_cases.dev_env(e, keep), ref_cases.host_env(e)
    f = _frame(w, h, layers, "edges", 0x700, N10, F16, True)
    f["ms"] = (0.9 + 0.1 * f["ms"]).astype(F)                         # nearer the far plane, where the projection of synth.ssr_constants puts geometry
    f["ms"][f["ms"] > 0.9995] = 1.0
    for g in f["gb1"]:
        g[..., 3] = np.random.default_rng(3).random((h, w)).astype(F)  # roughness over the whole range: most pixels take the fallback
    cb = synth.ssr_constants(w, h, e["spec_mips"])
    res = _run_resolve(ctx, f, N10, False, N10, F16, True, hierarchy=True)
    got = ctx.ssr_environment_fallback(res["scene_color"], F16, res["hierarchy"][0], res["normals"], N10, cb, denv, F16)
    torch.cuda.synchronize()
    depth, _ = R.resolve_depth(f["ms"])
    normals = R.resolve_normals(f["normals"], f["cov"], N10, False, N10)
    scene = f["scene"].copy()
    scene[..., 3] = R.resolve_roughness(f["ms"], f["cov"], f["gb1"], f["bg"], F16)
    want = O.ssr_environment_fallback(scene, F16, depth, normals, N10, cb, henv, F16)
    n, idx = O.bits_equal(_np(got), want)
    assert n == 0, f"{n} mismatching elements, first {idx.tolist()}"
    assert (want[..., :3].astype(F).sum(-1) > 0).mean() > 0.1                  # the frame does take the fallback


# ---- argument errors ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_a_message_and_launch_nothing(ctx):
    lib = ctx.lib
    w, h = 32, 8
    ms = dev(np.ones((h, w, 4), F))
    cov = dev(np.full((h, w), 0xF, np.uint8))
    nrm = dev(np.zeros((h, w), np.int32))
    gb1 = dev(np.zeros((h, w, 4), F))
    sentinel = 7.0
    outd = torch.full((h, w), sentinel, dtype=torch.float32, device="cuda")
    outn = torch.full((h, w), 7, dtype=torch.int32, device="cuda")
    scene = torch.full((h, w, 4), sentinel, dtype=torch.float16, device="cuda")
    hier = torch.full((abi.mip_chain_px(w, h, abi.mip_level_count(w, h)),), sentinel, dtype=torch.float32, device="cuda")

    def surf(**kw):
        s = abi.MSAASurfaces()
        s.depth_ms, s.width, s.height, s.layers, s.normals_fmt = ms.data_ptr(), w, h, 1, N10
        s.coverage[0], s.normals[0], s.roughness[0] = cov.data_ptr(), nrm.data_ptr(), gb1.data_ptr()
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def call(s, d=None, dp=0, n=None, nf=N10, np_=0, sc=None, sf=F16, sp=0, hi=None, flags=0):
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
        return lib.vqhip_msaa_resolve_surfaces(ctx._h, None, C.byref(s), p(d), dp, p(n), nf, np_, p(sc), sf, sp, p(hi), flags)

    def err():
        return (lib.vqhip_last_error(ctx._h) or b"").decode()

    INV, UNS = abi.VQHIP_ERR_INVALID_ARG, abi.VQHIP_ERR_UNSUPPORTED
    assert call(surf()) == INV and "every output is NULL" in err()
    assert call(surf(layers=0), d=outd) == INV and "layers" in err()
    assert call(surf(layers=5), d=outd) == INV and "layers" in err()
    assert call(surf(depth_pitch_px=w - 1), d=outd) == INV and "pitch" in err()
    assert call(surf(), d=outd, dp=w - 1) == INV and "pitch" in err()
    assert call(surf(), n=outn, np_=w - 1) == INV and "pitch" in err()
    assert call(surf(coverage_pitch=w - 1), n=outn) == INV and "pitch" in err()
    assert call(surf(), n=outn, nf=F16) == UNS and "normals" in err()
    assert call(surf(normals_fmt=abi.FMT_RGBA8_UNORM), n=outn) == UNS and "normals" in err()
    assert call(surf(), sc=scene, sf=abi.FMT_RGBA8_UNORM) == UNS and "sceneFmt" in err()
    assert call(surf(), d=outd, flags=2) == INV and "flag" in err()
    assert call(surf(width=4097), hi=hier) == UNS and "4096" in err()
    assert call(surf(), d=ms.view(-1)[:w * h].view(h, w)) == INV and "overlaps" in err()
    s = surf()
    s.coverage[0] = None
    assert call(s, n=outn) == INV and "coverage" in err()
    # vqhip_depth_hierarchy
    d = dev(np.ones((h, w), F))
    p = lambda t: C.c_void_p(t.data_ptr())                                     # noqa: E731
    assert lib.vqhip_depth_hierarchy(ctx._h, None, p(d), 0, 4097, 8, p(hier), 0) == UNS and "4096" in err()
    assert lib.vqhip_depth_hierarchy(ctx._h, None, p(d), 0, 8, 4097, p(hier), 0) == UNS
    assert lib.vqhip_depth_hierarchy(ctx._h, None, p(d), w - 1, w, h, p(hier), 0) == INV and "pitch" in err()
    assert lib.vqhip_depth_hierarchy(ctx._h, None, None, 0, w, h, p(hier), 0) == INV and "NULL" in err()
    assert lib.vqhip_depth_hierarchy(ctx._h, None, p(d), 0, 0, h, p(hier), 0) == INV
    assert lib.vqhip_depth_hierarchy(ctx._h, None, p(d), 0, w, h, p(hier), 4) == INV and "flag" in err()
    assert lib.vqhip_depth_hierarchy(ctx._h, None, p(hier), 0, w, h, p(hier), 0) == INV and "overlaps" in err()
    with pytest.raises(ValueError):
        ctx.depth_hierarchy(torch.zeros((8, 4097), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        ctx.msaa_resolve_surfaces(ms)
    torch.cuda.synchronize()
    for t in (outd, scene, hier):
        assert bool((t == sentinel).all()), "a refused call must not have launched anything"
    assert bool((outn == 7).all())
