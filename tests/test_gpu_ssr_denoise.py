"""-m gpu: vqhip_ssr_prefilter and vqhip_ssr_resolve_temporal (csrc/ssr_denoise.hip, docs/DESIGN_DETAILS.md §7.12) through the C ABI against
tests/ssr_denoise_ref.py, bit for bit, no tolerance anywhere: white-noise planes with every tile listed in both arithmetic readings and every format
combination, a shuffled sparse list with a duplicate and an entry beyond the grid, an empty list, pitched buffers, a second stream, special values, refusals, and
the chain fallback -> classify -> intersect -> prefilter -> resolve -> composite on synth.ssr_room. Each GPU step runs once."""
import itertools

import numpy as np
import pytest
import torch

from tests import depth_ref
from tests import oracle_lib as O
from tests import ref_cases
from tests import ssr_denoise_ref as D
from tests import ssr_trace_ref as R
from vqengine_amd import abi, capi, synth

pytestmark = pytest.mark.gpu
dev = ref_cases._dev
F16, F32, N10, R11 = abi.FMT_RGBA16F, abi.FMT_RGBA32F, abi.FMT_R10G10B10A2_UNORM, abi.FMT_R11G11B10_FLOAT
SENTINEL = -7.0                     # no pass can write it: radiance alpha repeats blue (>= 0 here), the variance is a square


def _np(t):
    return t.cpu().numpy()


def assert_bits(got, ref, what):
    n, idx = O.bits_equal(_np(got) if hasattr(got, "cpu") else got, ref)
    assert n == 0, f"{what}: {n} mismatching elements, first {idx.tolist()}"


def all_tiles(w, h):
    tx, ty = (w + 7) // 8, (h + 7) // 8
    return np.array([((y * 8) << 16) | (x * 8) for y in range(ty) for x in range(tx)], np.uint32)


def frame(w, h, seed, radiance=None, smooth=False):
    """white-noise surfaces (nearly every prefilter tap's weight vanishes), or smooth ones (all 15 taps of a pixel carry weight, their order is observable:
    tests/test_ssr_denoise_cpu.py::test_taps_and_their_order_are_observable_on_smooth_surfaces)"""
    if smooth:
        depth, packed, n01 = synth.ssr_smooth_surfaces(w, h, seed=seed)
    else:
        _, depth, packed, n01 = synth.ssr_surfaces(w, h, seed=seed)
    f = synth.ssr_denoise_planes(w, h, seed=seed, radiance=radiance)
    f.update(depth=depth, packed=packed, n01=n01, cb=synth.ssr_constants(w, h, 1))
    return f


def _img(a, fmt):
    return np.ascontiguousarray(a.astype(np.float16 if fmt == F16 else np.float32))


def _dtiles(tiles, w, h):
    """the list in a buffer of the size the entry points may read: ceil(w/8) * ceil(h/8) entries"""
    buf = np.zeros(((w + 7) // 8) * ((h + 7) // 8), np.uint32)
    buf[:min(len(tiles), buf.size)] = tiles[:buf.size]
    return dev(buf.view(np.int32))


def run_both(ctx, f, tiles, count=None, rad_fmt=F16, out_fmt=F16, normal_fmt=N10, avg_fmt=R11, dxc=False, stream=None, what=""):
    """both passes back to back on the GPU (no host synchronisation in between) and in numpy; asserts all four outputs bit for bit and returns the reference's"""
    w, h = int(f["cb"].bufferDimensions[0]), int(f["cb"].bufferDimensions[1])
    count = len(tiles) if count is None else count
    rad, rep = _img(f["radiance"], rad_fmt), _img(f["reprojected"], rad_fmt)
    normals = f["packed"] if normal_fmt == N10 else f["n01"]
    avg = f["average_r11"] if avg_fmt == R11 else f["average"]
    odt = np.float16 if out_fmt == F16 else np.float32
    o_r, o_v = np.full((h, w, 4), SENTINEL, odt), np.full((h, w), SENTINEL, np.float16)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        dt, dc = _dtiles(tiles, w, h), dev(np.array([0, count], np.uint32).view(np.int32))
        dn = dev(normals.view(np.int32)) if normal_fmt == N10 else dev(normals)
        da = dev(avg.view(np.int32)) if avg_fmt == R11 else dev(avg)
        d8, dvar, dcnt, drep = dev(f["roughness8"]), dev(f["variance"]), dev(f["sample_count"]), dev(rep)
        p_r, p_v = ctx.ssr_prefilter(dt, dc, dev(f["depth"]), dn, normal_fmt, d8, da, avg_fmt, dev(rad), rad_fmt, dvar, f["cb"],
                                     out=dev(o_r), out_fmt=out_fmt, out_variance=dev(o_v), stream=stream)
        t_r, t_v = ctx.ssr_resolve_temporal(dt, dc, d8, da, avg_fmt, p_r, out_fmt, drep, rad_fmt, p_v, dcnt, f["cb"],
                                            out=dev(o_r), out_fmt=out_fmt, out_variance=dev(o_v), stream=stream)
    torch.cuda.synchronize()
    rp_r, rp_v = D.prefilter(tiles, count, f["depth"], normals, normal_fmt, f["roughness8"], avg, avg_fmt, rad, f["variance"], f["cb"], o_r, o_v, dxc=dxc)
    rt_r, rt_v = D.resolve_temporal(tiles, count, f["roughness8"], avg, avg_fmt, rp_r, rep, rp_v, f["sample_count"], f["cb"], o_r, o_v, dxc=dxc)
    assert_bits(p_r, rp_r, f"{what}: prefiltered radiance")
    assert_bits(p_v, rp_v, f"{what}: prefiltered variance")
    assert_bits(t_r, rt_r, f"{what}: resolved radiance")
    assert_bits(t_v, rt_v, f"{what}: resolved variance")
    return rp_r, rp_v, rt_r, rt_v


# ---- white noise, every tile listed ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dxc", [False, True])
@pytest.mark.parametrize("W,H,smooth", [(8, 8, False), (9, 9, False), (67, 45, False), (67, 45, True)])
def test_white_noise_every_format_combination(ctx, W, H, smooth, dxc):
    f = frame(W, H, 0xD00 + W, smooth=smooth)
    ctx.set_arithmetic(dxc)
    try:
        for rad_fmt, out_fmt, normal_fmt, avg_fmt in itertools.product([F16, F32], [F16, F32], [N10, F32], [R11, F32]):
            out = run_both(ctx, f, all_tiles(W, H), rad_fmt=rad_fmt, out_fmt=out_fmt, normal_fmt=normal_fmt, avg_fmt=avg_fmt, dxc=dxc,
                           what=f"{'smooth' if smooth else 'noise'} {W} x {H} dxc {dxc} formats {rad_fmt}/{out_fmt}/{normal_fmt}/{avg_fmt}")
            assert not (out[1] == SENTINEL).any() and not (out[3] == SENTINEL).any()
    finally:
        ctx.set_arithmetic(False)


def test_sparse_shuffled_list_with_a_duplicate_and_an_entry_beyond_the_grid(ctx):
    W, H = 256, 144
    f = frame(W, H, 0x256)
    rng = np.random.default_rng(0x5BA5)
    every = all_tiles(W, H)
    pick = rng.choice(every.size, 150, replace=False)
    tiles = every[pick].copy()
    tiles[::3] += np.uint32((5 << 16) | 3)                            # the contract's definition: the tile of an entry is (x >> 3, y >> 3) (vqhip_ssr_classify writes aligned entries)
    tiles = np.concatenate([tiles, tiles[:1], np.array([(8 << 16) | (W + 8), ((H + 16) << 16) | 0, 0xFFFFFFFF], np.uint32)])
    rng.shuffle(tiles)
    _, rp_v, _, rt_v = run_both(ctx, f, tiles, what="sparse list")
    listed = np.zeros((H, W), bool)
    for e in every[pick]:
        x, y = int(e & 0xFFFF), int(e >> 16)
        listed[y:y + 8, x:x + 8] = True
    for v in (rp_v, rt_v):                                            # the statement itself: listed tiles written, every other pixel untouched
        assert (v[listed] != SENTINEL).all() and (v[~listed] == SENTINEL).all()


def test_tile_count_zero_and_count_above_the_grid(ctx):
    W, H = 40, 24
    f = frame(W, H, 0x40)
    out = run_both(ctx, f, all_tiles(W, H), count=0, what="count 0")
    assert all((o == SENTINEL).all() for o in out)
    out = run_both(ctx, f, all_tiles(W, H), count=0xFFFFFFF0, what="count above the grid")       # clamped on the device to 5 x 3 tiles
    assert not (out[3] == SENTINEL).any()


def test_pitched_buffers(ctx):
    W, H = 67, 45
    f = frame(W, H, 0x717C)
    P = W + 13
    tiles = all_tiles(W, H)
    rad, rep = _img(f["radiance"], F16), _img(f["reprojected"], F16)
    o_r, o_v = np.full((H, W, 4), SENTINEL, np.float16), np.full((H, W), SENTINEL, np.float16)

    def pitched(a, fill):
        a = dev(a)
        out = torch.full((H, P) + tuple(a.shape[2:]), fill, dtype=a.dtype, device="cuda")
        out[:, :W] = a
        return out
    dp, nm, rd, rp, vr, sc = (pitched(f["depth"], 0.5), pitched(f["packed"].view(np.int32), 0), pitched(rad, 9.0), pitched(rep, 9.0), pitched(f["variance"], 9.0),
                              pitched(f["sample_count"], 9.0))
    p_r, p_v, t_r, t_v = pitched(o_r, SENTINEL), pitched(o_v, SENTINEL), pitched(o_r, SENTINEL), pitched(o_v, SENTINEL)
    dt, dc, d8, da = _dtiles(tiles, W, H), dev(np.array([0, tiles.size], np.uint32).view(np.int32)), dev(f["roughness8"]), dev(f["average_r11"].view(np.int32))
    lib, p = ctx.lib, lambda t: t.data_ptr()
    rc = lib.vqhip_ssr_prefilter(ctx._h, None, p(dt), p(dc), p(dp), P, p(nm), N10, P, p(d8), p(da), R11, p(rd), F16, P, p(vr), P, f["cb"], p(p_r), F16, P, p(p_v), P)
    assert rc == 0, lib.vqhip_last_error(ctx._h)
    rc = lib.vqhip_ssr_resolve_temporal(ctx._h, None, p(dt), p(dc), p(d8), p(da), R11, p(p_r), F16, P, p(rp), F16, P, p(p_v), P, p(sc), P, f["cb"],
                                        p(t_r), F16, P, p(t_v), P)
    assert rc == 0, lib.vqhip_last_error(ctx._h)
    torch.cuda.synchronize()
    rp_r, rp_v = D.prefilter(tiles, tiles.size, f["depth"], f["packed"], N10, f["roughness8"], f["average_r11"], R11, rad, f["variance"], f["cb"], o_r, o_v)
    rt_r, rt_v = D.resolve_temporal(tiles, tiles.size, f["roughness8"], f["average_r11"], R11, rp_r, rep, rp_v, f["sample_count"], f["cb"], o_r, o_v)
    for got, ref, what in ((p_r, rp_r, "prefiltered radiance"), (p_v, rp_v, "prefiltered variance"), (t_r, rt_r, "resolved radiance"), (t_v, rt_v, "resolved variance")):
        assert_bits(got[:, :W].contiguous(), ref, f"pitched {what}")
        assert (got[:, W:] == SENTINEL).all(), f"pitched {what}: the padding was written"


def test_non_default_stream(ctx):
    f = frame(67, 45, 0x57)
    torch.cuda.synchronize()
    run_both(ctx, f, all_tiles(67, 45), stream=torch.cuda.Stream(), what="second stream")


def special_frame():
    """planted special values: inf / NaN / 1e6 radiance (RGBA32F: 1e6 becomes inf in the neighbourhood), inf and NaN variance and sample counts, zero-vector
    and NaN normals, far-plane depth, inf / NaN / denormal texels of the average radiance"""
    W, H = 24, 24
    f = frame(W, H, 0x5BEC)
    rng = np.random.default_rng(0x5BEC)
    vals = np.array([np.inf, np.nan, 1e6, 65520.0, 0.0, 6e-8, 1e-30], np.float32)
    for name in ("radiance", "reprojected"):
        ys, xs, cs = rng.integers(0, H, 40), rng.integers(0, W, 40), rng.integers(0, 3, 40)
        f[name][ys, xs, cs] = vals[rng.integers(0, vals.size, 40)]
    for name in ("variance", "sample_count"):
        ys, xs = rng.integers(0, H, 20), rng.integers(0, W, 20)
        f[name][ys, xs] = np.array([np.inf, np.nan, 65504.0, 0.0, 6e-8], np.float16)[rng.integers(0, 5, 20)]
    f["n01"][rng.integers(0, H, 10), rng.integers(0, W, 10), :3] = 0.5                      # normalize(0, 0, 0)
    f["n01"][rng.integers(0, H, 4), rng.integers(0, W, 4), 0] = np.nan
    f["depth"][rng.integers(0, H, 20), rng.integers(0, W, 20)] = 1.0
    f["average"][0, 0, :3], f["average"][1, 1, 0], f["average"][2, 0, 1] = np.inf, np.nan, 3e-6
    f["average_r11"][0, 0] = (31 << 6) | (31 << 17) | (31 << 27)                             # inf, inf, inf
    f["average_r11"][1, 1] = ((31 << 6) | 5) | (3 << 11) | (1 << 22)                         # NaN, denormal, denormal
    f["roughness8"][:] = rng.integers(11, 51, (H, W))                                        # all glossy: every pixel takes the long paths
    return f


@pytest.mark.parametrize("rad_fmt,normal_fmt,avg_fmt", [(F32, F32, F32), (F16, N10, R11)])
def test_special_values(ctx, rad_fmt, normal_fmt, avg_fmt):
    f = special_frame()
    _, _, rt_r, rt_v = run_both(ctx, f, all_tiles(24, 24), rad_fmt=rad_fmt, out_fmt=F32, normal_fmt=normal_fmt, avg_fmt=avg_fmt, what="special values")
    assert np.isfinite(rt_r).all() and np.isfinite(rt_v.astype(np.float32)).all(), "the inf / NaN guard leaves nothing non-finite behind"


def test_argument_refusals(ctx):
    W, H = 40, 24
    f = frame(W, H, 0x4EF)
    tiles = all_tiles(W, H)
    dt, dc = _dtiles(tiles, W, H), dev(np.array([0, tiles.size], np.uint32).view(np.int32))
    dp, nm, d8, da = dev(f["depth"]), dev(f["packed"].view(np.int32)), dev(f["roughness8"]), dev(f["average_r11"].view(np.int32))
    rd, rp, vr, sc = dev(_img(f["radiance"], F16)), dev(_img(f["reprojected"], F16)), dev(f["variance"]), dev(f["sample_count"])
    o_r = torch.full((H, W, 4), SENTINEL, dtype=torch.float16, device="cuda")
    o_v = torch.full((H, W), SENTINEL, dtype=torch.float16, device="cuda")
    lib, p = ctx.lib, lambda t: t.data_ptr() if t is not None else None
    INV, UNS = abi.VQHIP_ERR_INVALID_ARG, abi.VQHIP_ERR_UNSUPPORTED
    err = lambda: lib.vqhip_last_error(ctx._h).decode()

    def cb_dims(w, h):
        cb = synth.ssr_constants(W, H, 1)
        cb.bufferDimensions[0], cb.bufferDimensions[1] = w, h
        return cb

    def pre(tl=dt, cnt=dc, depth=dp, normals=nm, nfmt=N10, r8=d8, avg=da, afmt=R11, rad=rd, rfmt=F16, rpitch=0, var=vr, cb=f["cb"], out=o_r, ofmt=F16, ovar=o_v):
        return lib.vqhip_ssr_prefilter(ctx._h, None, p(tl), p(cnt), p(depth), 0, p(normals), nfmt, 0, p(r8), p(avg), afmt, p(rad), rfmt, rpitch, p(var), 0, cb,
                                       p(out), ofmt, 0, p(ovar), 0)

    def res(tl=dt, cnt=dc, r8=d8, avg=da, afmt=R11, rad=rd, rfmt=F16, rep=rp, pfmt=F16, var=vr, cnt16=sc, spitch=0, cb=f["cb"], out=o_r, ofmt=F16, ovar=o_v):
        return lib.vqhip_ssr_resolve_temporal(ctx._h, None, p(tl), p(cnt), p(r8), p(avg), afmt, p(rad), rfmt, 0, p(rep), pfmt, 0, p(var), 0, p(cnt16), spitch, cb,
                                              p(out), ofmt, 0, p(ovar), 0)
    # everything below is refused before a launch: the outputs keep the sentinel
    for call, nulls in ((pre, ("tl", "cnt", "depth", "normals", "r8", "avg", "rad", "var", "out", "ovar")), (res, ("tl", "cnt", "r8", "avg", "rad", "rep", "var", "cnt16", "out", "ovar"))):
        for k in nulls:
            assert call(**{k: None}) == INV and "NULL" in err(), k
        assert call(cb=None) == INV and "NULL" in err()
        assert call(out=dt) == INV and "overlaps" in err()                   # an output over the tile list / its counters
        assert call(ovar=dc) == INV and "overlaps" in err()
        assert call(cb=cb_dims(4097, 8)) == UNS and "4096" in err()
        assert call(cb=cb_dims(8, 4097)) == UNS
        assert call(cb=cb_dims(0, 8)) == INV
        assert call(afmt=F16) == UNS and call(rfmt=abi.FMT_RGBA8_UNORM) == UNS and call(ofmt=N10) == UNS and call(ofmt=R11) == UNS
        assert call(out=rd) == INV and "overlaps" in err()                   # aliasing: equal base pointers
        assert call(ovar=vr) == INV and "overlaps" in err()
        assert call(out=da) == INV
    assert pre(nfmt=F16) == UNS and pre(rpitch=W - 1) == INV and "pitch" in err()
    assert pre(out=dp) == INV and pre(out=nm) == INV
    assert res(pfmt=R11) == UNS and res(spitch=W - 1) == INV
    assert res(out=rp) == INV and res(ovar=sc) == INV
    torch.cuda.synchronize()
    assert (o_r == SENTINEL).all() and (o_v == SENTINEL).all(), "a refused call launched something"
    with pytest.raises(ValueError):
        ctx.ssr_prefilter(dt[:3], dc, dp, nm, N10, d8, da, R11, rd, F16, vr, f["cb"])


# ---- the room -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    e = ref_cases.small_env()
    keep = []
    return {"e": e, "henv": ref_cases.host_env(e), "denv": ref_cases.dev_env(e, keep), "keep": keep}


def test_whole_chain_on_the_room(ctx, small):
    """vqhip_ssr_environment_fallback -> vqhip_ssr_classify -> vqhip_ssr_intersect -> vqhip_ssr_prefilter -> vqhip_ssr_resolve_temporal ->
    vqhip_composite_reflections at 640 x 360 against the same chain in numpy / the oracle; Reproject's four planes are this test's stand-in
    (synth.ssr_denoise_planes around the traced radiance)"""
    w, h = 640, 360
    rm = synth.ssr_room(w, h, small["e"]["spec_mips"])
    cb = rm["cb"]
    scene = rm["scene"].astype(np.float16)
    levels = depth_ref.hierarchy(rm["depth"])
    # reference chain
    rad, r8 = O.ssr_environment_fallback(scene, F16, rm["depth"], rm["packed"], N10, cb, small["henv"], F16, extract_roughness=True)
    want = R.classify(scene, rm["depth"], cb)
    rad = R.intersect(want["rays"], want["rays"].size, scene, levels, rm["packed"], N10, r8, rm["noise"], cb, small["henv"], rad)
    pl = synth.ssr_denoise_planes(w, h, seed=0xC4A1, radiance=rad.astype(np.float32))
    rep = pl["reprojected"].astype(np.float16)
    zr, zv = np.zeros((h, w, 4), np.float16), np.zeros((h, w), np.float16)
    p_r, p_v = D.prefilter(want["tiles"], want["tiles"].size, rm["depth"], rm["packed"], N10, r8, pl["average_r11"], R11, rad, pl["variance"], cb, zr, zv)
    t_r, t_v = D.resolve_temporal(want["tiles"], want["tiles"].size, r8, pl["average_r11"], R11, p_r, rep, p_v, pl["sample_count"], cb, zr, zv)
    final = O.composite_reflections(t_r, scene, F16)
    # the library
    dscene, nrm = dev(scene), dev(rm["packed"].view(np.int32))
    glevels = ctx.depth_hierarchy(dev(rm["depth"]))
    grad, g8 = ctx.ssr_environment_fallback(dscene, F16, glevels[0].contiguous(), nrm, N10, cb, small["denv"], F16, extract_roughness=True)
    rays, counters, tiles = ctx.ssr_classify(dscene, F16, glevels[0], cb)
    ctx.ssr_intersect(rays, counters, dscene, F16, glevels, nrm, N10, g8, dev(rm["noise"]), cb, small["denv"], grad, F16)
    da, dvar = dev(pl["average_r11"].view(np.int32)), dev(pl["variance"])
    gp_r, gp_v = ctx.ssr_prefilter(tiles, counters, glevels[0], nrm, N10, g8, da, R11, grad, F16, dvar, cb, out=dev(zr), out_variance=dev(zv))
    gt_r, gt_v = ctx.ssr_resolve_temporal(tiles, counters, g8, da, R11, gp_r, F16, dev(rep), F16, gp_v, dev(pl["sample_count"]), cb, out=dev(zr), out_variance=dev(zv))
    resolved = _np(gt_r).copy()
    ctx.composite_reflections(gt_r, dscene, F16)
    torch.cuda.synchronize()
    assert_bits(grad, rad, "chain: traced radiance")
    assert_bits(gp_r, p_r, "chain: prefiltered radiance")
    assert_bits(gp_v, p_v, "chain: prefiltered variance")
    assert_bits(resolved, t_r, "chain: resolved radiance")
    assert_bits(gt_v, t_v, "chain: resolved variance")
    assert_bits(dscene, final, "chain: composited scene colour")


def test_room_1080p_on_64_seeded_tiles(ctx):
    """1920 x 1080: the statement takes a tile subset; the planes are built around a smooth stand-in radiance (the lit scene of the room)"""
    w, h = 1920, 1080
    rm = synth.ssr_room(w, h, 1)
    f = synth.ssr_denoise_planes(w, h, seed=0x1080, radiance=rm["scene"])
    f.update(depth=rm["depth"], packed=rm["packed"], n01=rm["n01"], cb=rm["cb"])
    f["roughness8"] = ref_cases.to_unorm8(rm["scene"][..., 3].astype(np.float32))
    tiles = np.random.default_rng(0x1080).choice(all_tiles(w, h), 64, replace=False)
    _, _, _, rt_v = run_both(ctx, f, tiles, what="room 1920 x 1080, 64 tiles")
    assert (rt_v != SENTINEL).sum() >= 64 * 64 - 8 * 64
