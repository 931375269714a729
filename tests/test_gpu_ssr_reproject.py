"""-m gpu: vqhip_ssr_reproject (csrc/ssr_reproject.hip, docs/DESIGN_DETAILS.md §7.13) through the C ABI against tests/ssr_reproject_ref.py, bit for bit, no
tolerance anywhere: the designed frames of synth.ssr_reproject_frames with every tile listed in both arithmetic readings and every format combination, a shuffled
sparse list with a duplicate and an entry beyond the grid, an empty list, pitched buffers, a second stream running the three denoiser passes back to back, special
values, refusals, and two consecutive frames of fallback -> classify -> intersect -> reproject -> prefilter -> resolve -> composite on synth.ssr_room with the
engine's ping-pong. Each GPU step runs once."""
import itertools

import numpy as np
import pytest
import torch

from tests import depth_ref
from tests import oracle_lib as O
from tests import ref_cases
from tests import ssr_denoise_ref as D
from tests import ssr_reproject_ref as P
from tests import ssr_trace_ref as R
from vqengine_amd import abi, synth

pytestmark = pytest.mark.gpu
dev = ref_cases._dev
F16, F32, N10, R11, M16, M32 = abi.FMT_RGBA16F, abi.FMT_RGBA32F, abi.FMT_R10G10B10A2_UNORM, abi.FMT_R11G11B10_FLOAT, abi.FMT_RG16F, abi.FMT_RG32F
SENTINEL = -7.0                     # no store of the pass can produce it: the variance is a lerp of squares or 1, the sample count is >= 1, the radiance alpha is 0
AVG_SENTINEL = 0x80000000           # as an R11G11B10 word: not an encode of the pass for this input (blue would be 2^1 * 1.0 with red and green 0)
FORMATS = dict(normal_fmt=N10, hist_normal_fmt=N10, rad_fmt=F16, hist_fmt=F16, motion_fmt=M16, out_fmt=F16, avg_fmt=R11)


def _np(t):
    return t.cpu().numpy()


def assert_bits(got, ref, what):
    n, idx = O.bits_equal(_np(got) if hasattr(got, "cpu") else got, ref)
    assert n == 0, f"{what}: {n} mismatching elements, first {idx.tolist()}"


def all_tiles(w, h):
    tx, ty = (w + 7) // 8, (h + 7) // 8
    return np.array([((y * 8) << 16) | (x * 8) for y in range(ty) for x in range(tx)], np.uint32)


def _dtiles(tiles, w, h):
    buf = np.zeros(((w + 7) // 8) * ((h + 7) // 8), np.uint32)
    buf[:min(len(tiles), buf.size)] = tiles[:buf.size]
    return dev(buf.view(np.int32))


def _img(a, fmt):
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(a.astype(np.float16 if fmt in (F16, M16) else np.float32))


def host_inputs(f, normal_fmt, hist_normal_fmt, rad_fmt, hist_fmt, motion_fmt):
    """the planes in the chosen formats, in the statement's argument order after (tiles, count)"""
    return dict(depth=f["depth"], normals=f["packed"] if normal_fmt == N10 else f["n01"], roughness8=f["roughness8"], depth_hist=f["depth_hist"],
                normal_hist=f["packed_hist"] if hist_normal_fmt == N10 else f["n01_hist"], roughness8_hist=f["roughness8_hist"],
                radiance=_img(f["radiance"], rad_fmt), radiance_hist=_img(f["radiance_hist"], hist_fmt), motion=_img(f["motion"], motion_fmt),
                variance_hist=f["variance_hist"], sample_count_hist=f["sample_count_hist"])


def host_outputs(w, h, out_fmt, avg_fmt):
    h8, w8 = (h + 7) // 8, (w + 7) // 8
    avg = np.full((h8, w8), AVG_SENTINEL, np.uint32) if avg_fmt == R11 else np.full((h8, w8, 4), SENTINEL, np.float32)
    return (np.full((h, w, 4), SENTINEL, np.float16 if out_fmt == F16 else np.float32), avg, np.full((h, w), SENTINEL, np.float16), np.full((h, w), SENTINEL, np.float16))


def statement(f, tiles, count, hi, outs, fm, dxc=False, stats=None):
    return P.reproject(tiles, count, hi["depth"], hi["normals"], fm["normal_fmt"], hi["roughness8"], hi["depth_hist"], hi["normal_hist"], fm["hist_normal_fmt"],
                       hi["roughness8_hist"], hi["radiance"], hi["radiance_hist"], hi["motion"], hi["variance_hist"], hi["sample_count_hist"], f["cb"],
                       outs[0], outs[1], fm["avg_fmt"], outs[2], outs[3], dxc=dxc, stats=stats)


def device_call(ctx, f, dt, dc, hi, outs, fm, stream=None):
    word = lambda a, fmt: dev(a.view(np.int32)) if fmt == N10 else dev(a)                                            # noqa: E731
    d_avg = dev(outs[1].view(np.int32)) if fm["avg_fmt"] == R11 else dev(outs[1])
    return ctx.ssr_reproject(dt, dc, dev(hi["depth"]), word(hi["normals"], fm["normal_fmt"]), fm["normal_fmt"], dev(hi["roughness8"]), dev(hi["depth_hist"]),
                             word(hi["normal_hist"], fm["hist_normal_fmt"]), fm["hist_normal_fmt"], dev(hi["roughness8_hist"]), dev(hi["radiance"]), fm["rad_fmt"],
                             dev(hi["radiance_hist"]), fm["hist_fmt"], dev(hi["motion"]), fm["motion_fmt"], dev(hi["variance_hist"]), dev(hi["sample_count_hist"]), f["cb"],
                             out_reprojected=dev(outs[0]), out_fmt=fm["out_fmt"], out_average=d_avg, avg_fmt=fm["avg_fmt"], out_variance=dev(outs[2]),
                             out_sample_count=dev(outs[3]), stream=stream)


def compare(got, ref, fm, what):
    g_avg = _np(got[1]).view(np.uint32) if fm["avg_fmt"] == R11 else got[1]
    assert_bits(got[0], ref[0], f"{what}: reprojected radiance")
    assert_bits(g_avg, ref[1], f"{what}: average radiance")
    assert_bits(got[2], ref[2], f"{what}: variance")
    assert_bits(got[3], ref[3], f"{what}: sample count")


def run(ctx, f, tiles, count=None, dxc=False, what="", stats=None, **formats):
    fm = dict(FORMATS, **formats)
    w, h = int(f["cb"].bufferDimensions[0]), int(f["cb"].bufferDimensions[1])
    count = len(tiles) if count is None else count
    hi = host_inputs(f, fm["normal_fmt"], fm["hist_normal_fmt"], fm["rad_fmt"], fm["hist_fmt"], fm["motion_fmt"])
    outs = host_outputs(w, h, fm["out_fmt"], fm["avg_fmt"])
    got = device_call(ctx, f, _dtiles(tiles, w, h), dev(np.array([0, count], np.uint32).view(np.int32)), hi, outs, fm)
    torch.cuda.synchronize()
    ref = statement(f, tiles, count, hi, outs, fm, dxc=dxc, stats=stats)
    compare(got, ref, fm, what)
    return ref


# ---- the designed frames, every tile listed ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dxc", [False, True])
@pytest.mark.parametrize("W,H", [(8, 8), (9, 9), (67, 45)])
def test_designed_frames_both_readings(ctx, W, H, dxc):
    f = synth.ssr_reproject_frames(W, H, seed=0x4E00 + W)
    ctx.set_arithmetic(dxc)
    try:
        st = {}
        ref = run(ctx, f, all_tiles(W, H), dxc=dxc, what=f"{W} x {H} dxc {dxc}", stats=st)
    finally:
        ctx.set_arithmetic(False)
    assert (ref[1] != AVG_SENTINEL).all(), "every tile's average texel is written"
    glossy = f["roughness8"].astype(np.float32) / np.float32(255.0) < np.float32(f["cb"].roughnessThreshold)
    assert ((ref[2] != SENTINEL) == glossy).all() and ((ref[3] != SENTINEL) == glossy).all(), "glossy pixels are stored, the others keep their bytes"
    if (W, H) == (67, 45):                                                                    # the comparison above went through every branch
        for k in ("hit", "surface", "discard", "early_out", "search", "slow", "uv_outside"):
            assert st[k].sum() >= 32, k
        assert (~st["glossy"]).sum() >= 32


@pytest.mark.parametrize("dxc", [False, True])
def test_every_format_combination_at_8x8(ctx, dxc):
    f = synth.ssr_reproject_frames(8, 8, seed=0xF08)
    f["roughness8"][:] = np.where(np.arange(8)[None, :] < 6, 25, 200)                          # glossy columns and two rough ones
    ctx.set_arithmetic(dxc)
    try:
        for nf, hnf, rf, hf, mf, of, af in itertools.product([N10, F32], [N10, F32], [F16, F32], [F16, F32], [M16, M32], [F16, F32], [R11, F32]):
            run(ctx, f, all_tiles(8, 8), dxc=dxc, normal_fmt=nf, hist_normal_fmt=hnf, rad_fmt=rf, hist_fmt=hf, motion_fmt=mf, out_fmt=of, avg_fmt=af,
                what=f"8 x 8 dxc {dxc} formats {nf}/{hnf}/{rf}/{hf}/{mf}/{of}/{af}")
    finally:
        ctx.set_arithmetic(False)


@pytest.mark.parametrize("formats", [dict(normal_fmt=F32, hist_normal_fmt=F32, rad_fmt=F32, hist_fmt=F32, motion_fmt=M32, out_fmt=F32, avg_fmt=F32),
                                     dict(rad_fmt=F32, hist_fmt=F16, out_fmt=F32), dict(normal_fmt=F32, motion_fmt=M32, avg_fmt=F32), dict(hist_normal_fmt=F32, hist_fmt=F32)])
def test_format_cross_section_at_67x45(ctx, formats):
    f = synth.ssr_reproject_frames(67, 45, seed=0x6745)
    run(ctx, f, all_tiles(67, 45), what=f"67 x 45 formats {formats}", **formats)


@pytest.mark.parametrize("dxc", [False, True])
def test_disocclusion_factor_exactly_at_the_threshold(ctx, dxc):
    """synth.ssr_reproject_threshold_frames: every glossy pixel's factor is the word of 0.9f — neither the early-out nor the search nor the 2 x 2 path, history kept"""
    f = synth.ssr_reproject_threshold_frames()
    ctx.set_arithmetic(dxc)
    try:
        st = {}
        run(ctx, f, all_tiles(16, 16), dxc=dxc, what=f"threshold dxc {dxc}", stats=st, normal_fmt=F32, hist_normal_fmt=F32)
    finally:
        ctx.set_arithmetic(False)
    assert st["kept"].sum() == 64 and st["early_out"].sum() == 0 and st["search"].sum() == 0 and st["slow"].sum() == 0


def magnitude_frames():
    """64 x 40, rough everywhere (the average is the weighted mean of the traced radiance alone), tile t scaled by 2^(2 t - 30): the 40 averages run from below the
    smallest R11G11B10 denormal through the denormal and normal ranges to binary16 overflow in the downsample (inf)"""
    W, H = 64, 40
    f = synth.ssr_reproject_frames(W, H, seed=0x3A6)
    f["roughness8"][:] = 255
    ys, xs = np.mgrid[0:H, 0:W]
    f["radiance"][..., :3] *= np.exp2(2.0 * ((ys // 8) * 8 + xs // 8) - 30.0).astype(np.float32)[..., None]
    return f


def test_average_encode_across_magnitudes(ctx):
    """the device's R11G11B10 encode and downsample on averages of every class a finite radiance reaches: zero, denormal, normal, inf — both average formats against the statement"""
    f = magnitude_frames()
    words = run(ctx, f, all_tiles(64, 40), what="magnitudes, R11G11B10", rad_fmt=F32)[1]
    run(ctx, f, all_tiles(64, 40), what="magnitudes, RGBA32F", rad_fmt=F32, avg_fmt=F32)
    e, m = (words >> 6) & 31, words & 63                                  # the red field
    assert (words & 0x7FF == 0).any() and ((e == 0) & (m != 0)).sum() >= 2 and ((e > 0) & (e < 31)).sum() >= 8 and ((e == 31) & (m == 0)).any()


def test_sparse_shuffled_list_with_a_duplicate_and_an_entry_beyond_the_grid(ctx):
    W, H = 64, 40
    f = synth.ssr_reproject_frames(W, H, seed=0x6440)
    rng = np.random.default_rng(0x5BA5)
    every = all_tiles(W, H)
    pick = rng.choice(every.size, 17, replace=False)
    tiles = every[pick].copy()
    tiles[::3] += np.uint32((5 << 16) | 3)                            # the tile of an entry is (x >> 3, y >> 3)
    tiles = np.concatenate([tiles, tiles[:1], np.array([(8 << 16) | (W + 8), ((H + 16) << 16) | 0, 0xFFFFFFFF], np.uint32)])
    rng.shuffle(tiles)
    st = {}
    ref = run(ctx, f, tiles, what="sparse list", stats=st)
    listed = np.zeros((H, W), bool)
    listed8 = np.zeros((H // 8, W // 8), bool)
    for e in every[pick]:
        x, y = int(e & 0xFFFF), int(e >> 16)
        listed[y:y + 8, x:x + 8] = True
        listed8[y // 8, x // 8] = True
    glossy = f["roughness8"].astype(np.float32) / np.float32(255.0) < np.float32(f["cb"].roughnessThreshold)
    for plane in (ref[0][..., 3], ref[2], ref[3]):                    # the statement itself: glossy pixels of listed tiles written, every other pixel untouched
        assert ((plane != SENTINEL) == (listed & glossy)).all()
    assert ((ref[1] != AVG_SENTINEL) == listed8).all()                # ... and the average texels of unlisted tiles


def test_tile_count_zero_and_count_above_the_grid(ctx):
    W, H = 40, 24
    f = synth.ssr_reproject_frames(W, H, seed=0x4024)
    ref = run(ctx, f, all_tiles(W, H), count=0, what="count 0")
    assert all((o == s).all() for o, s in zip(ref, (SENTINEL, AVG_SENTINEL, SENTINEL, SENTINEL)))
    ref = run(ctx, f, all_tiles(W, H), count=0xFFFFFFF0, what="count above the grid")         # clamped on the device to 5 x 3 tiles
    assert (ref[1] != AVG_SENTINEL).all()


def test_pitched_buffers(ctx):
    W, H = 67, 45
    P_ = W + 13
    f = synth.ssr_reproject_frames(W, H, seed=0x717C)
    tiles = all_tiles(W, H)
    hi = host_inputs(f, N10, N10, F16, F16, M16)
    outs = host_outputs(W, H, F16, R11)
    keep = []

    def pitched(a, fill):
        a = dev(a)
        out = torch.full((H, P_) + tuple(a.shape[2:]), fill, dtype=a.dtype, device="cuda")
        out[:, :W] = a
        keep.append(out)
        return out
    s = abi.SSRReprojectSurfaces()
    dt, dc, d_avg = _dtiles(tiles, W, H), dev(np.array([0, tiles.size], np.uint32).view(np.int32)), dev(outs[1].view(np.int32))
    s.tile_list, s.counters, s.out_average = dt.data_ptr(), dc.data_ptr(), d_avg.data_ptr()
    for name, arr, fill in (("depth", hi["depth"], 0.5), ("normals", hi["normals"].view(np.int32), 0), ("roughness", hi["roughness8"], 3), ("depth_history", hi["depth_hist"], 0.5),
                            ("normal_history", hi["normal_hist"].view(np.int32), 0), ("roughness_history", hi["roughness8_hist"], 3), ("radiance", hi["radiance"], 9.0),
                            ("radiance_history", hi["radiance_hist"], 9.0), ("motion_vectors", hi["motion"], 9.0), ("variance_history", hi["variance_hist"], 9.0),
                            ("sample_count_history", hi["sample_count_hist"], 9.0), ("out_reprojected", outs[0], SENTINEL), ("out_variance", outs[2], SENTINEL),
                            ("out_sample_count", outs[3], SENTINEL)):
        setattr(s, name, pitched(arr, fill).data_ptr())
    for name in ("depth", "normals", "roughness", "depth_history", "normal_history", "roughness_history", "radiance", "radiance_history", "variance_history",
                 "sample_count_history", "out_reprojected", "out_variance", "out_sample_count"):
        setattr(s, name + "_pitch_px", P_)
    s.motion_pitch_px = P_
    s.normals_fmt, s.normal_history_fmt, s.radiance_fmt, s.radiance_history_fmt, s.motion_fmt, s.out_reprojected_fmt, s.out_average_fmt = N10, N10, F16, F16, M16, F16, R11
    rc = ctx.lib.vqhip_ssr_reproject(ctx._h, None, s, f["cb"])
    assert rc == 0, ctx.lib.vqhip_last_error(ctx._h)
    torch.cuda.synchronize()
    ref = statement(f, tiles, tiles.size, hi, outs, FORMATS)
    g_rep, g_var, g_cnt = keep[-3], keep[-2], keep[-1]
    for got, want, what in ((g_rep, ref[0], "reprojected radiance"), (g_var, ref[2], "variance"), (g_cnt, ref[3], "sample count")):
        assert_bits(got[:, :W].contiguous(), want, f"pitched {what}")
        assert (got[:, W:] == SENTINEL).all(), f"pitched {what}: the padding was written"
    assert_bits(_np(d_avg).view(np.uint32), ref[1], "pitched: average radiance")


def test_second_stream_three_passes_back_to_back(ctx):
    """reproject -> prefilter -> resolve on a non-default stream without a host synchronisation in between, against the three statements chained"""
    W, H = 67, 45
    f = synth.ssr_reproject_frames(W, H, seed=0x57)
    tiles = all_tiles(W, H)
    hi = host_inputs(f, N10, N10, F16, F16, M16)
    zr, zv = np.zeros((H, W, 4), np.float16), np.zeros((H, W), np.float16)
    outs = (zr, np.zeros(((H + 7) // 8, (W + 7) // 8), np.uint32), zv, zv)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        dt, dc = _dtiles(tiles, W, H), dev(np.array([0, tiles.size], np.uint32).view(np.int32))
        rep, avg, var, cnt = device_call(ctx, f, dt, dc, hi, outs, FORMATS, stream=stream)
        dn, d8, dd, drad = dev(hi["normals"].view(np.int32)), dev(hi["roughness8"]), dev(hi["depth"]), dev(hi["radiance"])
        p_r, p_v = ctx.ssr_prefilter(dt, dc, dd, dn, N10, d8, avg, R11, drad, F16, var, f["cb"], out=dev(zr), out_variance=dev(zv), stream=stream)
        t_r, t_v = ctx.ssr_resolve_temporal(dt, dc, d8, avg, R11, p_r, F16, rep, F16, p_v, cnt, f["cb"], out=dev(zr), out_variance=dev(zv), stream=stream)
    torch.cuda.synchronize()
    ref = statement(f, tiles, tiles.size, hi, outs, FORMATS)
    compare((rep, avg, var, cnt), ref, FORMATS, "second stream")
    rp_r, rp_v = D.prefilter(tiles, tiles.size, hi["depth"], hi["normals"], N10, hi["roughness8"], ref[1], R11, hi["radiance"], ref[2], f["cb"], zr, zv)
    rt_r, rt_v = D.resolve_temporal(tiles, tiles.size, hi["roughness8"], ref[1], R11, rp_r, ref[0], rp_v, ref[3], f["cb"], zr, zv)
    assert_bits(p_r, rp_r, "second stream: prefiltered radiance")
    assert_bits(t_r, rt_r, "second stream: resolved radiance")
    assert_bits(t_v, rt_v, "second stream: resolved variance")


@pytest.mark.parametrize("formats", [dict(normal_fmt=F32, hist_normal_fmt=F32, rad_fmt=F32, hist_fmt=F32, motion_fmt=M32, out_fmt=F32, avg_fmt=F32), dict()])
def test_special_values(ctx, formats):
    """inf / NaN / huge radiance and history, inf and NaN variance and sample-count history, NaN and huge motion vectors, zero-vector normals, far-plane depth"""
    W, H = 24, 24
    f = synth.ssr_reproject_frames(W, H, seed=0x5BEC)
    rng = np.random.default_rng(0x5BEC)
    vals = np.array([np.inf, -np.inf, np.nan, 1e6, 65520.0, 0.0, 6e-8, 1e-30], np.float32)
    for name in ("radiance", "radiance_hist"):
        ys, xs, cs = rng.integers(0, H, 40), rng.integers(0, W, 40), rng.integers(0, 4 if name == "radiance" else 3, 40)
        f[name][ys, xs, cs] = vals[rng.integers(0, vals.size, 40)]
    for name in ("variance_hist", "sample_count_hist"):
        f[name][rng.integers(0, H, 20), rng.integers(0, W, 20)] = np.array([np.inf, np.nan, 65504.0, 0.0, 6e-8], np.float16)[rng.integers(0, 5, 20)]
    f["motion"][rng.integers(0, H, 12), rng.integers(0, W, 12), rng.integers(0, 2, 12)] = np.array([np.nan, np.inf, -np.inf, 1e30, -3e4, 7.0], np.float32)[rng.integers(0, 6, 12)]
    for n01, packed in ((f["n01"], f["packed"]), (f["n01_hist"], f["packed_hist"])):
        ys, xs = rng.integers(0, H, 8), rng.integers(0, W, 8)
        n01[ys, xs, :3] = 0.5                                                                   # normalize(0, 0, 0) in the float format ...
        packed[rng.integers(0, H, 8), rng.integers(0, W, 8)] = 0                                 # ... and the word the history clear leaves in the packed one
    f["depth"][rng.integers(0, H, 20), rng.integers(0, W, 20)] = 1.0
    f["depth_hist"][rng.integers(0, H, 20), rng.integers(0, W, 20)] = 1.0
    f["roughness8"][:] = rng.integers(0, 51, (H, W))                                             # all glossy
    ref = run(ctx, f, all_tiles(W, H), what=f"special values {formats}", **formats)
    avg = D.average_rgb(ref[1], formats.get("avg_fmt", R11))
    assert np.isfinite(avg).all(), "the guard keeps inf / NaN radiance out of the average"


def test_argument_refusals(ctx):
    W, H = 40, 24
    f = synth.ssr_reproject_frames(W, H, seed=0x4EF)
    tiles = all_tiles(W, H)
    hi = host_inputs(f, N10, N10, F16, F16, M16)
    t = dict(tile_list=_dtiles(tiles, W, H), counters=dev(np.array([0, tiles.size], np.uint32).view(np.int32)), depth=dev(hi["depth"]), normals=dev(hi["normals"].view(np.int32)),
             roughness=dev(hi["roughness8"]), depth_history=dev(hi["depth_hist"]), normal_history=dev(hi["normal_hist"].view(np.int32)), roughness_history=dev(hi["roughness8_hist"]),
             radiance=dev(hi["radiance"]), radiance_history=dev(hi["radiance_hist"]), motion_vectors=dev(hi["motion"]), variance_history=dev(hi["variance_hist"]),
             sample_count_history=dev(hi["sample_count_hist"]),
             out_reprojected=torch.full((H, W, 4), SENTINEL, dtype=torch.float16, device="cuda"), out_average=torch.full((3, 5), 7, dtype=torch.int32, device="cuda"),
             out_variance=torch.full((H, W), SENTINEL, dtype=torch.float16, device="cuda"), out_sample_count=torch.full((H, W), SENTINEL, dtype=torch.float16, device="cuda"))
    fmts = dict(normals_fmt=N10, normal_history_fmt=N10, radiance_fmt=F16, radiance_history_fmt=F16, motion_fmt=M16, out_reprojected_fmt=F16, out_average_fmt=R11)
    lib = ctx.lib
    INV, UNS = abi.VQHIP_ERR_INVALID_ARG, abi.VQHIP_ERR_UNSUPPORTED
    err = lambda: lib.vqhip_last_error(ctx._h).decode()                                          # noqa: E731

    def call(cb=f["cb"], **over):
        s = abi.SSRReprojectSurfaces()
        for k, v in t.items():
            v = over.get(k, v)
            setattr(s, k, v.data_ptr() if v is not None else None)
        for k, v in fmts.items():
            setattr(s, k, over.get(k, v))
        for k, v in over.items():
            if k.endswith("_pitch_px"):
                setattr(s, k, v)
        return lib.vqhip_ssr_reproject(ctx._h, None, s, cb)

    def cb_dims(w, h):
        cb = synth.ssr_constants(W, H, 1)
        cb.bufferDimensions[0], cb.bufferDimensions[1] = w, h
        return cb
    for k in t:
        assert call(**{k: None}) == INV and "NULL" in err(), k
    assert call(cb=None) == INV and "NULL" in err()
    assert lib.vqhip_ssr_reproject(ctx._h, None, None, f["cb"]) == INV
    outs = ("out_reprojected", "out_average", "out_variance", "out_sample_count")
    for o in outs:                                                                                # an output over any input, the list or its counters
        for i in (k for k in t if k not in outs):
            assert call(**{o: t[i]}) == INV and "overlaps" in err(), (o, i)
    assert call(out_variance=t["out_sample_count"]) == INV and "overlap" in err()
    assert call(out_average=t["out_reprojected"]) == INV
    assert call(cb=cb_dims(4097, 8)) == UNS and "4096" in err()
    assert call(cb=cb_dims(8, 4097)) == UNS
    assert call(cb=cb_dims(0, 8)) == INV
    for k, bad in (("normals_fmt", F16), ("normal_history_fmt", R11), ("radiance_fmt", abi.FMT_RGBA8_UNORM), ("radiance_history_fmt", N10), ("motion_fmt", F16),
                   ("out_reprojected_fmt", R11), ("out_average_fmt", F16)):
        assert call(**{k: bad}) == UNS, k
    for k in ("depth_pitch_px", "motion_pitch_px", "sample_count_history_pitch_px", "out_variance_pitch_px"):
        assert call(**{k: W - 1}) == INV and "pitch" in err(), k
    torch.cuda.synchronize()
    assert all((t[o] == (7 if o == "out_average" else SENTINEL)).all() for o in outs), "a refused call launched something"
    with pytest.raises(ValueError):
        ctx.ssr_reproject(t["tile_list"][:3], t["counters"], t["depth"], t["normals"], N10, t["roughness"], t["depth_history"], t["normal_history"], N10, t["roughness_history"],
                          t["radiance"], F16, t["radiance_history"], F16, t["motion_vectors"], M16, t["variance_history"], t["sample_count_history"], f["cb"])


# ---- two frames of the room ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    e = ref_cases.small_env()
    keep = []
    return {"e": e, "henv": ref_cases.host_env(e), "denv": ref_cases.dev_env(e, keep), "keep": keep}


def test_temporal_chain_two_frames_on_the_room(ctx, small):
    """Two consecutive frames at 160 x 92 with a moved camera, each fallback -> classify -> intersect -> reproject -> prefilter -> resolve -> composite, with the engine's
    ping-pong (ScreenSpaceReflections.cpp:1177-1222): frame i traces into TexRadiance[i]; Reproject reads TexRadiance / TexVariance / TexSampleCount [1 - i] as history
    and writes TexReprojectedRadiance, TexAvgRadiance[i], TexVariance[i], TexSampleCount[i]; Prefilter writes TexRadiance / TexVariance [1 - i]; ResolveTemporal reads
    those and TexSampleCount[1 - i] and writes TexRadiance / TexVariance [i]. Frame 0 starts from cleared history; its outputs and surfaces are frame 1's history. Every
    intermediate plane of both frames is compared with the three statements chained on the CPU."""
    w, h = 160, 92
    h8, w8 = (h + 7) // 8, (w + 7) // 8
    cams = ((3.0, 10.0, -60.0), (3.6, 10.2, -59.2))
    rooms = [synth.ssr_room(w, h, small["e"]["spec_mips"], camera=c) for c in cams]
    for k, rm in enumerate(rooms):                                                                # the previous camera of frame k
        prev = rooms[max(k - 1, 0)]["cb"]
        m = np.array([[prev.view.m[i][j] for j in range(4)] for i in range(4)], np.float64) @ np.array([[prev.projection.m[i][j] for j in range(4)] for i in range(4)], np.float64)
        synth._set_matrix(rm["cb"].prevViewProjection, m)
        rm["motion"] = synth.ssr_motion_vectors(rm["depth"], rm["cb"]).astype(np.float16)
    z4, z1 = np.zeros((h, w, 4), np.float16), np.zeros((h, w), np.float16)
    # ---- the CPU chain
    Rad, Var, Cnt = [z4.copy(), z4.copy()], [z1.copy(), z1.copy()], [z1.copy(), z1.copy()]
    Avg, Rep = [np.zeros((h8, w8), np.uint32), np.zeros((h8, w8), np.uint32)], z4.copy()
    hist = {"depth": np.zeros((h, w), np.float32), "packed": np.zeros((h, w), np.uint32), "r8": np.zeros((h, w), np.uint8)}
    want = []
    for i, rm in enumerate(rooms):
        cb, scene = rm["cb"], rm["scene"].astype(np.float16)
        rad, r8 = O.ssr_environment_fallback(scene, F16, rm["depth"], rm["packed"], N10, cb, small["henv"], F16, extract_roughness=True)
        cl = R.classify(scene, rm["depth"], cb)
        Rad[i] = R.intersect(cl["rays"], cl["rays"].size, scene, depth_ref.hierarchy(rm["depth"]), rm["packed"], N10, r8, rm["noise"], cb, small["henv"], rad)
        traced = Rad[i].copy()
        T, n = cl["tiles"], cl["tiles"].size
        st = {}
        Rep, Avg[i], Var[i], Cnt[i] = P.reproject(T, n, rm["depth"], rm["packed"], N10, r8, hist["depth"], hist["packed"], N10, hist["r8"], Rad[i], Rad[1 - i], rm["motion"],
                                                  Var[1 - i], Cnt[1 - i], cb, Rep, Avg[i], R11, Var[i], Cnt[i], stats=st)
        reproj = (Rep.copy(), Avg[i].copy(), Var[i].copy(), Cnt[i].copy())
        Rad[1 - i], Var[1 - i] = D.prefilter(T, n, rm["depth"], rm["packed"], N10, r8, Avg[i], R11, Rad[i], Var[i], cb, Rad[1 - i], Var[1 - i])
        pre = (Rad[1 - i].copy(), Var[1 - i].copy())
        Rad[i], Var[i] = D.resolve_temporal(T, n, r8, Avg[i], R11, Rad[1 - i], Rep, Var[1 - i], Cnt[1 - i], cb, Rad[i], Var[i])
        want.append(dict(traced=traced, reproj=reproj, pre=pre, res=(Rad[i].copy(), Var[i].copy()), final=O.composite_reflections(Rad[i], scene, F16), kept=int(st["kept"].sum())))
        hist = {"depth": rm["depth"], "packed": rm["packed"], "r8": r8}
    assert want[0]["kept"] == 0, "frame 0 has no history to keep"
    assert want[1]["kept"] >= 1000, "frame 1 keeps reprojected history: frame 0's output is observable in it"
    # ---- the library, with the same buffers
    gRad, gVar, gCnt = [dev(z4), dev(z4)], [dev(z1), dev(z1)], [dev(z1), dev(z1)]
    gAvg, gRep = [dev(np.zeros((h8, w8), np.int32)), dev(np.zeros((h8, w8), np.int32))], dev(z4)
    ghist = {"depth": dev(np.zeros((h, w), np.float32)), "packed": dev(np.zeros((h, w), np.int32)), "r8": dev(np.zeros((h, w), np.uint8))}
    got = []
    for i, rm in enumerate(rooms):
        cb = rm["cb"]
        dscene, nrm = dev(rm["scene"].astype(np.float16)), dev(rm["packed"].view(np.int32))
        glevels = ctx.depth_hierarchy(dev(rm["depth"]))
        d0 = glevels[0].contiguous()
        grad, g8 = ctx.ssr_environment_fallback(dscene, F16, d0, nrm, N10, cb, small["denv"], F16, extract_roughness=True)
        gRad[i].copy_(grad)
        rays, counters, tiles = ctx.ssr_classify(dscene, F16, glevels[0], cb)
        ctx.ssr_intersect(rays, counters, dscene, F16, glevels, nrm, N10, g8, dev(rm["noise"]), cb, small["denv"], gRad[i], F16)
        traced = _np(gRad[i]).copy()
        ctx.ssr_reproject(tiles, counters, d0, nrm, N10, g8, ghist["depth"], ghist["packed"], N10, ghist["r8"], gRad[i], F16, gRad[1 - i], F16, dev(rm["motion"]), M16,
                          gVar[1 - i], gCnt[1 - i], cb, out_reprojected=gRep, out_average=gAvg[i], out_variance=gVar[i], out_sample_count=gCnt[i])
        reproj = (_np(gRep).copy(), _np(gAvg[i]).view(np.uint32).copy(), _np(gVar[i]).copy(), _np(gCnt[i]).copy())
        ctx.ssr_prefilter(tiles, counters, d0, nrm, N10, g8, gAvg[i], R11, gRad[i], F16, gVar[i], cb, out=gRad[1 - i], out_variance=gVar[1 - i])
        pre = (_np(gRad[1 - i]).copy(), _np(gVar[1 - i]).copy())
        ctx.ssr_resolve_temporal(tiles, counters, g8, gAvg[i], R11, gRad[1 - i], F16, gRep, F16, gVar[1 - i], gCnt[1 - i], cb, out=gRad[i], out_variance=gVar[i])
        res = (_np(gRad[i]).copy(), _np(gVar[i]).copy())
        ctx.composite_reflections(gRad[i], dscene, F16)
        got.append(dict(traced=traced, reproj=reproj, pre=pre, res=res, final=_np(dscene).copy()))
        ghist = {"depth": d0, "packed": nrm, "r8": g8}
    torch.cuda.synchronize()
    for i in (0, 1):
        assert_bits(got[i]["traced"], want[i]["traced"], f"frame {i}: traced radiance")
        for k, name in enumerate(("reprojected radiance", "average radiance", "variance", "sample count")):
            assert_bits(got[i]["reproj"][k], want[i]["reproj"][k], f"frame {i}: reproject: {name}")
        for k, name in enumerate(("radiance", "variance")):
            assert_bits(got[i]["pre"][k], want[i]["pre"][k], f"frame {i}: prefiltered {name}")
            assert_bits(got[i]["res"][k], want[i]["res"][k], f"frame {i}: resolved {name}")
        assert_bits(got[i]["final"], want[i]["final"], f"frame {i}: composited scene colour")
