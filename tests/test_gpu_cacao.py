"""vqhip_cacao on the GPU (docs/DESIGN_DETAILS.md §7.14): every plane the five kernels write — the deinterleaved depths with their four mips, the view-space
normals, the ping and pong occlusion / edge planes and the final AO plane — bit for bit against tests/cacao_ref.py, through the C ABI. Sizes are the smallest at
which each mechanism can go wrong: 37 x 23 (19 x 12 half resolution: less than one blur tile, partial prepare groups in both directions, a 2 x 1 mip 3, clamped last
column and row), 64 x 48 (everything divides), 125 x 93 (two blur tiles in each direction at p = 2, odd everywhere), 1280 x 720 (the room in full) and
3840 x 2160 stage by stage. Each GPU step runs once; references are computed once per case and shared."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import cacao_ref as R
from tests import oracle_lib as O
from vqengine_amd import abi, cacao, capi, synth

pytestmark = pytest.mark.gpu

R10, F32 = abi.FMT_R10G10B10A2_UNORM, abi.FMT_RGBA32F
SMALL = ((37, 23), (64, 48), (125, 93))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def scaled_radius(w):
    """the radius that gives a small frame the sampling discs 1280 x 720 has at the default 1.2 (in texels), so that its noise frame selects every depth mip"""
    return 1.2 * 640.0 / ((w + 1) // 2)


@functools.lru_cache(maxsize=None)
def inputs(kind, w, h):
    f = synth.cacao_room(w, h) if kind == "room" else synth.cacao_noise(w, h)
    return f


@functools.lru_cache(maxsize=None)
def consts(kind, w, h, variant="default"):
    f = inputs(kind, w, h)
    over = {"qualityLevel": abi.CACAO_QUALITY_HIGH}
    if kind == "noise":
        over["radius"] = scaled_radius(w)
    if variant == "other":
        over.update(radius=0.5 * (scaled_radius(w) / 1.2 if kind == "noise" else 1.0), shadowPower=1.0, sharpness=0.5, detailShadowStrength=0.0)
    return cacao.constants(w, h, f["proj"], f["normals_to_view"], cacao.settings(**over))


@functools.lru_cache(maxsize=None)
def reference(kind, w, h, blur=2, fmt=R10, variant="default"):
    f = inputs(kind, w, h)
    sh, pp = consts(kind, w, h, variant)
    return R.frame(f["depth"], f["packed"] if fmt == R10 else f["n01"], fmt, sh, pp, blur)


def normals_tensor(f, fmt):
    return dev(f["packed"].view(np.int32)) if fmt == R10 else dev(f["n01"])


def planes_to_host(work, w, h):
    v = capi.cacao_work_planes(work, w, h)
    return {"depths": [d.cpu().numpy() for d in v["depths"]], "normals": v["normals"].cpu().numpy(), "ping": v["ping"].cpu().numpy(), "pong": v["pong"].cpu().numpy()}


def assert_same(name, got, ref):
    n_bad, idx = O.bits_equal(np.asarray(got), np.asarray(ref))
    assert n_bad == 0, f"{name}: {n_bad} of {np.asarray(ref).size} elements differ from tests/cacao_ref.py, first at {idx.tolist()}"


def assert_frame(got, ao, ref, blur, label):
    for k in range(4):
        assert_same(f"{label}: depths mip {k}", got["depths"][k], ref["depths"][k])
    assert_same(f"{label}: normals", got["normals"], ref["normals"])
    assert_same(f"{label}: ping", got["ping"], ref["ping"])
    if blur:
        assert_same(f"{label}: pong", got["pong"], ref["pong"])
    assert_same(f"{label}: ao", ao, ref["ao"])


def run(ctx, kind, w, h, blur=2, fmt=R10, variant="default", stream=None):
    f = inputs(kind, w, h)
    sh, pp = consts(kind, w, h, variant)
    ao, work = ctx.cacao(dev(f["depth"]), normals_tensor(f, fmt), fmt, sh, pp, blur_passes=blur, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return ao.cpu().numpy(), planes_to_host(work, w, h)


@pytest.mark.parametrize("size", SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ("room", "noise"))
def test_small_frames_every_plane(ctx, kind, size):
    w, h = size
    ref = reference(kind, w, h)
    if kind == "noise":                                                   # maximal divergence: every mip selected, every edge path taken
        assert (ref["stats"]["mip_histogram"] > 0).all() and ref["stats"]["packed_edge_share"] > 0.9, ref["stats"]
    ao, got = run(ctx, kind, w, h)
    assert_frame(got, ao, ref, 2, f"{kind} {w}x{h}")


@pytest.mark.parametrize("passes", (0, 1, 2, 3, 8))
def test_blur_pass_counts(ctx, passes):
    """skip (apply reads ping), odd (the result is in the back tile), even, and 8: the smallest inner region, 48 x 32"""
    w, h = 125, 93
    ref = reference("room", w, h, blur=passes)
    ao, got = run(ctx, "room", w, h, blur=passes)
    assert_frame(got, ao, ref, passes, f"blurPassCount {passes}")


def test_rgba32f_normals(ctx):
    w, h = 125, 93
    ref = reference("noise", w, h, fmt=F32)
    ao, got = run(ctx, "noise", w, h, fmt=F32)
    assert_frame(got, ao, ref, 2, "RGBA32F normals")


def test_non_default_settings(ctx):
    """radius 0.5, shadowPower 1, sharpness 0.5, detailShadowStrength 0"""
    w, h = 125, 93
    for kind in ("room", "noise"):
        ref = reference(kind, w, h, variant="other")
        ao, got = run(ctx, kind, w, h, variant="other")
        assert_frame(got, ao, ref, 2, f"other settings, {kind}")


def test_pitched_buffers_keep_their_padding(ctx):
    w, h = 125, 93
    f = inputs("room", w, h)
    sh, pp = consts("room", w, h)
    ref = reference("room", w, h)
    depth = torch.full((h, w + 7), float("nan"), dtype=torch.float32, device="cuda")
    depth[:, :w] = dev(f["depth"])
    normals = torch.full((h, w + 5), -1, dtype=torch.int32, device="cuda")
    normals[:, :w] = dev(f["packed"].view(np.int32))
    out = torch.full((h, w + 11), 0xA5, dtype=torch.uint8, device="cuda")
    ao, work = ctx.cacao(depth[:, :w], normals[:, :w], R10, sh, pp, out=out[:, :w])
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[:, w:] == 0xA5).all(), "the padding of the AO plane was written"
    assert_frame(planes_to_host(work, w, h), host[:, :w], ref, 2, "pitched")
    assert torch.isnan(depth[:, w:]).all() and (normals[:, w:] == -1).all()


def test_non_default_stream(ctx):
    w, h = 64, 48
    s = torch.cuda.Stream()
    ao, got = run(ctx, "noise", w, h, stream=s)
    assert_frame(got, ao, reference("noise", w, h), 2, "side stream")


def test_two_calls_on_one_work_buffer_give_identical_bytes(ctx):
    w, h = 125, 93
    f = inputs("noise", w, h)
    sh, pp = consts("noise", w, h)
    d, n = dev(f["depth"]), normals_tensor(f, R10)
    ao1, work = ctx.cacao(d, n, R10, sh, pp)
    torch.cuda.synchronize()
    first, ao1 = work.cpu().numpy().copy(), ao1.cpu().numpy()
    ao2, _ = ctx.cacao(d, n, R10, sh, pp, work=work)
    torch.cuda.synchronize()
    planes1, planes2 = capi.cacao_work_planes(first, w, h), capi.cacao_work_planes(work.cpu().numpy(), w, h)
    for key in ("normals", "ping", "pong"):
        assert np.array_equal(planes1[key], planes2[key]), key
    for k in range(4):
        assert np.array_equal(planes1["depths"][k].view(np.uint16), planes2["depths"][k].view(np.uint16)), f"depths mip {k}"
    assert np.array_equal(ao1, ao2.cpu().numpy())


def test_refusals_launch_nothing(ctx):
    w, h = 37, 23
    f = inputs("room", w, h)
    sh, pp = consts("room", w, h)
    sh64, pp64 = consts("room", 64, 48)
    d, n = dev(f["depth"]), normals_tensor(f, R10)
    work = torch.zeros((capi.cacao_work_bytes(w, h),), dtype=torch.uint8, device="cuda")
    ao = torch.full((h, w), 0x5A, dtype=torch.uint8, device="cuda")
    lib, hnd, st = ctx.lib, ctx._h, ctx._stream()
    p = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(None)
    good = dict(depth=p(d), dpitch=w * 4, normals=p(n), fmt=R10, npitch=w * 4, shared=C.byref(sh), per_pass=pp, quality=abi.CACAO_QUALITY_HIGH, blur=2,
                work=p(work), wbytes=work.numel(), ao=p(ao), apitch=w, w=w, h=h)

    def call(**over):
        a = dict(good)
        a.update(over)
        return lib.vqhip_cacao(hnd, st, a["depth"], a["dpitch"], a["normals"], a["fmt"], a["npitch"], a["shared"], a["per_pass"], a["quality"], a["blur"],
                               a["work"], a["wbytes"], a["ao"], a["apitch"], a["w"], a["h"])
    INV, UNS = abi.VQHIP_ERR_INVALID_ARG, abi.VQHIP_ERR_UNSUPPORTED
    cases = [("NULL depth", dict(depth=null), INV), ("NULL normals", dict(normals=null), INV), ("NULL shared", dict(shared=None), INV), ("NULL perPass", dict(per_pass=None), INV),
             ("NULL work", dict(work=null), INV), ("NULL ao", dict(ao=null), INV), ("zero width", dict(w=0), INV), ("negative height", dict(h=-3), INV),
             ("depth pitch", dict(dpitch=w * 4 - 4), INV), ("normal pitch", dict(npitch=w * 4 - 4), INV), ("ao pitch", dict(apitch=w - 1), INV),
             ("workBytes", dict(wbytes=work.numel() - 1), INV), ("blurPassCount 9", dict(blur=9), INV), ("blurPassCount -1", dict(blur=-1), INV),
             ("constants of another frame", dict(shared=C.byref(sh64), per_pass=pp64), INV),
             ("quality HIGHEST", dict(quality=abi.CACAO_QUALITY_HIGHEST), UNS), ("quality MEDIUM", dict(quality=abi.CACAO_QUALITY_MEDIUM), UNS),
             ("quality LOWEST", dict(quality=abi.CACAO_QUALITY_LOWEST), UNS), ("RGBA16F normals", dict(fmt=abi.FMT_RGBA16F), UNS),
             ("frame above the limit", dict(w=abi.CACAO_MAX_DIM + 1), UNS)]
    for name, over, code in cases:
        assert call(**over) == code, name
        assert len(lib.vqhip_last_error(hnd) or b"") > 10, name
    torch.cuda.synchronize()
    assert (ao == 0x5A).all() and (work == 0).all(), "a refused call wrote to its outputs"
    assert call() == abi.VQHIP_OK
    torch.cuda.synchronize()
    assert_same("after the refusals", ao.cpu().numpy(), reference("room", w, h)["ao"])


def test_1280x720_room_every_plane(ctx):
    w, h = 1280, 720
    ref = reference("room", w, h)
    ao, got = run(ctx, "room", w, h)
    assert_frame(got, ao, ref, 2, "room 1280x720")


def test_3840x2160_stage_by_stage(ctx):
    """The prepare planes in full; generate on 64 seeded 8 x 8 tiles per slice; blur as cacao_ref.blur(GPU ping) and apply as cacao_ref.apply(GPU pong), in full.
    The frame is the 960 x 540 room enlarged four times (texel replication, which keeps the ray cast and the numpy side within seconds) with a seeded per-pixel
    perturbation — view depths by up to 0.2 %, every normal channel by up to two UNORM10 steps — so that the four texels of a gather footprint, and with them the
    four deinterleaved slices, all differ: a slice-order or parity mistake of the address arithmetic at this size cannot hide behind equal texels."""
    w, h, k = 3840, 2160, 4
    f = inputs("room", w // k, h // k)
    depth, packed = (np.repeat(np.repeat(f[key], k, 0), k, 1) for key in ("depth", "packed"))
    rng = np.random.default_rng(0x4CAC)
    add = np.float64(f["proj"][2, 2])
    depth = np.minimum(add - (add - depth.astype(np.float64)) * (1.0 + 0.004 * (rng.random((h, w)) - 0.5)), 1.0).astype(np.float32)
    q = np.stack([(packed >> np.uint32(s)) & np.uint32(1023) for s in (0, 10, 20)], -1).astype(np.int64)
    q = np.clip(q + rng.integers(-2, 3, q.shape), 0, 1023).astype(np.uint32)
    packed = (q[..., 0] | (q[..., 1] << np.uint32(10)) | (q[..., 2] << np.uint32(20)) | (np.uint32(3) << np.uint32(30))).astype(np.uint32)
    for a in (depth, packed):                                                  # the four texels of (nearly) every 2 x 2 footprint differ
        assert ((a[0::2, 0::2] != a[0::2, 1::2]) & (a[0::2, 0::2] != a[1::2, 0::2]) & (a[1::2, 1::2] != a[0::2, 1::2])).mean() > 0.5
    sh, pp = cacao.constants(w, h, f["proj"], f["normals_to_view"])
    ao, work = ctx.cacao(dev(depth), dev(packed.view(np.int32)), R10, sh, pp)
    torch.cuda.synchronize()
    got, ao = planes_to_host(work, w, h), ao.cpu().numpy()
    cs, cp = R.Consts(sh), [R.Consts(pp[i]) for i in range(4)]
    ref_depths, ref_normals = R.prepare_depths(depth, cs), R.prepare_normals(packed, R10, cs)
    for m in range(4):
        assert_same(f"4K depths mip {m}", got["depths"][m], ref_depths[m])
    assert_same("4K normals", got["normals"], ref_normals)
    hw, hh = abi.cacao_half_dims(w, h)
    rng = np.random.default_rng(0x4C0)
    pixels = []
    for _ in range(4):
        tx, ty = rng.integers(0, hw // 8, 64), rng.integers(0, hh // 8, 64)
        tx[0], ty[0], tx[1], ty[1] = 0, 0, hw // 8 - 1, hh // 8 - 1                                  # two frame corners always
        ys, xs = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
        pixels.append(((tx[:, None, None] * 8 + xs).ravel(), (ty[:, None, None] * 8 + ys).ravel()))
    ref_ping, _ = R.generate(ref_depths, ref_normals, cp, pixels)
    for s, (xs, ys) in enumerate(pixels):
        assert_same(f"4K ping, slice {s}, 64 tiles", got["ping"][s, ys, xs], ref_ping[s, ys, xs])
    assert_same("4K pong = blur(GPU ping)", got["pong"], R.blur(got["ping"], cp, 2))
    assert_same("4K ao = apply(GPU pong)", ao, R.apply(got["pong"], cs, w, h))


def test_ao_plane_feeds_forward_lighting(ctx):
    """The chain the pass exists for: the AO plane of vqhip_cacao as texScreenSpaceAO of the G-buffer producer, then vqhip_forward_lighting — equal to the oracle's
    forward lighting given cacao_ref.frame's plane."""
    from tests.test_gpu_gbuffer import build_materials
    w, h, nm = 160, 24, 3
    ref = reference("room", w, h)
    f = inputs("room", w, h)
    sh, pp = consts("room", w, h)
    ao, _ = ctx.cacao(dev(f["depth"]), normals_tensor(f, R10), R10, sh, pp)
    ip = synth.interpolants(w, h, nm)
    _, _, hmats, dmats, keep = build_materials(ctx, nm, max_dim=64)
    pf, _ = synth.per_frame(points=synth.point_lights(8), spots=synth.spot_lights(2), directional=synth.directional_light())
    pv = synth.per_view(w, h)
    gb_o = O.gbuffer_from_materials(ip, hmats, pf.fAmbientLightingFactor, ref["ao"])
    col_o = O.forward_lighting(gb_o, pf, pv, abi.FMT_RGBA16F)
    gb_g = ctx.gbuffer_from_materials([dev(p) for p in ip], dmats, pf.fAmbientLightingFactor, ao)
    col_g = ctx.forward_lighting(gb_g, pf, pv, out_fmt=abi.FMT_RGBA16F)
    torch.cuda.synchronize()
    assert_same("AO plane", ao.cpu().numpy(), ref["ao"])
    assert len(np.unique(ref["ao"])) > 4, "the AO plane of the test frame is flat: the chain would not see it"
    assert_same("scene colour lit with the CACAO plane", col_g.cpu().numpy(), col_o)
