"""vqhip_adaptive_cacao on the GPU (docs/DESIGN_DETAILS.md §7.15): FidelityFX CACAO at quality HIGHEST. Every plane the ten kernels write — the deinterleaved depths
and normals, the base pass's (obscurance, weight / 20) in the PONG slices, the importance map after A and after B, the load counter, the adaptive PING planes, the
blurred PONG planes and the AO plane — bit for bit against tests/cacao_adaptive_ref.py, through the C ABI. Sizes as in tests/test_gpu_cacao.py: 37 x 23 (a 10 x 6
importance map inside 16 x 8 threads of CSPostprocessImportanceMapB: the threads outside the map add to the counter), 64 x 48 (everything divides), 125 x 93 (odd
everywhere, 32 x 24 map in whole groups). Each GPU step runs once; references are computed once per case and shared."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import cacao_adaptive_ref as A
from tests import oracle_lib as O
from vqengine_amd import abi, cacao, capi, synth

pytestmark = pytest.mark.gpu

R10, F32 = abi.FMT_R10G10B10A2_UNORM, abi.FMT_RGBA32F
SMALL = ((37, 23), (64, 48), (125, 93))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def scaled_radius(w):
    """tests/test_gpu_cacao.py's: the radius that gives a small frame the sampling discs 1280 x 720 has at the default 1.2"""
    return 1.2 * 640.0 / ((w + 1) // 2)


def constant_frame(w=8, h=8):
    """Constant depth and a constant normal that faces the camera: every tap lies behind the texel's plane, so every obscurance is 0, the base planes are flat, the
    importance map is 0 and so is the counter"""
    f = synth.cacao_room(w, h)
    m = np.asarray(f["normals_to_view"], np.float64)[:3, :3]
    world = m.T @ np.array([0.0, 0.0, -1.0])                                   # view = m @ world (cacao_ref.prepare_normals), m a rotation
    n01 = np.ones((h, w, 4), np.float32)
    n01[..., :3] = ((world + 1.0) / 2.0).astype(np.float32)
    return {"depth": np.full((h, w), 0.5, np.float32), "n01": n01, "proj": f["proj"], "normals_to_view": f["normals_to_view"]}


@functools.lru_cache(maxsize=None)
def inputs(kind, w, h):
    if kind == "constant":
        return constant_frame(w, h)
    return synth.cacao_room(w, h) if kind == "room" else synth.cacao_noise(w, h)


@functools.lru_cache(maxsize=None)
def consts(kind, w, h, variant="default", limit=0.45):
    f = inputs(kind, w, h)
    over = {"adaptiveQualityLimit": limit}                                      # qualityLevel stays the default: HIGHEST
    if kind == "noise":
        over["radius"] = scaled_radius(w)
    if variant == "other":
        over.update(radius=0.5 * (scaled_radius(w) / 1.2 if kind == "noise" else 1.0), shadowPower=1.0, sharpness=0.5, detailShadowStrength=0.0)
    s = cacao.settings(**over)
    assert s["qualityLevel"] == abi.CACAO_QUALITY_HIGHEST
    return cacao.constants(w, h, f["proj"], f["normals_to_view"], s)


@functools.lru_cache(maxsize=None)
def reference(kind, w, h, blur=0, fmt=R10, variant="default", limit=0.45):
    f = inputs(kind, w, h)
    sh, pp = consts(kind, w, h, variant, limit)
    return A.frame(f["depth"], f["packed"] if fmt == R10 else f["n01"], fmt, sh, pp, blur)


def normals_tensor(f, fmt):
    return dev(f["packed"].view(np.int32)) if fmt == R10 else dev(f["n01"])


def planes_to_host(work, w, h):
    v = capi.adaptive_cacao_work_planes(work.cpu().numpy(), w, h)
    return {k: ([np.array(d) for d in p] if k == "depths" else np.array(p)) for k, p in v.items()}


def assert_same(name, got, ref):
    n_bad, idx = O.bits_equal(np.asarray(got), np.asarray(ref))
    assert n_bad == 0, f"{name}: {n_bad} of {np.asarray(ref).size} elements differ from tests/cacao_adaptive_ref.py, first at {idx.tolist()}"


def assert_frame(got, ao, ref, blur, label):
    for k in range(4):
        assert_same(f"{label}: depths mip {k}", got["depths"][k], ref["depths"][k])
    assert_same(f"{label}: normals", got["normals"], ref["normals"])
    if blur:
        assert_same(f"{label}: pong (blurred)", got["pong"], ref["pong"])
    else:
        assert_same(f"{label}: pong (the base pass)", got["pong"], ref["base"])
    assert_same(f"{label}: importance pong (after A)", got["importance_pong"], ref["importance_pong"])
    assert_same(f"{label}: importance (after B)", got["importance"], ref["importance"])
    assert int(got["counter"][0]) == ref["counter"], f"{label}: load counter {int(got['counter'][0])}, tests/cacao_adaptive_ref.py has {ref['counter']}"
    assert_same(f"{label}: ping", got["ping"], ref["ping"])
    assert_same(f"{label}: ao", ao, ref["ao"])


def run(ctx, kind, w, h, blur=0, fmt=R10, variant="default", limit=0.45, stream=None):
    f = inputs(kind, w, h)
    sh, pp = consts(kind, w, h, variant, limit)
    ao, work = ctx.adaptive_cacao(dev(f["depth"]), normals_tensor(f, fmt), fmt, sh, pp, blur_passes=blur, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return ao.cpu().numpy(), planes_to_host(work, w, h)


@pytest.mark.parametrize("blur", (0, 2))
@pytest.mark.parametrize("size", SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ("room", "noise"))
def test_small_frames_every_plane(ctx, kind, size, blur):
    w, h = size
    ref = reference(kind, w, h, blur)
    ao, got = run(ctx, kind, w, h, blur)
    assert_frame(got, ao, ref, blur, f"{kind} {w}x{h} blur {blur}")


@pytest.mark.parametrize("limit", (0.0, 0.45, 1.0))
@pytest.mark.parametrize("kind", ("room", "noise"))
def test_adaptive_quality_limits(ctx, kind, limit):
    """0: the limiter is 0 and every texel stops at 6 taps; 1.0 on the noise frame: most texels run all 32"""
    w, h = 125, 93
    ref = reference(kind, w, h, 2, limit=limit)
    hist = ref["stats"]["tap_histogram"]
    if limit == 0.0:
        assert hist[6] == hist.sum()
    if limit == 1.0 and kind == "noise":
        assert hist[32] >= 32
    ao, got = run(ctx, kind, w, h, 2, limit=limit)
    assert_frame(got, ao, ref, 2, f"{kind} adaptiveQualityLimit {limit}")


def test_rgba32f_normals(ctx):
    w, h = 125, 93
    ref = reference("noise", w, h, 2, fmt=F32)
    ao, got = run(ctx, "noise", w, h, 2, fmt=F32)
    assert_frame(got, ao, ref, 2, "RGBA32F normals")


@pytest.mark.parametrize("limit", (0.45, 0.0))
def test_constant_frame(ctx, limit):
    """importance 0 and counter 0: limit / 0 = +inf saturates to 1, and with adaptiveQualityLimit 0 the quotient 0 / 0 = NaN saturates to 0; 6 taps either way"""
    w, h = 8, 8
    ref = reference("constant", w, h, 0, fmt=F32, limit=limit)
    assert ref["counter"] == 0 and not ref["importance"].any() and ref["stats"]["limiter"] == (1.0 if limit else 0.0) and ref["stats"]["tap_histogram"][6] == 64
    ao, got = run(ctx, "constant", w, h, 0, fmt=F32, limit=limit)
    assert_frame(got, ao, ref, 0, f"constant frame, limit {limit}")


def test_non_default_settings(ctx):
    """radius 0.5, shadowPower 1, sharpness 0.5, detailShadowStrength 0"""
    w, h = 125, 93
    for kind in ("room", "noise"):
        ref = reference(kind, w, h, 2, variant="other")
        ao, got = run(ctx, kind, w, h, 2, variant="other")
        assert_frame(got, ao, ref, 2, f"other settings, {kind}")


def test_prefilled_work_buffer_and_second_call(ctx):
    """A work buffer full of 0xFF, then the same buffer again: both leave the bytes of a fresh run in every plane, the counter included — the counter is cleared by
    the call itself and nothing reads memory the call has not written"""
    w, h = 125, 93
    f = inputs("room", w, h)
    sh, pp = consts("room", w, h)
    ref = reference("room", w, h, 2)
    d, n = dev(f["depth"]), normals_tensor(f, R10)
    work = torch.full((capi.adaptive_cacao_work_bytes(w, h),), 0xFF, dtype=torch.uint8, device="cuda")
    for label in ("0xFF-filled work buffer", "second call on the same buffer"):
        ao, _ = ctx.adaptive_cacao(d, n, R10, sh, pp, blur_passes=2, work=work)
        torch.cuda.synchronize()
        assert_frame(planes_to_host(work, w, h), ao.cpu().numpy(), ref, 2, label)


def test_pitched_buffers_keep_their_padding(ctx):
    w, h = 125, 93
    f = inputs("room", w, h)
    sh, pp = consts("room", w, h)
    ref = reference("room", w, h, 2)
    depth = torch.full((h, w + 7), float("nan"), dtype=torch.float32, device="cuda")
    depth[:, :w] = dev(f["depth"])
    normals = torch.full((h, w + 5), -1, dtype=torch.int32, device="cuda")
    normals[:, :w] = dev(f["packed"].view(np.int32))
    out = torch.full((h, w + 11), 0xA5, dtype=torch.uint8, device="cuda")
    ao, work = ctx.adaptive_cacao(depth[:, :w], normals[:, :w], R10, sh, pp, blur_passes=2, out=out[:, :w])
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[:, w:] == 0xA5).all(), "the padding of the AO plane was written"
    assert_frame(planes_to_host(work, w, h), host[:, :w], ref, 2, "pitched")
    assert torch.isnan(depth[:, w:]).all() and (normals[:, w:] == -1).all()


def test_non_default_stream(ctx):
    w, h = 64, 48
    s = torch.cuda.Stream()
    ao, got = run(ctx, "noise", w, h, 2, stream=s)
    assert_frame(got, ao, reference("noise", w, h, 2), 2, "side stream")


def test_refusals_launch_nothing(ctx):
    w, h = 37, 23
    f = inputs("room", w, h)
    sh, pp = consts("room", w, h)
    sh64, pp64 = consts("room", 64, 48)
    bad_map = cacao.constants(w, h, f["proj"], f["normals_to_view"], cacao.settings())
    bad_map[0].ImportanceMapDimensions[0] += 1.0
    d, n = dev(f["depth"]), normals_tensor(f, R10)
    work = torch.full((capi.adaptive_cacao_work_bytes(w, h),), 0x3C, dtype=torch.uint8, device="cuda")
    ao = torch.full((h, w), 0x5A, dtype=torch.uint8, device="cuda")
    lib, hnd, st = ctx.lib, ctx._h, ctx._stream()
    p = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(None)
    good = dict(depth=p(d), dpitch=w * 4, normals=p(n), fmt=R10, npitch=w * 4, shared=C.byref(sh), per_pass=pp, blur=2,
                work=p(work), wbytes=work.numel(), ao=p(ao), apitch=w, w=w, h=h)

    def call(**over):
        a = dict(good)
        a.update(over)
        return lib.vqhip_adaptive_cacao(hnd, st, a["depth"], a["dpitch"], a["normals"], a["fmt"], a["npitch"], a["shared"], a["per_pass"], a["blur"],
                                        a["work"], a["wbytes"], a["ao"], a["apitch"], a["w"], a["h"])
    INV, UNS = abi.VQHIP_ERR_INVALID_ARG, abi.VQHIP_ERR_UNSUPPORTED
    cases = [("NULL depth", dict(depth=null), INV), ("NULL normals", dict(normals=null), INV), ("NULL shared", dict(shared=None), INV), ("NULL perPass", dict(per_pass=None), INV),
             ("NULL work", dict(work=null), INV), ("NULL ao", dict(ao=null), INV), ("zero width", dict(w=0), INV), ("negative height", dict(h=-3), INV),
             ("depth pitch", dict(dpitch=w * 4 - 4), INV), ("normal pitch", dict(npitch=w * 4 - 4), INV), ("ao pitch", dict(apitch=w - 1), INV),
             ("workBytes", dict(wbytes=work.numel() - 1), INV), ("HIGH's workBytes", dict(wbytes=capi.cacao_work_bytes(w, h)), INV),
             ("blurPassCount 9", dict(blur=9), INV), ("blurPassCount -1", dict(blur=-1), INV),
             ("constants of another frame", dict(shared=C.byref(sh64), per_pass=pp64), INV),
             ("importance map of another size", dict(shared=C.byref(bad_map[0])), INV),
             ("work overlaps ao", dict(ao=p(work), apitch=w), INV),
             ("RGBA16F normals", dict(fmt=abi.FMT_RGBA16F), UNS), ("frame above the limit", dict(w=abi.CACAO_MAX_DIM + 1), UNS)]
    for name, over, code in cases:
        assert call(**over) == code, name
        assert len(lib.vqhip_last_error(hnd) or b"") > 10, name
    # vqhip_cacao keeps refusing HIGHEST, and names the entry point that runs it
    rc = lib.vqhip_cacao(hnd, st, p(d), w * 4, p(n), R10, w * 4, C.byref(sh), pp, abi.CACAO_QUALITY_HIGHEST, 2, p(work), work.numel(), p(ao), w, w, h)
    assert rc == UNS and b"vqhip_adaptive_cacao" in lib.vqhip_last_error(hnd)
    torch.cuda.synchronize()
    assert (ao == 0x5A).all() and (work == 0x3C).all(), "a refused call wrote to its outputs"
    assert call() == abi.VQHIP_OK
    torch.cuda.synchronize()
    assert_same("after the refusals", ao.cpu().numpy(), reference("room", w, h, 2)["ao"])


def test_ao_plane_feeds_forward_lighting(ctx):
    """The chain the pass exists for: the HIGHEST AO plane as texScreenSpaceAO of the G-buffer producer, then vqhip_forward_lighting — equal to the oracle's forward
    lighting given cacao_adaptive_ref.frame's plane."""
    from tests.test_gpu_gbuffer import build_materials
    w, h, nm = 64, 48, 3
    ref = reference("room", w, h, 2)
    f = inputs("room", w, h)
    sh, pp = consts("room", w, h)
    ao, _ = ctx.adaptive_cacao(dev(f["depth"]), normals_tensor(f, R10), R10, sh, pp, blur_passes=2)
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
