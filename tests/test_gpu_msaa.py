"""-m gpu: vqhip_forward_lighting_msaa (docs/DESIGN_DETAILS.md §7.9) bit for bit against the contract: every layer shaded by the oracle
(tests/oracle_lib.forward_lighting), resolved by tests/msaa_ref.py; full coverage against vqhip_forward_lighting itself."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import msaa_ref
from tests import oracle_lib as O
from tests import ref_cases
from tests.test_arith_modes import dxc_mode
from vqengine_amd import abi, capi, synth

pytestmark = pytest.mark.gpu
dev = ref_cases._dev
F16, F32 = abi.FMT_RGBA16F, abi.FMT_RGBA32F


def assert_bits(got, ref, what):
    n, idx = O.bits_equal(got.cpu().numpy() if hasattr(got, "cpu") else got, ref)
    assert n == 0, f"{what}: {n} mismatching elements, first {idx.tolist()}"


def _lights(w, h, seed):
    pf, extra = synth.per_frame(points=synth.point_lights(12, seed=seed), spots=synth.spot_lights(2, seed=seed), directional=synth.directional_light())
    return pf, extra, synth.per_view(w, h)


def _expected(gbs, cov, pf, pv, fmt, extra=None, background=None, env=None, shadow=None):
    with np.errstate(all="ignore"):
        shaded = [O.forward_lighting(g, pf, pv, fmt, extra_point=extra, env=env, shadow=shadow) for g in gbs]
    return msaa_ref.resolve(shaded, cov, background, fmt)


def _bg(w, h, fmt, seed):
    img = synth.hdr_image(w, h, seed=seed)
    return img.astype(np.float16 if fmt == F16 else np.float32)


@pytest.mark.parametrize("w,h", [(1920, 1080), (333, 37), (64, 1)])
@pytest.mark.parametrize("kind", ["plain", "env", "casters"])
@pytest.mark.parametrize("dxc", [False, True])
def test_full_coverage_equals_forward_lighting(ctx, w, h, kind, dxc):
    if w == 1920 and (kind != "plain" or dxc):
        w, h = 480, 270                                            # the 1080p frame once; the variants at a smaller size
    keep = []
    gb = synth.gbuffer(w, h, seed=0x3A1)
    env = shadow = None
    if kind == "casters":
        pf, s = ref_cases.shadow_scene()
        extra = None
        shadow = ref_cases.dev_shadow(s, keep)
    else:
        pf, extra = synth.per_frame(points=synth.point_lights(24, seed=0x3A1), spots=synth.spot_lights(2), directional=synth.directional_light(), hdri_offset=0.3)
    e = ref_cases.small_env() if kind == "env" else None
    pv = synth.per_view(w, h, max_env_lod=e["spec_mips"] if e else 0)
    if e:
        env = ref_cases.dev_env(e, keep)
    planes = [dev(g) for g in gb]
    cov = torch.full((h, w), 0xF, dtype=torch.uint8, device="cuda")
    if dxc:
        with dxc_mode(ctx):
            want = ctx.forward_lighting(planes, pf, pv, out_fmt=F16, extra_point=extra, env=env, shadow=shadow)
            got = ctx.forward_lighting_msaa([planes], [cov], pf, pv, out_fmt=F16, extra_point=extra, env=env, shadow=shadow)
    else:
        want = ctx.forward_lighting(planes, pf, pv, out_fmt=F16, extra_point=extra, env=env, shadow=shadow)
        got = ctx.forward_lighting_msaa([planes], [cov], pf, pv, out_fmt=F16, extra_point=extra, env=env, shadow=shadow)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy().view(np.uint16), want.cpu().numpy().view(np.uint16)), (w, h, kind, dxc)


@pytest.mark.parametrize("layers", [2, 3, 4])
@pytest.mark.parametrize("fmt", [F16, F32])
@pytest.mark.parametrize("with_bg", [False, True])
def test_edges_frames_match_oracle_and_resolve(ctx, layers, fmt, with_bg):
    w, h = 160, 48
    gbs, cov = synth.gbuffer_msaa(w, h, layers, 0.2, seed=0x70 + layers)
    pf, extra, pv = _lights(w, h, 0x70 + layers)
    bg = _bg(w, h, fmt, 0x71) if with_bg else None
    want = _expected(gbs, cov, pf, pv, fmt, extra, bg)
    got = ctx.forward_lighting_msaa([[dev(p) for p in g] for g in gbs], [dev(c) for c in cov], pf, pv, background=dev(bg) if with_bg else None,
                                    out_fmt=fmt, extra_point=extra)
    assert_bits(got, want, f"edges frame, {layers} layers, fmt {fmt}, background {with_bg}")


def _padded(a, pitch, fill):
    out = np.full((a.shape[0], pitch) + a.shape[2:], fill, a.dtype)
    out[:, :a.shape[1]] = a
    return out


@pytest.mark.parametrize("fmt", [F16, F32])
def test_every_pitch_differs_from_the_width(ctx, fmt):
    w, h, layers = 101, 23, 3
    gbs, cov = synth.gbuffer_msaa(w, h, layers, 0.3, seed=0x91)
    pf, extra, pv = _lights(w, h, 0x91)
    bg = _bg(w, h, fmt, 0x92)
    want = _expected(gbs, cov, pf, pv, fmt, extra, bg)
    keep = []
    g = abi.GBufferMSAA()
    g.layers, g.coverage_pitch = layers, w + 13
    for k in range(layers):
        pl = [dev(_padded(p, w + 3 + 2 * k, np.float32(np.nan))) for p in gbs[k]]
        c = dev(_padded(cov[k], w + 13, np.uint8(0xFF)))
        keep += pl + [c]
        g.layer[k] = abi.GBuffer(pl[0].data_ptr(), pl[1].data_ptr(), pl[2].data_ptr(), pl[3].data_ptr(), w, h, w + 3 + 2 * k)
        g.coverage[k] = c.data_ptr()
    bgd = dev(_padded(bg, w + 5, bg.dtype.type(np.nan)))
    fill = 7.0
    dt = torch.float16 if fmt == F16 else torch.float32
    out = torch.full((h, w + 9, 4), fill, dtype=dt, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = ctx.lib.vqhip_forward_lighting_msaa(ctx._h, st, C.byref(g), C.byref(pf), C.byref(pv), C.cast(extra, C.c_void_p) if extra is not None and len(extra) else None,
                                             len(extra) if extra is not None else 0, None, None, C.c_void_p(bgd.data_ptr()), w + 5, C.c_void_p(out.data_ptr()), w + 9, fmt)
    assert rc == 0, ctx.lib.vqhip_last_error(ctx._h)
    o = out.cpu().numpy()
    assert_bits(o[:, :w], want, "pitched layers / coverage / background / out")
    assert np.all(o[:, w:] == fill), "padding of out written"


def test_random_contract_slice(ctx):
    """all 256 mask bytes, NaN records in layers that own nothing, emissive outliers whose RGBA32F sums overflow"""
    w, h, layers = 256, 6, 4
    gbs, cov = synth.gbuffer_msaa(w, h, layers, 0.0, seed=0xAB, mode="random")
    cov[0][0] = np.arange(256, dtype=np.uint8)                    # every byte value in layer 0
    cov[1][1] = np.arange(256, dtype=np.uint8)
    own = msaa_ref.owners(cov)
    for k in range(layers):
        owns = (own == k).any(-1)
        for p in gbs[k]:
            p[~owns] = np.nan                                     # a layer that owns nothing there may hold anything
    gbs[2][3][4, :, :3] = np.float32(1.0)                         # emissive outliers: 3e38 per channel, so the four-sample sums overflow in RGBA32F
    gbs[2][3][4, :, 3] = np.float32(3e38)                         # (and the samples are already Inf in RGBA16F)
    pf, extra, pv = _lights(w, h, 0xAB)
    for fmt in (F16, F32):
        for bg in (None, _bg(w, h, fmt, 0xAC)):
            want = _expected(gbs, cov, pf, pv, fmt, extra, bg)
            got = ctx.forward_lighting_msaa([[dev(p) for p in g] for g in gbs], [dev(c) for c in cov], pf, pv,
                                            background=dev(bg) if bg is not None else None, out_fmt=fmt, extra_point=extra)
            assert_bits(got, want, f"random slice fmt {fmt} background {bg is not None}")


@pytest.mark.parametrize("w,h,case", [(1, 1, "random"), (3, 2, "random"), (97, 31, "none_split"), (97, 31, "all_split")])
def test_tiny_frames_and_split_extremes(ctx, w, h, case):
    gbs, cov = synth.gbuffer_msaa(w, h, 3, 0.0, seed=0xC3 + w, mode="random" if case != "none_split" else "edges")
    if case == "none_split":
        cov[1][::2] = 0xF                                          # whole pixels of layer 1 on even rows: no pixel has two owners
        cov[0][::2] = 0
    if case == "all_split":
        cov = [np.full((h, w), m, np.uint8) for m in (0x1, 0x2, 0x4)]   # every pixel: three layers + background
    pf, extra, pv = _lights(w, h, 0xC3)
    for fmt in (F16, F32):
        want = _expected(gbs, cov, pf, pv, fmt, extra)
        got = ctx.forward_lighting_msaa([[dev(p) for p in g] for g in gbs], [dev(c) for c in cov], pf, pv, out_fmt=fmt, extra_point=extra)
        assert_bits(got, want, f"{case} {w}x{h} fmt {fmt}")


def test_deterministic_two_streams_and_forward_lighting_unchanged(ctx):
    w, h = 640, 96
    gbs, cov = synth.gbuffer_msaa(w, h, 3, 0.15, seed=0xD1)
    pf, extra, pv = _lights(w, h, 0xD1)
    L = [[dev(p) for p in g] for g in gbs]
    Cv = [dev(c) for c in cov]
    fl0 = ctx.forward_lighting(L[0], pf, pv, out_fmt=F16, extra_point=extra).cpu().numpy()
    a = ctx.forward_lighting_msaa(L, Cv, pf, pv, out_fmt=F16, extra_point=extra)
    b = ctx.forward_lighting_msaa(L, Cv, pf, pv, out_fmt=F16, extra_point=extra)
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy().view(np.uint16), b.cpu().numpy().view(np.uint16))
    want = _expected(gbs, cov, pf, pv, F16, extra)
    assert_bits(a, want, "msaa vs oracle")
    # back to back on two streams of one context: the edge list is handed over by an event
    gbs2, cov2 = synth.gbuffer_msaa(w, h, 2, 0.3, seed=0xD2)
    L2 = [[dev(p) for p in g] for g in gbs2]
    C2 = [dev(c) for c in cov2]
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    o1 = torch.empty((h, w, 4), dtype=torch.float16, device="cuda")
    o2 = torch.empty((h, w, 4), dtype=torch.float16, device="cuda")
    for _ in range(3):
        ctx.forward_lighting_msaa(L, Cv, pf, pv, out=o1, out_fmt=F16, extra_point=extra, stream=s1)
        ctx.forward_lighting_msaa(L2, C2, pf, pv, out=o2, out_fmt=F16, extra_point=extra, stream=s2)
    torch.cuda.synchronize()
    assert_bits(o1, want, "stream 1")
    assert_bits(o2, _expected(gbs2, cov2, pf, pv, F16, extra), "stream 2")
    fl1 = ctx.forward_lighting(L[0], pf, pv, out_fmt=F16, extra_point=extra).cpu().numpy()
    assert np.array_equal(fl0.view(np.uint16), fl1.view(np.uint16))


def test_argument_checks(ctx):
    w, h = 32, 8
    gbs, cov = synth.gbuffer_msaa(w, h, 2, 0.2, seed=0xE1)
    pf, extra, pv = _lights(w, h, 0xE1)
    keep = [[dev(p) for p in g] for g in gbs]
    cv = [dev(c) for c in cov]
    out = torch.zeros((h, w, 4), dtype=torch.float16, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def mk():
        g = abi.GBufferMSAA()
        g.layers, g.coverage_pitch = 2, 0
        for k in range(2):
            p = keep[k]
            g.layer[k] = abi.GBuffer(p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), p[3].data_ptr(), w, h, w)
            g.coverage[k] = cv[k].data_ptr()
        return g

    def call(g, fmt=F16, bg=None, bgp=0, op=w):
        return ctx.lib.vqhip_forward_lighting_msaa(ctx._h, st, C.byref(g), C.byref(pf), C.byref(pv), None, 0, None, None,
                                                   C.c_void_p(bg), bgp, C.c_void_p(out.data_ptr()), op, fmt)
    assert call(mk()) == 0
    INV, UNS = abi.VQHIP_ERR_INVALID_ARG, abi.VQHIP_ERR_UNSUPPORTED
    for layers in (0, 5, -1):
        g = mk(); g.layers = layers
        assert call(g) == INV
    g = mk(); g.layer[1].gb2 = None
    assert call(g) == INV
    g = mk(); g.coverage[1] = None
    assert call(g) == INV
    g = mk(); g.layer[1].width = w - 1
    assert call(g) == INV
    g = mk(); g.layer[0].row_pitch_px = w - 1
    assert call(g) == INV
    g = mk(); g.coverage_pitch = w - 1
    assert call(g) == INV
    assert call(mk(), op=w - 1) == INV
    assert call(mk(), bg=out.data_ptr() + 0, bgp=w) == INV                     # background aliasing out
    assert call(mk(), bg=keep[0][0].data_ptr(), bgp=w - 1) == INV
    for fmt in (abi.FMT_RGBA8_UNORM, abi.FMT_RG16F, 99):
        assert call(mk(), fmt=fmt) == UNS
    g = mk(); g.layers = 1; g.layer[1].gb0 = None; g.coverage[1] = None        # entries >= layers are ignored
    assert call(g) == 0
    torch.cuda.synchronize()
