"""What the shared host front ends of the lit draw (capi.hip: stageConstants, gbufferPlanes, gbufArgs, planeFitsOffsets, validateQuadPlane over a list of outputs, the
bodies forwardLighting and forwardFromMaterials; capi.py: _interpolants, _gbuffer, _ssao, _extra_point, _out_image, _byref) could break: what a refusal says, and which of
two refusals a call that is wrong twice gets. Every text is compared with tests/golden/lit_refusals.json, which scripts/record_ssr_cacao_refusals.py --module tests.test_gpu_lit_front_ends wrote from the library and the
bindings as they were while each entry point had its own copy of that code. Three parts, as in tests/test_gpu_ssr_cacao_front_ends.py:
  * the five refusal tests of the lit-draw modules, run as they stand while the context's library listens: every refusal they provoke, whole and in order;
  * for each of the ten entry points, calls with two faults on different rungs of its ladder (on the same rung where it is the ladder's last): the code and the text, and
    every plane a call could write, ip2 among them, keeps its bits;
  * every distinct ValueError of the bindings forward_lighting, forward_lighting_mrt, forward_lighting_msaa, gbuffer_from_materials, scene_normals_from_materials,
    forward_lighting_from_materials and their _quad forms.
The frames here are 40 x 24 beyond what the five refusal tests use themselves; a plane of 4 GiB exists in a struct's pitch or height alone, since the call is refused
before anything is read. All tensors come from a memory pool of their own (refusal_listener.fresh_allocations)."""
import contextlib
import ctypes as C
import json
import os

import pytest
import torch

from tests import test_gpu_msaa as TM
from tests import test_gpu_parity as TP
from tests import test_gpu_psmain_targets as TT
from tests import test_gpu_psmain_variants as TV
from tests import test_gpu_quad_interp as TQ
from tests.refusal_listener import Listening, fresh_allocations
from vqengine_amd import abi

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lit_refusals.json")
W, H = 40, 24
F16, F32, U8, N10, M16 = abi.FMT_RGBA16F, abi.FMT_RGBA32F, abi.FMT_RGBA8_UNORM, abi.FMT_R10G10B10A2_UNORM, abi.FMT_RG16F
SENTINEL = -7.0
INV, UNS = abi.VQHIP_ERR_INVALID_ARG, abi.VQHIP_ERR_UNSUPPORTED
PLANE = H * W * 16                                              # bytes of a float4 plane


def make_small():
    return {}                                                   # nothing is shared between the parts; the recording script passes it through


@pytest.fixture(scope="module")
def small():
    return make_small()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def said(entry, rc, text):
    return f"{entry} -> {rc}: {text}"


# ---- 1. the refusal tests as they stand --------------------------------------------------------------------------------------------------------------------------------
def _quad_refusals(c):
    try:
        TQ.test_producer_refusals(c)
    finally:
        TQ._KEEP.clear()                                        # what the module's autouse fixture does behind each of its tests


LISTENED = {"psmain_targets": TT.test_argument_checks, "msaa": TM.test_argument_checks, "quad_interp": _quad_refusals, "parity": TP.test_abi_errors,
            "psmain_variants": TV.test_psmain_waves_refuses_other_values}


@contextlib.contextmanager
def _listening(ctx, refused):
    """the context itself with a library that listens: the bindings' own calls (ctx.forward_lighting in test_abi_errors) are heard too"""
    lib = ctx.lib
    ctx.lib = Listening(lib, [], refused, ctx._h)
    try:
        yield ctx
    finally:
        ctx.lib = lib


def listen(ctx, small, which):
    """-> every refusal of that test, in order, as text"""
    refused = []
    with fresh_allocations(), _listening(ctx, refused) as c:
        LISTENED[which](c)
    return [said(*r) for r in refused]


@pytest.mark.parametrize("which", sorted(LISTENED))
def test_refusal_tests_hear_what_they_heard(ctx, small, golden, which):
    got, want = listen(ctx, small, which), golden["library"][which]
    assert len(got) == len(want) and len(got) >= 2, f"{which}: the refusal test provoked {len(got)} refusals, {len(want)} are recorded"
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{which}: refusal {k} of the test's cases"


# ---- 2. calls that are wrong twice --------------------------------------------------------------------------------------------------------------------------------------
def _planes():
    """One float32 tensor [10, H, W, 4] that holds every plane a call could write, so that one comparison shows that nothing was written and the quad-uv plane can lie
    on two of them at once: 0..3 the G-buffer planes (or the scene normals from 0 on), 4 the scene colour, 5 ip2, 7 the albedo target and behind it the motion vectors;
    6, 8 and 9 are spare, for a quad-uv plane that reaches one target alone. Inputs are tensors of their own"""
    pool = torch.full((10, H, W, 4), SENTINEL, dtype=torch.float32, device="cuda")
    pool[5] = 0.25
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")                       # noqa: E731
    return dict(pool=pool, before=pool.clone(), gb=z(4, H, W, 4), ip=z(2, H, W, 4), quv=z(H, W, 4), sv=z(2, H, W, 4), cov=z(2, H, W, dtype=torch.uint8),
                ssao=z(H, W, dtype=torch.uint8), bg=z(H, W, 4, dtype=torch.float16), blob=z(4096, dtype=torch.uint8), tex=z(16, 16, 4, dtype=torch.uint8))


def _with(struct, fields):
    for k, v in fields.items():
        setattr(struct, k, v)
    return struct


def _lit_calls(ctx, t):
    """-> {entry point: (call(**overrides), [(case, overrides)])}; every case names two faults, the one that the call reports first"""
    lib, hnd, st = ctx.lib, ctx._h, ctx._stream()
    at = lambda k, off=0: t["pool"][k].data_ptr() + off                                                           # noqa: E731
    blob, colour, ip2, albedo, motion, quv = t["blob"].data_ptr(), at(4), at(5), at(7), at(7, H * W * 8), t["quv"].data_ptr()
    pf0, extra, pv = TQ.lights(W, H)
    mats = (abi.MaterialDesc * 2)()

    def pf(directional=None, **counts):
        p = abi.PerFrameData.from_buffer_copy(pf0)
        _with(p.Lights, counts)
        if directional:
            p.Lights.directional.enabled = p.Lights.directional.shadowing = 1
        return p

    def bad_mats(slot, **fields):
        m = (abi.MaterialDesc * 2)()
        setattr(m[1], slot, _with(abi.Texture2D(t["tex"].data_ptr(), 16, 16, 5, 0), fields))
        return m
    env = abi.EnvMap(blob, 8, blob, 16, 5, blob, 32)
    no_diffuse, no_specular = abi.EnvMap(None, 0, blob, 16, 5, blob, 32), abi.EnvMap(blob, 8, None, 0, 0, blob, 32)
    sm = lambda **f: _with(abi.ShadowMaps(blob, 64, blob, 32, blob, 16), f)                                    # noqa: E731
    gbuf = lambda planes, **f: _with(abi.GBuffer(*planes, W, H, W), f)                                         # noqa: E731
    gb_in = lambda **f: gbuf([t["gb"][k].data_ptr() for k in range(4)], **f)                                   # noqa: E731
    gb_out = lambda **f: gbuf([at(k) for k in range(4)], **f)                                                  # noqa: E731
    inter = lambda **f: _with(abi.Interpolants(t["ip"][0].data_ptr(), t["ip"][1].data_ptr(), ip2, W, H, W), f)  # noqa: E731
    ssao = lambda **f: _with(abi.SSAO(t["ssao"].data_ptr(), W, H), f)                                          # noqa: E731
    targets = lambda **f: _with(abi.PsmainTargets(albedo, F16, 0, motion, M16, 0, t["sv"][0].data_ptr(), t["sv"][1].data_ptr(), 0, 0), f)   # noqa: E731
    ref = lambda s: C.byref(s) if s is not None else None                                                      # noqa: E731
    vp = C.c_void_p

    def lighting(pf=pf0, pv=pv, extra=None, n_extra=0, env=None, sm=None):
        return ref(pf), ref(pv), C.cast(extra, vp) if extra is not None else None, n_extra, ref(env), ref(sm)

    def forward(gb=gb_in(), out=colour, pitch=W, fmt=F16, **light):
        return lib.vqhip_forward_lighting(hnd, st, ref(gb), *lighting(**light), vp(out), pitch, fmt)

    def forward_mrt(gb=gb_in(), out=colour, pitch=W, fmt=F16, mrt=targets(), **light):
        return lib.vqhip_forward_lighting_mrt(hnd, st, ref(gb), *lighting(**light), vp(out), pitch, fmt, ref(mrt))

    def msaa_gb(layers=2, cov_pitch=0, layer0=None, layer1=None, cov1=True):
        g = abi.GBufferMSAA()
        g.layers, g.coverage_pitch = layers, cov_pitch
        for k, over in enumerate((layer0 or {}, layer1 or {})):
            g.layer[k] = gb_in(**over)
            g.coverage[k] = t["cov"][k].data_ptr() if k == 0 or cov1 else None
        return g

    def msaa(gb=msaa_gb(), bg=None, bg_pitch=0, out=colour, pitch=W, fmt=F16, **light):
        return lib.vqhip_forward_lighting_msaa(hnd, st, ref(gb), *lighting(**light), vp(bg), bg_pitch, vp(out), pitch, fmt)

    def gbuffer(ip=inter(), m=mats, n=2, s=None, out=gb_out()):
        return lib.vqhip_gbuffer_from_materials(hnd, st, ref(ip), m, n, 0.1, ref(s), ref(out))

    def gbuffer_quad(ip=inter(), m=mats, n=2, s=None, out=gb_out(), q=quv, qpitch=0):
        return lib.vqhip_gbuffer_from_materials_quad(hnd, st, ref(ip), m, n, 0.1, ref(s), ref(out), vp(q), qpitch)

    def normals(ip=inter(), m=mats, n=2, out=at(0), fmt=N10, pitch=0):
        return lib.vqhip_scene_normals_from_materials(hnd, st, ref(ip), m, n, vp(out), fmt, pitch)

    def normals_quad(ip=inter(), m=mats, n=2, out=at(0), fmt=N10, pitch=0, q=quv, qpitch=0):
        return lib.vqhip_scene_normals_from_materials_quad(hnd, st, ref(ip), m, n, vp(out), fmt, pitch, vp(q), qpitch)

    def psmain(ip=inter(), m=mats, n=2, s=None, out=colour, pitch=W, fmt=F16, **light):
        return lib.vqhip_forward_lighting_from_materials(hnd, st, ref(ip), m, n, ref(s), *lighting(**light), vp(out), pitch, fmt)

    def psmain_mrt(ip=inter(), m=mats, n=2, s=None, out=colour, pitch=W, fmt=F16, mrt=targets(), **light):
        return lib.vqhip_forward_lighting_from_materials_mrt(hnd, st, ref(ip), m, n, ref(s), *lighting(**light), vp(out), pitch, fmt, ref(mrt))

    def psmain_quad(ip=inter(), m=mats, n=2, s=None, out=colour, pitch=W, fmt=F16, mrt=targets(), q=quv, qpitch=0, **light):
        return lib.vqhip_forward_lighting_from_materials_quad(hnd, st, ref(ip), m, n, ref(s), *lighting(**light), vp(out), pitch, fmt, ref(mrt), vp(q), qpitch)

    too_many = lib.vqhip_max_materials() + 1
    tall = 7000000                                               # 40 px x 7 000 000 rows x 16 B > 4 GiB, and below 2^24 rows
    wide = 12000000                                              # 12 000 000 px x 24 rows x 16 B > 4 GiB, and below 2^24 px
    lighting_ladder = [                                          # validateLighting, the same for every entry point that lights
        ("RGBA8 outFmt, 101 point lights", dict(fmt=U8, pf=pf(numPointLights=101))),
        ("one spot light too many, extraPoint count without the array", dict(pf=pf(numSpotLights=abi.NUM_LIGHTS__SPOT + 1), n_extra=3)),
        ("one point caster too many, a spot caster without sm", dict(pf=pf(numPointCasters=abi.NUM_SHADOWING_LIGHTS__POINT + 1, numSpotCasters=1))),
        ("negative numExtraPoint, a point caster without sm", dict(n_extra=-1, pf=pf(numPointCasters=1))),
        ("numExtraPoint above the maximum, env without diffuse", dict(extra=extra, n_extra=1 << 20, env=no_diffuse)),
        ("a spot caster without sm, env without diffuse", dict(pf=pf(numSpotCasters=1), env=no_diffuse)),
        ("a point caster without its map, an oversize spot map", dict(pf=pf(numPointCasters=1, numSpotCasters=1), sm=sm(point=None, spot_dim=40000))),
        ("a directional caster whose map has no size, env without specular", dict(pf=pf(directional=True), sm=sm(dir_dim=0), env=no_specular)),
        ("an oversize point cube, env without diffuse", dict(pf=pf(numPointCasters=1), sm=sm(point_dim=16385), env=no_diffuse)),
        ("an oversize directional map, env without specular", dict(pf=pf(directional=True), sm=sm(dir_dim=32769), env=no_specular)),
        ("env without diffuse and without specular", dict(env=abi.EnvMap(None, 0, None, 0, 0, None, 0))),
        ("env without specular and without its BRDF LUT", dict(env=abi.EnvMap(blob, 8, None, 0, 0, None, 0)))]
    mrt_ladder = [                                               # fillMrt
        ("env without specular, RGBA8 albedo_fmt", dict(env=no_specular, mrt=targets(albedo_fmt=U8))),
        ("env whose mip count exceeds the cube, short albedo pitch", dict(env=abi.EnvMap(blob, 8, blob, 16, 6, blob, 32), mrt=targets(albedo_pitch_px=W - 1))),
        ("RGBA8 albedo_fmt, short albedo pitch", dict(mrt=targets(albedo_fmt=U8, albedo_pitch_px=W - 1))),
        ("short albedo pitch, RGBA16F motion_fmt", dict(mrt=targets(albedo_pitch_px=W - 1, motion_fmt=F16))),
        ("RGBA16F motion_fmt, motion vectors without svPositionCurr", dict(mrt=targets(motion_fmt=F16, svPositionCurr=None))),
        ("motion vectors without svPositionPrev, short motion pitch", dict(mrt=targets(svPositionPrev=None, motion_pitch_px=W - 1))),
        ("short motion pitch, short sv pitch", dict(mrt=targets(motion_pitch_px=W - 1, sv_pitch_px=W - 1))),
        ("short sv pitch alone, the albedo target not bound", dict(mrt=targets(albedo_metallic=None, sv_pitch_px=W - 1)))]
    producer_ladder = [                                          # validateProducer
        ("NULL ip1, zero width", dict(ip=inter(ip1=None, width=0))),
        ("zero width, 7 000 000 rows", dict(ip=inter(width=0, height=tall))),
        ("short ip pitch, numMaterials -1", dict(ip=inter(row_pitch_px=W - 1), n=-1)),
        ("7 000 000 rows, numMaterials -1", dict(ip=inter(height=tall), n=-1)),
        ("ip pitch 2^24 at 8 rows, numMaterials -1", dict(ip=inter(row_pitch_px=1 << 24, height=8), n=-1)),
        ("width 1 at 2^24 rows, materials NULL", dict(ip=inter(width=1, row_pitch_px=1, height=1 << 24), m=None)),
        ("numMaterials above vqhip_max_materials, a texture of zero width", dict(n=too_many, m=bad_mats("texDiffuse", width=0))),
        ("materials NULL, short out pitch", dict(m=None, pitch=W - 1)),
        ("a normal map with zero mips, short out pitch", dict(m=bad_mats("texNormals", mips=0), pitch=W - 1)),
        ("a local-AO map with more mips than its size has, short out pitch", dict(m=bad_mats("texLocalAO", mips=6), pitch=W - 1))]
    ssao_ladder = [("a texture of negative height, ssao of zero width", dict(m=bad_mats("texEmissive", height=-1), s=ssao(width=0))),
                   ("ssao of zero height, short out pitch", dict(s=ssao(height=0), pitch=W - 1))]
    def quad_ladder(on, **low):
        """validateQuadPlane up to the overlaps, which differ from producer to producer. on: the producer's output; low: what else has to be 8 rows high"""
        return [("NULL quadUV, negative quad pitch", dict(q=None, qpitch=-1)),
                ("misaligned quadUV, negative quad pitch", dict(q=quv + 8, qpitch=-1)),
                ("negative quad pitch, quadUV on the output", dict(qpitch=-1, q=on)),
                ("short quad pitch, quadUV on the output", dict(qpitch=W - 1, q=on)),
                ("quad pitch of 12 000 000, quadUV on the output", dict(qpitch=wide, q=on)),
                ("quad pitch 2^24 at 8 rows, quadUV on ip2", dict(ip=inter(height=8), qpitch=1 << 24, q=ip2, **low))]

    def for_gbuffer(cases):
        """vqhip_gbuffer_from_materials has no pitch argument: its `out` carries the frame a second time"""
        return [(c.replace("short out pitch", "out narrower than the planes"), dict({k: v for k, v in o.items() if k != "pitch"}, **({"out": gb_out(width=W - 1)} if "pitch" in o else {})))
                for c, o in cases]
    return {
        "vqhip_forward_lighting": (forward, [
            ("NULL out, NULL gb2", dict(out=None, gb=gb_in(gb2=None))), ("NULL perView, zero width", dict(pv=None, gb=gb_in(width=0))),
            ("NULL gb2, zero width", dict(gb=gb_in(gb2=None, width=0))), ("zero height, RGBA8 outFmt", dict(gb=gb_in(height=0), fmt=U8)),
            ("short gb pitch, RGBA8 outFmt", dict(gb=gb_in(row_pitch_px=W - 1), fmt=U8)), ("short out pitch, 101 point lights", dict(pitch=W - 1, pf=pf(numPointLights=101)))]
            + lighting_ladder),
        "vqhip_forward_lighting_mrt": (forward_mrt, [
            ("NULL perFrame, RGBA8 albedo_fmt", dict(pf=None, mrt=targets(albedo_fmt=U8))), ("NULL gb0, RGBA8 albedo_fmt", dict(gb=gb_in(gb0=None), mrt=targets(albedo_fmt=U8))),
            ("short out pitch, short albedo pitch", dict(pitch=W - 1, mrt=targets(albedo_pitch_px=W - 1)))] + lighting_ladder[:3] + mrt_ladder),
        "vqhip_forward_lighting_msaa": (msaa, [
            ("NULL out, 5 layers", dict(out=None, gb=msaa_gb(layers=5))), ("0 layers, zero width", dict(gb=msaa_gb(layers=0, layer0=dict(width=0)))),
            ("zero width, short out pitch", dict(gb=msaa_gb(layer0=dict(width=0)), pitch=-1)),
            ("65536 x 65536 pixels, short out pitch", dict(gb=msaa_gb(layer0=dict(width=65536, height=65536)), pitch=W - 1)),
            ("short coverage pitch, background on out", dict(gb=msaa_gb(cov_pitch=W - 1), bg=colour, bg_pitch=W)),
            ("short background pitch, background on out", dict(bg=colour, bg_pitch=W - 1)),
            ("background on out, NULL gb1 of layer 1", dict(bg=colour, bg_pitch=W, gb=msaa_gb(layer1=dict(gb1=None)))),
            ("NULL coverage of layer 1, layer 1 of another size", dict(gb=msaa_gb(cov1=False, layer1=dict(height=H - 1)))),
            ("NULL gb3 of layer 0, short pitch of layer 0", dict(gb=msaa_gb(layer0=dict(gb3=None, row_pitch_px=W - 1)))),
            ("layer 1 of another size, short pitch of layer 1", dict(gb=msaa_gb(layer1=dict(width=W + 1, row_pitch_px=W - 1)))),
            ("short pitch of layer 1, NULL perFrame", dict(gb=msaa_gb(layer1=dict(row_pitch_px=W - 1)), pf=None)),
            ("NULL perView, RGBA8 outFmt", dict(pv=None, fmt=U8))] + lighting_ladder),
        "vqhip_gbuffer_from_materials": (gbuffer, [
            ("NULL out, NULL ip0", dict(out=None, ip=inter(ip0=None))), ("NULL gb3, zero width", dict(out=gb_out(gb3=None), ip=inter(width=0))), ("NULL ip, numMaterials -1", dict(ip=None, n=-1))]
            + for_gbuffer(producer_ladder + ssao_ladder) + [
            ("out of another height, out pitch of 12 000 000", dict(out=gb_out(height=H + 1, row_pitch_px=wide))),
            ("out pitch of 12 000 000 and above 2^24", dict(out=gb_out(row_pitch_px=1 << 25))), ("out pitch of 12 000 000", dict(out=gb_out(row_pitch_px=wide))),
            ("out pitch 2^24 at 8 rows", dict(ip=inter(height=8), out=gb_out(height=8, row_pitch_px=1 << 24)))]),
        "vqhip_gbuffer_from_materials_quad": (gbuffer_quad, [
            ("NULL gb0, NULL quadUV", dict(out=gb_out(gb0=None), q=None)), ("ssao of zero width, NULL quadUV", dict(s=ssao(width=0), q=None)),
            ("out pitch of 12 000 000, NULL quadUV", dict(out=gb_out(row_pitch_px=wide), q=None))] + quad_ladder(at(0), out=gb_out(height=8)) + [
            ("quadUV on gb0", dict(q=at(0))), ("quadUV on the end of gb3", dict(q=at(3, PLANE - 16))), ("quadUV on ip2", dict(q=ip2)),
            ("quadUV on gb1 and on gb2", dict(q=at(1, PLANE // 2))), ("quadUV on gb3 and on ip2, through the colour plane between them", dict(q=at(3, 16), qpitch=3 * W))]),
        "vqhip_scene_normals_from_materials": (normals, [
            ("NULL out, RGBA16F outFmt", dict(out=None, fmt=F16)), ("RGBA16F outFmt, NULL ip0", dict(fmt=F16, ip=inter(ip0=None))), ("NULL ip2, numMaterials -1", dict(ip=inter(ip2=None), n=-1))]
            + producer_ladder + [("short out pitch, RGBA32F", dict(pitch=W - 1, fmt=F32))]),
        "vqhip_scene_normals_from_materials_quad": (normals_quad, [
            ("RGBA8 outFmt, NULL quadUV", dict(fmt=U8, q=None)), ("a texture of zero height, NULL quadUV", dict(m=bad_mats("texMetalness", height=0), q=None)),
            ("short out pitch, NULL quadUV", dict(pitch=W - 1, q=None))] + quad_ladder(at(0)) + [
            ("quadUV on the last pixels of R10G10B10A2 normals", dict(q=at(0, H * W * 4 - 16))), ("quadUV behind R10G10B10A2 normals, on RGBA32F normals", dict(q=at(0, H * W * 4), fmt=F32)),
            ("quadUV on pitched normals", dict(q=at(1), pitch=8 * W))]),
        "vqhip_forward_lighting_from_materials": (psmain, [
            ("NULL out, NULL ip2", dict(out=None, ip=inter(ip2=None))), ("NULL ip, short out pitch", dict(ip=None, pitch=W - 1))] + producer_ladder + ssao_ladder + [
            ("short out pitch, RGBA8 outFmt", dict(pitch=W - 1, fmt=U8)), ("short out pitch, NULL perFrame", dict(pitch=W - 1, pf=None)), ("NULL perView, RGBA8 outFmt", dict(pv=None, fmt=U8))]
            + lighting_ladder),
        "vqhip_forward_lighting_from_materials_mrt": (psmain_mrt, [
            ("NULL out, RGBA8 albedo_fmt", dict(out=None, mrt=targets(albedo_fmt=U8))), ("ssao of zero width, RGBA8 albedo_fmt", dict(s=ssao(width=0), mrt=targets(albedo_fmt=U8))),
            ("short out pitch, short albedo pitch", dict(pitch=W - 1, mrt=targets(albedo_pitch_px=W - 1)))] + lighting_ladder[:3] + mrt_ladder),
        "vqhip_forward_lighting_from_materials_quad": (psmain_quad, [
            ("numMaterials -1, NULL quadUV", dict(n=-1, q=None)), ("101 point lights, NULL quadUV", dict(pf=pf(numPointLights=101), q=None)),
            ("env without diffuse, NULL quadUV", dict(env=no_diffuse, q=None)), ("RGBA16F motion_fmt, NULL quadUV", dict(mrt=targets(motion_fmt=F16), q=None)),
            ("short sv pitch, misaligned quadUV", dict(mrt=targets(sv_pitch_px=W - 1), q=quv + 4))] + quad_ladder(colour) + [
            ("quadUV on the scene colour", dict(q=colour)),
            ("quadUV behind an RGBA16F scene colour of 12 pitched rows, on an RGBA32F one", dict(ip=inter(height=H // 2), q=at(4, PLANE // 2), pitch=2 * W, fmt=F32)),
            ("quadUV on ip2", dict(q=ip2)), ("quadUV on the scene colour and on ip2", dict(q=at(4, 16))), ("quadUV on the albedo target", dict(q=at(6, 16), mrt=targets(motion_vectors=None))),
            ("quadUV on the motion vectors", dict(q=motion + H * W * 4 - 16)), ("quadUV on the albedo target and on the motion vectors", dict(q=albedo + 16)),
            ("quadUV on an RG32F motion plane's second half", dict(q=motion + H * W * 4, mrt=targets(motion_fmt=abi.FMT_RG32F))),
            ("quadUV on a pitched albedo target", dict(q=at(8), mrt=targets(albedo_pitch_px=3 * W, motion_vectors=None)))]),
    }


def wrong_twice(ctx, small):
    """-> {"<entry point>: <case>": what the library said}; asserts that every call was refused and that no plane was written"""
    out = {}
    with fresh_allocations():
        t = _planes()
        for entry, (call, cases) in _lit_calls(ctx, t).items():
            assert 3 <= len(cases)
            for case, over in cases:
                assert f"{entry}: {case}" not in out, case
                rc = call(**over)
                assert rc in (INV, UNS), f"{entry}: {case}: status {rc}"
                out[f"{entry}: {case}"] = said(entry, rc, (ctx.lib.vqhip_last_error(ctx._h) or b"").decode())
        torch.cuda.synchronize()
        assert torch.equal(t["pool"].view(torch.int32), t["before"].view(torch.int32)), "a refused call wrote to an output or to ip2"
    return out


def test_calls_wrong_twice_get_the_refusal_they_got(ctx, small, golden):
    got, want = wrong_twice(ctx, small), golden["wrong_twice"]
    assert sorted(got) == sorted(want)
    for case in got:
        assert got[case] == want[case], case


# ---- 3. the bindings' own refusals ----------------------------------------------------------------------------------------------------------------------------------------
def _variants(t):
    """the three ways a tensor of the right size can be wrong"""
    doubled = t.repeat_interleave(2, dim=-1)
    return {"dtype": t.to(torch.float64), "shape": t[:-1], "strides": doubled[..., ::2]}


def python_refusals(ctx, small):
    """-> {"<binding>: <argument> <what is wrong with it>": the ValueError's text}. `ctx` is a capi.Context or one of an earlier capi.py"""
    out = {}
    with fresh_allocations():
        z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")                   # noqa: E731
        s = lambda *shape, dtype=torch.float32: torch.full(shape, SENTINEL, dtype=dtype, device="cuda")          # noqa: E731
        pf, extra, pv = TQ.lights(W, H)
        mats = (abi.MaterialDesc * 1)()
        gb, ip, quv, sv, cov = [z(H, W, 4) for _ in range(4)], [z(H, W, 4) for _ in range(3)], z(H, W, 4), [z(H, W, 4) for _ in range(2)], z(H, W, dtype=torch.uint8)
        col, gbo, nrm, bg, ssao = s(H, W, 4, dtype=torch.float16), [s(H, W, 4) for _ in range(4)], torch.full((H, W), 7, dtype=torch.int32, device="cuda"), z(H, W, 4, dtype=torch.float16), cov.clone()

        def swap(planes, k, wrong):
            return [wrong if i == k else p for i, p in enumerate(planes)]
        bindings = {
            "forward_lighting": (ctx.forward_lighting, dict(gb=gb, per_frame=pf, per_view=pv, out=col)),
            "forward_lighting_mrt": (ctx.forward_lighting_mrt, dict(gb=gb, per_frame=pf, per_view=pv, out=col, motion_fmt=M16, sv_curr=sv[0], sv_prev=sv[1])),
            "forward_lighting_msaa": (ctx.forward_lighting_msaa, dict(layers=[gb, gb], coverage=[cov, cov], per_frame=pf, per_view=pv, background=bg, out=col)),
            "gbuffer_from_materials": (ctx.gbuffer_from_materials, dict(ip=ip, materials=mats, ambient=0.1, ssao=ssao, out=gbo)),
            "gbuffer_from_materials_quad": (ctx.gbuffer_from_materials_quad, dict(ip=ip, materials=mats, ambient=0.1, quad_uv=quv, ssao=ssao, out=gbo)),
            "scene_normals_from_materials": (ctx.scene_normals_from_materials, dict(ip=ip, materials=mats, out=nrm)),
            "scene_normals_from_materials_quad": (ctx.scene_normals_from_materials_quad, dict(ip=ip, materials=mats, quad_uv=quv, out=nrm)),
            "forward_lighting_from_materials": (ctx.forward_lighting_from_materials, dict(ip=ip, materials=mats, per_frame=pf, per_view=pv, ssao=ssao, out=col)),
            "forward_lighting_from_materials_mrt": (ctx.forward_lighting_from_materials_mrt, dict(ip=ip, materials=mats, per_frame=pf, per_view=pv, ssao=ssao, out=col, motion_fmt=M16,
                                                                                                  sv_curr=sv[0], sv_prev=sv[1])),
            "forward_lighting_from_materials_quad": (ctx.forward_lighting_from_materials_quad, dict(ip=ip, materials=mats, per_frame=pf, per_view=pv, quad_uv=quv, ssao=ssao, out=col)),
        }
        all3, two, one = ("dtype", "shape", "strides"), ("dtype", "strides"), ("dtype",)
        # argument -> (plane of a list or None, the ways it is made wrong): all three where the binding checks the shape (it does not for ip, for the G-buffer that
        # gbuffer_from_materials writes and for ssao: there a smaller plane would not be refused), the dtype alone where the same check has been through the others
        wrong = {
            "forward_lighting": dict(gb=[(0, one), (2, all3)], out=[(None, all3)]),
            "forward_lighting_mrt": dict(gb=[(3, one)], out=[(None, one)], sv_curr=[(None, all3)], sv_prev=[(None, all3)]),
            "forward_lighting_msaa": dict(background=[(None, all3)], out=[(None, all3)]),
            "gbuffer_from_materials": dict(ip=[(0, two), (1, one), (2, one)], out=[(0, one), (3, two)], ssao=[(None, two)]),
            "gbuffer_from_materials_quad": dict(ip=[(1, one)], out=[(2, one)], ssao=[(None, one)], quad_uv=[(None, all3)]),
            "scene_normals_from_materials": dict(ip=[(0, one), (2, two)]),
            "scene_normals_from_materials_quad": dict(ip=[(1, one)], quad_uv=[(None, all3)]),
            "forward_lighting_from_materials": dict(ip=[(0, one), (1, two)], out=[(None, all3)], ssao=[(None, two)]),
            "forward_lighting_from_materials_mrt": dict(ip=[(2, one)], out=[(None, one)], ssao=[(None, one)], sv_curr=[(None, one)], sv_prev=[(None, one)]),
            "forward_lighting_from_materials_quad": dict(ip=[(0, one)], out=[(None, one)], ssao=[(None, one)], quad_uv=[(None, all3)]),
        }

        def raised(key, call, **kw):
            with pytest.raises(ValueError) as e:
                call(**kw)
            assert key not in out, key
            out[key] = str(e.value)
        for name, (call, good) in bindings.items():
            for arg, places in wrong[name].items():
                for k, ways in places:
                    for way in ways:
                        plane = good[arg] if k is None else good[arg][k]
                        bad = _variants(plane)[way]
                        raised(f"{name}: {arg}{'' if k is None else f'[{k}]'} with the wrong {way}", call, **dict(good, **{arg: bad if k is None else swap(good[arg], k, bad)}))
        # the layer, coverage and background checks of forward_lighting_msaa
        call, good = bindings["forward_lighting_msaa"]
        raised("forward_lighting_msaa: no layers", call, **dict(good, layers=[], coverage=[]))
        raised("forward_lighting_msaa: five layers", call, **dict(good, layers=[gb] * 5, coverage=[cov] * 5))
        raised("forward_lighting_msaa: two layers and one coverage plane", call, **dict(good, coverage=[cov]))
        for way in all3:
            raised(f"forward_lighting_msaa: layer 1 gb2 with the wrong {way}", call, **dict(good, layers=[gb, swap(gb, 2, _variants(gb[2])[way])]))
            raised(f"forward_lighting_msaa: coverage 1 with the wrong {way}", call, **dict(good, coverage=[cov, _variants(cov)[way]]))
        raised("forward_lighting_msaa: layer 0 gb0 with the wrong dtype", call, **dict(good, layers=[swap(gb, 0, _variants(gb[0])["dtype"]), gb]))
        raised("forward_lighting_msaa: background of another format than out", call, **dict(good, background=z(H, W, 4)))
        # _psmain_targets
        for name in ("forward_lighting_mrt", "forward_lighting_from_materials_mrt", "forward_lighting_from_materials_quad"):
            call, good = bindings[name]
            raised(f"{name}: motion vectors without sv_curr", call, **dict(good, motion_fmt=M16, sv_curr=None, sv_prev=sv[1]))
            raised(f"{name}: motion vectors without sv_prev", call, **dict(good, motion_fmt=M16, sv_curr=sv[0], sv_prev=None))
        # a call that is wrong twice: the earlier check speaks
        for name, over in (("forward_lighting", dict(gb=swap(gb, 1, gb[1].half()), out=col[:-1])), ("forward_lighting_msaa", dict(background=z(H, W, 4), out=col[:-1])),
                           ("gbuffer_from_materials", dict(ip=swap(ip, 2, ip[2].half()), out=swap(gbo, 1, gbo[1].half()))),
                           ("gbuffer_from_materials", dict(out=swap(gbo, 1, gbo[1].half()), ssao=ssao.int())),
                           ("gbuffer_from_materials_quad", dict(ssao=ssao.int(), quad_uv=quv[:, :-1])),
                           ("scene_normals_from_materials_quad", dict(ip=swap(ip, 0, ip[0].half()), quad_uv=quv.half())),
                           ("forward_lighting_from_materials", dict(ip=swap(ip, 1, ip[1].half()), out=col.float())), ("forward_lighting_from_materials", dict(out=col.float(), ssao=ssao[0])),
                           ("forward_lighting_from_materials_quad", dict(ssao=ssao[0], quad_uv=quv[::2])),
                           ("forward_lighting_from_materials_quad", dict(out=col[:-1], motion_fmt=M16))):
            call, good = bindings[name]
            raised(f"{name}: {', '.join(sorted(over))} that do not fit", call, **dict(good, **over))
        torch.cuda.synchronize()
        assert bool((col == SENTINEL).all()) and all(bool((g == SENTINEL).all()) for g in gbo) and bool((nrm == 7).all()), "a refused call wrote to an output"
    return out


def test_bindings_raise_what_they_raised(ctx, small, golden):
    got, want = python_refusals(ctx, small), golden["python"]
    assert sorted(got) == sorted(want)
    for case in got:
        assert got[case] == want[case], case
