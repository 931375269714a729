"""-m gpu: EVERY instantiation of the two kernels that shade a frame's pixels, bit for bit against the oracle chain (tests/oracle_lib.py) on small ragged frames.
The frames, lights and expectations are tests/psmain_variant_cases.py's; what makes them worth running (polished pixels, discards, holes, casters and IBL that
decide the image, two readings that differ) is asserted from the oracle alone in tests/test_psmain_variants_cpu.py.

k_forward_from_materials<HAS_ENV, HAS_CASTERS, OUTFMT, WAVES, AR, QA...> (vqengine_amd/csrc/gbuffer.hip, launchForward), 64 instantiations:
  test_fused_every_variant[form-kind-fmt-cap]   form   plain -> QA empty (vqhip_forward_lighting_from_materials), frame P 131 x 37
                                                       quad  -> QA = QuadPlane (vqhip_forward_lighting_from_materials_quad), frame Q 129 x 67
                                                kind   plain | env | casters | env+casters -> (HAS_ENV, HAS_CASTERS)
                                                fmt    RGBA16F -> OUTFMT 1, RGBA32F -> OUTFMT 0
                                                cap    w4 | w5 | w6 -> (WAVES 4 | 5 | 6, AR 0) through option psmain_waves; dxc -> (WAVES = the default, AR 1)
  test_fused_extra_targets_under_the_other_caps (true, true, both formats, WAVES 4 | 5, AR 0) of both forms with SV_TARGET1 and the motion vectors bound
  test_dxc_reading_ignores_psmain_waves         (true, true, RGBA16F, default WAVES, AR 1) of both forms with psmain_waves = 4 set
  test_psmain_waves_refuses_other_values        the option's argument check: 3 and 7

k_forward_lighting<HAS_ENV, HAS_CASTERS, OUTFMT, AR, MRT> (vqengine_amd/csrc/shade.hip, launch_forward_lighting), 32 instantiations, frame L 333 x 6:
  test_forward_lighting_every_variant[kind-fmt-reading-mrt]   kind -> (HAS_ENV, HAS_CASTERS), fmt -> OUTFMT, reading literal | dxc -> AR 0 | 1,
                                                              mrt targets | colour -> MRT true (vqhip_forward_lighting_mrt, both targets) | false
  test_forward_lighting_workgroup_shapes[kind-wg]             (kind, RGBA16F, AR 0, MRT false) launched with 64, 128 and 256 lanes (option shade_wg): 333 is no
                                                              multiple of any, the last workgroup of every row is partial
  test_forward_lighting_single_lane_and_one_lane_past_a_workgroup   1 x 1 and 257 x 1 at 256 lanes: one live lane; a second workgroup with one live lane"""
import numpy as np
import pytest
import torch

from tests import psmain_variant_cases as V
from tests import ref_cases
from tests import test_gpu_msaa_edges as E
from tests import test_gpu_quad_interp as TQ
from tests.test_gpu_gbuffer import build_materials
from vqengine_amd import abi, synth

pytestmark = pytest.mark.gpu
dev = TQ.dev                                       # a copy: the shared inputs are read-only
F16, F32 = V.F16, V.F32
FMT_IDS = {F16: "rgba16f", F32: "rgba32f"}
CAPS = ("w4", "w5", "w6", "dxc")
assert_bits = TQ.assert_bits


# ---- device inputs ------------------------------------------------------------------------------------------------------------------------------------------------------
def _p_device_materials(ctx):
    """frame P's device material table: tests/test_gpu_gbuffer.build_materials' (device chains compared there with the oracle's), then the edits of
    psmain_variant_cases on the same records. The helper module's restatement of build_materials' host side must give build_materials' chains."""
    def make():
        hmats, plain_chains = V.p_host_materials()
        datas, host_chains, _, dmats, keep = build_materials(ctx, V.P_NMAT, seed=V.P_MAT_SEED, max_dim=V.P_MAX_DIM)
        assert len(host_chains) == len(plain_chains)
        for a, b in zip(host_chains, plain_chains):
            assert a.keys() == b.keys() and all(np.array_equal(a[s][0], b[s][0]) and a[s][1:] == b[s][1:] for s in a), "psmain_variant_cases no longer restates build_materials"
        V.p_edit_material_data([dmats[i].data for i in range(V.P_NMAT)])
        for slot in abi.MATERIAL_TEXTURE_SLOTS:
            setattr(dmats[V.P_BARE], slot, abi.Texture2D())
        _, texsets = V.p_material_set()
        img = V.p_masked_diffuse(texsets[V.P_MASKED]["texDiffuse"])
        chain, n = ctx.mip_chain_rgba8(dev(img))
        assert np.array_equal(chain.cpu().numpy(), hmats._keep[V.P_MASKED]["texDiffuse"][0])
        keep.append(chain)
        dmats[V.P_MASKED].texDiffuse = abi.Texture2D(chain.data_ptr(), img.shape[1], img.shape[0], n, abi.MATERIAL_ALPHA_MASKED)
        for i in range(V.P_NMAT):
            assert bytes(dmats[i].data) == bytes(hmats[i].data), i
            for slot in abi.MATERIAL_TEXTURE_SLOTS:
                d, h = getattr(dmats[i], slot), getattr(hmats[i], slot)
                assert (bool(d.texels), d.width, d.height, d.mips, d.reserved) == (bool(h.texels), h.width, h.height, h.mips, h.reserved), (i, slot)
        return dmats, keep
    return V.memo(("device", "P materials"), make)[0]


def _q_device_materials(ctx):
    def make():
        mats = TQ.device_materials(ctx, V.Q_NAME)
        return mats, list(TQ._KEEP)                # that module releases its chains after each of ITS tests: hold them here
    return V.memo(("device", "Q materials"), make)[0]


def _device_lights(sc):
    """(env, shadow, the tensors they point into) of a scene with device pointers"""
    keep = []
    return ref_cases.dev_env(sc["env"], keep), ref_cases.dev_shadow_dims(sc["shadow"], keep) if sc["shadow"] is not None else None, keep


def _fused(ctx, form, kind, fmt, targets=False):
    """one launch of the fused kernel on the form's frame -> (colour, albedo | None, motion | None, ip2.w after the call)"""
    sc = V.fused_scene(form, kind)
    env, shadow, _keep = _device_lights(sc)
    kw = dict(out_fmt=fmt, extra_point=sc["extra"], env=env, shadow=shadow)
    mrt = {}
    if form == "plain":
        ip, mats, kw["ssao"] = [dev(p) for p in V.p_interpolants()], _p_device_materials(ctx), dev(V.p_ssao())
        cur, prev = V.p_clip_positions()
    else:
        _, quv = TQ.dev_planes(V.q_planes())                                   # the quad plane is the case's own; the three planes carry the hole
        ip, mats, kw["ssao"] = [dev(p) for p in V.q_interpolants()[0]], _q_device_materials(ctx), dev(V.q_ssao())
        cur, prev = V.q_clip_positions()
    if targets:
        afmt, mfmt = V.MRT_FMTS[fmt]
        mrt = dict(albedo_fmt=afmt, motion_fmt=mfmt, sv_curr=dev(cur), sv_prev=dev(prev))
    if form == "plain":
        got = ctx.forward_lighting_from_materials_mrt(ip, mats, sc["pf"], sc["pv"], **mrt, **kw) if targets else ctx.forward_lighting_from_materials(ip, mats, sc["pf"], sc["pv"], **kw)
    else:
        got = ctx.forward_lighting_from_materials_quad(ip, mats, sc["pf"], sc["pv"], quv, **mrt, **kw)
    torch.cuda.synchronize()
    colour, albedo, motion = got if targets else (got, None, None)
    return colour, albedo, motion, ip[2][..., 3].contiguous().view(torch.int32).cpu().numpy()


def _set_cap(ctx, set_opt, cap):
    """the register cap of a case: psmain_waves in the literal reading, or the DXC reading (a context manager either way)"""
    if cap != "dxc":
        set_opt("psmain_waves", int(cap[1]))
    return V.reading(cap == "dxc", ctx)


# ---- the helper module builds its lights as the edge tests do ----------------------------------------------------------------------------------------------------------
def test_scenes_restate_the_edge_tests_scenes():
    """psmain_variant_cases.scene against tests/test_gpu_msaa_edges._scene at the same size, seed and planted light: the casters are the same bytes and maps; without
    casters the spots, the directional light and the first twelve point lights are, and 92 more point lights follow"""
    above = V.l_gbuffer()[1]
    for kind in V.KINDS:
        mine, theirs = V.scene(kind, V.LW, V.LH, V.L_SEED, above=above), E._scene(kind, V.LW, V.LH, seed=V.L_SEED, above=above)
        assert bytes(mine["pv"]) == bytes(theirs["pv"]) and (mine["env"] is None) == (theirs["env"] is None)
        if "casters" in kind:
            assert bytes(mine["pf"]) == bytes(theirs["pf"]) and mine["extra"] is None and theirs["extra"] is None
            assert mine["shadow"]["dims"] == theirs["shadow"]["dims"] and all(np.array_equal(mine["shadow"][k], theirs["shadow"][k]) for k in ("dir", "spot", "point"))
        else:
            a, b = mine["pf"].Lights, theirs["pf"].Lights
            assert b.numPointLights == 12 and a.numPointLights == abi.NUM_LIGHTS__POINT
            assert all(bytes(a.point_lights[i]) == bytes(b.point_lights[i]) for i in range(12))
            assert a.numSpotLights == b.numSpotLights == 2 and all(bytes(a.spot_lights[i]) == bytes(b.spot_lights[i]) for i in range(2))
            assert bytes(a.directional) == bytes(b.directional)
        if mine["env"] is not None:
            assert all(np.array_equal(mine["env"][k], theirs["env"][k]) for k in ("diffuse", "specular", "lut"))


# ---- k_forward_from_materials ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("fmt", [F16, F32], ids=FMT_IDS.get)
@pytest.mark.parametrize("kind", V.KINDS)
@pytest.mark.parametrize("form", V.FORMS)
def test_fused_every_variant(ctx, set_opt, form, kind, fmt, cap):
    """one instantiation per case (the module docstring maps the axes). Every pixel, covered or not (an uncovered pixel shades the all-zero record), and ip2.w after
    the call against the oracle's discards. w4, w5 and w6 share one expectation: the three caps agree."""
    dxc = cap == "dxc"
    want, want_idx = V.fused_expected(form, kind, fmt, dxc), V.fused_gbuffer(form, dxc)[1]
    with _set_cap(ctx, set_opt, cap):
        colour, _, _, idx = _fused(ctx, form, kind, fmt)
    assert_bits(colour, want, f"fused {form} form, {kind}, {FMT_IDS[fmt]}, {cap}")
    assert np.array_equal(idx, want_idx), f"fused {form} form, {kind}, {FMT_IDS[fmt]}, {cap}: ip2.w after the call differs at {np.argwhere(idx != want_idx)[:5].tolist()}"


@pytest.mark.parametrize("cap", ["w4", "w5"])
@pytest.mark.parametrize("fmt", [F16, F32], ids=FMT_IDS.get)
@pytest.mark.parametrize("form", V.FORMS)
def test_fused_extra_targets_under_the_other_caps(ctx, set_opt, form, fmt, cap):
    """SV_TARGET1 and the motion vectors from the 4- and 5-wave forms under IBL + casters: the colour as without them, the targets the oracle's on covered pixels,
    the clear value on the others (PSMain never runs there)"""
    kind = "env+casters"
    want_a, want_m = V.fused_extra_targets(form, fmt)
    cov = V.covered(form)
    with _set_cap(ctx, set_opt, cap):
        colour, albedo, motion, idx = _fused(ctx, form, kind, fmt, targets=True)
    what = f"fused {form} form with targets, {FMT_IDS[fmt]}, {cap}"
    assert_bits(colour, V.fused_expected(form, kind, fmt, False), what)
    assert np.array_equal(idx, V.fused_gbuffer(form, False)[1]), what
    for got, ref, name in ((albedo.cpu().numpy(), want_a, "albedo / metalness"), (motion.cpu().numpy(), want_m, "motion vectors")):
        assert_bits(np.ascontiguousarray(got[cov]), np.ascontiguousarray(ref[cov]), f"{what}: {name} on covered pixels")
        assert not got[~cov].view(np.uint8).any(), f"{what}: {name} written on a pixel without a fragment"


@pytest.mark.parametrize("form", V.FORMS)
def test_dxc_reading_ignores_psmain_waves(ctx, set_opt, form):
    """the DXC reading has one register cap: psmain_waves = 4 must launch the same instantiation — the default's bits, which are the oracle's"""
    kind = "env+casters"
    with V.reading(True, ctx):
        default, _, _, _ = _fused(ctx, form, kind, F16)
        set_opt("psmain_waves", 4)
        capped, _, _, idx = _fused(ctx, form, kind, F16)
    assert torch.equal(default.view(torch.int16), capped.view(torch.int16)), f"{form} form: psmain_waves changed the DXC reading's image"
    assert_bits(capped, V.fused_expected(form, kind, F16, True), f"fused {form} form, DXC reading, psmain_waves = 4")
    assert np.array_equal(idx, V.fused_gbuffer(form, True)[1])


def test_psmain_waves_refuses_other_values(ctx):
    for value in (b"3", b"7"):
        assert ctx.lib.vqhip_set_option(ctx._h, b"psmain_waves", value) == abi.VQHIP_ERR_INVALID_ARG, value
    colour, _, _, _ = _fused(ctx, "plain", "plain", F16)
    assert_bits(colour, V.fused_expected("plain", "plain", F16, False), "frame P after two refused values of psmain_waves")


# ---- k_forward_lighting ---------------------------------------------------------------------------------------------------------------------------------------------------
def _lit(ctx, gb, sc, fmt, clip=None):
    """vqhip_forward_lighting, or with clip = (sv_curr, sv_prev) vqhip_forward_lighting_mrt with both targets -> (colour, albedo | None, motion | None)"""
    env, shadow, _keep = _device_lights(sc)
    kw = dict(out_fmt=fmt, extra_point=sc["extra"], env=env, shadow=shadow)
    gbd = [dev(g) for g in gb]
    if clip is None:
        got = ctx.forward_lighting(gbd, sc["pf"], sc["pv"], **kw), None, None
    else:
        afmt, mfmt = V.MRT_FMTS[fmt]
        got = ctx.forward_lighting_mrt(gbd, sc["pf"], sc["pv"], albedo_fmt=afmt, motion_fmt=mfmt, sv_curr=dev(clip[0]), sv_prev=dev(clip[1]), **kw)
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("mrt", [False, True], ids=["colour", "targets"])
@pytest.mark.parametrize("dxc", [False, True], ids=["literal", "dxc"])
@pytest.mark.parametrize("fmt", [F16, F32], ids=FMT_IDS.get)
@pytest.mark.parametrize("kind", V.KINDS)
def test_forward_lighting_every_variant(ctx, kind, fmt, dxc, mrt):
    gb, sc = V.l_gbuffer()[0], V.l_scene(kind)
    what = f"frame L, {kind}, {FMT_IDS[fmt]}, DXC reading {dxc}, extra targets {mrt}"
    with V.reading(dxc, ctx):
        colour, albedo, motion = _lit(ctx, gb, sc, fmt, V.l_clip_positions() if mrt else None)
    assert_bits(colour, V.l_expected(kind, fmt, dxc), what)
    if mrt:
        want_a, want_m = V.l_extra_targets(fmt)
        assert_bits(albedo, want_a, what + ": albedo / metalness")
        assert_bits(motion, want_m, what + ": motion vectors")


@pytest.mark.parametrize("wg", [64, 128, 256])
@pytest.mark.parametrize("kind", V.KINDS)
def test_forward_lighting_workgroup_shapes(ctx, set_opt, kind, wg):
    set_opt("shade_wg", wg)
    colour, _, _ = _lit(ctx, V.l_gbuffer()[0], V.l_scene(kind), F16)
    assert_bits(colour, V.l_expected(kind, F16, False), f"frame L, {kind}, {wg} lanes per workgroup")


def test_forward_lighting_single_lane_and_one_lane_past_a_workgroup(ctx, set_opt):
    set_opt("shade_wg", 256)
    for w in (1, 257):
        gb = synth.gbuffer(w, 1, seed=V.L_SEED + w)
        sc = V.scene("env+casters", w, 1, V.L_SEED)
        colour, _, _ = _lit(ctx, gb, sc, F16)
        assert_bits(colour, V.shade(gb, sc, F16, False), f"{w} x 1 at 256 lanes per workgroup")
