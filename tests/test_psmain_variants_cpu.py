"""What tests/test_gpu_psmain_variants.py counts on, asserted from the oracle alone (tests/psmain_variant_cases.py): conditions on the frames, not measurements of
the product. A frame that misses one is to be changed; the floors stay.

  (a) frame P's oracle G-buffer has covered pixels with roughness below 0.04 (the EPSILON-select form of the point-light loop). Found: 1 271 of 3 745 covered
      pixels; frame Q (room_129x67_s1) has them too without any planting: 846 of its 8 258 covered pixels, down to roughness 0.
  (b) both frames have covered and uncovered pixels, frame P has discarded fragments. Found: P 3 745 covered / 1 102 uncovered, 459 of them discarded by the
      alpha mask; Q 8 258 / 385 (the room fills its view: Q's uncovered pixels are the block psmain_variant_cases.Q_HOLE cuts out of it).
  (c) with casters, replacing every shadow map by depth 1.0 changes >= 10 % of the covered pixels of the oracle image;
  (d) with IBL, dropping the environment changes >= 90 % of them;
  (e) the DXC and the literal oracle image of every frame and kind differ somewhere.

Shares found, literal reading (RGBA16F / RGBA32F); (c) shadow maps, (d) IBL:
  frame P  casters      (c) 0.898 / 0.908                 env      (d) 1.000 / 1.000      env+casters  (c) 0.771 / 0.908  (d) 1.000 / 1.000
  frame Q  casters      (c) 0.969 / 0.969                 env      (d) 1.000 / 1.000      env+casters  (c) 0.957 / 0.969  (d) 1.000 / 1.000
  frame L  casters      (c) 0.560 / 0.567                 env      (d) 1.000 / 1.000      env+casters  (c) 0.529 / 0.566  (d) 1.000 / 1.000
(frame L, synth.gbuffer at 333 x 6 for k_forward_lighting, has no uncovered pixels: its shares are of all pixels. Frame Q's are with the shadow views and the
caster lights of psmain_variant_cases.room_casters: under ref_cases.shadow_scene's own layout, made for frames a hundred units across, the room sits on a few
texels of each map.)"""
import numpy as np
import pytest

from tests import oracle_lib as O
from tests import psmain_variant_cases as V
from tests import quad_interp_cases as QC
from tests import ref_cases

F16, F32 = V.F16, V.F32
FRAMES = ("P", "Q", "L")


def _frame(frame, dxc=False):
    """(G-buffer, pixels that count, scene of a kind, expected image of (kind, fmt, dxc))"""
    if frame == "L":
        gb = V.l_gbuffer()[0]
        return gb, np.ones(gb[0].shape[:2], bool), V.l_scene, V.l_expected
    form = "plain" if frame == "P" else "quad"
    return (V.fused_gbuffer(form, dxc)[0], V.covered(form, dxc), lambda kind: V.fused_scene(form, kind), lambda kind, fmt, d: V.fused_expected(form, kind, fmt, d))


def test_frame_p_has_polished_pixels_discards_and_a_hole():
    for dxc in (False, True):
        gb, after = V.p_gbuffer(dxc)
        before = np.ascontiguousarray(V.p_interpolants()[2][..., 3]).view(np.int32)
        cov = V.covered("plain", dxc)
        assert int(((gb[1][..., 3] < 0.04) & cov).sum()) >= 64, "(a) less than a wave of covered pixels with roughness below 0.04"
        assert cov.any() and (~cov).any(), "(b)"
        valid = (before >= 0) & (before < V.P_NMAT)
        discarded = valid & (after == -1)
        assert discarded.any() and (valid & ~discarded & (before == V.P_MASKED)).any(), "(b) the alpha mask discards none or all of its material's fragments"
        assert set(range(V.P_NMAT)) <= set(np.unique(before).tolist()), "a material of the table occurs nowhere in the frame"
        assert (before[V.P_HOLE] == -1).all() and not any(g[V.P_HOLE].view(np.uint32).any() for g in gb)
        assert not any(g[~cov].view(np.uint32).any() for g in gb), "an uncovered pixel's record is not all-zero"
    assert (V.PW % 32, V.PW % 128, V.PH % 2) != (0, 0, 0) and V.PW > 128


def test_frame_q_has_covered_and_uncovered_pixels_and_restates_its_case():
    for dxc in (False, True):
        gb, after = V.q_gbuffer(dxc)                                   # asserts the restatement against quad_interp_cases.expected_gbuffer
        cov = V.covered("quad", dxc)
        assert cov.any() and (~cov).any(), "(b)"
        assert ((gb[1][..., 3] < 0.04) & cov).any()
    assert (V.QW % 2, V.QH % 2) == (1, 1) and QC.cases()[V.Q_NAME]["samples"] == 1


def test_frame_l_carries_its_plants():
    gb, above = V.l_gbuffer()
    r = gb[1][..., 3]
    assert {float(np.float32(x)) for x in (0.0, 0.01, 0.039, 2.0)} <= set(np.unique(r).tolist())
    assert all(V.LW % wg for wg in (64, 128, 256)) and V.LW > 256
    P = gb[0][V.L_ABOVE]
    sc = V.l_scene("plain")
    pos = sc["pf"].Lights.point_lights[0].position
    assert (pos.x, pos.z) == (float(P[0]), float(P[2])) and pos.y > float(P[1]), "point light 0 is not exactly above its pixel"


def test_kinds_without_casters_use_the_extension_array():
    for sc in (V.fused_scene("plain", "plain"), V.fused_scene("quad", "env"), V.l_scene("plain")):
        assert sc["pf"].Lights.numPointLights == V.abi.NUM_LIGHTS__POINT and len(sc["extra"]) == 4
    gb, sc = V.l_gbuffer()[0], V.l_scene("plain")
    with_extra = V.shade(gb, sc, F32, False)
    without = V.shade(gb, dict(sc, extra=None), F32, False)
    assert V.changed(with_extra, without, np.ones(gb[0].shape[:2], bool)) >= 0.10, "the lights of the extension array reach almost no pixel"


@pytest.mark.parametrize("fmt", [F16, F32])
@pytest.mark.parametrize("kind", V.KINDS)
@pytest.mark.parametrize("frame", FRAMES)
def test_casters_and_ibl_decide_the_image(frame, kind, fmt):
    """(c) and (d), in both readings"""
    for dxc in (False, True):
        gb, where, scene_of, expected = _frame(frame, dxc)
        sc, want = scene_of(kind), expected(kind, fmt, dxc)
        assert (sc["shadow"] is not None) == ("casters" in kind) and (sc["env"] is not None) == ("env" in kind)
        if sc["shadow"] is not None:
            share = V.changed(want, V.shade(gb, sc, fmt, dxc, shadow=False), where)
            assert share >= 0.10, f"(c) frame {frame}, {kind}: shadow maps decide only {share:.3f} of the covered pixels"
        if sc["env"] is not None:
            share = V.changed(want, V.shade(gb, sc, fmt, dxc, env=False), where)
            assert share >= 0.90, f"(d) frame {frame}, {kind}: IBL decides only {share:.3f} of the covered pixels"


@pytest.mark.parametrize("kind", V.KINDS)
@pytest.mark.parametrize("frame", FRAMES)
def test_the_two_readings_are_two_images(frame, kind):
    """(e), in both formats"""
    _, where, _, expected = _frame(frame)
    for fmt in (F16, F32):
        assert V.changed(expected(kind, fmt, False), expected(kind, fmt, True), np.ones_like(where)) > 0.0, f"(e) frame {frame}, {kind}, fmt {fmt}"


def test_room_casters_keep_the_maps_of_shadow_scene():
    _, s = ref_cases.shadow_scene()
    sc = V.fused_scene("quad", "env+casters")
    assert all(np.array_equal(sc["shadow"][k], s[k]) for k in s) and sc["shadow"]["dims"] == V.SHADOW_DIMS
    plain = V.fused_scene("plain", "casters")
    pf, _ = ref_cases.shadow_scene()
    assert bytes(plain["pf"]) == bytes(pf), "outside the room the casters are ref_cases.shadow_scene's, untouched"


def test_expectations_are_shared_and_read_only():
    a = V.fused_expected("plain", "env", F16, False)
    assert a is V.fused_expected("plain", "env", F16, False) and not a.flags.writeable
    n, _ = O.bits_equal(a, V.shade(V.p_gbuffer(False)[0], V.fused_scene("plain", "env"), F16, False))
    assert n == 0
