"""What the rasterisers' shared host front end (capi.hip: badMeshDraw, stageJobs, stageMask) could break, on the GPU, for vqhip_shadow_depth, vqhip_scene_depth and
their masked forms — vqhip_scene_interpolants has test_many_draws_cross_the_ring_slots of its own:
  * calls whose job table, and in the masked calls whose texture table, fills two whole constant-ring slots and part of a third, bit for bit against the
    statement references (tests/shadow_raster_ref.py, scene_depth_ref.py, masked_depth_ref.py). Only such calls show whether firstBlock restarts in each slot
    while firstQ, firstMasked and maskSlot run on;
  * the whole text of every refusal the five *_refusals_launch_nothing tests provoke, as the library worded it while each entry point had a check ladder of its
    own (taken from that source): those tests are run as they stand on a context whose vqhip_last_error is written down."""
import numpy as np
import pytest

from tests import masked_depth_cases as MC
from tests import masked_depth_ref as M
from tests import raster_ring_cases as RC
from tests import scene_depth_cases as SC
from tests import scene_depth_ref as V
from tests import shadow_raster_cases as K
from tests import shadow_raster_ref as R
from tests import test_gpu_masked_depth as TM
from tests import test_gpu_scene_depth as TD
from tests import test_gpu_scene_interp as TI
from tests import test_gpu_shadow_raster as TS

pytestmark = pytest.mark.gpu
SLOT = RC.RING_SLOT_BYTES
RING_TEX = ("t8", "t12", "cols8")


@pytest.fixture(autouse=True)
def _release_device_chains():
    """as tests/test_gpu_masked_depth.py does: its helpers keep the textures' device copies alive for one test"""
    yield
    TM._KEEP.clear()


# ---- jobs across ring slots --------------------------------------------------------------------------------------------------------------------------------------------
def test_shadow_draws_cross_the_ring_slots(ctx):
    """1 500 draws of one triangle each in two 48-texel views, 900 in a z / w map and 600 in a linear one. A RasterJob is 64 bytes and a ring slot holds
    44 544 // 64 = 696 of them, so the call stages slots of 696, 696 and 108 jobs: firstBlock restarts in each, and the view changes inside the second"""
    per_slot = SLOT // 64
    n = 2 * per_slot + 108
    assert (per_slot, n) == (696, 1500)
    draws = RC.slot_crossing_draws(n, seed=21)
    views = [K.view(48, draws[:900]), K.view(48, draws[900:], linear=True, camera=(0.1, -0.2, -1.5), far=8.0)]
    ref = R.rasterize(views)
    assert all((m < 1.0).sum() > 1000 for m in ref)
    for i, (g, e) in enumerate(zip(TS.run(ctx, views), ref)):
        TS.assert_same(f"1500 draws view {i}", g, e)


def test_scene_draws_cross_the_ring_slots(ctx):
    """1 500 draws of one triangle each on a 48 x 48 target, at both sample counts. A SceneDepthJob is 64 bytes and a ring slot holds 44 544 // 64 = 696 of
    them, so the call stages slots of 696, 696 and 108 jobs: firstBlock restarts in each, firstQ runs on — primitive and every layerPrimitive name the owners"""
    per_slot = SLOT // 64
    n = 2 * per_slot + 108
    assert (per_slot, n) == (696, 1500)
    draws = RC.slot_crossing_draws(n, seed=21)
    for s in (1, 4):
        scene = SC.scene(48, 48, s, draws)
        ref = V.rasterize(scene)
        owners = np.unique(ref["primitive"])
        assert len(owners) > 600 and owners[owners != V.NO_PRIMITIVE].max() >= 2 * per_slot, "owners from all three slots"
        TD.assert_outputs(f"1500 draws at {s}x", TD.run(ctx, scene), ref, 48)


def test_masked_scene_draws_cross_the_ring_slots(ctx):
    """1 642 draws of one triangle each on a 48 x 48 target, at both sample counts; two of every three carry a masked material, each with its own uvScaleOffset,
    and every eleventh of those lacks the diffuse bit (masked by the header's rule, no table entry, maskSlot 0). A ring slot of 44 544 bytes holds 696
    SceneDepthJobs (64 bytes) and 928 MaskTex entries (48 bytes): the jobs go in slots of 696, 696 and 250, the 995 table entries in slots of 928 and 67, and
    firstQ, firstMasked and maskSlot run across all of them with opaque draws in between"""
    per_job, per_tex = SLOT // 64, SLOT // 48
    n = 2 * per_job + 250

    def mask_of(k):
        if k % 3 == 0:
            return None
        return MC.mask(RING_TEX[k % 3 if k % 2 else 0], (1.0 + 0.25 * (k % 4), 1.0 - 0.5 * (k % 3), 0.125 * (k % 5), -0.25 * (k % 2)), 2.0 if k % 11 == 3 else 1.0)
    draws = RC.slot_crossing_draws(n, seed=22, mask_of=mask_of)
    entries = sum(d["mask"] is not None and d["mask"]["texture_config"] == 1.0 for d in draws)
    assert (per_job, per_tex, n, entries) == (696, 928, 1642, 995)
    for s in (1, 4):
        scene = MC.scene(48, 48, s, draws)
        st = M.new_stats()
        ref = M.rasterize_scene(scene, stats=st)
        owners = np.unique(ref["primitive"])
        assert st["discarded"] > 50 and len(owners) > 600 and owners[owners != 0xFFFFFFFF].max() >= 2 * per_job
        TD.assert_outputs(f"1642 draws at {s}x", TM.run(ctx, scene), ref, 48)


def test_masked_shadow_draws_cross_the_ring_slots(ctx):
    """1 500 draws of one triangle each in two 48-texel views (700 z / w, 800 linear), two of every three with a texture. A ring slot of 44 544 bytes holds 556
    RasterMaskedJobs (80 bytes) and 928 MaskTex entries (48 bytes): the jobs go in slots of 556, 556 and 388, the 1 000 table entries in slots of 928 and 72;
    the view changes inside the second job slot, firstMasked and maskSlot run across all of them with opaque draws in between"""
    per_job, per_tex = SLOT // 80, SLOT // 48
    n = 2 * per_job + 388
    draws = RC.slot_crossing_draws(n, seed=23, mask_of=lambda k: None if k % 3 == 0 else MC.mask(RING_TEX[k % 3 if k % 2 else 0]))
    assert (per_job, per_tex, n, sum(d["mask"] is not None for d in draws)) == (556, 928, 1500, 1000)
    views = [MC.view(48, draws[:700]), MC.view(48, draws[700:], True, (0.1, -0.2, -1.5), 8.0)]
    st = M.new_stats()
    ref = M.rasterize_shadow(views, stats=st)
    assert st["discarded"] > 500 and all((m < 1.0).sum() > 1000 for m in ref)
    TM.assert_maps("1500 draws", TM.run_shadow(ctx, views), ref, [48, 48])


# ---- refusal texts -------------------------------------------------------------------------------------------------------------------------------------------------------
class _Listening:
    """`inner` (a Context, or its library) with every answer of vqhip_last_error written down"""
    def __init__(self, inner, texts):
        self._inner, self._texts = inner, texts
        if hasattr(inner, "lib"):
            self.lib = _Listening(inner.lib, texts)

    def __getattr__(self, name):
        attr = getattr(self._inner, name)
        if name != "vqhip_last_error":
            return attr

        def last_error(handle):
            text = attr(handle)
            self._texts.append((text or b"").decode())
            return text
        return last_error


_V, _D = "view 0: ", "view 0 draw 0: "
_NULL_DRAW = "positions, indices or matWorldViewProj is NULL"
_SIZE = "width and height must be 1..8192"
_STRIDE12 = "strideBytes below 12 or not a multiple of 4"
_MASK_STRIDE = "a masked draw needs the engine's vertex (uv at byte 36): strideBytes below 44"
_MASK_SIZE = "masked texture: width and height must be 1..16384"
_MASK_MIPS = "masked texture: mips must be 1..vqhip_mip_level_count(width, height)"
_MASK_TEXELS = "masked texture: texels must be 4-byte aligned"
_SCENE_NULL = "NULL argument (out, out->depth or work)"
_SCENE_ALIGN = "depth / primitive must be 4-byte (samples 1) or 16-byte (samples 4) aligned"
_IP_NULL = "NULL argument (out, ip0, ip1, ip2, owner or work)"
_IP_NULL_DRAW = "draw 0: positions, indices, matWorldViewProj, matWorld or matNormal is NULL"
_IP_MISALIGNED = "draw 0: positions / matrices must be 4-byte aligned, indices aligned to their size"
_OWNER = "an output overlaps the owner plane"
# per refusal test, in the order of its cases: the text after "<entry point>: "; a tuple: either
REFUSALS = {
    "shadow_depth": (TS.test_refusals_launch_nothing,
                     ["NULL argument"] * 2 + ["numViews must be 1..64"] * 2 + [_V + "depth is NULL"] + [_V + "dim must be 1..8192"] * 2 +
                     [_V + "pitchBytes below 4 * dim or not a multiple of 4"] * 2 + [_V + "numDraws < 0, or draws is NULL"] * 2 + [_V + "linearDepth must be 0 or 1"] +
                     [_D + _NULL_DRAW] * 3 + [_D + "matWorld is NULL in a linear-depth view", _D + "indexBits must be 16 or 32", _D + "numIndices is not a multiple of 3"] +
                     [_D + _STRIDE12] * 2 + [_D + "numInstances must be 1..128"] * 2 + [_D + "unknown cullMode"] +
                     ["workBytes below vqhip_shadow_depth_work_bytes(the call's instanced triangles, numViews)", "work must be 256-byte aligned",
                      _V + "depth overlaps the work buffer"]),
    "scene_depth": (TD.test_refusals_launch_nothing,
                    ["numDraws < 0, or draws is NULL"] + [_SCENE_NULL] * 3 + ["numDraws < 0, or draws is NULL"] + ["samples must be 1 or 4"] * 3 +
                    ["layers are defined at samples == 4 only"] + ["layers must be 0..4"] * 2 + [_SIZE] * 4 + ["a pitch below width", "negative pitch", "a pitch below width"] +
                    [_SCENE_ALIGN] * 2 + ["reserved must be 0"] + ["draw 0: " + _NULL_DRAW] * 3 + ["draw 0: indexBits must be 16 or 32", "draw 0: numIndices is not a multiple of 3"] +
                    ["draw 0: " + _STRIDE12] * 2 + ["draw 0: numInstances must be 1..64"] * 2 + ["draw 0: unknown cullMode"] +
                    ["workBytes below vqhip_scene_depth_work_bytes(the call's instanced triangles)", "work must be 256-byte aligned", "an output overlaps the work buffer"]),
    "scene_interpolants": (TI.test_refusals_launch_nothing,
                           ["numDraws < 0, or draws is NULL"] + [_IP_NULL] * 6 + ["numDraws < 0, or draws is NULL"] + ["svPositionCurr and svPositionPrev: both or neither"] * 2 +
                           ["draw 0: matWorldViewProjPrev is NULL while the sv planes are asked for"] + [_IP_NULL_DRAW] * 5 + [_SIZE] * 4 +
                           ["a pitch below width", "negative pitch"] * 3 + ["a target is not 16-byte aligned"] * 2 + ["owner must be 4-byte aligned"] +
                           ["draw 0: strideBytes below 44 or not a multiple of 4"] * 3 + ["draw 0: indexBits must be 16 or 32", "draw 0: numIndices is not a multiple of 3"] +
                           ["draw 0: numInstances must be 1..64"] * 2 + ["draw 0: materialIndex is negative"] + [_IP_MISALIGNED] * 5 +
                           ["workBytes below vqhip_scene_interpolants_work_bytes(numDraws)", "work must be 256-byte aligned", "an output overlaps the work buffer",
                            # ip2 on the owner plane: its 16-byte pixels reach far past the 4-byte owner plane; where the allocator put the work buffer behind it, that check comes first
                            (_OWNER, "an output overlaps the work buffer"), _OWNER]),
    "scene_masked_depth": (TM.test_scene_refusals_launch_nothing,
                           ["draw 1: " + _MASK_STRIDE] * 2 + ["draw 1: " + _MASK_SIZE] * 4 + ["draw 1: " + _MASK_MIPS] * 2 + ["draw 1: " + _MASK_TEXELS] +
                           ["workBytes below vqhip_scene_masked_depth_work_bytes(the call's instanced and masked instanced triangles, numDraws)"] * 2 +
                           ["samples must be 1 or 4", "draw 1: numInstances must be 1..64"]),
    "shadow_masked_depth": (TM.test_shadow_refusals_launch_nothing,
                            ["view 0 draw 1: " + _MASK_STRIDE] + ["view 0 draw 1: " + _MASK_SIZE] * 2 + ["view 0 draw 1: " + _MASK_MIPS] * 2 + ["view 0 draw 1: " + _MASK_TEXELS] +
                            ["workBytes below vqhip_shadow_masked_depth_work_bytes(the call's instanced and masked instanced triangles, numViews, the views' draws)",
                             _V + "dim must be 1..8192"]),
}


@pytest.mark.parametrize("who", sorted(REFUSALS))
def test_refusals_say_what_they_said(ctx, who):
    test, want = REFUSALS[who]
    said = []
    test(_Listening(ctx, said))
    assert len(said) == len(want), f"{who}: the refusal test asked for {len(said)} messages, {len(want)} are listed here"
    for k, (got, text) in enumerate(zip(said, want)):
        assert got in [f"{who}: {t}" for t in (text if isinstance(text, tuple) else (text,))], f"{who}: refusal {k} of the test's cases"
