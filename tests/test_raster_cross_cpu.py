"""The two rasterisers' numpy statements (tests/shadow_raster_ref.py, tests/scene_depth_ref.py) on one mesh where their contracts coincide
(docs/DESIGN_DETAILS.md §7.16: one statement of the rules on the device). This is the condition that keeps tests/test_gpu_raster_cross.py honest."""
import numpy as np
import pytest

from tests import raster_cross_cases as X
from tests import shadow_raster_ref as R

F = np.float32


@pytest.mark.parametrize("bits", (16, 32))
def test_shadow_and_scene_statements_agree_where_the_contracts_coincide(bits):
    """One soup through both statements at a square target, 1 sample, cull NONE, z / w: with 0 < z < w at every clip-space vertex the scene's two extra planes cut
    nothing, planes 0 .. 4, the snap, the fan and the saturate are the same, and the scene's skip of >= 1.0 equals a minimum against the clear value: the shadow
    map and the scene's depth plane are the same bits. The conditions on the input are asserted first."""
    view, scene, shadow, out, stats = X.expected(bits)
    d = view["draws"][0]
    P = d["positions"].copy()
    P[:, 1] = P[:, 1] + F(0.0)
    clip = R.mul_point(P, d["wvp"][0])
    assert (clip[:, 2] > 0).all() and (clip[:, 2] < clip[:, 3]).all(), "the input violates 0 < z < w"
    cut = stats["cut_by_plane"]
    assert cut[0] >= 1 and min(cut[1:5]) >= 1 and cut[5] == 0 and cut[6] == 0, cut         # the w plane and every side plane cut; the z planes do not
    assert sum(stats["clipped"][1:]) >= 20 and stats["records"] >= 100
    assert shadow.shape == out["depth"].shape == (X.DIM, X.DIM)
    covered = shadow.view(np.uint32) != 0x3F800000
    assert covered.sum() >= 500 and not covered.all()
    assert np.array_equal(shadow.view(np.uint32), out["depth"].view(np.uint32)), f"{int((shadow.view(np.uint32) != out['depth'].view(np.uint32)).sum())} texels differ"
    assert np.array_equal(covered, out["primitive"] != 0xFFFFFFFF)
