"""vqhip_shadow_depth and vqhip_scene_depth on one mesh where their contracts coincide: the two rasterisers share one device core (vq_raster.h;
docs/DESIGN_DETAILS.md §7.16), so the shadow map and the scene's depth plane are the same bits — and both are the statement's, which
tests/test_raster_cross_cpu.py shows to agree on this input."""
import numpy as np
import pytest
import torch

from tests import oracle_lib as O
from tests import raster_cross_cases as X
from vqengine_amd import capi

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_draw(d):
    idx = d["indices"]
    ix = dev(idx.astype(np.uint16).view(np.int16)) if d["bits"] == 16 else dev(idx.astype(np.int32))
    return capi.ShadowDraw(dev(d["positions"]), ix, dev(d["wvp"]), None, d["cull"])


def assert_same(name, got, ref):
    n_bad, idx = O.bits_equal(np.asarray(got), np.asarray(ref))
    assert n_bad == 0, f"{name}: {n_bad} of {np.asarray(ref).size} texels differ from the statement, first at {idx.tolist()}"


@pytest.mark.parametrize("bits", (16, 32))
def test_shadow_and_scene_depth_agree_where_the_contracts_coincide(ctx, set_opt, bits):
    """tests/raster_cross_cases.py's soup (0 < z < w at every vertex; the w plane and the side planes cut it) through both entry points at dim 96, 1 sample,
    cull NONE, z / w, at both raster tiles (3 x 3 full tiles; 2 x 2 with partial edge tiles), with 16- and 32-bit indices"""
    view, scene, shadow, out, _ = X.expected(bits)
    dim = X.DIM
    for tile in (64, 32):
        set_opt("raster_tile", tile)
        smap = torch.full((dim, dim), SENTINEL, dtype=torch.float32, device="cuda")
        ctx.shadow_depth([capi.ShadowView(smap, [device_draw(d) for d in view["draws"]], view["linear"], view["camera"], view["far"])])
        depth = torch.full((dim, dim), SENTINEL, dtype=torch.float32, device="cuda")
        primitive = torch.full((dim, dim), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        ctx.scene_depth([device_draw(d) for d in scene["draws"]], dim, dim, 1, primitive=True, layers=0, out={"depth": depth, "primitive": primitive})
        torch.cuda.synchronize()
        got_shadow, got_scene = smap.cpu().numpy(), depth.cpu().numpy()
        assert np.array_equal(got_shadow.view(np.uint32), got_scene.view(np.uint32)), f"tile {tile}: the shadow map and the scene's depth plane differ"
        assert_same(f"tile {tile} shadow map", got_shadow, shadow)
        assert_same(f"tile {tile} scene depth", got_scene, out["depth"])
        assert np.array_equal(primitive.cpu().numpy().view(np.uint32), out["primitive"]), f"tile {tile}: the scene's primitive plane differs from the statement"
