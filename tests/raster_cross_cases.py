"""The input of the cross test (tests/test_raster_cross_cpu.py, tests/test_gpu_raster_cross.py): one mesh for vqhip_shadow_depth and vqhip_scene_depth where their
contracts coincide — a square target, 1 sample, cull NONE, z / w, and 0 < z < w at every clip-space vertex. Draws and views are tests/shadow_raster_cases.py's
(the scene takes the same draw, as tests/scene_depth_cases.py's do). Expectations are computed once per process and shared read-only."""
import functools

import numpy as np

from tests import scene_depth_cases as SC
from tests import scene_depth_ref as V
from tests import shadow_raster_cases as K
from tests import shadow_raster_ref as R

F = np.float32
DIM = 96                                         # 3 x 3 full tiles at tile 32; 2 x 2 tiles with partial edge tiles at tile 64
# clip = (x, y, 0.5 w + 0.1 x + 0.05 y, w) with w = the position's z: 0 < clip z < w wherever w > 0 and |x|, |y| <= 3 w (0.45 w at the most on either side of
# 0.5 w), at the vertices and — the three quantities being linear — at every vertex the clipper makes. The scene's two z planes then cut nothing.
WVP = np.array([[(1, 0, 0.1, 0), (0, 1, 0.05, 0), (0, 0, 0.5, 1), (0, 0, 0, 0)]], dtype=F)


def soup_draw(bits, n=200, seed=23):
    """an indexed soup of n triangles for both rasterisers at once: centres up to 1.3 from the axis in NDC (many cross a side plane), z / w between 0.05 and
    0.95; every seventh triangle has one vertex at w = 1e-9, below the w plane's 2^-24. The index buffer visits the vertices in a shuffled order."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 4.0, (n, 1, 1)) * rng.uniform(0.8, 1.25, (n, 3, 1))
    ndc = np.clip(rng.uniform(-1.3, 1.3, (n, 1, 2)) + rng.normal(0.0, 0.15, (n, 3, 2)), -2.5, 2.5)
    w[::7, 0, 0] = 1e-9
    pos = np.concatenate([ndc * w, w], axis=2).reshape(-1, 3).astype(F)
    order = rng.permutation(3 * n)                                     # vertex k of the soup lives at order[k]
    shuffled = np.empty_like(pos)
    shuffled[order] = pos
    return K.draw(shuffled, order, WVP, None, K.NONE, bits=bits, stride=12)


@functools.lru_cache(maxsize=None)
def expected(bits):
    """(view, scene, shadow map, scene outputs, scene statistics): both statements on the same draw"""
    d = soup_draw(bits)
    view, scene = K.view(DIM, [d]), SC.scene(DIM, DIM, 1, [d])
    stats = V.new_stats()
    shadow, out = R.rasterize([view])[0], V.rasterize(scene, stats=stats)
    for a in (shadow, out["depth"], out["primitive"]):
        a.setflags(write=False)
    return view, scene, shadow, out, stats
