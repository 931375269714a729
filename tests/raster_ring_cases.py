"""Many small draws: scenes whose job tables cross the context's constant-ring slots (tests/test_gpu_raster_front_ends.py), in the dict form every rasteriser's
statement reads (tests/shadow_raster_ref.py, scene_depth_ref.py, masked_depth_ref.py)."""
import numpy as np

from tests import shadow_raster_cases as K

F = np.float32
RING_SLOT_BYTES = 44544                         # kConstSlotBytes of vqengine_amd/csrc/vq_internal.h: what one ring slot holds of a staged host table


def slot_crossing_draws(n, seed, mask_of=None):
    """n draws of one triangle and one instance each: the engine's vertex (stride 44: position, six floats nobody reads, uv in 0 .. 2), the triangle a few
    texels wide at a random place and depth of the map, index width and cull mode alternating, the matrix a uniform scale of 1, 2 or 3 (the same NDC triangle;
    the world positions differ). mask_of(k) -> the `mask` of draw k for the alpha-tested statements, or None."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        v = np.zeros((3, 11), dtype=F)
        v[:, :2] = rng.uniform(-0.9, 0.9, 2)[None, :] + rng.uniform(-0.18, 0.18, (3, 2))
        v[:, 2] = rng.uniform(0.1, 0.9, 3)
        v[:, 3:9] = rng.uniform(-1, 1, (3, 6))
        v[:, 9:11] = rng.uniform(0, 2, (3, 2))
        m = (np.eye(4, dtype=F) * F(1 + k % 3))[None]
        d = {"positions": v, "indices": np.array([0, 1, 2], dtype=np.int64), "wvp": m, "world": m, "cull": K.BACK if k % 5 == 4 else K.NONE,
             "bits": 16 if k % 2 else 32, "stride": 44}
        if mask_of is not None:
            d["mask"] = mask_of(k)
        out.append(d)
    return out
