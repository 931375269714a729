"""The rasterisers' work-buffer sizes (vqhip_shadow_depth_work_bytes, vqhip_shadow_masked_depth_work_bytes, vqhip_scene_depth_work_bytes,
vqhip_scene_masked_depth_work_bytes) over a grid of arguments, against values recorded once from the library as it was while each rasteriser still had a layout
function of its own (tests/golden/raster_work_bytes.json). Host-only: no context, no device. The grid holds 0, 1 and the limits themselves — 2^29 - 1 and 2^29
triangles (the scene call's record counter), 2^40 and 2^40 + 1 (the shadow call's), 0 / 1 / 64 / 65 views, -1 / 0 / 1 draws, more masked triangles than
triangles — with the arguments for which the functions return 0."""
import itertools
import json
import os

from vqengine_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raster_work_bytes.json")
TRIANGLES = (0, 1, 2, 1000, 12345, 2 ** 20 + 1, 2 ** 29 - 1, 2 ** 29, 2 ** 29 + 1, 2 ** 32, 2 ** 40 - 1, 2 ** 40, 2 ** 40 + 1, 2 ** 63)
VIEWS = (-1, 0, 1, 37, 64, 65)
DRAWS = (-1, 0, 1, 2, 5, 6, 1000, 20000, 2 ** 31 - 1)


def masked_counts(tris):
    """0, 1, half, all, and one more than all"""
    return sorted({0, min(1, tris), tris // 2, tris, tris + 1})


def grid():
    """name -> (function, list of argument tuples)"""
    return {
        "shadow_depth": (capi.shadow_depth_work_bytes, list(itertools.product(TRIANGLES, VIEWS))),
        "scene_depth": (capi.scene_depth_work_bytes, [(t,) for t in TRIANGLES]),
        "shadow_masked_depth": (capi.shadow_masked_depth_work_bytes, [(t, m, v, d) for t in TRIANGLES for m in masked_counts(t) for v in (0, 1, 64, 65) for d in DRAWS]),
        "scene_masked_depth": (capi.scene_masked_depth_work_bytes, [(t, m, d) for t in TRIANGLES for m in masked_counts(t) for d in DRAWS]),
    }


def test_work_sizes_are_the_recorded_ones():
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(grid())
    for name, (fn, args) in grid().items():
        want = golden[name]
        assert [tuple(row[:-1]) for row in want] == args, f"{name}: the fixture was recorded over another grid"
        zeros = 0
        for row in want:
            got = fn(*row[:-1])
            assert got == row[-1], f"vqhip_{name}_work_bytes{tuple(row[:-1])}: {got}, recorded {row[-1]}"
            zeros += got == 0
        assert 0 < zeros < len(want), f"{name}: the grid holds both accepted and refused arguments"
