"""No GPU: what tests/fuzz/fuzz_raster.py generates. The generator is deterministic; the slice tests/test_gpu_raster_fuzz.py runs holds every class the fuzzer is
aimed at — counted from the statements' own statistics and printed (run with -v -s to read them) —; and on a dozen cases per pass the vectorised statement equals
the scalar transcriptions of tests/test_scene_depth_cpu.py and tests/test_shadow_raster_cpu.py, so that the GPU is judged by a statement that was itself checked on
these inputs. The thresholds are conditions on the generator, not measurements of a kernel."""
import os
import sys

import numpy as np
import pytest

from tests import scene_depth_ref as V
from tests import shadow_raster_ref as R
from tests import unlit_ref as UR
from tests.test_scene_depth_cpu import scalar_scene
from tests.test_shadow_raster_cpu import scalar_view

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz"))
import fuzz_raster as Z  # noqa: E402

F = np.float32
SCALAR_CASES = 12
SCALAR_AREA = 400                # pixels of a frame the scalar transcription walks in seconds: 3 x 129, 2 x 97, ... (a third of the frames drawn)
SCALAR_DIM = 33                  # ... and the largest shadow view


def test_case_is_deterministic():
    for seed in range(Z.SLICE_FIRST, Z.SLICE_FIRST + 2 * len(Z.PASSES)):
        a, b = Z.case(seed), Z.case(seed)
        assert Z.describe(a) == Z.describe(b) and a["pass"] == Z.pass_of(seed)
        xa, xb = Z.arrays(a), Z.arrays(b)
        assert sorted(xa) == sorted(xb) and len(xa) >= 3
        for k in xa:
            assert xa[k].dtype == xb[k].dtype and xa[k].shape == xb[k].shape and xa[k].tobytes() == xb[k].tobytes(), (seed, k)
    assert Z.describe(Z.case(Z.SLICE_FIRST)) != Z.describe(Z.case(Z.SLICE_FIRST + len(Z.PASSES)))


def test_the_fixed_enclosing_triangles_keep_their_fans():
    """ENCLOSING_FIXED[0]: six planes cut it and nine vertices are left, a fan of 7, the most a triangle in general position can have (three edges of its own
    and six of the clip volume; the tenth vertex needs the w plane to meet the volume, which it does only at the apex). [1]: the four sides leave seven."""
    tri = np.array(Z.ENCLOSING_FIXED, dtype=F)
    clip = R.mul_point(tri, Z.IDENTITY).astype(F)
    poly, cut = V.clip_polygon(clip[0])
    assert poly.shape[0] == 9 and cut == [1, 2, 3, 4, 5, 6]
    poly, cut = R.clip_polygon(np.concatenate([clip[1], np.zeros((3, 3), dtype=F)], axis=1))
    assert poly.shape[0] == 7 and cut == 4


@pytest.mark.parametrize("pas", Z.PASSES)
def test_slice_reaches_every_class(pas):
    """over exactly the seeds of the GPU slice of this pass"""
    shadow, outline, unlit = pas == "shadow_depth", pas == "outline", pas.startswith("unlit")
    planes = 5 if shadow else 7
    total = {k: 0 for k in ("triangles", "records", "nonfinite", "bad_index", "unsnappable", "zero_area", "culled", "no_sample", "edge_zero")}
    cut, most_planes, max_fan = [0] * planes, 0, 0
    landed, tiles, widths, culls, dims, mixes = set(), set(), set(), set(), set(), set()
    for seed in Z.slice_seeds(pas):
        c = Z.case(seed)
        st = Z.class_stats(c)
        for k in total:
            total[k] += st[k]
        cut = [a + b for a, b in zip(cut, st["cut_by_plane"])]
        most_planes, max_fan = max(most_planes, st["most_planes"]), max(max_fan, st["max_fan"])
        kind, target = c["target"]
        if st[kind] == target:
            landed.add((kind, target))
        tiles.add(c["tile"])
        widths |= set(c["bits"]) if isinstance(c["bits"], tuple) else {c["bits"]}
        culls |= set() if outline else set(sum(c["culls"], []) if shadow else c["culls"])       # the outline has no cull mode
        dims |= set(c["dims"]) if shadow else {c["width"], c["height"]}
        mixes |= {g for view in (c["mix"] if shadow else [c["mix"]]) for d in view for g in d}
    print(f"\n{pas}: {Z.SLICE_CASES} cases from seed {Z.slice_seeds(pas)[0]}: {total} cut_by_plane {cut} most planes through one triangle {most_planes} largest fan {max_fan} "
          f"targets hit {sorted(landed)}")
    assert total["edge_zero"] >= 500, "covered samples with an edge exactly through them"
    for k in ("nonfinite", "bad_index", "unsnappable", "zero_area", "no_sample") + (() if outline else ("culled",)):      # the outline has no cull mode
        assert total[k] >= 1, k
    assert all(n >= 1 for n in cut), cut
    if shadow:
        # five planes, and a fan of 5: the four sides leave at most 3 + 4 vertices, and the w plane adds none — it meets the volume |x|, |y| <= w at its apex only
        assert most_planes == 5 and max_fan >= 5
    else:
        assert most_planes >= 6 and max_fan >= 6
    want = set(Z.UNLIT_TARGETS) if unlit else {("records", n) for n in Z.RECORD_TARGETS}
    assert landed >= want, sorted(want - landed)
    assert tiles == {32, 64} and widths == {16, 32} and dims == set(Z.DIMS), (tiles, widths, sorted(dims))
    assert outline or culls == {0, 1, 2}
    assert mixes >= set(Z.GENERATORS)


def _small(pas, want=SCALAR_CASES):
    """the first cases of the pass, from the slice's first seed on, whose frames the scalar transcription walks in seconds"""
    out, k = [], 0
    while len(out) < want:
        seed = Z.slice_seeds(pas, cases=k + 1)[k]
        k += 1
        c = Z.case(seed)
        if (max(c["dims"]) <= SCALAR_DIM) if pas == "shadow_depth" else (c["width"] * c["height"] <= SCALAR_AREA):
            out.append(c)
    return out


@pytest.mark.parametrize("pas", Z.PASSES)
def test_statement_equals_the_scalar_transcription(pas):
    """shadow views whole; the scene passes' depth and primitive; of the outline its mark pass and of the unlit draws their setup and V5's depth, as scenes of
    tests/scene_depth_ref.py (what these two statements add on top — the colour, the fold — has its own pins in tests/test_outline_cpu.py and
    tests/test_unlit_draws_cpu.py)"""
    triangles = 0
    for c in _small(pas):
        if pas == "shadow_depth":
            for v, view in enumerate(c["views"]):
                got, want = R.rasterize_view(view), scalar_view(view)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{Z.describe(c)}: view {v}"
                triangles += sum(len(d["indices"]) // 3 for d in view["draws"])
            continue
        sc = c["scene"]
        scene = Z.outline_mark_scene(sc) if pas == "outline" else UR.depth_scene(sc) if pas.startswith("unlit") else sc
        depth, prim = V.fill(V.setup(scene), scene)
        sdepth, sprim = scalar_scene(scene)
        assert np.array_equal(depth.view(np.uint32), sdepth.view(np.uint32)) and np.array_equal(prim, sprim), Z.describe(c)
        triangles += V.instanced_triangles(scene)
    assert triangles > 1000
