"""-m gpu: a slice of the randomised parity run of tests/fuzz/fuzz_raster.py over the rasterised fills (vqhip_shadow_depth, vqhip_scene_depth at 1 and 4 samples,
vqhip_outline, vqhip_unlit_draws opaque and blended): per pass SLICE_CASES cases from SLICE_FIRST on, each with its own frame, tile size, index width, stride,
cull modes, generator mix (lattice, enclosing, crossing, hostile, soup) and counting target, every output plane bit for bit against the pass's numpy statement.
tests/test_raster_fuzz_cpu.py shows without a GPU what this slice reaches (per pass: thousands of covered samples with an edge exactly through them, every dropped
class, every clip plane, fans of 7, every counting target) and checks the statement on such inputs against its scalar transcription. The statements of a pass's
slice take 4 .. 9 s on the CPU (profiles/r26a_raster_fuzz.md); the long run is the script itself, and the seeds that ever failed in one are replayed here."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz"))
import fuzz_raster as Z  # noqa: E402

pytestmark = pytest.mark.gpu

REPLAYED_SEEDS = ()              # seeds of `python tests/fuzz/fuzz_raster.py` runs that ever differed (none so far: profiles/r26a_raster_fuzz.md)


def _failures(ctx, seeds):
    bad = []
    for seed in seeds:
        n, idx, what = Z.run_case(ctx, seed)[:3]
        if n:
            bad.append(f"{what}: {n} elements differ")
    return bad


@pytest.mark.parametrize("pas", Z.PASSES)
def test_fuzz_slice(ctx, pas):
    bad = _failures(ctx, Z.slice_seeds(pas))
    assert not bad, "\n".join(bad)


def test_replayed_seeds(ctx):
    bad = _failures(ctx, REPLAYED_SEEDS)
    assert not bad, "\n".join(bad)
