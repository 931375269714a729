"""-m gpu: a slice of the randomised parity run of tests/fuzz/fuzz_lines.py over vqhip_line_draws: SLICE_CASES cases from SLICE_FIRST on, each with its own
frame, tile size, index width, pitch, draw kinds, generator mix (lattice, clip, hostile, soup) and line-count target, scene colour and writer bit for bit
against tests/line_ref.py. tests/test_line_fuzz_cpu.py shows without a GPU what this slice reaches (every corner and edge class as a line's end, every clip
plane, both kinds, every dropped class, the scan's chunk boundary). The long run is the script itself, and the seeds that ever failed in one are replayed here."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz"))
import fuzz_lines as Z  # noqa: E402

pytestmark = pytest.mark.gpu

REPLAYED_SEEDS = ()              # seeds of `python tests/fuzz/fuzz_lines.py` runs that ever differed (none so far)


def _failures(ctx, seeds):
    bad = []
    for seed in seeds:
        n, idx, what = Z.run_case(ctx, seed)
        if n:
            bad.append(f"{what}: {n} elements differ")
    return bad


def test_fuzz_slice(ctx):
    bad = _failures(ctx, Z.slice_seeds())
    assert not bad, "\n".join(bad)


def test_replayed_seeds(ctx):
    bad = _failures(ctx, REPLAYED_SEEDS)
    assert not bad, "\n".join(bad)
