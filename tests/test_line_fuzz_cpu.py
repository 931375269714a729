"""What the fixed-seed slice of tests/test_gpu_line_fuzz.py reaches, counted without a GPU (tests/fuzz/fuzz_lines.class_stats): every corner and edge class of a
diamond, the centre and the gap as the snapped end of a line that reaches the fill; every clip plane cutting a line; both kinds of draw; every class of dropped
line; line counts on both sides of the fill's 256-line scan chunk; both tile sizes, both index widths, frames of one pixel and of partial tiles."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz"))
import fuzz_lines as Z  # noqa: E402

from tests import line_ref as L  # noqa: E402


def test_the_slice_reaches_every_class():
    cases = [Z.case(s) for s in Z.slice_seeds()]
    stats = [Z.class_stats(c) for c in cases]
    ends = {k: sum(s["ends"][k] for s in stats) for k in Z.END_OFFSETS}
    print("fuzz_lines slice:", {"ends": ends, "kinds": {k: sum(s["kinds"][k] for s in stats) for k in ("wireframe", "axes")},
                                "cut_by_plane": [sum(s["cut_by_plane"][p] for s in stats) for p in range(7)],
                                "fragments": sum(s["fragments"] for s in stats)})
    for k, n in ends.items():
        assert n >= 5, f"fewer than five line ends on `{k}` reach the fill"
    for p in range(7):
        assert sum(s["cut_by_plane"][p] for s in stats) >= 3, f"clip plane {p} cuts fewer than three lines"
    for k in ("wireframe", "axes"):
        assert sum(1 for s in stats if s["kinds"][k]) >= 5, k
    for k in ("nonfinite", "bad_index", "zero_length", "clipped_away"):
        assert sum(s[k] for s in stats) >= 5, k
    assert sum(s["fragments"] for s in stats) > 5000 and sum(s["written"] for s in stats) > 2000
    totals = {L.total_lines(c["scene"]) for c in cases}
    assert any(t % 256 == 255 for t in totals) and any(t % 256 == 0 for t in totals) and any(t % 256 == 1 for t in totals), sorted(totals)
    assert {c["tile"] for c in cases} == {32, 64} and {c["bits"] for c in cases} == {16, 32}
    assert any(c["width"] == 1 or c["height"] == 1 for c in cases) and any(c["width"] > 64 for c in cases)
    assert any((c["scene"]["depth"] == 0.0).any() for c in cases) and any((c["scene"]["depth"] == 1.0).all() for c in cases)


def test_a_case_is_a_function_of_its_seed():
    a, b = Z.case(Z.SLICE_FIRST + 3), Z.case(Z.SLICE_FIRST + 3)
    assert Z.describe(a) == Z.describe(b) and len(a["scene"]["draws"]) == len(b["scene"]["draws"])
    for da, db in zip(a["scene"]["draws"], b["scene"]["draws"]):
        assert da["kind"] == db["kind"] and da["vertices"].tobytes() == db["vertices"].tobytes() and da["indices"].tobytes() == db["indices"].tobytes()
