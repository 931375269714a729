#!/usr/bin/env python3
"""Randomised parity of vqhip_line_draws: python tests/fuzz/fuzz_lines.py [--seconds 120] [--seed 1] (needs a GPU; tests/line_ref.py is the checker).

Every case draws from its seed a frame (sizes from DIMS: one tile, a tile edge on the frame's edge, one pixel past it, partial tiles both ways at both tile
sizes), the raster_tile option, the index width, 1 .. 5 draws of both kinds in a shuffled order, a depth plane (cleared, or patterned with NaN, 0 and 1) and a
MIX of line generators aimed at what the seeded scenes of the GPU tests hold only a few of:
  lattice   ends ON pixel centres, the four corners and the four edges of diamonds, pixel corners (the gap between diamonds) — written as NDC so that the snap
            recovers the point —, horizontal, vertical and slope +-1 lines among them, lines shorter than a diamond, zero-length lines, both directions
  clip      a perspective matrix and ends on either side of w = 0, z = 0, z = w and the four side planes, and exactly ON z == 0 and z == w
  hostile   NaN, +-inf and 1e30 positions, indices past the vertex buffer (0xFFFF at 16 bits), zero normals and tangents in axes draws
  soup      plain random lines, for contrast
and a COUNTING target: filler lines bring the call's line count (the fill's scan length) to one of LINE_TARGETS: multiples of three on both sides of the 256-line scan chunk's multiples (255, 768 and 513 are a chunk - 1, exact and + 1).
Scene colour and writer must equal the statement bit for bit, through the `run` helper of tests/test_gpu_line_draws.py (prefilled sentinel outputs, the
recognisable scene-colour prefill). Prints one line per failure — seed, frame, options, mix; --replay SEED runs that case again — and a summary; exit status 1 if
any case differed. tests/test_line_fuzz_cpu.py pins the generator (what the slice of tests/test_gpu_line_fuzz.py reaches); class_stats(case) counts it."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import line_cases as LC  # noqa: E402
from tests import line_ref as L  # noqa: E402
from vqengine_amd import shadow_scene as S  # noqa: E402

F = np.float32
DIMS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 96, 97, 129)
GENERATORS = ("lattice", "clip", "hostile", "soup")
LINE_TARGETS = (255, 258, 510, 513, 765, 768, 771)     # every draw has a multiple of three lines: 255 = a chunk - 1, 768 = three chunks, 513 = two chunks + 1
END_OFFSETS = {"centre": (0, 0), "top": (0, -128), "bottom": (0, 128), "left": (-128, 0), "right": (128, 0), "upper_left": (-64, -64), "upper_right": (64, -64),
               "lower_left": (-64, 64), "lower_right": (64, 64), "gap": (128, 128)}
BAD_POSITIONS = (np.nan, np.inf, -np.inf, 1e30, -1e30)
SLICE_FIRST, SLICE_CASES = 9000001, 40           # the slice of tests/test_gpu_line_fuzz.py, which tests/test_line_fuzz_cpu.py measures


def slice_seeds(first=SLICE_FIRST, cases=SLICE_CASES):
    return [first + k for k in range(cases)]


def gen_lattice(r, n, W, H):
    """n directed lines (x0, y0, x1, y1) on the snapped grid whose ends lie on named points of diamonds"""
    names = list(END_OFFSETS)
    out = []
    for _ in range(n):
        i, j = int(r.integers(0, W)), int(r.integers(0, H))
        a = END_OFFSETS[names[int(r.integers(len(names)))]]
        x0, y0 = 256 * i + 128 + a[0], 256 * j + 128 + a[1]
        kind = int(r.integers(6))
        if kind == 0:                                                       # zero length
            x1, y1 = x0, y0
        elif kind == 1:                                                     # shorter than a diamond
            x1, y1 = x0 + int(r.integers(-200, 201)), y0 + int(r.integers(-200, 201))
        elif kind == 2:                                                     # horizontal, vertical or slope +-1, whole or half pixels long
            dx, dy = LC.DIRECTIONS[int(r.integers(8))]
            step = 128 * int(r.integers(1, 12))
            x1, y1 = x0 + dx * step, y0 + dy * step
        else:                                                               # to another named point
            b = END_OFFSETS[names[int(r.integers(len(names)))]]
            x1, y1 = 256 * int(r.integers(0, W)) + 128 + b[0], 256 * int(r.integers(0, H)) + 128 + b[1]
        out.append(tuple(min(max(v, 0), 256 * (W if k % 2 == 0 else H)) for k, v in enumerate((x0, y0, x1, y1))))
    return out


def wire_from_lines(lines, W, H, colour, r):
    return LC.lines_as_wire(lines, W, H, colour, z=(float(r.choice((0.0, 0.25, 0.5, 1.0))), float(r.choice((0.25, 0.5, 0.75, 1.0)))))


def gen_clip(r, n, W, H, colour):
    """triangles in front of, across and behind every plane of a perspective frustum; some vertices exactly on z == 0 and z == w (view z == near, == far)"""
    near, far = 0.5, 8.0
    proj = S.perspective_fov_lh(0.5 * np.pi, W / H, near, far)
    v = (r.random((3 * n, 3)) * (8.0, 8.0, 14.0) - (4.0, 4.0, 4.0)).astype(F)
    pick = r.integers(0, 6, size=3 * n)
    v[pick == 0, 2] = near
    v[pick == 1, 2] = far
    v[pick == 2, 2] = 0.0
    return LC.wire((v, np.arange(3 * n)), proj, colour)


def gen_hostile_wire(r, n, W, H, colour, bits):
    v = np.array([LC.ndc(int(r.integers(0, 256 * W + 1)), int(r.integers(0, 256 * H + 1)), W, H, float(r.random())) for _ in range(3 * n)], dtype=F).reshape(-1, 3)
    idx = np.arange(3 * n)
    for k in r.integers(0, 3 * n, size=max(1, n // 2)):
        v[k, int(r.integers(3))] = BAD_POSITIONS[int(r.integers(len(BAD_POSITIONS)))]
    for k in r.integers(0, 3 * n, size=max(1, n // 3)):
        idx[k] = 0xFFFF if bits == 16 else int(r.choice((3 * n, 3 * n + 7, 2 ** 31 - 1)))
    return LC.wire((v, idx), LC.IDENTITY, colour)


def gen_axes(r, n, W, H, hostile):
    """n points inside the frame with random frames; hostile: zero normals, zero tangents, parallel pairs, a non-finite position, an index past the buffer"""
    v = np.zeros((n, 9), dtype=F)
    for k in range(n):
        v[k, :3] = LC.ndc(int(r.integers(0, 256 * W + 1)), int(r.integers(0, 256 * H + 1)), W, H, float(r.random()))
    v[:, 3:9] = r.standard_normal((n, 6)).astype(F)
    idx = r.integers(0, n, size=n + 2)                                     # repeated indices
    if hostile:
        for k in range(n):
            what = int(r.integers(8))
            if what == 0:
                v[k, 3:6] = 0.0
            elif what == 1:
                v[k, 6:9] = 0.0
            elif what == 2:
                v[k, 6:9] = v[k, 3:6] * F(-3.0)
            elif what == 3:
                v[k, int(r.integers(3))] = BAD_POSITIONS[int(r.integers(len(BAD_POSITIONS)))]
        idx[int(r.integers(len(idx)))] = n + 3
    scale = np.diag([1.0, float(r.choice((1.0, 0.5, 2.0))), float(r.choice((1.0, 3.0))), 1.0])
    size = float(r.choice((0.0, 2.0 / W, 0.1, 0.5, 3.0)))
    return LC.axes(v, idx, np.eye(4), scale, np.eye(4), size)


def case(seed):
    r = np.random.default_rng(int(seed))
    W, H = int(r.choice(DIMS)), int(r.choice(DIMS))
    c = {"seed": int(seed), "width": W, "height": H, "tile": int(r.choice((32, 64))), "bits": int(r.choice((16, 32))), "mix": [], "target": int(r.choice(LINE_TARGETS))}
    draws = []
    for k in range(int(r.integers(1, 6))):
        g = GENERATORS[int(r.integers(len(GENERATORS)))]
        n = int(r.integers(1, 14))
        colour = LC.colour_of(int(r.integers(1000)))
        axes = bool(r.integers(3) == 0) and g in ("hostile", "soup")
        c["mix"].append(g + ("/axes" if axes else ""))
        if axes:
            draws.append(gen_axes(r, n, W, H, g == "hostile"))
        elif g == "lattice":
            draws.append(wire_from_lines(gen_lattice(r, 3 * n, W, H), W, H, colour, r))
        elif g == "clip":
            draws.append(gen_clip(r, n, W, H, colour))
        elif g == "hostile":
            draws.append(gen_hostile_wire(r, n, W, H, colour, c["bits"]))
        else:
            ls = [tuple(int(v) for v in r.integers(0, 256 * np.array([W, H, W, H]) + 1)) for _ in range(3 * n)]
            draws.append(wire_from_lines(ls, W, H, colour, r))
    if c["bits"] == 16:
        draws = [d for d in draws if len(d["vertices"]) < 0xFFFF]
    have = L.total_lines({"draws": draws})
    if have < c["target"]:                                                  # fillers: degenerate triangles of three lines each
        draws.append(wire_from_lines(gen_lattice(r, (c["target"] - have) // 3, W, H), W, H, LC.LIME, r))
    depth = np.ones((H, W), dtype=F)
    if r.integers(2):
        depth = (r.random((H, W)) * 0.8 + 0.2).astype(F)
        flat = depth.reshape(-1)
        m = np.arange(flat.shape[0])
        flat[m % 13 == 5], flat[m % 17 == 3], flat[m % 19 == 7] = np.nan, 0.0, 1.0
    order = r.permutation(len(draws))
    c["scene"] = LC.scene(W, H, [draws[k] for k in order], depth)
    return c


def describe(c):
    return f"seed {c['seed']} {c['width']}x{c['height']} tile {c['tile']} bits {c['bits']} lines {L.total_lines(c['scene'])} mix {','.join(c['mix'])}"


def run_case(ctx, seed):
    """(number of differing elements, first index, description): scene colour and writer whole, bit for bit; sceneDepth unchanged"""
    from tests import test_gpu_line_draws as G
    c = case(seed)
    sc = c["scene"]
    ref = L.line_draws(sc, LC.prefill(sc["width"], sc["height"]))
    ctx.set_option("raster_tile", str(c["tile"]))
    try:
        got = G.run(ctx, sc, pad=int(seed) % 3, bits=c["bits"])
    finally:
        ctx.set_option("raster_tile", None)
    n_bad, first, where = 0, [], ""
    w = sc["width"]
    for k in ("scene_color", "writer"):
        g, e = got[k][:, :w], ref[k]
        bad = np.argwhere(g != e)
        if len(bad) and not n_bad:
            first, where = bad[0].tolist(), f" first in {k} at {bad[0].tolist()}: {g[tuple(bad[0])]:#x} != {e[tuple(bad[0])]:#x}"
        n_bad += len(bad)
    n_bad += int((got["depth"][:, :w].view(np.uint32) != sc["depth"].view(np.uint32)).sum())
    return n_bad, first, describe(c) + where


def end_class(x, y):
    """the name of the point relative to the diamond of the pixel it lies nearest to (END_OFFSETS' names for corners and gap, `edge` names by quadrant), or None"""
    dx, dy = (x % 256) - 128, (y % 256) - 128
    a = abs(dx) + abs(dy)
    if (dx, dy) == (0, 0):
        return "centre"
    if a == 256 or (dx == -128 and dy == -128):
        return "gap"
    if a != 128:
        return None
    if dx == 0:
        return "bottom" if dy > 0 else "top"
    if dy == 0:
        return "right" if dx > 0 else "left"
    return ("lower_" if dy > 0 else "upper_") + ("right" if dx > 0 else "left")


def class_stats(c):
    """what the case reaches, without a GPU: lines per kind, snapped ends per class of END_OFFSETS, cuts per clip plane, dropped lines per cause, fragments"""
    sc = c["scene"]
    st = L.new_stats()
    rec = L.lines(sc, st)
    ends = {k: 0 for k in END_OFFSETS}
    for (x0, y0), (x1, y1) in rec["xy"].tolist():
        for x, y in ((x0, y0), (x1, y1)):
            k = end_class(x, y)
            if k:
                ends[k] += 1
    ends["bottom"], ends["right"] = ends["top"], ends["left"]          # one point: a pixel's bottom corner is the top corner of the pixel below, its right corner the next one's left
    kinds = {"wireframe": 0, "axes": 0}
    for d in sc["draws"]:
        kinds[d["kind"]] += L.total_lines({"draws": [d]})
    out = L.line_draws(sc, LC.prefill(sc["width"], sc["height"]), st)
    return {"ends": ends, "kinds": kinds, "cut_by_plane": st["cut_by_plane"], "nonfinite": st["nonfinite"], "bad_index": st["bad_index"], "zero_length": st["zero_length"],
            "clipped_away": st["clipped_away"], "lines": st["lines"], "records": st["records"], "fragments": int(st["fragments"].sum()),
            "written": int((out["writer"] != L.NO_WRITER).sum())}


def main():
    import torch  # noqa: F401
    from vqengine_amd import capi
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=120.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--cases", type=int, default=0, help="stop after this many cases (0: by time)")
    ap.add_argument("--replay", type=int, nargs="*", default=[], help="run exactly these case seeds (the `seed N` of a MISMATCH line) and stop")
    a = ap.parse_args()
    ctx = capi.Context(0)
    t0, n, fails = time.time(), 0, []
    while n < len(a.replay) if a.replay else ((a.cases and n < a.cases) or (not a.cases and time.time() - t0 < a.seconds)):
        seed = a.replay[n] if a.replay else a.seed * 1000003 + n
        bad, _, what = run_case(ctx, seed)
        if bad:
            fails.append(seed)
            print(f"MISMATCH {what}: {bad} elements", flush=True)
        n += 1
        if n % 100 == 0:
            print(f"fuzz_lines: {n} cases so far, {len(fails)} failed", flush=True)
    print(f"fuzz_lines: {n} cases, {len(fails)} failed {fails[:20]}", flush=True)
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    main()
