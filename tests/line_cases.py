"""The seeded lines and scenes both vqhip_line_draws test files use (tests/test_line_draws_cpu.py, tests/test_gpu_line_draws.py), in the form tests/line_ref.py
reads. Frames are 16 x 16 (one tile), 64 x 40 (several tiles) and 129 x 67 (a partial last tile on both axes, odd last column and row). The adversarial lines are
given on the snapped grid (1/256 of a pixel) inside a cell of 8 x 8 pixels around the centre C of the cell's pixel (4, 4); a scene spreads them over the cells of
its frame, one line per cell and draw, so that a line's pixels are its own. Expectations are computed once per process and shared read-only."""
import functools

import numpy as np

from tests import line_ref as L
from tests import unlit_cases as UC
from vqengine_amd import line_scene as LS
from vqengine_amd import shadow_scene as S

F = np.float32
SIZES = UC.SIZES
CELL = 8                                          # pixels
C0 = 4 * 256 + 128                                # the centre of pixel (4, 4), on both axes
RED, TEAL, AMBER, LIME = (0.9, 0.2, 0.1, 0.45), (0.1, 0.7, 0.8, 0.25), (1.0, 0.6, 0.05, 1.0), (0.3, 1.5, 0.2, 0.0)
IDENTITY = np.eye(4, dtype=F)
CORNERS = {"top": (0, -128), "bottom": (0, 128), "left": (-128, 0), "right": (128, 0)}
EDGES = {"upper_left": (-64, -64), "upper_right": (64, -64), "lower_left": (-64, 64), "lower_right": (64, 64)}
DIRECTIONS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1))


@functools.lru_cache(maxsize=None)
def adversarial_lines(seed=11):
    """(x0, y0, x1, y1) relative to the cell's corner, every line with its reverse: the list of docs/DESIGN_DETAILS.md §7.24's test plan, then a seeded set"""
    out = []
    far = ((768, 256), (256, 768), (-768, -256), (-256, 700), (640, -640), (-512, -512), (700, 0), (0, -700))
    for dx, dy in DIRECTIONS:                                              # horizontal, vertical, slope exactly +-1: centre to centre, and off the centres
        out.append((C0, C0, C0 + 768 * dx, C0 + 768 * dy))
        out.append((C0 + 37, C0 - 90, C0 + 37 + 700 * dx, C0 - 90 + 700 * dy))
    for ox, oy in list(CORNERS.values()) + list(EDGES.values()) + [(128, 128), (-128, 128), (100, 100), (-90, -110), (127, 0), (0, 127), (1, 127), (-1, 127)]:
        for fx, fy in far:                                                 # an end on a corner, on an edge, in the gap between diamonds
            out.append((C0 + ox, C0 + oy, C0 + ox + fx, C0 + oy + fy))
    for ox, oy in EDGES.values():                                          # along each edge of the diamond (slope exactly +-1), ending on corners and beyond
        tx, ty = (oy // 64) * 64, -(ox // 64) * 64                         # the edge's direction
        for a, b in ((-1, 1), (-3, 3), (-1, 5), (0, 1), (-1, 0)):
            out.append((C0 + ox + a * tx, C0 + oy + a * ty, C0 + ox + b * tx, C0 + oy + b * ty))
    out += [(C0 - 20, C0 - 10, C0 + 30, C0 + 5), (C0 - 20, C0 - 10, C0 + 200, C0 + 40), (C0 - 100, C0 - 60, C0 + 100, C0 + 60), (C0 + 100, C0 + 90, C0 + 150, C0 + 120),
            (C0 - 5, C0 + 100, C0 + 5, C0 + 140), (C0 + 120, C0 - 3, C0 + 140, C0 + 3), (C0, C0 + 128, C0 + 1, C0 + 128), (C0 + 128, C0, C0 + 128, C0 + 1),
            (C0 - 30, C0 - 20, C0 + 10, C0 + 118), (C0 + 3, C0 - 40, C0 + 3, C0 + 40), (C0, C0, C0, C0), (C0 + 128, C0 + 128, C0 + 128, C0 + 128)]     # short lines, zero length
    out += [(C0 - 300, C0 + 128, C0 + 300, C0 + 128), (C0 + 128, C0 - 300, C0 + 128, C0 + 300),                  # through bottom corners only; through right corners only
            (C0 - 72, C0 - 100, C0 + 328, C0 + 100), (C0 - 100, C0 + 28, C0 + 100, C0 + 228), (C0 + 28, C0 - 100, C0 + 228, C0 + 100)]
    rng = np.random.default_rng(seed)
    for k in range(260):
        p = rng.integers(256, 7 * 256, size=4)
        if k % 3 == 0:
            p = (p // 64) * 64
        elif k % 3 == 1:
            p = (p // 128) * 128
        if k % 5 == 0:
            p[2:] = p[:2] + rng.integers(-200, 201, size=2)                # shorter than a diamond
        out.append(tuple(int(v) for v in p))
    out = [tuple(int(v) for v in l) for l in out]
    assert all(0 <= v <= CELL * 256 for l in out for v in l)
    return tuple(out + [(x1, y1, x0, y0) for (x0, y0, x1, y1) in out])


def cells(w, h):
    return [(cx, cy) for cy in range(h // CELL) for cx in range(w // CELL)]


def placed_lines(w, h):
    """the adversarial lines over the frame's cells: a list of layers (one draw each), each a list of absolute (x0, y0, x1, y1)"""
    cs = cells(w, h)
    lines = adversarial_lines()
    layers = []
    for k, (x0, y0, x1, y1) in enumerate(lines):
        if k % len(cs) == 0:
            layers.append([])
        ox, oy = (256 * CELL * c for c in cs[k % len(cs)])
        layers[-1].append((x0 + ox, y0 + oy, x1 + ox, y1 + oy))
    return layers


def ndc(sx, sy, w, h, z=0.5):
    """the clip-space position (w = 1, identity matrix) that V3 snaps to (sx, sy)"""
    return (sx / (128.0 * w) - 1.0, 1.0 - sy / (128.0 * h), z)


def wire(mesh, matrices, color):
    return {"kind": "wireframe", "vertices": np.ascontiguousarray(mesh[0], dtype=F), "indices": np.asarray(mesh[1], dtype=np.int64),
            "matrices": np.ascontiguousarray(np.asarray(matrices, dtype=np.float64).reshape(-1, 4, 4).astype(F)), "color": np.asarray(color, dtype=F)}


def axes(vertices, indices, world, normal, view_proj, size):
    return {"kind": "axes", "vertices": np.ascontiguousarray(vertices, dtype=F), "indices": np.asarray(indices, dtype=np.int64),
            "cb": LS.vertex_axes_data(world, normal, view_proj, size)}


def lines_as_wire(lines, w, h, color, z=(0.3, 0.7)):
    """directed lines as degenerate triangles (a, b, a vertex without a finite position): L1 drops b->n and n->a, a->b remains, alone"""
    v = [ndc(x, y, w, h, z[k % 2]) for (x0, y0, x1, y1) in lines for k, (x, y) in enumerate(((x0, y0), (x1, y1)))] + [(np.nan, 0.0, 0.5)]
    n = len(lines)
    idx = np.stack([2 * np.arange(n), 2 * np.arange(n) + 1, np.full(n, 2 * n)], axis=1).reshape(-1)
    return wire((np.array(v, dtype=F), idx), IDENTITY, color)


def line_as_axes(line, w, h):
    """one point at the line's start whose tangent axis is the line (to the precision of the vertex stage), the other two axes short"""
    x0, y0, x1, y1 = line
    a, b = np.array(ndc(x0, y0, w, h, 0.4)), np.array(ndc(x1, y1, w, h, 0.4))
    t = b - a
    size = float(np.linalg.norm(t))
    if size == 0.0:
        t = np.array([1.0, 0.0, 0.0])
    n = np.array([0.0, 0.0, 1.0])
    return axes(np.concatenate([a, n, t])[None, :], [0], IDENTITY, IDENTITY, IDENTITY, size)


def scene(w, h, draws, depth=None, **extra):
    return UC.scene(w, h, draws, depth, **extra)


def colour_of(k):
    rng = np.random.default_rng(1000 + k)
    return tuple(rng.random(3) * 2.0) + (float(k % 3) * 0.5,)


def adversarial_wire(w, h):
    return scene(w, h, [lines_as_wire(layer, w, h, colour_of(k)) for k, layer in enumerate(placed_lines(w, h))])


def adversarial_axes(w, h):
    """every third adversarial line as the tangent axis of a point of its own, one draw per line (LocalAxisSize is the line's length)"""
    flat = [l for layer in placed_lines(w, h) for l in layer][::3]
    return scene(w, h, [line_as_axes(l, w, h) for l in flat])


def tile_boundaries(w, h):
    """lines along and across x, y = 31 / 32 / 63 / 64 and the frame's last column and row"""
    ls = []
    for e in sorted({31, 32, 63, 64, w - 1, h - 1}):
        for off in (0, 128, 255):
            p = 256 * e + off
            if e < w:
                ls += [(p, 40, p, 256 * h - 40), (p - 300, 256 * (h // 2) + 77, p + 300, 256 * (h // 2) + 130), (p - 250, 100, p + 250, 600)]
            if e < h:
                ls += [(40, p, 256 * w - 40, p), (256 * (w // 2) + 77, p - 300, 256 * (w // 2) + 130, p + 300), (100, p - 250, 600, p + 250)]
    ls += [(0, 0, 256 * w, 256 * h), (256 * w, 0, 0, 256 * h), (0, 256 * h - 128, 256 * w, 256 * h - 128), (256 * w - 128, 0, 256 * w - 128, 256 * h)]
    ls = [tuple(min(max(v, 0), 256 * (w if k % 2 == 0 else h)) for k, v in enumerate(l)) for l in ls]
    return scene(w, h, [lines_as_wire(ls[k::4], w, h, colour_of(k)) for k in range(4)] + [lines_as_wire([(x1, y1, x0, y0) for (x0, y0, x1, y1) in ls], w, h, LIME)])


def cube_instances(w, h, n=512):
    """one cube, 512 instances (the instanced cbuffer at its limit), in front of and behind a rasterised box"""
    rng = np.random.default_rng(21)
    vp = UC.view_proj(w, h)
    mats = [S.scaling(tuple(rng.random(3) * 0.5 + 0.1)) @ S.rotation_y(rng.random() * 6.0) @ S.translation(tuple(rng.random(3) * (6.0, 4.0, 5.0) - (3.0, 2.0, 2.5))) @ vp
            for _ in range(n)]
    return scene(w, h, [wire(LS.CUBE, mats, TEAL)], UC.rasterised_depth(w, h, [UC.box_producer(w, h)]))


def crossing(w, h, swapped=False):
    """two draws of different colours whose lines cross"""
    vp = UC.view_proj(w, h)
    a = wire(S.box((1.5, 1.0, 1.2)), [S.rotation_y(0.5) @ S.rotation_x(0.3) @ vp], RED)
    b = wire(S.uv_sphere(1.3, 8, 6), [S.rotation_x(0.2) @ S.translation((0.2, 0.0, 0.0)) @ vp], AMBER)
    return scene(w, h, [b, a] if swapped else [a, b])


def shared_edge(w, h):
    """two triangles with a shared edge (drawn twice, once in each direction) — and the same pair as two draws"""
    v = np.array([ndc(300, 300, w, h, 0.2), ndc(256 * w - 500, 900, w, h, 0.4), ndc(800, 256 * h - 300, w, h, 0.6), ndc(256 * w - 300, 256 * h - 700, w, h, 0.8)], dtype=F)
    return scene(w, h, [wire((v, [0, 1, 2, 2, 1, 3]), IDENTITY, RED), wire((v, [0, 1, 2]), IDENTITY, TEAL), wire((v, [2, 1, 3]), IDENTITY, AMBER)])


def clip_planes(w, h):
    """lines across w = 0, z = 0, z = w and each side plane; a non-finite position; indices past the buffer"""
    proj = S.perspective_fov_lh(0.5 * np.pi, w / h, 0.25, 8.0)
    v = np.array([[-1.0, -0.5, -2.0], [1.5, -0.3, 20.0], [0.0, 1.0, 3.0], [-9.0, 0.2, 3.0], [9.0, -0.4, 4.0], [0.3, 9.0, 2.0], [-0.2, -9.0, 5.0], [0.1, 0.1, 0.1],
                  [np.inf, 0.0, 2.0], [0.5, np.nan, 2.0], [0.0, 0.0, 1e30], [0.4, 0.3, 0.26], [-0.5, 0.2, 7.9]], dtype=F)
    idx = [0, 1, 2, 3, 4, 2, 5, 6, 2, 7, 1, 3, 8, 2, 4, 9, 5, 6, 10, 11, 12, 11, 12, 2, 0, 13, 1, 2, 3, 99, 4, 5, 6]
    return scene(w, h, [wire((v, idx), proj, RED), wire((v[:, [1, 0, 2]], idx), proj, TEAL)])


def axes_mesh(w, h):
    """a sphere's vertices with normals and tangents: a repeated index, an index past the buffer, a zero normal (its normal and cross axes vanish, the tangent
    axis stays), a zero tangent, a normal parallel to the tangent, under a non-uniform matNormal — and a second draw with LocalAxisSize 0 (nothing drawn)"""
    pos, _ = S.uv_sphere(1.4, 7, 5)
    pos = np.asarray(pos, dtype=F)[:, :3]
    nrm = pos / np.maximum(np.linalg.norm(pos, axis=1, keepdims=True), 1e-9)
    tan = np.cross(nrm, (0.0, 1.0, 0.2))
    v = np.concatenate([pos, nrm, tan], axis=1).astype(F)
    v[3, 3:6] = 0.0
    v[5, 6:9] = 0.0
    v[7, 6:9] = v[7, 3:6] * 2.0
    idx = list(range(len(v))) + [3, 3, 2, len(v) + 5, 0]
    world = S.scaling((1.0, 0.7, 1.2)) @ S.rotation_y(0.4)
    normal = np.linalg.inv(world).T
    vp = UC.view_proj(w, h)
    return scene(w, h, [axes(v, idx, world, normal, vp, 0.6), axes(v, idx, world, normal, vp, 0.0)], UC.rasterised_depth(w, h, [UC.box_producer(w, h)]))


def depth_plane(w, h):
    """a depth plane with NaNs, 0.0 and 1.0 under full-frame lines, and the depth producer's own box drawn as wire over its own depth"""
    rng = np.random.default_rng(5)
    prod = UC.box_producer(w, h)
    depth = UC.rasterised_depth(w, h, [prod]).copy()
    flat = depth.reshape(-1)
    n = np.arange(flat.shape[0])
    flat[n % 29 == 7] = np.nan
    flat[n % 31 == 3] = 0.0
    ls = [tuple(int(v) for v in rng.integers(0, 256 * np.array([w, h, w, h]))) for _ in range(40)]
    own = wire((prod["vertices"], prod["indices"]), prod["cb"][:16].reshape(1, 4, 4), LIME)
    return scene(w, h, [lines_as_wire(ls, w, h, RED, z=(0.1, 0.95)), own], depth, producer=prod)


SOUP_LINES = 256 * 9 + 77


def soup(w, h, seed=7):
    """more than 256 x 9 lines inside the first 32 x 32 tile, from five draws of both kinds, over a patterned depth"""
    rng = np.random.default_rng(seed)
    rw, rh = min(w, 32), min(h, 32)
    draws = []
    per = SOUP_LINES // 4 + 1
    for k in range(4):
        a = rng.integers(30, 256 * np.array([rw, rh]) - 30, size=(per, 2))
        b = np.clip(a + rng.integers(-1500, 1501, size=(per, 2)), 10, 256 * np.array([rw, rh]) - 10)
        draws.append(lines_as_wire([tuple(int(v) for v in (p[0], p[1], q[0], q[1])) for p, q in zip(a, b)], w, h, colour_of(50 + k), z=(0.2 + 0.1 * k, 0.9 - 0.1 * k)))
    v = np.zeros((40, 9), dtype=F)
    for k in range(40):
        v[k, :3] = ndc(int(rng.integers(1400, 256 * rw - 1400)), int(rng.integers(1400, 256 * rh - 1400)), w, h, 0.35)    # the axes are 4 pixels long
    v[:, 3:6], v[:, 6:9] = (0.0, 0.0, 1.0), (1.0, 0.5, 0.0)
    draws.insert(2, axes(v, np.arange(40), IDENTITY, IDENTITY, IDENTITY, 8.0 / w))
    depth = (rng.random((h, w)) * 0.7 + 0.3).astype(F)
    return scene(w, h, draws, depth)


BUILDERS = {"adversarial_wire": adversarial_wire, "adversarial_axes": adversarial_axes, "tile_boundaries": tile_boundaries, "cube_instances": cube_instances,
            "crossing_ab": crossing, "crossing_ba": lambda w, h: crossing(w, h, True), "shared_edge": shared_edge, "clip_planes": clip_planes, "axes_mesh": axes_mesh,
            "depth_plane": depth_plane, "soup": soup}


@functools.lru_cache(maxsize=None)
def case(name):
    base, size = name.rsplit("_", 1)
    w, h = (int(v) for v in size.split("x"))
    return BUILDERS[base](w, h)


def names():
    return [f"{b}_{w}x{h}" for (w, h) in SIZES for b in BUILDERS]


prefill = UC.prefill


@functools.lru_cache(maxsize=None)
def expected(name):
    """the statement's outputs of a case over prefill(w, h), computed once and shared (read-only), with the statistics of the run under `stats`"""
    sc = case(name)
    stats = L.new_stats()
    out = L.line_draws(sc, prefill(sc["width"], sc["height"]), stats)
    for a in out.values():
        a.setflags(write=False)
    out["stats"] = stats
    return out
