"""What both vqhip_object_ids test files use (tests/test_object_ids_cpu.py, tests/test_gpu_object_ids.py): the id tables of a scene's draws, the ObjectID pass's
chain on tests/scene_depth_cases.py's scenes with every cull mode forced to NONE (the pass ignores iFaceCull), and the hand-made owner planes of rule P0.
Expectations are computed once per process and shared read-only."""
import functools

import numpy as np

from tests import object_ids_ref as P
from tests import scene_depth_cases as SC
from tests import scene_depth_ref as V

SIZES = SC.SIZES


def id_draws(draws, seed=5):
    """one ObjectID table per draw: objID rows of any int32 (negative and large values included; .y and .z, which the pass does not read, are poison), ids that
    tell the draws apart"""
    rng = np.random.default_rng(seed)
    out = []
    for k, d in enumerate(draws):
        n = np.asarray(d["wvp"]).shape[0]
        obj = rng.integers(-2**31, 2**31, size=(n, 4), dtype=np.int64).astype(np.int32)
        obj[:, 1], obj[:, 2] = 0x0BADF00D, -0x0BADF00D
        obj[:, 0] = 1000 * (k + 1) + np.arange(n)                                   # readable: draw and instance
        out.append(P.id_draw(len(d["indices"]), obj, 7 + k, -3 - k if k % 2 else 40 + k))
    return out


def cull_none(scene):
    return dict(scene, draws=[dict(d, cull=V.CULL_NONE) for d in scene["draws"]])


@functools.lru_cache(maxsize=None)
def chain_cases():
    """name -> scene at 1 sample with all cull modes NONE: the instanced boxes (64 instances, 16-bit indices, 44-byte stride) and the room from inside"""
    c = {}
    for w, h in SIZES:
        c[f"boxes_{w}x{h}"] = cull_none(SC.boxes_scene(w, h, 1))
        c[f"room_{w}x{h}"] = cull_none(SC.room_scene(w, h, 1))
    return c


@functools.lru_cache(maxsize=None)
def chain_expected(name):
    """(owner plane of the statement of §7.17 at cull NONE, the id draws, the ids of P0 over that plane)"""
    scene = chain_cases()[name]
    owner = V.rasterize(scene)["primitive"]
    draws = id_draws(scene["draws"])
    ids = P.resolve(draws, owner)
    owner.setflags(write=False); ids.setflags(write=False)
    return owner, draws, ids


@functools.lru_cache(maxsize=None)
def table():
    """the hand-made draw list of the P0 tests: empty draws at the head, in the middle and at the tail; one, three and 64 instances. q: [0, 4) draw 1, [4, 10)
    draw 3 (three instances of two triangles), [10, 74) draw 4 (64 instances of one triangle), [74, 79) draw 6; total 79"""
    rng = np.random.default_rng(21)
    obj = lambda n: rng.integers(-2**31, 2**31, size=(n, 4), dtype=np.int64).astype(np.int32)     # noqa: E731
    return [P.id_draw(0, obj(2), 900, 901), P.id_draw(12, obj(1), 1, -1), P.id_draw(0, obj(1), 902, 903), P.id_draw(6, obj(3), 2, 2**31 - 1),
            P.id_draw(3, obj(64), -2**31, 5), P.id_draw(0, obj(64), 904, 905), P.id_draw(15, obj(1), 6, 7), P.id_draw(0, obj(1), 906, 907)]


TABLE_TOTAL = 79


def owner_planes(w, h, seed=3):
    """name -> uint32 [h, w]: every q at and around each boundary of the table in the first pixels of a plane of no-owner values, the last q of each draw, q = total,
    0xFFFFFFFF, and two random planes: one of owned values with a tenth of no-owner pixels, one of any uint32 (garbage)"""
    rng = np.random.default_rng(seed)
    edges = np.array([0, 3, 4, 5, 6, 7, 8, 9, 10, 11, 72, 73, 74, 78, 79, 80, 2**29 - 1, 2**29, 2**31 - 1, 2**31, 2**32 - 2, 2**32 - 1], dtype=np.uint32)
    bound = np.full((h, w), P.NO_OWNER, dtype=np.uint32)
    bound.reshape(-1)[:len(edges)] = edges
    owned = rng.integers(0, TABLE_TOTAL, size=(h, w)).astype(np.uint32)
    owned[rng.random((h, w)) < 0.1] = P.NO_OWNER
    owned[rng.random((h, w)) < 0.05] = TABLE_TOTAL
    uniform = np.full((h, w), 9, dtype=np.uint32)                                   # every wave has one owner: the last instance of draw 3
    garbage = rng.integers(0, 2**32, size=(h, w), dtype=np.uint64).astype(np.uint32)
    garbage[rng.random((h, w)) < 0.3] %= 128                                        # a share of it lands in and just past the table
    return {"boundaries": bound, "owned": owned, "uniform": uniform, "garbage": garbage}
