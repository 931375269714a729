"""vqhip_object_ids on the GPU (docs/DESIGN_DETAILS.md §7.21 P0): the ids plane bit for bit against tests/object_ids_ref.py, no tolerance, through the Python binding
and, for the refusals, the raw C ABI. Frames of 16 x 16, 64 x 40 and 129 x 67: one block, several blocks, partial blocks on both axes. The chain tests run the
ObjectID pass as the engine does: its own depth call with every cull mode NONE, then the resolve over that call's owner plane. References are computed once per
case and shared; each GPU step runs once."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import masked_depth_cases as MC
from tests import object_ids_cases as PC
from tests import object_ids_ref as P
from tests import scene_depth_ref as V
from tests.test_gpu_masked_depth import _KEEP as MASKED_KEEP, device_draw as masked_device_draw
from tests.test_gpu_scene_depth import device_draw as depth_device_draw
from vqengine_amd import abi, capi

pytestmark = pytest.mark.gpu
SENT = 0x5A5A5A5A


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_owner(owner):
    return dev(np.ascontiguousarray(owner).view(np.int32))


def id_device_draw(d):
    return capi.ObjectIdDraw(d["num_indices"], dev(d["obj_id"]), d["mesh_id"], d["material_id"])


def run(ctx, draws, owner, pad=0, work=None, stream=None, ddraws=None):
    """ids (with `pad` sentinel columns behind each row) of the host id draws under the host owner plane (or a device tensor)"""
    h, w = owner.shape
    back = torch.full((h, w + pad, 4), SENT, dtype=torch.int32, device="cuda")
    if stream is not None:
        torch.cuda.synchronize()                                                   # the prefill and the uploads ran on the current stream
    ctx.object_ids(ddraws if ddraws is not None else [id_device_draw(d) for d in draws], w, h, owner if torch.is_tensor(owner) else dev_owner(owner),
                   out=back[:, :w], work=work, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return back.cpu().numpy()


def assert_ids(name, got, ref):
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, f"{name}: {len(bad)} of {ref.size} elements differ from tests/object_ids_ref.py, first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {ref[tuple(bad[0])]}"


# ---- P0 on hand-made owner planes --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["wave", "lane"])
@pytest.mark.parametrize("size", PC.SIZES)
def test_p0_planes_match_the_statement(ctx, set_opt, size, form):
    """the table with empty draws, one, three and 64 instances under the boundary plane (instance boundaries, last q of each draw, q = total, 2^29, 2^31, 0xFFFFFFFF),
    the owned plane, the one-owner plane (every wave takes the uniform path) and the garbage plane, in both forms of the resolve"""
    set_opt("interp_form", form)
    w, h = size
    t = PC.table()
    ddraws = [id_device_draw(d) for d in t]
    for name, plane in PC.owner_planes(w, h).items():
        assert_ids(f"{name} {w}x{h} {form}", run(ctx, t, plane, ddraws=ddraws), P.resolve(t, plane))


def test_garbage_owner_plane_yields_only_table_values_or_zeros(ctx):
    t = PC.table()
    got = run(ctx, t, PC.owner_planes(129, 67, seed=17)["garbage"]).reshape(-1, 4)
    allowed = {(0, 0, 0, 0)}
    for d in t:
        if d["num_indices"]:
            allowed |= {(int(o[0]), d["mesh_id"], d["material_id"], int(o[3])) for o in d["obj_id"]}
    seen = set(map(tuple, got.tolist()))
    assert seen <= allowed and len(seen) > 20 and (0, 0, 0, 0) in seen


# ---- the ObjectID chain ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PC.chain_cases()))
def test_chain_scene_depth_then_object_ids(ctx, name):
    """boxes (64 instances, 16-bit indices, 44-byte stride) and the room, all cull modes NONE: vqhip_scene_depth's owner plane == the statement of §7.17, and
    vqhip_object_ids over THAT device plane == P0 over the statement's"""
    scene = PC.chain_cases()[name]
    owner, draws, ids = PC.chain_expected(name)
    assert all(d["cull"] == V.CULL_NONE for d in scene["draws"])
    z = ctx.scene_depth([depth_device_draw(d) for d in scene["draws"]], scene["width"], scene["height"], 1, primitive=True)
    got = run(ctx, draws, z["primitive"])
    assert np.array_equal(z["primitive"].cpu().numpy().view(np.uint32), owner), f"{name}: the owner plane differs from tests/scene_depth_ref.py"
    assert_ids(name, got, ids)


def test_masked_chain_shows_the_object_behind_the_holes(ctx):
    """the checker card (alpha_checker, masked material) in front of the wall through vqhip_scene_masked_depth: inside the card's silhouette the ids are the card's
    where the texture is opaque and the WALL's in the holes"""
    name = "magnified_64x48_s1"
    scene = MC.cases()[name]
    draws = PC.id_draws(scene["draws"])
    z = ctx.scene_masked_depth([masked_device_draw(d) for d in scene["draws"]], 64, 48, 1, primitive=True)
    got = run(ctx, draws, z["primitive"])
    MASKED_KEEP.clear()                                                            # the device textures that module's helper keeps alive for its own tests
    owner = MC.expected(name)["primitive"]
    assert np.array_equal(z["primitive"].cpu().numpy().view(np.uint32), owner)
    assert_ids(name, got, P.resolve(draws, owner))
    solid = V.rasterize(MC.opaque(scene))["primitive"]                             # the card drawn opaque: its silhouette
    wall, card = draws[0], draws[1]
    inside = P.resolve(draws, solid)[..., 1] == card["mesh_id"]
    holes = inside & (got[..., 1] == wall["mesh_id"])
    assert inside.sum() > 200 and holes.sum() > 40 and (inside & (got[..., 1] == card["mesh_id"])).sum() > 40
    assert (got[holes][:, 0] == wall["obj_id"][0, 0]).all() and (got[holes][:, 2] == wall["material_id"]).all() and (got[holes][:, 3] == wall["obj_id"][0, 3]).all()


# ---- buffers, pitches, streams -------------------------------------------------------------------------------------------------------------------------------------------
def test_pitched_planes_keep_their_padding(ctx):
    t = PC.table()
    plane = PC.owner_planes(129, 67)["owned"]
    wide = torch.full((67, 140), 5, dtype=torch.int32, device="cuda")              # a pitched owner plane whose padding holds an owned q
    wide[:, :129] = dev_owner(plane)
    got = run(ctx, t, wide[:, :129], pad=3)
    assert_ids("pitched", got[:, :129], P.resolve(t, plane))
    assert (got[:, 129:] == SENT).all(), "the padding of ids was written"


def test_prefilled_work_buffer_second_call_and_work_size(ctx):
    t = PC.table()
    plane = PC.owner_planes(64, 40)["owned"]
    need = capi.object_ids_work_bytes(len(t))
    assert need == 256
    work = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    for label in ("0xFF-filled work buffer", "second call on the same buffer"):
        assert_ids(label, run(ctx, t, plane, work=work[:need]), P.resolve(t, plane))
    assert (work[need:] == 0xFF).all(), "the call wrote past vqhip_object_ids_work_bytes"
    jobs = sum(1 for d in t if d["num_indices"])
    assert (work[jobs * abi.OBJECT_ID_JOB_BYTES:need] == 0xFF).all()               # the table holds the draws with indices, nothing else


def test_non_default_stream(ctx):
    s = torch.cuda.Stream()
    t = PC.table()
    plane = PC.owner_planes(64, 40)["owned"]
    owner = dev_owner(plane)
    ddraws = [id_device_draw(d) for d in t]
    torch.cuda.synchronize()
    assert_ids("side stream", run(ctx, t, owner, stream=s, ddraws=ddraws), P.resolve(t, plane))


def test_no_draws_clears_the_plane(ctx):
    plane = PC.owner_planes(64, 40)["garbage"]
    assert (run(ctx, [], plane) == 0).all()
    assert (run(ctx, [P.id_draw(0, np.ones((2, 4)), 3, 4)], plane) == 0).all()      # a list of empty draws: no table entry at all


def test_many_draws_cross_the_ring_slots(ctx):
    """3 500 draws of one or two triangles and one to three instances (3 000 table entries: three ring slots), every seventh one empty, and an owner plane that walks
    through every q: the binary search meets every entry, empty draws own nothing and do not shift q"""
    rng = np.random.default_rng(9)
    n = 3500
    pool = dev(rng.integers(-2**31, 2**31, size=(n + 3, 4), dtype=np.int64).astype(np.int32))
    host_pool = pool.cpu().numpy()
    draws, ddraws = [], []
    for k in range(n):
        idx, inst = (0 if k % 7 == 3 else 3 * int(rng.integers(1, 3))), int(rng.integers(1, 4))
        draws.append(P.id_draw(idx, host_pool[k:k + inst], k + 1, -k))
        ddraws.append(capi.ObjectIdDraw(idx, pool[k:k + inst], k + 1, -k))
    total = P.instanced_triangles(draws)
    w = 129
    h = (total + 2 + w - 1) // w
    assert sum(1 for d in draws if d["num_indices"]) == 3000 and h < 100
    plane = np.full(w * h, P.NO_OWNER, dtype=np.uint32)
    plane[:total + 2] = rng.permutation(total + 2)
    plane = plane.reshape(h, w)
    got = run(ctx, draws, plane, ddraws=ddraws)
    assert_ids("3500 draws", got, P.resolve(draws, plane))
    assert len(set(got[..., 1].reshape(-1).tolist())) == 1 + sum(1 for d in draws if d["num_indices"])      # every draw with indices, and 0


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx):
    w, h = 64, 40
    t = PC.table()[3]                                                              # 6 indices, 3 instances
    plane = np.full((h, w), 4, dtype=np.uint32)
    owner = dev_owner(plane)
    obj = dev(t["obj_id"])
    ids = torch.full((h, w, 4), SENT, dtype=torch.int32, device="cuda")
    need = capi.object_ids_work_bytes(1)
    work = torch.full((need,), 0x3C, dtype=torch.uint8, device="cuda")
    lib, hnd, st = ctx.lib, ctx._h, ctx._stream()

    def call(ndraws=1, draws_null=False, width=w, height=h, optr=None, opitch=0, iptr=None, ipitch=0, wptr=None, wbytes=None, **over):
        draw = abi.ObjectIdDraw()
        draw.numIndices, draw.numInstances, draw.objID, draw.meshID, draw.materialID = t["num_indices"], 3, obj.data_ptr(), t["mesh_id"], t["material_id"]
        for k, val in over.items():
            setattr(draw, k, val)
        return lib.vqhip_object_ids(hnd, st, None if draws_null else C.pointer(draw), ndraws, width, height, C.c_void_p(owner.data_ptr() if optr is None else optr), opitch,
                                    C.c_void_p(ids.data_ptr() if iptr is None else iptr), ipitch, C.c_void_p(work.data_ptr() if wptr is None else wptr),
                                    work.numel() if wbytes is None else wbytes)
    INV = abi.VQHIP_ERR_INVALID_ARG
    cases = [("NULL draws", dict(draws_null=True)), ("NULL owner", dict(optr=0)), ("NULL ids", dict(iptr=0)), ("NULL work", dict(wptr=0)), ("NULL objID", dict(objID=None)),
             ("negative numDraws", dict(ndraws=-1)), ("width 0", dict(width=0)), ("height 0", dict(height=0)),
             ("width above the limit", dict(width=abi.SCENE_DEPTH_MAX_DIM + 1)), ("height above the limit", dict(height=abi.SCENE_DEPTH_MAX_DIM + 1)),
             ("owner pitch below the row", dict(opitch=w - 1)), ("negative owner pitch", dict(opitch=-w)), ("ids pitch below the row", dict(ipitch=w - 1)),
             ("negative ids pitch", dict(ipitch=-1)), ("ids not 16-byte aligned", dict(iptr=ids.data_ptr() + 8)), ("owner not 4-byte aligned", dict(optr=owner.data_ptr() + 2)),
             ("objID not 4-byte aligned", dict(objID=obj.data_ptr() + 2)), ("no instances", dict(numInstances=0)), ("65 instances", dict(numInstances=65)),
             ("numIndices not a multiple of 3", dict(numIndices=7)), ("workBytes one short", dict(wbytes=need - 1)), ("work not aligned", dict(wptr=work.data_ptr() + 16)),
             ("ids inside the work buffer", dict(iptr=work.data_ptr() + 16)), ("ids on the owner plane", dict(iptr=owner.data_ptr())),
             ("owner inside ids", dict(optr=ids.data_ptr() + 64))]
    for label, over in cases:
        assert call(**over) == INV, label
        assert len(lib.vqhip_last_error(hnd) or b"") > 10, label
    # 64 instances of 2^23 triangles are 2^29 instanced triangles: vqhip_scene_depth's limit, the q this call could be handed
    assert call(numIndices=3 * 2 ** 23, numInstances=64) == abi.VQHIP_ERR_UNSUPPORTED and len(lib.vqhip_last_error(hnd) or b"") > 10
    many = (abi.ObjectIdDraw * 20001)()
    one = abi.ObjectIdDraw()
    one.numIndices, one.numInstances, one.objID = 3, 1, obj.data_ptr()
    for k in range(20001):
        many[k] = one
    big = torch.full((capi.object_ids_work_bytes(20001),), 0x3C, dtype=torch.uint8, device="cuda")
    assert lib.vqhip_object_ids(hnd, st, many, 20001, w, h, C.c_void_p(owner.data_ptr()), 0, C.c_void_p(ids.data_ptr()), 0, C.c_void_p(big.data_ptr()), big.numel()) == abi.VQHIP_ERR_UNSUPPORTED
    assert len(lib.vqhip_last_error(hnd) or b"") > 10
    torch.cuda.synchronize()
    assert (ids == SENT).all(), "a refused call wrote to ids"
    assert (work == 0x3C).all() and (big == 0x3C).all(), "a refused call wrote to the work buffer"
    assert call() == abi.VQHIP_OK
    torch.cuda.synchronize()
    assert_ids("after the refusals", ids.cpu().numpy(), P.resolve([t], plane))
    # the Python binding validates before it calls
    d = capi.ObjectIdDraw(6, obj, 1, 2)
    with pytest.raises(ValueError):
        ctx.object_ids([d], w, h, owner[:, :-1])
    with pytest.raises(ValueError):
        ctx.object_ids([capi.ObjectIdDraw(7, obj, 1, 2)], w, h, owner)
    with pytest.raises(ValueError):
        ctx.object_ids([capi.ObjectIdDraw(6, obj[:, :3], 1, 2)], w, h, owner)
    with pytest.raises(ValueError):
        ctx.object_ids([d], w, h, owner, out=torch.empty((h, w - 1, 4), dtype=torch.int32, device="cuda"))
