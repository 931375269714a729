"""vqhip_displace_meshes on the GPU (docs/DESIGN_DETAILS.md §7.22): the displaced streams bit for bit against tests/displace_ref.py at both output strides, every
refusal through the raw C ABI, and the chains — the library's stream fed straight into the existing rasterisers, compared bit for bit against the EXISTING numpy
references fed tests/displace_ref.py's stream. No tolerance anywhere. References are computed once per process (tests/displace_cases.py) and shared."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import displace_cases as DC
from tests import object_ids_ref as P
from tests import oracle_lib as O
from tests import outline_cases as OC
from tests import scene_interp_cases as IC
from tests.test_gpu_scene_interp import lights, materials, ref_planes
from vqengine_amd import abi, capi

pytestmark = pytest.mark.gpu
GUARD = 0x5A                                             # every byte of an output buffer before the call


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()            # a copy: the shared expectations and cases are read-only


def dev_indices(idx):
    return dev(np.asarray(idx).astype(np.int32))


def device_heightmap(tex, keep):
    if tex["chain"] is None:
        return None
    t = dev(tex["chain"])
    keep.append(t)
    return abi.Texture2D(t.data_ptr(), tex["w"], tex["h"], tex["mips"], 0)


def device_job(jb, compact, keep, tail_rows=3):
    """(capi.DisplaceJob, backing): the output lies inside a guard-filled backing tensor with `tail_rows` spare rows behind it"""
    v = dev(jb["vertices"])
    n, k = v.shape
    back = torch.full((n + tail_rows, 3 if compact else k), 0, dtype=torch.float32, device="cuda")
    back.view(torch.uint8).fill_(GUARD)
    keep.append(v)
    return capi.DisplaceJob(v, device_heightmap(jb["heightmap"], keep), jb["scale_offset"], jb["displacement"], compact, out=back[:n]), back


def hill_streams(ctx, keep):
    """the library's two streams of the chain scene's grid, made by ONE call: (full [V, 11], compact [V, 3])"""
    jb = DC.hill_job()
    v = dev(jb["vertices"])
    hm = device_heightmap(jb["heightmap"], keep)
    keep.append(v)
    full, compact = ctx.displace_meshes([capi.DisplaceJob(v, hm, jb["scale_offset"], jb["displacement"]),
                                         capi.DisplaceJob(v, hm, jb["scale_offset"], jb["displacement"], compact=True)])
    return full, compact


def assert_bits(name, got, ref):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    if got.dtype != ref.dtype and got.dtype.itemsize == ref.dtype.itemsize:
        got = got.view(ref.dtype)                         # torch has no uint32: owner planes and writers travel as int32
    n_bad, idx = O.bits_equal(got, ref)
    assert n_bad == 0, f"{name}: {n_bad} of {ref.size} elements differ, first at {idx.tolist()}"


# ---- 1: the displaced stream ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compact", [False, True], ids=["full_stride", "positions_12_bytes"])
def test_streams_match_the_statement_and_keep_their_guards(ctx, compact):
    """every job of tests/displace_cases.py in ONE call: 4 x 4 / 8 x 8 / 5 x 3 / 1 x 7 maps, the two-level map, the null SRV, 44- and 48-byte vertices, two
    blocks, the batch of 1, 64, 65 and 0 vertices, NaN and +-inf uvs, displacements 100, 0, -2.5 and -0"""
    keep, jobs, backs = [], [], []
    for jb in DC.stream_jobs().values():
        j, b = device_job(jb, compact, keep)
        jobs.append(j)
        backs.append(b)
    outs = ctx.displace_meshes(jobs)
    torch.cuda.synchronize()
    assert len(outs) == len(jobs)
    for name, back in zip(DC.stream_jobs(), backs):
        ref = DC.stream_expected(name, compact)
        n = ref.shape[0]
        got = back.cpu().numpy()
        assert_bits(f"{name} ({'12-byte' if compact else 'full'} stream)", got[:n].view(np.uint32), ref.view(np.uint32))
        assert (got[n:].view(np.uint8) == GUARD).all(), f"{name}: bytes behind the last vertex were written"


def test_second_call_side_stream_and_prepared_call(ctx):
    keep = []
    jb = DC.stream_jobs()["two_blocks_grid17"]
    j, back = device_job(jb, False, keep)
    call, outs = ctx.displace_meshes_prepared([j])
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(2):                                    # the input is untouched: a second call gives the same stream, not a twice displaced one
        call(s)
    s.synchronize()
    torch.cuda.synchronize()
    assert_bits("second call on a side stream", outs[0].cpu().numpy().view(np.uint32), DC.stream_expected("two_blocks_grid17", False).view(np.uint32))
    assert_bits("the input", keep[0].cpu().numpy().view(np.uint32), jb["vertices"].view(np.uint32))


def test_no_jobs_and_empty_jobs_are_ok(ctx):
    assert ctx.displace_meshes([]) == []
    assert ctx.lib.vqhip_displace_meshes(ctx._h, ctx._stream(), None, 0) == abi.VQHIP_OK
    empty = abi.DisplaceJob()
    empty.strideBytes, empty.outStrideBytes = 44, 12        # NULL pointers are fine without vertices
    assert ctx.lib.vqhip_displace_meshes(ctx._h, ctx._stream(), C.pointer(empty), 1) == abi.VQHIP_OK


# ---- 2: every refusal ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx):
    jb = DC.stream_jobs()["wrap_8x8_grid9"]
    n = jb["vertices"].shape[0]
    v, v2 = dev(jb["vertices"]), dev(jb["vertices"])
    chain = dev(jb["heightmap"]["chain"])
    out = torch.zeros((n + 2, 11), dtype=torch.float32, device="cuda")
    out2 = torch.zeros((n + 2, 11), dtype=torch.float32, device="cuda")
    for t in (out, out2):
        t.view(torch.uint8).fill_(GUARD)
    before_v, before_chain = v.clone(), chain.clone()
    lib, hnd, st = ctx.lib, ctx._h, ctx._stream()
    INV, UNS = abi.VQHIP_ERR_INVALID_ARG, abi.VQHIP_ERR_UNSUPPORTED

    def make(**over):
        j = abi.DisplaceJob()
        j.vertices, j.strideBytes, j.numVertices, j.out, j.outStrideBytes, j.reserved = v.data_ptr(), 44, n, out.data_ptr(), 44, 0
        j.heightmap = abi.Texture2D(chain.data_ptr(), 8, 8, jb["heightmap"]["mips"], 0)
        j.uvScaleOffset, j.displacement = abi.float4(*jb["scale_offset"]), jb["displacement"]
        for k, val in over.items():
            if k.startswith("hm_"):
                setattr(j.heightmap, k[3:], val)
            else:
                setattr(j, k, val)
        return j

    def call(*jobs, count=None, null=False):
        arr = (abi.DisplaceJob * max(1, len(jobs)))(*jobs)
        return lib.vqhip_displace_meshes(hnd, st, None if null else arr, len(jobs) if count is None else count)
    second = dict(vertices=v2.data_ptr(), out=out2.data_ptr())
    cases = [("NULL jobs", INV, lambda: call(make(), null=True)), ("negative numJobs", INV, lambda: call(make(), count=-1)),
             ("NULL vertices", INV, lambda: call(make(vertices=None))), ("NULL out", INV, lambda: call(make(out=None))),
             ("stride 40", INV, lambda: call(make(strideBytes=40, outStrideBytes=40))), ("stride 46", INV, lambda: call(make(strideBytes=46, outStrideBytes=46))),
             ("stride above 2048", INV, lambda: call(make(strideBytes=2052, outStrideBytes=12, numVertices=1))),
             ("out stride 16", INV, lambda: call(make(outStrideBytes=16))), ("out stride 48 of a 44-byte vertex", INV, lambda: call(make(outStrideBytes=48))),
             ("reserved", INV, lambda: call(make(reserved=1))), ("vertices misaligned", INV, lambda: call(make(vertices=v.data_ptr() + 2))),
             ("out misaligned", INV, lambda: call(make(out=out.data_ptr() + 2))),
             ("height map width 0", INV, lambda: call(make(hm_width=0))), ("height map height 16385", INV, lambda: call(make(hm_height=16385))),
             ("height map mips 0", INV, lambda: call(make(hm_mips=0))), ("height map mips 5 of 8 x 8", INV, lambda: call(make(hm_mips=5))),
             ("height map misaligned", INV, lambda: call(make(hm_texels=chain.data_ptr() + 2))),
             ("in place", INV, lambda: call(make(out=v.data_ptr()))), ("output inside its input", INV, lambda: call(make(out=v.data_ptr() + 44 * (n - 1)))),
             ("output on the height map", INV, lambda: call(make(out=chain.data_ptr(), numVertices=2))),
             ("output on another job's input", INV, lambda: call(make(), make(vertices=v2.data_ptr(), out=v.data_ptr() + 88, outStrideBytes=12))),
             ("two jobs, one output", INV, lambda: call(make(), make(vertices=v2.data_ptr()))),
             ("outputs overlap by a vertex", INV, lambda: call(make(), make(vertices=v2.data_ptr(), out=out.data_ptr() + 44 * (n - 1)))),
             ("a bad job behind a good one", INV, lambda: call(make(), make(reserved=7, **second))),
             ("2^31 vertices in the call", UNS, lambda: call(make(numVertices=2 ** 30, outStrideBytes=12), make(numVertices=2 ** 30, outStrideBytes=12, **second)))]
    for label, want, fn in cases:
        assert fn() == want, label
        assert len(lib.vqhip_last_error(hnd) or b"") > 10, label
    many = (abi.DisplaceJob * (abi.DISPLACE_MAX_JOBS + 1))()
    big_in = torch.zeros((abi.DISPLACE_MAX_JOBS + 1, 11), dtype=torch.float32, device="cuda")
    big_out = torch.zeros((abi.DISPLACE_MAX_JOBS + 1, 3), dtype=torch.float32, device="cuda")
    big_out.view(torch.uint8).fill_(GUARD)
    for k in range(abi.DISPLACE_MAX_JOBS + 1):
        many[k] = make(vertices=big_in.data_ptr() + 44 * k, numVertices=1, out=big_out.data_ptr() + 12 * k, outStrideBytes=12)
    assert lib.vqhip_displace_meshes(hnd, st, many, abi.DISPLACE_MAX_JOBS + 1) == UNS and len(lib.vqhip_last_error(hnd) or b"") > 10
    torch.cuda.synchronize()
    for t in (out, out2, big_out):
        assert (t.view(torch.uint8) == GUARD).all(), "a refused call wrote to an output"
    assert torch.equal(v, before_v) and torch.equal(chain, before_chain)
    # the same descriptors, accepted: aliased INPUTS and a shared height map are fine, and the table's last entry is the bound
    assert call(make(), make(out=out2.data_ptr(), outStrideBytes=12)) == abi.VQHIP_OK
    assert lib.vqhip_displace_meshes(hnd, st, many, abi.DISPLACE_MAX_JOBS) == abi.VQHIP_OK
    torch.cuda.synchronize()
    assert_bits("after the refusals", out[:n].cpu().numpy().view(np.uint32), DC.stream_expected("wrap_8x8_grid9", False).view(np.uint32))
    assert_bits("after the refusals, 12-byte", out2.view(-1)[:3 * n].cpu().numpy().view(np.uint32).reshape(n, 3), DC.stream_expected("wrap_8x8_grid9", True).view(np.uint32))
    assert (out[n:].view(torch.uint8) == GUARD).all() and (big_out[abi.DISPLACE_MAX_JOBS:].view(torch.uint8) == GUARD).all() and not (big_out[0].view(torch.uint8) == GUARD).any()
    # the Python binding validates before it calls
    with pytest.raises(ValueError):
        ctx.displace_meshes([capi.DisplaceJob(v[:, :10])])
    with pytest.raises(ValueError):
        ctx.displace_meshes([capi.DisplaceJob(v, compact=True, out=out[:n])])
    with pytest.raises(ValueError):
        ctx.displace_meshes([capi.DisplaceJob(v, heightmap=chain)])


# ---- 3: the chains -------------------------------------------------------------------------------------------------------------------------------------------------------
def scene_draws(scene, full, compact=None, masked=False, keep=None):
    """the device draws of the hill scene: draw 0 reads the LIBRARY's stream (compact for the opaque depth calls, else full), draw 1 the card"""
    hill, card = scene["draws"]
    cardv = dev(card["positions"])
    mk = lambda d, p: capi.SurfaceDraw(p, dev_indices(d["indices"]), dev(d["wvp"]), dev(d["world"]), dev(d["normal"]), dev(d["wvp_prev"]), d["material"])   # noqa: E731
    surf = [mk(hill, full), mk(card, cardv)]
    depth = [capi.ShadowDraw(compact if compact is not None else full, surf[0].indices, surf[0].wvp, None, hill["cull"]), surf[1].depth_draw(card["cull"])]
    if masked:
        m = card["mask"]
        mat = abi.MaterialDesc()
        mat.data.uvScaleOffset, mat.data.textureConfig = abi.float4(*m["scale_offset"]), m["texture_config"]
        mat.texDiffuse = device_heightmap(m["tex"], keep)
        mat.texDiffuse.reserved = abi.MATERIAL_ALPHA_MASKED
        depth = [capi.MaskedDraw(full, surf[0].indices, surf[0].wvp, None, hill["cull"]), capi.MaskedDraw(cardv, surf[1].indices, surf[1].wvp, None, card["cull"], material=mat)]
    return surf, depth


def test_chain_scene_depth_1x_and_4x(ctx):
    """the 12-byte stream -> vqhip_scene_depth at 64 x 48 (1x) and 32 x 32 (4x, two layers) == tests/scene_depth_ref.py on the statement's stream"""
    keep = []
    full, compact = hill_streams(ctx, keep)
    for (w, h, s, layers) in ((64, 48, 1, 0), (32, 32, 4, 2)):
        _, depth = scene_draws(DC.hill_scene(w, h, s), full, compact)
        z = ctx.scene_depth(depth, w, h, s, primitive=True, layers=layers)
        torch.cuda.synchronize()
        e = DC.depth_expected(w, h, s, layers or None)
        assert_bits(f"depth {w}x{h} s{s}", z["depth"].cpu().numpy(), e["depth"])
        assert_bits(f"primitive {w}x{h} s{s}", z["primitive"].cpu().numpy(), e["primitive"])
        for k in range(layers):
            assert_bits(f"coverage[{k}]", z["coverage"][k].cpu().numpy(), e["coverage"][k])
            assert_bits(f"layerPrimitive[{k}]", z["layer_primitive"][k].cpu().numpy(), e["layer_primitive"][k])
        flat = DC.depth_expected(w, h, s, layers or None, displaced=False)
        assert DC.changed_fraction(z["depth"].cpu().numpy(), flat["depth"]) >= 0.25


def test_chain_shadow_depth(ctx):
    """the 12-byte stream -> vqhip_shadow_depth, one z / w view and one LINEAR_DEPTH view at dim 48 == tests/shadow_raster_ref.py"""
    keep = []
    _, compact = hill_streams(ctx, keep)
    views, maps = [], []
    for v in DC.shadow_views(48):
        t = torch.full((48, 48), -7.0, dtype=torch.float32, device="cuda")
        maps.append(t)
        hill, card = v["draws"]
        views.append(capi.ShadowView(t, [capi.ShadowDraw(compact, dev_indices(hill["indices"]), dev(hill["wvp"]), dev(hill["world"]), hill["cull"]),
                                         capi.ShadowDraw(dev(card["positions"]), dev_indices(card["indices"]), dev(card["wvp"]), dev(card["world"]), card["cull"])],
                                     v["linear"], v["camera"], v["far"]))
    ctx.shadow_depth(views)
    torch.cuda.synchronize()
    for k, (t, e, f) in enumerate(zip(maps, DC.shadow_expected(48), DC.shadow_expected(48, displaced=False))):
        assert_bits(f"shadow view {k}", t.cpu().numpy(), e)
        assert DC.changed_fraction(t.cpu().numpy(), f) >= 0.25


def test_chain_masked_depth_interpolants_ids_and_lit_frame(ctx):
    """the full-stride stream -> vqhip_scene_masked_depth (the card behind the hill is alpha-tested) -> vqhip_scene_interpolants and vqhip_scene_quad_interpolants over
    that owner plane -> vqhip_forward_lighting_from_materials; vqhip_scene_depth -> vqhip_object_ids. Each against its existing reference on the statement's stream;
    the lit frame against the oracle on the reference's interpolants."""
    keep = []
    w, h = 64, 48
    full, compact = hill_streams(ctx, keep)
    scene = DC.hill_scene(w, h, 1)
    surf, masked = scene_draws(scene, full, masked=True, keep=keep)
    z = ctx.scene_masked_depth(masked, w, h, 1, primitive=True)
    torch.cuda.synchronize()
    e = DC.masked_expected(w, h)
    assert_bits("masked depth", z["depth"].cpu().numpy(), e["depth"])
    assert_bits("masked owner plane", z["primitive"].cpu().numpy(), e["primitive"])
    flat = DC.masked_expected(w, h, displaced=False)
    assert DC.changed_fraction(z["depth"].cpu().numpy(), flat["depth"]) >= 0.25
    hill_tris = len(DC.hill_job()["indices"]) // 3
    got_owner = z["primitive"].cpu().numpy().view(np.uint32)
    assert ((flat["primitive"] >= hill_tris) & (flat["primitive"] != 0xFFFFFFFF) & (got_owner < hill_tris)).sum() >= 1, "the hill hides part of the card"

    ref_ip, ref_quad = DC.interp_expected(w, h)
    ip = ctx.scene_interpolants(surf, w, h, z["primitive"], sv=True)
    qp = ctx.scene_quad_interpolants(surf, w, h, z["primitive"], sv=True)
    torch.cuda.synchronize()
    for k in IC.PLANES:
        assert_bits(f"interpolants {k}", ip[k].cpu().numpy().view(np.uint32), ref_ip[k])
        assert_bits(f"quad interpolants {k}", qp[k].cpu().numpy().view(np.uint32), ref_quad[k])
    assert_bits("quad_uv", qp["quad_uv"].cpu().numpy().view(np.uint32), ref_quad["quad_uv"])

    hmats, dmats, mkeep = materials(ctx)
    pf, extra, pv = lights(w, h)
    lit = ctx.forward_lighting_from_materials([ip[k] for k in IC.PLANES[:3]], dmats, pf, pv, extra_point=extra)
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        gb = O.gbuffer_from_materials(ref_planes(ref_ip), hmats, pf.fAmbientLightingFactor)
        want = O.forward_lighting(gb, pf, pv, abi.FMT_RGBA16F, extra_point=extra)
    assert_bits("lit frame of the hill", lit.cpu().numpy(), want)

    _, depth = scene_draws(scene, full, compact)
    zo = ctx.scene_depth(depth, w, h, 1, primitive=True)              # the ObjectID pass's own depth call: every draw of the scene has cull NONE
    id_draws, want_ids = DC.ids_expected(w, h)
    ids = ctx.object_ids([capi.ObjectIdDraw(d["num_indices"], dev(d["obj_id"]), d["mesh_id"], d["material_id"]) for d in id_draws], w, h, zo["primitive"])
    torch.cuda.synchronize()
    assert_bits("object ids", ids["ids"].cpu().numpy(), want_ids)
    assert_bits("object ids' owner plane", zo["primitive"].cpu().numpy(), DC.depth_expected(w, h, 1, None)["primitive"])
    assert want_ids.shape == (h, w, 4) and P.instanced_triangles(id_draws) == hill_tris + 2


def test_chain_outline_of_the_selected_hill(ctx):
    """the full-stride stream -> vqhip_outline with the displaced grid selected == tests/outline_ref.py on the statement's stream"""
    keep = []
    w, h = 64, 48
    full, _ = hill_streams(ctx, keep)
    d = DC.outline_scene(w, h)["draws"][0]
    color = dev(OC.prefill(w, h).view(np.int16))
    res = ctx.outline([capi.OutlineDraw(full, dev_indices(d["indices"]), dev(d["cb"]))], w, h, color.view(torch.float16))
    torch.cuda.synchronize()
    e = DC.outline_expected(w, h)
    assert_bits("outline scene colour", color.cpu().numpy().view(np.uint16), e["scene_color"])
    assert_bits("outline selection", res["selection"].cpu().numpy(), e["selection"])
    assert_bits("outline writer", res["writer"].cpu().numpy(), e["writer"])
    assert (res["selection"].cpu().numpy() != DC.outline_expected(w, h, displaced=False)["selection"]).sum() > 100
