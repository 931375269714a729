"""vqhip_line_draws on the GPU (docs/DESIGN_DETAILS.md §7.24 L1 .. L8): scene colour and writer bit for bit against tests/line_ref.py, no tolerance, through the
Python binding and, for the refusals, the raw C ABI. The scenes are tests/line_cases.py's at 16 x 16, 64 x 40 and 129 x 67 (one tile, several tiles, a partial last
tile with an odd last column and row); scene colour is prefilled with tests/unlit_cases.py's recognisable half pattern and every pixel without a passing fragment
must keep its exact bits; sceneDepth must keep its own. References are computed once per case and shared; each GPU step runs once."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import line_cases as LC
from tests import line_ref as L
from tests import oracle_lib as O
from tests import outline_cases as OC
from tests import outline_ref as OR
from tests import unlit_cases as UC
from tests import unlit_ref as R
from tests.test_gpu_unlit_draws import ROOM_LIGHTS, device_draw as unlit_device_draw, room_view_proj
from vqengine_amd import abi, capi
from vqengine_amd import line_scene as LS
from vqengine_amd import shadow_scene as S
from vqengine_amd import unlit_scene as US

pytestmark = pytest.mark.gpu
SENT_H, SENT_I = 0x1234, 0x5A5A5A5A


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_draw(d, bits=32):
    idx = np.asarray(d["indices"])
    ix = dev(idx.astype(np.uint16).view(np.int16)) if bits == 16 else dev(idx.astype(np.int32))
    if d["kind"] == "axes":
        return capi.VertexAxesDraw(dev(d["vertices"]), ix, dev(d["cb"]))
    return capi.WireframeDraw(dev(d["vertices"]), ix, dev(d["matrices"]), dev(d["color"]))


def run(ctx, scene, pad=0, writer=True, work=None, stream=None, bits=32, color=None):
    """the planes as numpy (uint16 half bits, uint32, float32), each with `pad` sentinel columns behind its rows; the depth plane comes back to show it was not written"""
    w, h = scene["width"], scene["height"]
    plane = torch.full((h, w + pad, 4), SENT_H, dtype=torch.int16, device="cuda")
    plane[:, :w] = dev((LC.prefill(w, h) if color is None else color).view(np.int16).copy())
    depth = torch.full((h, w + pad), -7.0, dtype=torch.float32, device="cuda")
    depth[:, :w] = dev(scene["depth"])
    wr = torch.full((h, w + pad), SENT_I, dtype=torch.int32, device="cuda")
    draws = [device_draw(d, bits) for d in scene["draws"]]
    if stream is not None:
        torch.cuda.synchronize()                                                   # the prefills and uploads ran on the current stream
    ctx.line_draws(draws, w, h, plane.view(torch.float16)[:, :w], depth[:, :w], writer=writer, out={"writer": wr[:, :w]}, work=work, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return {"scene_color": plane.cpu().numpy().view(np.uint16), "writer": wr.cpu().numpy().view(np.uint32), "depth": depth.cpu().numpy()}


def assert_planes(name, got, ref, w, keys=("scene_color", "writer")):
    for k in keys:
        g, e = got[k][:, :w], ref[k]
        bad = np.argwhere(g != e)
        assert len(bad) == 0, f"{name} {k}: {len(bad)} of {e.size} elements differ from tests/line_ref.py, first at {bad[0].tolist()}: {g[tuple(bad[0])]:#x} != {e[tuple(bad[0])]:#x}"


def assert_depth_kept(name, got, scene):
    w = scene["width"]
    assert np.array_equal(got["depth"][:, :w].view(np.uint32), np.asarray(scene["depth"], dtype=np.float32).view(np.uint32)), f"{name}: sceneDepth was written"


@pytest.mark.parametrize("name", LC.names())
def test_case_matches_the_statement(ctx, name):
    """every case at each size over the prefilled scene colour: colour (every pixel without a passing fragment keeps its prefilled bits, NaN payloads included) and
    writer; sceneDepth keeps its bits. The adversarial lines come as degenerate triangles and as axes; the cube comes 512 times; the soup puts more than
    256 x 9 lines into one tile; the clip case crosses every plane and carries non-finite positions and indices past the buffer."""
    scene = LC.case(name)
    w, h = scene["width"], scene["height"]
    got, ref = run(ctx, scene), LC.expected(name)
    assert_planes(name, got, ref, w)
    assert_depth_kept(name, got, scene)
    keep = ref["writer"] == L.NO_WRITER
    assert np.array_equal(got["scene_color"][keep], LC.prefill(w, h)[keep])


def test_both_tile_sizes_give_the_same_bits(ctx, set_opt):
    """every scene at 129 x 67 (at tile 64: three tiles across, two down, the last partial on both axes) and the adversarial lines at 64 x 40, under raster_tile 64 and 32"""
    for tile in (64, 32):
        set_opt("raster_tile", tile)
        for name in [f"{b}_129x67" for b in LC.BUILDERS] + ["adversarial_wire_64x40", "adversarial_axes_64x40", "soup_64x40"]:
            assert_planes(f"tile {tile} {name}", run(ctx, LC.case(name)), LC.expected(name), LC.case(name)["width"])


def test_submission_order_decides_exactly_the_shared_pixels(ctx):
    for (w, h) in LC.SIZES:
        ab, ba = run(ctx, LC.case(f"crossing_ab_{w}x{h}")), run(ctx, LC.case(f"crossing_ba_{w}x{h}"))
        assert_planes("ab", ab, LC.expected(f"crossing_ab_{w}x{h}"), w)
        assert_planes("ba", ba, LC.expected(f"crossing_ba_{w}x{h}"), w)
        # ab's draw 0 is ba's draw 1: a pixel both draws reach goes to the later one in both orders — the same writer index, another draw, another colour
        shared = (ab["writer"] == 1) & (ba["writer"] == 1)
        differ = (ab["scene_color"] != ba["scene_color"]).any(axis=-1)
        assert shared.sum() >= 4 and np.array_equal(differ, shared)


def test_pitched_planes_keep_their_padding_and_16_bit_indices(ctx):
    for name, bits in (("soup_129x67", 32), ("crossing_ab_64x40", 16), ("axes_mesh_129x67", 16), ("clip_planes_64x40", 16)):
        scene = LC.case(name)
        w = scene["width"]
        got = run(ctx, scene, pad=5, bits=bits)
        assert_planes(f"pitched {name}", got, LC.expected(name), w)
        assert_depth_kept(f"pitched {name}", got, scene)
        assert (got["scene_color"][:, w:] == SENT_H).all() and (got["writer"][:, w:] == SENT_I).all() and (got["depth"][:, w:] == -7.0).all(), f"{name}: padding written"


def test_prefilled_work_buffer_second_call_and_work_size(ctx):
    name = "soup_64x40"
    scene = LC.case(name)
    need = capi.line_draws_work_bytes(L.total_lines(scene))
    assert need >= L.total_lines(scene) * abi.LINE_BYTES
    work = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    for label in ("0xFF-filled work buffer", "second call on the same buffer"):
        assert_planes(f"{name}: {label}", run(ctx, scene, work=work[:need]), LC.expected(name), 64)
    other = "cube_instances_64x40"                                                  # another call's lines over the first call's records
    work2 = torch.full((capi.line_draws_work_bytes(L.total_lines(LC.case(other))) + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    assert_planes(other, run(ctx, LC.case(other), work=work2[:-256]), LC.expected(other), 64)
    assert_planes(f"{name} after {other}", run(ctx, scene, work=work2[:-256]), LC.expected(name), 64)
    assert (work[need:] == 0xFF).all() and (work2[-256:] == 0xFF).all(), "the call wrote past vqhip_line_draws_work_bytes"


def test_non_default_stream(ctx):
    name = "crossing_ab_129x67"
    assert_planes("side stream", run(ctx, LC.case(name), stream=torch.cuda.Stream()), LC.expected(name), 129)


def test_writer_null(ctx):
    """writer NULL: scene colour is unchanged by its absence, the tensor is not touched"""
    name = "crossing_ab_64x40"
    got = run(ctx, LC.case(name), writer=False)
    assert_planes("writer NULL", got, LC.expected(name), 64, ("scene_color",))
    assert (got["writer"] == SENT_I).all()


def test_no_draws_clears_writer(ctx):
    w, h = 64, 40
    got = run(ctx, LC.scene(w, h, []), pad=2)
    assert np.array_equal(got["scene_color"][:, :w], LC.prefill(w, h)) and (got["writer"][:, :w] == L.NO_WRITER).all()
    assert (got["writer"][:, w:] == SENT_I).all() and (got["scene_color"][:, w:] == SENT_H).all()
    got = run(ctx, LC.scene(w, h, []), writer=False)                                # nothing to draw, nothing to clear
    assert np.array_equal(got["scene_color"], LC.prefill(w, h)) and (got["writer"] == SENT_I).all()
    # a list of empty draws is the same call, and an empty draw in front shifts the writer index, not the picture
    sc = LC.case("crossing_ab_64x40")
    empty = dict(sc["draws"][0], indices=np.zeros(0, dtype=np.int64))
    got = run(ctx, dict(sc, draws=[empty, empty]))
    assert np.array_equal(got["scene_color"], LC.prefill(w, h)) and (got["writer"] == L.NO_WRITER).all()
    got, ref = run(ctx, dict(sc, draws=[empty] + sc["draws"])), LC.expected("crossing_ab_64x40")
    assert np.array_equal(got["scene_color"], ref["scene_color"])
    assert np.array_equal(got["writer"], np.where(ref["writer"] == L.NO_WRITER, ref["writer"], ref["writer"] + 1))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx):
    w, h = 64, 40
    sc = LC.case("crossing_ab_64x40")
    wd = device_draw(sc["draws"][0])
    ad = device_draw(LC.case("axes_mesh_64x40")["draws"][0])
    color = dev(LC.prefill(w, h).view(np.int16).copy())
    depth = dev(sc["depth"])
    wr = torch.full((h, w), SENT_I, dtype=torch.int32, device="cuda")
    need = capi.line_draws_work_bytes(wd.indices.numel())
    work = torch.full((max(need, w * h * 8 + 1024),), 0x3C, dtype=torch.uint8, device="cuda")
    lib, hnd, st = ctx.lib, ctx._h, ctx._stream()

    def wire_draw():
        draw = abi.LineDraw()
        draw.mesh.positions, draw.mesh.strideBytes, draw.mesh.numVertices = wd.positions.data_ptr(), wd.positions.stride(0) * 4, wd.positions.shape[0]
        draw.mesh.indices, draw.mesh.indexBits, draw.mesh.numIndices = wd.indices.data_ptr(), 32, wd.indices.numel()
        draw.matModelViewProj, draw.color, draw.numInstances, draw.kind = wd.matrices.data_ptr(), wd.color.data_ptr(), 1, abi.LINES_WIREFRAME
        return draw

    def axes_draw():
        draw = abi.LineDraw()
        draw.mesh.positions, draw.mesh.strideBytes, draw.mesh.numVertices = ad.vertices.data_ptr(), ad.vertices.stride(0) * 4, ad.vertices.shape[0]
        draw.mesh.indices, draw.mesh.indexBits, draw.mesh.numIndices = ad.indices.data_ptr(), 32, 12
        draw.axes, draw.numInstances, draw.kind = ad.cb.data_ptr(), 1, abi.LINES_VERTEX_AXES
        return draw

    def targets():
        tg = abi.UnlitTargets()
        tg.sceneColor, tg.sceneDepth, tg.writer = color.data_ptr(), depth.data_ptr(), wr.data_ptr()
        return tg

    def call(make=wire_draw, ndraws=1, wptr=None, wbytes=None, draws_null=False, out_null=False, width=w, height=h, **over):
        draw, tg = make(), targets()
        for k, val in over.items():
            obj, field = {"m": (draw.mesh, k[2:]), "d": (draw, k[2:]), "t": (tg, k[2:])}[k[0]]
            setattr(obj, field, val)
        return lib.vqhip_line_draws(hnd, st, None if draws_null else C.pointer(draw), ndraws, width, height, None if out_null else C.byref(tg),
                                    C.c_void_p(work.data_ptr() if wptr is None else wptr), need if wbytes is None else wbytes)
    INV = abi.VQHIP_ERR_INVALID_ARG
    A = dict(make=axes_draw)
    cases = [("NULL draws", dict(draws_null=True)), ("NULL out", dict(out_null=True)), ("NULL sceneColor", dict(t_sceneColor=None)), ("NULL sceneDepth", dict(t_sceneDepth=None)),
             ("NULL work", dict(wptr=0)), ("negative numDraws", dict(ndraws=-1)), ("NULL positions", dict(m_positions=None)), ("NULL indices", dict(m_indices=None)),
             ("width 0", dict(width=0)), ("height 0", dict(height=0)), ("width above the limit", dict(width=abi.SCENE_DEPTH_MAX_DIM + 1)),
             ("height above the limit", dict(height=abi.SCENE_DEPTH_MAX_DIM + 1)), ("targets reserved set", dict(t_reserved=1)),
             ("kind 2", dict(d_kind=2)), ("kind -1", dict(d_kind=-1)),
             ("wireframe without matrices", dict(d_matModelViewProj=None)), ("wireframe without colour", dict(d_color=None)), ("wireframe with axes", dict(d_axes=ad.cb.data_ptr())),
             ("axes without cb", dict(A, d_axes=None)), ("axes with matrices", dict(A, d_matModelViewProj=wd.matrices.data_ptr())), ("axes with colour", dict(A, d_color=wd.color.data_ptr())),
             ("0 instances", dict(d_numInstances=0)), ("513 instances", dict(d_numInstances=513)), ("axes with 2 instances", dict(A, d_numInstances=2)),
             ("axes with 0 instances", dict(A, d_numInstances=0)),
             ("pitch below the row", dict(t_pitch=w - 1)), ("negative pitch", dict(t_pitch=-w)), ("depth pitch below the row", dict(t_depth_pitch=w - 1)),
             ("negative depth pitch", dict(t_depth_pitch=-1)), ("writer pitch below the row", dict(t_writer_pitch=w - 1)), ("negative writer pitch", dict(t_writer_pitch=-1)),
             ("sceneColor not 8-byte aligned", dict(t_sceneColor=color.data_ptr() + 4)), ("sceneDepth not 4-byte aligned", dict(t_sceneDepth=depth.data_ptr() + 2)),
             ("writer not 4-byte aligned", dict(t_writer=wr.data_ptr() + 2)),
             ("stride 8", dict(m_strideBytes=8)), ("stride 14", dict(m_strideBytes=14)), ("axes stride 32", dict(A, m_strideBytes=32)), ("axes stride 38", dict(A, m_strideBytes=38)),
             ("indexBits 8", dict(m_indexBits=8)), ("axes indexBits 24", dict(A, m_indexBits=24)),
             ("numIndices not a multiple of 3", dict(m_numIndices=wd.indices.numel() - 1)),
             ("positions not 4-byte aligned", dict(m_positions=wd.positions.data_ptr() + 2)), ("indices not aligned to their size", dict(m_indices=wd.indices.data_ptr() + 2)),
             ("matrices not 4-byte aligned", dict(d_matModelViewProj=wd.matrices.data_ptr() + 2)), ("colour not 4-byte aligned", dict(d_color=wd.color.data_ptr() + 2)),
             ("axes cb not 4-byte aligned", dict(A, d_axes=ad.cb.data_ptr() + 2)),
             ("workBytes one short", dict(wbytes=need - 1)), ("work not aligned", dict(wptr=work.data_ptr() + 16)),
             ("sceneColor inside the work buffer", dict(t_sceneColor=work.data_ptr() + 16)), ("writer inside the work buffer", dict(t_writer=work.data_ptr() + 512)),
             ("sceneDepth inside the work buffer", dict(t_sceneDepth=work.data_ptr() + 256)), ("writer on sceneColor", dict(t_writer=color.data_ptr())),
             ("sceneDepth on sceneColor", dict(t_sceneDepth=color.data_ptr() + 64)), ("sceneDepth on writer", dict(t_sceneDepth=wr.data_ptr()))]
    for label, over in cases:
        assert call(**over) == INV, label
        assert len(lib.vqhip_last_error(hnd) or b"") > 10, label
    assert lib.vqhip_line_draws(None, st, None, 0, w, h, None, None, 0) == INV
    # 2^31 lines: q + 1 no longer fits the fill's 32-bit word
    assert call(m_numIndices=3 * 2 ** 22, d_numInstances=512) == abi.VQHIP_ERR_UNSUPPORTED and len(lib.vqhip_last_error(hnd) or b"") > 10
    assert call(make=axes_draw, m_numIndices=2 ** 30) == abi.VQHIP_ERR_UNSUPPORTED
    assert capi.line_draws_work_bytes(2 ** 31) == 0 and capi.line_draws_work_bytes(2 ** 31 - 1) > 0
    many = (abi.LineDraw * 20001)()
    one = wire_draw()
    one.mesh.numIndices = 3
    for k in range(20001):
        many[k] = one
    big = torch.full((capi.line_draws_work_bytes(3 * 20001),), 0x3C, dtype=torch.uint8, device="cuda")
    tg = targets()
    assert lib.vqhip_line_draws(hnd, st, many, 20001, w, h, C.byref(tg), C.c_void_p(big.data_ptr()), big.numel()) == abi.VQHIP_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert np.array_equal(color.cpu().numpy().view(np.uint16), LC.prefill(w, h)), "a refused call wrote to sceneColor"
    assert (wr == SENT_I).all(), "a refused call wrote to writer"
    assert (work == 0x3C).all() and (big == 0x3C).all(), "a refused call wrote to the work buffer"
    assert call() == abi.VQHIP_OK
    torch.cuda.synchronize()
    ref = L.line_draws(dict(sc, draws=sc["draws"][:1]), LC.prefill(w, h))
    assert_planes("after the refusals", {"scene_color": color.cpu().numpy().view(np.uint16), "writer": wr.cpu().numpy().view(np.uint32)}, ref, w)
    # the Python binding validates before it calls
    half = color.view(torch.float16)
    with pytest.raises(ValueError):
        ctx.line_draws([wd], w, h, half[:, :-1], depth)
    with pytest.raises(ValueError):
        ctx.line_draws([wd], w, h, half, depth[:, :-1])
    with pytest.raises(ValueError):
        ctx.line_draws([capi.WireframeDraw(wd.positions[:, :2], wd.indices, wd.matrices, wd.color)], w, h, half, depth)
    with pytest.raises(ValueError):
        ctx.line_draws([capi.WireframeDraw(wd.positions, wd.indices, wd.matrices, wd.color[:3])], w, h, half, depth)
    with pytest.raises(ValueError):
        ctx.line_draws([capi.VertexAxesDraw(ad.vertices[:, :8], ad.indices, ad.cb)], w, h, half, depth)
    with pytest.raises(ValueError):
        ctx.line_draws([capi.VertexAxesDraw(ad.vertices, ad.indices, ad.cb[:51])], w, h, half, depth)
    with pytest.raises(ValueError):
        ctx.line_draws([object()], w, h, half, depth)
    with pytest.raises(ValueError):
        ctx.line_draws([wd], w, h, half, depth, out={"writer": torch.empty((h, w - 1), dtype=torch.int32, device="cuda")})


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_chain_scene_bounding_volumes_then_composite_reflections(ctx):
    """RenderSceneBoundingVolumes at one sample, on the room at 64 x 40: a zero-cleared plane -> vqhip_line_draws (bounding boxes) -> vqhip_unlit_draws (light
    bounds, opaque) -> vqhip_line_draws (the light bounds as wire, then the vertex axes of one mesh) -> vqhip_outline -> vqhip_composite_reflections, against
    the oracle's composite fed the statements' plane"""
    w, h = 64, 40
    vp = room_view_proj(w, h)
    sphere = S.uv_sphere(1.0, 12, 10)
    cone = (sphere[0] * np.float32(0.5) + np.array([0.0, 0.5, 0.0], dtype=np.float32), sphere[1])
    room = UC.draw(S.room((4.0, 2.0, 4.0)), np.eye(4), vp, UC.AMBER)
    depth = UC.rasterised_depth(w, h, [room])
    boxes = [((-1.5, -0.9, 0.2), (-0.4, 0.3, 1.4)), ((0.2, -1.0, 1.0), (1.6, 0.1, 2.2)), ((-0.3, -0.2, 0.4), (0.4, 0.9, 1.1))]
    box_scene = LC.scene(w, h, [dict(d, kind="wireframe") for d in LS.bounding_box_draws(boxes, vp)], depth)
    solid = UC.scene(w, h, [dict(b, cull=abi.CULL_BACK) for b in US.light_bounds_draws(ROOM_LIGHTS, vp, sphere, cone, blended=False)], depth)
    pos = np.asarray(sphere[0], dtype=np.float32)[:, :3]
    mesh = np.concatenate([pos, pos, np.cross(pos, (0.0, 1.0, 0.3)).astype(np.float32)], axis=1)
    world = S.scaling((0.5, 0.4, 0.5)) @ S.translation((0.0, 0.1, 1.2))
    wire_scene = LC.scene(w, h, [dict(d, kind="wireframe") for d in LS.light_bounds_wire_draws(ROOM_LIGHTS, vp, sphere, cone)] +
                          [dict(d, kind="axes") for d in LS.vertex_axes_draws([(mesh, np.arange(len(mesh)), world)], vp, 0.15)], depth)
    out_scene = OC.cases()["sphere_64x40"]
    # the statements, one after the other on one plane
    plane = np.zeros((h, w, 4), dtype=np.uint16)
    ref1 = L.line_draws(box_scene, plane)
    ref2 = R.unlit_draws(solid, ref1["scene_color"], False)
    ref3 = L.line_draws(wire_scene, ref2["scene_color"])
    ref4 = OR.outline(out_scene, ref3["scene_color"])
    assert (ref1["writer"] != L.NO_WRITER).sum() > 30 and (ref2["writer"] != R.NO_WRITER).sum() > 50
    assert len(np.unique(ref3["writer"])) >= 4 and (ref3["writer"] == len(wire_scene["draws"]) - 1).sum() > 10, "wire bounds and axes both reach the plane"
    # the library
    bv = torch.zeros((h, w, 4), dtype=torch.float16, device="cuda")
    zd = dev(depth)
    ctx.line_draws([device_draw(d) for d in box_scene["draws"]], w, h, bv, zd)
    ctx.unlit_draws([unlit_device_draw(d) for d in solid["draws"]], w, h, bv, zd, blend=False)
    res = ctx.line_draws([device_draw(d) for d in wire_scene["draws"]], w, h, bv, zd)
    torch.cuda.synchronize()
    assert np.array_equal(bv.cpu().numpy().view(np.uint16), ref3["scene_color"]) and np.array_equal(res["writer"].cpu().numpy().view(np.uint32), ref3["writer"])
    from tests.test_gpu_outline import device_draw as outline_device_draw
    ctx.outline([outline_device_draw(d) for d in out_scene["draws"]], w, h, bv)
    torch.cuda.synchronize()
    assert np.array_equal(bv.cpu().numpy().view(np.uint16), ref4["scene_color"])
    from vqengine_amd import synth
    scene_color = synth.hdr_image(w, h, seed=3).astype(np.float16)
    refl = synth.hdr_image(w, h, seed=4, scale=0.5).astype(np.float16)
    want = O.composite_reflections(refl, scene_color, abi.FMT_RGBA16F, ref4["scene_color"].view(np.float16))
    got = ctx.composite_reflections(dev(refl), dev(scene_color), abi.FMT_RGBA16F, bv)
    n, idx = O.bits_equal(got.cpu().numpy(), want)
    assert n == 0, (n, idx)
