"""vqhip_outline on the GPU (docs/DESIGN_DETAILS.md §7.21 O1 .. O6): scene colour, selection and writer bit for bit against tests/outline_ref.py, no tolerance,
through the Python binding and, for the refusals, the raw C ABI. The scenes are tests/outline_cases.py's at 16 x 16, 64 x 40 and 129 x 67 (one tile, several
tiles, a partial last tile on both axes); scene colour is prefilled with a recognisable half pattern (non-canonical NaN payloads included) and every unwritten
pixel must keep its exact bits. References are computed once per case and shared; each GPU step runs once."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import outline_cases as OC
from tests import outline_ref as R
from tests import scene_interp_cases as IC
from tests import shadow_raster_cases as K
from tests.test_gpu_scene_interp import PLANES, device_draw as surface_device_draw, lights, materials
from vqengine_amd import abi, capi
from vqengine_amd import outline_scene as OS
from vqengine_amd import shadow_scene as S
from vqengine_amd import surface_scene as SS

pytestmark = pytest.mark.gpu
SENT_H, SENT_B, SENT_I = 0x1234, 0xA5, 0x5A5A5A5A


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_draw(d, bits=32):
    idx = d["indices"]
    ix = dev(idx.astype(np.uint16).view(np.int16)) if bits == 16 else dev(idx.astype(np.int32))
    return capi.OutlineDraw(dev(d["vertices"]), ix, dev(d["cb"]))


def run(ctx, scene, pad=0, selection=True, writer=True, work=None, stream=None, bits=32, prefill=None):
    """the three planes as numpy (uint16 half bits, uint8, uint32), each with `pad` sentinel columns behind its rows"""
    w, h = scene["width"], scene["height"]
    color = torch.full((h, w + pad, 4), SENT_H, dtype=torch.int16, device="cuda")
    color[:, :w] = dev((OC.prefill(w, h) if prefill is None else prefill).view(np.int16))
    back = {"selection": torch.full((h, w + pad), SENT_B, dtype=torch.uint8, device="cuda"), "writer": torch.full((h, w + pad), SENT_I, dtype=torch.int32, device="cuda")}
    draws = [device_draw(d, bits) for d in scene["draws"]]
    if stream is not None:
        torch.cuda.synchronize()                                                   # the prefills and uploads ran on the current stream
    ctx.outline(draws, w, h, color.view(torch.float16)[:, :w], selection=selection, writer=writer, out={k: t[:, :w] for k, t in back.items()}, work=work, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return {"scene_color": color.cpu().numpy().view(np.uint16), "selection": back["selection"].cpu().numpy(), "writer": back["writer"].cpu().numpy().view(np.uint32)}


def assert_planes(name, got, ref, w, keys=("scene_color", "selection", "writer")):
    for k in keys:
        g, e = got[k][:, :w], ref[k]
        bad = np.argwhere(g != e)
        assert len(bad) == 0, f"{name} {k}: {len(bad)} of {e.size} elements differ from tests/outline_ref.py, first at {bad[0].tolist()}: {g[tuple(bad[0])]:#x} != {e[tuple(bad[0])]:#x}"


@pytest.mark.parametrize("name", sorted(OC.cases()))
def test_case_matches_the_statement(ctx, name):
    """the sphere, the two overlapping boxes, the two colours in both orders and the 2 000-triangle soup with random normals across all seven planes, at each size:
    scene colour (every unwritten pixel keeps its prefilled bits, NaN payloads included), selection, writer"""
    scene = OC.cases()[name]
    got = run(ctx, scene)
    ref = OC.expected(name)
    assert_planes(name, got, ref, scene["width"])
    keep = ref["writer"] == R.NO_WRITER
    assert np.array_equal(got["scene_color"][keep], OC.prefill(scene["width"], scene["height"])[keep]) and (~keep).any()


def test_both_tile_sizes_give_the_same_bits(ctx, set_opt):
    """every scene at 129 x 67 (at tile 64: three tiles across, two down, the last partial on both axes) and one at 64 x 40, under raster_tile 64 and 32"""
    for tile in (64, 32):
        set_opt("raster_tile", tile)
        for name in [f"{b}_129x67" for b in OC.BUILDERS] + ["two_colours_ba_64x40"]:
            assert_planes(f"tile {tile} {name}", run(ctx, OC.cases()[name]), OC.expected(name), OC.cases()[name]["width"])


def test_pitched_outputs_keep_their_padding_and_16_bit_indices(ctx):
    for name, bits in (("soup_129x67", 32), ("two_boxes_64x40", 16)):
        scene = OC.cases()[name]
        w = scene["width"]
        got = run(ctx, scene, pad=5, bits=bits)
        assert_planes(f"pitched {name}", got, OC.expected(name), w)
        assert (got["scene_color"][:, w:] == SENT_H).all() and (got["selection"][:, w:] == SENT_B).all() and (got["writer"][:, w:] == SENT_I).all(), f"{name}: padding written"


def test_prefilled_work_buffer_second_call_and_work_size(ctx):
    name = "soup_64x40"
    scene = OC.cases()[name]
    need = capi.outline_work_bytes(OC.triangles(scene))
    work = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    for label in ("0xFF-filled work buffer", "second call on the same buffer"):
        assert_planes(f"{name}: {label}", run(ctx, scene, work=work[:need]), OC.expected(name), 64)
    assert (work[need:] == 0xFF).all(), "the call wrote past vqhip_outline_work_bytes"


def test_non_default_stream(ctx):
    name = "two_boxes_129x67"
    assert_planes("side stream", run(ctx, OC.cases()[name], stream=torch.cuda.Stream()), OC.expected(name), 129)


def test_optional_planes(ctx):
    """selection and writer NULL, each alone and both: scene colour and the plane that is left are unchanged, the missing plane's tensor is not touched"""
    name = "two_colours_ab_64x40"
    scene, ref = OC.cases()[name], OC.expected(name)
    for sel, wr in ((False, True), (True, False), (False, False)):
        got = run(ctx, scene, selection=sel, writer=wr)
        assert_planes(f"selection={sel} writer={wr}", got, ref, 64, ("scene_color",) + (("selection",) if sel else ()) + (("writer",) if wr else ()))
        assert sel or (got["selection"] == SENT_B).all()
        assert wr or (got["writer"] == SENT_I).all()


def test_no_draws_clears_selection_and_writer(ctx):
    w, h = 64, 40
    got = run(ctx, {"width": w, "height": h, "draws": []}, pad=2)
    assert np.array_equal(got["scene_color"][:, :w], OC.prefill(w, h)) and (got["selection"][:, :w] == 0).all() and (got["writer"][:, :w] == R.NO_WRITER).all()
    assert (got["selection"][:, w:] == SENT_B).all() and (got["writer"][:, w:] == SENT_I).all()
    # a list of empty draws is the same call
    sc = OC.cases()["sphere_64x40"]
    empty = dict(sc["draws"][0], indices=np.zeros(0, dtype=np.int64))
    got = run(ctx, {"width": w, "height": h, "draws": [empty, empty]})
    assert np.array_equal(got["scene_color"], OC.prefill(w, h)) and (got["selection"] == 0).all() and (got["writer"] == R.NO_WRITER).all()
    # ... and an empty draw in front shifts the writer index, not the picture
    got = run(ctx, {"width": w, "height": h, "draws": [empty] + sc["draws"]})
    ref = OC.expected("sphere_64x40")
    assert np.array_equal(got["scene_color"], ref["scene_color"]) and np.array_equal(got["selection"], ref["selection"])
    assert np.array_equal(got["writer"], np.where(ref["writer"] == R.NO_WRITER, ref["writer"], ref["writer"] + 1))


def test_colour_bits(ctx):
    """Color components 0, 1, 0.5, a denormal and a negative one (NaN by the contract): the bits of vqo_pow and one RNE half conversion"""
    sc = OC.cases()["sphere_16x16"]
    for color in ((0.0, 1.0, 0.5, 1e-40), (-0.5, 0.25, 2.0, 70000.0), (float("inf"), -0.0, 0.9999, 3.0e-5)):
        d = dict(sc["draws"][0])
        d["cb"] = d["cb"].copy()
        d["cb"][R.CB_COLOR:R.CB_COLOR + 4] = np.asarray(color, dtype=np.float32)
        scene = dict(sc, draws=[d])
        got, ref = run(ctx, scene), R.outline(scene, OC.prefill(16, 16))
        assert_planes(f"colour {color}", got, ref, 16)
        assert (ref["writer"] == 0).sum() > 10
    assert R.colour_halfs((0.0, 1.0, 0.5, -1.0)).tolist()[:2] == [0x0000, 0x3C00] and (R.colour_halfs((0.0, 1.0, 0.5, -1.0))[3] & 0x7FFF) == 0x7E00


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx):
    name = "sphere_64x40"
    scene = OC.cases()[name]
    w, h = 64, 40
    dd = device_draw(scene["draws"][0])
    color = dev(OC.prefill(w, h).view(np.int16))
    sel = torch.full((h, w), SENT_B, dtype=torch.uint8, device="cuda")
    wr = torch.full((h, w), SENT_I, dtype=torch.int32, device="cuda")
    need = capi.outline_work_bytes(OC.triangles(scene))
    work = torch.full((need,), 0x3C, dtype=torch.uint8, device="cuda")
    lib, hnd, st = ctx.lib, ctx._h, ctx._stream()

    def call(ndraws=1, wptr=None, wbytes=None, draws_null=False, out_null=False, width=w, height=h, **over):
        draw = abi.OutlineDraw()
        draw.mesh.positions, draw.mesh.strideBytes, draw.mesh.numVertices = dd.vertices.data_ptr(), dd.vertices.stride(0) * 4, dd.vertices.shape[0]
        draw.mesh.indices, draw.mesh.indexBits, draw.mesh.numIndices = dd.indices.data_ptr(), 32, dd.indices.numel()
        draw.cb = dd.cb.data_ptr()
        tg = abi.OutlineTargets()
        tg.sceneColor, tg.selection, tg.writer = color.data_ptr(), sel.data_ptr(), wr.data_ptr()
        for k, val in over.items():
            obj, field = {"m": (draw.mesh, k[2:]), "d": (draw, k[2:]), "t": (tg, k[2:])}[k[0]]
            setattr(obj, field, val)
        return lib.vqhip_outline(hnd, st, None if draws_null else C.pointer(draw), ndraws, width, height, None if out_null else C.byref(tg),
                                 C.c_void_p(work.data_ptr() if wptr is None else wptr), work.numel() if wbytes is None else wbytes)
    INV = abi.VQHIP_ERR_INVALID_ARG
    cases = [("NULL draws", dict(draws_null=True)), ("NULL out", dict(out_null=True)), ("NULL sceneColor", dict(t_sceneColor=None)), ("NULL work", dict(wptr=0)),
             ("negative numDraws", dict(ndraws=-1)), ("NULL positions", dict(m_positions=None)), ("NULL indices", dict(m_indices=None)), ("NULL cb", dict(d_cb=None)),
             ("width 0", dict(width=0)), ("height 0", dict(height=0)), ("width above the limit", dict(width=abi.SCENE_DEPTH_MAX_DIM + 1)),
             ("height above the limit", dict(height=abi.SCENE_DEPTH_MAX_DIM + 1)), ("reserved set", dict(t_reserved=1)),
             ("pitch below the row", dict(t_pitch=w - 1)), ("negative pitch", dict(t_pitch=-w)), ("selection pitch below the row", dict(t_selection_pitch=w - 1)),
             ("negative selection pitch", dict(t_selection_pitch=-1)), ("writer pitch below the row", dict(t_writer_pitch=w - 1)), ("negative writer pitch", dict(t_writer_pitch=-1)),
             ("sceneColor not 8-byte aligned", dict(t_sceneColor=color.data_ptr() + 4)), ("writer not 4-byte aligned", dict(t_writer=wr.data_ptr() + 2)),
             ("stride 20", dict(m_strideBytes=20)), ("stride 26", dict(m_strideBytes=26)), ("stride 12", dict(m_strideBytes=12)), ("indexBits 8", dict(m_indexBits=8)),
             ("numIndices not a multiple of 3", dict(m_numIndices=dd.indices.numel() - 1)),
             ("positions not 4-byte aligned", dict(m_positions=dd.vertices.data_ptr() + 2)), ("indices not aligned to their size", dict(m_indices=dd.indices.data_ptr() + 2)),
             ("cb not 4-byte aligned", dict(d_cb=dd.cb.data_ptr() + 2)),
             ("workBytes one short", dict(wbytes=need - 1)), ("work not aligned", dict(wptr=work.data_ptr() + 16)),
             ("sceneColor inside the work buffer", dict(t_sceneColor=work.data_ptr() + 16)), ("selection inside the work buffer", dict(t_selection=work.data_ptr() + 300)),
             ("writer inside the work buffer", dict(t_writer=work.data_ptr() + 512)), ("selection on sceneColor", dict(t_selection=color.data_ptr() + 100)),
             ("writer on sceneColor", dict(t_writer=color.data_ptr())), ("writer on selection", dict(t_writer=sel.data_ptr()))]
    for label, over in cases:
        assert call(**over) == INV, label
        assert len(lib.vqhip_last_error(hnd) or b"") > 10, label
    # 2^28 triangles: sixteen records each no longer fit the 32-bit counter
    assert call(m_numIndices=3 * 2 ** 28) == abi.VQHIP_ERR_UNSUPPORTED and len(lib.vqhip_last_error(hnd) or b"") > 10
    many = (abi.OutlineDraw * 20001)()
    one = abi.OutlineDraw()
    one.mesh.positions, one.mesh.strideBytes, one.mesh.numVertices = dd.vertices.data_ptr(), dd.vertices.stride(0) * 4, dd.vertices.shape[0]
    one.mesh.indices, one.mesh.indexBits, one.mesh.numIndices, one.cb = dd.indices.data_ptr(), 32, 3, dd.cb.data_ptr()
    for k in range(20001):
        many[k] = one
    big = torch.full((capi.outline_work_bytes(20001),), 0x3C, dtype=torch.uint8, device="cuda")
    tg = abi.OutlineTargets()
    tg.sceneColor, tg.selection, tg.writer = color.data_ptr(), sel.data_ptr(), wr.data_ptr()
    assert lib.vqhip_outline(hnd, st, many, 20001, w, h, C.byref(tg), C.c_void_p(big.data_ptr()), big.numel()) == abi.VQHIP_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert np.array_equal(color.cpu().numpy().view(np.uint16), OC.prefill(w, h)), "a refused call wrote to sceneColor"
    assert (sel == SENT_B).all() and (wr == SENT_I).all(), "a refused call wrote to selection / writer"
    assert (work == 0x3C).all() and (big == 0x3C).all(), "a refused call wrote to the work buffer"
    assert call() == abi.VQHIP_OK
    torch.cuda.synchronize()
    assert_planes("after the refusals", {"scene_color": color.cpu().numpy().view(np.uint16), "selection": sel.cpu().numpy(), "writer": wr.cpu().numpy().view(np.uint32)},
                  OC.expected(name), w)
    # the Python binding validates before it calls
    half = color.view(torch.float16)
    with pytest.raises(ValueError):
        ctx.outline([dd], w, h, half[:, :-1])
    with pytest.raises(ValueError):
        ctx.outline([capi.OutlineDraw(dd.vertices[:, :5], dd.indices, dd.cb)], w, h, half)
    with pytest.raises(ValueError):
        ctx.outline([capi.OutlineDraw(dd.vertices, dd.indices, dd.cb[:91])], w, h, half)
    with pytest.raises(ValueError):
        ctx.outline([dd], w, h, half, out={"writer": torch.empty((h, w - 1), dtype=torch.int32, device="cuda")})


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_chain_lit_frame_then_outline(ctx):
    """room, 64 x 40: meshes -> vqhip_scene_depth -> vqhip_scene_interpolants -> vqhip_forward_lighting_from_materials -> vqhip_outline with one occluder box
    selected: the lit pixels equal the frame without the outline call except exactly at writer != 0xFFFFFFFF, and there they equal the colour halfs"""
    name = "room_64x40_s1"
    scene = IC.cases()[name]
    w, h = 64, 40
    draws = [surface_device_draw(d) for d in scene["draws"]]
    z = ctx.scene_depth([d.depth_draw() for d in draws], w, h, 1, primitive=True)
    ip = ctx.scene_interpolants(draws, w, h, z["primitive"])
    hmats, dmats, keep = materials(ctx)
    pf, extra, pv = lights(w, h)
    lit = ctx.forward_lighting_from_materials([ip[k] for k in PLANES[:3]], dmats, pf, pv, extra_point=extra)
    torch.cuda.synchronize()
    before = lit.cpu().numpy().view(np.uint16).copy()
    assert before.shape == (h, w, 4)
    centre, half = K.OCCLUDERS[3]
    world = S.scaling(half) @ S.rotation_y(0.3 * 3) @ S.translation(centre)         # the fourth occluder of tests/scene_interp_cases.room_scene
    view = S.look_at_lh(IC.ROOM_EYE, IC.ROOM_AT, (0.0, 1.0, 0.0))
    proj = S.perspective_fov_lh(np.radians(70.0), w / h, 0.1, 15.0)
    bv, bi = SS.box((1.0, 1.0, 1.0))
    sel = {"vertices": bv, "indices": bi, "cb": OS.outline_data(world, view, proj, OC.GREEN)}
    res = ctx.outline([device_draw(sel)], w, h, lit)
    torch.cuda.synchronize()
    after = lit.cpu().numpy().view(np.uint16)
    ref = R.outline({"width": w, "height": h, "draws": [sel]}, before)
    writer = res["writer"].cpu().numpy().view(np.uint32)
    assert np.array_equal(writer, ref["writer"]) and np.array_equal(res["selection"].cpu().numpy(), ref["selection"])
    written = writer != R.NO_WRITER
    assert written.sum() > 20 and ref["selection"].sum() > 20
    assert np.array_equal(after[~written], before[~written]), "a pixel outside the outline changed"
    assert (after[written] == R.colour_halfs(OC.GREEN)).all()
    assert np.array_equal(after, ref["scene_color"])
