"""vqhip_unlit_draws on the GPU (docs/DESIGN_DETAILS.md §7.23 U1 .. U7): scene colour and writer bit for bit against tests/unlit_ref.py, no tolerance, in both
modes, through the Python binding and, for the refusals, the raw C ABI. The scenes are tests/unlit_cases.py's at 16 x 16, 64 x 40 and 129 x 67 (one tile, several
tiles, a partial last tile on both axes); scene colour is prefilled with a recognisable half pattern (non-canonical NaN payloads, infinities, denormals, the largest
finite half) and every untouched pixel must keep its exact bits. The blend is a fold in submission order: the soup puts nine times the fill's queue capacity
into one tile, and the two spheres come in both orders. References are computed once per case and shared; each GPU step runs once."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import oracle_lib as O
from tests import scene_interp_cases as IC
from tests import unlit_cases as UC
from tests import unlit_ref as R
from tests.test_gpu_scene_interp import PLANES, device_draw as surface_device_draw, lights, materials
from vqengine_amd import abi, capi
from vqengine_amd import shadow_scene as S
from vqengine_amd import unlit_scene as US

pytestmark = pytest.mark.gpu
SENT_H, SENT_I = 0x1234, 0x5A5A5A5A
MODES = (("opaque", False), ("blend", True))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_draw(d, bits=32):
    idx = d["indices"]
    ix = dev(idx.astype(np.uint16).view(np.int16)) if bits == 16 else dev(idx.astype(np.int32))
    return capi.UnlitDraw(dev(d["vertices"]), ix, dev(d["cb"]), d["cull"])


def run(ctx, scene, blend, pad=0, writer=True, work=None, stream=None, bits=32):
    """the planes as numpy (uint16 half bits, uint32, float32), each with `pad` sentinel columns behind its rows; the depth plane comes back to show it was not written"""
    w, h = scene["width"], scene["height"]
    color = torch.full((h, w + pad, 4), SENT_H, dtype=torch.int16, device="cuda")
    color[:, :w] = dev(UC.prefill(w, h).view(np.int16).copy())
    depth = torch.full((h, w + pad), -7.0, dtype=torch.float32, device="cuda")
    depth[:, :w] = dev(scene["depth"])
    wr = torch.full((h, w + pad), SENT_I, dtype=torch.int32, device="cuda")
    draws = [device_draw(d, bits) for d in scene["draws"]]
    if stream is not None:
        torch.cuda.synchronize()                                                   # the prefills and uploads ran on the current stream
    ctx.unlit_draws(draws, w, h, color.view(torch.float16)[:, :w], depth[:, :w], blend=blend, writer=writer, out={"writer": wr[:, :w]}, work=work, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return {"scene_color": color.cpu().numpy().view(np.uint16), "writer": wr.cpu().numpy().view(np.uint32), "depth": depth.cpu().numpy()}


def assert_planes(name, got, ref, w, keys=("scene_color", "writer")):
    for k in keys:
        g, e = got[k][:, :w], ref[k]
        bad = np.argwhere(g != e)
        assert len(bad) == 0, f"{name} {k}: {len(bad)} of {e.size} elements differ from tests/unlit_ref.py, first at {bad[0].tolist()}: {g[tuple(bad[0])]:#x} != {e[tuple(bad[0])]:#x}"


def assert_depth_kept(name, got, scene):
    assert np.array_equal(got["depth"][:, :scene["width"]].view(np.uint32), scene["depth"].view(np.uint32)), f"{name}: sceneDepth was written"


@pytest.mark.parametrize("name", sorted(UC.cases()))
def test_case_matches_the_statement(ctx, name):
    """every case at each size, opaque and blended, over the prefilled scene colour: colour (every untouched pixel keeps its prefilled bits, NaN payloads included)
    and writer; sceneDepth keeps its bits"""
    scene = UC.cases()[name]
    w, h = scene["width"], scene["height"]
    for label, blend in MODES:
        got, ref = run(ctx, scene, blend), UC.expected(name, blend)
        assert_planes(f"{name} {label}", got, ref, w)
        assert_depth_kept(f"{name} {label}", got, scene)
        keep = ref["writer"] == R.NO_WRITER
        assert np.array_equal(got["scene_color"][keep], UC.prefill(w, h)[keep])
    if name.startswith("soup"):
        assert UC.expected(name, True)["stats"]["records"] > abi.UNLIT_QUEUE_CAPACITY


def test_both_tile_sizes_give_the_same_bits(ctx, set_opt):
    """every scene at 129 x 67 (at tile 64: three tiles across, two down, the last partial on both axes) and two at 64 x 40, under raster_tile 64 and 32, both modes"""
    for tile in (64, 32):
        set_opt("raster_tile", tile)
        for name in [f"{b}_129x67" for b in UC.BUILDERS] + ["two_spheres_ba_64x40", "soup_64x40"]:
            for label, blend in MODES:
                assert_planes(f"tile {tile} {name} {label}", run(ctx, UC.cases()[name], blend), UC.expected(name, blend), UC.cases()[name]["width"])


def test_pitched_planes_keep_their_padding_and_16_bit_indices(ctx):
    for name, bits, blend in (("soup_129x67", 32, True), ("two_spheres_ab_64x40", 16, True), ("sphere_and_box_129x67", 16, False)):
        scene = UC.cases()[name]
        w = scene["width"]
        got = run(ctx, scene, blend, pad=5, bits=bits)
        assert_planes(f"pitched {name}", got, UC.expected(name, blend), w)
        assert_depth_kept(f"pitched {name}", got, scene)
        assert (got["scene_color"][:, w:] == SENT_H).all() and (got["writer"][:, w:] == SENT_I).all() and (got["depth"][:, w:] == -7.0).all(), f"{name}: padding written"


def test_prefilled_work_buffer_second_call_and_work_size(ctx):
    name = "soup_64x40"
    scene = UC.cases()[name]
    need = capi.unlit_draws_work_bytes(UC.triangles(scene))
    assert need >= UC.triangles(scene) * abi.UNLIT_SLOTS_PER_TRIANGLE * 56
    work = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    for label in ("0xFF-filled work buffer", "second call on the same buffer"):
        assert_planes(f"{name}: {label}", run(ctx, scene, True, work=work[:need]), UC.expected(name, True), 64)
    assert_planes(f"{name}: opaque on the same buffer", run(ctx, scene, False, work=work[:need]), UC.expected(name, False), 64)
    assert (work[need:] == 0xFF).all(), "the call wrote past vqhip_unlit_draws_work_bytes"


def test_non_default_stream(ctx):
    name = "two_spheres_ab_129x67"
    assert_planes("side stream", run(ctx, UC.cases()[name], True, stream=torch.cuda.Stream()), UC.expected(name, True), 129)


def test_writer_null(ctx):
    """writer NULL: scene colour is unchanged by its absence, the tensor is not touched"""
    name = "two_spheres_ab_64x40"
    for label, blend in MODES:
        got = run(ctx, UC.cases()[name], blend, writer=False)
        assert_planes(f"writer NULL {label}", got, UC.expected(name, blend), 64, ("scene_color",))
        assert (got["writer"] == SENT_I).all()


def test_no_draws_clears_writer(ctx):
    w, h = 64, 40
    for label, blend in MODES:
        got = run(ctx, UC.scene(w, h, []), blend, pad=2)
        assert np.array_equal(got["scene_color"][:, :w], UC.prefill(w, h)) and (got["writer"][:, :w] == R.NO_WRITER).all(), label
        assert (got["writer"][:, w:] == SENT_I).all() and (got["scene_color"][:, w:] == SENT_H).all()
    got = run(ctx, UC.scene(w, h, []), True, writer=False)                          # nothing to draw, nothing to clear
    assert np.array_equal(got["scene_color"], UC.prefill(w, h)) and (got["writer"] == SENT_I).all()
    # a list of empty draws is the same call
    sc = UC.cases()["sphere_cull_none_64x40"]
    empty = dict(sc["draws"][0], indices=np.zeros(0, dtype=np.int64))
    got = run(ctx, dict(sc, draws=[empty, empty]), True)
    assert np.array_equal(got["scene_color"], UC.prefill(w, h)) and (got["writer"] == R.NO_WRITER).all()
    # ... and an empty draw in front shifts the writer index, not the picture
    got, ref = run(ctx, dict(sc, draws=[empty] + sc["draws"]), True), UC.expected("sphere_cull_none_64x40", True)
    assert np.array_equal(got["scene_color"], ref["scene_color"])
    assert np.array_equal(got["writer"], np.where(ref["writer"] == R.NO_WRITER, ref["writer"], ref["writer"] + 1))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx):
    name = "sphere_and_box_64x40"
    scene = UC.cases()[name]
    w, h = 64, 40
    dd = device_draw(scene["draws"][0])
    color = dev(UC.prefill(w, h).view(np.int16).copy())
    depth = dev(scene["depth"])
    wr = torch.full((h, w), SENT_I, dtype=torch.int32, device="cuda")
    need = capi.unlit_draws_work_bytes(UC.triangles(scene))
    work = torch.full((max(need, w * h * 8 + 1024),), 0x3C, dtype=torch.uint8, device="cuda")
    lib, hnd, st = ctx.lib, ctx._h, ctx._stream()

    def one_draw():
        draw = abi.UnlitDraw()
        draw.mesh.positions, draw.mesh.strideBytes, draw.mesh.numVertices = dd.positions.data_ptr(), dd.positions.stride(0) * 4, dd.positions.shape[0]
        draw.mesh.indices, draw.mesh.indexBits, draw.mesh.numIndices = dd.indices.data_ptr(), 32, dd.indices.numel()
        draw.cb, draw.cullMode = dd.cb.data_ptr(), abi.CULL_BACK
        return draw

    def targets():
        tg = abi.UnlitTargets()
        tg.sceneColor, tg.sceneDepth, tg.writer = color.data_ptr(), depth.data_ptr(), wr.data_ptr()
        return tg

    def call(ndraws=1, wptr=None, wbytes=None, draws_null=False, out_null=False, width=w, height=h, blend=1, **over):
        draw, tg = one_draw(), targets()
        for k, val in over.items():
            obj, field = {"m": (draw.mesh, k[2:]), "d": (draw, k[2:]), "t": (tg, k[2:])}[k[0]]
            setattr(obj, field, val)
        return lib.vqhip_unlit_draws(hnd, st, None if draws_null else C.pointer(draw), ndraws, width, height, blend, None if out_null else C.byref(tg),
                                     C.c_void_p(work.data_ptr() if wptr is None else wptr), need if wbytes is None else wbytes)
    INV = abi.VQHIP_ERR_INVALID_ARG
    cases = [("NULL draws", dict(draws_null=True)), ("NULL out", dict(out_null=True)), ("NULL sceneColor", dict(t_sceneColor=None)), ("NULL sceneDepth", dict(t_sceneDepth=None)),
             ("NULL work", dict(wptr=0)), ("negative numDraws", dict(ndraws=-1)), ("NULL positions", dict(m_positions=None)), ("NULL indices", dict(m_indices=None)),
             ("NULL cb", dict(d_cb=None)), ("width 0", dict(width=0)), ("height 0", dict(height=0)), ("width above the limit", dict(width=abi.SCENE_DEPTH_MAX_DIM + 1)),
             ("height above the limit", dict(height=abi.SCENE_DEPTH_MAX_DIM + 1)), ("blend 2", dict(blend=2)), ("blend -1", dict(blend=-1)),
             ("targets reserved set", dict(t_reserved=1)), ("draw reserved set", dict(d_reserved=1)), ("cullMode 3", dict(d_cullMode=3)), ("cullMode -1", dict(d_cullMode=-1)),
             ("pitch below the row", dict(t_pitch=w - 1)), ("negative pitch", dict(t_pitch=-w)), ("depth pitch below the row", dict(t_depth_pitch=w - 1)),
             ("negative depth pitch", dict(t_depth_pitch=-1)), ("writer pitch below the row", dict(t_writer_pitch=w - 1)), ("negative writer pitch", dict(t_writer_pitch=-1)),
             ("sceneColor not 8-byte aligned", dict(t_sceneColor=color.data_ptr() + 4)), ("sceneDepth not 4-byte aligned", dict(t_sceneDepth=depth.data_ptr() + 2)),
             ("writer not 4-byte aligned", dict(t_writer=wr.data_ptr() + 2)),
             ("stride 8", dict(m_strideBytes=8)), ("stride 14", dict(m_strideBytes=14)), ("indexBits 8", dict(m_indexBits=8)),
             ("numIndices not a multiple of 3", dict(m_numIndices=dd.indices.numel() - 1)),
             ("positions not 4-byte aligned", dict(m_positions=dd.positions.data_ptr() + 2)), ("indices not aligned to their size", dict(m_indices=dd.indices.data_ptr() + 2)),
             ("cb not 4-byte aligned", dict(d_cb=dd.cb.data_ptr() + 2)),
             ("workBytes one short", dict(wbytes=need - 1)), ("work not aligned", dict(wptr=work.data_ptr() + 16)),
             ("sceneColor inside the work buffer", dict(t_sceneColor=work.data_ptr() + 16)), ("writer inside the work buffer", dict(t_writer=work.data_ptr() + 512)),
             ("sceneDepth inside the work buffer", dict(t_sceneDepth=work.data_ptr() + 256)), ("writer on sceneColor", dict(t_writer=color.data_ptr())),
             ("sceneDepth on sceneColor", dict(t_sceneDepth=color.data_ptr() + 64)), ("sceneDepth on writer", dict(t_sceneDepth=wr.data_ptr()))]
    for label, over in cases:
        assert call(**over) == INV, label
        assert len(lib.vqhip_last_error(hnd) or b"") > 10, label
    assert lib.vqhip_unlit_draws(None, st, None, 0, w, h, 0, None, None, 0) == INV
    # 2^28 triangles: eight slots each no longer fit a 32-bit slot number
    assert call(m_numIndices=3 * 2 ** 28) == abi.VQHIP_ERR_UNSUPPORTED and len(lib.vqhip_last_error(hnd) or b"") > 10
    assert capi.unlit_draws_work_bytes(2 ** 28) == 0 and capi.unlit_draws_work_bytes(2 ** 28 - 1) > 0
    many = (abi.UnlitDraw * 20001)()
    one = one_draw()
    one.mesh.numIndices = 3
    for k in range(20001):
        many[k] = one
    big = torch.full((capi.unlit_draws_work_bytes(20001),), 0x3C, dtype=torch.uint8, device="cuda")
    tg = targets()
    assert lib.vqhip_unlit_draws(hnd, st, many, 20001, w, h, 1, C.byref(tg), C.c_void_p(big.data_ptr()), big.numel()) == abi.VQHIP_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert np.array_equal(color.cpu().numpy().view(np.uint16), UC.prefill(w, h)), "a refused call wrote to sceneColor"
    assert (wr == SENT_I).all(), "a refused call wrote to writer"
    assert (work == 0x3C).all() and (big == 0x3C).all(), "a refused call wrote to the work buffer"
    assert call() == abi.VQHIP_OK
    torch.cuda.synchronize()
    assert_planes("after the refusals", {"scene_color": color.cpu().numpy().view(np.uint16), "writer": wr.cpu().numpy().view(np.uint32)}, UC.expected(name, True), w)
    # the Python binding validates before it calls
    half = color.view(torch.float16)
    with pytest.raises(ValueError):
        ctx.unlit_draws([dd], w, h, half[:, :-1], depth)
    with pytest.raises(ValueError):
        ctx.unlit_draws([dd], w, h, half, depth[:, :-1])
    with pytest.raises(ValueError):
        ctx.unlit_draws([capi.UnlitDraw(dd.positions[:, :2], dd.indices, dd.cb)], w, h, half, depth)
    with pytest.raises(ValueError):
        ctx.unlit_draws([capi.UnlitDraw(dd.positions, dd.indices, dd.cb[:19])], w, h, half, depth)
    with pytest.raises(ValueError):
        ctx.unlit_draws([capi.UnlitDraw(dd.positions, dd.indices, dd.cb, 7)], w, h, half, depth)
    with pytest.raises(ValueError):
        ctx.unlit_draws([dd], w, h, half, depth, out={"writer": torch.empty((h, w - 1), dtype=torch.int32, device="cuda")})


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------------------------
ROOM_LIGHTS = ({"type": "point", "position": (-1.0, 0.6, 0.5), "color": (1.0, 0.8, 0.3), "brightness": 40.0, "range": 1.2},
               {"type": "spot", "position": (1.4, 0.5, 1.5), "color": (0.0, 0.4, 1.0), "brightness": 90.0, "range": 1.5, "outer_cone_degrees": 25.0},
               {"type": "directional", "position": (0.0, 5.0, 0.0), "color": (1.0, 1.0, 1.0), "brightness": 3.0, "range": 100.0},
               {"type": "point", "position": (0.3, -0.4, 1.5), "color": (0.2, 1.0, 0.2), "brightness": 15.0, "range": 1.0})


GIZMO_RADIUS = 3.0               # x Light::GetWorldTransformationMatrix's 0.1: large enough to cover pixels at 64 x 40


def room_view_proj(w, h):
    return S.look_at_lh(IC.ROOM_EYE, IC.ROOM_AT, (0.0, 1.0, 0.0)) @ S.perspective_fov_lh(np.radians(70.0), w / h, 0.1, 15.0)


def test_chain_lit_frame_then_light_gizmos(ctx):
    """room, 64 x 40: meshes -> vqhip_scene_depth -> vqhip_scene_interpolants -> vqhip_forward_lighting_from_materials -> vqhip_unlit_draws with the light gizmos of
    unlit_scene.light_mesh_draws (scaled up to be seen at this size), opaque, against the depth the library rasterised: the lit pixels change exactly where
    writer != 0xFFFFFFFF, and the frame equals the statement's over the same depth"""
    scene = IC.cases()["room_64x40_s1"]
    w, h = 64, 40
    draws = [surface_device_draw(d) for d in scene["draws"]]
    z = ctx.scene_depth([d.depth_draw() for d in draws], w, h, 1, primitive=True)
    ip = ctx.scene_interpolants(draws, w, h, z["primitive"])
    hmats, dmats, keep = materials(ctx)
    pf, extra, pv = lights(w, h)
    lit = ctx.forward_lighting_from_materials([ip[k] for k in PLANES[:3]], dmats, pf, pv, extra_point=extra)
    torch.cuda.synchronize()
    before = lit.cpu().numpy().view(np.uint16).copy()
    depth = z["depth"].cpu().numpy().reshape(h, w)
    gizmos = US.light_mesh_draws(ROOM_LIGHTS, IC.ROOM_EYE, room_view_proj(w, h), S.uv_sphere(GIZMO_RADIUS, 10, 8))
    assert [g["light"] for g in gizmos] == [0, 1, 3]
    sc = UC.scene(w, h, [dict(g, cull=abi.CULL_BACK) for g in gizmos], depth)
    res = ctx.unlit_draws([device_draw(d) for d in sc["draws"]], w, h, lit, z["depth"].view(h, w), blend=False)
    torch.cuda.synchronize()
    after = lit.cpu().numpy().view(np.uint16)
    ref = R.unlit_draws(sc, before, False)
    writer = res["writer"].cpu().numpy().view(np.uint32)
    assert np.array_equal(writer, ref["writer"])
    written = writer != R.NO_WRITER
    assert written.sum() > 10 and len(np.unique(writer[written])) >= 2
    assert np.array_equal(after[~written], before[~written]), "a pixel outside the gizmos changed"
    assert (after[written] != before[written]).any(axis=-1).all(), "a gizmo pixel kept the lit colour"
    assert np.array_equal(after, ref["scene_color"])


def test_chain_light_bounds_then_composite_reflections(ctx):
    """a zero-cleared plane -> vqhip_unlit_draws with the light bounds of unlit_scene.light_bounds_draws, opaque (the reflections-on path: the cleared
    Tex_SceneColorBoundingVolumes) -> vqhip_composite_reflections, against the oracle's composite fed the statement's plane"""
    w, h = 64, 40
    vp = room_view_proj(w, h)
    sphere = S.uv_sphere(1.0, 12, 10)
    cone = (sphere[0] * np.float32(0.5) + np.array([0.0, 0.5, 0.0], dtype=np.float32), sphere[1])          # a stand-in for the engine's unit cone
    bounds = US.light_bounds_draws(ROOM_LIGHTS, vp, sphere, cone, blended=False)
    assert [b["light"] for b in bounds] == [0, 1, 3]
    room = UC.draw(S.room((4.0, 2.0, 4.0)), np.eye(4), vp, UC.AMBER)
    sc = UC.scene(w, h, [dict(b, cull=abi.CULL_BACK) for b in bounds], UC.rasterised_depth(w, h, [room]))
    zero = np.zeros((h, w, 4), dtype=np.uint16)
    ref = R.unlit_draws(sc, zero, False)
    assert (ref["writer"] != R.NO_WRITER).sum() > 50 and len(np.unique(ref["writer"])) == 4
    bv = torch.zeros((h, w, 4), dtype=torch.float16, device="cuda")
    res = ctx.unlit_draws([device_draw(d) for d in sc["draws"]], w, h, bv, dev(sc["depth"]), blend=False)
    torch.cuda.synchronize()
    assert np.array_equal(bv.cpu().numpy().view(np.uint16), ref["scene_color"]) and np.array_equal(res["writer"].cpu().numpy().view(np.uint32), ref["writer"])
    from vqengine_amd import synth
    scene_color = synth.hdr_image(w, h, seed=3).astype(np.float16)
    refl = synth.hdr_image(w, h, seed=4, scale=0.5).astype(np.float16)
    want = O.composite_reflections(refl, scene_color, abi.FMT_RGBA16F, ref["scene_color"].view(np.float16))
    got = ctx.composite_reflections(dev(refl), dev(scene_color), abi.FMT_RGBA16F, bv)
    n, idx = O.bits_equal(got.cpu().numpy(), want)
    assert n == 0, (n, idx)
