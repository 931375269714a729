"""vqhip_scene_depth on the GPU (docs/DESIGN_DETAILS.md §7.17): every output bit for bit against tests/scene_depth_ref.py, no tolerance, through the Python binding
and, for the refusals, the raw C ABI. The scenes are tests/scene_depth_cases.py's at the smallest sizes that can still go wrong: 16 x 16, 64 x 40 (two tiles
across, a partial tile down) and 129 x 67 (partial tiles both ways, non-square). References are computed once per case and shared; each GPU step runs once.
The chains at the end feed the outputs into the stages that consume them: the MSAA depth resolve with its hierarchy, the 4x lit resolve, the 1x hierarchy."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import depth_ref
from tests import msaa_ref
from tests import oracle_lib as O
from tests import scene_depth_cases as SC
from tests import scene_depth_ref as V
from vqengine_amd import abi, capi, synth

pytestmark = pytest.mark.gpu

SENT_F, SENT_I, SENT_B = -7.0, 0x5A5A5A5A, 0xA5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_draw(d):
    idx = d["indices"]
    ix = dev(idx.astype(np.uint16).view(np.int16)) if d["bits"] == 16 else dev(idx.astype(np.int32))
    return capi.ShadowDraw(dev(d["positions"]), ix, dev(d["wvp"]), None, d["cull"])


def targets(scene, layers, pad=0, cov_pad=0):
    """prefilled backing tensors, wider than the target by the pads, and the views of them handed to the call"""
    w, h, s = scene["width"], scene["height"], scene["samples"]
    px = () if s == 1 else (4,)
    back = {"depth": torch.full((h, w + pad) + px, SENT_F, dtype=torch.float32, device="cuda"),
            "primitive": torch.full((h, w + pad) + px, SENT_I, dtype=torch.int32, device="cuda")}
    if layers:
        back["coverage"] = [torch.full((h, w + cov_pad), SENT_B, dtype=torch.uint8, device="cuda") for _ in range(layers)]
        back["layer_primitive"] = [torch.full((h, w + pad), SENT_I, dtype=torch.int32, device="cuda") for _ in range(layers)]
    out = {k: ([t[:, :w] for t in v] if isinstance(v, list) else v[:, :w]) for k, v in back.items()}
    return back, out


def run(ctx, scene, layers=None, pad=0, cov_pad=0, work=None, stream=None):
    layers = (4 if scene["samples"] == 4 else 0) if layers is None else layers
    back, out = targets(scene, layers, pad, cov_pad)
    ctx.scene_depth([device_draw(d) for d in scene["draws"]], scene["width"], scene["height"], scene["samples"], primitive=True, layers=layers, out=out,
                    work=work, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return {k: ([t.cpu().numpy() for t in v] if isinstance(v, list) else v.cpu().numpy()) for k, v in back.items()}


def assert_same(name, got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    if got.dtype == np.int32:
        got = got.view(np.uint32)
    n_bad, idx = O.bits_equal(got, ref)
    assert n_bad == 0, f"{name}: {n_bad} of {ref.size} elements differ from tests/scene_depth_ref.py, first at {idx.tolist()}"


def assert_outputs(name, got, e, w, layers=None):
    assert_same(f"{name} depth", got["depth"][:, :w], e["depth"])
    assert_same(f"{name} primitive", got["primitive"][:, :w], e["primitive"])
    n = len(got.get("coverage", ())) if layers is None else layers
    for k in range(n):
        assert_same(f"{name} coverage[{k}]", got["coverage"][k][:, :w], e["coverage"][k])
        assert_same(f"{name} layerPrimitive[{k}]", got["layer_primitive"][k][:, :w], e["layer_primitive"][k])


@pytest.mark.parametrize("name", sorted(SC.cases()))
def test_case_matches_the_statement(ctx, name):
    """rules, soup (all seven planes), instanced boxes (16-bit indices, 44-byte stride), the room from inside and the equal-depth pair in both draw orders, at each
    size and both sample counts: depth, primitive, all four masks and all four layerPrimitive planes"""
    scene = SC.cases()[name]
    assert_outputs(name, run(ctx, scene), SC.expected(name), scene["width"])


def test_equal_depth_goes_to_the_first_submitted(ctx):
    for s in (1, 4):
        ab, ba = run(ctx, SC.cases()[f"pair_ab_64x40_s{s}"]), run(ctx, SC.cases()[f"pair_ba_64x40_s{s}"])
        shared = ab["primitive"].view(np.uint32) == 0                          # the samples of the shared triangle: q(A) = 0 in the order A, B
        assert shared.sum() > 100 * s and (ba["primitive"].view(np.uint32)[shared] == 1).all()      # q(B's copy) = 1 in the order B, A; A's copy is 2
        assert np.array_equal(ab["depth"].view(np.uint32)[shared], ba["depth"].view(np.uint32)[shared])


def test_both_tile_sizes_give_the_same_bits(ctx, set_opt):
    """raster_tile 64 is honoured at 1 sample; at 4 samples the tile stays 32 (the LDS budget) and the option changes nothing"""
    for tile in (64, 32):
        set_opt("raster_tile", tile)
        for name in ("soup_129x67_s1", "room_129x67_s1", "soup_129x67_s4"):
            assert_outputs(f"tile {tile} {name}", run(ctx, SC.cases()[name]), SC.expected(name), 129)


def test_pitched_outputs_keep_their_padding(ctx):
    for name in ("soup_129x67_s1", "soup_129x67_s4", "room_64x40_s4"):
        scene = SC.cases()[name]
        w = scene["width"]
        got = run(ctx, scene, pad=5, cov_pad=3)
        assert_outputs(f"pitched {name}", got, SC.expected(name), w)
        assert (got["depth"][:, w:] == SENT_F).all() and (got["primitive"][:, w:] == SENT_I).all(), f"{name}: the padding of depth / primitive was written"
        for k in range(len(got.get("coverage", ()))):
            assert (got["coverage"][k][:, w:] == SENT_B).all() and (got["layer_primitive"][k][:, w:] == SENT_I).all(), f"{name}: the padding of layer {k} was written"


def test_prefilled_work_buffer_second_call_and_work_size(ctx):
    for name in ("soup_129x67_s4", "soup_64x40_s1"):
        scene = SC.cases()[name]
        need = capi.scene_depth_work_bytes(V.instanced_triangles(scene))
        work = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device="cuda")
        for label in ("0xFF-filled work buffer", "second call on the same buffer"):
            assert_outputs(f"{name}: {label}", run(ctx, scene, work=work[:need]), SC.expected(name), scene["width"])
        assert (work[need:] == 0xFF).all(), "the call wrote past vqhip_scene_depth_work_bytes"


def test_non_default_stream(ctx):
    s = torch.cuda.Stream()
    name = "boxes_64x40_s4"
    assert_outputs("side stream", run(ctx, SC.cases()[name], stream=s), SC.expected(name), 64)


def test_depth_alone_and_fewer_layers(ctx):
    name = "soup_64x40_s4"
    scene, e = SC.cases()[name], SC.expected(name)
    draws = [device_draw(d) for d in scene["draws"]]
    for s_name in ("soup_64x40_s1", name):
        sc = SC.cases()[s_name]
        res = ctx.scene_depth(draws, 64, 40, sc["samples"])
        torch.cuda.synchronize()
        assert set(res) == {"depth", "work"}
        assert_same(f"{s_name}: depth alone", res["depth"].cpu().numpy(), SC.expected(s_name)["depth"])
    # two layers asked for where pixels have three and four owners: the planes are the first two of the four, depth and primitive do not change
    assert ((e["coverage"][2] != 0).sum() > 0) and ((e["coverage"][3] != 0).sum() > 0)
    got = run(ctx, scene, layers=2)
    assert_outputs("two layers", got, e, 64, layers=2)
    # masks without their primitives
    res = ctx.scene_depth(draws, 64, 40, 4, layers=3, layer_primitive=False)
    torch.cuda.synchronize()
    assert "layer_primitive" not in res
    for k in range(3):
        assert_same(f"coverage[{k}] without layerPrimitive", res["coverage"][k].cpu().numpy(), e["coverage"][k])


def test_no_draws_clears_every_output(ctx):
    for s in (1, 4):
        got = run(ctx, SC.scene(33, 9, s, []))
        assert (got["depth"] == 1.0).all() and (got["primitive"].view(np.uint32) == V.NO_PRIMITIVE).all()
        for k in range(len(got.get("coverage", ()))):
            assert (got["coverage"][k] == 0).all() and (got["layer_primitive"][k].view(np.uint32) == V.NO_PRIMITIVE).all()


def test_refusals_launch_nothing(ctx):
    name = "boxes_64x40_s4"
    scene = SC.cases()[name]
    d = scene["draws"][0]
    dd = device_draw(d)
    w, h = 64, 40
    back, out = targets(scene, 4)
    need = capi.scene_depth_work_bytes(V.instanced_triangles(scene))
    work = torch.full((need,), 0x3C, dtype=torch.uint8, device="cuda")
    lib, hnd, st = ctx.lib, ctx._h, ctx._stream()

    def call(ndraws=1, wptr=None, wbytes=None, draws_null=False, out_null=False, width=w, height=h, samples=4, **over):
        draw = abi.SceneDepthDraw()
        draw.mesh.positions, draw.mesh.strideBytes, draw.mesh.numVertices = dd.positions.data_ptr(), dd.positions.stride(0) * 4, dd.positions.shape[0]
        draw.mesh.indices, draw.mesh.indexBits, draw.mesh.numIndices = dd.indices.data_ptr(), d["bits"], dd.indices.numel()
        draw.matWorldViewProj, draw.numInstances, draw.cullMode = dd.wvp.data_ptr(), dd.wvp.shape[0], d["cull"]
        tg = abi.SceneDepthTargets()
        tg.depth, tg.primitive, tg.layers = back["depth"].data_ptr(), back["primitive"].data_ptr(), 4
        for k in range(4):
            tg.coverage[k], tg.layerPrimitive[k] = back["coverage"][k].data_ptr(), back["layer_primitive"][k].data_ptr()
        for k, val in over.items():
            obj, field = {"m": (draw.mesh, k[2:]), "d": (draw, k[2:]), "t": (tg, k[2:])}[k[0]]
            setattr(obj, field, val)
        return lib.vqhip_scene_depth(hnd, st, None if draws_null else C.pointer(draw), ndraws, width, height, samples, None if out_null else C.byref(tg),
                                     C.c_void_p(work.data_ptr() if wptr is None else wptr), work.numel() if wbytes is None else wbytes)
    INV = abi.VQHIP_ERR_INVALID_ARG
    cases = [("NULL draws", dict(draws_null=True)), ("NULL out", dict(out_null=True)), ("NULL depth", dict(t_depth=None)), ("NULL work", dict(wptr=0)),
             ("negative numDraws", dict(ndraws=-1)), ("samples 2", dict(samples=2)), ("samples 0", dict(samples=0)), ("samples 8", dict(samples=8)),
             ("layers at 1x", dict(samples=1)), ("five layers", dict(t_layers=5)), ("negative layers", dict(t_layers=-1)),
             ("width 0", dict(width=0)), ("height 0", dict(height=0)), ("width above the limit", dict(width=abi.SCENE_DEPTH_MAX_DIM + 1)),
             ("height above the limit", dict(height=abi.SCENE_DEPTH_MAX_DIM + 1)),
             ("pitch below the row", dict(t_pitch=w - 1)), ("negative pitch", dict(t_pitch=-w)), ("coverage pitch below the row", dict(t_coverage_pitch=w - 1)),
             ("depth not 16-byte aligned at 4x", dict(t_depth=back["depth"].data_ptr() + 4)), ("primitive not 16-byte aligned at 4x", dict(t_primitive=back["primitive"].data_ptr() + 8)),
             ("reserved set", dict(t_reserved=1)),
             ("NULL positions", dict(m_positions=None)), ("NULL indices", dict(m_indices=None)), ("NULL matWorldViewProj", dict(d_matWorldViewProj=None)),
             ("indexBits 8", dict(m_indexBits=8)), ("numIndices not a multiple of 3", dict(m_numIndices=dd.indices.numel() - 1)),
             ("stride 8", dict(m_strideBytes=8)), ("stride 14", dict(m_strideBytes=14)),
             ("no instances", dict(d_numInstances=0)), ("65 instances", dict(d_numInstances=65)), ("cull mode 3", dict(d_cullMode=3)),
             ("workBytes one short", dict(wbytes=need - 1)), ("work not aligned", dict(wptr=work.data_ptr() + 4)),
             ("depth inside the work buffer", dict(t_depth=work.data_ptr() + 256))]
    for label, over in cases:
        assert call(**over) == INV, label
        assert len(lib.vqhip_last_error(hnd) or b"") > 10, label
    # 64 instances of 2^23 triangles are 2^29 instanced triangles: more than the record counter (and far less than the 2^32 - 1 at which q meets "no owner")
    assert call(m_numIndices=3 * 2 ** 23, d_numInstances=64) == abi.VQHIP_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (back["depth"] == SENT_F).all() and (back["primitive"] == SENT_I).all() and (work == 0x3C).all(), "a refused call wrote to its outputs"
    for k in range(4):
        assert (back["coverage"][k] == SENT_B).all() and (back["layer_primitive"][k] == SENT_I).all(), "a refused call wrote to its layer planes"
    assert call() == abi.VQHIP_OK
    torch.cuda.synchronize()
    assert_outputs("after the refusals", {k: ([t.cpu().numpy() for t in v] if isinstance(v, list) else v.cpu().numpy()) for k, v in back.items()}, SC.expected(name), w)
    # the Python binding validates before it calls
    with pytest.raises(ValueError):
        ctx.scene_depth([dd], w, h, samples=2)
    with pytest.raises(ValueError):
        ctx.scene_depth([dd], w, h, samples=1, layers=2)
    with pytest.raises(ValueError):
        ctx.scene_depth([capi.ShadowDraw(dd.positions, dd.indices[:-1], dd.wvp)], w, h)
    with pytest.raises(ValueError):
        ctx.scene_depth([dd], w, h, samples=4, out={"depth": torch.empty((h, w - 1, 4), dtype=torch.float32, device="cuda")})


# ---- the chains: the pre-pass feeds the stages that consume it ------------------------------------------------------------------------------------------------------
def _levels_equal(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for l, (g, e) in enumerate(zip(got, want)):
        g = g.cpu().numpy()
        assert g.shape == e.shape and np.array_equal(g.view(np.uint32), np.ascontiguousarray(e, np.float32).view(np.uint32)), f"{what}: level {l} differs"


def test_chain_4x_depth_resolve_and_hierarchy(ctx):
    """room at 64 x 40: depth and coverage into vqhip_msaa_resolve_surfaces with the hierarchy == tests/depth_ref.py on this pass's reference arrays"""
    name = "room_64x40_s4"
    scene, e = SC.cases()[name], SC.expected(name)
    F32 = abi.FMT_RGBA32F
    n = V.instanced_triangles(scene)
    words = synth.packed_unit_normals((1, n + 1), seed=0x5CD)                                      # one normal per primitive; the last stands for "no owner"
    table = np.concatenate([depth_ref.decode_normals01(words, abi.FMT_R10G10B10A2_UNORM), np.ones((1, n + 1, 1), np.float32)], -1)[0]
    res = ctx.scene_depth([device_draw(d) for d in scene["draws"]], 64, 40, 4, layers=4)
    dtab, normals_dev, normals_ref = dev(table), [], []
    for k in range(4):                                                                             # the coverage planes are read for the normals: give it normals
        lp = res["layer_primitive"][k].to(torch.int64) & 0xFFFFFFFF
        normals_dev.append(dtab[torch.where(lp == V.NO_PRIMITIVE, torch.full_like(lp, n), lp)].contiguous())
        lr = e["layer_primitive"][k].astype(np.int64)
        normals_ref.append(np.ascontiguousarray(table[np.where(lr == V.NO_PRIMITIVE, n, lr)]))
    got = ctx.msaa_resolve_surfaces(res["depth"], res["coverage"], normals=normals_dev, normals_fmt=F32, out_depth=True, out_normals_fmt=F32, hierarchy=True)
    torch.cuda.synchronize()
    want = depth_ref.hierarchy(depth_ref.resolve_depth(np.ascontiguousarray(e["depth"]))[0])
    _levels_equal(got["hierarchy"], want, "resolve + hierarchy of the rasterised room")
    assert np.array_equal(got["depth"].cpu().numpy().view(np.uint32), want[0].view(np.uint32))
    want_n = depth_ref.resolve_normals(normals_ref, [np.ascontiguousarray(c) for c in e["coverage"]], F32, False, F32)
    n_bad, idx = O.bits_equal(got["normals"].cpu().numpy(), want_n)
    assert n_bad == 0, f"normals resolved under the rasterised masks: {n_bad} elements differ, first {idx.tolist()}"


def test_chain_4x_masks_shade_and_resolve(ctx):
    """room at 64 x 40: per-layer G-buffers filled on the device from layerPrimitive (one constant record per primitive), shaded and resolved by
    vqhip_forward_lighting_msaa under the rasterised masks == the oracle's shading of the same records resolved by tests/msaa_ref.py under the reference masks"""
    name = "room_64x40_s4"
    scene, e = SC.cases()[name], SC.expected(name)
    w, h = 64, 40
    n = V.instanced_triangles(scene)
    table = synth.gbuffer(n + 1, 1, seed=0x5CE)                                                     # record q at [0, q]; the last one stands for "no owner"
    res = ctx.scene_depth([device_draw(d) for d in scene["draws"]], w, h, 4, layers=4)
    dtab = [dev(p[0]) for p in table]
    layers_dev, layers_ref = [], []
    for k in range(4):
        lp = res["layer_primitive"][k].to(torch.int64) & 0xFFFFFFFF
        lp = torch.where(lp == V.NO_PRIMITIVE, torch.full_like(lp, n), lp)
        layers_dev.append([t[lp].contiguous() for t in dtab])
        lr = e["layer_primitive"][k].astype(np.int64)
        lr = np.where(lr == V.NO_PRIMITIVE, n, lr)
        layers_ref.append([np.ascontiguousarray(p[0][lr]) for p in table])
    pf, extra = synth.per_frame(points=synth.point_lights(12, seed=0x5CE), spots=synth.spot_lights(2, seed=0x5CE), directional=synth.directional_light())
    pv = synth.per_view(w, h)
    got = ctx.forward_lighting_msaa(layers_dev, res["coverage"], pf, pv, out_fmt=abi.FMT_RGBA16F, extra_point=extra)
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        shaded = [O.forward_lighting(g, pf, pv, abi.FMT_RGBA16F, extra_point=extra) for g in layers_ref]
    want = msaa_ref.resolve(shaded, [np.ascontiguousarray(c) for c in e["coverage"]], None, abi.FMT_RGBA16F)
    n_bad, idx = O.bits_equal(got.cpu().numpy(), want)
    assert n_bad == 0, f"lit resolve under the rasterised masks: {n_bad} elements differ, first {idx.tolist()}"
    assert sum(int((c != 0).sum()) for c in e["coverage"][1:]) > 100, "the room has edge pixels"


def test_chain_1x_depth_hierarchy(ctx):
    name = "room_129x67_s1"
    scene, e = SC.cases()[name], SC.expected(name)
    res = ctx.scene_depth([device_draw(d) for d in scene["draws"]], 129, 67, 1)
    got = ctx.depth_hierarchy(res["depth"])
    torch.cuda.synchronize()
    _levels_equal(got, depth_ref.hierarchy(np.ascontiguousarray(e["depth"])), "hierarchy of the rasterised room")
