"""vqhip_scene_masked_depth and vqhip_shadow_masked_depth on the GPU (docs/DESIGN_DETAILS.md §7.19): every output plane bit for bit against
tests/masked_depth_ref.py, no tolerance, through the Python binding and, for the refusals, the raw C ABI. The scenes are tests/masked_depth_cases.py's: frames of
33 x 17 and 64 x 48, maps of 32 and 48 texels, textures 8 x 8, 12 x 6 and 1 x 1. References are computed once per case and shared."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import masked_depth_cases as MC
from tests import masked_depth_ref as M
from tests import oracle_lib as O
from tests import scene_depth_cases as SC
from tests import scene_interp_ref as I
from tests import shadow_raster_cases as K
from tests.test_gpu_scene_depth import SENT_B, SENT_F, SENT_I, assert_outputs, dev, targets
from vqengine_amd import abi, capi, synth

pytestmark = pytest.mark.gpu
_KEEP = []                                        # device chains stay alive while a test runs


@pytest.fixture(autouse=True)
def _release_device_chains():
    """nothing of this module stays allocated on the device after a test: the modules that run later find the allocator as they would without this one"""
    yield
    _KEEP.clear()


def device_texture(tex):
    """abi.Texture2D over a device copy of the case's chain (texels NULL for the null SRV)"""
    if tex["chain"] is None:
        return abi.Texture2D(None, 0, 0, 0, 0)
    t = dev(tex["chain"])
    _KEEP.append(t)
    return abi.Texture2D(t.data_ptr(), tex["w"], tex["h"], tex["mips"], 0)


def device_material(m):
    mat = abi.MaterialDesc()
    mat.data.uvScaleOffset = abi.float4(*m["scale_offset"])
    mat.data.textureConfig = m["texture_config"]
    mat.texDiffuse = device_texture(m["tex"])
    mat.texDiffuse.reserved = abi.MATERIAL_ALPHA_MASKED
    return mat


def device_draw(d, shadow=False, masked=True):
    idx = d["indices"]
    ix = dev(idx.astype(np.uint16).view(np.int16)) if d["bits"] == 16 else dev(idx.astype(np.int32))
    m = d.get("mask") if masked else None
    return capi.MaskedDraw(dev(d["positions"]), ix, dev(d["wvp"]), None if d.get("world") is None else dev(d["world"]), d["cull"],
                           material=device_material(m) if m is not None and not shadow else None,
                           texture=device_texture(m["tex"]) if m is not None and shadow else None)


def run(ctx, scene, pad=0, cov_pad=0, work=None, stream=None, masked_entry=True, masked=True):
    layers = 4 if scene["samples"] == 4 else 0
    back, out = targets(scene, layers, pad, cov_pad)
    fn = ctx.scene_masked_depth if masked_entry else ctx.scene_depth
    fn([device_draw(d, masked=masked) for d in scene["draws"]], scene["width"], scene["height"], scene["samples"], primitive=True, layers=layers, out=out,
       work=work, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return {k: ([t.cpu().numpy() for t in v] if isinstance(v, list) else v.cpu().numpy()) for k, v in back.items()}


def shadow_views(views, pad=0, masked=True, fill=-7.0):
    out, backing = [], []
    for v in views:
        t = torch.full((v["dim"], v["dim"] + pad), fill, dtype=torch.float32, device="cuda")
        backing.append(t)
        out.append(capi.ShadowView(t[:, :v["dim"]], [device_draw(d, True, masked) for d in v["draws"]], v["linear"], v["camera"], v["far"]))
    return out, backing


def run_shadow(ctx, views, pad=0, work=None, stream=None, masked_entry=True, masked=True):
    dviews, backing = shadow_views(views, pad, masked)
    (ctx.shadow_masked_depth if masked_entry else ctx.shadow_depth)(dviews, work=work, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return [b.cpu().numpy() for b in backing]


def assert_maps(name, got, ref, dims):
    for k, (g, e, d) in enumerate(zip(got, ref, dims)):
        n_bad, idx = O.bits_equal(np.ascontiguousarray(g[:, :d]), e)
        assert n_bad == 0, f"{name} view {k}: {n_bad} of {e.size} texels differ from tests/masked_depth_ref.py, first at {idx.tolist()}"


@pytest.mark.parametrize("name", sorted(MC.cases()))
def test_scene_case_matches_the_statement(ctx, name):
    """magnified checker over a wall, minified stripes across two mip levels, the tilted card, uvScaleOffset with WRAP (8 x 8 and 12 x 6), the diffuse bit and the
    null / 1 x 1 textures, clipping, two textures in one tile + instancing + 16-bit indices + strides 44 and 64, the equal-depth pair — depth, primitive and at 4x
    all four coverage / layerPrimitive planes"""
    scene = MC.cases()[name]
    assert_outputs(name, run(ctx, scene), MC.expected(name), scene["width"])


@pytest.mark.parametrize("name", sorted(MC.shadow_cases()))
def test_shadow_case_matches_the_statement(ctx, name):
    views = MC.shadow_cases()[name]
    assert_maps(name, run_shadow(ctx, views), MC.shadow_expected(name)["maps"], [v["dim"] for v in views])


def test_no_masked_draw_equals_the_opaque_entry_points(ctx):
    """all materials NULL: bit-identical to vqhip_scene_depth / vqhip_shadow_depth on the same draws (existing case scenes and the new ones)"""
    for name in ("soup_64x40_s4", "room_64x40_s1", "boxes_16x16_s4"):
        scene = SC.cases()[name]
        a, b = run(ctx, scene), run(ctx, scene, masked_entry=False)
        assert_outputs(name, a, SC.expected(name), scene["width"])
        for key in a:
            for x, y in zip(a[key] if isinstance(a[key], list) else [a[key]], b[key] if isinstance(b[key], list) else [b[key]]):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{name} {key}"
    sc = MC.cases()["variety_64x48_s4"]
    a, b = run(ctx, sc, masked=False), run(ctx, sc, masked_entry=False, masked=False)
    for key in a:
        for x, y in zip(a[key] if isinstance(a[key], list) else [a[key]], b[key] if isinstance(b[key], list) else [b[key]]):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"variety {key}"
    for views in (K.cases()["soup_64_linear"], K.cases()["cube6_64"], MC.shadow_cases()["both"]):
        a, b = run_shadow(ctx, views, masked=False), run_shadow(ctx, views, masked_entry=False, masked=False)
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_both_tile_sizes_give_the_same_bits(ctx, set_opt):
    for tile in (64, 32):
        set_opt("raster_tile", tile)
        for name in ("variety_64x48_s1", "clipped_64x48_s1", "magnified_64x48_s4"):
            assert_outputs(f"tile {tile} {name}", run(ctx, MC.cases()[name]), MC.expected(name), 64)
        views = MC.shadow_cases()["both"]
        assert_maps(f"tile {tile}", run_shadow(ctx, views), MC.shadow_expected("both")["maps"], [v["dim"] for v in views])


def test_pitched_outputs_keep_their_padding(ctx):
    for name in ("variety_64x48_s4", "magnified_33x17_s1"):
        scene = MC.cases()[name]
        w = scene["width"]
        got = run(ctx, scene, pad=5, cov_pad=3)
        assert_outputs(f"pitched {name}", got, MC.expected(name), w)
        assert (got["depth"][:, w:] == SENT_F).all() and (got["primitive"][:, w:] == SENT_I).all()
        for k in range(len(got.get("coverage", ()))):
            assert (got["coverage"][k][:, w:] == SENT_B).all() and (got["layer_primitive"][k][:, w:] == SENT_I).all()
    views = MC.shadow_cases()["both"]
    got = run_shadow(ctx, views, pad=3)
    assert_maps("pitched", got, MC.shadow_expected("both")["maps"], [v["dim"] for v in views])
    for g, v in zip(got, views):
        assert (g[:, v["dim"]:] == -7.0).all()


def test_prefilled_work_buffer_second_call_and_side_stream(ctx):
    name = "variety_64x48_s4"
    scene = MC.cases()[name]
    need = capi.scene_masked_depth_work_bytes(MC.instanced_triangles(scene["draws"]), MC.instanced_triangles(scene["draws"], True), len(scene["draws"]))
    work = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    for label in ("0xFF-filled work buffer", "second call on the same buffer"):
        assert_outputs(f"{name}: {label}", run(ctx, scene, work=work[:need]), MC.expected(name), 64)
    assert (work[need:] == 0xFF).all(), "the call wrote past vqhip_scene_masked_depth_work_bytes"
    assert_outputs("side stream", run(ctx, MC.cases()["clipped_33x17_s4"], stream=torch.cuda.Stream()), MC.expected("clipped_33x17_s4"), 33)
    views = MC.shadow_cases()["both"]
    draws = [d for v in views for d in v["draws"]]
    need = capi.shadow_masked_depth_work_bytes(MC.instanced_triangles(draws), MC.instanced_triangles(draws, True), len(views), len(draws))
    work = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    for label in ("0xFF-filled work buffer", "second call"):
        assert_maps(label, run_shadow(ctx, views, work=work[:need]), MC.shadow_expected("both")["maps"], [v["dim"] for v in views])
    assert (work[need:] == 0xFF).all()
    assert_maps("side stream", run_shadow(ctx, views, stream=torch.cuda.Stream()), MC.shadow_expected("both")["maps"], [v["dim"] for v in views])


def test_scene_refusals_launch_nothing(ctx):
    name = "magnified_64x48_s4"
    scene = MC.cases()[name]
    dds = [device_draw(d) for d in scene["draws"]]
    w, h = 64, 48
    back, out = targets(scene, 4)
    tris, mtris = MC.instanced_triangles(scene["draws"]), MC.instanced_triangles(scene["draws"], True)
    need = capi.scene_masked_depth_work_bytes(tris, mtris, 2)
    work = torch.full((need,), 0x3C, dtype=torch.uint8, device="cuda")
    lib, hnd, st = ctx.lib, ctx._h, ctx._stream()
    chain = dev(scene["draws"][1]["mask"]["tex"]["chain"])

    def call(wbytes=None, samples=4, **over):
        arr = (abi.SceneDepthMaskedDraw * 2)()
        mat = device_material(scene["draws"][1]["mask"])
        mat.texDiffuse.texels = chain.data_ptr()
        for c, dd, d in zip(arr, dds, scene["draws"]):
            c.draw.mesh.positions, c.draw.mesh.strideBytes, c.draw.mesh.numVertices = dd.positions.data_ptr(), dd.positions.stride(0) * 4, dd.positions.shape[0]
            c.draw.mesh.indices, c.draw.mesh.indexBits, c.draw.mesh.numIndices = dd.indices.data_ptr(), d["bits"], dd.indices.numel()
            c.draw.matWorldViewProj, c.draw.numInstances, c.draw.cullMode = dd.wvp.data_ptr(), dd.wvp.shape[0], d["cull"]
        arr[1].material = C.pointer(mat)
        tg = abi.SceneDepthTargets()
        tg.depth, tg.primitive, tg.layers = back["depth"].data_ptr(), back["primitive"].data_ptr(), 4
        for k in range(4):
            tg.coverage[k], tg.layerPrimitive[k] = back["coverage"][k].data_ptr(), back["layer_primitive"][k].data_ptr()
        for k, val in over.items():
            obj = {"m": arr[1].draw.mesh, "x": mat.texDiffuse, "d": arr[1].draw}[k[0]]
            setattr(obj, k[2:], val)
        return lib.vqhip_scene_masked_depth(hnd, st, arr, 2, w, h, samples, C.byref(tg), C.c_void_p(work.data_ptr()), work.numel() if wbytes is None else wbytes)
    INV = abi.VQHIP_ERR_INVALID_ARG
    cases = [("masked stride 40", dict(m_strideBytes=40)), ("masked stride 12", dict(m_strideBytes=12)),
             ("texture width 0", dict(x_width=0)), ("texture width above the limit", dict(x_width=abi.MASK_TEXTURE_MAX_DIM + 1)),
             ("texture height negative", dict(x_height=-8)), ("texture height above the limit", dict(x_height=abi.MASK_TEXTURE_MAX_DIM + 1)),
             ("no mips", dict(x_mips=0)), ("more mips than the size has", dict(x_mips=5)), ("misaligned texels", dict(x_texels=chain.data_ptr() + 2)),
             ("workBytes one short", dict(wbytes=need - 1)), ("workBytes of the opaque call", dict(wbytes=capi.scene_depth_work_bytes(tris))),
             ("inherited: samples 2", dict(samples=2)), ("inherited: 65 instances", dict(d_numInstances=65))]
    for label, over in cases:
        assert call(**over) == INV, label
        assert len(lib.vqhip_last_error(hnd) or b"") > 10, label
    torch.cuda.synchronize()
    assert (back["depth"] == SENT_F).all() and (back["primitive"] == SENT_I).all() and (work == 0x3C).all(), "a refused call wrote to its outputs"
    for k in range(4):
        assert (back["coverage"][k] == SENT_B).all() and (back["layer_primitive"][k] == SENT_I).all()
    assert call() == abi.VQHIP_OK
    torch.cuda.synchronize()
    assert_outputs("after the refusals", {k: ([t.cpu().numpy() for t in v] if isinstance(v, list) else v.cpu().numpy()) for k, v in back.items()}, MC.expected(name), w)
    with pytest.raises(ValueError):                                    # the binding validates before it calls: a masked draw on tight positions
        ctx.scene_masked_depth([capi.MaskedDraw(dds[1].positions[:, :3], dds[1].indices, dds[1].wvp, material=dds[1].material)], w, h)


def test_shadow_refusals_launch_nothing(ctx):
    views = MC.shadow_cases()["spot_48"]
    dviews, backing = shadow_views(views)
    draws = views[0]["draws"]
    need = capi.shadow_masked_depth_work_bytes(MC.instanced_triangles(draws), MC.instanced_triangles(draws, True), 1, len(draws))
    work = torch.full((need,), 0x3C, dtype=torch.uint8, device="cuda")
    lib, hnd, st = ctx.lib, ctx._h, ctx._stream()
    dds = dviews[0].draws
    chain = dev(draws[1]["mask"]["tex"]["chain"])

    def call(wbytes=None, **over):
        arr = (abi.ShadowMaskedDraw * len(dds))()
        texs = [abi.Texture2D(chain.data_ptr(), 8, 8, 4, 0), device_texture(draws[2]["mask"]["tex"]), abi.Texture2D(None, 0, 0, 0, 0)]
        for c, dd, d in zip(arr, dds, draws):
            c.draw.mesh.positions, c.draw.mesh.strideBytes, c.draw.mesh.numVertices = dd.positions.data_ptr(), dd.positions.stride(0) * 4, dd.positions.shape[0]
            c.draw.mesh.indices, c.draw.mesh.indexBits, c.draw.mesh.numIndices = dd.indices.data_ptr(), d["bits"], dd.indices.numel()
            c.draw.matWorldViewProj, c.draw.matWorld, c.draw.numInstances, c.draw.cullMode = dd.wvp.data_ptr(), dd.world.data_ptr(), dd.wvp.shape[0], d["cull"]
        for k in range(3):
            arr[1 + k].texDiffuseAlpha = C.pointer(texs[k])
        v = abi.ShadowMaskedView()
        v.depth, v.pitchBytes, v.dim, v.linearDepth, v.farPlane, v.numDraws = backing[0].data_ptr(), backing[0].stride(0) * 4, 48, 0, 1.0, len(dds)
        v.draws = C.cast(arr, C.POINTER(abi.ShadowMaskedDraw))
        for k, val in over.items():
            obj = {"m": arr[1].draw.mesh, "x": texs[0], "v": v}[k[0]]
            setattr(obj, k[2:], val)
        return lib.vqhip_shadow_masked_depth(hnd, st, C.byref(v), 1, C.c_void_p(work.data_ptr()), work.numel() if wbytes is None else wbytes)
    for label, over in [("masked stride 36", dict(m_strideBytes=36)), ("texture width 0", dict(x_width=0)), ("texture height above the limit", dict(x_height=1 << 20)),
                        ("no mips", dict(x_mips=0)), ("too many mips", dict(x_mips=9)), ("misaligned texels", dict(x_texels=chain.data_ptr() + 1)),
                        ("workBytes one short", dict(wbytes=need - 1)), ("inherited: dim 0", dict(v_dim=0))]:
        assert call(**over) == abi.VQHIP_ERR_INVALID_ARG, label
        assert len(lib.vqhip_last_error(hnd) or b"") > 10, label
    torch.cuda.synchronize()
    assert (backing[0] == -7.0).all() and (work == 0x3C).all(), "a refused call wrote to its outputs"
    assert call() == abi.VQHIP_OK
    torch.cuda.synchronize()
    assert_maps("after the refusals", [backing[0].cpu().numpy()], MC.shadow_expected("spot_48")["maps"], [48])


def test_chain_interpolants_see_the_background_through_the_holes(ctx):
    """vqhip_scene_masked_depth -> vqhip_scene_interpolants: hole pixels carry the wall's materialIndex; all planes == scene_interp_ref on the statement's owners"""
    name = "magnified_64x48_s1"
    sc, e = MC.cases()[name], MC.expected(name)
    full = dict(sc, draws=[dict(d, normal=d["world"], wvp_prev=None, material=7 + k) for k, d in enumerate(sc["draws"])])
    res = ctx.scene_masked_depth([device_draw(d) for d in sc["draws"]], 64, 48, 1, primitive=True)
    sdraws = [capi.SurfaceDraw(dev(d["positions"]), dev(d["indices"].astype(np.int32)), dev(d["wvp"]), dev(d["world"]), dev(d["normal"]), None, d["material"])
              for d in full["draws"]]
    got = ctx.scene_interpolants(sdraws, 64, 48, res["primitive"])
    torch.cuda.synchronize()
    want = I.interpolate(full, e["primitive"])
    for key in ("ip0", "ip1", "ip2"):
        n_bad, idx = O.bits_equal(got[key].cpu().numpy().view(np.uint32), want[key])
        assert n_bad == 0, f"{key}: {n_bad} elements differ, first {idx.tolist()}"
    opaque_owner = M.V.rasterize(MC.opaque(sc))["primitive"]
    holes = (opaque_owner >= 2) & (e["primitive"] < 2)
    mat = got["ip2"].cpu().numpy().view(np.int32)[..., 3]
    assert holes.sum() > 200 and (mat[holes] == 7).all() and (mat[e["primitive"] >= 2] == 8).all()


def test_chain_masked_caster_lights_through_its_holes(ctx):
    """vqhip_shadow_masked_depth -> vqhip_forward_lighting: floor points under the checker card, lit by the spot caster through the rasterised map == the oracle
    lit with the statement's map; among them points behind a hole are fully lit and points behind an opaque texel fully shadowed"""
    from vqengine_amd import scene, shadow_scene as S
    view = MC.spot_view(48)
    n = 24
    gx, gz = np.meshgrid(np.linspace(-2.4, 1.4, n), np.linspace(-1.6, 2.2, n))
    gb = [np.zeros((n, n, 4), np.float32) for _ in range(4)]
    gb[0][..., 0], gb[0][..., 1], gb[0][..., 2], gb[0][..., 3] = gx, -1.0, gz, 1.0
    gb[1][..., 1], gb[1][..., 3] = 1.0, 0.6
    gb[2][..., :3], gb[3][..., 3] = 0.8, 0.0
    pf, _ = synth.per_frame(ambient=0.0)
    L = pf.Lights
    L.numSpotCasters = 1
    sc = L.spot_casters[0]
    sc.position.set((0.0, 3.0, -2.0)); sc.spotDir.set((0.0, -0.8, 0.6)); sc.color.set((1.0, 1.0, 1.0)); sc.brightness = 80.0
    sc.outerConeAngle, sc.innerConeAngle, sc.depthBias, sc.range = float(np.float32(0.75)), float(np.float32(0.6)), 1e-2, 15.0
    scene._set_matrix(L.shadowViews[0], S.spot_view_proj((0.0, 3.0, -2.0), (0.0, -0.8, 0.6), 0.1, 15.0))
    scene._set_shadow_dims(pf, (48, 48, 48))
    pv = synth.per_view(n, n, camera=(0.0, 2.0, -3.0))
    spot = torch.ones((abi.NUM_SHADOWING_LIGHTS__SPOT, 48, 48), dtype=torch.float32, device="cuda")
    one_d, one_p = torch.ones((48, 48), dtype=torch.float32, device="cuda"), torch.ones((1, 6, 48, 48), dtype=torch.float32, device="cuda")
    ctx.shadow_masked_depth([capi.ShadowView(spot[0], [device_draw(d, True) for d in view["draws"]], False, view["camera"], view["far"])])
    gbd = [dev(g) for g in gb]

    def lit_with(sp):
        sm = abi.ShadowMaps(one_d.data_ptr(), 48, sp.data_ptr(), 48, one_p.data_ptr(), 48)
        out = ctx.forward_lighting(gbd, pf, pv, out_fmt=abi.FMT_RGBA32F, shadow=sm)
        torch.cuda.synchronize()
        return out.cpu().numpy()
    got = lit_with(spot)
    ref_map = MC.shadow_expected("spot_48")["maps"][0]
    host = {"dir": np.ones((48, 48), np.float32), "spot": np.ones((abi.NUM_SHADOWING_LIGHTS__SPOT, 48, 48), np.float32), "point": np.ones((1, 6, 48, 48), np.float32),
            "dims": (48, 48, 48)}
    host["spot"][0] = ref_map
    ref = O.forward_lighting(gb, pf, pv, abi.FMT_RGBA32F, shadow=scene.shadow_maps_struct(host, lambda a: a.ctypes.data))
    n_bad, idx = O.bits_equal(got, ref)
    assert n_bad == 0, f"lit with the rasterised masked map: {n_bad} elements differ from the oracle, first {idx.tolist()}"
    hi, lo = lit_with(torch.ones_like(spot)), lit_with(torch.zeros_like(spot))
    reach = (hi != lo).any(axis=2)
    opaque_map = M.R.rasterize([MC.opaque([view])[0]])[0]
    host["spot"][0] = opaque_map
    solid = O.forward_lighting(gb, pf, pv, abi.FMT_RGBA32F, shadow=scene.shadow_maps_struct(host, lambda a: a.ctypes.data))
    host["spot"][0] = M.R.rasterize([dict(view, draws=view["draws"][:1])])[0]
    bare = O.forward_lighting(gb, pf, pv, abi.FMT_RGBA32F, shadow=scene.shadow_maps_struct(host, lambda a: a.ctypes.data))
    under = reach & (solid == lo).all(axis=2) & (bare == hi).all(axis=2)       # lit on the bare floor, fully shadowed by the cards drawn solid
    through = under & (got == hi).all(axis=2)                          # ... and fully lit through a hole of the masked card
    blocked = under & (got == lo).all(axis=2)
    assert through.sum() >= 3 and blocked.sum() >= 3, (int(under.sum()), int(through.sum()), int(blocked.sum()))
