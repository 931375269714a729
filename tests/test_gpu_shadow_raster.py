"""vqhip_shadow_depth on the GPU (docs/DESIGN_DETAILS.md §7.16): every map bit for bit against tests/shadow_raster_ref.py, through the Python binding and, for the
refusals, the raw C ABI. The scenes are tests/shadow_raster_cases.py's, at the smallest sizes that can still go wrong: dim 16, 64 (two tiles a side) and 129 (a
partial tile in both directions). References are computed once per case and shared; each GPU step runs once."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import oracle_lib as O
from tests import shadow_raster_cases as K
from tests import shadow_raster_ref as R
from vqengine_amd import abi, capi

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_draw(d):
    idx = d["indices"]
    ix = dev(idx.astype(np.uint16).view(np.int16)) if d["bits"] == 16 else dev(idx.astype(np.int32))
    return capi.ShadowDraw(dev(d["positions"]), ix, dev(d["wvp"]), None if d["world"] is None else dev(d["world"]), d["cull"])


def device_views(views, pad=0, fill=SENTINEL):
    """(capi views, backing tensors): each map is the left dim columns of a [dim, dim + pad] tensor prefilled with `fill`"""
    out, backing = [], []
    for v in views:
        t = torch.full((v["dim"], v["dim"] + pad), fill, dtype=torch.float32, device="cuda")
        backing.append(t)
        out.append(capi.ShadowView(t[:, :v["dim"]], [device_draw(d) for d in v["draws"]], v["linear"], v["camera"], v["far"]))
    return out, backing


def assert_same(name, got, ref):
    n_bad, idx = O.bits_equal(np.asarray(got), np.asarray(ref))
    assert n_bad == 0, f"{name}: {n_bad} of {np.asarray(ref).size} texels differ from tests/shadow_raster_ref.py, first at {idx.tolist()}"


def run(ctx, views, pad=0, work=None, stream=None):
    dviews, backing = device_views(views, pad)
    ctx.shadow_depth(dviews, work=work, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return [b.cpu().numpy() for b in backing]


@pytest.mark.parametrize("name", sorted(K.cases()))
def test_case_matches_the_statement(ctx, name):
    views = K.cases()[name]
    got = run(ctx, views)
    for i, (g, e) in enumerate(zip(got, K.expected(name))):
        assert_same(f"{name} view {i}", g, e)


def test_both_tile_sizes_give_the_same_bits(ctx, set_opt):
    for tile in (64, 32):
        set_opt("raster_tile", tile)
        for name in ("soup_129", "quad_w0_129", "cube6_64"):
            for i, (g, e) in enumerate(zip(run(ctx, K.cases()[name]), K.expected(name))):
                assert_same(f"tile {tile} {name} view {i}", g, e)


def test_six_faces_in_one_call_and_one_call_each(ctx):
    views = K.cases()["cube6_64"]
    together = run(ctx, views)
    for f in range(6):
        alone = run(ctx, [views[f]])[0]
        assert_same(f"face {f} alone", alone, K.expected("cube6_64")[f])
        assert np.array_equal(alone.view(np.uint32), together[f].view(np.uint32)), f"face {f}: one call each differs from six views in one call"


def test_pitched_outputs_keep_their_padding(ctx):
    for name in ("soup_129", "cube6_64"):
        got = run(ctx, K.cases()[name], pad=5)
        for i, (g, e) in enumerate(zip(got, K.expected(name))):
            dim = e.shape[0]
            assert (g[:, dim:] == SENTINEL).all(), f"{name} view {i}: the padding was written"
            assert_same(f"pitched {name} view {i}", g[:, :dim], e)


def test_slices_of_one_array_keep_their_neighbours(ctx):
    """the six faces as slices 1 .. 6 of an eight-slice array: slices 0 and 7 keep the sentinel"""
    views = K.cases()["cube6_64"]
    arr = torch.full((8, 64, 64), SENTINEL, dtype=torch.float32, device="cuda")
    dviews = [capi.ShadowView(arr[1 + f], [device_draw(d) for d in v["draws"]], v["linear"], v["camera"], v["far"]) for f, v in enumerate(views)]
    ctx.shadow_depth(dviews)
    torch.cuda.synchronize()
    host = arr.cpu().numpy()
    assert (host[0] == SENTINEL).all() and (host[7] == SENTINEL).all()
    for f in range(6):
        assert_same(f"slice {1 + f}", host[1 + f], K.expected("cube6_64")[f])


def test_prefilled_work_buffer_and_second_call(ctx):
    views = K.cases()["soup_129"]
    need = capi.shadow_depth_work_bytes(R.instanced_triangles(views), len(views))
    work = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    for label in ("0xFF-filled work buffer", "second call on the same buffer"):
        got = run(ctx, views, work=work[:need])
        assert_same(label, got[0], K.expected("soup_129")[0])
    assert (work[need:] == 0xFF).all(), "the call wrote past vqhip_shadow_depth_work_bytes"


def test_two_runs_are_bit_equal(ctx):
    """the records are appended in whatever order the workgroups arrive; the maps are minima and do not depend on it"""
    a = run(ctx, K.cases()["soup_129"])[0]
    b = run(ctx, K.cases()["soup_129"])[0]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_non_default_stream(ctx):
    s = torch.cuda.Stream()
    got = run(ctx, K.cases()["boxes128_64"], stream=s)
    assert_same("side stream", got[0], K.expected("boxes128_64")[0])


def test_empty_views_are_cleared(ctx):
    views = [K.view(16, []), K.view(129, [], linear=True), K.view(1, [])]
    for g in run(ctx, views):
        assert (g == 1.0).all()


def test_refusals_launch_nothing(ctx):
    v = K.cases()["boxes128_64"][0]
    d = v["draws"][0]
    dd = device_draw(d)
    dim = v["dim"]
    depth = torch.full((dim, dim), SENTINEL, dtype=torch.float32, device="cuda")
    need = capi.shadow_depth_work_bytes(R.instanced_triangles([v]), 1)
    work = torch.full((need,), 0x3C, dtype=torch.uint8, device="cuda")
    lib, hnd, st = ctx.lib, ctx._h, ctx._stream()

    def call(nviews=1, wptr=None, wbytes=None, views_null=False, **over):
        draw = abi.ShadowDraw()
        draw.mesh.positions, draw.mesh.strideBytes, draw.mesh.numVertices = dd.positions.data_ptr(), dd.positions.stride(0) * 4, dd.positions.shape[0]
        draw.mesh.indices, draw.mesh.indexBits, draw.mesh.numIndices = dd.indices.data_ptr(), d["bits"], dd.indices.numel()
        draw.matWorldViewProj, draw.matWorld, draw.numInstances, draw.cullMode = dd.wvp.data_ptr(), dd.world.data_ptr(), dd.wvp.shape[0], d["cull"]
        view = abi.ShadowView()
        view.depth, view.pitchBytes, view.dim, view.linearDepth, view.farPlane = depth.data_ptr(), dim * 4, dim, 0, 1.0
        view.draws, view.numDraws = C.pointer(draw), 1
        for k, val in over.items():
            obj, field = {"m": (draw.mesh, k[2:]), "d": (draw, k[2:]), "v": (view, k[2:])}[k[0]]
            setattr(obj, field, val)
        views = (abi.ShadowView * 64)(*([view] * 64))
        return lib.vqhip_shadow_depth(hnd, st, None if views_null else views, nviews, C.c_void_p(work.data_ptr() if wptr is None else wptr),
                                      work.numel() if wbytes is None else wbytes)
    INV = abi.VQHIP_ERR_INVALID_ARG
    cases = [("NULL views", dict(views_null=True)), ("NULL work", dict(wptr=0)), ("no views", dict(nviews=0)), ("65 views", dict(nviews=65)),
             ("NULL depth", dict(v_depth=None)), ("dim 0", dict(v_dim=0)), ("dim above the limit", dict(v_dim=abi.SHADOW_MAX_DIM + 1)),
             ("pitch below the row", dict(v_pitchBytes=dim * 4 - 4)), ("pitch not a multiple of 4", dict(v_pitchBytes=dim * 4 + 2)),
             ("negative numDraws", dict(v_numDraws=-1)), ("NULL draws", dict(v_draws=C.POINTER(abi.ShadowDraw)())), ("linearDepth 2", dict(v_linearDepth=2)),
             ("NULL positions", dict(m_positions=None)), ("NULL indices", dict(m_indices=None)), ("NULL matWorldViewProj", dict(d_matWorldViewProj=None)),
             ("NULL matWorld in a linear-depth view", dict(d_matWorld=None, v_linearDepth=1)), ("indexBits 8", dict(m_indexBits=8)),
             ("numIndices not a multiple of 3", dict(m_numIndices=dd.indices.numel() - 1)), ("stride 8", dict(m_strideBytes=8)), ("stride 14", dict(m_strideBytes=14)),
             ("no instances", dict(d_numInstances=0)), ("129 instances", dict(d_numInstances=129)), ("cull mode 3", dict(d_cullMode=3)),
             ("workBytes one short", dict(wbytes=need - 1)), ("work not aligned", dict(wptr=work.data_ptr() + 4)),
             ("depth inside the work buffer", dict(v_depth=work.data_ptr() + 256))]
    for name, over in cases:
        assert call(**over) == INV, name
        assert len(lib.vqhip_last_error(hnd) or b"") > 10, name
    torch.cuda.synchronize()
    assert (depth == SENTINEL).all() and (work == 0x3C).all(), "a refused call wrote to its outputs"
    assert call() == abi.VQHIP_OK
    torch.cuda.synchronize()
    assert_same("after the refusals", depth.cpu().numpy(), K.expected("boxes128_64")[0])
    # the Python binding validates before it calls
    with pytest.raises(ValueError):
        ctx.shadow_depth([])
    with pytest.raises(ValueError):
        ctx.shadow_depth([capi.ShadowView(depth[:, :dim - 1], [])])
    with pytest.raises(ValueError):
        ctx.shadow_depth([capi.ShadowView(depth, [capi.ShadowDraw(dd.positions, dd.indices[:-1], dd.wvp)])])


# ---- end to end: rasterise the casters' maps, light the room with them -------------------------------------------------------------------------------------------------
def e2e_frame():
    """PerFrameData / PerViewLightingData of the room: one point, one spot and one directional caster, nothing else; no ambient term"""
    from vqengine_amd import scene, synth
    from vqengine_amd import shadow_scene as S
    pf, _ = synth.per_frame(ambient=0.0)
    L = pf.Lights
    L.numPointCasters = 1
    pc = L.point_casters[0]
    pc.position.set(K.E2E_POINT["position"]); pc.range = K.E2E_POINT["range"]; pc.color.set((1.0, 0.9, 0.8)); pc.brightness = 40.0
    pc.attenuation.set((1.0, 0.0, 0.0)); pc.depthBias = K.E2E_POINT["bias"]
    L.numSpotCasters = 1
    sc = L.spot_casters[0]
    sc.position.set(K.E2E_SPOT["position"]); sc.spotDir.set(K.E2E_SPOT["direction"]); sc.color.set((0.6, 0.8, 1.0)); sc.brightness = 60.0
    sc.outerConeAngle, sc.innerConeAngle, sc.depthBias, sc.range = float(np.float32(0.7)), float(np.float32(0.5)), 5e-5, K.E2E_SPOT["far"]
    scene._set_matrix(L.shadowViews[0], S.spot_view_proj(K.E2E_SPOT["position"], K.E2E_SPOT["direction"], K.E2E_SPOT["near"], K.E2E_SPOT["far"]))
    L.directional = synth.directional_light(direction=K.E2E_DIRECTIONAL["direction"], shadowing=1, depth_bias=5e-4)
    e = K.E2E_DIRECTIONAL
    scene._set_matrix(L.shadowViewDirectional, S.directional_view_proj(e["direction"], e["distance"], (e["extent"], e["extent"]), e["near"], e["far"]))
    scene._set_shadow_dims(pf, K.E2E_DIMS)
    h, w = 6 * K.E2E_LATTICE, K.E2E_LATTICE
    return pf, synth.per_view(w, h, camera=K.E2E_CAMERA)


def e2e_host_maps(point_fill=None):
    """tests/shadow_raster_ref.py's maps of the three casters in the arrays vqhip_shadowmaps reads; point_fill: that value in every point texel instead"""
    d, s, p = K.E2E_DIMS
    ref = R.rasterize(K.e2e_views()) if point_fill is None else None
    maps = {"dir": np.ones((d, d), np.float32), "spot": np.ones((abi.NUM_SHADOWING_LIGHTS__SPOT, s, s), np.float32),
            "point": np.ones((1, 6, p, p), np.float32), "dims": K.E2E_DIMS}
    if ref is not None:
        maps["dir"][:], maps["spot"][0] = ref[0], ref[1]
        for f in range(6):
            maps["point"][0, f] = ref[2 + f]
    return maps


def test_rasterised_maps_light_the_room_like_the_oracle(ctx):
    """One call rasterises the eight views into the arrays of vqhip_shadowmaps; vqhip_forward_lighting with them equals the oracle lit with the statement's maps,
    bit for bit. Then the orientation of the cube, without a tolerance: on the probes the geometry decides (tests/shadow_raster_cases.py: e2e_probes, at least
    four texels from any shadow edge) the frame equals the one lit with an all-1.0 cube where the probe is lit and the one lit with an all-0.0 cube where it is
    shadowed. A swapped or flipped face moves the occluders' shadows off their probes."""
    from vqengine_amd import scene
    pf, pv = e2e_frame()
    gb = K.e2e_gbuffer()
    host = e2e_host_maps()
    d, s, p = K.E2E_DIMS
    dmaps = {"dir": torch.full((d, d), SENTINEL, dtype=torch.float32, device="cuda"),
             "spot": torch.ones((abi.NUM_SHADOWING_LIGHTS__SPOT, s, s), dtype=torch.float32, device="cuda"),
             "point": torch.full((1, 6, p, p), SENTINEL, dtype=torch.float32, device="cuda")}
    views = K.e2e_views()
    targets = [dmaps["dir"], dmaps["spot"][0]] + [dmaps["point"][0, f] for f in range(6)]
    ctx.shadow_depth([capi.ShadowView(t, [device_draw(x) for x in v["draws"]], v["linear"], v["camera"], v["far"]) for t, v in zip(targets, views)])
    gbd = [dev(g) for g in gb]

    def lit_with(m):
        sm = abi.ShadowMaps(m["dir"].data_ptr(), d, m["spot"].data_ptr(), s, m["point"].data_ptr(), p)
        out = ctx.forward_lighting(gbd, pf, pv, out_fmt=abi.FMT_RGBA16F, shadow=sm)
        torch.cuda.synchronize()
        return out.cpu().numpy()
    got = lit_with(dmaps)
    for k in ("dir", "spot", "point"):
        assert_same(f"{k} maps", dmaps[k].cpu().numpy(), host[k])
    ref = O.forward_lighting(gb, pf, pv, abi.FMT_RGBA16F, shadow=scene.shadow_maps_struct(host, lambda a: a.ctypes.data))
    n_bad, idx = O.bits_equal(got, ref)
    assert n_bad == 0, f"scene colour lit with the rasterised maps differs from the oracle in {n_bad} elements, first {idx.tolist()}"
    all_lit = lit_with(dict(dmaps, point=torch.ones_like(dmaps["point"])))
    all_dark = lit_with(dict(dmaps, point=torch.zeros_like(dmaps["point"])))
    lit, shadowed, face = K.e2e_probes()
    flat = lambda a: a.reshape(-1, 4).view(np.uint16)      # noqa: E731
    g, hi, lo = flat(got), flat(all_lit), flat(all_dark)
    assert (hi[lit | shadowed] != lo[lit | shadowed]).any(axis=1).all(), "the point light does not reach a probe: the check would be vacuous there"
    for f in range(6):
        on, off = lit & (face == f), shadowed & (face == f)
        assert on.sum() >= 1 and off.sum() >= 1
        assert (g[on] == hi[on]).all(), f"cube face {f}: {int((g[on] != hi[on]).any(axis=1).sum())} of {int(on.sum())} lit probes are not fully lit"
        assert (g[off] == lo[off]).all(), f"cube face {f}: {int((g[off] != lo[off]).any(axis=1).sum())} of {int(off.sum())} shadowed probes are not fully shadowed"
