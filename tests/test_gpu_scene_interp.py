"""vqhip_scene_interpolants on the GPU (docs/DESIGN_DETAILS.md §7.18): all five planes bit for bit against tests/scene_interp_ref.py (an integer view: NaNs are
canonical), no tolerance, through the Python binding and, for the refusals, the raw C ABI. The scenes are tests/scene_interp_cases.py's at 16 x 16, 64 x 40 and
129 x 67, both sample counts; the owner planes handed to the call are the statement's (tests/scene_depth_ref.py), except in the chains, where vqhip_scene_depth
writes them. The chains at the end run meshes -> depth -> interpolants -> G-buffer -> lit frame inside the library, at 1x and at 4x MSAA, against the oracle's
producer and shade fed the statement's planes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import msaa_ref
from tests import oracle_lib as O
from tests import scene_interp_cases as IC
from tests import scene_interp_ref as I
from vqengine_amd import abi, capi, synth

pytestmark = pytest.mark.gpu
EXE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "test_passes_interpolants")
SENT = -7.0
PLANES = IC.PLANES


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_draw(d):
    idx = d["indices"]
    ix = dev(idx.astype(np.uint16).view(np.int16)) if d["bits"] == 16 else dev(idx.astype(np.int32))
    return capi.SurfaceDraw(dev(d["positions"]), ix, dev(d["wvp"]), dev(d["world"]), dev(d["normal"]), dev(d["wvp_prev"]), d["material"])


def dev_owner(owner):
    return dev(np.ascontiguousarray(owner, dtype=np.uint32).view(np.int32))


def targets(w, h, sv=True, pad=0, sv_pad=0):
    """prefilled backing tensors, wider than the target by the pads, and the views of them handed to the call"""
    back = {k: torch.full((h, w + (sv_pad if k.startswith("sv") else pad), 4), SENT, dtype=torch.float32, device="cuda") for k in (PLANES if sv else PLANES[:3])}
    return back, {k: t[:, :w] for k, t in back.items()}


def run(ctx, scene, owner, draws=None, sv=True, pad=0, sv_pad=0, work=None, stream=None):
    w, h = scene["width"], scene["height"]
    back, out = targets(w, h, sv, pad, sv_pad)
    ctx.scene_interpolants(draws if draws is not None else [device_draw(d) for d in scene["draws"]], w, h, dev_owner(owner), sv=sv, out=out, work=work, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return {k: t.cpu().numpy().view(np.uint32) for k, t in back.items()}


def assert_planes(name, got, ref, w, planes=PLANES):
    for k in planes:
        g, e = got[k][:, :w], ref[k]
        bad = np.argwhere(g != e)
        assert len(bad) == 0, f"{name} {k}: {len(bad)} of {e.size} words differ from tests/scene_interp_ref.py, first at {bad[0].tolist()}: {g[tuple(bad[0])]:#x} != {e[tuple(bad[0])]:#x}"


# ---- 1: every case, every owner plane, all five planes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(IC.cases()))
def test_case_matches_the_statement(ctx, name):
    """the room from inside (w = 0 crossed, two draws), 64 instanced boxes (16-bit indices, stride 44), the sphere (sub-pixel triangles, 32-bit indices, stride 48)
    and the grazing grid, at each size; at 4 samples one call per layerPrimitive plane"""
    scene = IC.cases()[name]
    draws = [device_draw(d) for d in scene["draws"]]
    for k, (owner, (ref, _)) in enumerate(zip(IC.owners(name)[0], IC.expected(name))):
        assert_planes(f"{name} plane {k}", run(ctx, scene, owner, draws), ref, scene["width"])


def test_both_kernel_forms_give_the_same_bits(ctx, set_opt):
    """interp_form lane (every lane fetches its owner) and wave (a wave whose pixels share one owner fetches it once; the default): the room's waves mostly share
    an owner, the sphere's never do, the boxes' and the grid's are mixed; partial waves at 129 x 67"""
    for form in ("lane", "wave"):
        set_opt("interp_form", form)
        for name in ("room_129x67_s1", "room_64x40_s4", "sphere_129x67_s4", "boxes_129x67_s1", "grid_129x67_s4", "room_16x16_s1"):
            scene = IC.cases()[name]
            for k, (owner, (ref, _)) in enumerate(zip(IC.owners(name)[0], IC.expected(name))):
                assert_planes(f"{form} form, {name} plane {k}", run(ctx, scene, owner), ref, scene["width"])


# ---- 2: any owner plane is safe ------------------------------------------------------------------------------------------------------------------------------------------
def test_garbage_owner_plane_gives_no_owner_records_and_nothing_else(ctx):
    name = "boxes_64x40_s1"
    scene = IC.cases()[name]
    total = I.total_triangles(scene)
    rng = np.random.default_rng(3)
    owner = rng.integers(total, 2 ** 32, size=(40, 64), dtype=np.uint64).astype(np.uint32)          # every value at or beyond the triangle count
    owner[0, :8] = (total, total + 1, 0xFFFFFFFF, 0xFFFFFFFE, 0x80000000, 2 ** 29, 2 ** 31 - 1, total)
    got = run(ctx, scene, owner)
    for k in ("ip0", "ip1"):
        assert not got[k].any()
    assert not got["ip2"][..., :3].any() and (got["ip2"][..., 3] == 0xFFFFFFFF).all()
    for k in ("sv_curr", "sv_prev"):
        assert not got[k][..., :3].any() and (got[k][..., 3] == 0x3F800000).all()
    # the same plane with valid owners scattered in: those pixels and no others carry records; a mesh whose indices point past its vertices owns nothing
    valid = rng.random((40, 64)) < 0.3
    owner2 = np.where(valid, rng.integers(0, total, size=(40, 64)), owner).astype(np.uint32)
    assert_planes("garbage with valid owners", run(ctx, scene, owner2), I.interpolate(scene, owner2), 64)
    d = dict(scene["draws"][0])
    d["indices"] = d["indices"].copy()
    d["indices"][3::7] = 24 + (d["indices"][3::7] % 3)                                                # 24, 25, 26: one past the box's 24 vertices and beyond
    broken = IC.scene(64, 40, 1, [d])
    ref = I.interpolate(broken, owner2)
    assert (ref["ip2"][..., 3][valid] == 0xFFFFFFFF).sum() > 20, "some valid q meet a triangle with a bad index"
    assert_planes("indices past the vertex buffer", run(ctx, broken, owner2), ref, 64)


# ---- 3, 4, 5 ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_pitched_outputs_keep_their_padding(ctx):
    for name in ("room_129x67_s1", "grid_64x40_s4"):
        scene = IC.cases()[name]
        w = scene["width"]
        got = run(ctx, scene, IC.owners(name)[0][0], pad=5, sv_pad=3)
        assert_planes(f"pitched {name}", got, IC.expected(name)[0][0], w)
        sent = np.float32(SENT).view(np.uint32)
        for k in PLANES:
            assert (got[k][:, w:] == sent).all(), f"{name}: the padding of {k} was written"
    # a pitched owner plane
    name = "room_64x40_s1"
    scene, owner = IC.cases()[name], IC.owners(name)[0][0]
    wide = torch.full((40, 71), 0x12345, dtype=torch.int32, device="cuda")
    wide[:, :64] = dev_owner(owner)
    res = ctx.scene_interpolants([device_draw(d) for d in scene["draws"]], 64, 40, wide[:, :64], sv=True)
    torch.cuda.synchronize()
    assert_planes("pitched owner", {k: res[k].cpu().numpy().view(np.uint32) for k in PLANES}, IC.expected(name)[0][0], 64)


def test_without_the_sv_planes(ctx):
    name = "room_64x40_s1"
    scene = IC.cases()[name]
    draws = [device_draw(d) for d in scene["draws"]]
    for d in draws:
        d.wvp_prev = None                                                                            # may be NULL when no svPosition plane is asked for
    got = run(ctx, scene, IC.owners(name)[0][0], draws, sv=False)
    assert set(got) == set(PLANES[:3])
    assert_planes("ip planes alone", got, IC.expected(name)[0][0], 64, PLANES[:3])


def test_prefilled_work_buffer_and_second_call(ctx):
    name = "room_129x67_s4"
    scene = IC.cases()[name]
    need = capi.scene_interpolants_work_bytes(len(scene["draws"]))
    work = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    for label in ("0xFF-filled work buffer", "second call on the same buffer"):
        assert_planes(f"{name}: {label}", run(ctx, scene, IC.owners(name)[0][1], work=work[:need]), IC.expected(name)[1][0], 129)
    assert (work[need:] == 0xFF).all(), "the call wrote past vqhip_scene_interpolants_work_bytes"


def test_non_default_stream(ctx):
    s = torch.cuda.Stream()
    name = "sphere_64x40_s4"
    assert_planes("side stream", run(ctx, IC.cases()[name], IC.owners(name)[0][2], stream=s), IC.expected(name)[2][0], 64)


# ---- 6: refusals -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx):
    name = "boxes_64x40_s1"
    scene = IC.cases()[name]
    d = scene["draws"][0]
    dd = device_draw(d)
    w, h = 64, 40
    back, _ = targets(w, h)
    owner = dev_owner(IC.owners(name)[0][0])
    need = capi.scene_interpolants_work_bytes(1)
    work = torch.full((need,), 0x3C, dtype=torch.uint8, device="cuda")
    lib, hnd, st = ctx.lib, ctx._h, ctx._stream()

    def call(ndraws=1, wptr=None, wbytes=None, draws_null=False, out_null=False, width=w, height=h, optr=None, opitch=0, **over):
        draw = abi.SceneSurfaceDraw()
        draw.mesh.positions, draw.mesh.strideBytes, draw.mesh.numVertices = dd.vertices.data_ptr(), dd.vertices.stride(0) * 4, dd.vertices.shape[0]
        draw.mesh.indices, draw.mesh.indexBits, draw.mesh.numIndices = dd.indices.data_ptr(), d["bits"], dd.indices.numel()
        draw.matWorldViewProj, draw.matWorld, draw.matNormal, draw.matWorldViewProjPrev = dd.wvp.data_ptr(), dd.world.data_ptr(), dd.normal.data_ptr(), dd.wvp_prev.data_ptr()
        draw.numInstances, draw.materialIndex = dd.wvp.shape[0], d["material"]
        tg = abi.SceneInterpolantTargets()
        tg.ip0, tg.ip1, tg.ip2 = (back[k].data_ptr() for k in PLANES[:3])
        tg.svPositionCurr, tg.svPositionPrev = back["sv_curr"].data_ptr(), back["sv_prev"].data_ptr()
        for k, val in over.items():
            obj, field = {"m": (draw.mesh, k[2:]), "d": (draw, k[2:]), "t": (tg, k[2:])}[k[0]]
            setattr(obj, field, val)
        return lib.vqhip_scene_interpolants(hnd, st, None if draws_null else C.pointer(draw), ndraws, width, height,
                                            C.c_void_p(owner.data_ptr() if optr is None else optr), opitch, None if out_null else C.byref(tg),
                                            C.c_void_p(work.data_ptr() if wptr is None else wptr), work.numel() if wbytes is None else wbytes)
    INV = abi.VQHIP_ERR_INVALID_ARG
    ip0 = back["ip0"].data_ptr()
    cases = [("NULL draws", dict(draws_null=True)), ("NULL out", dict(out_null=True)), ("NULL ip0", dict(t_ip0=None)), ("NULL ip1", dict(t_ip1=None)),
             ("NULL ip2", dict(t_ip2=None)), ("NULL owner", dict(optr=0)), ("NULL work", dict(wptr=0)), ("negative numDraws", dict(ndraws=-1)),
             ("svPositionCurr alone", dict(t_svPositionPrev=None)), ("svPositionPrev alone", dict(t_svPositionCurr=None)),
             ("sv planes without matWorldViewProjPrev", dict(d_matWorldViewProjPrev=None)),
             ("NULL positions", dict(m_positions=None)), ("NULL indices", dict(m_indices=None)), ("NULL matWorldViewProj", dict(d_matWorldViewProj=None)),
             ("NULL matWorld", dict(d_matWorld=None)), ("NULL matNormal", dict(d_matNormal=None)),
             ("width 0", dict(width=0)), ("height 0", dict(height=0)), ("width above the limit", dict(width=abi.SCENE_DEPTH_MAX_DIM + 1)),
             ("height above the limit", dict(height=abi.SCENE_DEPTH_MAX_DIM + 1)),
             ("pitch below the row", dict(t_pitch=w - 1)), ("negative pitch", dict(t_pitch=-w)), ("sv pitch below the row", dict(t_sv_pitch=w - 1)),
             ("negative sv pitch", dict(t_sv_pitch=-1)), ("owner pitch below the row", dict(opitch=w - 1)), ("negative owner pitch", dict(opitch=-w)),
             ("ip1 not 16-byte aligned", dict(t_ip1=back["ip1"].data_ptr() + 4)), ("sv plane not 16-byte aligned", dict(t_svPositionCurr=back["sv_curr"].data_ptr() + 8)),
             ("owner not 4-byte aligned", dict(optr=owner.data_ptr() + 2)),
             ("stride 40", dict(m_strideBytes=40)), ("stride 46", dict(m_strideBytes=46)), ("stride 12", dict(m_strideBytes=12)),
             ("indexBits 8", dict(m_indexBits=8)), ("numIndices not a multiple of 3", dict(m_numIndices=dd.indices.numel() - 1)),
             ("no instances", dict(d_numInstances=0)), ("65 instances", dict(d_numInstances=65)), ("negative materialIndex", dict(d_materialIndex=-1)),
             ("positions not 4-byte aligned", dict(m_positions=dd.vertices.data_ptr() + 2)), ("indices not aligned to their size", dict(m_indices=dd.indices.data_ptr() + 1)),
             ("matWorld not 4-byte aligned", dict(d_matWorld=dd.world.data_ptr() + 1)), ("matNormal not 4-byte aligned", dict(d_matNormal=dd.normal.data_ptr() + 2)),
             ("matWorldViewProjPrev not 4-byte aligned", dict(d_matWorldViewProjPrev=dd.wvp_prev.data_ptr() + 2)),
             ("workBytes one short", dict(wbytes=need - 1)), ("work not aligned", dict(wptr=work.data_ptr() + 16)),
             ("ip0 inside the work buffer", dict(t_ip0=work.data_ptr() + 16)), ("ip2 on the owner plane", dict(t_ip2=owner.data_ptr())),
             ("owner inside ip0", dict(optr=ip0 + 64))]
    for label, over in cases:
        assert call(**over) == INV, label
        assert len(lib.vqhip_last_error(hnd) or b"") > 10, label
    # 64 instances of 2^23 triangles are 2^29 instanced triangles: vqhip_scene_depth's limit, the q this call could be handed
    assert call(m_numIndices=3 * 2 ** 23, d_numInstances=64) == abi.VQHIP_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    for k in PLANES:
        assert (back[k] == SENT).all(), f"a refused call wrote to {k}"
    assert (work == 0x3C).all(), "a refused call wrote to the work buffer"
    assert call() == abi.VQHIP_OK
    torch.cuda.synchronize()
    assert_planes("after the refusals", {k: t.cpu().numpy().view(np.uint32) for k, t in back.items()}, IC.expected(name)[0][0], w)
    # more than 20 000 draws
    many = (abi.SceneSurfaceDraw * 20001)()
    one = abi.SceneSurfaceDraw()
    one.mesh.positions, one.mesh.strideBytes, one.mesh.numVertices = dd.vertices.data_ptr(), 44, 24
    one.mesh.indices, one.mesh.indexBits, one.mesh.numIndices = dd.indices.data_ptr(), 16, 3
    one.matWorldViewProj, one.matWorld, one.matNormal, one.matWorldViewProjPrev = dd.wvp.data_ptr(), dd.world.data_ptr(), dd.normal.data_ptr(), dd.wvp_prev.data_ptr()
    one.numInstances = 1
    for k in range(20001):
        many[k] = one
    big = torch.empty((capi.scene_interpolants_work_bytes(20001),), dtype=torch.uint8, device="cuda")
    tg = abi.SceneInterpolantTargets()
    tg.ip0, tg.ip1, tg.ip2 = (back[k].data_ptr() for k in PLANES[:3])
    assert lib.vqhip_scene_interpolants(hnd, st, many, 20001, w, h, C.c_void_p(owner.data_ptr()), 0, C.byref(tg), C.c_void_p(big.data_ptr()), big.numel()) == abi.VQHIP_ERR_UNSUPPORTED
    # the Python binding validates before it calls
    with pytest.raises(ValueError):
        ctx.scene_interpolants([dd], w, h, owner[:, :-1])
    with pytest.raises(ValueError):
        ctx.scene_interpolants([capi.SurfaceDraw(dd.vertices[:, :10], dd.indices, dd.wvp, dd.world, dd.normal, dd.wvp_prev)], w, h, owner)
    with pytest.raises(ValueError):
        ctx.scene_interpolants([capi.SurfaceDraw(dd.vertices, dd.indices, dd.wvp, dd.world, dd.normal, None)], w, h, owner, sv=True)
    with pytest.raises(ValueError):
        ctx.scene_interpolants([dd], w, h, owner, out={"ip0": torch.empty((h, w - 1, 4), dtype=torch.float32, device="cuda")})


def test_many_draws_cross_the_ring_slots(ctx):
    """1 500 draws of one triangle each (three ring slots of the draw table) and an owner plane that walks through all of them: the binary search meets every
    entry, empty draws in between own nothing and do not shift q"""
    w, h = 64, 24
    rng = np.random.default_rng(9)
    draws = []
    for k in range(1500):
        v = np.zeros((3, 11), dtype=np.float32)
        v[:, :3] = rng.uniform(-1, 1, (3, 3))
        v[:, 2] = rng.uniform(0.1, 0.9, 3)
        v[:, 3:9] = rng.uniform(-1, 1, (3, 6))
        v[:, 9:11] = rng.uniform(0, 1, (3, 2))
        m = (np.eye(4, dtype=np.float32) * np.float32(1 + k % 3))[None]
        draws.append(IC.draw(v, [0, 1, 2] if k % 10 else [], (m, m, m, m), k % 7, bits=16 if k % 2 else 32))
    scene = IC.scene(w, h, 1, draws)
    total = I.total_triangles(scene)
    assert total == 1350
    owner = (np.arange(w * h, dtype=np.uint32).reshape(h, w) * 7) % np.uint32(total + 3)
    st = {}
    ref = I.interpolate(scene, owner, stats=st)
    assert st["no_owner"] > 0 and st["owned"] > 1300
    assert_planes("1500 draws", run(ctx, scene, owner), ref, w)


# ---- 7, 8, 9: the chains ------------------------------------------------------------------------------------------------------------------------------------------------
def materials(ctx):
    """two materials, the first textured (every map bound), the second plain: (host table for the oracle, device table, what must stay alive)"""
    datas, texsets = synth.material_set(2, seed=0x718, max_dim=32)
    texsets[1] = {}
    datas[1].textureConfig = 0.0
    host_chains, keep = [], []
    dmats = (abi.MaterialDesc * 2)()
    for i, (d, ts) in enumerate(zip(datas, texsets)):
        cs = {}
        dmats[i].data = d
        for slot, img in ts.items():
            chain_o, nm = O.mip_chain_rgba8(img)
            chain_g, _ = ctx.mip_chain_rgba8(dev(img))
            cs[slot] = (chain_o, img.shape[1], img.shape[0], nm)
            keep.append(chain_g)
            setattr(dmats[i], slot, abi.Texture2D(chain_g.data_ptr(), img.shape[1], img.shape[0], nm, 0))
        host_chains.append(cs)
    return O.host_materials(datas, host_chains), dmats, keep


def ref_planes(ref):
    return [np.ascontiguousarray(ref[k]).view(np.float32) for k in PLANES[:3]]


def lights(w, h):
    pf, extra = synth.per_frame(points=synth.point_lights(12, seed=0x718), spots=synth.spot_lights(2, seed=0x718), directional=synth.directional_light())
    return pf, extra, synth.per_view(w, h)


def assert_bits(got, ref, what):
    n_bad, idx = O.bits_equal(got.cpu().numpy() if hasattr(got, "cpu") else got, ref)
    assert n_bad == 0, f"{what}: {n_bad} elements differ, first {idx.tolist()}"


def test_chain_1x_depth_interpolants_lit_frame(ctx):
    """room, 64 x 40: vqhip_scene_depth -> vqhip_scene_interpolants -> vqhip_forward_lighting_from_materials_mrt (scene colour, albedo / metalness, motion vectors)
    == the oracle's producer and shade on the statement's planes; motion vectors against the oracle's statement of ForwardLighting.hlsl:382-389"""
    name = "room_64x40_s1"
    scene, (ref, _) = IC.cases()[name], IC.expected(name)[0]
    w, h = 64, 40
    draws = [device_draw(d) for d in scene["draws"]]
    z = ctx.scene_depth([d.depth_draw() for d in draws], w, h, 1, primitive=True)
    ip = ctx.scene_interpolants(draws, w, h, z["primitive"], sv=True)
    torch.cuda.synchronize()
    assert np.array_equal(z["primitive"].cpu().numpy().view(np.uint32), IC.owners(name)[0][0]), "vqhip_scene_depth's owner plane is the statement's"
    assert_planes("planes of the chain", {k: ip[k].cpu().numpy().view(np.uint32) for k in PLANES}, ref, w)
    hmats, dmats, keep = materials(ctx)
    pf, extra, pv = lights(w, h)
    out, alb, mv = ctx.forward_lighting_from_materials_mrt([ip[k] for k in PLANES[:3]], dmats, pf, pv, albedo_fmt=abi.FMT_RGBA16F, motion_fmt=abi.FMT_RG16F,
                                                           sv_curr=ip["sv_curr"], sv_prev=ip["sv_prev"], extra_point=extra)
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        gb = O.gbuffer_from_materials(ref_planes(ref), hmats, pf.fAmbientLightingFactor)
        want = O.forward_lighting(gb, pf, pv, abi.FMT_RGBA16F, extra_point=extra)
        want_a, want_m = O.psmain_extra_targets(gb, ref["sv_curr"].view(np.float32), ref["sv_prev"].view(np.float32), abi.FMT_RGBA16F, abi.FMT_RG16F)
    assert_bits(out, want, "lit frame of the rasterised room")
    idx = ip["ip2"][..., 3].contiguous().view(torch.int32).cpu().numpy()                              # after the call: alpha-mask discards are marked -1
    cov = (idx >= 0) & (idx < 2)
    assert cov.mean() > 0.5 and set(np.unique(idx[cov])) == {0, 1}, "both materials are on screen"
    assert_bits(np.ascontiguousarray(alb.cpu().numpy()[cov]), np.ascontiguousarray(want_a[cov]), "albedo / metalness")
    assert_bits(np.ascontiguousarray(mv.cpu().numpy()[cov]), np.ascontiguousarray(want_m[cov]), "motion vectors")
    assert (np.abs(want_m[cov].astype(np.float32)) > 0).mean() > 0.9, "the camera moved"


def test_chain_4x_layers_gbuffers_lit_resolve(ctx):
    """room, 64 x 40, 4x MSAA: four vqhip_scene_interpolants calls on layerPrimitive[k] -> four vqhip_gbuffer_from_materials -> vqhip_forward_lighting_msaa under
    vqhip_scene_depth's masks == the oracle per layer on the statement's planes, resolved by tests/msaa_ref.py under the statement's masks. No constant
    record per primitive: every layer's record is interpolated."""
    name = "room_64x40_s4"
    scene, exp = IC.cases()[name], IC.expected(name)
    w, h = 64, 40
    draws = [device_draw(d) for d in scene["draws"]]
    z = ctx.scene_depth([d.depth_draw() for d in draws], w, h, 4, layers=4)
    hmats, dmats, keep = materials(ctx)
    pf, extra, pv = lights(w, h)
    layers_dev = []
    for k in range(4):
        ip = ctx.scene_interpolants(draws, w, h, z["layer_primitive"][k])
        torch.cuda.synchronize()
        assert_planes(f"layer {k}", {p: ip[p].cpu().numpy().view(np.uint32) for p in PLANES[:3]}, exp[k][0], w, PLANES[:3])
        layers_dev.append(ctx.gbuffer_from_materials([ip[p] for p in PLANES[:3]], dmats, pf.fAmbientLightingFactor))
    got = ctx.forward_lighting_msaa(layers_dev, z["coverage"], pf, pv, out_fmt=abi.FMT_RGBA16F, extra_point=extra)
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        shaded = [O.forward_lighting(O.gbuffer_from_materials(ref_planes(exp[k][0]), hmats, pf.fAmbientLightingFactor), pf, pv, abi.FMT_RGBA16F, extra_point=extra)
                  for k in range(4)]
    cov = IC.owners(name)[1]
    assert_bits(got, msaa_ref.resolve(shaded, cov, None, abi.FMT_RGBA16F), "lit 4x resolve of the rasterised room")
    assert sum(int((c != 0).sum()) for c in cov[1:]) > 100, "the room has edge pixels"


def test_chain_scene_normals(ctx):
    name = "room_64x40_s1"
    scene, (ref, _) = IC.cases()[name], IC.expected(name)[0]
    ip = ctx.scene_interpolants([device_draw(d) for d in scene["draws"]], 64, 40, dev_owner(IC.owners(name)[0][0]))
    hmats, dmats, keep = materials(ctx)
    got = ctx.scene_normals_from_materials([ip[k] for k in PLANES[:3]], dmats)
    torch.cuda.synchronize()
    want = O.scene_normals_from_materials(ref_planes(ref), hmats)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want), "R10G10B10A2 normals of the rasterised room"


# ---- 10: the C++ adaptor -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["room_64x40_s1", "room_64x40_s4"])
def test_cpp_adaptor_program(tmp_path, name):
    """tests/cpp/test_passes_interpolants (built by vqengine_amd/csrc/Makefile behind the library it links): vqhip::DepthPrePass then vqhip::SceneInterpolantsPass per owner plane, as a child process"""
    scene = IC.cases()[name]
    lines = []
    for k, d in enumerate(scene["draws"]):
        d["positions"].tofile(tmp_path / f"d{k}_vertices.bin")
        (d["indices"].astype(np.uint16) if d["bits"] == 16 else d["indices"].astype(np.uint32)).tofile(tmp_path / f"d{k}_indices.bin")
        for key, fn in (("wvp", "wvp"), ("world", "world"), ("normal", "normal"), ("wvp_prev", "prev")):
            d[key].tofile(tmp_path / f"d{k}_{fn}.bin")
        lines.append(f"{d['positions'].shape[0]} {d['positions'].shape[1] * 4} {d['bits']} {len(d['indices'])} {d['wvp'].shape[0]} {d['material']} {d['cull']}")
    (tmp_path / "draws.txt").write_text("\n".join(lines) + "\n")
    w, h = scene["width"], scene["height"]
    r = subprocess.run([EXE, str(tmp_path), str(w), str(h), str(scene["samples"])], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "scene interpolants adaptor OK" in r.stdout, r.stdout + r.stderr
    for p, (owner, (ref, _)) in enumerate(zip(IC.owners(name)[0], IC.expected(name))):
        assert np.array_equal(np.fromfile(tmp_path / f"owner{p}.bin", np.uint32).reshape(h, w), owner)
        assert_planes(f"adaptor plane {p}", {k: np.fromfile(tmp_path / f"{k}_{p}.bin", np.uint32).reshape(h, w, 4) for k in PLANES}, ref, w)
