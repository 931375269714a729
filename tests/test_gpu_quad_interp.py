"""docs/DESIGN_DETAILS.md §7.20 on the GPU: vqhip_scene_quad_interpolants and the three _quad producers, every plane compared as integers against
tests/quad_interp_ref.py, no tolerance. The scenes are tests/quad_interp_cases.py's: §7.18's room, boxes, sphere and grid at 16 x 16, 64 x 40 and 129 x 67 with 1
and 4 samples (one call per layer), and the masked cards. The chains at the end run meshes -> masked depth -> quad resolve -> lit frame inside the library."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import msaa_ref
from tests import oracle_lib as O
from tests import quad_interp_cases as QC
from tests import quad_interp_ref as Q
from tests import scene_interp_ref as I
from vqengine_amd import abi, capi, synth

pytestmark = pytest.mark.gpu
PLANES = QC.PLANES
AMBIENT = 0.055
SENT = -7.0
_KEEP = []
INCONSISTENT, disagreements = QC.INCONSISTENT, QC.disagreements


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # a copy: the shared expectations are read-only


def dev_owner(owner):
    return dev(np.ascontiguousarray(owner, dtype=np.uint32).view(np.int32))


def device_draw(d):
    idx = d["indices"]
    ix = dev(idx.astype(np.uint16).view(np.int16)) if d["bits"] == 16 else dev(idx.astype(np.int32))
    return capi.SurfaceDraw(dev(d["positions"]), ix, dev(d["wvp"]), dev(d["world"]), dev(d["normal"]), dev(d["wvp_prev"]), d["material"])


def lights(w, h):
    pf, extra = synth.per_frame(points=synth.point_lights(12, seed=0x720), spots=synth.spot_lights(2, seed=0x720), directional=synth.directional_light())
    return pf, extra, synth.per_view(w, h)


def assert_bits(got, ref, what):
    n_bad, idx = O.bits_equal(got.cpu().numpy() if hasattr(got, "cpu") else got, ref)
    assert n_bad == 0, f"{what}: {n_bad} elements differ, first {idx.tolist()}"


@pytest.fixture(autouse=True)
def _release_device_chains():
    yield
    _KEEP.clear()


def device_materials(ctx, name):
    datas, chains, masked = QC.material_inputs(name)
    arr = (abi.MaterialDesc * len(datas))()
    for i, (d, cs) in enumerate(zip(datas, chains)):
        arr[i].data = d
        for slot, (chain, n, w, h) in cs.items():
            t = dev(chain)
            _KEEP.append(t)
            setattr(arr[i], slot, abi.Texture2D(t.data_ptr(), w, h, n, 0))
        if masked[i]:
            arr[i].texDiffuse.reserved = abi.MATERIAL_ALPHA_MASKED
    return arr


def targets(w, h, sv=True, pad=0):
    back = {k: torch.full((h, w + pad, 4), SENT, dtype=torch.float32, device="cuda") for k in PLANES if sv or not k.startswith("sv")}
    return back, {k: t[:, :w] for k, t in back.items()}


def run(ctx, scene, owner, draws=None, sv=True, pad=0, work=None, stream=None):
    w, h = scene["width"], scene["height"]
    back, out = targets(w, h, sv, pad)
    ctx.scene_quad_interpolants(draws if draws is not None else [device_draw(d) for d in scene["draws"]], w, h, dev_owner(owner), sv=sv, out=out, work=work, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return {k: t.cpu().numpy().view(np.uint32) for k, t in back.items()}


def assert_planes(name, got, ref, w, planes=PLANES):
    for k in planes:
        g, e = got[k][:, :w], ref[k]
        bad = np.argwhere(g != e)
        assert len(bad) == 0, f"{name} {k}: {len(bad)} of {e.size} words differ from tests/quad_interp_ref.py, first at {bad[0].tolist()}: {g[tuple(bad[0])]:#x} != {e[tuple(bad[0])]:#x}"


# ---- vqhip_scene_quad_interpolants -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(QC.cases()))
def test_case_matches_the_statement(ctx, name):
    """all six planes of every owner plane of the case; the five existing planes are also what vqhip_scene_interpolants writes on the same inputs"""
    scene = QC.cases()[name]
    w, h = scene["width"], scene["height"]
    draws = [device_draw(d) for d in scene["draws"]]
    for k, (owner, (ref, _)) in enumerate(zip(QC.owners(name)[0], QC.expected(name))):
        got = run(ctx, scene, owner, draws)
        assert_planes(f"{name} plane {k}", got, ref, w)
        plain = ctx.scene_interpolants(draws, w, h, dev_owner(owner), sv=True)
        torch.cuda.synchronize()
        for p in PLANES[:5]:
            assert np.array_equal(plain[p].cpu().numpy().view(np.uint32), got[p]), f"{name} plane {k}: {p} differs from vqhip_scene_interpolants"


def test_both_kernel_forms_give_the_same_bits(ctx, set_opt):
    for form in ("lane", "wave"):
        set_opt("interp_form", form)
        for name in ("room_129x67_s1", "room_64x40_s4", "sphere_129x67_s4", "boxes_129x67_s1", "grid_129x67_s4", "room_16x16_s1", "cards_minified_64x48_s4"):
            scene = QC.cases()[name]
            for k, (owner, (ref, _)) in enumerate(zip(QC.owners(name)[0], QC.expected(name))):
                assert_planes(f"{form} form, {name} plane {k}", run(ctx, scene, owner), ref, scene["width"])
                assert_planes(f"{form} form without sv, {name} plane {k}", run(ctx, scene, owner, sv=False), ref, scene["width"], PLANES[:3] + ("quad_uv",))


def test_garbage_owner_plane_and_indices_past_the_vertex_buffer(ctx):
    name = "boxes_64x40_s1"
    scene = QC.cases()[name]
    total = I.total_triangles(scene)
    rng = np.random.default_rng(3)
    owner = rng.integers(total, 2 ** 32, size=(40, 64), dtype=np.uint64).astype(np.uint32)
    owner[0, :8] = (total, total + 1, 0xFFFFFFFF, 0xFFFFFFFE, 0x80000000, 2 ** 29, 2 ** 31 - 1, total)
    got = run(ctx, scene, owner)
    assert not got["quad_uv"].any() and not got["ip0"].any() and (got["ip2"][..., 3] == 0xFFFFFFFF).all()
    valid = rng.random((40, 64)) < 0.3
    owner2 = np.where(valid, rng.integers(0, total, size=(40, 64)), owner).astype(np.uint32)
    assert_planes("garbage with valid owners", run(ctx, scene, owner2), Q.interpolate(scene, owner2), 64)
    d = dict(scene["draws"][0])
    d["indices"] = d["indices"].copy()
    d["indices"][3::7] = 24 + (d["indices"][3::7] % 3)
    broken = dict(scene, draws=[d])
    ref = Q.interpolate(broken, owner2)
    assert (ref["ip2"][..., 3][valid] == 0xFFFFFFFF).sum() > 20
    assert_planes("indices past the vertex buffer", run(ctx, broken, owner2), ref, 64)


def test_pitched_quad_plane_keeps_its_padding(ctx):
    name = "room_129x67_s1"
    scene = QC.cases()[name]
    w, h = 129, 67
    back, out = targets(w, h)
    wide = torch.full((h, w + 7, 4), SENT, dtype=torch.float32, device="cuda")         # quad_uv alone pitched: its pitch is its own
    out["quad_uv"] = wide[:, :w]
    ctx.scene_quad_interpolants([device_draw(d) for d in scene["draws"]], w, h, dev_owner(QC.owners(name)[0][0]), sv=True, out=out)
    torch.cuda.synchronize()
    got = {k: t.cpu().numpy().view(np.uint32) for k, t in back.items()}
    got["quad_uv"] = wide.cpu().numpy().view(np.uint32)
    assert_planes("pitched quadUV", got, QC.expected(name)[0][0], w)
    assert (got["quad_uv"][:, w:] == np.float32(SENT).view(np.uint32)).all(), "the padding of quadUV was written"
    got = run(ctx, scene, QC.owners(name)[0][0], pad=5)
    assert_planes("all pitched", got, QC.expected(name)[0][0], w)
    for k in PLANES:
        assert (got[k][:, w:] == np.float32(SENT).view(np.uint32)).all(), k


def test_prefilled_work_buffer_second_call_and_side_stream(ctx):
    name = "room_129x67_s4"
    scene = QC.cases()[name]
    need = capi.scene_interpolants_work_bytes(len(scene["draws"]))
    work = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    for label in ("0xFF-filled work buffer", "second call on the same buffer"):
        assert_planes(f"{name}: {label}", run(ctx, scene, QC.owners(name)[0][1], work=work[:need]), QC.expected(name)[1][0], 129)
    assert (work[need:] == 0xFF).all()
    s = torch.cuda.Stream()
    name = "sphere_64x40_s4"
    assert_planes("side stream", run(ctx, QC.cases()[name], QC.owners(name)[0][2], stream=s), QC.expected(name)[2][0], 64)


def test_many_draws_cross_the_ring_slots(ctx):
    w, h = 64, 24
    rng = np.random.default_rng(9)
    draws = []
    from tests import scene_interp_cases as IC
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
    owner = (np.arange(w * h, dtype=np.uint32).reshape(h, w) * 7) % np.uint32(total + 3)
    assert_planes("1500 draws", run(ctx, scene, owner), Q.interpolate(scene, owner), w)


def test_new_refusals_launch_nothing(ctx):
    name = "boxes_64x40_s1"
    scene = QC.cases()[name]
    dd = device_draw(scene["draws"][0])
    w, h = 64, 40
    back, _ = targets(w, h)
    owner = dev_owner(QC.owners(name)[0][0])
    need = capi.scene_interpolants_work_bytes(1)
    work = torch.full((need,), 0x3C, dtype=torch.uint8, device="cuda")
    lib, hnd, st = ctx.lib, ctx._h, ctx._stream()
    draw = abi.SceneSurfaceDraw()
    draw.mesh.positions, draw.mesh.strideBytes, draw.mesh.numVertices = dd.vertices.data_ptr(), dd.vertices.stride(0) * 4, dd.vertices.shape[0]
    draw.mesh.indices, draw.mesh.indexBits, draw.mesh.numIndices = dd.indices.data_ptr(), scene["draws"][0]["bits"], dd.indices.numel()
    draw.matWorldViewProj, draw.matWorld, draw.matNormal, draw.matWorldViewProjPrev = dd.wvp.data_ptr(), dd.world.data_ptr(), dd.normal.data_ptr(), dd.wvp_prev.data_ptr()
    draw.numInstances, draw.materialIndex = dd.wvp.shape[0], scene["draws"][0]["material"]

    def call(out_null=False, **over):
        tg = abi.SceneQuadTargets()
        tg.planes.ip0, tg.planes.ip1, tg.planes.ip2 = (back[k].data_ptr() for k in PLANES[:3])
        tg.planes.svPositionCurr, tg.planes.svPositionPrev = back["sv_curr"].data_ptr(), back["sv_prev"].data_ptr()
        tg.quadUV = back["quad_uv"].data_ptr()
        for k, val in over.items():
            setattr(tg.planes if k.startswith("p_") else tg, k[2:] if k.startswith("p_") else k, val)
        return lib.vqhip_scene_quad_interpolants(hnd, st, C.pointer(draw), 1, w, h, C.c_void_p(owner.data_ptr()), 0, None if out_null else C.byref(tg),
                                                 C.c_void_p(work.data_ptr()), work.numel())
    q = back["quad_uv"].data_ptr()
    cases = [("NULL out", dict(out_null=True)), ("NULL quadUV", dict(quadUV=None)), ("quadUV misaligned", dict(quadUV=q + 8)), ("quad pitch below width", dict(quad_pitch=w - 1)),
             ("negative quad pitch", dict(quad_pitch=-w)), ("quadUV on the owner plane", dict(quadUV=owner.data_ptr())), ("quadUV in the work buffer", dict(quadUV=work.data_ptr() + 16)),
             ("quadUV on ip1", dict(quadUV=back["ip1"].data_ptr() + 64)), ("quadUV on sv_prev", dict(quadUV=back["sv_prev"].data_ptr())),
             ("a sibling's refusal: NULL ip0", dict(p_ip0=None)), ("a sibling's refusal: pitch", dict(p_pitch=w - 1))]
    for label, over in cases:
        assert call(**over) == abi.VQHIP_ERR_INVALID_ARG, label
        assert len(lib.vqhip_last_error(hnd) or b"") > 10, label
    torch.cuda.synchronize()
    for k in PLANES:
        assert (back[k] == SENT).all(), f"a refused call wrote to {k}"
    assert (work == 0x3C).all()
    assert call() == abi.VQHIP_OK
    torch.cuda.synchronize()
    assert_planes("after the refusals", {k: t.cpu().numpy().view(np.uint32) for k, t in back.items()}, QC.expected(name)[0][0], w)
    with pytest.raises(ValueError):
        ctx.scene_quad_interpolants([dd], w, h, owner, out={"quad_uv": torch.empty((h, w, 3), dtype=torch.float32, device="cuda")})


# ---- the producers ----------------------------------------------------------------------------------------------------------------------------------------------------------
def dev_planes(out):
    ip = [dev(np.array(out[k]).view(np.float32)) for k in PLANES[:3]]
    return ip, dev(np.array(out["quad_uv"]).view(np.float32))


PRODUCER_SET = QC.PRODUCER_NAMES + tuple(f"cards_{n}" for n in QC.CARD_NAMES)


@pytest.mark.parametrize("name", PRODUCER_SET)
def test_gbuffer_quad_matches_the_exploded_oracle(ctx, name):
    """every owner plane of the case, with SSAO: the four planes and ip2.w after the call (the discard's -1)"""
    scene = QC.cases()[name]
    mats = device_materials(ctx, name)
    ssao = dev(QC.ssao_plane(scene["width"], scene["height"]))
    for layer, (out, _) in enumerate(QC.expected(name)):
        ip, quv = dev_planes(out)
        gb = ctx.gbuffer_from_materials_quad(ip, mats, AMBIENT, quv, ssao=ssao)
        torch.cuda.synchronize()
        want, want_idx = QC.expected_gbuffer(name, layer, True)
        for k in range(4):
            assert_bits(gb[k], want[k], f"{name} layer {layer} gb{k}")
        assert np.array_equal(ip[2][..., 3].contiguous().view(torch.int32).cpu().numpy(), want_idx), f"{name} layer {layer}: ip2.w after the call"


@pytest.mark.parametrize("dxc", [0, 1])
def test_both_arithmetic_readings_without_ssao_and_the_pre_pass_normals(ctx, dxc):
    """vqhip_gbuffer_from_materials_quad and vqhip_scene_normals_from_materials_quad (both formats) against the exploded oracle switched to the same reading"""
    ctx.set_arithmetic(dxc)
    try:
        for name, layer in (("room_64x40_s1", 0), ("cards_minified_64x48_s1", 0), ("boxes_129x67_s4", 1), ("room_129x67_s1", 0)):
            mats = device_materials(ctx, name)
            out, _ = QC.expected(name)[layer]
            ip, quv = dev_planes(out)
            nrm = ctx.scene_normals_from_materials_quad(ip, mats, quv)
            nrm32 = ctx.scene_normals_from_materials_quad(ip, mats, quv, out_fmt=abi.FMT_RGBA32F)
            gb = ctx.gbuffer_from_materials_quad(ip, mats, AMBIENT, quv)
            torch.cuda.synchronize()
            want, want_idx = QC.expected_gbuffer(name, layer, False, dxc)
            for k in range(4):
                assert_bits(gb[k], want[k], f"{name} gb{k}, dxc {dxc}")
            assert np.array_equal(ip[2][..., 3].contiguous().view(torch.int32).cpu().numpy(), want_idx), name
            assert np.array_equal(nrm.cpu().numpy().view(np.uint32), QC.expected_scene_normals(name, layer, abi.FMT_R10G10B10A2_UNORM, dxc)), f"{name}, dxc {dxc}"
            assert_bits(nrm32, QC.expected_scene_normals(name, layer, abi.FMT_RGBA32F, dxc), f"{name} float normals, dxc {dxc}")
        if dxc:                                                           # the reading reaches the record: the two expectations are not one
            a, b = QC.expected_gbuffer("room_129x67_s1", 0, False, 0)[0], QC.expected_gbuffer("room_129x67_s1", 0, False, 1)[0]
            assert any(O.bits_equal(x, y)[0] > 0 for x, y in zip(a, b))
    finally:
        ctx.set_arithmetic(0)


@pytest.mark.parametrize("dxc", [0, 1])
def test_fused_form_equals_gbuffer_quad_plus_forward_lighting_mrt(ctx, dxc):
    """both readings, with and without SSAO, with the extra targets: on every covered pixel"""
    ctx.set_arithmetic(dxc)
    try:
        for name, use_ssao in (("room_64x40_s1", True), ("cards_minified_64x48_s1", False), ("room_129x67_s1", False)):
            scene = QC.cases()[name]
            w, h = scene["width"], scene["height"]
            mats = device_materials(ctx, name)
            out, _ = QC.expected(name)[0]
            pf, extra, pv = lights(w, h)
            pf.fAmbientLightingFactor = AMBIENT
            ssao = dev(QC.ssao_plane(w, h)) if use_ssao else None
            svc, svp = dev(np.array(out["sv_curr"]).view(np.float32)), dev(np.array(out["sv_prev"]).view(np.float32))
            ip, quv = dev_planes(out)
            gb = ctx.gbuffer_from_materials_quad(ip, mats, AMBIENT, quv, ssao=ssao)
            want, want_a, want_m = ctx.forward_lighting_mrt(gb, pf, pv, albedo_fmt=abi.FMT_RGBA16F, motion_fmt=abi.FMT_RG16F, sv_curr=svc, sv_prev=svp, extra_point=extra)
            ip2, _ = dev_planes(out)
            got, got_a, got_m = ctx.forward_lighting_from_materials_quad(ip2, mats, pf, pv, quv, albedo_fmt=abi.FMT_RGBA16F, motion_fmt=abi.FMT_RG16F, sv_curr=svc, sv_prev=svp,
                                                                         ssao=ssao, extra_point=extra)
            plain = ctx.forward_lighting_from_materials_quad(dev_planes(out)[0], mats, pf, pv, quv, ssao=ssao, extra_point=extra)
            torch.cuda.synchronize()
            assert_bits(got, want.cpu().numpy(), f"{name} scene colour")
            assert_bits(plain, want.cpu().numpy(), f"{name} scene colour without targets")
            cov = ip2[2][..., 3].contiguous().view(torch.int32).cpu().numpy() >= 0
            assert cov.sum() > 100
            assert_bits(np.ascontiguousarray(got_a.cpu().numpy()[cov]), np.ascontiguousarray(want_a.cpu().numpy()[cov]), f"{name} albedo")
            assert_bits(np.ascontiguousarray(got_m.cpu().numpy()[cov]), np.ascontiguousarray(want_m.cpu().numpy()[cov]), f"{name} motion vectors")
            wgb, _ = QC.expected_gbuffer(name, 0, use_ssao, dxc)
            with np.errstate(all="ignore"), QC.oracle_arithmetic(dxc):
                want_o = O.forward_lighting(wgb, pf, pv, abi.FMT_RGBA16F, extra_point=extra)
                want_oa, want_om = O.psmain_extra_targets(wgb, np.array(out["sv_curr"]).view(np.float32), np.array(out["sv_prev"]).view(np.float32), abi.FMT_RGBA16F, abi.FMT_RG16F)
            assert_bits(got, want_o, f"{name} against the oracle, dxc {dxc}")
            assert_bits(np.ascontiguousarray(got_a.cpu().numpy()[cov]), np.ascontiguousarray(want_oa[cov]), f"{name} albedo against the oracle")
            assert_bits(np.ascontiguousarray(got_m.cpu().numpy()[cov]), np.ascontiguousarray(want_om[cov]), f"{name} motion vectors against the oracle")
    finally:
        ctx.set_arithmetic(0)


@pytest.mark.parametrize("dxc", [0, 1])
def test_on_single_owner_quads_each_quad_producer_equals_its_sibling(ctx, dxc):
    """a frame of single-owner, in-image quads (even size, the material constant per aligned quad) with the true neighbours' uv as the quad plane"""
    ctx.set_arithmetic(dxc)
    try:
        w, h = 48, 26
        ipn = QC.single_owner_frame(w, h, 4, 0x720)
        quv, ok = Q.neighbour_quad_uv(ipn[0], ipn[1])
        assert ok.all()
        mats = device_materials(ctx, "room_64x40_s1")
        mats[1].texDiffuse.reserved = abi.MATERIAL_ALPHA_MASKED
        ssao = dev(QC.ssao_plane(w, h))
        pf, extra, pv = lights(w, h)
        dq = dev(quv.view(np.float32))
        fresh = lambda: [dev(p) for p in ipn]      # noqa: E731
        a, b = fresh(), fresh()
        for x, y in zip(ctx.gbuffer_from_materials(a, mats, AMBIENT, ssao=ssao), ctx.gbuffer_from_materials_quad(b, mats, AMBIENT, dq, ssao=ssao)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32)), "the discards' -1"
        assert torch.equal(ctx.scene_normals_from_materials(fresh(), mats), ctx.scene_normals_from_materials_quad(fresh(), mats, dq))
        x = ctx.forward_lighting_from_materials(fresh(), mats, pf, pv, ssao=ssao, extra_point=extra)
        y = ctx.forward_lighting_from_materials_quad(fresh(), mats, pf, pv, dq, ssao=ssao, extra_point=extra)
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))
    finally:
        ctx.set_arithmetic(0)


def test_producer_refusals(ctx):
    name = "room_64x40_s1"
    out, _ = QC.expected(name)[0]
    ip, quv = dev_planes(out)
    mats = device_materials(ctx, name)
    w, h = 64, 40
    lib, hnd, st = ctx.lib, ctx._h, ctx._stream()
    gbt = [torch.full((h, w, 4), SENT, dtype=torch.float32, device="cuda") for _ in range(4)]
    inter = abi.Interpolants(ip[0].data_ptr(), ip[1].data_ptr(), ip[2].data_ptr(), w, h, w)
    gb = abi.GBuffer(*(t.data_ptr() for t in gbt), w, h, w)
    nrm = torch.full((h, w), 7, dtype=torch.int32, device="cuda")
    col = torch.full((h, w, 4), SENT, dtype=torch.float16, device="cuda")
    pf, extra, pv = lights(w, h)
    q = quv.data_ptr()
    def refused(rc, label):
        assert rc == abi.VQHIP_ERR_INVALID_ARG, label
        assert b"quad" in (lib.vqhip_last_error(hnd) or b""), (label, lib.vqhip_last_error(hnd))
    for label, ptr, pitch in (("NULL", None, 0), ("misaligned", q + 4, 0), ("negative pitch", q, -1), ("pitch below the width", q, w - 1), ("on gb1", gbt[1].data_ptr(), 0),
                              ("on ip2", ip[2].data_ptr() + 160, 0)):
        refused(lib.vqhip_gbuffer_from_materials_quad(hnd, st, C.byref(inter), mats, len(mats), 0.1, None, C.byref(gb), C.c_void_p(ptr), pitch), f"gbuffer: {label}")
    for label, ptr, pitch in (("NULL", None, 0), ("misaligned", q + 8, 0), ("negative pitch", q, -5), ("pitch below the width", q, 1), ("on the output", nrm.data_ptr(), 0)):
        refused(lib.vqhip_scene_normals_from_materials_quad(hnd, st, C.byref(inter), mats, len(mats), C.c_void_p(nrm.data_ptr()), abi.FMT_R10G10B10A2_UNORM, 0,
                                                            C.c_void_p(ptr), pitch), f"scene normals: {label}")
    alb = torch.full((h, w, 4), SENT, dtype=torch.float16, device="cuda")
    mot = torch.full((h, w, 2), SENT, dtype=torch.float16, device="cuda")
    svc, svp = dev(np.array(out["sv_curr"]).view(np.float32)), dev(np.array(out["sv_prev"]).view(np.float32))
    mrt = abi.PsmainTargets()
    mrt.albedo_metallic, mrt.albedo_fmt, mrt.motion_vectors, mrt.motion_fmt = alb.data_ptr(), abi.FMT_RGBA16F, mot.data_ptr(), abi.FMT_RG16F
    mrt.svPositionCurr, mrt.svPositionPrev = svc.data_ptr(), svp.data_ptr()
    for label, ptr, pitch in (("NULL", None, 0), ("misaligned", q + 12, 0), ("negative pitch", q, -1), ("pitch below the width", q, w - 1), ("on the output", col.data_ptr(), 0),
                              ("on ip2", ip[2].data_ptr(), 0), ("on the albedo target", alb.data_ptr(), 0), ("on the motion vectors", mot.data_ptr(), 0)):
        refused(lib.vqhip_forward_lighting_from_materials_quad(hnd, st, C.byref(inter), mats, len(mats), None, C.byref(pf), C.byref(pv), None, 0, None, None,
                                                               C.c_void_p(col.data_ptr()), w, abi.FMT_RGBA16F, C.byref(mrt), C.c_void_p(ptr), pitch), f"forward: {label}")
    torch.cuda.synchronize()
    assert all((t == SENT).all() for t in gbt) and (nrm == 7).all() and (col == SENT).all() and (alb == SENT).all() and (mot == SENT).all()
    ref_ip2 = np.array(out["ip2"])
    assert np.array_equal(ip[2].cpu().numpy().view(np.uint32), ref_ip2), "a refused call wrote ip2"
    with pytest.raises(ValueError):
        ctx.gbuffer_from_materials_quad(ip, mats, 0.1, quv[:, :-1])


# ---- the chains -----------------------------------------------------------------------------------------------------------------------------------------------------------------
def masked_draws(ctx, name):
    """the cards case's draws for the masked pre-pass and for the resolve, and the device material table"""
    scene = QC.cases()[name]
    mats = device_materials(ctx, name)
    surf = [device_draw(d) for d in scene["draws"]]
    zdraws = [capi.MaskedDraw(s.vertices, s.indices, s.wvp, s.world, d["cull"], material=mats[k] if d.get("mask") is not None else None)
              for k, (s, d) in enumerate(zip(surf, scene["draws"]))]
    return scene, mats, surf, zdraws


def test_chain_1x_masked_depth_quad_resolve_lit_frame(ctx):
    """cards_minified_64x48_s1: vqhip_scene_masked_depth -> vqhip_scene_quad_interpolants -> vqhip_forward_lighting_from_materials_quad == the oracle on the
    statement's planes; afterwards no pixel owned by a masked primitive has -1 in ip2.w, while the existing producer leaves the count the CPU test printed"""
    name = "cards_minified_64x48_s1"
    scene, mats, surf, zdraws = masked_draws(ctx, name)
    w, h = 64, 48
    z = ctx.scene_masked_depth(zdraws, w, h, 1, primitive=True)
    res = ctx.scene_quad_interpolants(surf, w, h, z["primitive"], sv=False)
    torch.cuda.synchronize()
    assert np.array_equal(z["primitive"].cpu().numpy().view(np.uint32), QC.owners(name)[0][0])
    ref, _ = QC.expected(name)[0]
    assert_planes("planes of the chain", {k: res[k].cpu().numpy().view(np.uint32) for k in PLANES[:3] + ("quad_uv",)}, ref, w, PLANES[:3] + ("quad_uv",))
    pf, extra, pv = lights(w, h)
    pf.fAmbientLightingFactor = AMBIENT
    ip_old = [res[k].clone() for k in PLANES[:3]]
    ip = [res[k] for k in PLANES[:3]]
    got = ctx.forward_lighting_from_materials_quad(ip, mats, pf, pv, res["quad_uv"], extra_point=extra)
    ctx.forward_lighting_from_materials(ip_old, mats, pf, pv, extra_point=extra)
    torch.cuda.synchronize()
    wgb, _ = QC.expected_gbuffer(name, 0, False)
    with np.errstate(all="ignore"):
        assert_bits(got, O.forward_lighting(wgb, pf, pv, abi.FMT_RGBA16F, extra_point=extra), "lit frame of the cards")
    m = QC.masked_owner_mask(name, 0)
    new, old = (t[2][..., 3].contiguous().view(torch.int32).cpu().numpy() for t in (ip, ip_old))
    n_cpu, _ = disagreements(name, 0)
    print(f"{name}: pixels that own their depth and are discarded by the lit draw: existing producer {int((m & (old == -1)).sum())} (CPU statement {n_cpu}), _quad producer {int((m & (new == -1)).sum())}")
    assert int((m & (new == -1)).sum()) == 0
    assert int((m & (old == -1)).sum()) == n_cpu >= 1


def test_chain_4x_layers_gbuffers_lit_resolve(ctx):
    """cards_minified_64x48_s4: four layers -> four vqhip_gbuffer_from_materials_quad -> vqhip_forward_lighting_msaa == the oracle per layer, resolved by tests/msaa_ref.py"""
    name = "cards_minified_64x48_s4"
    scene, mats, surf, zdraws = masked_draws(ctx, name)
    w, h = 64, 48
    z = ctx.scene_masked_depth(zdraws, w, h, 4, layers=4)
    pf, extra, pv = lights(w, h)
    pf.fAmbientLightingFactor = AMBIENT
    layers_dev, bad_new, bad_old = [], 0, 0
    for k in range(4):
        res = ctx.scene_quad_interpolants(surf, w, h, z["layer_primitive"][k], sv=False)
        ip_old = [res[p].clone() for p in PLANES[:3]]
        ip = [res[p] for p in PLANES[:3]]
        layers_dev.append(ctx.gbuffer_from_materials_quad(ip, mats, AMBIENT, res["quad_uv"]))
        ctx.gbuffer_from_materials(ip_old, mats, AMBIENT)
        torch.cuda.synchronize()
        assert np.array_equal(z["layer_primitive"][k].cpu().numpy().view(np.uint32), QC.owners(name)[0][k]), f"layer {k} owner plane"
        want, _ = QC.expected_gbuffer(name, k, False)
        for g in range(4):
            assert_bits(layers_dev[k][g], want[g], f"layer {k} gb{g}")
        m = QC.masked_owner_mask(name, k)
        new, old = (t[2][..., 3].contiguous().view(torch.int32).cpu().numpy() for t in (ip, ip_old))
        bad_new += int((m & (new == -1)).sum())
        bad_old += int((m & (old == -1)).sum())
    got = ctx.forward_lighting_msaa(layers_dev, z["coverage"], pf, pv, out_fmt=abi.FMT_RGBA16F, extra_point=extra)
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        shaded = [O.forward_lighting(QC.expected_gbuffer(name, k, False)[0], pf, pv, abi.FMT_RGBA16F, extra_point=extra) for k in range(4)]
    assert_bits(got, msaa_ref.resolve(shaded, QC.owners(name)[1], None, abi.FMT_RGBA16F), "lit 4x resolve of the cards")
    n_cpu = sum(disagreements(name, k)[0] for k in range(4))
    print(f"{name}: existing producer {bad_old} (CPU statement {n_cpu}), _quad producer {bad_new}")
    assert bad_new == 0 and bad_old == n_cpu >= 1 and n_cpu == sum(disagreements(name, k)[0] for k in INCONSISTENT[name])
