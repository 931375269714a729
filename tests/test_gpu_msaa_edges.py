"""-m gpu: NON-EMPTY edge lists through every instantiation of k_msaa_edges (vqengine_amd/csrc/msaa.hip, docs/DESIGN_DETAILS.md §7.9): IBL x casters x
format x reading, its grid-stride loop (option msaa_edge_wgs), k_msaa_shade in its three workgroup shapes (option shade_wg), and the neighbour
independence of shade_pixel stated directly. Every image is compared bit for bit with the contract: each layer shaded by the oracle
(tests/oracle_lib.forward_lighting), resolved by tests/msaa_ref.py. The frames, helpers and the other MSAA tests are tests/test_gpu_msaa.py's."""
import contextlib

import numpy as np
import pytest
import torch

from tests import msaa_ref
from tests import ref_cases
from tests.test_arith_modes import dxc_mode
from tests.test_gpu_msaa import F16, F32, _bg, _expected, _lights, assert_bits
from vqengine_amd import abi, synth

pytestmark = pytest.mark.gpu
dev = ref_cases._dev

_MEMO = {}


def _memo(key, fn):
    """inputs and oracle results shared by the tests of this module (never modified by a test)"""
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def _small_env():
    return _memo("small_env", ref_cases.small_env)


def _shadow_maps(dims):
    """the maps of ref_cases.shadow_scene at other sizes: its seed, its draw order, occluders in one half of the 2D maps, random cube depths"""
    dd, ds, dp = dims
    rng = np.random.default_rng(11)
    dmap = rng.random((dd, dd), dtype=np.float32) * 0.2 + 0.4
    dmap[:, dd // 2:] = 1.0
    smap = rng.random((5, ds, ds), dtype=np.float32) * 0.3 + 0.35
    smap[:, ds // 2:, :] = 1.0
    pmap = rng.random((5, 6, dp, dp), dtype=np.float32) * 0.5 + 0.05
    return {"dir": dmap, "spot": smap, "point": pmap, "dims": (dd, ds, dp)}


def _shadow_scene(dims=(64, 32, 16)):
    """ref_cases.shadow_scene()'s lights and views with maps of `dims` = (directional, spot, point) texels per side -> (per-frame data, maps with their "dims"
    for ref_cases.host_shadow_dims / dev_shadow_dims). _shadow_maps restates shadow_scene's construction: at shadow_scene's own sizes it must give
    shadow_scene's maps bit for bit, which is asserted on every call, so the two cannot drift apart unnoticed."""
    pf, s = ref_cases.shadow_scene()
    same = _shadow_maps((64, 32, 16))
    assert all(np.array_equal(same[k], s[k]) for k in s), "tests/ref_cases.shadow_scene changed: _shadow_maps no longer restates it"
    pf.f2DirectionalLightShadowMapDimensions = abi.float2(float(dims[0]), float(dims[0]))
    pf.f2SpotLightShadowMapDimensions = abi.float2(float(dims[1]), float(dims[1]))
    pf.f2PointLightShadowMapDimensions = abi.float2(float(dims[2]), float(dims[2]))
    return pf, _shadow_maps(dims)


# ---------------------------------------------------------------------------------------------------------------------
# Frame A: 96 x 24, four layers, 692 of its 2 304 pixels split
# (639 between two layers, 53 between three): eleven waves of edge pixels. The oracle shades its four layers with IBL and casters
# in about 15 ms, so every expectation below is computed in full and shared (_memo).
# ---------------------------------------------------------------------------------------------------------------------
AW, AH, ASEED = 96, 24, 0x51
NPOT_DIMS = (48, 24, 12)                       # no power of two: pcf_2d wraps by division, omni_pcf indexes a 12-texel face
KINDS = ["env", "casters", "env+casters", "casters_npot"]


def _split(cov):
    own = msaa_ref.owners(cov)
    return (own != own[..., :1]).any(-1)


def _edge_records(cov, k, n):
    """the first n pixels (row-major) where layer k owns a sample and a lower layer owns one too: k's record there is shaded by k_msaa_edges, never by k_msaa_shade"""
    own = msaa_ref.owners(cov)
    lower = np.zeros(cov[0].shape, bool)
    for j in range(k):
        lower |= (own == j).any(-1)
    ys, xs = np.nonzero((own == k).any(-1) & lower)
    assert len(ys) >= n, (k, len(ys))
    return [(int(y), int(x)) for y, x in zip(ys[:n], xs[:n])]


def _frame_a():
    """(layers, coverage, position of the planted light). Planted in records that only k_msaa_edges shades:
      * roughness 0 / 0.01 / 0.039 in each of the layers 1..3: below 0.04 the wave takes the EPSILON-select form of the point-light loop (vq_shade.h `eps`);
      * roughness 2.0 in one more record of the layers 1 and 3: px.fastOK is false (setup_pixel: roughness <= 1), the lane stays out of the fast loop, its vmin stays 0
        and `!(vmin >= 2^-80)` sends it through the IEEE redo of the loop while its neighbours keep the fast result;
      * one record of layer 2 with a point light exactly above it on the y axis, as tests/test_gpu_arith_modes.py plants it: two zero components of Lw - P. (With
        vmin = min(dd, hh) and dd = 9 this plant need not reach the redo in the present vq_shade.h; the roughness 2.0 records are the ones that do.)"""
    def make():
        gbs, cov = synth.gbuffer_msaa(AW, AH, 4, 0.3, seed=ASEED)
        for k in (1, 2, 3):
            for (y, x), r in zip(_edge_records(cov, k, 3), (0.0, 0.01, 0.039)):
                gbs[k][1][y, x, 3] = np.float32(r)
        for k in (1, 3):
            y, x = _edge_records(cov, k, 4)[3]
            gbs[k][1][y, x, 3] = np.float32(2.0)
        y, x = _edge_records(cov, 2, 4)[3]
        P = gbs[2][0][y, x]
        return gbs, cov, (float(P[0]), float(P[1]) + 3.0, float(P[2]))
    return _memo("frame A", make)


def _scene(kind, w, h, seed=ASEED, above=None, points=None):
    """lights of one kind: plain | env | casters | env+casters | casters_npot -> dict(pf, extra, pv, env, shadow); env / shadow are the HOST inputs
    (ref_cases.small_env / the maps of _shadow_scene) or None. above: position given to point light 0; points: replaces the point lights"""
    env = _small_env() if "env" in kind else None
    shadow = extra = None
    if "casters" in kind:
        pf, shadow = _shadow_scene(NPOT_DIMS) if kind.endswith("npot") else _shadow_scene()
        assert all(d & (d - 1) for d in shadow["dims"]) == kind.endswith("npot")
    else:
        pf, extra, _ = _lights(w, h, seed)
    if points is not None:
        assert len(points) <= abi.NUM_LIGHTS__POINT
        pf.Lights.numPointLights = len(points)
        for i in range(len(points)):
            pf.Lights.point_lights[i] = points[i]
        extra = None
    if above is not None:
        pf.Lights.point_lights[0].position.set(above)
    return {"pf": pf, "extra": extra, "pv": synth.per_view(w, h, max_env_lod=env["spec_mips"] if env else 0), "env": env, "shadow": shadow}


def _reading(dxc, ctx=None):
    return dxc_mode(ctx) if dxc else contextlib.nullcontext()


def _oracle(gbs, cov, sc, fmt, bg, dxc=False, env=True, shadow=True, pf=None):
    """the contract's image; env=False drops the IBL, shadow=False replaces every shadow map by an unoccluded one (depth 1.0)"""
    sh = sc["shadow"]
    if sh is not None and not shadow:
        sh = {k: v if k == "dims" else np.ones_like(v) for k, v in sh.items()}
    with _reading(dxc):
        return _expected(gbs, cov, pf if pf is not None else sc["pf"], sc["pv"], fmt, sc["extra"], bg, env=ref_cases.host_env(sc["env"]) if env else None,
                         shadow=ref_cases.host_shadow_dims(sh) if sh is not None else None)


def _product(ctx, gbs, cov, sc, fmt, bg, dxc=False):
    keep = []
    with _reading(dxc, ctx):
        got = ctx.forward_lighting_msaa([[dev(p) for p in g] for g in gbs], [dev(c) for c in cov], sc["pf"], sc["pv"], background=dev(bg) if bg is not None else None,
                                        out_fmt=fmt, extra_point=sc["extra"], env=ref_cases.dev_env(sc["env"], keep), shadow=ref_cases.dev_shadow_dims(sc["shadow"], keep) if sc["shadow"] is not None else None)
        return got.cpu().numpy()


def _changed(a, b, where):
    """share of the pixels `where` at which two images differ in any bit"""
    u = np.uint16 if a.dtype == np.float16 else np.uint32
    return float((a.view(u) != b.view(u)).any(-1)[where].mean())


def _case_a(kind, fmt, dxc):
    """(layers, coverage, scene, background, expected image) of frame A under one kind of lighting: shared by the variant, grid-stride and permutation tests"""
    def make():
        gbs, cov, above = _frame_a()
        sc = _scene(kind, AW, AH, above=above)
        bg = _bg(AW, AH, fmt, ASEED + 1)
        return gbs, cov, sc, bg, _oracle(gbs, cov, sc, fmt, bg, dxc)
    return _memo(("case A", kind, fmt, dxc), make)


def test_frame_a_is_the_frame_the_edge_tests_count_on():
    """the figures the tests below rely on, from the coverage alone: 692 split pixels = eleven waves, three passes of one 256-lane workgroup, the last one partial"""
    _, cov, _ = _frame_a()
    owners_n = np.array([[len(set(px.tolist())) for px in row] for row in msaa_ref.owners(cov)])
    assert (int(_split(cov).sum()), int((owners_n == 2).sum()), int((owners_n == 3).sum())) == (692, 639, 53)
    assert 2 * 256 < 692 < 3 * 256


@pytest.mark.parametrize("dxc", [False, True])
@pytest.mark.parametrize("fmt", [F16, F32])
@pytest.mark.parametrize("kind", KINDS)
def test_edge_kernel_every_variant(ctx, kind, fmt, dxc):
    """k_msaa_edges<HAS_ENV, HAS_CASTERS, fmt, AR> on frame A for every pair that has IBL or casters; (false, false, *, 1) are test_skip_form_in_the_edge_kernel's DXC cases.
    Not vacuous, from the oracle alone: unoccluded shadow maps change >= 25 % of the split pixels, dropping the IBL changes >= 90 % of them."""
    gbs, cov, sc, bg, want = _case_a(kind, fmt, dxc)
    split = _split(cov)
    if sc["shadow"] is not None:
        share = _changed(want, _oracle(gbs, cov, sc, fmt, bg, dxc, shadow=False), split)
        assert share >= 0.25, f"shadow maps decide only {share:.2f} of the split pixels"
    if sc["env"] is not None:
        share = _changed(want, _oracle(gbs, cov, sc, fmt, bg, dxc, env=False), split)
        assert share >= 0.90, f"IBL decides only {share:.2f} of the split pixels"
    assert_bits(_product(ctx, gbs, cov, sc, fmt, bg, dxc), want, f"frame A, {kind}, fmt {fmt}, DXC reading {dxc}")


@pytest.mark.parametrize("fmt", [F16, F32])
def test_four_owners_and_three_owners_with_background(ctx, fmt):
    """arbitrary coverage bytes: the `while (todo)` loop of k_msaa_edges runs three times in some lanes and once in their neighbours, under IBL + casters"""
    w, h = 64, 8
    gbs, cov = synth.gbuffer_msaa(w, h, 4, 0.0, seed=0xB4, mode="random")
    own = msaa_ref.owners(cov)
    layers_owning = sum((own == k).any(-1).astype(int) for k in range(4))
    assert (layers_owning == 4).any(), "no pixel with four owning layers"
    assert ((layers_owning == 3) & (own == -1).any(-1)).any(), "no pixel with three owning layers and background"
    for k in range(4):
        for p in gbs[k]:
            p[~(own == k).any(-1)] = np.nan                       # a layer that owns nothing there may hold anything
    sc = _scene("env+casters", w, h)
    bg = _bg(w, h, fmt, 0xB5)
    assert_bits(_product(ctx, gbs, cov, sc, fmt, bg), _oracle(gbs, cov, sc, fmt, bg), f"random coverage, env+casters, fmt {fmt}")


@pytest.mark.parametrize("wgs", [1, 2, 1000])
def test_edge_list_longer_and_shorter_than_the_grid(ctx, set_opt, wgs):
    """the grid-stride step of k_msaa_edges: 692 edge pixels through 256 lanes (three passes, the last one partial), 512 lanes (two), and 1000 workgroups asked for: clamped
    at launch to one lane per pixel (nine workgroups, 2 304 lanes), still more lanes than edge pixels, most of them idle"""
    gbs, cov, sc, bg, want = _case_a("env+casters", F16, False)
    set_opt("msaa_edge_wgs", wgs)
    assert_bits(_product(ctx, gbs, cov, sc, F16, bg), want, f"frame A with {wgs} workgroups of k_msaa_edges")


def test_msaa_edge_wgs_option(ctx, set_opt):
    """The option's argument checks and its round trip (value, then None / "default" / "0" / ""). Every grid size gives the same image and the library has no getter, so
    the images compared after those calls show only that the calls were accepted or refused without disturbing the next frame, not which grid was then launched."""
    gbs, cov, sc, bg, want = _case_a("env+casters", F16, False)
    set_opt("msaa_edge_wgs", 1)
    # an empty edge list under one workgroup: full coverage is vqhip_forward_lighting itself
    keep = []
    planes = [dev(p) for p in gbs[0]]
    full = torch.full((AH, AW), 0xF, dtype=torch.uint8, device="cuda")
    env, sh = ref_cases.dev_env(sc["env"], keep), ref_cases.dev_shadow_dims(sc["shadow"], keep)
    fl = ctx.forward_lighting(planes, sc["pf"], sc["pv"], out_fmt=F16, env=env, shadow=sh)
    ms = ctx.forward_lighting_msaa([planes], [full], sc["pf"], sc["pv"], out_fmt=F16, env=env, shadow=sh)
    assert np.array_equal(ms.cpu().numpy().view(np.uint16), fl.cpu().numpy().view(np.uint16))
    for junk in (b"-1", b"x", b"1.5", b"3 "):
        assert ctx.lib.vqhip_set_option(ctx._h, b"msaa_edge_wgs", junk) == abi.VQHIP_ERR_INVALID_ARG
    assert_bits(_product(ctx, gbs, cov, sc, F16, bg), want, "frame A after four refused values of msaa_edge_wgs")
    for restore in (None, "default", "0", ""):                     # each of them accepted: the spellings of "the default"
        ctx.set_option("msaa_edge_wgs", 3)
        ctx.set_option("msaa_edge_wgs", restore)
    assert_bits(_product(ctx, gbs, cov, sc, F16, bg), want, "frame A after msaa_edge_wgs was set and reset")


@pytest.mark.parametrize("wg", [64, 128, 256])
def test_shade_kernel_workgroup_shapes(ctx, set_opt, wg):
    """k_msaa_shade in each workgroup shape (256 lanes is the default from 4 Mi pixels on): 333 is no multiple of any, so the last workgroup of a row hangs over
    the frame while its in-frame lanes append to the edge list, and with 128 / 256 lanes several waves of one workgroup take their slots"""
    w, h = 333, 37

    def make():
        gbs, cov = synth.gbuffer_msaa(w, h, 3, 0.3, seed=0xD4)
        sc = _scene("plain", w, h, seed=0xD4)
        bg = _bg(w, h, F16, 0xD5)
        assert _split(cov)[:, 320:].any(), "no edge pixel in the row's last, partial workgroup"
        return gbs, cov, sc, bg, _oracle(gbs, cov, sc, F16, bg)
    gbs, cov, sc, bg, want = _memo("333 x 37", make)
    set_opt("shade_wg", wg)
    assert_bits(_product(ctx, gbs, cov, sc, F16, bg), want, f"333 x 37, k_msaa_shade with {wg} lanes per workgroup")


@pytest.mark.parametrize("dxc", [False, True])
def test_permuted_pixels_give_the_permuted_image(ctx, dxc):
    """shade_pixel reads its record and the frame constants only, so moving the pixels of frame A about (every plane of every layer, the coverage, the
    background) moves the output with them, bit for bit — whatever waves k_msaa_shade (row coherence gone) and k_msaa_edges (another list) then form"""
    gbs, cov, sc, bg, want = _case_a("env+casters", F16, dxc)
    perm = np.random.default_rng(0xE5).permutation(AW * AH)

    def moved(a):
        return np.ascontiguousarray(a.reshape((AW * AH,) + a.shape[2:])[perm].reshape(a.shape))
    got = _product(ctx, gbs, cov, sc, F16, bg, dxc)
    got_moved = _product(ctx, [[moved(p) for p in g] for g in gbs], [moved(c) for c in cov], sc, F16, moved(bg), dxc)
    assert_bits(got, want, f"frame A, DXC reading {dxc}")
    assert np.array_equal(got_moved.view(np.uint16), moved(got).view(np.uint16)), f"a pixel's result depends on its neighbours (DXC reading {dxc})"


def _surface_frame():
    """frame A with every layer's normals replaced by a smooth unit field within 19.5 degrees of +y, and twelve point lights: six 60..80 above y = 0, six 60..80 below"""
    def make():
        gbs, cov, _ = _frame_a()
        gbs = [[p.copy() for p in g] for g in gbs]
        ys, xs = np.mgrid[0:AH, 0:AW].astype(np.float64)
        for k, g in enumerate(gbs):
            n = np.stack([0.25 * np.sin(0.37 * xs + 1.3 * k), np.ones_like(xs), 0.25 * np.cos(0.29 * ys - 0.7 * k)], -1)
            g[1][..., :3] = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
        pts = synth.point_lights(12, seed=0xF6)
        for i in range(12):
            x, y, z = pts[i].position.x, pts[i].position.y, pts[i].position.z
            pts[i].position.set((0.5 * x, (60.0 + y) * (1.0 if i % 2 == 0 else -1.0), 0.5 * z))
            pts[i].range = 400.0
        return gbs, cov, pts
    return _memo("surface frame", make)


@pytest.mark.parametrize("kind,fmt,dxc", [("plain", F16, False), ("casters", F16, False), ("plain", F16, True), ("plain", F32, True)])
def test_skip_form_in_the_edge_kernel(ctx, kind, fmt, dxc):
    """The `skip` form of the point-light loop from the waves of k_msaa_edges, whichever lanes they hold. Relied on (vqengine_amd/csrc/vq_shade.h):
      :500      fast = px.fastOK & fc->pointFastOK — records and lights of ordinary magnitude, roughness in [0, 1] (setup_pixel :84-99, capi.hip :362-364);
      :105-106  px.skipOK = |F0| + |kA| below 2^40 — albedo and metalness in [0, 1];
      :512      laneSkipOK = px.skipOK & dot(N, N of the first active lane) > 0.5 — every normal of every layer is a unit vector within 20 degrees of +y, so ANY two
                of them are within 40 degrees (dot >= 0.76): the condition holds for any subset of lanes and whichever layer each lane picked;
      :513      skip = fc->pointSkipOK (finite colour * brightness, capi.hip :368) & !p5ExpLog & no lane without laneSkipOK — so the default reading takes the
                skip forms (with A's planted roughness < 0.04: the eps + skip form too) and the DXC reading of dxc_mode (exp2/log2 Fresnel) must not;
      :245      in the skip form a light is dropped for the wave when no lane has dot(N, Wi) > 0 (and no accumulator holds a zero): the six lights below the
                surface face away from EVERY record, the six above face every record — asserted here in float64 with a wide margin.
    The two DXC cases are also the only non-empty edge lists of k_msaa_edges<false, false, *, 1>.
    From the oracle alone: the lights below add nothing (the image without them is the same, bit for bit); the lights above decide >= 90 % of the split pixels."""
    gbs, cov, pts = _surface_frame()
    N = np.stack([g[1][..., :3] for g in gbs]).astype(np.float64)
    P = np.stack([g[0][..., :3] for g in gbs]).astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(N, axis=-1) - 1.0) < 1e-6) and np.all(N[..., 1] >= np.cos(np.deg2rad(20.0)))
    for i in range(12):
        d = np.array([pts[i].position.x, pts[i].position.y, pts[i].position.z]) - P
        cosine = (N * d).sum(-1) / np.linalg.norm(d, axis=-1)
        assert np.all(cosine > 0.05) if i % 2 == 0 else np.all(cosine < -0.05), (i, float(cosine.min()), float(cosine.max()))
        assert np.all(np.linalg.norm(d, axis=-1) < 0.75 * pts[i].range)
    sc = _scene(kind, AW, AH, points=pts)
    bg = _bg(AW, AH, fmt, ASEED + 1)
    want = _oracle(gbs, cov, sc, fmt, bg, dxc)
    split = _split(cov)
    only_front = _scene(kind, AW, AH, points=(abi.PointLight * 6)(*[pts[i] for i in range(0, 12, 2)]))       # the six lights above the surface alone
    only_behind = _scene(kind, AW, AH, points=(abi.PointLight * 6)(*[pts[i] for i in range(1, 12, 2)]))     # the six lights below it alone
    assert _changed(want, _oracle(gbs, cov, sc, fmt, bg, dxc, pf=only_front["pf"]), np.ones_like(split)) == 0.0, "a light behind every surface adds light"
    share = _changed(want, _oracle(gbs, cov, sc, fmt, bg, dxc, pf=only_behind["pf"]), split)
    assert share >= 0.90, f"the lights in front decide only {share:.2f} of the split pixels"
    assert_bits(_product(ctx, gbs, cov, sc, fmt, bg, dxc), want, f"surface frame, {kind}, fmt {fmt}, DXC reading {dxc}")
