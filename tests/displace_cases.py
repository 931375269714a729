"""What both vqhip_displace_meshes test files use (tests/test_displace_cpu.py, tests/test_gpu_displace.py; docs/DESIGN_DETAILS.md §7.22), in the form
tests/displace_ref.py reads: the stream jobs (height maps 4 x 4, 8 x 8, 5 x 3, 1 x 7, one with a second level that must not be read, the null SRV; grids of
36, 100 and 324 vertices with 44- and 48-byte vertices; uvs on texel centres, at fraction 255/256, outside [0, 1) on both sides, NaN and +-inf; displacements 100,
0, negative and -0) and the chain scene — a hill in front of an alpha-tested card — in the forms the existing references of §7.16 .. §7.21 read.
Expectations are computed once per process and shared read-only."""
import functools

import numpy as np

from tests import displace_ref as D
from tests import masked_depth_cases as MC
from tests import masked_depth_ref as M
from tests import object_ids_cases as PC
from tests import object_ids_ref as P
from tests import outline_cases as OC
from tests import outline_ref as OR
from tests import quad_interp_ref as Q
from tests import scene_depth_ref as V
from tests import scene_interp_cases as IC
from tests import scene_interp_ref as I
from tests import shadow_raster_cases as K
from tests import shadow_raster_ref as R
from vqengine_amd import shadow_scene as S
from vqengine_amd import surface_scene as SS

F = np.float32
IDENTITY = (1.0, 1.0, 0.0, 0.0)
CENTRES_4 = (1.0, 1.0, 0.125, 0.125)                    # uv 0 -> 0.125: 0.125 * 4 - 0.5 = 0, a texel centre of a 4-texel axis (weights 0)
FRACTION_255 = (1.0, 1.0, 383.0 / 1024.0, 383.0 / 1024.0)    # uv 0 -> 383/1024: * 4 - 0.5 = 255/256 exactly
WRAP_BOTH = (-1.5, 2.25, -0.3, 0.4)                     # u from -1.8 to -0.3, v from 0.4 to 2.65


@functools.lru_cache(maxsize=None)
def heightmaps():
    def tex(w, h, kind, seed, mips=None):
        chain, n = SS.heightmap_chain(w, h, kind, seed, mips)
        return {"chain": chain, "w": w, "h": h, "mips": n}
    t = {"h4": tex(4, 4, "steps", 1, 1), "h8": tex(8, 8, "noise", 2), "h5x3": tex(5, 3, "noise", 3), "h1x7": tex(1, 7, "steps", 4), "hill8": tex(8, 8, "hill", 5),
         "zero4": tex(4, 4, "zero", 6, 1), "null": {"chain": None, "w": 0, "h": 0, "mips": 0}}
    # two levels, the second one nothing like the first (the box filter's would be its mean): red 255 - the mean, so that a fetch that strays to level 1 shows
    lv0 = SS.heightmap_chain(8, 8, "noise", 7, 1)[0]
    lv1 = 255 - SS.heightmap_chain(8, 8, "noise", 7, 2)[0][64:]
    t["h8_two_levels"] = {"chain": np.ascontiguousarray(np.concatenate([lv0, lv1], axis=0)), "w": 8, "h": 8, "mips": 2}
    for v in t.values():
        if v["chain"] is not None:
            v["chain"].setflags(write=False)
    return t


def grid(n, stride=44, size=2.0):
    """surface_scene.grid in the engine's vertex, or with one float of padding (48 bytes) that must travel untouched"""
    v, idx = SS.grid(n, size)
    if stride == 48:
        v = np.ascontiguousarray(np.concatenate([v, np.full((v.shape[0], 1), 777.0, dtype=F)], axis=1))
    return v, idx


def job(mesh, tex, so=IDENTITY, displacement=1.0):
    t = heightmaps()[tex]
    return dict(SS.with_heightmap(mesh, t["chain"], t["w"], t["h"], t["mips"], so, displacement), heightmap=t, name=tex)


def _special_uv(mesh):
    """NaN, +inf and -inf in the uv of the first vertices of a copy of the mesh, in every pairing with a finite coordinate"""
    v, idx = mesh[0].copy(), mesh[1]
    nan, inf = F(np.nan), F(np.inf)
    for k, (a, b) in enumerate(((nan, nan), (nan, 0.3), (0.3, nan), (inf, 0.6), (0.6, -inf), (-inf, inf), (3.0e38, -3.0e38))):
        v[k, 9], v[k, 10] = a, b
    return v, idx


def _negative_zero_y(mesh):
    """every y of the mesh -0.0: with a zero sample and displacement -0.0 the reference's y + h is -0 (H4)"""
    v, idx = mesh[0].copy(), mesh[1]
    v[:, 1] = F(-0.0)
    return v, idx


@functools.lru_cache(maxsize=None)
def stream_jobs():
    """name -> job, in the order the GPU test submits them in ONE call (per output stride)"""
    g9 = grid(9)
    j = {
        "centres_4x4_grid5": job(grid(5), "h4", CENTRES_4, 100.0),
        "fraction255_4x4_grid5_s48": job(grid(5, 48), "h4", FRACTION_255, 100.0),
        "wrap_8x8_grid9": job(g9, "h8", WRAP_BOTH, -2.5),
        "wrap_5x3_grid9_s48": job(grid(9, 48), "h5x3", WRAP_BOTH, 100.0),
        "one_texel_axis_1x7_grid5": job(grid(5), "h1x7", (3.0, -2.0, -1.0, 1.25), 0.75),
        "level0_only_grid9": job(g9, "h8_two_levels", (0.9, 1.1, 0.05, -0.02), 100.0),
        "null_srv_grid5": job(grid(5), "null", WRAP_BOTH, 100.0),
        "zero_displacement_grid9_s48": job(grid(9, 48), "h8", IDENTITY, 0.0),
        "special_uv_8x8_grid5": job(_special_uv(grid(5)), "h8", (1.0, 1.0, 0.1, 0.1), 3.0),
        "special_uv_5x3_grid5": job(_special_uv(grid(5)), "h5x3", (0.0, 2.0, 0.5, 0.0), -1.0),
        "negative_zero_grid5": job(_negative_zero_y(grid(5)), "zero4", IDENTITY, -0.0),
        "two_blocks_grid17": job(grid(17), "hill8", IDENTITY, 100.0),
        # wave boundaries and the empty job, sharing the call with two different height maps
        "batch_1": job((g9[0][:1], g9[1][:0]), "h8", WRAP_BOTH, 100.0),
        "batch_64": job((g9[0][:64], g9[1][:0]), "h5x3", WRAP_BOTH, 100.0),
        "batch_65": job((g9[0][:65], g9[1][:0]), "h8", IDENTITY, -2.5),
        "batch_0": job((g9[0][:0], g9[1][:0]), "h5x3", IDENTITY, 100.0),
    }
    for v in j.values():
        v["vertices"].setflags(write=False)
    return j


@functools.lru_cache(maxsize=None)
def stream_expected(name, compact):
    out = D.displace(stream_jobs()[name], compact)
    out.setflags(write=False)
    return out


def footprint(jb):
    """(u, v, wx, wy) of a job's vertices on level 0 of its height map: what the landing-place assertions read"""
    u, v = D.transformed_uv(jb["vertices"], jb["scale_offset"])
    _, _, _, _, wx, wy = D.level_taps(jb["heightmap"], 0, u, v)
    return u, v, wx, wy


# ---- the chain scene: a hill (the displaced grid) in front of an alpha-tested card ----------------------------------------------------------------------------------
EYE, AT, EYE_PREV = (0.3, 2.2, -4.2), (0.0, 0.5, 0.4), (0.25, 2.25, -4.3)
HILL_DISPLACEMENT = 1.6


def hill_job(stride=44):
    return job(grid(9, stride, 4.0), "hill8", (1.0, 1.0, 0.0, 0.0), HILL_DISPLACEMENT)


def _views(w, h):
    fov, near, far = np.radians(60.0), 0.1, 30.0
    return S.camera_view_proj(EYE, AT, fov, w / h, near, far), S.camera_view_proj(EYE_PREV, AT, fov, w / h, near, far)


@functools.lru_cache(maxsize=None)
def hill_scene(w, h, samples, displaced=True):
    """two draws in every form the references read (scene_depth_ref, masked_depth_ref, scene_interp_ref / quad_interp_ref): draw 0 the grid of hill_job() — its
    positions the displaced stream of tests/displace_ref.py, or the flat mesh —, material 0; draw 1 an upright checker card behind the hill, masked, material 1"""
    vp, pvp = _views(w, h)
    jb = hill_job()
    verts = D.displace(jb) if displaced else jb["vertices"]
    hill = dict(IC.draw(verts, jb["indices"], SS.instance_matrices_full([S.translation((0.0, 0.0, 0.0))], vp, pvp), 0, V.CULL_NONE, 32, 44), mask=None)
    cv, ci = SS.card(1.8, 0.9)
    card = dict(IC.draw(cv, ci, SS.instance_matrices_full([S.translation((0.0, 0.9, 2.4))], vp, pvp), 1, V.CULL_NONE, 32, 44), mask=MC.mask("t8"))
    return IC.scene(w, h, samples, [hill, card])


def opaque(scene):
    return MC.opaque(scene)


@functools.lru_cache(maxsize=None)
def depth_expected(w, h, samples, layers, displaced=True):
    """vqhip_scene_depth of the hill scene, every draw opaque (tests/scene_depth_ref.py)"""
    out = V.rasterize(opaque(hill_scene(w, h, samples, displaced)), layers=layers)
    for a in out.values():
        for b in (a if isinstance(a, list) else [a]):
            b.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def masked_expected(w, h, displaced=True):
    """vqhip_scene_masked_depth at one sample (tests/masked_depth_ref.py)"""
    out = M.rasterize_scene(hill_scene(w, h, 1, displaced))
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def interp_expected(w, h):
    """vqhip_scene_interpolants and vqhip_scene_quad_interpolants over the masked call's owner plane (tests/scene_interp_ref.py, tests/quad_interp_ref.py)"""
    sc, owner = hill_scene(w, h, 1), masked_expected(w, h)["primitive"]
    return I.interpolate(sc, owner), Q.interpolate(sc, owner)


@functools.lru_cache(maxsize=None)
def ids_expected(w, h):
    """(id draws, ids) of vqhip_object_ids over the opaque depth call's owner plane: every draw of the scene already has cull NONE"""
    draws = PC.id_draws(hill_scene(w, h, 1)["draws"])
    return draws, P.resolve(draws, depth_expected(w, h, 1, None)["primitive"])


def shadow_views(dim, displaced=True):
    """one z / w view (a spot light above the hill) and one LINEAR_DEPTH view (the -Y face of a point light), both over the 12-byte stream"""
    jb = hill_job()
    pos = np.ascontiguousarray((D.displace(jb) if displaced else jb["vertices"])[:, :3])
    cv, ci = SS.card(1.8, 0.9)
    worlds = ([S.translation((0.0, 0.0, 0.0))], [S.translation((0.0, 0.9, 2.4))])
    out = []
    for linear, lp, vp, far in ((False, (0.4, 4.5, -2.5), S.spot_view_proj((0.4, 4.5, -2.5), (-0.1, -0.85, 0.5), 0.1, 20.0), 1.0),
                                (True, (0.3, 3.6, 0.2), S.point_face_view_proj((0.3, 3.6, 0.2), 3, 0.05, 9.0), 9.0)):
        draws = []
        for (p, i), wl in zip(((pos, jb["indices"]), (np.ascontiguousarray(cv[:, :3]), ci)), worlds):
            wvp, world = S.instance_matrices(wl, vp)
            draws.append(K.draw(p, i, wvp, world, V.CULL_NONE, 32, 12))
        out.append(K.view(dim, draws, linear, lp, far))
    return out


@functools.lru_cache(maxsize=None)
def shadow_expected(dim, displaced=True):
    maps = R.rasterize(shadow_views(dim, displaced))
    for a in maps:
        a.setflags(write=False)
    return maps


def outline_scene(w, h, displaced=True):
    """the displaced grid selected (tests/outline_ref.py)"""
    jb = hill_job()
    view, proj = OC.camera(w, h, EYE, AT)
    return OC.scene(w, h, [OC.draw(D.displace(jb) if displaced else jb["vertices"], jb["indices"], S.translation((0.0, 0.0, 0.0)), view, proj)])


@functools.lru_cache(maxsize=None)
def outline_expected(w, h, displaced=True):
    out = OR.outline(outline_scene(w, h, displaced), OC.prefill(w, h))
    for a in out.values():
        a.setflags(write=False)
    return out


def changed_fraction(a, b):
    """of the pixels either depth plane covers (depth below 1), the fraction whose depth bits differ"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    covered = (a < 1) | (b < 1)
    return float((a.view(np.uint32) != b.view(np.uint32))[covered].mean()) if covered.any() else 0.0
