"""The case sets both test files of §7.20 use (tests/test_quad_interp_cpu.py, tests/test_gpu_quad_interp.py): tests/scene_interp_cases.py's scenes (§7.18's room
with occluders, the 64 instanced boxes, the sphere and the grazing grid at 16 x 16, 64 x 40 and 129 x 67, 1 and 4 samples) and the masked cards of
tests/masked_depth_cases.py (§7.19's 4- and 3-texel patterns and the T O O T stripes) completed to lit draws. Owner planes are the statements'
(tests/scene_depth_ref.py, tests/masked_depth_ref.py). Expectations are computed once per process and shared read-only."""
import functools

import numpy as np

from tests import masked_depth_cases as MC
from tests import oracle_lib as O
from tests import quad_interp_ref as Q
from tests import scene_interp_cases as IC
from vqengine_amd import abi, synth

F = np.float32
PLANES = IC.PLANES + ("quad_uv",)
CARD_NAMES = ("magnified_64x48_s1", "magnified_t12_64x48_s1", "minified_64x48_s1", "magnified_33x17_s1", "magnified_33x17_s4", "minified_64x48_s4")
# the producers run on these (every builder, every size, both sample counts somewhere) and on the cards
PRODUCER_NAMES = ("room_16x16_s1", "boxes_16x16_s4", "sphere_64x40_s1", "room_64x40_s4", "grid_64x40_s1", "boxes_64x40_s1", "room_129x67_s1", "boxes_129x67_s4",
                  "sphere_129x67_s1", "grid_129x67_s4")


def lit_scene(mc_scene):
    """a masked_depth_cases scene as scene_interp_ref reads it: identity normal matrices, a camera that has not moved, material = the draw's number"""
    draws = []
    for k, d in enumerate(mc_scene["draws"]):
        n = d["wvp"].shape[0]
        draws.append(dict(d, normal=np.ascontiguousarray(np.tile(np.eye(4, dtype=F), (n, 1, 1))), wvp_prev=d["wvp"], material=k))
    return dict(mc_scene, draws=draws)


@functools.lru_cache(maxsize=None)
def cases():
    c = dict(IC.cases())
    c.update({f"cards_{n}": lit_scene(MC.cases()[n]) for n in CARD_NAMES})
    return c


def is_cards(name):
    return name.startswith("cards_")


@functools.lru_cache(maxsize=None)
def owners(name):
    """the owner planes of a case (one at 1 sample, four at 4) and the 4x coverage masks or None"""
    if not is_cards(name):
        return IC.owners(name)
    e = MC.expected(name[len("cards_"):])
    if cases()[name]["samples"] == 1:
        return [np.ascontiguousarray(e["primitive"], dtype=np.uint32)], None
    return [np.ascontiguousarray(e["layer_primitive"][k], dtype=np.uint32) for k in range(4)], [np.ascontiguousarray(c) for c in e["coverage"]]


@functools.lru_cache(maxsize=None)
def expected(name):
    """per owner plane: (the statement's six planes as uint32 bits, the statistics of the call: scene_interp_ref's and quad_interp_ref.classify's)"""
    res = []
    for owner in owners(name)[0]:
        st = {}
        out = Q.interpolate(cases()[name], owner, stats=st)
        for a in out.values():
            a.setflags(write=False)
        res.append((out, st))
    return res


def ip_planes(out):
    """the three vqhip_interpolants planes of a statement's dict as fresh float32 arrays (the producers write ip2.w)"""
    return [np.array(out[k]).view(F) for k in PLANES[:3]]


# ---- materials ---------------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene_material_inputs():
    """four materials for the scenes' indices 0 .. 3: every map bound on the first three, mip-chained 32-texel textures at most; the last plain"""
    datas, texsets = synth.material_set(4, seed=0x720, max_dim=32)
    texsets[3] = {}
    datas[3].textureConfig = 0.0
    return datas, [{slot: (O.mip_chain_rgba8(img) + (img.shape[1], img.shape[0])) for slot, img in ts.items()} for ts in texsets]


@functools.lru_cache(maxsize=None)
def card_material_inputs(name):
    """one material per draw of a cards case: the mask's texture as the diffuse map of an alpha-masked material, or a plain opaque material"""
    datas, chains, masked = [], [], []
    for d in cases()[name]["draws"]:
        m = d.get("mask")
        md = abi.MaterialData()
        md.diffuse.set((0.7, 0.6, 0.5))
        md.alpha, md.roughness, md.metalness = 1.0, 0.6, 0.1
        md.uvScaleOffset = abi.float4(*(m["scale_offset"] if m else (1.0, 1.0, 0.0, 0.0)))
        md.textureConfig = m["texture_config"] if m else 0.0
        datas.append(md)
        t = m["tex"] if m else None
        chains.append({"texDiffuse": (t["chain"], t["mips"], t["w"], t["h"])} if t is not None and t["chain"] is not None else {})
        masked.append(m is not None)
    return datas, chains, masked


def material_inputs(name):
    """(MaterialData list, per material {slot: (host chain, mips, w, h)}, per material alpha-masked flag)"""
    if is_cards(name):
        return card_material_inputs(name)
    datas, chains = scene_material_inputs()
    return datas, chains, [False] * len(datas)


def host_materials(name):
    datas, chains, masked = material_inputs(name)
    mats = O.host_materials(datas, [{slot: (c, w, h, n) for slot, (c, n, w, h) in cs.items()} for cs in chains])
    for m, flag in zip(mats, masked):
        if flag:
            m.texDiffuse.reserved = abi.MATERIAL_ALPHA_MASKED
    return mats


def ssao_plane(w, h):
    return synth.ssao_image(w, h, seed=0x720)


# ---- what the CPU and the GPU tests share ------------------------------------------------------------------------------------------------------------------------------
class oracle_arithmetic:
    """the oracle's reading of dot / normalize / length (vqhip_set_arithmetic's counterpart) for the length of a `with` block"""

    def __init__(self, dxc):
        self.dxc = int(bool(dxc))

    def __enter__(self):
        O.load().vqo_set_arithmetic(self.dxc)

    def __exit__(self, *exc):
        O.load().vqo_set_arithmetic(0)


@functools.lru_cache(maxsize=None)
def expected_gbuffer(name, layer, ssao, dxc=0):
    """the helper rule's G-buffer of one owner plane of a case in one arithmetic reading: (four planes, ip2.w after the call)"""
    sc = cases()[name]
    out, _ = expected(name)[layer]
    s = ssao_plane(sc["width"], sc["height"]) if ssao else None
    with oracle_arithmetic(dxc):
        gb, idx = Q.gbuffer_from_materials_quad(ip_planes(out), out["quad_uv"], host_materials(name), 0.055, s)
    for a in gb + [idx]:
        a.setflags(write=False)
    return gb, idx


def expected_scene_normals(name, layer, out_fmt, dxc=0):
    out, _ = expected(name)[layer]
    with oracle_arithmetic(dxc):
        return Q.scene_normals_from_materials_quad(ip_planes(out), out["quad_uv"], host_materials(name), out_fmt)


@functools.lru_cache(maxsize=None)
def neighbour_gbuffer(name, layer, ssao):
    """the neighbour rule's (vqhip_gbuffer_from_materials') G-buffer of the same planes: (four planes, ip2.w after the call)"""
    sc = cases()[name]
    out, _ = expected(name)[layer]
    ip = ip_planes(out)
    with np.errstate(all="ignore"):
        gb = O.gbuffer_from_materials(ip, host_materials(name), 0.055, ssao_plane(sc["width"], sc["height"]) if ssao else None)
    return gb, np.ascontiguousarray(ip[2][..., 3]).view(np.int32)


def masked_owner_mask(name, layer):
    """the pixels of one owner plane of a cards case whose owner is a primitive of a masked draw"""
    sc = cases()[name]
    q = owners(name)[0][layer].astype(np.int64)
    m = np.zeros(q.shape, bool)
    first = 0
    for d in sc["draws"]:
        n = (len(d["indices"]) // 3) * np.asarray(d["wvp"]).shape[0]
        if d.get("mask") is not None:
            m |= (q >= first) & (q < first + n)
        first += n
    return m


# the cases and layers on which the neighbour rule disagrees with the pre-pass (tests/test_quad_interp_cpu.py asserts it; the GPU chains find the same counts)
INCONSISTENT = {"cards_minified_64x48_s1": (0,), "cards_minified_64x48_s4": (0, 1)}


def disagreements(name, layer):
    """(neighbour rule, helper rule): the (primitive, pixel) pairs that own a depth sample — the masked primitive passed masked_depth_ref's test there — and are
    discarded by the lit draw's producer all the same"""
    m = masked_owner_mask(name, layer)
    return int((m & (neighbour_gbuffer(name, layer, False)[1] == -1)).sum()), int((m & (expected_gbuffer(name, layer, False)[1] == -1)).sum())


def single_owner_frame(w, h, n_mat, seed):
    """synth.interpolants' ground plane with the material constant over every aligned 2 x 2 quad (even sizes): each quad has one owner, all of it inside the image"""
    ip = synth.interpolants(w, h, n_mat, seed=seed)
    idx = np.ascontiguousarray(ip[2][..., 3]).view(np.int32)
    jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    geometry = np.repeat(np.repeat(idx[0::2, 0::2], 2, axis=0), 2, axis=1) >= 0
    ip[2][..., 3] = np.where(geometry, ((ii // 2) // 3 + (jj // 2) // 2) % n_mat, -1).astype(np.int32).view(F)     # the material changes every few quads
    return ip
