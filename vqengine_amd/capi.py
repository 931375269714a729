"""Thin ctypes binding over the C ABI (include/vqhip.h, vqengine_amd/lib/libvqhip.so).

torch is used only as plumbing: device memory (tensor.data_ptr()) and the current HIP stream.
There is NO fallback: if the library is missing, or no gfx950 device is visible, this raises."""
import ctypes as C
import os

import torch

from . import abi
from .abi import (FMT_RGBA32F, FMT_RGBA16F, FMT_RGBA8_UNORM, FMT_RG16F, FMT_RG32F, CONV_SEQUENTIAL)

# $VQHIP_LIBRARY_PATH: another build of the SAME library (the sanitizer build of `make -C vqengine_amd/csrc asan`); never a different implementation
_LIB_PATH = os.environ.get("VQHIP_LIBRARY_PATH") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libvqhip.so")
_lib = None


class VQHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"vqhip error {code}: {msg}")
        self.code = code


def lib_path():
    return _LIB_PATH


def load_library():
    """dlopen libvqhip.so and declare every entry point of include/vqhip.h. Loud failure if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise FileNotFoundError(f"{_LIB_PATH} not built — run `python -c 'import __graft_entry__ as g; g.build()'` "
                                "(hipcc --offload-arch=gfx950). There is no CPU/PyTorch fallback for this path.")
    lib = C.CDLL(_LIB_PATH)
    vp, i32, f32, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    sig = {
        "vqhip_abi_version": (i32, []),
        "vqhip_create": (i32, [i32, C.POINTER(vp)]),
        "vqhip_destroy": (None, [vp]),
        "vqhip_last_error": (C.c_char_p, [vp]),
        "vqhip_forward_lighting": (i32, [vp, vp, C.POINTER(abi.GBuffer), C.POINTER(abi.PerFrameData), C.POINTER(abi.PerViewLightingData),
                                         vp, i32, C.POINTER(abi.EnvMap), C.POINTER(abi.ShadowMaps), vp, i32, i32]),
        "vqhip_forward_lighting_mrt": (i32, [vp, vp, C.POINTER(abi.GBuffer), C.POINTER(abi.PerFrameData), C.POINTER(abi.PerViewLightingData),
                                             vp, i32, C.POINTER(abi.EnvMap), C.POINTER(abi.ShadowMaps), vp, i32, i32, C.POINTER(abi.PsmainTargets)]),
        "vqhip_forward_lighting_msaa": (i32, [vp, vp, C.POINTER(abi.GBufferMSAA), C.POINTER(abi.PerFrameData), C.POINTER(abi.PerViewLightingData),
                                              vp, i32, C.POINTER(abi.EnvMap), C.POINTER(abi.ShadowMaps), vp, i32, vp, i32, i32]),
        "vqhip_msaa_resolve_surfaces": (i32, [vp, vp, C.POINTER(abi.MSAASurfaces), vp, i32, vp, i32, i32, vp, i32, i32, vp, C.c_uint]),
        "vqhip_depth_hierarchy_bytes": (sz, [i32, i32]),
        "vqhip_depth_hierarchy_level_offset_bytes": (sz, [i32, i32, i32]),
        "vqhip_depth_hierarchy": (i32, [vp, vp, vp, i32, i32, i32, vp, C.c_uint]),
        "vqhip_gaussian_blur": (i32, [vp, vp, vp, vp, vp, C.POINTER(abi.BlurParams), i32]),
        "vqhip_gaussian_blur_x": (i32, [vp, vp, vp, vp, C.POINTER(abi.BlurParams), i32]),
        "vqhip_gaussian_blur_y": (i32, [vp, vp, vp, vp, vp, vp, i32, C.POINTER(abi.BlurParams), i32]),
        "vqhip_tonemap": (i32, [vp, vp, vp, vp, i32, i32, C.POINTER(abi.TonemapperParams), i32, i32]),
        "vqhip_gaussian_blur_y_tonemap": (i32, [vp, vp, vp, vp, vp, vp, i32, C.POINTER(abi.BlurParams), C.POINTER(abi.TonemapperParams), i32, i32]),
        "vqhip_post_process": (i32, [vp, vp, vp, vp, i32, i32, C.POINTER(abi.TonemapperParams), i32, i32, i32]),
        "vqhip_post_process_tile": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, C.POINTER(abi.TonemapperParams), i32, i32]),
        "vqhip_brdf_lut": (i32, [vp, vp, vp, i32, i32, i32]),
        "vqhip_mip_level_count": (i32, [i32, i32]),
        "vqhip_mip_chain_bytes": (sz, [i32, i32, i32]),
        "vqhip_mip_level_offset_bytes": (sz, [i32, i32, i32]),
        "vqhip_mip_chain_min_rgba32f": (i32, [vp, vp, vp, i32, i32, i32]),
        "vqhip_specular_mip_count": (i32, [i32]),
        "vqhip_cube_bytes": (sz, [i32, i32, i32]),
        "vqhip_conv_diffuse": (i32, [vp, vp, vp, i32, i32, i32, i32, f32, i32, vp, i32]),
        "vqhip_conv_specular": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp, i32]),
        "vqhip_envmap_prefilter": (i32, [vp, vp, vp, i32, i32, i32, i32, f32, i32, i32, C.POINTER(abi.EnvMapOut)]),
        "vqhip_max_materials": (i32, []),
        "vqhip_gbuffer_from_materials": (i32, [vp, vp, C.POINTER(abi.Interpolants), C.POINTER(abi.MaterialDesc), i32, f32,
                                               C.POINTER(abi.SSAO), C.POINTER(abi.GBuffer)]),
        "vqhip_forward_lighting_from_materials": (i32, [vp, vp, C.POINTER(abi.Interpolants), C.POINTER(abi.MaterialDesc), i32, C.POINTER(abi.SSAO),
                                                        C.POINTER(abi.PerFrameData), C.POINTER(abi.PerViewLightingData), vp, i32,
                                                        C.POINTER(abi.EnvMap), C.POINTER(abi.ShadowMaps), vp, i32, i32]),
        "vqhip_forward_lighting_from_materials_mrt": (i32, [vp, vp, C.POINTER(abi.Interpolants), C.POINTER(abi.MaterialDesc), i32, C.POINTER(abi.SSAO),
                                                            C.POINTER(abi.PerFrameData), C.POINTER(abi.PerViewLightingData), vp, i32,
                                                            C.POINTER(abi.EnvMap), C.POINTER(abi.ShadowMaps), vp, i32, i32, C.POINTER(abi.PsmainTargets)]),
        "vqhip_scene_normals_from_materials": (i32, [vp, vp, C.POINTER(abi.Interpolants), C.POINTER(abi.MaterialDesc), i32, vp, i32, i32]),
        "vqhip_mip_chain_bytes_rgba8": (sz, [i32, i32, i32]),
        "vqhip_mip_chain_box_rgba8": (i32, [vp, vp, vp, i32, i32, i32]),
        "vqhip_set_fresnel_pow": (i32, [vp, i32]),
        "vqhip_set_arithmetic": (i32, [vp, i32]),
        "vqhip_set_option": (i32, [vp, C.c_char_p, C.c_char_p]),
        "vqhip_unlit_composite": (i32, [vp, vp, C.POINTER(abi.Interpolants), vp, i32, vp, i32, i32, i32, i32]),
        "vqhip_skydome": (i32, [vp, vp, vp, i32, i32, C.POINTER(abi.SkydomeParams), C.POINTER(abi.Interpolants), vp, i32, i32, i32, i32]),
        "vqhip_hdr_parse_header": (i32, [C.c_char_p, sz, C.POINTER(i32), C.POINTER(i32), C.POINTER(sz)]),
        "vqhip_hdr_decode_rgba32f": (i32, [vp, vp, C.c_char_p, sz, vp, i32, i32]),
        "vqhip_hdr_downsize_rgba32f": (i32, [vp, vp, vp, i32, i32, vp, i32, i32]),
        "vqhip_fsr_easu_con": (None, [C.POINTER(C.c_uint32), f32, f32, f32, f32, f32, f32]),
        "vqhip_fsr_rcas_con": (None, [C.POINTER(C.c_uint32), f32]),
        "vqhip_fsr_easu": (i32, [vp, vp, vp, i32, i32, i32, C.POINTER(C.c_uint32), vp, i32, i32, i32]),
        "vqhip_fsr_rcas": (i32, [vp, vp, vp, vp, i32, i32, C.POINTER(C.c_uint32), i32, i32]),
        "vqhip_visualize": (i32, [vp, vp, vp, vp, i32, i32, C.POINTER(abi.VizParams), i32, i32]),
        "vqhip_apply_reflections": (i32, [vp, vp, vp, vp, i32, i32, i32]),
        "vqhip_composite_reflections": (i32, [vp, vp, vp, vp, vp, i32, i32, i32]),
        "vqhip_ssr_environment_fallback": (i32, [vp, vp, vp, i32, i32, vp, i32, vp, i32, i32, i32, i32, C.POINTER(abi.SSSRConstants), C.POINTER(abi.EnvMap),
                                                 vp, i32, i32, vp]),
        "vqhip_ssr_classify": (i32, [vp, vp, vp, i32, i32, vp, i32, vp, i32, C.POINTER(abi.SSSRConstants), vp, vp, vp]),
        "vqhip_ssr_intersect": (i32, [vp, vp, vp, vp, vp, i32, i32, vp, vp, i32, i32, vp, vp, C.POINTER(abi.SSSRConstants), C.POINTER(abi.EnvMap),
                                      vp, i32, i32]),
        "vqhip_ssr_prefilter": (i32, [vp, vp, vp, vp, vp, i32, vp, i32, i32, vp, vp, i32, vp, i32, i32, vp, i32, C.POINTER(abi.SSSRConstants),
                                      vp, i32, i32, vp, i32]),
        "vqhip_ssr_resolve_temporal": (i32, [vp, vp, vp, vp, vp, vp, i32, vp, i32, i32, vp, i32, i32, vp, i32, vp, i32, C.POINTER(abi.SSSRConstants),
                                             vp, i32, i32, vp, i32]),
        "vqhip_ssr_reproject": (i32, [vp, vp, C.POINTER(abi.SSRReprojectSurfaces), C.POINTER(abi.SSSRConstants)]),
        "vqhip_cacao_work_bytes": (sz, [i32, i32]),
        "vqhip_cacao_plane_offset_bytes": (sz, [i32, i32, i32, i32, i32]),
        "vqhip_cacao": (i32, [vp, vp, vp, sz, vp, i32, sz, C.POINTER(abi.CacaoConstants), C.POINTER(abi.CacaoConstants), i32, i32, vp, sz, vp, sz, i32, i32]),
        "vqhip_adaptive_cacao_work_bytes": (sz, [i32, i32]),
        "vqhip_adaptive_cacao_plane_offset_bytes": (sz, [i32, i32, i32, i32, i32]),
        "vqhip_adaptive_cacao": (i32, [vp, vp, vp, sz, vp, i32, sz, C.POINTER(abi.CacaoConstants), C.POINTER(abi.CacaoConstants), i32, vp, sz, vp, sz, i32, i32]),
        "vqhip_shadow_depth_work_bytes": (sz, [C.c_uint64, i32]),
        "vqhip_shadow_depth": (i32, [vp, vp, C.POINTER(abi.ShadowView), i32, vp, sz]),
        "vqhip_scene_depth_work_bytes": (sz, [C.c_uint64]),
        "vqhip_scene_depth": (i32, [vp, vp, C.POINTER(abi.SceneDepthDraw), i32, i32, i32, i32, C.POINTER(abi.SceneDepthTargets), vp, sz]),
        "vqhip_scene_interpolants_work_bytes": (sz, [i32]),
        "vqhip_scene_masked_depth_work_bytes": (sz, [C.c_uint64, C.c_uint64, i32]),
        "vqhip_scene_masked_depth": (i32, [vp, vp, C.POINTER(abi.SceneDepthMaskedDraw), i32, i32, i32, i32, C.POINTER(abi.SceneDepthTargets), vp, sz]),
        "vqhip_shadow_masked_depth_work_bytes": (sz, [C.c_uint64, C.c_uint64, i32, i32]),
        "vqhip_shadow_masked_depth": (i32, [vp, vp, C.POINTER(abi.ShadowMaskedView), i32, vp, sz]),
        "vqhip_scene_interpolants": (i32, [vp, vp, C.POINTER(abi.SceneSurfaceDraw), i32, i32, i32, vp, i32, C.POINTER(abi.SceneInterpolantTargets), vp, sz]),
        "vqhip_scene_quad_interpolants": (i32, [vp, vp, C.POINTER(abi.SceneSurfaceDraw), i32, i32, i32, vp, i32, C.POINTER(abi.SceneQuadTargets), vp, sz]),
        "vqhip_gbuffer_from_materials_quad": (i32, [vp, vp, C.POINTER(abi.Interpolants), C.POINTER(abi.MaterialDesc), i32, f32,
                                                    C.POINTER(abi.SSAO), C.POINTER(abi.GBuffer), vp, i32]),
        "vqhip_forward_lighting_from_materials_quad": (i32, [vp, vp, C.POINTER(abi.Interpolants), C.POINTER(abi.MaterialDesc), i32, C.POINTER(abi.SSAO),
                                                             C.POINTER(abi.PerFrameData), C.POINTER(abi.PerViewLightingData), vp, i32,
                                                             C.POINTER(abi.EnvMap), C.POINTER(abi.ShadowMaps), vp, i32, i32, C.POINTER(abi.PsmainTargets), vp, i32]),
        "vqhip_scene_normals_from_materials_quad": (i32, [vp, vp, C.POINTER(abi.Interpolants), C.POINTER(abi.MaterialDesc), i32, vp, i32, i32, vp, i32]),
        "vqhip_object_ids_work_bytes": (sz, [i32]),
        "vqhip_object_ids": (i32, [vp, vp, C.POINTER(abi.ObjectIdDraw), i32, i32, i32, vp, i32, vp, i32, vp, sz]),
        "vqhip_outline_work_bytes": (sz, [C.c_uint64]),
        "vqhip_outline": (i32, [vp, vp, C.POINTER(abi.OutlineDraw), i32, i32, i32, C.POINTER(abi.OutlineTargets), vp, sz]),
        "vqhip_displace_meshes": (i32, [vp, vp, C.POINTER(abi.DisplaceJob), i32]),
        "vqhip_unlit_draws_work_bytes": (sz, [C.c_uint64]),
        "vqhip_unlit_draws": (i32, [vp, vp, C.POINTER(abi.UnlitDraw), i32, i32, i32, i32, C.POINTER(abi.UnlitTargets), vp, sz]),
        "vqhip_line_draws_work_bytes": (sz, [C.c_uint64]),
        "vqhip_line_draws": (i32, [vp, vp, C.POINTER(abi.LineDraw), i32, i32, i32, C.POINTER(abi.UnlitTargets), vp, sz]),
        "vqhip_rowtile": (i32, [i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]),
        "vqhip_comm_unique_id": (i32, [vp]),
        "vqhip_comm_create": (i32, [vp, i32, i32, C.POINTER(vp)]),
        "vqhip_comm_adopt": (i32, [vp, i32, i32, C.POINTER(vp)]),
        "vqhip_comm_destroy": (None, [vp]),
        "vqhip_comm_query": (i32, [vp, C.POINTER(abi.CommInfo)]),
        "vqhip_comm_abort": (i32, [vp]),
        "vqhip_comm_loopback": (i32, [vp, vp, vp, vp, sz]),
        "vqhip_exchange_blur_halos": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, vp]),
        "vqhip_composite_tiles": (i32, [vp, vp, vp, i32, i32, i32, i32, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype, fn.argtypes = res, args
    if lib.vqhip_abi_version() != abi.ABI_VERSION:
        raise RuntimeError("libvqhip.so ABI version mismatch")
    _lib = lib
    return lib


EXPORTED_SYMBOLS = [
    "vqhip_abi_version", "vqhip_create", "vqhip_destroy", "vqhip_last_error", "vqhip_forward_lighting", "vqhip_forward_lighting_mrt", "vqhip_forward_lighting_from_materials_mrt", "vqhip_scene_normals_from_materials",
    "vqhip_gaussian_blur", "vqhip_gaussian_blur_x", "vqhip_gaussian_blur_y", "vqhip_gaussian_blur_y_tonemap", "vqhip_tonemap", "vqhip_post_process", "vqhip_post_process_tile", "vqhip_brdf_lut",
    "vqhip_mip_level_count", "vqhip_mip_chain_bytes", "vqhip_mip_level_offset_bytes", "vqhip_mip_chain_min_rgba32f",
    "vqhip_specular_mip_count", "vqhip_cube_bytes", "vqhip_conv_diffuse", "vqhip_conv_specular", "vqhip_envmap_prefilter",
    "vqhip_max_materials", "vqhip_gbuffer_from_materials", "vqhip_forward_lighting_from_materials", "vqhip_mip_chain_bytes_rgba8", "vqhip_mip_chain_box_rgba8",
    "vqhip_skydome", "vqhip_unlit_composite", "vqhip_set_fresnel_pow", "vqhip_set_arithmetic", "vqhip_set_option", "vqhip_hdr_parse_header", "vqhip_hdr_decode_rgba32f", "vqhip_hdr_downsize_rgba32f",
    "vqhip_fsr_easu_con", "vqhip_fsr_rcas_con", "vqhip_fsr_easu", "vqhip_fsr_rcas", "vqhip_visualize", "vqhip_apply_reflections", "vqhip_composite_reflections", "vqhip_ssr_environment_fallback",
    "vqhip_rowtile", "vqhip_comm_unique_id", "vqhip_comm_create", "vqhip_comm_adopt", "vqhip_comm_destroy", "vqhip_comm_query", "vqhip_comm_abort", "vqhip_comm_loopback", "vqhip_exchange_blur_halos",
    "vqhip_composite_tiles", "vqhip_forward_lighting_msaa",
    "vqhip_msaa_resolve_surfaces", "vqhip_depth_hierarchy", "vqhip_depth_hierarchy_bytes", "vqhip_depth_hierarchy_level_offset_bytes",
    "vqhip_ssr_classify", "vqhip_ssr_intersect", "vqhip_ssr_prefilter", "vqhip_ssr_resolve_temporal", "vqhip_ssr_reproject",
    "vqhip_cacao", "vqhip_cacao_work_bytes", "vqhip_cacao_plane_offset_bytes",
    "vqhip_adaptive_cacao", "vqhip_adaptive_cacao_work_bytes", "vqhip_adaptive_cacao_plane_offset_bytes",
    "vqhip_shadow_depth", "vqhip_shadow_depth_work_bytes",
    "vqhip_scene_depth", "vqhip_scene_depth_work_bytes",
    "vqhip_scene_interpolants", "vqhip_scene_interpolants_work_bytes",
    "vqhip_scene_masked_depth", "vqhip_scene_masked_depth_work_bytes", "vqhip_shadow_masked_depth", "vqhip_shadow_masked_depth_work_bytes",
    "vqhip_scene_quad_interpolants", "vqhip_gbuffer_from_materials_quad", "vqhip_forward_lighting_from_materials_quad", "vqhip_scene_normals_from_materials_quad",
    "vqhip_object_ids", "vqhip_object_ids_work_bytes", "vqhip_outline", "vqhip_outline_work_bytes",
    "vqhip_displace_meshes",
    "vqhip_unlit_draws", "vqhip_unlit_draws_work_bytes",
    "vqhip_line_draws", "vqhip_line_draws_work_bytes",
]


def _check_vertices(who, name, p, k):           # this and the helpers below: what the three rasteriser bindings (_*_prepared) check and fill alike
    if not (p.is_cuda and p.dtype == torch.float32 and p.dim() == 2 and p.shape[1] >= k and p.stride(1) == 1 and p.stride(0) >= p.shape[1]):
        raise ValueError(f"{who}: {name}: expected cuda float32 [V, k >= {k}] with unit column stride")


def _check_indices(who, ix):                    # -> the index width in bits
    bits = {2: 16, 4: 32}.get(ix.element_size()) if not ix.dtype.is_floating_point else None
    if not (ix.is_cuda and ix.dim() == 1 and ix.is_contiguous() and bits and ix.numel() % 3 == 0):
        raise ValueError(f"{who}: indices: expected a contiguous cuda 1-D 16-bit or 32-bit integer tensor whose length is a multiple of 3")
    return bits


def _check_matrix_blocks(who, blocks, same=""):
    """blocks: (name, tensor, optional: may be None), the first one sets n; `same` ends the message -> n, the instance count"""
    n = blocks[0][1].shape[0] if blocks[0][1].dim() == 3 else 0
    for name, m, optional in blocks:
        if not (optional if m is None else m.is_cuda and m.dtype == torch.float32 and tuple(m.shape) == (n, 4, 4) and m.is_contiguous()):
            raise ValueError(f"{who}: {name}: expected cuda float32 [n, 4, 4] contiguous{same}")
    return n


def _check_instances_cull(who, n, limit, cull=abi.CULL_NONE):
    if not 1 <= n <= limit:
        raise ValueError(f"{who}: 1..{limit} instances, got {n}")
    if cull not in (abi.CULL_NONE, abi.CULL_FRONT, abi.CULL_BACK):
        raise ValueError(f"{who}: cull: expected abi.CULL_NONE, CULL_FRONT or CULL_BACK")


def _fill_mesh(c, p, ix, bits, empty_indices=None):     # empty_indices: the address an index tensor without elements (which has none) is given
    c.mesh.positions, c.mesh.strideBytes, c.mesh.numVertices = p.data_ptr(), p.stride(0) * 4, p.shape[0]
    c.mesh.indices, c.mesh.indexBits, c.mesh.numIndices = ix.data_ptr() or empty_indices, bits, ix.numel()


def _work_tensor(who, work, need, device, zero=""):     # allocated when None, else checked; zero: what need == 0 means, where it is refused
    if work is None:
        work = torch.empty((need,), dtype=torch.uint8, device=device)
    if not (work.is_cuda and work.dtype == torch.uint8 and work.is_contiguous() and work.numel() >= need and (need or not zero)):
        raise ValueError(f"{who}: work: expected a contiguous cuda uint8 tensor of at least {need} bytes{zero}")
    return work


def scene_interpolants_work_bytes(num_draws):
    """vqhip_scene_interpolants_work_bytes: the work buffer (the draw table's device home) of a vqhip_scene_interpolants call of `num_draws` draws. Host-only."""
    return load_library().vqhip_scene_interpolants_work_bytes(int(num_draws))


class SurfaceDraw:
    """One vqhip_scene_surface_draw. vertices: cuda float32 [V, k] with k >= 11 and unit column stride (position 3, normal 3, tangent 3, uv 2; the row stride is
    the vertex stride); indices: cuda 1-D int16 / uint16 (read as 16-bit unsigned) or int32, a triangle list; wvp / world / normal / wvp_prev: cuda float32
    [n, 4, 4] contiguous, VQ_matrix memory order (wvp_prev may be None when no svPosition plane is asked for); material: the index written to ip2.w."""

    def __init__(self, vertices, indices, wvp, world, normal, wvp_prev=None, material=0):
        self.vertices, self.indices, self.wvp, self.world, self.normal, self.wvp_prev, self.material = vertices, indices, wvp, world, normal, wvp_prev, int(material)

    def depth_draw(self, cull=abi.CULL_NONE):
        """the same draw for vqhip_scene_depth / vqhip_shadow_depth"""
        return ShadowDraw(self.vertices, self.indices, self.wvp, self.world, cull)


def object_ids_work_bytes(num_draws):
    """vqhip_object_ids_work_bytes: the work buffer (the draw table's device home) of a vqhip_object_ids call of `num_draws` draws. Host-only."""
    return load_library().vqhip_object_ids_work_bytes(int(num_draws))


class ObjectIdDraw:
    """One vqhip_object_id_draw: what one draw of the depth call that wrote the owner plane drew (num_indices, and the instance count = obj_id.shape[0]), and what
    ObjectID.hlsl writes for it. obj_id: cuda int32 [n, 4] contiguous (PerObjectLightingData.ObjID; columns 0 and 3 are read); mesh_id, material_id: ints."""

    def __init__(self, num_indices, obj_id, mesh_id, material_id):
        self.num_indices, self.obj_id, self.mesh_id, self.material_id = int(num_indices), obj_id, int(mesh_id), int(material_id)


def outline_work_bytes(triangles):
    """vqhip_outline_work_bytes: the work buffer of a vqhip_outline call that draws `triangles` triangles in all (0: too many). Host-only."""
    return load_library().vqhip_outline_work_bytes(int(triangles))


class OutlineDraw:
    """One vqhip_outline_draw: one selected (mesh, material) pair. vertices: cuda float32 [V, k] with k >= 6 and unit column stride (position 3, normal 3; the row
    stride is the vertex stride); indices: cuda 1-D int16 / uint16 (read as 16-bit unsigned) or int32, a triangle list; cb: cuda uint8 [368] contiguous or float32
    [92], one VQ_OutlineData (outline_scene.outline_data builds it)."""

    def __init__(self, vertices, indices, cb):
        self.vertices, self.indices, self.cb = vertices, indices, cb


def unlit_draws_work_bytes(triangles):
    """vqhip_unlit_draws_work_bytes: the work buffer of a vqhip_unlit_draws call that draws `triangles` triangles in all (0: too many). Host-only."""
    return load_library().vqhip_unlit_draws_work_bytes(int(triangles))


class UnlitDraw:
    """One vqhip_unlit_draw: one mesh with one matrix and one colour. positions: cuda float32 [V, k] with k >= 3 and unit column stride (the row stride is the
    vertex stride); indices: cuda 1-D int16 / uint16 (read as 16-bit unsigned) or int32, a triangle list; cb: cuda uint8 [80] contiguous or float32 [20], one
    VQ_UnlitData (unlit_scene.unlit_data builds it); cull: abi.CULL_* (the reference draws with CULL_BACK)."""

    def __init__(self, positions, indices, cb, cull=abi.CULL_BACK):
        self.positions, self.indices, self.cb, self.cull = positions, indices, cb, int(cull)


def line_draws_work_bytes(lines):
    """vqhip_line_draws_work_bytes: the work buffer of a vqhip_line_draws call that draws `lines` lines in all (0: too many). Host-only."""
    return load_library().vqhip_line_draws_work_bytes(int(lines))


class WireframeDraw:
    """One vqhip_line_draw of kind WIREFRAME: every edge of every triangle of one mesh, once per instance, in one colour. positions: cuda float32 [V, k] with
    k >= 3 and unit column stride; indices: cuda 1-D int16 / uint16 (read as 16-bit unsigned) or int32, a triangle list; matrices: cuda float32 [n, 4, 4]
    contiguous, n = 1 .. 512 (matModelViewProj per instance); color: cuda float32 [4] contiguous."""
    kind = abi.LINES_WIREFRAME

    def __init__(self, positions, indices, matrices, color):
        self.positions, self.indices, self.matrices, self.color = positions, indices, matrices, color


class VertexAxesDraw:
    """One vqhip_line_draw of kind VERTEX_AXES: three coloured lines per INDEX of a point list. vertices: cuda float32 [V, k] with k >= 9 and unit column stride
    (position 3, normal 3, tangent 3); indices: cuda 1-D 16-bit or 32-bit integers, any length; cb: cuda uint8 [208] contiguous or float32 [52], one
    VQ_VertexAxesData (line_scene.vertex_axes_data builds it)."""
    kind = abi.LINES_VERTEX_AXES

    def __init__(self, vertices, indices, cb):
        self.vertices, self.indices, self.cb = vertices, indices, cb


class DisplaceJob:
    """One vqhip_displace_job. vertices: cuda float32 [V, k] with k >= 11 and unit column stride (the engine's vertex: position 3, normal 3, tangent 3, uv 2; the
    row stride is the vertex stride; V may be 0); heightmap: abi.Texture2D (host descriptor of a cuda RGBA8 mip chain, level 0 is read; texels None = null SRV) or
    None for the null SRV; uv_scale_offset: MaterialData.uvScaleOffset, 4 floats (scale.xy, offset.xy); displacement: MaterialData.displacement; compact: write
    the 12-byte positions-only stream instead of the full-stride copy; out: a preallocated cuda float32 [V, 3] contiguous (compact) or [V, k'] with the input's row
    stride, else allocated."""

    def __init__(self, vertices, heightmap=None, uv_scale_offset=(1.0, 1.0, 0.0, 0.0), displacement=0.0, compact=False, out=None):
        self.vertices, self.heightmap, self.uv_scale_offset, self.displacement = vertices, heightmap, tuple(float(x) for x in uv_scale_offset), float(displacement)
        self.compact, self.out = bool(compact), out


def scene_depth_work_bytes(instanced_triangles):
    """vqhip_scene_depth_work_bytes: the work buffer of a vqhip_scene_depth call that draws `instanced_triangles` triangles in all. Host-only."""
    return load_library().vqhip_scene_depth_work_bytes(int(instanced_triangles))


def shadow_depth_work_bytes(instanced_triangles, num_views):
    """vqhip_shadow_depth_work_bytes: the work buffer of a vqhip_shadow_depth call whose views draw `instanced_triangles` triangles in all. Host-only."""
    return load_library().vqhip_shadow_depth_work_bytes(int(instanced_triangles), int(num_views))


class ShadowDraw:
    """One vqhip_shadow_draw. positions: cuda float32 [V, k] with k >= 3 and unit column stride (the row stride is the vertex stride: k = 3 tight, k = 11 the
    engine's 44-byte vertex); indices: cuda 1-D int16 / uint16 (read as 16-bit unsigned) or int32, a triangle list; wvp / world: cuda float32 [n, 4, 4]
    contiguous, VQ_matrix memory order (world may be None outside linear-depth views); cull: abi.CULL_*."""

    def __init__(self, positions, indices, wvp, world=None, cull=abi.CULL_NONE):
        self.positions, self.indices, self.wvp, self.world, self.cull = positions, indices, wvp, world, cull


class MaskedDraw(ShadowDraw):
    """A ShadowDraw for vqhip_scene_masked_depth / vqhip_shadow_masked_depth: positions are the engine's vertex (cuda float32 [V, k >= 11], uv at floats 9, 10).
    material: abi.MaterialDesc (host) or None, read by scene_masked_depth — masked iff texDiffuse.reserved has abi.MATERIAL_ALPHA_MASKED; texture: abi.Texture2D
    (host descriptor of a cuda RGBA8 mip chain; texels None = null SRV) or None, read by shadow_masked_depth — masked iff not None."""

    def __init__(self, positions, indices, wvp, world=None, cull=abi.CULL_NONE, material=None, texture=None):
        super().__init__(positions, indices, wvp, world, cull)
        self.material, self.texture = material, texture


def scene_masked_depth_work_bytes(instanced_triangles, masked_instanced_triangles, num_draws):
    """vqhip_scene_masked_depth_work_bytes. Host-only."""
    return load_library().vqhip_scene_masked_depth_work_bytes(int(instanced_triangles), int(masked_instanced_triangles), int(num_draws))


def shadow_masked_depth_work_bytes(instanced_triangles, masked_instanced_triangles, num_views, num_draws):
    """vqhip_shadow_masked_depth_work_bytes (num_draws: the draws of all views). Host-only."""
    return load_library().vqhip_shadow_masked_depth_work_bytes(int(instanced_triangles), int(masked_instanced_triangles), int(num_views), int(num_draws))


class ShadowView:
    """One vqhip_shadow_view. depth: cuda float32 [dim, dim] with unit column stride (a slice of the arrays vqhip_shadowmaps points at); linear: LINEAR_DEPTH
    (point-light faces) with camera = the light's position and far = its range; draws: a list of ShadowDraw."""

    def __init__(self, depth, draws=(), linear=False, camera=(0.0, 0.0, 0.0), far=1.0):
        self.depth, self.draws, self.linear, self.camera, self.far = depth, list(draws), bool(linear), tuple(camera), float(far)

    def instanced_triangles(self):
        return sum((d.indices.numel() // 3) * d.wvp.shape[0] for d in self.draws)


def cacao_work_bytes(width, height):
    """vqhip_cacao_work_bytes: the size of vqhip_cacao's work buffer for a width x height frame. Host-only."""
    return load_library().vqhip_cacao_work_bytes(width, height)


def cacao_plane_offset_bytes(width, height, plane, slice_index=0, mip=0):
    """vqhip_cacao_plane_offset_bytes: where slice `slice_index` of abi.CACAO_PLANE_* (mip `mip` of the depths) starts inside the work buffer. Host-only."""
    return load_library().vqhip_cacao_plane_offset_bytes(width, height, plane, slice_index, mip)


def cacao_work_planes(work, width, height):
    """Views of every intermediate of vqhip_cacao inside its work buffer (a uint8 tensor or numpy array of cacao_work_bytes bytes): dict with `depths` (four
    float16 [4, rows, cols] mips), `normals` int8 [4, hh, hw, 4], `ping` / `pong` uint8 [4, hh, hw, 2]"""
    hw, hh = abi.cacao_half_dims(width, height)
    f16, i8 = (torch.float16, torch.int8) if hasattr(work, "is_cuda") else ("float16", "int8")

    def view(plane, mip, rows, cols, ch, dtype, size):
        off = cacao_plane_offset_bytes(width, height, plane, 0, mip)
        v = work[off:off + 4 * rows * cols * ch * size]
        v = v.view(dtype) if dtype is not None else v
        return v.reshape((4, rows, cols) + ((ch,) if ch > 1 else ()))
    depths = [view(abi.CACAO_PLANE_DEPTHS, k, abi.mip_dim(hh, k), abi.mip_dim(hw, k), 1, f16, 2) for k in range(abi.CACAO_DEPTH_MIPS)]
    return {"depths": depths, "normals": view(abi.CACAO_PLANE_NORMALS, 0, hh, hw, 4, i8, 1), "ping": view(abi.CACAO_PLANE_PING, 0, hh, hw, 2, None, 1),
            "pong": view(abi.CACAO_PLANE_PONG, 0, hh, hw, 2, None, 1)}


def adaptive_cacao_work_bytes(width, height):
    """vqhip_adaptive_cacao_work_bytes: the size of vqhip_adaptive_cacao's work buffer (quality HIGHEST) for a width x height frame. Host-only."""
    return load_library().vqhip_adaptive_cacao_work_bytes(width, height)


def adaptive_cacao_plane_offset_bytes(width, height, plane, slice_index=0, mip=0):
    """vqhip_adaptive_cacao_plane_offset_bytes: as cacao_plane_offset_bytes for the four planes of HIGH's layout (the prefix), and where abi.CACAO_PLANE_IMPORTANCE,
    _IMPORTANCE_PONG and _LOAD_COUNTER start (slice 0, mip 0). Host-only."""
    return load_library().vqhip_adaptive_cacao_plane_offset_bytes(width, height, plane, slice_index, mip)


def adaptive_cacao_work_planes(work, width, height):
    """cacao_work_planes of vqhip_adaptive_cacao's work buffer plus `importance` / `importance_pong` uint8 [ih, iw] and `counter`, a view of one int32 (torch has no
    uint32 arithmetic; a numpy buffer gives uint32). After a call with no blur `pong` is the base pass's (obscurance, weight / 20)."""
    hw, hh = abi.cacao_half_dims(width, height)
    iw, ih = abi.cacao_half_dims(hw, hh)
    out = cacao_work_planes(work, width, height)
    for key, plane in (("importance", abi.CACAO_PLANE_IMPORTANCE), ("importance_pong", abi.CACAO_PLANE_IMPORTANCE_PONG)):
        off = adaptive_cacao_plane_offset_bytes(width, height, plane)
        out[key] = work[off:off + iw * ih].reshape((ih, iw))
    off = adaptive_cacao_plane_offset_bytes(width, height, abi.CACAO_PLANE_LOAD_COUNTER)
    out["counter"] = work[off:off + 4].view(torch.int32 if hasattr(work, "is_cuda") else "uint32")
    return out


def fsr_easu_con(in_w, in_h, out_w, out_h, container_w=None, container_h=None):
    """FFSR1_EASU::UpdateEASUConstantBlock (PostProcess.cpp:47-79): the 16-dword EASU cbuffer. Host-only."""
    con = (C.c_uint32 * 16)()
    load_library().vqhip_fsr_easu_con(con, in_w, in_h, container_w or in_w, container_h or in_h, out_w, out_h)
    return con


def fsr_rcas_con(sharpness_stops=0.2):
    """FFSR1_RCAS::UpdateRCASConstantBlock (PostProcess.cpp:39-45; default RCASSharpnessStops 0.2, PostProcess.h:129)."""
    con = (C.c_uint32 * 4)()
    load_library().vqhip_fsr_rcas_con(con, sharpness_stops)
    return con


def hdr_parse_header(data):
    """(width, height, data_offset) of a Radiance .hdr file held in `data` (bytes). Host-only; raises VQHipError when malformed."""
    lib = load_library()
    w, h, off = C.c_int(), C.c_int(), C.c_size_t()
    rc = lib.vqhip_hdr_parse_header(data, len(data), C.byref(w), C.byref(h), C.byref(off))
    if rc != 0:
        raise VQHipError(rc, (lib.vqhip_last_error(None) or b"").decode())
    return w.value, h.value, off.value

HALO_ROWS = 10            # VQHIP_HALO_ROWS
ALL_RANKS = -1            # VQHIP_ALL_RANKS
COMM_ID_BYTES = 128       # VQHIP_COMM_ID_BYTES


def _global_error(rc):
    raise VQHipError(rc, (load_library().vqhip_last_error(None) or b"").decode())


def rowtile(frame_height, world, rank):
    """(row0, rows) of rank `rank` (vqhip_rowtile)."""
    r0, n = C.c_int(), C.c_int()
    rc = load_library().vqhip_rowtile(frame_height, world, rank, C.byref(r0), C.byref(n))
    if rc != 0:
        _global_error(rc)
    return r0.value, n.value


def comm_unique_id():
    """bytes(128): ncclGetUniqueId through the C ABI; made on rank 0 and handed to the other ranks out of band."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = load_library().vqhip_comm_unique_id(buf)
    if rc != 0:
        _global_error(rc)
    return buf.raw


def _addr(x):
    """device pointer of a torch tensor, or host pointer of a numpy array (the mock-RCCL tests); None -> NULL"""
    if x is None:
        return C.c_void_p(None)
    return C.c_void_p(x.data_ptr()) if hasattr(x, "data_ptr") else C.c_void_p(x.ctypes.data)


class Comm:
    """vqhip_comm: the RCCL communicator of the row-tiled multi-GPU mode (include/vqhip.h). Collective constructor."""

    def __init__(self, unique_id, world, rank):
        self.lib = load_library()
        self.world, self.rank = world, rank
        h = C.c_void_p()
        rc = self.lib.vqhip_comm_create(unique_id, world, rank, C.byref(h))
        if rc != 0:
            _global_error(rc)
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.lib.vqhip_comm_destroy(self._h)
            self._h = None

    def abort(self):
        """ncclCommAbort + free (vqhip_comm_abort): the way out of an exchange that does not complete. The object is dead afterwards."""
        if getattr(self, "_h", None):
            h, self._h = self._h, None
            rc = self.lib.vqhip_comm_abort(h)
            if rc != 0:
                _global_error(rc)

    def query(self):
        """What the communicator reports about itself (vqhip_comm_query): RCCL's own rank count / rank, its version, the library's path."""
        info = abi.CommInfo()
        rc = self.lib.vqhip_comm_query(self._h, C.byref(info))
        if rc != 0:
            _global_error(rc)
        return {"world": info.world, "rank": info.rank, "nranks_seen": info.nranks_seen, "rank_seen": info.rank_seen,
                "version": info.rccl_version, "library_path": info.library_path.decode(errors="replace")}

    def loopback(self, src, dst, stream=None):
        """One grouped ncclSend + ncclRecv from this rank to itself (vqhip_comm_loopback): src -> dst, same byte size, enqueued on `stream`."""
        n = src.numel() * src.element_size() if hasattr(src, "numel") else src.nbytes
        rc = self.lib.vqhip_comm_loopback(self._h, stream, _addr(src), _addr(dst), n)
        if rc != 0:
            _global_error(rc)

    def exchange_blur_halos(self, x_tile, fmt, halo_top, halo_bottom, stream=None):
        """x_tile [rows, W, 4]; halo_top / halo_bottom: preallocated [10, W, 4] buffers (None at the frame's edges)."""
        rows, w = x_tile.shape[0], x_tile.shape[1]
        rc = self.lib.vqhip_exchange_blur_halos(self._h, stream, _addr(x_tile), w, rows, w, fmt, _addr(halo_top), _addr(halo_bottom))
        if rc != 0:
            _global_error(rc)

    def composite_tiles(self, tile, fmt, frame_height, root, frame, stream=None):
        """tile [rows, W, C] -> frame [frame_height, W, C] on `root` (or every rank: ALL_RANKS)."""
        rc = self.lib.vqhip_composite_tiles(self._h, stream, _addr(tile), tile.shape[1], frame_height, fmt, root, _addr(frame))
        if rc != 0:
            _global_error(rc)


_TORCH_DTYPE = {FMT_RGBA32F: (torch.float32, 4), FMT_RGBA16F: (torch.float16, 4), FMT_RGBA8_UNORM: (torch.uint8, 4),
                FMT_RG16F: (torch.float16, 2), FMT_RG32F: (torch.float32, 2)}


def empty_image(h, w, fmt, device):
    dt, ch = _TORCH_DTYPE[fmt]
    return torch.empty((h, w, ch), dtype=dt, device=device)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _check_img(t, fmt, name, hw=None):
    """contiguous cuda image of `fmt`; hw = (rows, width) it must have (the C ABI takes raw pointers: a smaller `out` would be an
    out-of-bounds device write)."""
    dt, ch = _TORCH_DTYPE[fmt]
    if not (t.is_cuda and t.is_contiguous() and t.dtype == dt and t.shape[-1] == ch):
        raise ValueError(f"{name}: expected contiguous cuda tensor [...,{ch}] of {dt}, got {tuple(t.shape)} {t.dtype} {t.device}")
    if hw is not None and tuple(t.shape[:2]) != tuple(hw):
        raise ValueError(f"{name}: expected {hw[0]} x {hw[1]} pixels, got {tuple(t.shape[:2])}")


def _check_plane(what, t, dtype, hw):               # this and the helpers below: what the SSR bindings check alike; a label carries the binding's prefix, if it has one
    """one element per pixel, rows may be strided -> the row pitch in elements; what: "<label>: expected cuda <dtype as that binding spells it>" """
    if not (t.is_cuda and t.dtype == dtype and tuple(t.shape) == tuple(hw) and t.stride(1) == 1 and t.stride(0) >= hw[1]):
        raise ValueError(f"{what} {tuple(hw)} with unit column stride")
    return t.stride(0)


def _check_dense(label, t, dtype, shape):
    if not (t.is_cuda and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous()):
        raise ValueError(f"{label}: expected contiguous cuda {str(dtype)[6:]} {tuple(shape)}")


def _check_words(label, t, hw, fmt_name):           # packed 32-bit pixels, such as the R11G11B10_FLOAT average
    if not (t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == tuple(hw) and t.is_contiguous()):
        raise ValueError(f"{label}: expected contiguous cuda int32 {tuple(hw)} ({fmt_name} words)")


def _check_normals(who, name, t, fmt, hw):          # R10G10B10A2_UNORM words or an image
    if fmt == abi.FMT_R10G10B10A2_UNORM:
        _check_words(who + name, t, hw, "R10G10B10A2_UNORM")
    else:
        _check_img(t, fmt, name, hw)


def _check_list(label, t, n):                       # tile_list, counters, ray_list: at least n words
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= n):
        raise ValueError(f"{label}: expected contiguous cuda int32 [{n}]")


def _check_tiles(who, tile_list, counters, tiles):
    _check_list(who + "tile_list", tile_list, tiles)
    _check_list(who + "counters", counters, 2)


def _byref(struct):                                 # this and the helpers below: what the lit-draw bindings build alike. An optional struct argument
    return C.byref(struct) if struct is not None else None


def _interpolants(ip):
    """the vqhip_interpolants planes (float32 cuda [H,W,4]) -> (abi.Interpolants, H, W)"""
    for i, t in enumerate(ip):
        _check_img(t, FMT_RGBA32F, f"ip{i}")
    h, w = ip[0].shape[0], ip[0].shape[1]
    return abi.Interpolants(ip[0].data_ptr(), ip[1].data_ptr(), ip[2].data_ptr(), w, h, w), h, w


def _gbuffer(planes, h, w):                         # four dense planes that the caller has checked
    return abi.GBuffer(planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), planes[3].data_ptr(), w, h, w)


def _ssao(ssao):
    if ssao is None:
        return None
    if not (ssao.is_cuda and ssao.is_contiguous() and ssao.dtype == torch.uint8 and ssao.dim() == 2):
        raise ValueError("ssao: expected contiguous cuda uint8 [H,W]")
    return abi.SSAO(ssao.data_ptr(), ssao.shape[1], ssao.shape[0])


def _extra_point(extra_point):                      # the extension array of point lights -> (pointer, count)
    n = len(extra_point) if extra_point is not None else 0
    return (C.cast(extra_point, C.c_void_p) if n else C.c_void_p(None)), n


def _out_image(out, h, w, fmt, device):             # `out`, or a new image when None: H x W pixels of `fmt`
    if out is None:
        out = empty_image(h, w, fmt, device)
    _check_img(out, fmt, "out", (h, w))
    return out


def _halo_rows(halo_top, halo_bottom, fmt, width):
    """Both halos of a tile have the same row count (>= 10) and the tile's width and format."""
    rows = 0
    for hh in (halo_top, halo_bottom):
        if hh is not None:
            _check_img(hh, fmt, "halo", (hh.shape[0], width))
            if rows and hh.shape[0] != rows:
                raise ValueError(f"halo_top and halo_bottom must have the same number of rows, got {rows} and {hh.shape[0]}")
            rows = hh.shape[0]
    return rows


class Context:
    """One vqhip_ctx bound to one GPU. Calls enqueue on torch's current stream for that device."""

    def __init__(self, device_ordinal=0):
        self.lib = load_library()
        self.device = torch.device("cuda", device_ordinal)
        h = C.c_void_p()
        rc = self.lib.vqhip_create(device_ordinal, C.byref(h))
        if rc != 0:
            raise VQHipError(rc, (self.lib.vqhip_last_error(None) or b"").decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.lib.vqhip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self, stream=None):
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        return C.c_void_p(s.cuda_stream)

    def _ck(self, rc):
        if rc != 0:
            raise VQHipError(rc, (self.lib.vqhip_last_error(self._h) or b"").decode())

    # ---- forward lighting (RenderSceneColor, SceneRendering.cpp:1619) --------------------------------------
    def _psmain_targets(self, h, w, albedo_fmt, motion_fmt, sv_curr, sv_prev, stream=None):
        """vqhip_psmain_targets + the tensors it points at: (struct, albedo_metallic | None, motion_vectors | None). The clears run on `stream` — the stream the
        kernel is launched on: the kernel skips uncovered pixels, so a clear that is not ordered in front of it on the same stream could wipe written pixels."""
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            return self._psmain_targets_on_current_stream(h, w, albedo_fmt, motion_fmt, sv_curr, sv_prev)

    def _psmain_targets_on_current_stream(self, h, w, albedo_fmt, motion_fmt, sv_curr, sv_prev):
        t = abi.PsmainTargets()
        albedo = motion = None
        if albedo_fmt is not None:
            albedo = empty_image(h, w, albedo_fmt, self.device).zero_()          # the clear value: uncovered pixels of the one-kernel PSMain keep it
            t.albedo_metallic, t.albedo_fmt, t.albedo_pitch_px = albedo.data_ptr(), albedo_fmt, w
        if motion_fmt is not None:
            if sv_curr is None or sv_prev is None:
                raise ValueError("motion vectors need sv_curr and sv_prev (float32 cuda [H,W,4])")
            _check_img(sv_curr, FMT_RGBA32F, "sv_curr", (h, w)); _check_img(sv_prev, FMT_RGBA32F, "sv_prev", (h, w))
            motion = empty_image(h, w, motion_fmt, self.device).zero_()
            t.motion_vectors, t.motion_fmt, t.motion_pitch_px = motion.data_ptr(), motion_fmt, w
            t.svPositionCurr, t.svPositionPrev, t.sv_pitch_px = sv_curr.data_ptr(), sv_prev.data_ptr(), w
        return t, albedo, motion

    def forward_lighting_mrt(self, gb, per_frame, per_view, albedo_fmt=FMT_RGBA16F, motion_fmt=None, sv_curr=None, sv_prev=None, out=None,
                             out_fmt=FMT_RGBA16F, extra_point=None, env=None, shadow=None, stream=None):
        """forward_lighting + the draw's other render targets (ForwardLighting.hlsl:382-389) from the same kernel: returns (out, albedo_metallic, motion_vectors);
        albedo_fmt / motion_fmt None = that target not bound (-> None)."""
        h, w = gb[0].shape[0], gb[0].shape[1]
        t, albedo, motion = self._psmain_targets(h, w, albedo_fmt, motion_fmt, sv_curr, sv_prev, stream=stream)
        out = self.forward_lighting(gb, per_frame, per_view, out=out, out_fmt=out_fmt, extra_point=extra_point, env=env, shadow=shadow, stream=stream, _targets=t)
        return out, albedo, motion

    def forward_lighting(self, gb, per_frame, per_view, out=None, out_fmt=FMT_RGBA16F, extra_point=None, env=None, shadow=None, stream=None, _targets=None):
        """gb: tuple of 4 float32 cuda tensors [H,W,4] (gb0..gb3). env: abi.EnvMap or None. Returns out tensor."""
        g0, g1, g2, g3 = gb
        h, w = g0.shape[0], g0.shape[1]
        for i, g in enumerate(gb):
            _check_img(g, FMT_RGBA32F, f"gb{i}", (h, w))             # all four planes share one shape
        out = _out_image(out, h, w, out_fmt, self.device)
        gbuf = _gbuffer(gb, h, w)
        args = (self._h, self._stream(stream), C.byref(gbuf), C.byref(per_frame), C.byref(per_view), *_extra_point(extra_point), _byref(env), _byref(shadow),
                _ptr(out), out.shape[1], out_fmt)
        rc = self.lib.vqhip_forward_lighting(*args) if _targets is None else self.lib.vqhip_forward_lighting_mrt(*args, C.byref(_targets))
        self._ck(rc)
        return out

    def forward_lighting_msaa(self, layers, coverage, per_frame, per_view, background=None, out=None, out_fmt=FMT_RGBA16F, extra_point=None, env=None,
                              shadow=None, stream=None):
        """4x MSAA lit draw + resolve (vqhip_forward_lighting_msaa). layers: 1..4 G-buffers, each a tuple of 4 float32 cuda tensors [H,W,4];
        coverage: one uint8 cuda tensor [H,W] per layer (bit s = the layer's fragment covers sample s); background: None (clear value 0) or an
        out_fmt image [H,W,4] (e.g. the skydome). Returns the resolved image."""
        if not 1 <= len(layers) <= abi.MSAA_MAX_LAYERS or len(coverage) != len(layers):
            raise ValueError(f"forward_lighting_msaa: 1..{abi.MSAA_MAX_LAYERS} layers, one coverage plane each (got {len(layers)} and {len(coverage)})")
        h, w = layers[0][0].shape[0], layers[0][0].shape[1]
        g = abi.GBufferMSAA()
        g.layers, g.coverage_pitch = len(layers), w
        for k, (gb, cov) in enumerate(zip(layers, coverage)):
            for i, p in enumerate(gb):
                _check_img(p, FMT_RGBA32F, f"layer {k} gb{i}", (h, w))
            if not (cov.is_cuda and cov.is_contiguous() and cov.dtype == torch.uint8 and tuple(cov.shape) == (h, w)):
                raise ValueError(f"coverage {k}: expected contiguous cuda uint8 tensor of shape {(h, w)}, got {tuple(cov.shape)} {cov.dtype} {cov.device}")
            g.layer[k] = _gbuffer(gb, h, w)
            g.coverage[k] = cov.data_ptr()
        if background is not None:
            _check_img(background, out_fmt, "background", (h, w))
        out = _out_image(out, h, w, out_fmt, self.device)
        self._ck(self.lib.vqhip_forward_lighting_msaa(self._h, self._stream(stream), C.byref(g), C.byref(per_frame), C.byref(per_view), *_extra_point(extra_point),
                                                      _byref(env), _byref(shadow), _ptr(background), w, _ptr(out), w, out_fmt))
        return out

    # ---- 4x MSAA surface resolve + depth hierarchy (ResolveMSAA_DepthPrePass / DownsampleDepth, SceneRendering.cpp:484-499) ------
    def _hierarchy_views(self, flat, w, h):
        views, off = [], 0
        for (rows, cols) in abi.depth_hierarchy_shapes(w, h):
            views.append(flat[off:off + rows * cols].view(rows, cols))
            off += rows * cols
        return views

    def _hierarchy_buffer(self, w, h):
        if max(w, h) > abi.DEPTH_HIERARCHY_MAX_DIM:
            raise ValueError(f"depth hierarchy: frames above {abi.DEPTH_HIERARCHY_MAX_DIM} in either dimension are not supported (got {w} x {h})")
        return torch.empty((sum(r * c for r, c in abi.depth_hierarchy_shapes(w, h)),), dtype=torch.float32, device=self.device)

    def depth_hierarchy(self, depth, flags=0, stream=None):
        """vqhip_depth_hierarchy: depth float32 cuda [H,W] (rows may be strided: a column slice of a wider plane) -> the levels of the min-depth
        pyramid, level 0 first, as views of ONE flat tensor (views[0].storage). flags: abi.DEPTH_HIERARCHY_TRUE_TOP."""
        if not (depth.is_cuda and depth.dtype == torch.float32 and depth.dim() == 2 and depth.stride(1) == 1 and depth.stride(0) >= depth.shape[1]):
            raise ValueError(f"depth: expected cuda float32 [H,W] with unit column stride, got {tuple(depth.shape)} {depth.dtype} strides {depth.stride()}")
        h, w = depth.shape
        flat = self._hierarchy_buffer(w, h)
        self._ck(self.lib.vqhip_depth_hierarchy(self._h, self._stream(stream), _ptr(depth), depth.stride(0), w, h, _ptr(flat), int(flags)))
        return self._hierarchy_views(flat, w, h)

    # ---- FidelityFX CACAO (RenderAmbientOcclusion, SceneRendering.cpp:1503-1555) -----------------------------------------------------------
    def cacao(self, depth, normals, normal_fmt, shared, per_pass, quality=abi.CACAO_QUALITY_HIGH, blur_passes=2, work=None, out=None, stream=None):
        """vqhip_cacao: depth float32 cuda [H,W] (rows may be strided); normals int32 [H,W] (R10G10B10A2_UNORM words) or float32 [H,W,4], rows may be strided;
        shared / per_pass: abi.CacaoConstants and an array of four (vqengine_amd.cacao.constants). work: a cuda uint8 tensor of cacao_work_bytes bytes (allocated
        when None); out: uint8 [H,W], rows may be strided. Returns (ao, work): the R8_UNORM plane that forward lighting takes as texScreenSpaceAO, and the work
        buffer (cacao_work_planes views its intermediates)."""
        return self._cacao("cacao", cacao_work_bytes, self.lib.vqhip_cacao, depth, normals, normal_fmt, shared, per_pass, (int(quality), int(blur_passes)), work, out, stream)

    def adaptive_cacao(self, depth, normals, normal_fmt, shared, per_pass, blur_passes=2, work=None, out=None, stream=None):
        """vqhip_adaptive_cacao, quality HIGHEST: the arguments of cacao() without `quality`; shared / per_pass from vqengine_amd.cacao.constants with settings at
        HIGHEST (its defaults). work: a cuda uint8 tensor of adaptive_cacao_work_bytes bytes (allocated when None). Returns (ao, work); adaptive_cacao_work_planes
        views the intermediates, the importance map and the load counter included."""
        return self._cacao("adaptive_cacao", adaptive_cacao_work_bytes, self.lib.vqhip_adaptive_cacao, depth, normals, normal_fmt, shared, per_pass, (int(blur_passes),),
                           work, out, stream)

    def _cacao(self, who, work_bytes, call, depth, normals, normal_fmt, shared, per_pass, settings, work, out, stream):
        """both bindings; settings: what the entry point takes between per_pass and work"""
        if not (depth.is_cuda and depth.dtype == torch.float32 and depth.dim() == 2 and depth.stride(1) == 1):
            raise ValueError(f"{who}: depth: expected cuda float32 [H,W] with unit column stride, got {tuple(depth.shape)} {depth.dtype} strides {depth.stride()}")
        h, w = depth.shape
        if normal_fmt == abi.FMT_RGBA32F:
            ok = normals.dtype == torch.float32 and tuple(normals.shape) == (h, w, 4) and normals.stride(2) == 1 and normals.stride(1) == 4
        else:
            ok = normals.dtype == torch.int32 and tuple(normals.shape) == (h, w) and normals.stride(1) == 1
        if not (ok and normals.is_cuda):
            raise ValueError(f"{who}: normals: expected cuda int32 [H,W] (R10G10B10A2_UNORM words) or float32 [H,W,4] with dense pixels")
        if work is None:
            work = torch.empty((work_bytes(w, h),), dtype=torch.uint8, device=self.device)
        if not (work.is_cuda and work.dtype == torch.uint8 and work.is_contiguous()):
            raise ValueError(f"{who}: work: expected a contiguous cuda uint8 tensor")
        if out is None:
            out = torch.empty((h, w), dtype=torch.uint8, device=self.device)
        if not (out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (h, w) and out.stride(1) == 1):
            raise ValueError(f"{who}: out: expected cuda uint8 {(h, w)} with unit column stride")
        self._ck(call(self._h, self._stream(stream), _ptr(depth), depth.stride(0) * 4, _ptr(normals), normal_fmt, normals.stride(0) * normals.element_size(),
                      C.byref(shared), per_pass, *settings, _ptr(work), work.numel(), _ptr(out), out.stride(0), w, h))
        return out, work

    def shadow_depth(self, views, work=None, stream=None):
        """vqhip_shadow_depth: rasterise every ShadowView of `views` (at most 64) into its depth tensor, in one call. work: a cuda uint8 tensor of
        shadow_depth_work_bytes(total instanced triangles, len(views)) bytes (allocated when None). Returns work."""
        call, work = self.shadow_depth_prepared(views, work)
        call(stream)
        return work

    def shadow_depth_prepared(self, views, work=None):
        """The descriptors of a shadow_depth call built once: returns (call, work) with call(stream=None) issuing vqhip_shadow_depth on the same views again
        (a frame loop, a benchmark). The tensors of `views` must stay alive and in place."""
        return self._shadow_depth_prepared("shadow_depth", False, views, work)

    def shadow_masked_depth(self, views, work=None, stream=None):
        """vqhip_shadow_masked_depth: shadow_depth with alpha-tested draws. A draw that is a MaskedDraw with a `texture` (abi.Texture2D over a cuda RGBA8 mip chain;
        texels None = null SRV, which loses every fragment) is drawn through the "_AlphaMasked" shadow PSO; its positions are the engine's vertex (k >= 11).
        Any other draw is opaque. Returns work."""
        call, work = self.shadow_masked_depth_prepared(views, work)
        call(stream)
        return work

    def shadow_masked_depth_prepared(self, views, work=None):
        """shadow_depth_prepared for vqhip_shadow_masked_depth"""
        return self._shadow_depth_prepared("shadow_masked_depth", True, views, work)

    def _shadow_depth_prepared(self, who_, masked, views, work):
        views = list(views)
        if not 1 <= len(views) <= abi.SHADOW_MAX_VIEWS:
            raise ValueError(f"{who_}: expected 1..{abi.SHADOW_MAX_VIEWS} views, got {len(views)}")
        cviews = ((abi.ShadowMaskedView if masked else abi.ShadowView) * len(views))()
        masked_tris = num_draws = 0
        keep = []
        for i, v in enumerate(views):
            d = v.depth
            if not (d.is_cuda and d.dtype == torch.float32 and d.dim() == 2 and d.shape[0] == d.shape[1] and d.stride(1) == 1 and d.stride(0) >= d.shape[1]):
                raise ValueError(f"{who_}: view {i}: depth: expected cuda float32 [dim, dim] with unit column stride, got {tuple(d.shape)} {d.dtype} strides {d.stride()}")
            if not 1 <= d.shape[0] <= abi.SHADOW_MAX_DIM:
                raise ValueError(f"{who_}: view {i}: dim must be 1..{abi.SHADOW_MAX_DIM}")
            cdraws = ((abi.ShadowMaskedDraw if masked else abi.ShadowDraw) * max(1, len(v.draws)))()
            num_draws += len(v.draws)
            keep.append(cdraws)
            for j, dr in enumerate(v.draws):
                who = f"{who_}: view {i} draw {j}"
                p, ix = dr.positions, dr.indices
                _check_vertices(who, "positions", p, 3)
                bits = _check_indices(who, ix)
                n = _check_matrix_blocks(who, (("wvp", dr.wvp, False), ("world", dr.world, not v.linear)), ", n the same for wvp and world")
                _check_instances_cull(who, n, abi.SHADOW_MAX_INSTANCES, dr.cull)
                c = cdraws[j]
                if masked:
                    tex = getattr(dr, "texture", None)
                    if tex is not None:
                        if not isinstance(tex, abi.Texture2D):
                            raise ValueError(f"{who}: texture: expected abi.Texture2D or None")
                        if p.shape[1] < 11:
                            raise ValueError(f"{who}: a masked draw needs the engine's vertex, float32 [V, k >= 11] (uv at floats 9, 10)")
                        c.texDiffuseAlpha = C.pointer(tex)
                        keep.append(tex)
                        masked_tris += (ix.numel() // 3) * n
                    c = c.draw
                _fill_mesh(c, p, ix, bits)
                c.matWorldViewProj, c.matWorld = dr.wvp.data_ptr(), (dr.world.data_ptr() if dr.world is not None else None)
                c.numInstances, c.cullMode = n, dr.cull
            cv = cviews[i]
            cv.depth, cv.pitchBytes, cv.dim, cv.linearDepth = d.data_ptr(), d.stride(0) * 4, d.shape[0], int(v.linear)
            cv.cameraPosition = abi.float3(*[float(x) for x in v.camera])
            cv.farPlane, cv.numDraws = v.far, len(v.draws)
            cv.draws = C.cast(cdraws, C.POINTER(abi.ShadowMaskedDraw if masked else abi.ShadowDraw))
        tris = sum(v.instanced_triangles() for v in views)
        need = shadow_masked_depth_work_bytes(tris, masked_tris, len(views), num_draws) if masked else shadow_depth_work_bytes(tris, len(views))
        work = _work_tensor(who_, work, need, self.device)
        keep.append(views)

        def call(stream=None, _keep=keep):
            fn = self.lib.vqhip_shadow_masked_depth if masked else self.lib.vqhip_shadow_depth
            self._ck(fn(self._h, self._stream(stream), cviews, len(views), _ptr(work), work.numel()))
        return call, work

    def scene_depth(self, draws, width, height, samples=1, primitive=False, layers=0, layer_primitive=True, out=None, work=None, stream=None):
        """vqhip_scene_depth: rasterise the ShadowDraw list `draws` (world ignored; at most 64 instances each) as the main view's depth pre-pass into a
        width x height target of `samples` (1 | 4) samples. primitive: also return the owning primitive's sequence number per sample; layers (samples 4):
        the number of coverage-mask layers to return, with their primitives when layer_primitive. out: a dict of preallocated tensors under the keys of the
        result (their row strides are the pitches), else they are allocated dense. Returns a dict: depth float32 [H,W] | [H,W,4], primitive int32 of the same
        shape (the bits are uint32; -1 = no owner), coverage [layers] uint8 [H,W], layer_primitive [layers] int32 [H,W], work."""
        call, res = self.scene_depth_prepared(draws, width, height, samples, primitive, layers, layer_primitive, out, work)
        call(stream)
        return res

    def scene_depth_prepared(self, draws, width, height, samples=1, primitive=False, layers=0, layer_primitive=True, out=None, work=None):
        """The descriptors of a scene_depth call built once: returns (call, result) with call(stream=None) issuing vqhip_scene_depth on the same draws and
        targets again. The tensors must stay alive and in place."""
        return self._scene_depth_prepared("scene_depth", False, draws, width, height, samples, primitive, layers, layer_primitive, out, work)

    def scene_masked_depth(self, draws, width, height, samples=1, primitive=False, layers=0, layer_primitive=True, out=None, work=None, stream=None):
        """vqhip_scene_masked_depth: scene_depth with alpha-tested draws. A draw that is a MaskedDraw with a `material` (abi.MaterialDesc, host; its texDiffuse over
        a cuda RGBA8 mip chain) whose texDiffuse.reserved has abi.MATERIAL_ALPHA_MASKED is drawn through the "_AlphaMasked" pre-pass PSO; its positions are the
        engine's vertex (k >= 11). Any other draw is opaque. Same arguments and result as scene_depth."""
        call, res = self.scene_masked_depth_prepared(draws, width, height, samples, primitive, layers, layer_primitive, out, work)
        call(stream)
        return res

    def scene_masked_depth_prepared(self, draws, width, height, samples=1, primitive=False, layers=0, layer_primitive=True, out=None, work=None):
        """scene_depth_prepared for vqhip_scene_masked_depth"""
        return self._scene_depth_prepared("scene_masked_depth", True, draws, width, height, samples, primitive, layers, layer_primitive, out, work)

    def _scene_depth_prepared(self, who_, masked, draws, width, height, samples, primitive, layers, layer_primitive, out, work):
        draws, out = list(draws), dict(out or {})
        w, h = int(width), int(height)
        if samples not in (1, 4):
            raise ValueError(f"{who_}: samples: expected 1 or 4, got {samples}")
        if not 0 <= layers <= abi.SCENE_DEPTH_MAX_LAYERS or (samples == 1 and layers):
            raise ValueError(f"{who_}: layers: expected 0..4, and 0 at samples 1")
        if not (1 <= w <= abi.SCENE_DEPTH_MAX_DIM and 1 <= h <= abi.SCENE_DEPTH_MAX_DIM):
            raise ValueError(f"{who_}: width and height must be 1..{abi.SCENE_DEPTH_MAX_DIM}")
        shape = (h, w) if samples == 1 else (h, w, 4)

        def plane(key, dtype, shp, t):
            if t is None:
                t = torch.empty(shp, dtype=dtype, device=self.device)
            px = 1 if len(shp) == 2 else shp[2]
            if not (t.is_cuda and t.dtype == dtype and tuple(t.shape) == tuple(shp) and t.stride(-1) == 1 and (len(shp) == 2 or t.stride(1) == px)
                    and t.stride(0) % px == 0 and t.stride(0) >= w * px):
                raise ValueError(f"{who_}: {key}: expected cuda {dtype} {tuple(shp)} with dense pixels, got {tuple(t.shape)} {t.dtype} strides {t.stride()}")
            return t, t.stride(0) // px
        res, pitches, cov_pitches = {}, set(), set()
        res["depth"], p = plane("depth", torch.float32, shape, out.get("depth"))
        pitches.add(p)
        if primitive:
            res["primitive"], p = plane("primitive", torch.int32, shape, out.get("primitive"))
            pitches.add(p)
        if layers:
            given = list(out.get("coverage") or [None] * layers)
            res["coverage"] = []
            for k in range(layers):
                t, p = plane("coverage", torch.uint8, (h, w), given[k])
                res["coverage"].append(t)
                cov_pitches.add(p)
            if layer_primitive:
                given = list(out.get("layer_primitive") or [None] * layers)
                res["layer_primitive"] = []
                for k in range(layers):
                    t, p = plane("layer_primitive", torch.int32, (h, w), given[k])
                    res["layer_primitive"].append(t)
                    pitches.add(p)
        if len(pitches) != 1 or len(cov_pitches) > 1:
            raise ValueError(f"{who_}: depth, primitive and layer_primitive share one pitch in pixels, the coverage planes one pitch in bytes")
        cdraws = ((abi.SceneDepthMaskedDraw if masked else abi.SceneDepthDraw) * max(1, len(draws)))()
        tris = masked_tris = 0
        keep_mats = []
        for j, dr in enumerate(draws):
            who = f"{who_}: draw {j}"
            p, ix = dr.positions, dr.indices
            _check_vertices(who, "positions", p, 3)
            bits = _check_indices(who, ix)
            n = _check_matrix_blocks(who, (("wvp", dr.wvp, False),))
            _check_instances_cull(who, n, abi.SCENE_DEPTH_MAX_INSTANCES, dr.cull)
            c = cdraws[j]
            if masked:
                mat = getattr(dr, "material", None)
                if mat is not None:
                    if not isinstance(mat, abi.MaterialDesc):
                        raise ValueError(f"{who}: material: expected abi.MaterialDesc or None")
                    c.material = C.pointer(mat)
                    keep_mats.append(mat)
                    if mat.texDiffuse.reserved & abi.MATERIAL_ALPHA_MASKED:
                        if p.shape[1] < 11:
                            raise ValueError(f"{who}: a masked draw needs the engine's vertex, float32 [V, k >= 11] (uv at floats 9, 10)")
                        masked_tris += (ix.numel() // 3) * n
                c = c.draw
            _fill_mesh(c, p, ix, bits)
            c.matWorldViewProj, c.numInstances, c.cullMode = dr.wvp.data_ptr(), n, dr.cull
            tris += (ix.numel() // 3) * n
        need = scene_masked_depth_work_bytes(tris, masked_tris, len(draws)) if masked else scene_depth_work_bytes(tris)
        res["work"] = work = _work_tensor(who_, work, need, self.device, " (0: too many triangles)")
        tg = abi.SceneDepthTargets()
        tg.depth = res["depth"].data_ptr()
        tg.primitive = res["primitive"].data_ptr() if primitive else None
        for k in range(layers):
            tg.coverage[k] = res["coverage"][k].data_ptr()
            tg.layerPrimitive[k] = res["layer_primitive"][k].data_ptr() if layer_primitive else None
        tg.layers, tg.pitch, tg.coverage_pitch = layers, pitches.pop(), (cov_pitches.pop() if cov_pitches else 0)
        keep = (draws, res, keep_mats)

        def call(stream=None, _keep=keep):
            fn = self.lib.vqhip_scene_masked_depth if masked else self.lib.vqhip_scene_depth
            self._ck(fn(self._h, self._stream(stream), cdraws, len(draws), w, h, samples, C.byref(tg), _ptr(work), work.numel()))
        return call, res

    def scene_interpolants(self, draws, width, height, owner, sv=False, out=None, work=None, stream=None):
        """vqhip_scene_interpolants: the lit draw's PSInput planes of the SurfaceDraw list `draws` (the draw list of the scene_depth call that wrote `owner`, in
        the same order) under the owner plane `owner`: cuda int32 [H, W] with unit column stride — scene_depth's `primitive` at 1x, one `layer_primitive[k]` at
        4x. sv: also the svPositionCurr / svPositionPrev planes of psmain targets. out: a dict of preallocated cuda float32 [H, W, 4] tensors under the keys of
        the result (their row strides are the pitches), else they are allocated dense. Returns a dict: ip0, ip1, ip2, with sv also sv_curr and sv_prev, work."""
        call, res = self.scene_interpolants_prepared(draws, width, height, owner, sv, out, work)
        call(stream)
        return res

    def scene_interpolants_prepared(self, draws, width, height, owner, sv=False, out=None, work=None):
        """The descriptors of a scene_interpolants call built once: returns (call, result) with call(stream=None) issuing vqhip_scene_interpolants on the same
        draws, owner plane and targets again. The tensors must stay alive and in place."""
        return self._scene_interpolants_prepared("scene_interpolants", False, draws, width, height, owner, sv, out, work)

    def scene_quad_interpolants(self, draws, width, height, owner, sv=False, out=None, work=None, stream=None):
        """vqhip_scene_quad_interpolants (docs/DESIGN_DETAILS.md §7.20): scene_interpolants plus the plane `quad_uv`, cuda float32 [H, W, 4] = the owner primitive's
        vertex uv at the helper lanes (i ^ 1, j) and (i, j ^ 1), for the _quad producers. out may hold a preallocated `quad_uv` (its row stride is its pitch)."""
        call, res = self.scene_quad_interpolants_prepared(draws, width, height, owner, sv, out, work)
        call(stream)
        return res

    def scene_quad_interpolants_prepared(self, draws, width, height, owner, sv=False, out=None, work=None):
        """scene_interpolants_prepared for vqhip_scene_quad_interpolants"""
        return self._scene_interpolants_prepared("scene_quad_interpolants", True, draws, width, height, owner, sv, out, work)

    def _scene_interpolants_prepared(self, who_, quad, draws, width, height, owner, sv, out, work):
        draws, out = list(draws), dict(out or {})
        w, h = int(width), int(height)
        if not (1 <= w <= abi.SCENE_DEPTH_MAX_DIM and 1 <= h <= abi.SCENE_DEPTH_MAX_DIM):
            raise ValueError(f"{who_}: width and height must be 1..{abi.SCENE_DEPTH_MAX_DIM}")
        if not (owner.is_cuda and owner.dtype == torch.int32 and tuple(owner.shape) == (h, w) and owner.stride(1) == 1 and owner.stride(0) >= w):
            raise ValueError(f"{who_}: owner: expected cuda int32 {(h, w)} with unit column stride, got {tuple(owner.shape)} {owner.dtype} strides {owner.stride()}")
        res, pitches = {}, {}
        for key in ("ip0", "ip1", "ip2") + (("sv_curr", "sv_prev") if sv else ()) + (("quad_uv",) if quad else ()):
            t = out.get(key)
            if t is None:
                t = torch.empty((h, w, 4), dtype=torch.float32, device=self.device)
            if not (t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (h, w, 4) and t.stride(2) == 1 and t.stride(1) == 4 and t.stride(0) % 4 == 0
                    and t.stride(0) >= 4 * w):
                raise ValueError(f"{who_}: {key}: expected cuda float32 {(h, w, 4)} with dense pixels, got {tuple(t.shape)} {t.dtype} strides {t.stride()}")
            res[key] = t
            pitches.setdefault(key[:2], set()).add(t.stride(0) // 4)
        if any(len(p) != 1 for p in pitches.values()):
            raise ValueError(f"{who_}: ip0, ip1 and ip2 share one pitch in pixels, sv_curr and sv_prev another")
        cdraws = (abi.SceneSurfaceDraw * max(1, len(draws)))()
        for j, dr in enumerate(draws):
            who = f"{who_}: draw {j}"
            p, ix = dr.vertices, dr.indices
            _check_vertices(who, "vertices", p, 11)
            bits = _check_indices(who, ix)
            n = _check_matrix_blocks(who, (("wvp", dr.wvp, False), ("world", dr.world, False), ("normal", dr.normal, False), ("wvp_prev", dr.wvp_prev, not sv)),
                                     ", n the same for every matrix block")
            _check_instances_cull(who, n, abi.SCENE_DEPTH_MAX_INSTANCES)
            if dr.material < 0:
                raise ValueError(f"{who}: material: expected an index >= 0")
            c = cdraws[j]
            # an empty tensor has no address, and the library refuses a NULL index buffer whatever its length: an empty draw names the vertex buffer (never read)
            _fill_mesh(c, p, ix, bits, empty_indices=p.data_ptr())
            c.matWorldViewProj, c.matWorld, c.matNormal = dr.wvp.data_ptr(), dr.world.data_ptr(), dr.normal.data_ptr()
            c.matWorldViewProjPrev = dr.wvp_prev.data_ptr() if dr.wvp_prev is not None else None
            c.numInstances, c.materialIndex = n, dr.material
        res["work"] = work = _work_tensor(who_, work, scene_interpolants_work_bytes(len(draws)), self.device)
        tg = abi.SceneInterpolantTargets()
        tg.ip0, tg.ip1, tg.ip2 = res["ip0"].data_ptr(), res["ip1"].data_ptr(), res["ip2"].data_ptr()
        tg.pitch = pitches["ip"].pop()
        if sv:
            tg.svPositionCurr, tg.svPositionPrev, tg.sv_pitch = res["sv_curr"].data_ptr(), res["sv_prev"].data_ptr(), pitches["sv"].pop()
        keep = (draws, res, owner)
        fn, arg = self.lib.vqhip_scene_interpolants, tg
        if quad:
            arg = abi.SceneQuadTargets()
            arg.planes, arg.quadUV, arg.quad_pitch = tg, res["quad_uv"].data_ptr(), pitches["qu"].pop()
            fn = self.lib.vqhip_scene_quad_interpolants

        def call(stream=None, _keep=keep):
            self._ck(fn(self._h, self._stream(stream), cdraws, len(draws), w, h, _ptr(owner), owner.stride(0), C.byref(arg), _ptr(work), work.numel()))
        return call, res

    def object_ids(self, draws, width, height, owner, out=None, work=None, stream=None):
        """vqhip_object_ids: the ObjectID pass's target of the ObjectIdDraw list `draws` (the draw list of the cull-NONE scene_depth call that wrote `owner`, in the
        same order) under the owner plane `owner`: cuda int32 [H, W] with unit column stride — scene_depth's `primitive` at 1 sample. out: a preallocated cuda
        int32 [H, W, 4] with dense pixels (its row stride is the pitch), else allocated dense. Returns a dict: ids, work."""
        call, res = self.object_ids_prepared(draws, width, height, owner, out, work)
        call(stream)
        return res

    def object_ids_prepared(self, draws, width, height, owner, out=None, work=None):
        """The descriptors of an object_ids call built once: returns (call, result) with call(stream=None) issuing vqhip_object_ids on the same draws, owner plane
        and target again. The tensors must stay alive and in place."""
        who_ = "object_ids"
        draws = list(draws)
        w, h = int(width), int(height)
        if not (1 <= w <= abi.SCENE_DEPTH_MAX_DIM and 1 <= h <= abi.SCENE_DEPTH_MAX_DIM):
            raise ValueError(f"{who_}: width and height must be 1..{abi.SCENE_DEPTH_MAX_DIM}")
        if not (owner.is_cuda and owner.dtype == torch.int32 and tuple(owner.shape) == (h, w) and owner.stride(1) == 1 and owner.stride(0) >= w):
            raise ValueError(f"{who_}: owner: expected cuda int32 {(h, w)} with unit column stride, got {tuple(owner.shape)} {owner.dtype} strides {owner.stride()}")
        ids = out if out is not None else torch.empty((h, w, 4), dtype=torch.int32, device=self.device)
        if not (ids.is_cuda and ids.dtype == torch.int32 and tuple(ids.shape) == (h, w, 4) and ids.stride(2) == 1 and ids.stride(1) == 4 and ids.stride(0) % 4 == 0
                and ids.stride(0) >= 4 * w):
            raise ValueError(f"{who_}: out: expected cuda int32 {(h, w, 4)} with dense pixels, got {tuple(ids.shape)} {ids.dtype} strides {ids.stride()}")
        cdraws = (abi.ObjectIdDraw * max(1, len(draws)))()
        for j, dr in enumerate(draws):
            who = f"{who_}: draw {j}"
            o = dr.obj_id
            if not (o.is_cuda and o.dtype == torch.int32 and o.dim() == 2 and o.shape[1] == 4 and o.is_contiguous()):
                raise ValueError(f"{who}: obj_id: expected cuda int32 [n, 4] contiguous")
            _check_instances_cull(who, o.shape[0], abi.SCENE_DEPTH_MAX_INSTANCES)
            if dr.num_indices < 0 or dr.num_indices % 3:
                raise ValueError(f"{who}: num_indices: expected a multiple of 3")
            c = cdraws[j]
            c.numIndices, c.numInstances, c.objID, c.meshID, c.materialID = dr.num_indices, o.shape[0], o.data_ptr(), dr.mesh_id, dr.material_id
        work = _work_tensor(who_, work, object_ids_work_bytes(len(draws)), self.device)
        res = {"ids": ids, "work": work}
        keep = (draws, res, owner)

        def call(stream=None, _keep=keep):
            self._ck(self.lib.vqhip_object_ids(self._h, self._stream(stream), cdraws, len(draws), w, h, _ptr(owner), owner.stride(0), _ptr(ids), ids.stride(0) // 4,
                                               _ptr(work), work.numel()))
        return call, res

    def displace_meshes(self, jobs, stream=None):
        """vqhip_displace_meshes: the heightmap-displaced copies of the vertex streams of the DisplaceJob list `jobs`, all in one call. Returns the list of output
        tensors, one per job: float32 [V, 3] for a compact job, else float32 [V, k] with the input's row stride (every float of the row is copied)."""
        call, outs = self.displace_meshes_prepared(jobs)
        call(stream)
        return outs

    def displace_meshes_prepared(self, jobs):
        """The descriptors of a displace_meshes call built once: returns (call, outputs) with call(stream=None) issuing vqhip_displace_meshes on the same jobs
        again. The tensors must stay alive and in place."""
        who_ = "displace_meshes"
        jobs = list(jobs)
        cjobs = (abi.DisplaceJob * max(1, len(jobs)))()
        outs = []
        for j, jb in enumerate(jobs):
            who = f"{who_}: job {j}"
            p = jb.vertices
            if p.dim() == 2 and p.shape[0] == 0 and p.is_cuda and p.dtype == torch.float32 and p.shape[1] >= 11:
                p = p.new_empty((0, p.shape[1]))             # no vertices: whatever strides the empty tensor came with, the job reads nothing
            _check_vertices(who, "vertices", p, 11)
            if len(jb.uv_scale_offset) != 4:
                raise ValueError(f"{who}: uv_scale_offset: expected 4 floats")
            if jb.heightmap is not None and not isinstance(jb.heightmap, abi.Texture2D):
                raise ValueError(f"{who}: heightmap: expected abi.Texture2D or None")
            n, stride = p.shape[0], p.stride(0)
            o = jb.out
            if o is None:
                o = torch.empty((n, 3), dtype=torch.float32, device=self.device) if jb.compact else \
                    torch.empty((n, stride), dtype=torch.float32, device=self.device)[:, :p.shape[1]]
            ok = o.is_cuda and o.dtype == torch.float32 and o.dim() == 2 and o.shape[0] == n and o.stride(1) == 1
            if not (ok and ((o.shape[1] == 3 and o.stride(0) == 3) if jb.compact else o.stride(0) == stride)):
                raise ValueError(f"{who}: out: expected cuda float32 " + ("[V, 3] contiguous" if jb.compact else "[V, k] with the row stride of vertices"))
            c = cjobs[j]
            c.vertices, c.strideBytes, c.numVertices = p.data_ptr() or None, stride * 4, n
            c.out, c.outStrideBytes, c.reserved = o.data_ptr() or None, abi.DISPLACE_POSITION_BYTES if jb.compact else stride * 4, 0
            if jb.heightmap is not None:
                c.heightmap = jb.heightmap
            c.uvScaleOffset = abi.float4(*jb.uv_scale_offset)
            c.displacement = jb.displacement
            outs.append(o)
        keep = (jobs, outs)

        def call(stream=None, _keep=keep):
            self._ck(self.lib.vqhip_displace_meshes(self._h, self._stream(stream), cjobs, len(jobs)))
        return call, outs

    def outline(self, draws, width, height, scene_color, selection=True, writer=True, out=None, work=None, stream=None):
        """vqhip_outline: both passes of the Outline pass over the OutlineDraw list `draws`, writing the outline's colour IN PLACE into `scene_color`: cuda
        float16 [H, W, 4] with dense pixels (its row stride is the pitch). selection / writer: also return the stencil mark (uint8 [H, W]) and the index of the
        draw whose colour each pixel received (int32 [H, W]; the bits are uint32, -1 = not written). out: a dict of preallocated `selection` / `writer` tensors
        (their row strides are the pitches). Returns a dict: scene_color, selection, writer (where asked for), work."""
        call, res = self.outline_prepared(draws, width, height, scene_color, selection, writer, out, work)
        call(stream)
        return res

    def outline_prepared(self, draws, width, height, scene_color, selection=True, writer=True, out=None, work=None):
        """The descriptors of an outline call built once: returns (call, result) with call(stream=None) issuing vqhip_outline on the same draws and targets again.
        The tensors must stay alive and in place."""
        who_ = "outline"
        draws, out = list(draws), dict(out or {})
        w, h = int(width), int(height)
        if not (1 <= w <= abi.SCENE_DEPTH_MAX_DIM and 1 <= h <= abi.SCENE_DEPTH_MAX_DIM):
            raise ValueError(f"{who_}: width and height must be 1..{abi.SCENE_DEPTH_MAX_DIM}")
        sc = scene_color
        if not (sc.is_cuda and sc.dtype == torch.float16 and tuple(sc.shape) == (h, w, 4) and sc.stride(2) == 1 and sc.stride(1) == 4 and sc.stride(0) % 4 == 0
                and sc.stride(0) >= 4 * w):
            raise ValueError(f"{who_}: scene_color: expected cuda float16 {(h, w, 4)} with dense pixels, got {tuple(sc.shape)} {sc.dtype} strides {sc.stride()}")
        res = {"scene_color": sc}
        for key, want, dtype in (("selection", selection, torch.uint8), ("writer", writer, torch.int32)):
            if not want:
                continue
            t = out.get(key)
            if t is None:
                t = torch.empty((h, w), dtype=dtype, device=self.device)
            if not (t.is_cuda and t.dtype == dtype and tuple(t.shape) == (h, w) and t.stride(1) == 1 and t.stride(0) >= w):
                raise ValueError(f"{who_}: {key}: expected cuda {dtype} {(h, w)} with unit column stride, got {tuple(t.shape)} {t.dtype} strides {t.stride()}")
            res[key] = t
        cdraws = (abi.OutlineDraw * max(1, len(draws)))()
        tris = 0
        for j, dr in enumerate(draws):
            who = f"{who_}: draw {j}"
            p, ix, cb = dr.vertices, dr.indices, dr.cb
            _check_vertices(who, "vertices", p, 6)
            bits = _check_indices(who, ix)
            if not (cb.is_cuda and cb.is_contiguous() and cb.numel() * cb.element_size() == abi.OUTLINE_DATA_BYTES):
                raise ValueError(f"{who}: cb: expected a contiguous cuda tensor of {abi.OUTLINE_DATA_BYTES} bytes (one VQ_OutlineData)")
            c = cdraws[j]
            _fill_mesh(c, p, ix, bits, empty_indices=p.data_ptr())
            c.cb = cb.data_ptr()
            tris += ix.numel() // 3
        res["work"] = work = _work_tensor(who_, work, outline_work_bytes(tris), self.device, " (0: too many triangles)")
        tg = abi.OutlineTargets()
        tg.sceneColor, tg.pitch = sc.data_ptr(), sc.stride(0) // 4
        if selection:
            tg.selection, tg.selection_pitch = res["selection"].data_ptr(), res["selection"].stride(0)
        if writer:
            tg.writer, tg.writer_pitch = res["writer"].data_ptr(), res["writer"].stride(0)
        keep = (draws, res)

        def call(stream=None, _keep=keep):
            self._ck(self.lib.vqhip_outline(self._h, self._stream(stream), cdraws, len(draws), w, h, C.byref(tg), _ptr(work), work.numel()))
        return call, res

    def unlit_draws(self, draws, width, height, scene_color, scene_depth, blend=False, writer=True, out=None, work=None, stream=None):
        """vqhip_unlit_draws: the UnlitDraw list `draws` in submission order, depth-tested (LESS, no writes) against `scene_depth` (cuda float32 [H, W] with unit
        column stride) and written IN PLACE into `scene_color`: cuda float16 [H, W, 4] with dense pixels (its row stride is the pitch). blend: UNLIT_BLEND_PSO's
        SRC_ALPHA / INV_SRC_ALPHA fold instead of UNLIT_PSO's overwrite. writer: also return the index of the draw of each pixel's last passing fragment (int32
        [H, W]; the bits are uint32, -1 = none). out: a dict with a preallocated `writer` tensor (its row stride is the pitch). Returns a dict: scene_color, writer
        (where asked for), work."""
        call, res = self.unlit_draws_prepared(draws, width, height, scene_color, scene_depth, blend, writer, out, work)
        call(stream)
        return res

    def unlit_draws_prepared(self, draws, width, height, scene_color, scene_depth, blend=False, writer=True, out=None, work=None):
        """The descriptors of an unlit-draws call built once: returns (call, result) with call(stream=None) issuing vqhip_unlit_draws on the same draws and targets
        again. The tensors must stay alive and in place."""
        who_ = "unlit_draws"
        draws, out = list(draws), dict(out or {})
        w, h = int(width), int(height)
        if not (1 <= w <= abi.SCENE_DEPTH_MAX_DIM and 1 <= h <= abi.SCENE_DEPTH_MAX_DIM):
            raise ValueError(f"{who_}: width and height must be 1..{abi.SCENE_DEPTH_MAX_DIM}")
        sc, zd = scene_color, scene_depth
        if not (sc.is_cuda and sc.dtype == torch.float16 and tuple(sc.shape) == (h, w, 4) and sc.stride(2) == 1 and sc.stride(1) == 4 and sc.stride(0) % 4 == 0
                and sc.stride(0) >= 4 * w):
            raise ValueError(f"{who_}: scene_color: expected cuda float16 {(h, w, 4)} with dense pixels, got {tuple(sc.shape)} {sc.dtype} strides {sc.stride()}")
        if not (zd.is_cuda and zd.dtype == torch.float32 and tuple(zd.shape) == (h, w) and zd.stride(1) == 1 and zd.stride(0) >= w):
            raise ValueError(f"{who_}: scene_depth: expected cuda float32 {(h, w)} with unit column stride, got {tuple(zd.shape)} {zd.dtype} strides {zd.stride()}")
        res = {"scene_color": sc}
        if writer:
            t = out.get("writer")
            if t is None:
                t = torch.empty((h, w), dtype=torch.int32, device=self.device)
            if not (t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == (h, w) and t.stride(1) == 1 and t.stride(0) >= w):
                raise ValueError(f"{who_}: writer: expected cuda int32 {(h, w)} with unit column stride, got {tuple(t.shape)} {t.dtype} strides {t.stride()}")
            res["writer"] = t
        cdraws = (abi.UnlitDraw * max(1, len(draws)))()
        tris = 0
        for j, dr in enumerate(draws):
            who = f"{who_}: draw {j}"
            p, ix, cb = dr.positions, dr.indices, dr.cb
            _check_vertices(who, "positions", p, 3)
            bits = _check_indices(who, ix)
            if not (cb.is_cuda and cb.is_contiguous() and cb.numel() * cb.element_size() == abi.UNLIT_DATA_BYTES):
                raise ValueError(f"{who}: cb: expected a contiguous cuda tensor of {abi.UNLIT_DATA_BYTES} bytes (one VQ_UnlitData)")
            if dr.cull not in (abi.CULL_NONE, abi.CULL_FRONT, abi.CULL_BACK):
                raise ValueError(f"{who}: cull: expected abi.CULL_NONE, CULL_FRONT or CULL_BACK")
            c = cdraws[j]
            _fill_mesh(c, p, ix, bits, empty_indices=p.data_ptr())
            c.cb, c.cullMode = cb.data_ptr(), dr.cull
            tris += ix.numel() // 3
        res["work"] = work = _work_tensor(who_, work, unlit_draws_work_bytes(tris), self.device, " (0: too many triangles)")
        tg = abi.UnlitTargets()
        tg.sceneColor, tg.pitch = sc.data_ptr(), sc.stride(0) // 4
        tg.sceneDepth, tg.depth_pitch = zd.data_ptr(), zd.stride(0)
        if writer:
            tg.writer, tg.writer_pitch = res["writer"].data_ptr(), res["writer"].stride(0)
        keep = (draws, res, zd)
        mode = 1 if blend else 0

        def call(stream=None, _keep=keep):
            self._ck(self.lib.vqhip_unlit_draws(self._h, self._stream(stream), cdraws, len(draws), w, h, mode, C.byref(tg), _ptr(work), work.numel()))
        return call, res

    def line_draws(self, draws, width, height, scene_color, scene_depth, writer=True, out=None, work=None, stream=None):
        """vqhip_line_draws: the WireframeDraw / VertexAxesDraw list `draws` in submission order as aliased lines, depth-tested (LESS, no writes) against
        `scene_depth` (cuda float32 [H, W] with unit column stride) and written IN PLACE, without blending, into `scene_color`: cuda float16 [H, W, 4] with dense
        pixels (its row stride is the pitch). writer: also return the index of the draw of each pixel's winning fragment (int32 [H, W]; the bits are uint32,
        -1 = none). out: a dict with a preallocated `writer` tensor. Returns a dict: scene_color, writer (where asked for), work."""
        call, res = self.line_draws_prepared(draws, width, height, scene_color, scene_depth, writer, out, work)
        call(stream)
        return res

    def line_draws_prepared(self, draws, width, height, scene_color, scene_depth, writer=True, out=None, work=None):
        """The descriptors of a line-draws call built once: returns (call, result) with call(stream=None) issuing vqhip_line_draws on the same draws and targets
        again. The tensors must stay alive and in place."""
        who_ = "line_draws"
        draws, out = list(draws), dict(out or {})
        w, h = int(width), int(height)
        if not (1 <= w <= abi.SCENE_DEPTH_MAX_DIM and 1 <= h <= abi.SCENE_DEPTH_MAX_DIM):
            raise ValueError(f"{who_}: width and height must be 1..{abi.SCENE_DEPTH_MAX_DIM}")
        sc, zd = scene_color, scene_depth
        if not (sc.is_cuda and sc.dtype == torch.float16 and tuple(sc.shape) == (h, w, 4) and sc.stride(2) == 1 and sc.stride(1) == 4 and sc.stride(0) % 4 == 0
                and sc.stride(0) >= 4 * w):
            raise ValueError(f"{who_}: scene_color: expected cuda float16 {(h, w, 4)} with dense pixels, got {tuple(sc.shape)} {sc.dtype} strides {sc.stride()}")
        if not (zd.is_cuda and zd.dtype == torch.float32 and tuple(zd.shape) == (h, w) and zd.stride(1) == 1 and zd.stride(0) >= w):
            raise ValueError(f"{who_}: scene_depth: expected cuda float32 {(h, w)} with unit column stride, got {tuple(zd.shape)} {zd.dtype} strides {zd.stride()}")
        res = {"scene_color": sc}
        if writer:
            t = out.get("writer")
            if t is None:
                t = torch.empty((h, w), dtype=torch.int32, device=self.device)
            if not (t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == (h, w) and t.stride(1) == 1 and t.stride(0) >= w):
                raise ValueError(f"{who_}: writer: expected cuda int32 {(h, w)} with unit column stride, got {tuple(t.shape)} {t.dtype} strides {t.stride()}")
            res["writer"] = t
        cdraws = (abi.LineDraw * max(1, len(draws)))()
        lines = 0
        for j, dr in enumerate(draws):
            who = f"{who_}: draw {j}"
            c = cdraws[j]
            if getattr(dr, "kind", None) == abi.LINES_WIREFRAME:
                p, ix = dr.positions, dr.indices
                _check_vertices(who, "positions", p, 3)
                bits = _check_indices(who, ix)
                n = _check_matrix_blocks(who, (("matrices", dr.matrices, False),))
                _check_instances_cull(who, n, abi.LINES_MAX_INSTANCES)
                col = dr.color
                if not (col.is_cuda and col.dtype == torch.float32 and col.numel() == 4 and col.is_contiguous()):
                    raise ValueError(f"{who}: color: expected cuda float32 [4] contiguous")
                c.matModelViewProj, c.color, c.numInstances = dr.matrices.data_ptr(), col.data_ptr(), n
                lines += ix.numel() * n
            elif getattr(dr, "kind", None) == abi.LINES_VERTEX_AXES:
                p, ix, cb = dr.vertices, dr.indices, dr.cb
                _check_vertices(who, "vertices", p, 9)
                bits = {2: 16, 4: 32}.get(ix.element_size()) if not ix.dtype.is_floating_point else None
                if not (ix.is_cuda and ix.dim() == 1 and ix.is_contiguous() and bits):
                    raise ValueError(f"{who}: indices: expected a contiguous cuda 1-D 16-bit or 32-bit integer tensor")
                if not (cb.is_cuda and cb.is_contiguous() and cb.numel() * cb.element_size() == abi.VERTEX_AXES_DATA_BYTES):
                    raise ValueError(f"{who}: cb: expected a contiguous cuda tensor of {abi.VERTEX_AXES_DATA_BYTES} bytes (one VQ_VertexAxesData)")
                c.axes, c.numInstances = cb.data_ptr(), 1
                lines += 3 * ix.numel()
            else:
                raise ValueError(f"{who}: expected a WireframeDraw or a VertexAxesDraw")
            _fill_mesh(c, p, ix, bits, empty_indices=p.data_ptr())
            c.kind = dr.kind
        res["work"] = work = _work_tensor(who_, work, line_draws_work_bytes(lines), self.device, " (0: too many lines)")
        tg = abi.UnlitTargets()
        tg.sceneColor, tg.pitch = sc.data_ptr(), sc.stride(0) // 4
        tg.sceneDepth, tg.depth_pitch = zd.data_ptr(), zd.stride(0)
        if writer:
            tg.writer, tg.writer_pitch = res["writer"].data_ptr(), res["writer"].stride(0)
        keep = (draws, res, zd)

        def call(stream=None, _keep=keep):
            self._ck(self.lib.vqhip_line_draws(self._h, self._stream(stream), cdraws, len(draws), w, h, C.byref(tg), _ptr(work), work.numel()))
        return call, res

    def msaa_resolve_surfaces(self, depth_ms, coverage=None, normals=None, normals_fmt=abi.FMT_R10G10B10A2_UNORM, roughness=None, background=None,
                              out_depth=False, out_normals_fmt=None, scene_color=None, scene_fmt=FMT_RGBA16F, hierarchy=False, flags=0, stream=None):
        """vqhip_msaa_resolve_surfaces (DepthResolve.hlsl). depth_ms: float32 cuda [H,W,4] (sample s at [..., s]); coverage: one uint8 [H,W] plane per
        layer; normals: one plane per layer, int32 [H,W] (R10G10B10A2_UNORM words) or float32 [H,W,4]; roughness: one gb1 plane (float32 [H,W,4]) per layer;
        background: the scene colour's background plane (scene_fmt) or None. Outputs — out_depth: True -> float32 [H,W]; out_normals_fmt: a format -> the
        resolved normals in it; scene_color: an image of scene_fmt whose alpha is rewritten IN PLACE; hierarchy: True -> the fused depth hierarchy (list of
        level views, `flags` as depth_hierarchy). Returns a dict with the keys of the outputs asked for."""
        if not (depth_ms.is_cuda and depth_ms.is_contiguous() and depth_ms.dtype == torch.float32 and depth_ms.dim() == 3 and depth_ms.shape[2] == 4):
            raise ValueError(f"depth_ms: expected contiguous cuda float32 [H,W,4], got {tuple(depth_ms.shape)} {depth_ms.dtype}")
        h, w = depth_ms.shape[0], depth_ms.shape[1]
        want_n, want_r = out_normals_fmt is not None, scene_color is not None
        if not (out_depth or want_n or want_r or hierarchy):
            raise ValueError("msaa_resolve_surfaces: at least one output is required")
        s = abi.MSAASurfaces()
        s.depth_ms, s.width, s.height, s.depth_pitch_px, s.coverage_pitch, s.normals_fmt = depth_ms.data_ptr(), w, h, w, w, normals_fmt
        nl = len(coverage) if coverage is not None else 1
        if not 1 <= nl <= abi.MSAA_MAX_LAYERS:
            raise ValueError(f"msaa_resolve_surfaces: 1..{abi.MSAA_MAX_LAYERS} layers (got {nl})")
        s.layers = nl
        if want_n or want_r:
            if coverage is None:
                raise ValueError("msaa_resolve_surfaces: the normals / roughness outputs need the coverage planes")
            for k, cov in enumerate(coverage):
                if not (cov.is_cuda and cov.is_contiguous() and cov.dtype == torch.uint8 and tuple(cov.shape) == (h, w)):
                    raise ValueError(f"coverage {k}: expected contiguous cuda uint8 tensor of shape {(h, w)}, got {tuple(cov.shape)} {cov.dtype} {cov.device}")
                s.coverage[k] = cov.data_ptr()
        res = {}
        if want_n:
            if normals_fmt not in (abi.FMT_R10G10B10A2_UNORM, FMT_RGBA32F) or out_normals_fmt not in (abi.FMT_R10G10B10A2_UNORM, FMT_RGBA32F):
                raise ValueError("msaa_resolve_surfaces: normals are R10G10B10A2_UNORM or RGBA32F")
            if normals is None or len(normals) != nl:
                raise ValueError("msaa_resolve_surfaces: one normals plane per layer")
            for k, n in enumerate(normals):
                if normals_fmt == abi.FMT_R10G10B10A2_UNORM:
                    if not (n.is_cuda and n.is_contiguous() and n.dtype == torch.int32 and tuple(n.shape) == (h, w)):
                        raise ValueError(f"normals {k}: expected contiguous cuda int32 [H,W] (R10G10B10A2_UNORM words) of shape {(h, w)}")
                else:
                    _check_img(n, FMT_RGBA32F, f"normals {k}", (h, w))
                s.normals[k], s.normals_pitch_px[k] = n.data_ptr(), w
            res["normals"] = (torch.empty((h, w), dtype=torch.int32, device=self.device) if out_normals_fmt == abi.FMT_R10G10B10A2_UNORM
                              else empty_image(h, w, FMT_RGBA32F, self.device))
        if want_r:
            _check_img(scene_color, scene_fmt, "scene_color", (h, w))
            if roughness is None or len(roughness) != nl:
                raise ValueError("msaa_resolve_surfaces: one roughness (gb1) plane per layer")
            for k, g in enumerate(roughness):
                _check_img(g, FMT_RGBA32F, f"roughness {k}", (h, w))
                s.roughness[k], s.roughness_pitch_px[k] = g.data_ptr(), w
            if background is not None:
                _check_img(background, scene_fmt, "background", (h, w))
                if background.data_ptr() == scene_color.data_ptr():
                    raise ValueError("msaa_resolve_surfaces: background must not be scene_color")
                s.background, s.background_pitch_px = background.data_ptr(), w
            res["scene_color"] = scene_color
        if out_depth:
            res["depth"] = torch.empty((h, w), dtype=torch.float32, device=self.device)
        flat = self._hierarchy_buffer(w, h) if hierarchy else None
        self._ck(self.lib.vqhip_msaa_resolve_surfaces(self._h, self._stream(stream), C.byref(s), _ptr(res.get("depth")), w,
                                                      _ptr(res.get("normals")), out_normals_fmt if want_n else 0, w,
                                                      _ptr(scene_color), scene_fmt, w, _ptr(flat), int(flags)))
        if hierarchy:
            res["hierarchy"] = self._hierarchy_views(flat, w, h)
        return res

    # ---- post-process (RenderPostProcess, SceneRendering.cpp:2507) ------------------------------------------
    def gaussian_blur(self, src, fmt, tmp=None, out=None, stream=None):
        _check_img(src, fmt, "src")
        h, w = src.shape[0], src.shape[1]
        tmp = tmp if tmp is not None else torch.empty_like(src)
        out = out if out is not None else torch.empty_like(src)
        _check_img(tmp, fmt, "tmp", (h, w)); _check_img(out, fmt, "out", (h, w))
        p = abi.BlurParams(w, h)
        self._ck(self.lib.vqhip_gaussian_blur(self._h, self._stream(stream), _ptr(src), _ptr(tmp), _ptr(out), C.byref(p), fmt))
        return out

    def gaussian_blur_x(self, src, fmt, out=None, stream=None):
        _check_img(src, fmt, "src")
        out = out if out is not None else torch.empty_like(src)
        _check_img(out, fmt, "out", src.shape[:2])
        p = abi.BlurParams(src.shape[1], src.shape[0])
        self._ck(self.lib.vqhip_gaussian_blur_x(self._h, self._stream(stream), _ptr(src), _ptr(out), C.byref(p), fmt))
        return out

    def gaussian_blur_y(self, src, fmt, out=None, halo_top=None, halo_bottom=None, stream=None):
        _check_img(src, fmt, "src")
        out = out if out is not None else torch.empty_like(src)
        _check_img(out, fmt, "out", src.shape[:2])
        rows = _halo_rows(halo_top, halo_bottom, fmt, src.shape[1])
        p = abi.BlurParams(src.shape[1], src.shape[0])
        self._ck(self.lib.vqhip_gaussian_blur_y(self._h, self._stream(stream), _ptr(src), _ptr(out), _ptr(halo_top), _ptr(halo_bottom), rows, C.byref(p), fmt))
        return out

    def gaussian_blur_y_tonemap(self, src, fmt, out_fmt=FMT_RGBA8_UNORM, params=None, out=None, halo_top=None, halo_bottom=None, stream=None):
        """Fused CSMain_Y + Tonemapper (same bits as gaussian_blur_y followed by tonemap)."""
        _check_img(src, fmt, "src")
        h, w = src.shape[0], src.shape[1]
        out = out if out is not None else empty_image(h, w, out_fmt, self.device)
        _check_img(out, out_fmt, "out", (h, w))
        rows = _halo_rows(halo_top, halo_bottom, fmt, w)
        params = params if params is not None else abi.TonemapperParams.default()
        p = abi.BlurParams(w, h)
        self._ck(self.lib.vqhip_gaussian_blur_y_tonemap(self._h, self._stream(stream), _ptr(src), _ptr(out), _ptr(halo_top), _ptr(halo_bottom), rows,
                                                         C.byref(p), C.byref(params), fmt, out_fmt))
        return out

    def post_process_tile(self, src, in_fmt, out_fmt=FMT_RGBA8_UNORM, params=None, out=None, halo_top=None, halo_bottom=None, stream=None):
        """The blur + tonemapper chain over one row tile; halo_top / halo_bottom are the neighbouring tiles' SCENE-COLOUR rows (>= 10, in in_fmt)."""
        _check_img(src, in_fmt, "src")
        h, w = src.shape[0], src.shape[1]
        out = out if out is not None else empty_image(h, w, out_fmt, self.device)
        _check_img(out, out_fmt, "out", (h, w))
        rows = _halo_rows(halo_top, halo_bottom, in_fmt, w)
        params = params if params is not None else abi.TonemapperParams.default()
        self._ck(self.lib.vqhip_post_process_tile(self._h, self._stream(stream), _ptr(src), _ptr(out), _ptr(halo_top), _ptr(halo_bottom), rows, w, h,
                                                  C.byref(params), in_fmt, out_fmt))
        return out

    def post_process(self, src, in_fmt, out_fmt=FMT_RGBA8_UNORM, params=None, blur=True, out=None, stream=None):
        """RenderPostProcess's blur + tonemapper as one call (one kernel for RGBA16F -> RGBA8 and a per-channel curve); same bits as
        gaussian_blur_x -> gaussian_blur_y -> tonemap."""
        _check_img(src, in_fmt, "src")
        h, w = src.shape[0], src.shape[1]
        out = out if out is not None else empty_image(h, w, out_fmt, self.device)
        _check_img(out, out_fmt, "out", (h, w))
        params = params if params is not None else abi.TonemapperParams.default()
        self._ck(self.lib.vqhip_post_process(self._h, self._stream(stream), _ptr(src), _ptr(out), w, h, C.byref(params), int(bool(blur)), in_fmt, out_fmt))
        return out

    def tonemap(self, src, in_fmt, out_fmt=FMT_RGBA8_UNORM, params=None, out=None, stream=None):
        _check_img(src, in_fmt, "src")
        h, w = src.shape[0], src.shape[1]
        out = out if out is not None else empty_image(h, w, out_fmt, self.device)
        _check_img(out, out_fmt, "out", (h, w))
        params = params if params is not None else abi.TonemapperParams.default()
        self._ck(self.lib.vqhip_tonemap(self._h, self._stream(stream), _ptr(src), _ptr(out), w, h, C.byref(params), in_fmt, out_fmt))
        return out

    # ---- load-time IBL (ComputeBRDFIntegrationLUT Renderer.cpp:871, PreFilterEnvironmentMap EnvironmentMapRendering.cpp:139)
    def brdf_lut(self, size=1024, samples=2048, fmt=FMT_RG16F, stream=None):
        out = empty_image(size, size, fmt, self.device)
        self._ck(self.lib.vqhip_brdf_lut(self._h, self._stream(stream), _ptr(out), size, samples, fmt))
        return out

    def mip_chain(self, level0, stream=None):
        """level0: float32 cuda [H,W,4]. Returns (flat float32 chain [px,4], n_mips) incl. level 0 (min-filter mips)."""
        _check_img(level0, FMT_RGBA32F, "level0")
        h, w = level0.shape[0], level0.shape[1]
        n = abi.mip_level_count(w, h)
        chain = torch.empty((abi.mip_chain_px(w, h, n), 4), dtype=torch.float32, device=self.device)
        chain[: w * h].copy_(level0.reshape(-1, 4))
        self._ck(self.lib.vqhip_mip_chain_min_rgba32f(self._h, self._stream(stream), _ptr(chain), w, h, n))
        return chain, n

    # ---- G-buffer producer (ForwardLighting.hlsl:PSMain :226-287) --------------------------
    def mip_chain_rgba8(self, level0, stream=None):
        """level0: uint8 cuda [H,W,4], power-of-two dims. Returns (flat uint8 chain [px,4], n_mips), box-filtered mips."""
        _check_img(level0, FMT_RGBA8_UNORM, "level0")
        h, w = level0.shape[0], level0.shape[1]
        n = abi.mip_level_count(w, h)
        chain = torch.empty((abi.mip_chain_px(w, h, n), 4), dtype=torch.uint8, device=self.device)
        chain[: w * h].copy_(level0.reshape(-1, 4))
        self._ck(self.lib.vqhip_mip_chain_box_rgba8(self._h, self._stream(stream), _ptr(chain), w, h, n))
        return chain, n

    def _quad_plane(self, quad_uv, h, w, who):
        """(pointer, pitch in pixels) of a quad_uv plane for the _quad producers: cuda float32 [H, W, 4] with dense pixels; the row stride is the pitch"""
        t = quad_uv
        if not (t is not None and t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (h, w, 4) and t.stride(2) == 1 and t.stride(1) == 4
                and t.stride(0) % 4 == 0 and t.stride(0) >= 4 * w):
            raise ValueError(f"{who}: quad_uv: expected cuda float32 {(h, w, 4)} with dense pixels (the quad_uv plane of scene_quad_interpolants)")
        return _ptr(t), t.stride(0) // 4

    def gbuffer_from_materials_quad(self, ip, materials, ambient, quad_uv, ssao=None, out=None, stream=None):
        """vqhip_gbuffer_from_materials_quad (docs/DESIGN_DETAILS.md §7.20): gbuffer_from_materials with the uv derivatives taken from the helper lanes in
        `quad_uv` (scene_quad_interpolants' plane) instead of the planes' neighbours"""
        return self.gbuffer_from_materials(ip, materials, ambient, ssao, out, stream, _quad=quad_uv)

    def scene_normals_from_materials_quad(self, ip, materials, quad_uv, out_fmt=abi.FMT_R10G10B10A2_UNORM, out=None, stream=None):
        """vqhip_scene_normals_from_materials_quad: scene_normals_from_materials with helper-lane derivatives"""
        return self.scene_normals_from_materials(ip, materials, out_fmt, out, stream, _quad=quad_uv)

    def forward_lighting_from_materials_quad(self, ip, materials, per_frame, per_view, quad_uv, albedo_fmt=None, motion_fmt=None, sv_curr=None, sv_prev=None, **kw):
        """vqhip_forward_lighting_from_materials_quad: forward_lighting_from_materials with helper-lane derivatives. With albedo_fmt or motion_fmt the draw's
        other render targets are written too and (out, albedo_metallic, motion_vectors) is returned, as by forward_lighting_from_materials_mrt; else `out`."""
        if albedo_fmt is None and motion_fmt is None:
            return self.forward_lighting_from_materials(ip, materials, per_frame, per_view, _quad=quad_uv, **kw)
        h, w = ip[0].shape[0], ip[0].shape[1]
        t, albedo, motion = self._psmain_targets(h, w, albedo_fmt, motion_fmt, sv_curr, sv_prev, stream=kw.get("stream"))
        return self.forward_lighting_from_materials(ip, materials, per_frame, per_view, _targets=t, _quad=quad_uv, **kw), albedo, motion

    def gbuffer_from_materials(self, ip, materials, ambient, ssao=None, out=None, stream=None, _quad=None):
        """ip: 3 float32 cuda tensors [H,W,4] (vqhip_interpolants planes); materials: ctypes array of abi.MaterialDesc whose
        texture pointers are device pointers; ssao: uint8 cuda [H,W] or None. Returns the 4 G-buffer planes."""
        inter, h, w = _interpolants(ip)
        if out is None:
            out = tuple(torch.empty((h, w, 4), dtype=torch.float32, device=self.device) for _ in range(4))
        for i, t in enumerate(out):
            _check_img(t, FMT_RGBA32F, f"gb{i}")
        gbuf, s = _gbuffer(out, h, w), _ssao(ssao)
        n = len(materials) if materials is not None else 0
        args = (self._h, self._stream(stream), C.byref(inter), materials if n else None, n, float(ambient), _byref(s), C.byref(gbuf))
        self._ck(self.lib.vqhip_gbuffer_from_materials(*args) if _quad is None
                 else self.lib.vqhip_gbuffer_from_materials_quad(*args, *self._quad_plane(_quad, h, w, "gbuffer_from_materials_quad")))
        return out

    def scene_normals_from_materials(self, ip, materials, out_fmt=abi.FMT_R10G10B10A2_UNORM, out=None, stream=None, _quad=None):
        """The Z pre-pass's colour target (DepthPrePass.hlsl:PSMain): Tex_SceneNormals as int32 [H,W] (R10G10B10A2_UNORM bits; torch has no uint32) or
        float32 [H,W,4]. ip / materials as for gbuffer_from_materials (ip2 is not modified)."""
        inter, h, w = _interpolants(ip)
        if out is None:
            out = (torch.empty((h, w), dtype=torch.int32, device=self.device) if out_fmt == abi.FMT_R10G10B10A2_UNORM
                   else empty_image(h, w, FMT_RGBA32F, self.device))
        n = len(materials) if materials is not None else 0
        args = (self._h, self._stream(stream), C.byref(inter), materials if n else None, n, _ptr(out), out_fmt, w)
        self._ck(self.lib.vqhip_scene_normals_from_materials(*args) if _quad is None
                 else self.lib.vqhip_scene_normals_from_materials_quad(*args, *self._quad_plane(_quad, h, w, "scene_normals_from_materials_quad")))
        return out

    def forward_lighting_from_materials_mrt(self, ip, materials, per_frame, per_view, albedo_fmt=FMT_RGBA16F, motion_fmt=None, sv_curr=None, sv_prev=None,
                                            **kw):
        """forward_lighting_from_materials + the draw's other render targets: returns (out, albedo_metallic, motion_vectors)"""
        h, w = ip[0].shape[0], ip[0].shape[1]
        t, albedo, motion = self._psmain_targets(h, w, albedo_fmt, motion_fmt, sv_curr, sv_prev, stream=kw.get("stream"))
        return self.forward_lighting_from_materials(ip, materials, per_frame, per_view, _targets=t, **kw), albedo, motion

    def forward_lighting_from_materials(self, ip, materials, per_frame, per_view, ssao=None, out=None, out_fmt=FMT_RGBA16F, extra_point=None,
                                        env=None, shadow=None, stream=None, _targets=None, _quad=None):
        """PSMain in one kernel: gbuffer_from_materials(ip, materials, per_frame.fAmbientLightingFactor, ssao) + forward_lighting, the G-buffer
        record never leaving registers. Same bits as the two calls."""
        inter, h, w = _interpolants(ip)
        out = _out_image(out, h, w, out_fmt, self.device)
        s = _ssao(ssao)
        n = len(materials) if materials is not None else 0
        args = (self._h, self._stream(stream), C.byref(inter), materials if n else None, n, _byref(s), C.byref(per_frame), C.byref(per_view),
                *_extra_point(extra_point), _byref(env), _byref(shadow), _ptr(out), out.shape[1], out_fmt)
        if _quad is not None:
            self._ck(self.lib.vqhip_forward_lighting_from_materials_quad(*args, _byref(_targets), *self._quad_plane(_quad, h, w, "forward_lighting_from_materials_quad")))
            return out
        self._ck(self.lib.vqhip_forward_lighting_from_materials(*args) if _targets is None
                 else self.lib.vqhip_forward_lighting_from_materials_mrt(*args, C.byref(_targets)))
        return out

    # ---- FSR 1.0 (SceneRendering.cpp:2695-2784) -----------------------------------------------
    def fsr_easu(self, src, in_fmt, out_w, out_h, out_fmt=None, con=None, out=None, stream=None):
        _check_img(src, in_fmt, "src")
        out_fmt = in_fmt if out_fmt is None else out_fmt
        h, w = src.shape[0], src.shape[1]
        con = fsr_easu_con(w, h, out_w, out_h) if con is None else con
        if out is None:
            out = empty_image(out_h, out_w, out_fmt, self.device)
        _check_img(out, out_fmt, "out", (out_h, out_w))
        self._ck(self.lib.vqhip_fsr_easu(self._h, self._stream(stream), _ptr(src), w, h, in_fmt, con, _ptr(out), out_w, out_h, out_fmt))
        return out

    def fsr_rcas(self, src, in_fmt, out_fmt=None, con=None, out=None, stream=None):
        _check_img(src, in_fmt, "src")
        out_fmt = in_fmt if out_fmt is None else out_fmt
        h, w = src.shape[0], src.shape[1]
        con = fsr_rcas_con() if con is None else con
        if out is None:
            out = empty_image(h, w, out_fmt, self.device)
        _check_img(out, out_fmt, "out", (h, w))
        self._ck(self.lib.vqhip_fsr_rcas(self._h, self._stream(stream), _ptr(src), _ptr(out), w, h, con, in_fmt, out_fmt))
        return out

    def apply_reflections(self, reflection, scene_color, fmt, stream=None):
        """ApplyReflections.hlsl:CSMain: scene_color.rgb += reflection.rgb in place (alpha kept)."""
        _check_img(reflection, fmt, "reflection")
        _check_img(scene_color, fmt, "scene_color")
        h, w = scene_color.shape[0], scene_color.shape[1]
        self._ck(self.lib.vqhip_apply_reflections(self._h, self._stream(stream), _ptr(reflection), _ptr(scene_color), w, h, fmt))
        return scene_color

    def composite_reflections(self, reflection, scene_color, fmt, bounding_volumes=None, stream=None):
        """VQRenderer::CompositeReflections: apply_reflections, or — with the light-bounds image — the COMPOSITE_BOUNDING_VOLUMES permutation
        (rgb = BV.rgb * BV.a + (scene + reflection) * (1 - BV.a), alpha = BV.a). In place on scene_color."""
        _check_img(reflection, fmt, "reflection", scene_color.shape[:2])
        _check_img(scene_color, fmt, "scene_color")
        if bounding_volumes is not None:
            _check_img(bounding_volumes, fmt, "bounding_volumes", scene_color.shape[:2])
        h, w = scene_color.shape[0], scene_color.shape[1]
        self._ck(self.lib.vqhip_composite_reflections(self._h, self._stream(stream), _ptr(reflection), _ptr(bounding_volumes), _ptr(scene_color), w, h, fmt))
        return scene_color

    def ssr_environment_fallback(self, scene_color, scene_fmt, depth, normals, normal_fmt, cb, env, out_fmt=None, extract_roughness=False, out=None, stream=None):
        """ClassifyReflectionTiles.hlsl: the environment-map fallback of SSR's tile classification (SampleEnvironmentMap under the condition of
        ClassifyTiles :146-152). scene_color: [H,W,4] image whose alpha is the roughness; depth: float32 [H,W]; normals: uint32 [H,W]
        (R10G10B10A2_UNORM) or float32 [H,W,4]; cb: abi.SSSRConstants; env: abi.EnvMap. Returns the radiance image (and the R8 roughness)."""
        _check_img(scene_color, scene_fmt, "scene_color")
        h, w = scene_color.shape[0], scene_color.shape[1]
        assert depth.dtype == torch.float32 and tuple(depth.shape) == (h, w) and depth.is_contiguous()
        if normal_fmt == abi.FMT_R10G10B10A2_UNORM:
            assert normals.dtype == torch.int32 and tuple(normals.shape) == (h, w) and normals.is_contiguous()
        else:
            _check_img(normals, normal_fmt, "normals", (h, w))
        out_fmt = FMT_RGBA16F if out_fmt is None else out_fmt
        if out is None:
            out = empty_image(h, w, out_fmt, self.device)
        _check_img(out, out_fmt, "out", (h, w))
        rough = torch.empty((h, w), dtype=torch.uint8, device=self.device) if extract_roughness else None
        self._ck(self.lib.vqhip_ssr_environment_fallback(self._h, self._stream(stream), _ptr(scene_color), scene_fmt, 0, _ptr(depth), 0, _ptr(normals), normal_fmt, 0,
                                                         w, h, C.byref(cb), C.byref(env), _ptr(out), out_fmt, 0, _ptr(rough) if rough is not None else None))
        return (out, rough) if extract_roughness else out

    def ssr_classify(self, scene_color, scene_fmt, depth, cb, variance=None, tile_list=True, stream=None):
        """vqhip_ssr_classify: the ray list of ClassifyReflectionTiles.hlsl in this library's order (8 x 8 tiles row-major, lanes of RemapLane8x8 inside a tile).
        scene_color: [H,W,4] image whose alpha is the roughness; depth: float32 cuda [H,W], level 0 of the depth hierarchy (rows may be strided); variance: None or
        float16 cuda [H,W] (g_variance_history); cb: abi.SSSRConstants with bufferDimensions == (W, H). Returns (ray_list int32 [H*W] — PackRayCoords words, only
        the first counters[0] are written —, counters int32 [2] = (rays, denoiser tiles), tile_list int32 [tiles] | None); nothing is read back to the host."""
        _check_img(scene_color, scene_fmt, "scene_color")
        h, w = scene_color.shape[0], scene_color.shape[1]
        if (cb.bufferDimensions[0], cb.bufferDimensions[1]) != (w, h):
            raise ValueError(f"ssr_classify: cb.bufferDimensions {cb.bufferDimensions[0]} x {cb.bufferDimensions[1]} is not the frame {w} x {h}")
        if not (depth.is_cuda and depth.dtype == torch.float32 and tuple(depth.shape) == (h, w) and depth.stride(1) == 1 and depth.stride(0) >= w):
            raise ValueError(f"depth: expected cuda float32 {(h, w)} with unit column stride, got {tuple(depth.shape)} {depth.dtype} strides {depth.stride()}")
        if variance is not None and not (variance.is_cuda and variance.is_contiguous() and variance.dtype == torch.float16 and tuple(variance.shape) == (h, w)):
            raise ValueError(f"variance: expected contiguous cuda float16 {(h, w)}, got {tuple(variance.shape)} {variance.dtype}")
        rays = torch.empty((h * w,), dtype=torch.int32, device=self.device)
        counters = torch.empty((2,), dtype=torch.int32, device=self.device)
        tiles = torch.empty((((w + 7) // 8) * ((h + 7) // 8),), dtype=torch.int32, device=self.device) if tile_list else None
        self._ck(self.lib.vqhip_ssr_classify(self._h, self._stream(stream), _ptr(scene_color), scene_fmt, 0, _ptr(depth), depth.stride(0), _ptr(variance), 0,
                                             C.byref(cb), _ptr(rays), _ptr(counters), _ptr(tiles)))
        return rays, counters, tiles

    def ssr_intersect(self, ray_list, counters, lit_scene, lit_fmt, hierarchy, normals, normal_fmt, roughness8, blue_noise, cb, env, radiance, radiance_fmt, stream=None):
        """vqhip_ssr_intersect: Intersect.hlsl for every entry of the ray list, IN PLACE on `radiance` (the image ssr_environment_fallback filled; returned).
        ray_list / counters: as ssr_classify returned them; hierarchy: the level views of depth_hierarchy (or their flat tensor); normals: int32 [H,W]
        (R10G10B10A2_UNORM) or float32 [H,W,4]; roughness8: uint8 [H,W], the extracted roughness; blue_noise: uint8 [128,128,2]."""
        _check_img(lit_scene, lit_fmt, "lit_scene")
        h, w = lit_scene.shape[0], lit_scene.shape[1]
        if (cb.bufferDimensions[0], cb.bufferDimensions[1]) != (w, h):
            raise ValueError(f"ssr_intersect: cb.bufferDimensions {cb.bufferDimensions[0]} x {cb.bufferDimensions[1]} is not the frame {w} x {h}")
        _check_img(radiance, radiance_fmt, "radiance", (h, w))
        flat = hierarchy[0] if isinstance(hierarchy, (list, tuple)) else hierarchy
        n_floats = sum(r * c for r, c in abi.depth_hierarchy_shapes(w, h))
        if not (flat.is_cuda and flat.dtype == torch.float32 and flat.untyped_storage().nbytes() - flat.storage_offset() * 4 >= n_floats * 4):
            raise ValueError("hierarchy: expected the cuda float32 buffer of depth_hierarchy for this frame size")
        _check_normals("", "normals", normals, normal_fmt, (h, w))
        _check_dense("roughness8", roughness8, torch.uint8, (h, w))
        _check_dense("blue_noise", blue_noise, torch.uint8, (abi.SSR_BLUE_NOISE_SIZE, abi.SSR_BLUE_NOISE_SIZE, 2))
        _check_list("ray_list", ray_list, h * w)
        _check_list("counters", counters, 2)
        self._ck(self.lib.vqhip_ssr_intersect(self._h, self._stream(stream), _ptr(ray_list), _ptr(counters), _ptr(lit_scene), lit_fmt, 0, _ptr(flat),
                                              _ptr(normals), normal_fmt, 0, _ptr(roughness8), _ptr(blue_noise), C.byref(cb), C.byref(env),
                                              _ptr(radiance), radiance_fmt, 0))
        return radiance

    # ---- SSR denoiser passes 2 and 3 (docs/DESIGN_DETAILS.md §7.12) ------------------------------------------------
    def _denoise_common(self, who, tile_list, counters, roughness8, average, avg_fmt, cb, planes, out, out_fmt, out_variance):
        w, h = int(cb.bufferDimensions[0]), int(cb.bufferDimensions[1])
        h8, w8 = (h + 7) // 8, (w + 7) // 8
        _check_tiles(f"{who}: ", tile_list, counters, h8 * w8)
        _check_dense(f"{who}: roughness8", roughness8, torch.uint8, (h, w))
        if avg_fmt == abi.FMT_R11G11B10_FLOAT:
            _check_words(f"{who}: average", average, (h8, w8), "R11G11B10_FLOAT")
        else:
            _check_img(average, avg_fmt, "average", (h8, w8))
        for name, (t, fmt) in planes.items():
            if fmt is None:                                                     # an R16F plane; rows may be strided
                _check_plane(f"{who}: {name}: expected cuda float16", t, torch.float16, (h, w))
            else:
                _check_img(t, fmt, name, (h, w))
        if out is None:
            out = empty_image(h, w, out_fmt, self.device)
        _check_img(out, out_fmt, "out", (h, w))
        if out_variance is None:
            out_variance = torch.empty((h, w), dtype=torch.float16, device=self.device)
        _check_dense(f"{who}: out_variance", out_variance, torch.float16, (h, w))
        return out, out_variance

    def ssr_prefilter(self, tile_list, counters, depth, normals, normal_fmt, roughness8, average, avg_fmt, radiance, radiance_fmt, variance, cb,
                      out=None, out_fmt=FMT_RGBA16F, out_variance=None, stream=None):
        """vqhip_ssr_prefilter: Prefilter.hlsl for every tile of the denoiser tile list (as ssr_classify returned it with its counters). depth: float32 [H,W]
        (level 0 of the hierarchy, rows may be strided); normals: int32 [H,W] (R10G10B10A2_UNORM) or float32 [H,W,4]; average: int32 [H8,W8] (R11G11B10_FLOAT) or
        float32 [H8,W8,4]; variance: float16 [H,W]. Pixels of unlisted tiles keep what `out` / `out_variance` held. Returns (out, out_variance)."""
        w, h = int(cb.bufferDimensions[0]), int(cb.bufferDimensions[1])
        _check_plane("depth: expected cuda float32", depth, torch.float32, (h, w))
        _check_normals("", "normals", normals, normal_fmt, (h, w))
        out, out_variance = self._denoise_common("ssr_prefilter", tile_list, counters, roughness8, average, avg_fmt, cb,
                                                 {"radiance": (radiance, radiance_fmt), "variance": (variance, None)}, out, out_fmt, out_variance)
        self._ck(self.lib.vqhip_ssr_prefilter(self._h, self._stream(stream), _ptr(tile_list), _ptr(counters), _ptr(depth), depth.stride(0), _ptr(normals), normal_fmt, 0,
                                              _ptr(roughness8), _ptr(average), avg_fmt, _ptr(radiance), radiance_fmt, 0, _ptr(variance), variance.stride(0),
                                              C.byref(cb), _ptr(out), out_fmt, 0, _ptr(out_variance), 0))
        return out, out_variance

    def ssr_resolve_temporal(self, tile_list, counters, roughness8, average, avg_fmt, radiance, radiance_fmt, reprojected, reprojected_fmt, variance, sample_count, cb,
                             out=None, out_fmt=FMT_RGBA16F, out_variance=None, stream=None):
        """vqhip_ssr_resolve_temporal: ResolveTemporal.hlsl for every tile of the list. radiance: the prefiltered radiance; reprojected: [H,W,4] image; variance /
        sample_count: float16 [H,W]. Returns (out, out_variance); pixels of unlisted tiles keep what they held."""
        out, out_variance = self._denoise_common("ssr_resolve_temporal", tile_list, counters, roughness8, average, avg_fmt, cb,
                                                 {"radiance": (radiance, radiance_fmt), "reprojected": (reprojected, reprojected_fmt), "variance": (variance, None),
                                                  "sample_count": (sample_count, None)}, out, out_fmt, out_variance)
        self._ck(self.lib.vqhip_ssr_resolve_temporal(self._h, self._stream(stream), _ptr(tile_list), _ptr(counters), _ptr(roughness8), _ptr(average), avg_fmt,
                                                     _ptr(radiance), radiance_fmt, 0, _ptr(reprojected), reprojected_fmt, 0, _ptr(variance), variance.stride(0),
                                                     _ptr(sample_count), sample_count.stride(0), C.byref(cb), _ptr(out), out_fmt, 0, _ptr(out_variance), 0))
        return out, out_variance

    # ---- SSR denoiser pass 1 (docs/DESIGN_DETAILS.md §7.13) ---------------------------------------------------------
    def ssr_reproject(self, tile_list, counters, depth, normals, normal_fmt, roughness8, depth_history, normal_history, normal_history_fmt, roughness8_history,
                      radiance, radiance_fmt, radiance_history, radiance_history_fmt, motion, motion_fmt, variance_history, sample_count_history, cb,
                      out_reprojected=None, out_fmt=FMT_RGBA16F, out_average=None, avg_fmt=abi.FMT_R11G11B10_FLOAT, out_variance=None, out_sample_count=None, stream=None):
        """vqhip_ssr_reproject: Reproject.hlsl for every tile of the denoiser tile list. depth / depth_history: float32 [H,W] (rows may be strided); normals /
        normal_history: int32 [H,W] (R10G10B10A2_UNORM) or float32 [H,W,4]; roughness8 / roughness8_history: uint8 [H,W]; radiance (alpha = ray length) /
        radiance_history: [H,W,4] images; motion: [H,W,2] RG16F | RG32F; variance_history / sample_count_history: float16 [H,W]. Outputs that are not given are
        allocated ZEROED (the pass writes listed tiles and glossy pixels only). Returns (out_reprojected, out_average, out_variance, out_sample_count); out_average
        is int32 [H8,W8] (R11G11B10_FLOAT words) or float32 [H8,W8,4]."""
        w, h = int(cb.bufferDimensions[0]), int(cb.bufferDimensions[1])
        h8, w8 = (h + 7) // 8, (w + 7) // 8
        _check_tiles("ssr_reproject: ", tile_list, counters, h8 * w8)

        def plane(t, name, dtype):                                                  # these messages spell the dtype with its module
            return _check_plane(f"ssr_reproject: {name}: expected cuda {dtype}", t, dtype, (h, w))
        s = abi.SSRReprojectSurfaces()
        s.depth_pitch_px, s.depth_history_pitch_px = plane(depth, "depth", torch.float32), plane(depth_history, "depth_history", torch.float32)
        s.roughness_pitch_px, s.roughness_history_pitch_px = plane(roughness8, "roughness8", torch.uint8), plane(roughness8_history, "roughness8_history", torch.uint8)
        s.variance_history_pitch_px = plane(variance_history, "variance_history", torch.float16)
        s.sample_count_history_pitch_px = plane(sample_count_history, "sample_count_history", torch.float16)
        _check_normals("ssr_reproject: ", "normals", normals, normal_fmt, (h, w))
        _check_normals("ssr_reproject: ", "normal_history", normal_history, normal_history_fmt, (h, w))
        _check_img(radiance, radiance_fmt, "radiance", (h, w))
        _check_img(radiance_history, radiance_history_fmt, "radiance_history", (h, w))
        if motion_fmt not in (abi.FMT_RG16F, abi.FMT_RG32F):
            raise ValueError("ssr_reproject: motion_fmt must be RG16F or RG32F")
        _check_img(motion, motion_fmt, "motion", (h, w))
        if out_reprojected is None:
            out_reprojected = torch.zeros((h, w, 4), dtype=_TORCH_DTYPE[out_fmt][0], device=self.device)
        _check_img(out_reprojected, out_fmt, "out_reprojected", (h, w))
        if avg_fmt == abi.FMT_R11G11B10_FLOAT:
            if out_average is None:
                out_average = torch.zeros((h8, w8), dtype=torch.int32, device=self.device)
            _check_words("ssr_reproject: out_average", out_average, (h8, w8), "R11G11B10_FLOAT")
        else:
            if out_average is None:
                out_average = torch.zeros((h8, w8, 4), dtype=torch.float32, device=self.device)
            _check_img(out_average, avg_fmt, "out_average", (h8, w8))
        outs = []
        for t, name in ((out_variance, "out_variance"), (out_sample_count, "out_sample_count")):
            if t is None:
                t = torch.zeros((h, w), dtype=torch.float16, device=self.device)
            _check_dense(f"ssr_reproject: {name}", t, torch.float16, (h, w))
            outs.append(t)
        out_variance, out_sample_count = outs
        for name, t in (("tile_list", tile_list), ("counters", counters), ("depth", depth), ("normals", normals), ("roughness", roughness8), ("depth_history", depth_history),
                        ("normal_history", normal_history), ("roughness_history", roughness8_history), ("radiance", radiance), ("radiance_history", radiance_history),
                        ("motion_vectors", motion), ("variance_history", variance_history), ("sample_count_history", sample_count_history),
                        ("out_reprojected", out_reprojected), ("out_average", out_average), ("out_variance", out_variance), ("out_sample_count", out_sample_count)):
            setattr(s, name, t.data_ptr())
        s.normals_fmt, s.normal_history_fmt, s.radiance_fmt, s.radiance_history_fmt = normal_fmt, normal_history_fmt, radiance_fmt, radiance_history_fmt
        s.motion_fmt, s.out_reprojected_fmt, s.out_average_fmt = motion_fmt, out_fmt, avg_fmt
        self._ck(self.lib.vqhip_ssr_reproject(self._h, self._stream(stream), C.byref(s), C.byref(cb)))
        return out_reprojected, out_average, out_variance, out_sample_count

    def visualize(self, src, in_fmt, params, out_fmt=None, out=None, stream=None):
        """Visualization.hlsl:CSMain (debug draw modes). params: abi.VizParams. src in the format of the target the mode shows: a colour image, the int32 [H,W]
        words of scene_normals_from_materials (in_fmt R10G10B10A2_UNORM) or the RG16F / RG32F motion vectors of forward_lighting_mrt; out_fmt defaults to in_fmt
        for colour inputs, RGBA16F otherwise."""
        if in_fmt == abi.FMT_R10G10B10A2_UNORM:
            if not (src.is_cuda and src.is_contiguous() and src.dtype == torch.int32 and src.dim() == 2):
                raise ValueError("src: expected contiguous cuda int32 [H,W] (R10G10B10A2_UNORM words)")
        else:
            _check_img(src, in_fmt, "src")
        if out_fmt is None:
            out_fmt = in_fmt if in_fmt in (FMT_RGBA32F, FMT_RGBA16F, FMT_RGBA8_UNORM) else FMT_RGBA16F
        h, w = src.shape[0], src.shape[1]
        if out is None:
            out = empty_image(h, w, out_fmt, self.device)
        _check_img(out, out_fmt, "out")
        self._ck(self.lib.vqhip_visualize(self._h, self._stream(stream), _ptr(src), _ptr(out), w, h, C.byref(params), in_fmt, out_fmt))
        return out

    # ---- HDRI ingest (Image::LoadFromFile -> stbi_loadf, TextureManager.cpp:566) ----------------
    def load_hdr(self, data, stream=None):
        """data: bytes of a Radiance .hdr file. Returns the decoded float32 cuda image [H,W,4] (alpha 1) == level 0 of the chain."""
        w, h, _ = hdr_parse_header(data)
        out = torch.empty((h, w, 4), dtype=torch.float32, device=self.device)
        self._ck(self.lib.vqhip_hdr_decode_rgba32f(self._h, self._stream(stream), data, len(data), _ptr(out), w, h))
        return out

    def hdr_downsize(self, img, out_w, out_h, stream=None):
        """Image::CreateResizedImage as the HDRI fallback uses it (EnvironmentMap.cpp:167): integer ratios only (k x k mean), else VQHipError(-3)."""
        _check_img(img, FMT_RGBA32F, "img")
        out = torch.empty((out_h, out_w, 4), dtype=torch.float32, device=self.device)
        self._ck(self.lib.vqhip_hdr_downsize_rgba32f(self._h, self._stream(stream), _ptr(img), img.shape[1], img.shape[0], _ptr(out), out_w, out_h))
        return out

    # ---- skydome (Skydome.hlsl:39-56, SceneRendering.cpp:1822-1850) -------------------------
    def skydome(self, equirect_level0, params, color, fmt, coverage_ip=None, stream=None):
        """equirect_level0: float32 cuda [h0,w0,4]; params: abi.SkydomeParams; color: scene-colour tensor [H,W,4] written in place
        where coverage_ip (the 3 interpolant planes, or None = everywhere) has material index < 0."""
        _check_img(equirect_level0, FMT_RGBA32F, "equirect_level0")
        _check_img(color, fmt, "color")
        h, w = color.shape[0], color.shape[1]
        cov = None
        if coverage_ip is not None:
            for i, t in enumerate(coverage_ip):
                _check_img(t, FMT_RGBA32F, f"ip{i}")
            cov = abi.Interpolants(coverage_ip[0].data_ptr(), coverage_ip[1].data_ptr(), coverage_ip[2].data_ptr(), w, h, w)
        self._ck(self.lib.vqhip_skydome(self._h, self._stream(stream), _ptr(equirect_level0), equirect_level0.shape[1], equirect_level0.shape[0],
                                        C.byref(params), C.byref(cov) if cov is not None else None, _ptr(color), w, h, w, fmt))
        return color

    def set_fresnel_pow(self, exp2_log2):
        """False (default): pow(1 - cos, 5) as the product x*((x*x)*(x*x)); True: exp2(5*log2 x), the engine's own DXC lowering."""
        self._ck(self.lib.vqhip_set_fresnel_pow(self._h, 1 if exp2_log2 else 0))

    def set_arithmetic(self, dxc):
        """False (default): the literal reading of dot / normalize / length / reflect; True: the DXC reading (FMA-chain dot, v * correctly rounded rsqrt)."""
        self._ck(self.lib.vqhip_set_arithmetic(self._h, abi.ARITH_DXC if dxc else abi.ARITH_LITERAL))

    def set_option(self, key, value):
        """vqhip_set_option: a tuning / A-B option of this context (include/vqhip.h lists them); value None restores the default."""
        self._ck(self.lib.vqhip_set_option(self._h, key.encode(), None if value is None else str(value).encode()))

    # the environment variables of rounds 1-3 map onto options (scripts that sweep forms): VQHIP_LUT_FORM -> "lut_form", ...
    ENV_OPTIONS = {"VQHIP_LUT_FORM": "lut_form", "VQHIP_DIFFUSE_FORM": "diffuse_form", "VQHIP_DIFFUSE_SEQ_FORM": "diffuse_seq_form",
                   "VQHIP_BLUR_Y_WGS": "blur_y_wgs", "VQHIP_SHADE_WG": "shade_wg", "VQHIP_PSMAIN_WAVES": "psmain_waves"}

    def set_option_env(self, env_name, value):
        v = None if value in (None, "", "default", "0") else value
        self.set_option(self.ENV_OPTIONS[env_name], v)

    def unlit_composite(self, coverage_ip, colors, color, fmt, stream=None):
        """Light gizmo meshes (Unlit.hlsl:PSMain, SceneRendering.cpp:1787-1819): pixels whose ip2.w index is -(2+k) get colors[k]
        (sequence of 4-tuples); `color` is written in place."""
        _check_img(color, fmt, "color")
        h, w = color.shape[0], color.shape[1]
        for i, t in enumerate(coverage_ip):
            _check_img(t, FMT_RGBA32F, f"ip{i}")
        cov = abi.Interpolants(coverage_ip[0].data_ptr(), coverage_ip[1].data_ptr(), coverage_ip[2].data_ptr(), w, h, w)
        arr = (abi.float4 * max(len(colors), 1))(*[abi.float4(*[float(v) for v in c]) for c in colors])
        self._ck(self.lib.vqhip_unlit_composite(self._h, self._stream(stream), C.byref(cov), C.cast(arr, C.c_void_p), len(colors), _ptr(color), w, h, w, fmt))
        return color

    def conv_diffuse(self, chain, w0, h0, n_mips, res=64, step=0.010, order=CONV_SEQUENTIAL, fmt=FMT_RGBA16F, stream=None):
        dt, ch = _TORCH_DTYPE[fmt]
        out = torch.empty((6, res, res, ch), dtype=dt, device=self.device)
        self._ck(self.lib.vqhip_conv_diffuse(self._h, self._stream(stream), _ptr(chain), w0, h0, n_mips, res, step, order, _ptr(out), fmt))
        return out

    def conv_specular(self, chain, w0, h0, n_mips, res0=128, order=CONV_SEQUENTIAL, fmt=FMT_RGBA16F, stream=None):
        dt, ch = _TORCH_DTYPE[fmt]
        mips = abi.specular_mip_count(res0)
        out = torch.empty((abi.cube_px(res0, mips), ch), dtype=dt, device=self.device)
        self._ck(self.lib.vqhip_conv_specular(self._h, self._stream(stream), _ptr(chain), w0, h0, n_mips, res0, order, _ptr(out), fmt))
        return out, mips

    def envmap_prefilter(self, chain, w0, h0, n_mips, diffuse_res=64, diffuse_step=0.010, spec_res0=128, order=CONV_SEQUENTIAL, stream=None):
        """Returns dict(diffuse_unblurred, diffuse_blurred, specular, spec_mips) of float16 tensors (reference formats)."""
        mips = abi.specular_mip_count(spec_res0)
        d0 = torch.empty((6, diffuse_res, diffuse_res, 4), dtype=torch.float16, device=self.device)
        d1 = torch.empty_like(d0)
        tmp = torch.empty((diffuse_res, diffuse_res, 4), dtype=torch.float16, device=self.device)
        sp = torch.empty((abi.cube_px(spec_res0, mips), 4), dtype=torch.float16, device=self.device)
        o = abi.EnvMapOut(d0.data_ptr(), d1.data_ptr(), tmp.data_ptr(), sp.data_ptr())
        self._ck(self.lib.vqhip_envmap_prefilter(self._h, self._stream(stream), _ptr(chain), w0, h0, n_mips, diffuse_res, diffuse_step,
                                                 spec_res0, order, C.byref(o)))
        return {"diffuse_unblurred": d0, "diffuse_blurred": d1, "specular": sp, "spec_mips": mips, "_tmp": tmp}


def make_envmap(diffuse_cube, spec_cube, spec_res0, spec_mips, lut):
    """abi.EnvMap over device tensors (keeps no references — the caller owns the tensors)."""
    return abi.EnvMap(diffuse_cube.data_ptr(), diffuse_cube.shape[1], spec_cube.data_ptr(), spec_res0, spec_mips,
                      lut.data_ptr(), lut.shape[0])
