"""Host-side producer of what vqhip_outline consumes beside the meshes of surface_scene: the cbuffer OutlineData of one selected (mesh, material) pair, built from
world, view and projection as GatherOutlineMeshRenderData builds it (Scene.cpp:642-689): matWorldView = world x view, matNormalView = normal x view with normal the
rotation of the world transform (Transform::NormalMatrix), matViewInverse the inverse of view, Scale 1. numpy only.

Like shadow_scene this is an INPUT producer: the matrices are formed in binary64 and rounded once. Row vectors, VQ_matrix memory order."""
import ctypes as C

import numpy as np

from . import abi
from . import surface_scene as SS

F = np.float32


def outline_data(world, view, proj, color=(1.0, 0.5, 0.0, 1.0), uv_scale_bias=(1.0, 1.0, 0.0, 0.0), height_displacement=0.0, normal=None):
    """One VQ_OutlineData as float32 [92] (368 bytes). normal: the 4 x 4 normal matrix, default the rotation of `world`."""
    world, view, proj = (np.asarray(m, dtype=np.float64).reshape(4, 4) for m in (world, view, proj))
    normal = SS.rotation_of(world) if normal is None else np.asarray(normal, dtype=np.float64).reshape(4, 4)
    cb = np.zeros(abi.OUTLINE_DATA_BYTES // 4, dtype=F)
    for k, m in enumerate((world, world @ view, normal @ view, proj, np.linalg.inv(view))):
        cb[16 * k:16 * k + 16] = m.astype(F).reshape(-1)
    cb[80:84] = np.asarray(color, dtype=F)
    cb[84:88] = np.asarray(uv_scale_bias, dtype=F)
    cb[88], cb[89] = F(1.0), F(height_displacement)
    return cb


def as_struct(cb):
    """the abi.OutlineData view of a float32 [92] block (a copy)"""
    assert C.sizeof(abi.OutlineData) == abi.OUTLINE_DATA_BYTES
    return abi.OutlineData.from_buffer_copy(np.ascontiguousarray(cb, dtype=F).tobytes())
