"""Host-side producers of what vqhip_line_draws consumes beside the meshes: the host mirror of the three producers of line draws in the reference's
bounding-volumes pass — the batched bounding boxes (Batching.cpp:520-560, 566-567, 621-651, drawn by RenderBoundingBoxes, SceneRendering.cpp:1853-1922, through the
instanced cbuffer), the light bounds drawn again as wire (the second half of RenderLightBounds, SceneRendering.cpp:1991-2014) and the vertex axes of the selected
objects' meshes (Scene.cpp:596-639, drawn by RenderDebugVertexAxes, SceneRendering.cpp:2018-2058). numpy only.

A bounding box is a pair (extent_min (3), extent_max (3)). Lights and meshes are unlit_scene's. The matrices are INPUTS, like shadow_scene's: formed in binary64
and rounded once. Row vectors, VQ_matrix memory order."""
import ctypes as C

import numpy as np

from . import abi
from . import shadow_scene as S
from . import unlit_scene as US

F = np.float32
MAX_INSTANCES = abi.LINES_MAX_INSTANCES                  # MAX_INSTANCE_COUNT__UNLIT_SHADER: boxes per draw
BOX_TRANSPARENCY = 0.75                                  # Batching.cpp:566
GAME_OBJECT_BOX_COLOR = (0.0, 0.2, 0.8, BOX_TRANSPARENCY)
MESH_BOX_COLOR = (0.0, 0.8, 0.2, BOX_TRANSPARENCY)
CUBE = S.box((1.0, 1.0, 1.0))                            # the engine's cube: 12 triangles, 36 indices, corners at +-1


def bounding_box_world(extent_min, extent_max):
    """FBoundingBox::GetWorldTransformMatrix: the +-1 cube scaled by (max - min) * 0.5 and moved to (max + min) * 0.5, both in binary32"""
    lo, hi = np.asarray(extent_min, dtype=F), np.asarray(extent_max, dtype=F)
    return S.scaling(((hi - lo) * F(0.5)).astype(np.float64)) @ S.translation(((hi + lo) * F(0.5)).astype(np.float64))


def bounding_box_draws(boxes, view_proj, color=MESH_BOX_COLOR, cube=CUBE):
    """BatchBoundingBoxRenderCommandData: batches of at most 512 boxes, one instanced draw of the 36-index cube each, matWorldViewProj[i] =
    GetWorldTransformMatrix() * viewProj, one colour per draw. Returns a list of dict(vertices, indices, matrices float32 [n, 4, 4], color float32 [4])."""
    view_proj = np.asarray(view_proj, dtype=np.float64).reshape(4, 4)
    boxes = list(boxes)
    out = []
    for first in range(0, len(boxes), MAX_INSTANCES):
        mats = np.stack([(bounding_box_world(lo, hi) @ view_proj).astype(F) for lo, hi in boxes[first:first + MAX_INSTANCES]])
        out.append({"vertices": cube[0], "indices": cube[1], "matrices": mats, "color": np.asarray(color, dtype=F)})
    return out


def light_bounds_wire_draws(lights, view_proj, sphere, cone=None):
    """the wire loop of RenderLightBounds: the meshes and matrices of unlit_scene.light_bounds_draws, the colour as GatherLightBoundsRenderData left it — the
    solid loop's color.w *= 0.01f acts on the cbuffer copy of the blended path, not on the render data: alpha stays 0.45. Returns draws as bounding_box_draws
    does, with `light`: the index into `lights`."""
    out = []
    for d in US.light_bounds_draws(lights, view_proj, sphere, cone, blended=False):
        out.append({"vertices": d["vertices"], "indices": d["indices"], "matrices": d["cb"][:16].reshape(1, 4, 4).copy(), "color": d["cb"][16:20].copy(),
                    "light": d["light"]})
    return out


def vertex_axes_data(world, normal, view_proj, local_axis_size):
    """One VQ_VertexAxesData as float32 [52] (208 bytes): matWorld, matNormal, matViewProj, LocalAxisSize, padding"""
    cb = np.zeros(abi.VERTEX_AXES_DATA_BYTES // 4, dtype=F)
    for k, m in enumerate((world, normal, view_proj)):
        cb[16 * k:16 * k + 16] = np.asarray(m, dtype=np.float64).reshape(4, 4).astype(F).reshape(-1)
    cb[48] = F(local_axis_size)
    return cb


def as_struct(cb):
    """the abi.VertexAxesData view of a float32 [52] block (a copy)"""
    assert C.sizeof(abi.VertexAxesData) == abi.VERTEX_AXES_DATA_BYTES
    return abi.VertexAxesData.from_buffer_copy(np.ascontiguousarray(cb, dtype=F).tobytes())


def normal_matrix(world):
    """Transform::NormalMatrix: the inverse transpose of the world matrix's upper 3 x 3, the rest identity"""
    world = np.asarray(world, dtype=np.float64).reshape(4, 4)
    m = np.eye(4)
    m[:3, :3] = np.linalg.inv(world[:3, :3]).T
    return m


def vertex_axes_draws(meshes, view_proj, local_axis_size):
    """CollectDebugVertexDrawParams + RenderDebugVertexAxes: one point-list draw per mesh of the selected objects, LOD 0, no instancing. meshes: a list of
    (vertices [V, >= 9] — position, normal, tangent —, indices, world). Returns a list of dict(vertices, indices, cb float32 [52])."""
    return [{"vertices": v, "indices": i, "cb": vertex_axes_data(world, normal_matrix(world), view_proj, local_axis_size)} for v, i, world in meshes]
