"""Host-side producers of what vqhip_unlit_draws consumes beside the meshes: the cbuffer FFrameConstantBufferUnlit (VQ_UnlitData) of each draw, and the host mirror of
the two producers of FLightRenderData in Scene.cpp — GatherLightMeshRenderData (:1335-1381, the light gizmos drawn by SceneRendering.cpp:1787-1819) and
GatherLightBoundsRenderData (:691-753, the light volumes drawn by the solid half of RenderLightBounds, SceneRendering.cpp:1940-1989). numpy only.

A light is a dict: type "point" | "spot" | "directional", position (3), color (3), brightness, range, and optionally outer_cone_degrees (spot), rotation (the 4 x 4
rotation matrix of the light's quaternion, default identity) and enabled (default True). Meshes come from the caller as (vertices, indices); shadow_scene.uv_sphere
serves the tests for both the sphere and, scaled, the cone.

Colours are computed in binary32, operation by operation, as the C++ does. The matrices are INPUTS, like shadow_scene's: formed in binary64 and rounded once. Row
vectors, VQ_matrix memory order."""
import ctypes as C

import numpy as np

from . import abi
from . import shadow_scene as S

F = np.float32
LIGHT_MESH_SCALE = 0.1                   # Light::GetWorldTransformationMatrix (Light.cpp:123-131)
BOUNDS_ALPHA = F(0.45)                   # Scene.cpp:705
BLENDED_ALPHA_SCALE = F(0.01)            # SceneRendering.cpp:1971


def unlit_data(world, view_proj, color):
    """One VQ_UnlitData as float32 [20] (80 bytes): matModelViewProj = matWorldTransformation * viewProj (SceneRendering.cpp:1801, :1972), color."""
    world, view_proj = (np.asarray(m, dtype=np.float64).reshape(4, 4) for m in (world, view_proj))
    cb = np.zeros(abi.UNLIT_DATA_BYTES // 4, dtype=F)
    cb[:16] = (world @ view_proj).astype(F).reshape(-1)
    cb[16:20] = np.asarray(color, dtype=F)
    return cb


def as_struct(cb):
    """the abi.UnlitData view of a float32 [20] block (a copy)"""
    assert C.sizeof(abi.UnlitData) == abi.UNLIT_DATA_BYTES
    return abi.UnlitData.from_buffer_copy(np.ascontiguousarray(cb, dtype=F).tobytes())


def _rotation(light):
    return np.asarray(light.get("rotation", np.eye(4)), dtype=np.float64).reshape(4, 4)


def _attenuated_brightness(light, camera_position):
    """distanceSq = dot(camera - light, camera - light); attenuation = 1.0f / distanceSq; Brightness * attenuation — binary32, in that order"""
    with np.errstate(all="ignore"):
        d = np.asarray(camera_position, dtype=F) - np.asarray(light["position"], dtype=F)
        dist_sq = F(F(F(d[0] * d[0]) + F(d[1] * d[1])) + F(d[2] * d[2]))
        return F(F(light["brightness"]) * F(F(1.0) / dist_sq))


def light_mesh_color(light, camera_position, attenuate=True):
    """FLightRenderData::color of a gizmo AS THE C++ PARSES IT (Scene.cpp:1356-1361): `l.Color.x * bAttenuateLight ? attenuatedBrightness : 1.0f` is
    `(l.Color.x * bAttenuateLight) ? attenuatedBrightness : 1.0f` — the channel selects between the attenuated brightness (a non-zero product, NaN included) and
    1.0f and does not scale anything. Kept as written, like the outline's .xyx. Alpha 1."""
    ab = _attenuated_brightness(light, camera_position)
    with np.errstate(all="ignore"):
        rgb = [ab if F(F(c) * F(1.0 if attenuate else 0.0)) != F(0.0) else F(1.0) for c in np.asarray(light["color"], dtype=F)[:3]]
    return np.array(rgb + [F(1.0)], dtype=F)


def light_mesh_draws(lights, camera_position, view_proj, sphere, attenuate=True):
    """GatherLightMeshRenderData: one draw per enabled point or spot light (directional lights are skipped), the sphere at the light scaled by 0.1. Returns a
    list of dict(vertices, indices, cb, light: the index into `lights`), in the lights' order."""
    v, i = sphere
    out = []
    for n, l in enumerate(lights):
        if not l.get("enabled", True) or l["type"] == "directional":
            continue
        world = S.scaling((LIGHT_MESH_SCALE,) * 3) @ _rotation(l) @ S.translation(l["position"])
        out.append({"vertices": v, "indices": i, "cb": unlit_data(world, view_proj, light_mesh_color(l, camera_position, attenuate)), "light": n})
    return out


def light_bounds_color(light, blended):
    """FLightRenderData::color of a light volume (Scene.cpp:705-713): the light's colour, alpha 0.45; on the blended path color.w *= 0.01f as
    SceneRendering.cpp:1971 writes it into the cbuffer (binary32)."""
    a = F(BOUNDS_ALPHA * BLENDED_ALPHA_SCALE) if blended else BOUNDS_ALPHA
    return np.array(list(np.asarray(light["color"], dtype=F)[:3]) + [a], dtype=F)


def light_bounds_world(light):
    """matWorldTransformation of a light volume (Scene.cpp:720-751): the unit sphere scaled by Range at a point light; at a spot light the unit cone through
    scaleConeToRange * alignConeToSpotLightTransformation * (the light's transform at scale 1, turned -90 degrees about its local x axis). None: not drawn."""
    rng = float(light["range"])
    if light["type"] == "point":
        return S.scaling((rng,) * 3) @ _rotation(light) @ S.translation(light["position"])
    if light["type"] == "spot":
        base = float(np.tan(F(np.radians(F(light.get("outer_cone_degrees", 30.0))))) * rng)
        align = S.translation((0.0, -rng, 0.0))
        tf = S.rotation_x(np.radians(-90.0)) @ _rotation(light) @ S.translation(light["position"])
        return S.scaling((base, rng, base)) @ align @ tf
    return None


def light_bounds_draws(lights, view_proj, sphere, cone=None, blended=False):
    """GatherLightBoundsRenderData: one draw per enabled point light (sphere) or spot light (cone; skipped when the caller has no cone mesh). `blended`: the
    path of UNLIT_BLEND_PSO into scene colour (reflections off); else the opaque path into the bounding-volumes target. Returns draws as light_mesh_draws."""
    out = []
    for n, l in enumerate(lights):
        if not l.get("enabled", True):
            continue
        world = light_bounds_world(l)
        mesh = sphere if l["type"] == "point" else cone
        if world is None or mesh is None:
            continue
        out.append({"vertices": mesh[0], "indices": mesh[1], "cb": unlit_data(world, view_proj, light_bounds_color(l, blended)), "light": n})
    return out
