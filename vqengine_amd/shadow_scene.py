"""Host-side producers of what vqhip_shadow_depth and vqhip_scene_depth consume: procedural meshes, instance transforms, light view-projections and the main
camera's. numpy only.

Everything here is an INPUT of the library: the rasteriser reads positions, indices and VQ_matrix blocks as handed over, so this module is a valid producer of
them and is not bit-pinned to DirectXMath (its matrices are formed in binary64 and rounded once; XMMatrixLookAtLH / XMMatrixPerspectiveFovLH work in binary32
and may differ in the last bit). The meshes are written for this project. Conventions are the engine's: left-handed, row vectors (clip = [P, 1] @ M with M
stored as VQ_matrix.m[row][col]), front faces clockwise seen from outside.
  cube faces  : +X, -X, +Y, -Y, +Z, -Z with the up vectors of CubemapUtility::CalculateViewMatrix (CubemapUtility.cpp:42-47)
  projections : 90 degree FOV at aspect 1 for spot and point lights (Light.cpp:216-222), orthographic for the directional light (:227)"""
import numpy as np

F = np.float32
VERTEX_FLOATS_ENGINE = 11      # the engine's 44-byte vertex: position 3, normal 3, tangent 3, uv 2

CUBE_FACES = (  # (look direction, up): CUBEMAP_LOOK_RIGHT, _LEFT, _UP, _DOWN, _FRONT, _BACK
    ((1, 0, 0), (0, 1, 0)), ((-1, 0, 0), (0, 1, 0)), ((0, 1, 0), (0, 0, -1)), ((0, -1, 0), (0, 0, 1)), ((0, 0, 1), (0, 1, 0)), ((0, 0, -1), (0, 1, 0)))


# ---- meshes: (positions float32 [V, 3], indices int64 [3 T]) -------------------------------------------------------------------------------------------------
def box(half=(1.0, 1.0, 1.0)):
    """An axis-aligned box centred at the origin: 8 corners, 12 triangles, clockwise seen from outside (left-handed)."""
    hx, hy, hz = half
    p = np.array([[sx * hx, sy * hy, sz * hz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], dtype=F)   # corner index = x + 2 y + 4 z
    quads = ((0, 2, 3, 1), (5, 7, 6, 4), (4, 6, 2, 0), (1, 3, 7, 5), (2, 6, 7, 3), (4, 0, 1, 5))                 # -z, +z, -x, +x, +y, -y
    idx = [i for (a, b, c, d) in quads for i in (a, b, c, a, c, d)]
    return p, np.array(idx, dtype=np.int64)


def room(half=(1.0, 1.0, 1.0)):
    """The box seen from inside: the same corners with every triangle reversed."""
    p, idx = box(half)
    return p, idx.reshape(-1, 3)[:, ::-1].reshape(-1).copy()


def uv_sphere(radius=1.0, slices=24, stacks=22):
    """A latitude / longitude sphere: 2 poles + (stacks - 1) rings of `slices` vertices; 2 * slices * (stacks - 1) triangles, clockwise seen from outside."""
    pts = [(0.0, radius, 0.0)]
    for s in range(1, stacks):
        th = np.pi * s / stacks
        for k in range(slices):
            ph = 2.0 * np.pi * k / slices
            pts.append((radius * np.sin(th) * np.cos(ph), radius * np.cos(th), radius * np.sin(th) * np.sin(ph)))
    pts.append((0.0, -radius, 0.0))
    ring = lambda s, k: 1 + (s - 1) * slices + k % slices      # noqa: E731
    idx = []
    for k in range(slices):
        idx += [0, ring(1, k + 1), ring(1, k)]
        idx += [len(pts) - 1, ring(stacks - 1, k), ring(stacks - 1, k + 1)]
    for s in range(1, stacks - 1):
        for k in range(slices):
            a, b, c, d = ring(s, k), ring(s, k + 1), ring(s + 1, k + 1), ring(s + 1, k)
            idx += [a, b, c, a, c, d]
    return np.array(pts, dtype=F), np.array(idx, dtype=np.int64)


def grid(n, size=2.0, jitter=0.0, seed=0, height=0.0):
    """An n x n cell grid in the xz plane, centred at the origin, `size` on a side, facing +y; interior vertices move by up to jitter * cell in x and z (seeded)."""
    rng = np.random.default_rng(seed)
    u = np.linspace(-0.5 * size, 0.5 * size, n + 1)
    x, z = np.meshgrid(u, u, indexing="xy")
    cell = size / n
    dx = (rng.random((n + 1, n + 1)) - 0.5) * 2.0 * jitter * cell
    dz = (rng.random((n + 1, n + 1)) - 0.5) * 2.0 * jitter * cell
    inner = np.zeros((n + 1, n + 1), dtype=bool)
    inner[1:-1, 1:-1] = True
    x = x + np.where(inner, dx, 0.0)
    z = z + np.where(inner, dz, 0.0)
    p = np.stack([x, np.full_like(x, height), z], axis=-1).reshape(-1, 3).astype(F)
    v = lambda i, j: j * (n + 1) + i      # noqa: E731
    idx = []
    for j in range(n):
        for i in range(n):
            a, b, c, d = v(i, j), v(i + 1, j), v(i + 1, j + 1), v(i, j + 1)
            idx += [a, d, c, a, c, b]     # clockwise seen from +y (left-handed)
    return p, np.array(idx, dtype=np.int64)


def ground_quad(size=2.0, height=0.0):
    """Two triangles in the xz plane facing +y."""
    return grid(1, size, 0.0, 0, height)


def engine_vertices(positions):
    """positions [V, 3] as the engine's 44-byte vertices [V, 11]: the position first, a recognisable filler in the attributes the shadow pass never reads."""
    v = np.full((positions.shape[0], VERTEX_FLOATS_ENGINE), 12345.0, dtype=F)
    v[:, :3] = positions
    return v


# ---- matrices (row vectors; float64 in, float32 VQ_matrix out) -----------------------------------------------------------------------------------------------
def _norm(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt(np.dot(v, v))


def translation(t):
    m = np.eye(4)
    m[3, :3] = t
    return m


def scaling(s):
    return np.diag(list(np.broadcast_to(np.asarray(s, dtype=np.float64), (3,))) + [1.0])


def rotation_y(angle):
    c, s = np.cos(angle), np.sin(angle)
    m = np.eye(4)
    m[0, 0], m[0, 2], m[2, 0], m[2, 2] = c, -s, s, c
    return m


def rotation_x(angle):
    c, s = np.cos(angle), np.sin(angle)
    m = np.eye(4)
    m[1, 1], m[1, 2], m[2, 1], m[2, 2] = c, s, -s, c
    return m


def look_at_lh(eye, at, up):
    eye = np.asarray(eye, dtype=np.float64)
    z = _norm(np.asarray(at, dtype=np.float64) - eye)
    x = _norm(np.cross(np.asarray(up, dtype=np.float64), z))
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2] = x, y, z
    m[3, :3] = (-np.dot(x, eye), -np.dot(y, eye), -np.dot(z, eye))
    return m


def perspective_fov_lh(fov_y, aspect, near, far):
    h = 1.0 / np.tan(0.5 * fov_y)
    r = far / (far - near)
    m = np.zeros((4, 4))
    m[0, 0], m[1, 1], m[2, 2], m[2, 3], m[3, 2] = h / aspect, h, r, 1.0, -r * near
    return m


def orthographic_lh(width, height, near, far):
    m = np.eye(4)
    m[0, 0], m[1, 1], m[2, 2], m[3, 2] = 2.0 / width, 2.0 / height, 1.0 / (far - near), -near / (far - near)
    return m


def spot_view_proj(position, direction, near, far, up=(0.0, 1.0, 0.0)):
    """Light::CalculateSpotLightViewMatrix x CalculateProjectionMatrix(SPOT): look along `direction`, 90 degree FOV."""
    position = np.asarray(position, dtype=np.float64)
    return look_at_lh(position, position + _norm(direction), up) @ perspective_fov_lh(0.5 * np.pi, 1.0, near, far)


def directional_view_proj(direction, distance, viewport, near, far, up=(0.0, 1.0, 0.0)):
    """Light::CalculateDirectionalLightViewMatrix x the orthographic projection: the light sits `distance` from the origin against `direction`, looking at it."""
    d = _norm(direction)
    up = np.asarray(up, dtype=np.float64)
    if abs(np.dot(d, up)) == 1.0:
        up = _norm(up + np.array([0.001, 0.0, 0.0]))
    return look_at_lh(-d * distance, (0.0, 0.0, 0.0), up) @ orthographic_lh(viewport[0], viewport[1], near, far)


def point_face_view_proj(position, face, near, far):
    """CubemapUtility::CalculateViewMatrix(face, position) x CalculateProjectionMatrix(POINT): face 0..5 = +X, -X, +Y, -Y, +Z, -Z."""
    position = np.asarray(position, dtype=np.float64)
    look, up = CUBE_FACES[face]
    return look_at_lh(position, position + np.asarray(look, dtype=np.float64), up) @ perspective_fov_lh(0.5 * np.pi, 1.0, near, far)


def camera_view_proj(eye, at, fov_y, aspect, near, far, up=(0.0, 1.0, 0.0)):
    """The main camera of vqhip_scene_depth: Camera::UpdateViewMatrix x XMMatrixPerspectiveFovLH (Camera.cpp) — look from `eye` at `at`, perspective, left-handed,
    depth 0 .. 1, aspect = width / height of the viewport."""
    return look_at_lh(eye, at, up) @ perspective_fov_lh(fov_y, aspect, near, far)


def instance_matrices(worlds, view_proj):
    """(matWorldViewProj [n, 4, 4], matWorld [n, 4, 4]) as float32 VQ_matrix blocks of the world transforms `worlds` under one view-projection."""
    worlds = np.asarray(worlds, dtype=np.float64).reshape(-1, 4, 4)
    return np.ascontiguousarray((worlds @ view_proj).astype(F)), np.ascontiguousarray(worlds.astype(F))
