"""Host-side producers of what vqhip_scene_interpolants (and, at the end, vqhip_displace_meshes) consumes beside shadow_scene's: procedural meshes in the engine's full 44-byte vertex (position 3,
normal 3, tangent 3, uv 2 -> float32 [V, 11]) and the four matrix blocks of PerObjectLightingData per instance. numpy only; shadow_scene is imported unchanged.

Like shadow_scene this is an INPUT producer: the meshes are written for this project, the matrices are formed in binary64 and rounded once. Conventions are the
engine's: left-handed, row vectors, front faces clockwise seen from outside."""
import numpy as np

from . import shadow_scene as S

F = np.float32
VERTEX_FLOATS = S.VERTEX_FLOATS_ENGINE

# per face of the box: (normal, tangent = the direction uv.x grows in, bitangent = the direction uv.y grows in); normal = tangent x bitangent, left-handed
_FACES = (((0, 0, -1), (1, 0, 0), (0, 1, 0)), ((0, 0, 1), (-1, 0, 0), (0, 1, 0)), ((-1, 0, 0), (0, 0, -1), (0, 1, 0)),
          ((1, 0, 0), (0, 0, 1), (0, 1, 0)), ((0, 1, 0), (1, 0, 0), (0, 0, 1)), ((0, -1, 0), (1, 0, 0), (0, 0, -1)))


def box(half=(1.0, 1.0, 1.0)):
    """An axis-aligned box centred at the origin with per-face normals, tangents and uvs: 24 vertices, 12 triangles, clockwise seen from outside. uv runs over
    [0, 1]^2 on every face. Returns (vertices float32 [24, 11], indices int64 [36])."""
    h = np.asarray(half, dtype=np.float64)
    verts, idx = [], []
    for n, t, b in _FACES:
        n, t, b = (np.asarray(v, dtype=np.float64) for v in (n, t, b))
        base = len(verts)
        for (u, v) in ((0, 0), (0, 1), (1, 1), (1, 0)):
            p = (n + (2 * u - 1) * t + (2 * v - 1) * b) * h
            verts.append(np.concatenate([p, n, t, (u, v)]))
        idx += [base, base + 1, base + 2, base, base + 2, base + 3]
    return np.array(verts, dtype=F), np.array(idx, dtype=np.int64)


def room(half=(1.0, 1.0, 1.0)):
    """The box seen from inside: every triangle reversed, normals pointing inwards (tangents and uvs kept)."""
    v, idx = box(half)
    v = v.copy()
    v[:, 3:6] = -v[:, 3:6]
    return v, idx.reshape(-1, 3)[:, ::-1].reshape(-1).copy()


def uv_sphere(radius=1.0, slices=24, stacks=22):
    """shadow_scene.uv_sphere's vertices and triangles with normal = position / radius, tangent = the direction of growing longitude ((1, 0, 0) at the poles)
    and uv = (longitude / 2 pi, colatitude / pi). The seam shares its vertices: uv.x wraps inside the last column of triangles."""
    p, idx = S.uv_sphere(radius, slices, stacks)
    p64 = p.astype(np.float64)
    n = p64 / radius
    ph = np.arctan2(p64[:, 2], p64[:, 0]) % (2.0 * np.pi)
    th = np.arccos(np.clip(n[:, 1], -1.0, 1.0))
    t = np.stack([-np.sin(ph), np.zeros_like(ph), np.cos(ph)], axis=1)
    pole = (np.abs(p64[:, 0]) + np.abs(p64[:, 2])) == 0.0
    t[pole] = (1.0, 0.0, 0.0)
    uv = np.stack([ph / (2.0 * np.pi), th / np.pi], axis=1)
    return np.concatenate([p64, n, t, uv], axis=1).astype(F), idx


def grid(n, size=2.0, jitter=0.0, seed=0, height=0.0):
    """shadow_scene.grid with normal +y, tangent +x and uv = the position in the grid's square, [0, 1]^2."""
    p, idx = S.grid(n, size, jitter, seed, height)
    v = np.zeros((p.shape[0], VERTEX_FLOATS), dtype=F)
    v[:, :3] = p
    v[:, 4] = 1.0
    v[:, 6] = 1.0
    v[:, 9] = (p[:, 0].astype(np.float64) / size + 0.5).astype(F)
    v[:, 10] = (p[:, 2].astype(np.float64) / size + 0.5).astype(F)
    return v, idx


def rotation_of(world):
    """Transform::RotationMatrix of a world matrix built as scaling @ rotation @ translation (positive scales): the upper 3 x 3 with unit rows."""
    world = np.asarray(world, dtype=np.float64)
    m = np.eye(4)
    r = world[:3, :3]
    m[:3, :3] = r / np.sqrt((r * r).sum(axis=1, keepdims=True))
    return m


def instance_matrices_full(worlds, view_proj, prev_view_proj, prev_worlds=None):
    """(matWorldViewProj, matWorld, matNormal, matWorldViewProjPrev), each float32 [n, 4, 4] in VQ_matrix memory order: PerObjectLightingData of the instances
    `worlds` under this frame's and the previous frame's view-projection. matNormal is the rotation (Batching.cpp:281); prev_worlds defaults to worlds."""
    worlds = np.asarray(worlds, dtype=np.float64).reshape(-1, 4, 4)
    prev = worlds if prev_worlds is None else np.asarray(prev_worlds, dtype=np.float64).reshape(-1, 4, 4)
    c = lambda m: np.ascontiguousarray(np.asarray(m).astype(F))      # noqa: E731
    return c(worlds @ view_proj), c(worlds), c(np.stack([rotation_of(w) for w in worlds])), c(prev @ prev_view_proj)


# ---- alpha-tested geometry: what vqhip_scene_masked_depth / vqhip_shadow_masked_depth consume beside the meshes above ---------------------------------------------
def card(half_w=1.0, half_h=1.0, uv_min=(0.0, 0.0), uv_max=(1.0, 1.0)):
    """A leaf / fence / decal card: the box's -z face alone, in the plane z = 0 (normal -z, tangent +x), clockwise seen from -z. uv runs from uv_min (the corner
    -x, -y) to uv_max: values outside [0, 1] and negative ones exercise WRAP. Returns (vertices float32 [4, 11], indices int64 [6])."""
    (u0, v0), (u1, v1) = uv_min, uv_max
    verts = [np.array([(2 * u - 1) * half_w, (2 * v - 1) * half_h, 0.0, 0, 0, -1, 1, 0, 0, u0 + u * (u1 - u0), v0 + v * (v1 - v0)], dtype=np.float64)
             for (u, v) in ((0, 0), (0, 1), (1, 1), (1, 0))]
    return np.array(verts, dtype=F), np.array([0, 1, 2, 0, 2, 3], dtype=np.int64)


def alpha_checker(width, height, cell=1, rgb=(200, 180, 90)):
    """An RGBA8 checker of `cell`-texel squares whose alpha is 0 / 255 (texel (0, 0) is transparent): uint8 [height, width, 4]"""
    y, x = np.mgrid[0:height, 0:width]
    img = np.empty((height, width, 4), dtype=np.uint8)
    img[..., :3] = rgb
    img[..., 3] = np.where(((x // cell) + (y // cell)) % 2 == 1, 255, 0)
    return img


def alpha_columns(width, height, period=4, opaque=(1, 2), rgb=(90, 160, 60)):
    """An RGBA8 pattern of vertical stripes: alpha 255 in the columns whose x % period is in `opaque`, else 0. The default (T O O T) has two transparent columns
    side by side — a bilinear fetch reads 0 between them — while every 2 x 2 block is half opaque: mip 1 is 127 everywhere. uint8 [height, width, 4]"""
    img = np.empty((height, width, 4), dtype=np.uint8)
    img[..., :3] = rgb
    img[..., 3] = np.where(np.isin(np.arange(width) % period, opaque), 255, 0)[None, :]
    return img


def mip_chain_rgba8(level0, mips=None):
    """The mip chain the engine uploads (VQ_DXGI_UTILS::MipImage, 4-byte branch: each channel (a + b + c + d) / 4 in integers, the last row / column of an odd
    level repeated): (chain uint8 [texels of all levels, 4], number of levels). mips None = down to 1 x 1. A 1-texel alpha checker has mip 1 = 127 everywhere."""
    lv = np.ascontiguousarray(level0, dtype=np.uint8)
    h, w = lv.shape[:2]
    full = 1
    while max(w, h) >> full:
        full += 1
    n = full if mips is None else int(mips)
    if not 1 <= n <= full:
        raise ValueError(f"mip_chain_rgba8: mips must be 1..{full}")
    out = [lv.reshape(-1, 4)]
    for _ in range(1, n):
        sh, sw = lv.shape[:2]
        dh, dw = max(sh // 2, 1), max(sw // 2, 1)
        y0, x0 = 2 * np.arange(dh), 2 * np.arange(dw)
        y1, x1 = np.minimum(y0 + 1, sh - 1), np.minimum(x0 + 1, sw - 1)
        s = lv.astype(np.uint32)
        lv = ((s[y0][:, x0] + s[y0][:, x1] + s[y1][:, x0] + s[y1][:, x1]) // 4).astype(np.uint8)
        out.append(lv.reshape(-1, 4))
    return np.ascontiguousarray(np.concatenate(out, axis=0)), n


# ---- heightmap displacement: what vqhip_displace_meshes consumes beside the meshes above --------------------------------------------------------------------------
def heightmap_chain(w, h, kind="hill", seed=0, mips=None):
    """An RGBA8 height map and its mip chain (mip_chain_rgba8's box filter): (chain uint8 [texels of all levels, 4], number of levels). The height lives in RED;
    green is its complement, blue and alpha are seeded noise, so that a fetch of the wrong channel shows. kind: "hill" (a smooth bump on a raised base: no texel
    is 0), "noise" (seeded, every value), "steps" (red = 16 x the texel's number mod 256: bilinear fractions show), "zero" (red 0 everywhere, the rest noise)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    if kind == "hill":
        cx, cy = 0.5 * (w - 1), 0.5 * (h - 1)
        r2 = ((x - cx) / max(0.5 * w, 1.0)) ** 2 + ((y - cy) / max(0.5 * h, 1.0)) ** 2
        red = np.rint(40.0 + 215.0 * np.exp(-3.0 * r2))
    elif kind == "noise":
        red = rng.integers(0, 256, size=(h, w))
    elif kind == "steps":
        red = (16 * (y * w + x) + 8) % 256
    elif kind == "zero":
        red = np.zeros((h, w))
    else:
        raise ValueError(f"heightmap_chain: unknown kind {kind!r}")
    img = np.empty((h, w, 4), dtype=np.uint8)
    img[..., 0] = red
    img[..., 1] = 255 - img[..., 0]
    img[..., 2:] = rng.integers(1, 256, size=(h, w, 2))
    return mip_chain_rgba8(img, mips)


def with_heightmap(mesh, chain, w, h, mips, uv_scale_offset=(1.0, 1.0, 0.0, 0.0), displacement=0.0):
    """A grid / card / box mesh (vertices float32 [V, >= 11], indices) with the height map of its material attached: the dict tests/displace_ref.py reads and
    capi.DisplaceJob is filled from — vertices, indices, heightmap = dict(chain | None for the null SRV, w, h, mips), scale_offset, displacement."""
    v, idx = mesh
    return {"vertices": np.ascontiguousarray(v, dtype=F), "indices": np.asarray(idx, dtype=np.int64),
            "heightmap": {"chain": None if chain is None else np.ascontiguousarray(chain, dtype=np.uint8), "w": int(w), "h": int(h), "mips": int(mips)},
            "scale_offset": tuple(float(x) for x in uv_scale_offset), "displacement": float(displacement)}
