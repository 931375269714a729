"""docs/DESIGN_DETAILS.md §7.22 (the contract H1 .. H4 of vqhip_displace_meshes) stated in numpy, on the sampler arithmetic of tests/masked_depth_ref.level_alpha
generalised to a channel argument: CalcHeightOffset of the reference's five vertex stages, applied once to a vertex stream.

  H1  u = uv.x * scale.x + offset.x, v likewise: binary32, the product and the sum rounded separately.
  H2  s = the bilinear WRAP fetch of level 0 of an RGBA8 chain, red channel: 8-bit fixed-point fractions, exact weights, the FMA chain, then * RN(1 / 255).
      Only level 0 is read whatever `mips` says; a chain of None is the null SRV and samples 0. NaN and +-inf coordinates take what fixed8 / mod define.
  H3  h = s * displacement; y' = y + h; x, z and every other float of the vertex are copied bit for bit.
  H4  the reference's y + h keeps -0 only when y and h are both -0; the rasterisers' retained y + 0.0f then makes +0 of it (`consumed_y`): a sign of zero, the one
      known deviation between sampling in each vertex stage and displacing the stream once.

A height map is masked_depth_ref's texture dict: dict(chain uint8 [px, 4] | None, w, h, mips). A job is dict(vertices float32 [V, k >= 11] (uv at columns 9, 10),
heightmap, scale_offset = 4 floats, displacement)."""
import numpy as np

from tests.cacao_ref import fixed8
from tests.masked_depth_ref import RCP255, fma, level_offset, mip_dim

F, F64, I64 = np.float32, np.float64, np.int64
RED, GREEN, BLUE, ALPHA = 0, 1, 2, 3


def level_taps(tex, level, u, v):
    """the footprint of the bilinear WRAP fetch of one level: (x0, x1, y0, y1 int64, wx, wy float32 fractions in 1/256) of the float32 arrays u, v"""
    W, H = mip_dim(tex["w"], level), mip_dim(tex["h"], level)
    with np.errstate(all="ignore"):
        ix, wx = fixed8(u * F(W) - F(0.5))
        iy, wy = fixed8(v * F(H) - F(0.5))
    return np.mod(ix, W), np.mod(ix + 1, W), np.mod(iy, H), np.mod(iy + 1, H), wx, wy


def level_channel(tex, level, u, v, channel):
    """masked_depth_ref.level_alpha for any channel and ONE level: the blend in byte units (exact in binary32)"""
    u, v = np.asarray(u, F), np.asarray(v, F)
    W = mip_dim(tex["w"], level)
    x0, x1, y0, y1, wx, wy = level_taps(tex, level, u, v)
    c = tex["chain"][:, channel].astype(F)
    base = level_offset(tex["w"], tex["h"], level)
    c00, c10, c01, c11 = c[base + y0 * W + x0], c[base + y0 * W + x1], c[base + y1 * W + x0], c[base + y1 * W + x1]
    one = F(1.0)
    w00, w10, w01, w11 = (one - wx) * (one - wy), wx * (one - wy), (one - wx) * wy, wx * wy
    return fma(w11, c11, fma(w01, c01, fma(w10, c10, w00 * c00)))


def sample_level0(tex, u, v, channel=RED):
    """H2: SampleLevel(LinearSamplerTess, (u, v), 0)[channel]"""
    u, v = np.asarray(u, F), np.asarray(v, F)
    if tex is None or tex["chain"] is None:
        return np.zeros(u.shape, F)
    return (level_channel(tex, 0, u, v, channel) * RCP255).astype(F)


def transformed_uv(vertices, scale_offset):
    """H1"""
    sx, sy, ox, oy = (F(x) for x in scale_offset)
    uv = np.asarray(vertices, F)[:, 9:11]
    with np.errstate(all="ignore"):
        return (uv[:, 0] * sx + ox).astype(F), (uv[:, 1] * sy + oy).astype(F)


def height_offsets(job):
    """h of every vertex of a job (H1 .. H3's product), float32 [V]"""
    u, v = transformed_uv(job["vertices"], job["scale_offset"])
    with np.errstate(all="ignore"):
        return (sample_level0(job["heightmap"], u, v) * F(job["displacement"])).astype(F)


def displace(job, compact=False):
    """vqhip_displace_meshes for one job: float32 [V, k] (the full-stride copy, y replaced) or [V, 3] (outStrideBytes == 12)"""
    src = np.ascontiguousarray(job["vertices"], F)
    out = src.copy()
    with np.errstate(all="ignore"):
        out[:, 1] = src[:, 1] + height_offsets(job)
    return np.ascontiguousarray(out[:, :3]) if compact else out


def consumed_y(y):
    """what every rasteriser of the library makes of a stored y: the retained null-heightmap y + 0.0f (H4)"""
    return (np.asarray(y, F) + F(0.0)).astype(F)


def reference_stage_y(y, h):
    """the reference's vertex stage: ONE sum y + h, no + 0.0f behind it"""
    with np.errstate(all="ignore"):
        return (np.asarray(y, F) + np.asarray(h, F)).astype(F)
