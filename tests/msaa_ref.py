"""The 4x MSAA contract of vqhip_forward_lighting_msaa (docs/DESIGN_DETAILS.md §7.9) in numpy: sample ownership from the coverage bytes and the
resolve (((s0 + s1) + s2) + s3) * 0.25 in binary32, samples widened from the output format, the result stored back to it (astype: RNE)."""
import numpy as np

from vqengine_amd import abi


def owners(coverage):
    """coverage: list of L uint8 [H,W] planes -> int8 [H,W,4]: the owning layer of each sample (lowest layer whose mask has bit s), -1 = background"""
    own = np.full(coverage[0].shape + (4,), -1, np.int8)
    for k in reversed(range(len(coverage))):
        for s in range(4):
            own[..., s] = np.where((coverage[k] >> s) & 1, k, own[..., s])
    return own


def resolve_samples(samples, dtype):
    """samples: [..., 4 samples, C] of the stored format -> [..., C] of `dtype`: binary32 sums in sample order, * 0.25, stored"""
    s = samples.astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        r = (((s[..., 0, :] + s[..., 1, :]) + s[..., 2, :]) + s[..., 3, :]) * np.float32(0.25)
        return r.astype(dtype)


def resolve(shaded, coverage, background=None, out_fmt=abi.FMT_RGBA16F):
    """shaded: per layer the [H,W,4] image PSMain writes for that layer's record (output format; pixels a layer does not own are ignored);
    background: [H,W,4] of the output format or None (0) -> the resolved [H,W,4] image"""
    dtype = np.float16 if out_fmt == abi.FMT_RGBA16F else np.float32
    own = owners(coverage)
    bg = np.zeros(shaded[0].shape, dtype) if background is None else background.astype(dtype)
    samples = np.repeat(bg[..., None, :], 4, axis=-2)
    for k, img in enumerate(shaded):
        samples = np.where((own == k)[..., None], img.astype(dtype)[..., None, :], samples)
    return resolve_samples(samples, dtype)
