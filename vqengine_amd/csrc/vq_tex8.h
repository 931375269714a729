// vq_tex8.h — the lane-local pieces of the software RGBA8_UNORM mip-chain fetch (trilinear WRAP, DESIGN.md "G-buffer producer" / "Sampling contract"):
// the filter footprint (mip level + fraction, tap offsets and weights of both levels), the tap loads and the bilinear blend. gbuffer.hip builds its wave-level
// fetch (ballots, paired loads) on them; the rasterisers' alpha test (raster.hip, raster_view.hip; docs/DESIGN_DETAILS.md §7.19) runs in a divergent loop and uses
// the ballot-free fetch_lane below: the same arithmetic, lane by lane.
#pragma once
#include "vq_devmath.h"
#include "vq_sampling.h"

namespace vqk {
using namespace vqd;

struct __attribute__((packed, aligned(4))) TexelPair { uint32_t a, b; };

// One level of a footprint: texel offsets (from the chain base) of the two rows, the two columns, the 4 weights.
struct LevelTaps { uint32_t row0, row1; int x0, x1; float w00, w10, w01, w11; };
struct Footprint { LevelTaps l0, l1; float f; };


template <bool POT> VQD LevelTaps level_taps(int w0, int h0, int level, float u, float v) {
    const int W = mip_dim(w0, level), H = mip_dim(h0, level);
    int ix, iy; float wx, wy;
    fixed8(u * (float)W - 0.5f, &ix, &wx);
    fixed8(v * (float)H - 0.5f, &iy, &wy);
    LevelTaps t;
    int y0, y1;
    if (POT) { t.x0 = ix & (W - 1); t.x1 = (ix + 1) & (W - 1); y0 = iy & (H - 1); y1 = (iy + 1) & (H - 1); }
    else     { t.x0 = wrapi(ix, W); t.x1 = wrapi(ix + 1, W); y0 = wrapi(iy, H); y1 = wrapi(iy + 1, H); }
    const uint32_t base = chain_level_offset<POT>(w0, h0, level);    // vq_sampling.h: closed form for power-of-two chains
    t.row0 = base + __umul24(y0, W);                              // dims < 2^24: full-rate v_mad_u32_u24
    t.row1 = base + __umul24(y1, W);
    t.w00 = (1.0f - wx) * (1.0f - wy); t.w10 = wx * (1.0f - wy); t.w01 = (1.0f - wx) * wy; t.w11 = wx * wy;   // == blend4's weights
    return t;
}

// Texture2D.Sample / SampleBias: isotropic trilinear WRAP, LOD from the quad derivatives
template <bool POT> VQD Footprint make_footprint(int w, int h, int mips, float2 uv, float2 ddx, float2 ddy, float bias) {
    const float W = (float)w, H = (float)h;
    const float dXx = ddx.x * W, dXy = ddx.y * H, dYx = ddy.x * W, dYy = ddy.y * H;
    const float rx = fma_(dXy, dXy, dXx * dXx), ry = fma_(dYy, dYy, dYx * dYx);
    const float lod = 0.5f * log2_(max_(rx, ry)) + bias;
    const float maxl = (float)(mips - 1);
    const float l = (lod > 0.0f) ? ((lod < maxl) ? lod : maxl) : 0.0f;
    const int fl = f2i_floor(l * 256.0f + 0.5f);
    int lo = fl >> 8;
    Footprint fp;
    fp.f = (float)(fl & 255) * 0.00390625f;
    if (lo >= mips - 1) { lo = mips - 1; fp.f = 0.0f; }
    fp.l0 = level_taps<POT>(w, h, lo, uv.x, uv.y);
    fp.l1 = level_taps<POT>(w, h, min(lo + 1, mips - 1), uv.x, uv.y);     // unused (weight 0) when f == 0
    return fp;
}

VQD float4 dec8(uint32_t q) { return make_float4((float)(q & 255u), (float)((q >> 8) & 255u), (float)((q >> 16) & 255u), (float)(q >> 24)); }

// bilinear blend of one level in byte units (exact: 8-bit weights x 8-bit texels fit binary32); same FMA chain as blend4
struct Taps4 { uint32_t a, b, c, d; };
template <bool PAIRS> VQD Taps4 load_taps(const uint32_t* __restrict__ t, const LevelTaps& k) {
    Taps4 q;
    // 32-bit byte offsets from the wave-uniform chain pointer (a chain is < 4 GB): global_load with SGPR base + VGPR offset
    const char* b = (const char*)t;
    if (PAIRS) {                                                     // x1 == x0 + 1 in every lane: two 8-byte loads
        const TexelPair p0 = *(const TexelPair*)(b + ((k.row0 + (uint32_t)k.x0) << 2)), p1 = *(const TexelPair*)(b + ((k.row1 + (uint32_t)k.x0) << 2));
        q.a = p0.a; q.b = p0.b; q.c = p1.a; q.d = p1.b;
    } else {
        q.a = *(const uint32_t*)(b + ((k.row0 + (uint32_t)k.x0) << 2)); q.b = *(const uint32_t*)(b + ((k.row0 + (uint32_t)k.x1) << 2));
        q.c = *(const uint32_t*)(b + ((k.row1 + (uint32_t)k.x0) << 2)); q.d = *(const uint32_t*)(b + ((k.row1 + (uint32_t)k.x1) << 2));
    }
    return q;
}
VQD float4 blend_taps(const Taps4& q, const LevelTaps& k) {
    const float4 c00 = dec8(q.a), c10 = dec8(q.b), c01 = dec8(q.c), c11 = dec8(q.d);
    float4 r;
    r.x = fma_(k.w11, c11.x, fma_(k.w01, c01.x, fma_(k.w10, c10.x, k.w00 * c00.x)));
    r.y = fma_(k.w11, c11.y, fma_(k.w01, c01.y, fma_(k.w10, c10.y, k.w00 * c00.y)));
    r.z = fma_(k.w11, c11.z, fma_(k.w01, c01.z, fma_(k.w10, c10.z, k.w00 * c00.z)));
    r.w = fma_(k.w11, c11.w, fma_(k.w01, c01.w, fma_(k.w10, c10.w, k.w00 * c00.w)));     // alpha: read by the ENABLE_ALPHA_MASK discard test (:237-240)
    return r;
}

constexpr float kRcp255 = 0.0039215688593685627f;                   // RN(1/255) = rcp(255.0f)

// The alpha channel of gbuffer.hip's fetch() for one lane, with no ballot and no paired load: callable from divergent code. The second level is read only where
// this lane blends it; where f == 0 the wave-level form computes fma(0, b, 1 * a) == a, so the bits are the same. texels != NULL.
VQD float fetch_lane_alpha(const void* texels, const Footprint& fp) {
    const uint32_t* t = (const uint32_t*)texels;
    float r = blend_taps(load_taps<false>(t, fp.l0), fp.l0).w;
    if (fp.f != 0.0f) {
        const float b = blend_taps(load_taps<false>(t, fp.l1), fp.l1).w;
        const float f = fp.f, g = 1.0f - f;
        r = fma_(f, b, g * r);
    }
    return r * kRcp255;
}
// SampleLevel(..., 0) under a TRILINEAR_WRAP sampler: the bilinear WRAP fetch of level 0 (fetch() with f == 0), alpha channel
VQD float fetch_lane_alpha_level0(const void* texels, int w, int h, float u, float v) {
    const bool pot = ((w & (w - 1)) | (h & (h - 1))) == 0;
    const LevelTaps k = pot ? level_taps<true>(w, h, 0, u, v) : level_taps<false>(w, h, 0, u, v);
    return blend_taps(load_taps<false>((const uint32_t*)texels, k), k).w * kRcp255;
}
// the same fetch, red channel: texHeightmap.SampleLevel(LinearSamplerTess, uv, 0).r of the five vertex stages' CalcHeightOffset (displace.hip; §7.22 H2).
// Any u, v is safe: fixed8 turns NaN into 0 and clamps, WRAP brings every tap inside level 0.
VQD float fetch_lane_red_level0(const void* texels, int w, int h, float u, float v) {
    const bool pot = ((w & (w - 1)) | (h & (h - 1))) == 0;
    const LevelTaps k = pot ? level_taps<true>(w, h, 0, u, v) : level_taps<false>(w, h, 0, u, v);
    return blend_taps(load_taps<false>((const uint32_t*)texels, k), k).x * kRcp255;
}

} // namespace vqk
