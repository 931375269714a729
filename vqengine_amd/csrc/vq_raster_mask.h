// vq_raster_mask.h — the alpha test of the "_AlphaMasked" PSO permutations inside the two fill kernels (raster.hip, raster_view.hip): docs/DESIGN_DETAILS.md §7.19
// M1 .. M4; tests/masked_depth_ref.py states it in numpy. Everything here is lane-local (the fill loops are divergent): no ballot, no cross-lane operation.
//   M2  uv at a pixel centre: §7.18 I2 / I3 — binary64 weights from the unclipped triangle's (x, y, w), one rounding to binary32
//   M3  scene depth: uv * uvScaleOffset, derivatives from helper lanes (the same primitive at (i ^ 1, j) and (i, j ^ 1)), the trilinear WRAP fetch of gbuffer.hip
//   M4  shadow: the raw uv, the bilinear WRAP fetch of level 0
#pragma once
#include "vq_raster.h"
#include "vq_tex8.h"

namespace vqk {
using namespace vqd;

VQD const MaskArgs& maskArgsOf(const MaskArgs& m) { return m; }     // the one element of a kernel's mask parameter pack

// A masked record as the fill loop holds it: the three sub-determinants of each I2 weight (they depend on the triangle alone), the uv, the material's entry.
struct MaskUv {                        // the part M2 reads: also what the quad resolve of raster_attr.hip (§7.20 Q1) fills for its helper lanes
    double P[3], Q[3], R[3];          // k_n = (X * P[n] - Y * Q[n]) + R[n]
    float u[3], v[3];
};
struct MaskTri : MaskUv {
    MaskTex tex;
};

// false for an unstamped record (mk == 0: an opaque draw) and for an index out of range — cannot happen, setup wrote what it counted; the record is then opaque
VQD bool loadMaskTri(const MaskArgs& m, uint32_t mk, MaskTri& t) {
    if (mk == 0u || (uint64_t)(mk - 1u) >= m.sideCap) return false;
    const uint4* s = (const uint4*)(m.side + (mk - 1u));
    const uint4 s0 = s[0], s1 = s[1], s2 = s[2], s3 = s[3];
    if (s3.w >= m.tableCap) return false;
    const double x0 = __uint_as_float(s0.x), y0 = __uint_as_float(s0.y), w0 = __uint_as_float(s0.z);
    const double x1 = __uint_as_float(s0.w), y1 = __uint_as_float(s1.x), w1 = __uint_as_float(s1.y);
    const double x2 = __uint_as_float(s1.z), y2 = __uint_as_float(s1.w), w2 = __uint_as_float(s2.x);
    // §7.18 I2: D(a, b) = (X (ya wb - wa yb) - Y (xa wb - wa xb)) + (xa yb - ya xb); k0 = D(1, 2), k1 = D(2, 0), k2 = D(0, 1)
    t.P[0] = y1 * w2 - w1 * y2; t.Q[0] = x1 * w2 - w1 * x2; t.R[0] = x1 * y2 - y1 * x2;
    t.P[1] = y2 * w0 - w2 * y0; t.Q[1] = x2 * w0 - w2 * x0; t.R[1] = x2 * y0 - y2 * x0;
    t.P[2] = y0 * w1 - w0 * y1; t.Q[2] = x0 * w1 - w0 * x1; t.R[2] = x0 * y1 - y0 * x1;
    t.u[0] = __uint_as_float(s2.y); t.v[0] = __uint_as_float(s2.z);
    t.u[1] = __uint_as_float(s2.w); t.v[1] = __uint_as_float(s3.x);
    t.u[2] = __uint_as_float(s3.y); t.v[2] = __uint_as_float(s3.z);
    t.tex = m.table[s3.w];
    return true;
}

// M2: the primitive's uv at the pixel centre (X, Y), which may lie outside the primitive (extrapolation)
VQD float2 maskUvAt(const MaskUv& t, double X, double Y) {
    const double k0 = (X * t.P[0] - Y * t.Q[0]) + t.R[0], k1 = (X * t.P[1] - Y * t.Q[1]) + t.R[1], k2 = (X * t.P[2] - Y * t.Q[2]) + t.R[2];
    const double den = (k0 + k1) + k2;
    const double l1 = k1 / den, l2 = k2 / den;
    const double u0 = t.u[0], u1 = t.u[1], u2 = t.u[2], v0 = t.v[0], v1 = t.v[1], v2 = t.v[2];
    return make_float2((float)((u0 + l1 * (u1 - u0)) + l2 * (u2 - u0)), (float)((v0 + l1 * (v1 - v0)) + l2 * (v2 - v0)));     // I3: one rounding
}

// M3 (DepthPrePass.hlsl:155-161 under ENABLE_ALPHA_MASK; the host enters only materials with HasDiffuseMap into the table): true = discard
VQD bool maskDiscardScene(const MaskTri& t, int i, int j, int W, int H) {
    const MaskTex& x = t.tex;
    if (!x.texels) return true;                                       // null SRV: samples 0
    const double X = pixelCentreX(i, W), Y = pixelCentreY(j, H);        // the quotients of the own centre serve both helper lanes
    const float2 o = maskUvAt(t, X, Y), h = maskUvAt(t, pixelCentreX(i ^ 1, W), Y), v = maskUvAt(t, X, pixelCentreY(j ^ 1, H));
    const float2 uv = make_float2(o.x * x.sx + x.ox, o.y * x.sy + x.oy);                          // as produce_record (gbuffer.hip) evaluates it
    const float hu = h.x * x.sx + x.ox, hv = h.y * x.sy + x.oy, vu = v.x * x.sx + x.ox, vv = v.y * x.sy + x.oy;
    const float2 ddx = (i & 1) ? make_float2(uv.x - hu, uv.y - hv) : make_float2(hu - uv.x, hv - uv.y);
    const float2 ddy = (j & 1) ? make_float2(uv.x - vu, uv.y - vv) : make_float2(vu - uv.x, vv - uv.y);
    const bool pot = ((x.width & (x.width - 1)) | (x.height & (x.height - 1))) == 0;
    const Footprint fp = pot ? make_footprint<true>(x.width, x.height, x.mips, uv, ddx, ddy, 0.0f)
                             : make_footprint<false>(x.width, x.height, x.mips, uv, ddx, ddy, 0.0f);
    return fetch_lane_alpha(x.texels, fp) < 0.01f;
}

// M4 (ShadowDepthPass.hlsl:136-140): no HasDiffuseMap test, no uv transform; true = discard
VQD bool maskDiscardShadow(const MaskTri& t, int i, int j, int dim) {
    const MaskTex& x = t.tex;
    if (!x.texels) return true;
    const float2 uv = maskUvAt(t, pixelCentreX(i, dim), pixelCentreY(j, dim));
    return fetch_lane_alpha_level0(x.texels, x.width, x.height, uv.x, uv.y) < 0.01f;
}

} // namespace vqk
