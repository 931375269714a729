// vq_raster.h — the device core of the two depth rasterisers (raster.hip: shadow maps, §7.16; raster_view.hip: the main view's depth pre-pass, §7.17): the one
// statement of D3D's rules R1 .. R4 (= V1 .. V3 without the z planes) in docs/DESIGN_DETAILS.md. The kernels, their grids, LDS arrays and record layouts stay in the
// two .hip files; what they share lives here, lane-local unless it says otherwise (reserveSlots and binRecords are called by every lane of the block).
// Every floating-point expression is written in the contract's order (-ffp-contract=off): move one, and the bit-exact tests of both rasterisers notice.
#pragma once
#include "vq_internal.h"
#include "vq_devmath.h"

namespace vqk {
using namespace vqd;

constexpr float kSnapLimit = 16777216.0f;         // 2^24: a vertex whose p * 256 is NaN or beyond drops its fan triangle; edge products then stay below 2^52

VQD float sat01(float x) { return x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f; }    // the contract's saturate: NaN -> 0, -0 -> +0
VQD bool finite_(float x) { return __builtin_fabsf(x) <= 3.4028234663852886e38f; }
VQD int64_t edgeFn(int xj, int yj, int xk, int yk, int px, int py) {
    return (int64_t)(xj - px) * (int64_t)(yk - py) - (int64_t)(xk - px) * (int64_t)(yj - py);
}
// §7.18 I2's pixel centre on one axis: (2 i + 1) / W - 1 and 1 - (2 j + 1) / H, each operation rounded once; i, j may lie outside the viewport
VQD double pixelCentreX(int i, int W) { return (double)(2 * i + 1) / (double)W - 1.0; }
VQD double pixelCentreY(int j, int H) { return 1.0 - (double)(2 * j + 1) / (double)H; }

// the three indices of triangle tri; false when one lies past the vertex buffer (the triangle is dropped)
VQD bool fetchTriangle(const void* indices, int indexBits, uint32_t tri, uint32_t numVertices, uint32_t idx[3]) {
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        idx[k] = indexBits == 16 ? (uint32_t)((const uint16_t*)indices)[(size_t)tri * 3 + k] : ((const uint32_t*)indices)[(size_t)tri * 3 + k];
        ok = ok && idx[k] < numVertices;
    }
    return ok;
}

// R1: mul(float4(p, 1), M)[j] for the position xyz the shaders multiply (clipPosition returns it)
VQD float mulPoint(const float xyz[3], const VQ_matrix& M, int j) { return ((xyz[0] * M.m[0][j] + xyz[1] * M.m[1][j]) + xyz[2] * M.m[2][j]) + 1.0f * M.m[3][j]; }
// the vertex stage of both depth shaders: c = position through wvp; false when a component is not finite
VQD bool clipPosition(const float* p, const VQ_matrix& wvp, float xyz[3], float c[4]) {
    xyz[0] = p[0]; xyz[1] = p[1] + 0.0f; xyz[2] = p[2];             // the null heightmap's + 0.0f (ShadowDepthPass.hlsl:84, DepthPrePass.hlsl:118)
    for (int j = 0; j < 4; ++j) c[j] = mulPoint(xyz, wvp, j);
    return finite_(c[0]) && finite_(c[1]) && finite_(c[2]) && finite_(c[3]);
}

template <class V> VQD float planeDist(const V& v, int plane) {
    switch (plane) {
        case 0:  return v.cw - 0x1p-24f;
        case 1:  return v.cw + v.cx;
        case 2:  return v.cw - v.cx;
        case 3:  return v.cw + v.cy;
        case 4:  return v.cw - v.cy;
        case 5:  return v.cz;                     // DepthClipEnable (the scene alone: PLANES = 7): 0 <= z
        default: return v.cw - v.cz;              //                                                 z <= w
    }
}
// from the inside endpoint I towards the outside endpoint O: both triangles of a shared edge compute the same vertex. cut(r, I, O, t) fills what V holds beyond
// the clip-space position.
template <class V, class CUT> VQD V clipVertex(const V& I, const V& O, float dI, float dO, const CUT& cut) {
    const float t = fdiv_(dI, dI - dO);
    V r;
    r.cx = I.cx + t * (O.cx - I.cx); r.cy = I.cy + t * (O.cy - I.cy); r.cz = I.cz + t * (O.cz - I.cz); r.cw = I.cw + t * (O.cw - I.cw);
    cut(r, I, O, t);
    return r;
}
// R2 / V2: Sutherland-Hodgman against planes 0 .. PLANES - 1. A triangle against k planes has at most 3 + k = MAXP vertices; what a rounding accident adds is
// discarded. Returns the number of vertices left in poly: 0, or 3 .. MAXP.
template <int PLANES, int MAXP, class V, class CUT> VQD int clipPolygon(V (&poly)[MAXP], int n, const CUT& cut) {
    for (int plane = 0; plane < PLANES; ++plane) {
        V out[MAXP];
        int m = 0;
        for (int i = 0; i < MAXP; ++i) {
            if (i >= n) break;
            const V& a = poly[i];
            const V& b = poly[i + 1 < n ? i + 1 : 0];
            const float da = planeDist(a, plane), db = planeDist(b, plane);
            const bool ina = da >= 0.0f, inb = db >= 0.0f;
            if (ina) {
                if (m < MAXP) out[m++] = a;
                if (!inb && m < MAXP) out[m++] = clipVertex(a, b, da, db, cut);
            } else if (inb) {
                if (m < MAXP) out[m++] = clipVertex(b, a, db, da, cut);
            }
        }
        n = m;
        for (int i = 0; i < MAXP; ++i) if (i < n) poly[i] = out[i];
    }
    return n < 3 ? 0 : n;
}

// R3: the viewport of 2 halfW x 2 halfH pixels, then the snap to 1/256 of a pixel; false (and 0, 0) when a coordinate is NaN or beyond kSnapLimit
VQD bool snapVertex(float cx, float cy, float cw, float halfW, float halfH, int& sx, int& sy) {
    const float nx = fdiv_(cx, cw), ny = fdiv_(cy, cw);
    const float fx = ((nx + 1.0f) * halfW) * 256.0f, fy = ((1.0f - ny) * halfH) * 256.0f;
    const bool ok = __builtin_fabsf(fx) <= kSnapLimit && __builtin_fabsf(fy) <= kSnapLimit;      // false for NaN
    sx = ok ? (int)__builtin_rintf(fx) : 0;
    sy = ok ? (int)__builtin_rintf(fy) : 0;
    return ok;
}

// first / last pixel that holds a sample coordinate in [lo, hi] on one axis: the samples of a pixel sit at 128 (1x: the shadow maps' texel centres as well) or at
// 32 .. 224 (D3D's 4x pattern, both axes) in 1/256 of a pixel from its corner; floor division by the shift (the operands may be negative)
VQD int pixelFirst(int lo, int samples) { return (lo - (samples == 1 ? 128 : 224) + 255) >> 8; }
VQD int pixelLast(int hi, int samples)  { return (hi - (samples == 1 ? 128 : 32)) >> 8; }
// the pixels of a W x H target that can hold a sample of fan triangle (0, k + 1, k + 2), packed as the boxes array holds them; false: none
VQD bool fanBox(const int* sx, const int* sy, int k, int W, int H, int samples, uint2& box) {
    const int xmin = min(sx[0], min(sx[k + 1], sx[k + 2])), xmax = max(sx[0], max(sx[k + 1], sx[k + 2]));
    const int ymin = min(sy[0], min(sy[k + 1], sy[k + 2])), ymax = max(sy[0], max(sy[k + 1], sy[k + 2]));
    const int i0 = max(pixelFirst(xmin, samples), 0), i1 = min(pixelLast(xmax, samples), W - 1);
    const int j0 = max(pixelFirst(ymin, samples), 0), j1 = min(pixelLast(ymax, samples), H - 1);
    box = make_uint2((uint32_t)i0 | (uint32_t)i1 << 16, (uint32_t)j0 | (uint32_t)j1 << 16);
    return i0 <= i1 && j0 <= j1;
}
// R4: the fan (0, k + 1, k + 2) of the clipped polygon; bit k of the result: the triangle has snapped vertices, an area, the facing the cull mode keeps and a box
template <int MAXP> VQD uint32_t fanMask(const int* sx, const int* sy, const bool* vok, int n, int cullMode, int W, int H, int samples) {
    uint32_t emitMask = 0;
    for (int k = 0; k + 2 < MAXP; ++k) {
        if (k + 2 >= n) break;
        if (!(vok[0] && vok[k + 1] && vok[k + 2])) continue;
        const int64_t A = edgeFn(sx[k + 1], sy[k + 1], sx[k + 2], sy[k + 2], sx[0], sy[0]);
        if (A == 0) continue;
        if ((A > 0 && cullMode == VQHIP_CULL_FRONT) || (A < 0 && cullMode == VQHIP_CULL_BACK)) continue;
        uint2 box;
        if (fanBox(sx, sy, k, W, H, samples, box)) emitMask |= 1u << k;
    }
    return emitMask;
}

// Block-level: every lane of the workgroup calls this once, from uniform control flow. The lanes take their places in LDS, lane 0 reserves the block's records with
// one global atomicAdd; the lane's first record is sBase + the place returned. sCount is 0 on entry (the kernel zeroes it and syncs).
VQD uint32_t reserveSlots(uint32_t mine, uint32_t* counter, uint32_t& sCount, uint32_t& sBase) {
    uint32_t place = 0;
    if (mine) place = atomicAdd(&sCount, mine);                     // LDS
    __syncthreads();
    if (threadIdx.x == 0) sBase = sCount ? atomicAdd(counter, sCount) : 0u;
    __syncthreads();
    return place;
}

// §7.19: the side record of masked triangle `at` (the unclipped clip-space x, y, w and the uv of the three vertices, the material's table entry); the stamp its
// records carry, 0 (opaque) when `at` is out of range — cannot happen: at < the call's masked instanced triangles = sideCap
VQD uint32_t writeMaskSide(const MaskArgs& m, uint64_t at, const float mc[9], const float muv[6], uint32_t slot) {
    if (at >= m.sideCap) return 0u;
    uint4* sr = (uint4*)(m.side + at);
    sr[0] = make_uint4(__float_as_uint(mc[0]), __float_as_uint(mc[1]), __float_as_uint(mc[2]), __float_as_uint(mc[3]));
    sr[1] = make_uint4(__float_as_uint(mc[4]), __float_as_uint(mc[5]), __float_as_uint(mc[6]), __float_as_uint(mc[7]));
    sr[2] = make_uint4(__float_as_uint(mc[8]), __float_as_uint(muv[0]), __float_as_uint(muv[1]), __float_as_uint(muv[2]));
    sr[3] = make_uint4(__float_as_uint(muv[3]), __float_as_uint(muv[4]), __float_as_uint(muv[5]), slot);
    return (uint32_t)at + 1u;
}

// Block-level: the fill loops' binning step. Lane threadIdx.x looks at box base + threadIdx.x and queues the record when its box touches the tile.
VQD void binRecords(const uint2* boxes, uint32_t count, uint32_t base, int tx0, int ty0, int tx1, int ty1, uint32_t* queue, uint32_t& qn) {
    const uint32_t r = base + threadIdx.x;
    if (r < count) {
        const uint2 bb = boxes[r];
        const int i0 = (int)(bb.x & 0xffffu), i1 = (int)(bb.x >> 16), j0 = (int)(bb.y & 0xffffu), j1 = (int)(bb.y >> 16);
        if (i0 <= tx1 && i1 >= tx0 && j0 <= ty1 && j1 >= ty0) queue[atomicAdd(&qn, 1u)] = r;
    }
}
// a queued record's box inside the tile: sample p of a wave's walk lies in pixel (bx0 + p % bw, by0 + p / bw); npix = 1 .. T * T
struct TileBox {
    int bx0, by0, bw, npix;
    VQD TileBox(uint2 bb, int tx0, int ty0, int tx1, int ty1) {
        bx0 = max((int)(bb.x & 0xffffu), tx0); const int bx1 = min((int)(bb.x >> 16), tx1);
        by0 = max((int)(bb.y & 0xffffu), ty0); const int by1 = min((int)(bb.y >> 16), ty1);
        bw = bx1 - bx0 + 1; npix = bw * (by1 - by0 + 1);
    }
};

// R4: a record's triangle as the fill loops hold it, and the top-left rule
struct TriSetup {
    int x0, y0, x1, y1, x2, y2;
    int64_t A, sgn;                   // twice the signed area; +1 / -1: the winding that makes the triangle clockwise on the y-down target
    bool tl0, tl1, tl2;               // the edge opposite vertex 0 / 1 / 2 is a top or a left edge in that winding
    float fA;
    VQD bool topLeft(int xa, int ya, int xb, int yb) const { const int64_t dx = sgn * (xb - xa), dy = sgn * (yb - ya); return dy < 0 || (dy == 0 && dx > 0); }
    VQD TriSetup(int x0_, int y0_, int x1_, int y1_, int x2_, int y2_) : x0(x0_), y0(y0_), x1(x1_), y1(y1_), x2(x2_), y2(y2_) {
        A = edgeFn(x1, y1, x2, y2, x0, y0);
        sgn = A > 0 ? 1 : -1;
        tl0 = topLeft(x1, y1, x2, y2); tl1 = topLeft(x2, y2, x0, y0); tl2 = topLeft(x0, y0, x1, y1);
        fA = (float)A;
    }
    // one edge at a time, and sgn * E inside the call: with the three products taken first the compiler turned an edge product of the 1x fills into a full
    // 64-bit multiply, and those kernels ran 0.4 % .. 2.9 % slower (profiles/r18a_raster_core.md)
    static VQD bool inside(int64_t s, bool tl) { return s > 0 || (s == 0 && tl); }
    // the sample at (px, py), in 1/256 of a pixel: its three edge functions (E_n: the edge opposite vertex n), and whether the triangle covers it
    VQD bool covers(int px, int py, int64_t& E0, int64_t& E1, int64_t& E2) const {
        E0 = edgeFn(x1, y1, x2, y2, px, py); E1 = edgeFn(x2, y2, x0, y0, px, py); E2 = edgeFn(x0, y0, x1, y1, px, py);
        return inside(sgn * E0, tl0) && inside(sgn * E1, tl1) && inside(sgn * E2, tl2);
    }
};

} // namespace vqk
