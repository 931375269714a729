// raster.hip — vqhip_shadow_depth: the depth-only rasteriser that produces the R32F shadow maps vqhip_forward_lighting* reads (ShadowDepthPass.hlsl through
// the shadow PSOs of PipelineStateObjects.cpp:1697-1741). docs/DESIGN_DETAILS.md §7.16 is the contract (R1 .. R6); tests/shadow_raster_ref.py states it in numpy.
//   k_raster_begin : zeroes the per-view record counters (a kernel, not a memset node; the work buffer may hold anything)
//   k_raster_setup : one lane per (draw, instance, triangle): vertex stage, Sutherland-Hodgman against five planes, viewport, snap, cull; appends up to six
//                    records per triangle to its view's region of the work buffer (one global atomicAdd per workgroup, lanes take their places in LDS)
//   k_raster_fill  : one workgroup per (view, tile): the tile's depths live in LDS at 1.0; the group walks the view's bounding boxes 256 at a time, queues the
//                    records that touch the tile, and each wave rasterises queued records with LDS atomicMin on the bits (every value is >= +0, so unsigned
//                    order is float order); then one coalesced store of the tile. No global atomics on the maps, no clear pass.
// Every loop bound is dim, a record count clamped to the region's capacity, or a constant: nothing a vertex value can stretch.
// vqhip_shadow_masked_depth (§7.19; tests/masked_depth_ref.py) launches the <.., MaskArgs> instantiations of both kernels when a draw of the call is alpha-tested: the
// same two bodies with the "_AlphaMasked" pixel shader's discard (ShadowDepthPass.hlsl:136-140) in front of the minimum; vq_raster_mask.h holds the test.
#include "vq_internal.h"
#include "vq_devmath.h"
#include "vq_raster_mask.h"

namespace vqk {
using namespace vqd;
namespace {

constexpr int kSetupLanes = 256;
constexpr int kFillLanes = 256;
constexpr int kMaxPoly = 8;                       // a triangle against five planes: at most 3 + 5 vertices (§7.16 R2 discards what a rounding accident adds)
constexpr float kSnapLimit = 16777216.0f;         // 2^24: a vertex whose p * 256 is NaN or beyond drops its fan triangle; edge products then stay below 2^52

struct RVert { float cx, cy, cz, cw, wx, wy, wz; };

VQD float sat01(float x) { return x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f; }    // the contract's saturate: NaN -> 0, -0 -> +0

VQD float planeDist(const RVert& v, int plane) {
    switch (plane) {
        case 0:  return v.cw - 0x1p-24f;
        case 1:  return v.cw + v.cx;
        case 2:  return v.cw - v.cx;
        case 3:  return v.cw + v.cy;
        default: return v.cw - v.cy;
    }
}
// from the inside endpoint I towards the outside endpoint O: both triangles of a shared edge compute the same vertex
VQD RVert clipVertex(const RVert& I, const RVert& O, float dI, float dO, bool withWorld) {
    const float t = fdiv_(dI, dI - dO);
    RVert r;
    r.cx = I.cx + t * (O.cx - I.cx); r.cy = I.cy + t * (O.cy - I.cy); r.cz = I.cz + t * (O.cz - I.cz); r.cw = I.cw + t * (O.cw - I.cw);
    if (withWorld) { r.wx = I.wx + t * (O.wx - I.wx); r.wy = I.wy + t * (O.wy - I.wy); r.wz = I.wz + t * (O.wz - I.wz); }
    else { r.wx = r.wy = r.wz = 0.0f; }
    return r;
}
VQD bool finite_(float x) { return __builtin_fabsf(x) <= 3.4028234663852886e38f; }

VQD int64_t edgeFn(int xj, int yj, int xk, int yk, int px, int py) {
    return (int64_t)(xj - px) * (int64_t)(yk - py) - (int64_t)(xk - px) * (int64_t)(yj - py);
}
// first / last texel whose sample 256 i + 128 lies in [lo, hi] (floor division: the operands may be negative)
VQD int texelCeil(int v)  { return (v - 128 + 255) >> 8; }
VQD int texelFloor(int v) { return (v - 128) >> 8; }

__global__ void __launch_bounds__(64) k_raster_begin(uint32_t* counters, int numViews) {
    if ((int)threadIdx.x < numViews) counters[threadIdx.x] = 0u;
}

// JOB = RasterMaskedJob (§7.19): a draw with a maskSlot also writes its triangle's side record (the unclipped clip-space x, y, w and the uv of the three vertices,
// the slot) and stamps its records with 1 + the side record's index; with JOB = RasterJob this is the code it was.
// The mask arguments are a parameter pack so that the opaque instantiation keeps the parameter list (and the code) it had: MA = {} or {MaskArgs}.
template <class JOB, class... MA>
__global__ void __launch_bounds__(kSetupLanes) k_raster_setup(const JOB* __restrict__ jobs, int numJobs, const RasterView* __restrict__ views,
                                                              uint32_t* __restrict__ counters, uint2* __restrict__ boxes, uint4* __restrict__ records, MA... mask) {
    constexpr bool MASKED = sizeof...(MA) != 0;
    __shared__ uint32_t sCount, sBase;
    // the block's job: the last one whose firstBlock is <= blockIdx.x (block-uniform binary search; numJobs bounds it)
    int lo = 0, hi = numJobs - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (jobs[mid].firstBlock <= blockIdx.x) lo = mid; else hi = mid - 1; }
    const JOB job = jobs[lo];
    const RasterView view = views[job.view];
    if (threadIdx.x == 0) sCount = 0u;
    __syncthreads();

    const uint64_t t = (uint64_t)(blockIdx.x - job.firstBlock) * kSetupLanes + threadIdx.x;
    const bool live = t < (uint64_t)job.numTris * job.numInstances;
    const bool lin = view.linear != 0;
    int sx[kMaxPoly], sy[kMaxPoly];
    float dz[kMaxPoly];                          // z / w (linearDepth 0) or 1 / w (linearDepth 1)
    RVert poly[kMaxPoly];
    int n = 0;
    uint32_t emitMask = 0;                       // bit k: fan triangle (0, k + 1, k + 2) is emitted
    uint32_t maskSlot = 0u, firstMasked = 0u;
    if constexpr (MASKED) { maskSlot = job.maskSlot; firstMasked = job.firstMasked; }
    const bool masked = maskSlot != 0u;
    float mc[9], muv[6];                         // MASKED: the side record's fifteen floats
    if (live) {
        const uint32_t inst = (uint32_t)(t / job.numTris), tri = (uint32_t)(t % job.numTris);
        uint32_t idx[3];
        bool ok = true;
        for (int k = 0; k < 3; ++k) {
            idx[k] = job.indexBits == 16 ? (uint32_t)((const uint16_t*)job.indices)[(size_t)tri * 3 + k] : ((const uint32_t*)job.indices)[(size_t)tri * 3 + k];
            ok = ok && idx[k] < job.numVertices;                    // an index past the vertex buffer drops the triangle
        }
        if (ok) {
            const VQ_matrix& M = job.wvp[inst];
            for (int k = 0; k < 3; ++k) {
                const float* p = (const float*)(job.positions + (size_t)idx[k] * job.strideBytes);
                const float x = p[0], y = p[1] + 0.0f, z = p[2];    // the null heightmap's + 0.0f (ShadowDepthPass.hlsl:84)
                float c[4];
                for (int j = 0; j < 4; ++j) c[j] = ((x * M.m[0][j] + y * M.m[1][j]) + z * M.m[2][j]) + 1.0f * M.m[3][j];
                RVert v; v.cx = c[0]; v.cy = c[1]; v.cz = c[2]; v.cw = c[3]; v.wx = v.wy = v.wz = 0.0f;
                if (lin) {
                    const VQ_matrix& W = job.world[inst];
                    v.wx = ((x * W.m[0][0] + y * W.m[1][0]) + z * W.m[2][0]) + 1.0f * W.m[3][0];
                    v.wy = ((x * W.m[0][1] + y * W.m[1][1]) + z * W.m[2][1]) + 1.0f * W.m[3][1];
                    v.wz = ((x * W.m[0][2] + y * W.m[1][2]) + z * W.m[2][2]) + 1.0f * W.m[3][2];
                }
                ok = ok && finite_(c[0]) && finite_(c[1]) && finite_(c[2]) && finite_(c[3]);
                poly[k] = v;
                if (masked) { mc[3 * k] = c[0]; mc[3 * k + 1] = c[1]; mc[3 * k + 2] = c[3]; muv[2 * k] = p[9]; muv[2 * k + 1] = p[10]; }    // uv at byte 36 (stride >= 44: the host checks)
            }
        }
        if (ok) {
            n = 3;
            for (int plane = 0; plane < 5; ++plane) {
                RVert out[kMaxPoly];
                int m = 0;
                for (int i = 0; i < kMaxPoly; ++i) {
                    if (i >= n) break;
                    const RVert& a = poly[i];
                    const RVert& b = poly[i + 1 < n ? i + 1 : 0];
                    const float da = planeDist(a, plane), db = planeDist(b, plane);
                    const bool ina = da >= 0.0f, inb = db >= 0.0f;
                    if (ina) {
                        if (m < kMaxPoly) out[m++] = a;
                        if (!inb && m < kMaxPoly) out[m++] = clipVertex(a, b, da, db, lin);
                    } else if (inb) {
                        if (m < kMaxPoly) out[m++] = clipVertex(b, a, db, da, lin);
                    }
                }
                n = m;
                for (int i = 0; i < kMaxPoly; ++i) if (i < n) poly[i] = out[i];
            }
            if (n < 3) n = 0;
            const float half = 0.5f * (float)view.dim;
            bool vok[kMaxPoly];
            for (int i = 0; i < kMaxPoly; ++i) {
                if (i >= n) break;
                const RVert& v = poly[i];
                const float nx = fdiv_(v.cx, v.cw), ny = fdiv_(v.cy, v.cw);
                const float fx = ((nx + 1.0f) * half) * 256.0f, fy = ((1.0f - ny) * half) * 256.0f;
                vok[i] = __builtin_fabsf(fx) <= kSnapLimit && __builtin_fabsf(fy) <= kSnapLimit;      // false for NaN
                sx[i] = vok[i] ? (int)__builtin_rintf(fx) : 0;
                sy[i] = vok[i] ? (int)__builtin_rintf(fy) : 0;
                dz[i] = lin ? fdiv_(1.0f, v.cw) : fdiv_(v.cz, v.cw);
            }
            for (int k = 0; k + 2 < kMaxPoly; ++k) {
                if (k + 2 >= n) break;
                if (!(vok[0] && vok[k + 1] && vok[k + 2])) continue;
                const int64_t A = edgeFn(sx[k + 1], sy[k + 1], sx[k + 2], sy[k + 2], sx[0], sy[0]);
                if (A == 0) continue;
                if ((A > 0 && job.cullMode == VQHIP_CULL_FRONT) || (A < 0 && job.cullMode == VQHIP_CULL_BACK)) continue;
                const int xmin = min(sx[0], min(sx[k + 1], sx[k + 2])), xmax = max(sx[0], max(sx[k + 1], sx[k + 2]));
                const int ymin = min(sy[0], min(sy[k + 1], sy[k + 2])), ymax = max(sy[0], max(sy[k + 1], sy[k + 2]));
                const int i0 = max(texelCeil(xmin), 0), i1 = min(texelFloor(xmax), view.dim - 1);
                const int j0 = max(texelCeil(ymin), 0), j1 = min(texelFloor(ymax), view.dim - 1);
                if (i0 > i1 || j0 > j1) continue;                   // no sample inside the box: nothing to rasterise
                emitMask |= 1u << k;
            }
        }
    }
    const uint32_t mine = (uint32_t)__builtin_popcount(emitMask);
    uint32_t place = 0;
    if (mine) place = atomicAdd(&sCount, mine);                     // LDS
    __syncthreads();
    if (threadIdx.x == 0) sBase = sCount ? atomicAdd(&counters[job.view], sCount) : 0u;
    __syncthreads();
    if (!mine) return;
    uint32_t mk = 0u;
    if constexpr (MASKED) if (masked) {
        const MaskArgs& m = maskArgsOf(mask...);
        const uint64_t at = (uint64_t)firstMasked + t;              // below the call's masked instanced triangles = sideCap
        if (at < m.sideCap) {
            uint4* sr = (uint4*)(m.side + at);
            sr[0] = make_uint4(__float_as_uint(mc[0]), __float_as_uint(mc[1]), __float_as_uint(mc[2]), __float_as_uint(mc[3]));
            sr[1] = make_uint4(__float_as_uint(mc[4]), __float_as_uint(mc[5]), __float_as_uint(mc[6]), __float_as_uint(mc[7]));
            sr[2] = make_uint4(__float_as_uint(mc[8]), __float_as_uint(muv[0]), __float_as_uint(muv[1]), __float_as_uint(muv[2]));
            sr[3] = make_uint4(__float_as_uint(muv[3]), __float_as_uint(muv[4]), __float_as_uint(muv[5]), maskSlot - 1u);
            mk = (uint32_t)at + 1u;
        }
    }
    uint64_t slot = (uint64_t)sBase + place;
    for (int k = 0; k + 2 < kMaxPoly; ++k) {
        if (!(emitMask >> k & 1u)) continue;
        if (slot >= view.recCap) break;                             // cannot happen (the region holds six records per instanced triangle); never write past it
        const int a = 0, b = k + 1, c = k + 2;
        const int xmin = min(sx[a], min(sx[b], sx[c])), xmax = max(sx[a], max(sx[b], sx[c]));
        const int ymin = min(sy[a], min(sy[b], sy[c])), ymax = max(sy[a], max(sy[b], sy[c]));
        const uint32_t i0 = (uint32_t)max(texelCeil(xmin), 0), i1 = (uint32_t)min(texelFloor(xmax), view.dim - 1);
        const uint32_t j0 = (uint32_t)max(texelCeil(ymin), 0), j1 = (uint32_t)min(texelFloor(ymax), view.dim - 1);
        const uint64_t g = view.recBase + slot;
        boxes[g] = make_uint2(i0 | i1 << 16, j0 | j1 << 16);
        uint4* r = records + g * 5;
        r[0] = make_uint4((uint32_t)sx[a], (uint32_t)sy[a], (uint32_t)sx[b], (uint32_t)sy[b]);
        r[1] = make_uint4((uint32_t)sx[c], (uint32_t)sy[c], __float_as_uint(dz[a]), __float_as_uint(dz[b]));
        r[2] = make_uint4(__float_as_uint(dz[c]), __float_as_uint(poly[a].wx), __float_as_uint(poly[a].wy), __float_as_uint(poly[a].wz));
        r[3] = make_uint4(__float_as_uint(poly[b].wx), __float_as_uint(poly[b].wy), __float_as_uint(poly[b].wz), __float_as_uint(poly[c].wx));
        r[4] = make_uint4(__float_as_uint(poly[c].wy), __float_as_uint(poly[c].wz), mk, 0u);
        ++slot;
    }
}

// MASKED (§7.19): a covered texel of a stamped record runs the alpha test of ShadowDepthPass.hlsl:136-140 (pixel = texel) before its depth is computed
template <int T, class... MA>
__global__ void __launch_bounds__(kFillLanes) k_raster_fill(const RasterView* __restrict__ views, int numViews, const uint32_t* __restrict__ counters,
                                                            const uint2* __restrict__ boxes, const uint4* __restrict__ records, MA... mask) {
    constexpr bool MASKED = sizeof...(MA) != 0;
    __shared__ uint32_t tile[T * T];
    __shared__ uint32_t queue[kFillLanes];
    __shared__ uint32_t qn;
    int v = 0;
    for (int k = 1; k < numViews; ++k) if (views[k].firstFillBlock <= blockIdx.x) v = k;
    const RasterView view = views[v];
    const int tilesX = (view.dim + T - 1) / T;
    const int local = (int)(blockIdx.x - view.firstFillBlock);
    const int tx0 = (local % tilesX) * T, ty0 = (local / tilesX) * T;
    const int tx1 = min(tx0 + T, view.dim) - 1, ty1 = min(ty0 + T, view.dim) - 1;
    for (int i = threadIdx.x; i < T * T; i += kFillLanes) tile[i] = 0x3f800000u;
    if (threadIdx.x == 0) qn = 0u;
    __syncthreads();

    const uint64_t cnt64 = counters[v];
    const uint32_t count = (uint32_t)(cnt64 < view.recCap ? cnt64 : view.recCap);
    const uint2* vb = boxes + view.recBase;
    const uint4* vr = records + view.recBase * 5;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool lin = view.linear != 0;
    for (uint32_t base = 0; base < count; base += kFillLanes) {
        const uint32_t r = base + threadIdx.x;
        if (r < count) {
            const uint2 bb = vb[r];
            const int i0 = (int)(bb.x & 0xffffu), i1 = (int)(bb.x >> 16), j0 = (int)(bb.y & 0xffffu), j1 = (int)(bb.y >> 16);
            if (i0 <= tx1 && i1 >= tx0 && j0 <= ty1 && j1 >= ty0) queue[atomicAdd(&qn, 1u)] = r;
        }
        __syncthreads();
        const uint32_t nq = qn;
        for (uint32_t q = wave; q < nq; q += kFillLanes / 64) {
            const uint32_t rec = queue[q];
            const uint2 bb = vb[rec];
            const uint4 r0 = vr[(size_t)rec * 5], r1 = vr[(size_t)rec * 5 + 1];
            const int x0 = (int)r0.x, y0 = (int)r0.y, x1 = (int)r0.z, y1 = (int)r0.w, x2 = (int)r1.x, y2 = (int)r1.y;
            const float d0 = __uint_as_float(r1.z), d1 = __uint_as_float(r1.w);
            const uint4 r2 = vr[(size_t)rec * 5 + 2];
            const float d2 = __uint_as_float(r2.x);
            float P0x = 0, P0y = 0, P0z = 0, P1x = 0, P1y = 0, P1z = 0, P2x = 0, P2y = 0, P2z = 0;
            MaskTri mt;
            bool alphaTest = false;
            if constexpr (MASKED) alphaTest = loadMaskTri(maskArgsOf(mask...), vr[(size_t)rec * 5 + 4].z, mt);
            if (lin) {
                const uint4 r3 = vr[(size_t)rec * 5 + 3], r4 = vr[(size_t)rec * 5 + 4];
                P0x = __uint_as_float(r2.y); P0y = __uint_as_float(r2.z); P0z = __uint_as_float(r2.w);
                P1x = __uint_as_float(r3.x); P1y = __uint_as_float(r3.y); P1z = __uint_as_float(r3.z);
                P2x = __uint_as_float(r3.w); P2y = __uint_as_float(r4.x); P2z = __uint_as_float(r4.y);
            }
            const int bx0 = max((int)(bb.x & 0xffffu), tx0), bx1 = min((int)(bb.x >> 16), tx1);
            const int by0 = max((int)(bb.y & 0xffffu), ty0), by1 = min((int)(bb.y >> 16), ty1);
            const int bw = bx1 - bx0 + 1, npix = bw * (by1 - by0 + 1);                                  // 1 .. T * T
            const int64_t A = edgeFn(x1, y1, x2, y2, x0, y0);
            const int64_t sgn = A > 0 ? 1 : -1;
            // top-left of the edge opposite each vertex, in the winding that makes the triangle clockwise on the y-down map
            auto topLeft = [&](int xa, int ya, int xb, int yb) { const int64_t dx = sgn * (xb - xa), dy = sgn * (yb - ya); return dy < 0 || (dy == 0 && dx > 0); };
            const bool tl0 = topLeft(x1, y1, x2, y2), tl1 = topLeft(x2, y2, x0, y0), tl2 = topLeft(x0, y0, x1, y1);
            const float fA = (float)A;
            for (int p = lane; p < npix; p += 64) {
                const int i = bx0 + p % bw, j = by0 + p / bw;
                const int px = 256 * i + 128, py = 256 * j + 128;
                const int64_t E0 = edgeFn(x1, y1, x2, y2, px, py), E1 = edgeFn(x2, y2, x0, y0, px, py), E2 = edgeFn(x0, y0, x1, y1, px, py);
                const int64_t s0 = sgn * E0, s1 = sgn * E1, s2 = sgn * E2;
                if (!((s0 > 0 || (s0 == 0 && tl0)) && (s1 > 0 || (s1 == 0 && tl1)) && (s2 > 0 || (s2 == 0 && tl2)))) continue;
                if constexpr (MASKED) { if (alphaTest && maskDiscardShadow(mt, i, j, view.dim)) continue; }         // LINEAR_DEPTH is computed after the discard
                const float b1 = fdiv_((float)E1, fA), b2 = fdiv_((float)E2, fA);
                float d;
                if (!lin) {
                    d = (d0 + b1 * (d1 - d0)) + b2 * (d2 - d0);
                } else {
                    const float b0 = fdiv_((float)E0, fA);
                    const float k0 = b0 * d0, k1 = b1 * d1, k2 = b2 * d2;
                    const float den = (k0 + k1) + k2;
                    const float X = fdiv_((k0 * P0x + k1 * P1x) + k2 * P2x, den);
                    const float Y = fdiv_((k0 * P0y + k1 * P1y) + k2 * P2y, den);
                    const float Z = fdiv_((k0 * P0z + k1 * P1z) + k2 * P2z, den);
                    const float ex = view.cam[0] - X, ey = view.cam[1] - Y, ez = view.cam[2] - Z;
                    d = fdiv_(sqrt_((ex * ex + ey * ey) + ez * ez), view.farPlane);
                }
                atomicMin(&tile[(j - ty0) * T + (i - tx0)], __float_as_uint(sat01(d)));
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) qn = 0u;
        __syncthreads();
    }
    const int w = tx1 - tx0 + 1, h = ty1 - ty0 + 1;
    for (int p = threadIdx.x; p < T * h; p += kFillLanes) {
        const int i = p % T, j = p / T;
        if (i < w) view.depth[(size_t)(ty0 + j) * view.pitch + tx0 + i] = __uint_as_float(tile[j * T + i]);
    }
}

} // namespace

hipError_t launch_raster_begin(hipStream_t s, uint32_t* counters, int numViews) {
    hipLaunchKernelGGL(k_raster_begin, dim3(1), dim3(64), 0, s, counters, numViews);
    return hipGetLastError();
}
hipError_t launch_raster_setup(hipStream_t s, const RasterJob* jobs, int numJobs, uint32_t blocks, const RasterView* views, uint32_t* counters, void* boxes, void* records) {
    hipLaunchKernelGGL(k_raster_setup<RasterJob>, dim3(blocks), dim3(kSetupLanes), 0, s, jobs, numJobs, views, counters, (uint2*)boxes, (uint4*)records);
    return hipGetLastError();
}
hipError_t launch_raster_fill(hipStream_t s, const RasterView* views, int numViews, uint32_t blocks, int tile, const uint32_t* counters, const void* boxes, const void* records) {
    if (tile == 64) hipLaunchKernelGGL(k_raster_fill<64>, dim3(blocks), dim3(kFillLanes), 0, s, views, numViews, counters, (const uint2*)boxes, (const uint4*)records);
    else            hipLaunchKernelGGL(k_raster_fill<32>, dim3(blocks), dim3(kFillLanes), 0, s, views, numViews, counters, (const uint2*)boxes, (const uint4*)records);
    return hipGetLastError();
}

hipError_t launch_raster_setup_masked(hipStream_t s, const RasterMaskedJob* jobs, int numJobs, uint32_t blocks, const RasterView* views, uint32_t* counters, void* boxes, void* records,
                                      const MaskArgs& m) {
    hipLaunchKernelGGL((k_raster_setup<RasterMaskedJob, MaskArgs>), dim3(blocks), dim3(kSetupLanes), 0, s, jobs, numJobs, views, counters, (uint2*)boxes, (uint4*)records, m);
    return hipGetLastError();
}
hipError_t launch_raster_fill_masked(hipStream_t s, const RasterView* views, int numViews, uint32_t blocks, int tile, const uint32_t* counters, const void* boxes, const void* records,
                                     const MaskArgs& m) {
    if (tile == 64) hipLaunchKernelGGL((k_raster_fill<64, MaskArgs>), dim3(blocks), dim3(kFillLanes), 0, s, views, numViews, counters, (const uint2*)boxes, (const uint4*)records, m);
    else            hipLaunchKernelGGL((k_raster_fill<32, MaskArgs>), dim3(blocks), dim3(kFillLanes), 0, s, views, numViews, counters, (const uint2*)boxes, (const uint4*)records, m);
    return hipGetLastError();
}

} // namespace vqk
