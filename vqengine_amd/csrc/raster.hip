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
// vq_raster.h holds what this file shares with raster_view.hip: vertex stage, clipper, snap, fan walk and boxes, slot reservation, side record, binning, triangle
// setup and the coverage test. Here: the vertex with its world position, LINEAR_DEPTH, the five-uint4 record, the view table with its counters, the 32-bit tile.
#include "vq_raster.h"
#include "vq_raster_mask.h"

namespace vqk {
namespace {

constexpr int kSetupLanes = 256;
constexpr int kFillLanes = 256;
constexpr int kMaxPoly = 8;                       // a triangle against five planes: at most 3 + 5 vertices

struct RVert { float cx, cy, cz, cw, wx, wy, wz; };

__global__ void __launch_bounds__(64) k_raster_begin(uint32_t* counters, int numViews) {
    if ((int)threadIdx.x < numViews) counters[threadIdx.x] = 0u;
}

// JOB = RasterMaskedJob (§7.19): a draw with a maskSlot also writes its triangle's side record and stamps its records with 1 + the side record's index; with
// JOB = RasterJob this is the code it was.
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
    uint32_t emitMask = 0;                       // bit k: fan triangle (0, k + 1, k + 2) is emitted
    uint32_t maskSlot = 0u, firstMasked = 0u;
    if constexpr (MASKED) { maskSlot = job.maskSlot; firstMasked = job.firstMasked; }
    const bool masked = maskSlot != 0u;
    float mc[9], muv[6];                         // MASKED: the side record's fifteen floats
    if (live) {
        const uint32_t inst = (uint32_t)(t / job.numTris), tri = (uint32_t)(t % job.numTris);
        uint32_t idx[3];
        bool ok = fetchTriangle(job.indices, job.indexBits, tri, job.numVertices, idx);
        if (ok) {
            const VQ_matrix& M = job.wvp[inst];
            for (int k = 0; k < 3; ++k) {
                const float* p = (const float*)(job.positions + (size_t)idx[k] * job.strideBytes);
                float xyz[3], c[4];
                ok = clipPosition(p, M, xyz, c) && ok;
                RVert v; v.cx = c[0]; v.cy = c[1]; v.cz = c[2]; v.cw = c[3]; v.wx = v.wy = v.wz = 0.0f;
                if (lin) { const VQ_matrix& W = job.world[inst]; v.wx = mulPoint(xyz, W, 0); v.wy = mulPoint(xyz, W, 1); v.wz = mulPoint(xyz, W, 2); }
                poly[k] = v;
                if (masked) { mc[3 * k] = c[0]; mc[3 * k + 1] = c[1]; mc[3 * k + 2] = c[3]; muv[2 * k] = p[9]; muv[2 * k + 1] = p[10]; }    // uv at byte 36 (stride >= 44: the host checks)
            }
        }
        if (ok) {
            const int n = clipPolygon<5>(poly, 3, [lin](RVert& r, const RVert& I, const RVert& O, float t) {
                if (lin) { r.wx = I.wx + t * (O.wx - I.wx); r.wy = I.wy + t * (O.wy - I.wy); r.wz = I.wz + t * (O.wz - I.wz); }
                else { r.wx = r.wy = r.wz = 0.0f; }
            });
            const float half = 0.5f * (float)view.dim;
            bool vok[kMaxPoly];
            for (int i = 0; i < kMaxPoly; ++i) {
                if (i >= n) break;
                const RVert& v = poly[i];
                vok[i] = snapVertex(v.cx, v.cy, v.cw, half, half, sx[i], sy[i]);
                dz[i] = lin ? fdiv_(1.0f, v.cw) : fdiv_(v.cz, v.cw);
            }
            emitMask = fanMask<kMaxPoly>(sx, sy, vok, n, job.cullMode, view.dim, view.dim, 1);
        }
    }
    const uint32_t mine = (uint32_t)__builtin_popcount(emitMask);
    const uint32_t place = reserveSlots(mine, &counters[job.view], sCount, sBase);
    if (!mine) return;
    uint32_t mk = 0u;
    if constexpr (MASKED) if (masked) mk = writeMaskSide(maskArgsOf(mask...), (uint64_t)firstMasked + t, mc, muv, maskSlot - 1u);
    uint64_t slot = (uint64_t)sBase + place;
    for (int k = 0; k + 2 < kMaxPoly; ++k) {
        if (!(emitMask >> k & 1u)) continue;
        if (slot >= view.recCap) break;                             // cannot happen (the region holds six records per instanced triangle); never write past it
        const int a = 0, b = k + 1, c = k + 2;
        const uint64_t g = view.recBase + slot;
        fanBox(sx, sy, k, view.dim, view.dim, 1, boxes[g]);
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
        binRecords(vb, count, base, tx0, ty0, tx1, ty1, queue, qn);
        __syncthreads();
        const uint32_t nq = qn;
        for (uint32_t q = wave; q < nq; q += kFillLanes / 64) {
            const uint32_t rec = queue[q];
            const uint2 bb = vb[rec];
            const uint4 r0 = vr[(size_t)rec * 5], r1 = vr[(size_t)rec * 5 + 1];
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
            const TileBox tb(bb, tx0, ty0, tx1, ty1);
            const TriSetup ts((int)r0.x, (int)r0.y, (int)r0.z, (int)r0.w, (int)r1.x, (int)r1.y);
            for (int p = lane; p < tb.npix; p += 64) {
                const int i = tb.bx0 + p % tb.bw, j = tb.by0 + p / tb.bw;
                int64_t E0, E1, E2;
                if (!ts.covers(256 * i + 128, 256 * j + 128, E0, E1, E2)) continue;
                if constexpr (MASKED) { if (alphaTest && maskDiscardShadow(mt, i, j, view.dim)) continue; }         // LINEAR_DEPTH is computed after the discard
                const float b1 = fdiv_((float)E1, ts.fA), b2 = fdiv_((float)E2, ts.fA);
                float d;
                if (!lin) {
                    d = (d0 + b1 * (d1 - d0)) + b2 * (d2 - d0);
                } else {
                    const float b0 = fdiv_((float)E0, ts.fA);
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
template <class JOB, class... MA>
hipError_t launch_raster_setup(hipStream_t s, const JOB* jobs, int numJobs, uint32_t blocks, const RasterView* views, uint32_t* counters, void* boxes, void* records, const MA&... mask) {
    hipLaunchKernelGGL((k_raster_setup<JOB, MA...>), dim3(blocks), dim3(kSetupLanes), 0, s, jobs, numJobs, views, counters, (uint2*)boxes, (uint4*)records, mask...);
    return hipGetLastError();
}
template <class... MA>
hipError_t launch_raster_fill(hipStream_t s, const RasterView* views, int numViews, uint32_t blocks, int tile, const uint32_t* counters, const void* boxes, const void* records, const MA&... mask) {
    if (tile == 64) hipLaunchKernelGGL((k_raster_fill<64, MA...>), dim3(blocks), dim3(kFillLanes), 0, s, views, numViews, counters, (const uint2*)boxes, (const uint4*)records, mask...);
    else            hipLaunchKernelGGL((k_raster_fill<32, MA...>), dim3(blocks), dim3(kFillLanes), 0, s, views, numViews, counters, (const uint2*)boxes, (const uint4*)records, mask...);
    return hipGetLastError();
}
// the opaque and the masked form of each (capi.hip calls them with or without the trailing MaskArgs)
template hipError_t launch_raster_setup(hipStream_t, const RasterJob*, int, uint32_t, const RasterView*, uint32_t*, void*, void*);
template hipError_t launch_raster_setup(hipStream_t, const RasterMaskedJob*, int, uint32_t, const RasterView*, uint32_t*, void*, void*, const MaskArgs&);
template hipError_t launch_raster_fill(hipStream_t, const RasterView*, int, uint32_t, int, const uint32_t*, const void*, const void*);
template hipError_t launch_raster_fill(hipStream_t, const RasterView*, int, uint32_t, int, const uint32_t*, const void*, const void*, const MaskArgs&);

} // namespace vqk
