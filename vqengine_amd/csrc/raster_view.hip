// raster_view.hip — vqhip_scene_depth: the main view's depth pre-pass (DepthPrePass.hlsl through FDepthPrePassPSOs, PipelineStateObjects.cpp:1580-1635; drawn by
// VQRenderer::RenderDepthPrePass, SceneRendering.cpp:1265-1363) at 1 or 4 samples per pixel. docs/DESIGN_DETAILS.md §7.17 is the contract (V1 .. V5: what differs
// from §7.16's R1 .. R5); tests/scene_depth_ref.py states it in numpy.
//   k_raster_begin (raster.hip) : zeroes the record counter
//   k_scene_setup : one lane per (draw, instance, triangle): vertex stage, Sutherland-Hodgman against seven planes, the W x H viewport, snap, cull; appends up to
//                   eight records per triangle, each carrying the primitive's sequence number q (one global atomicAdd per workgroup on the counter)
//   k_scene_fill  : one workgroup per tile of T x T pixels: the tile's keys (depth bits << 32 | q, one per sample) live in LDS at the clear key; the group walks
//                   the records' boxes 256 at a time, queues those that touch the tile, and each wave rasterises queued records with the LDS 64-bit atomicMin
//                   (ds_min_u64: a minimum, so the result does not depend on the order of arrival). Then the tile is stored once: depth, primitive, and — from
//                   the pixel's own four keys — the layer masks and the layers' primitives. No global atomics on the outputs, no clear pass.
// Every loop bound is a viewport size, a record count clamped to capacity, or a constant: nothing a vertex value can stretch.
// vqhip_scene_masked_depth (§7.19; tests/masked_depth_ref.py) launches the <MaskArgs> instantiations of both kernels when a draw of the call is alpha-tested: the same
// two bodies with the "_AlphaMasked" pixel shader's discard (DepthPrePass.hlsl:155-161) in front of the minimum; vq_raster_mask.h holds the test.
#include "vq_internal.h"
#include "vq_devmath.h"
#include "vq_raster_mask.h"

namespace vqk {
using namespace vqd;
namespace {

constexpr int kSetupLanes = 256;
constexpr int kFillLanes = 256;
constexpr int kMaxPoly = 10;                      // a triangle against seven planes: at most 3 + 7 vertices (§7.17 V2 discards what a rounding accident adds)
constexpr float kSnapLimit = 16777216.0f;         // 2^24, as §7.16 R3
constexpr uint32_t kNoPrimitive = 0xffffffffu;
constexpr uint64_t kClearKey = ((uint64_t)0x3f800000u << 32) | kNoPrimitive;

struct CVert { float cx, cy, cz, cw; };

VQD float sat01(float x) { return x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f; }    // the contract's saturate: NaN -> 0, -0 -> +0

VQD float planeDist(const CVert& v, int plane) {
    switch (plane) {
        case 0:  return v.cw - 0x1p-24f;
        case 1:  return v.cw + v.cx;
        case 2:  return v.cw - v.cx;
        case 3:  return v.cw + v.cy;
        case 4:  return v.cw - v.cy;
        case 5:  return v.cz;                     // DepthClipEnable: 0 <= z
        default: return v.cw - v.cz;              //                  z <= w
    }
}
// from the inside endpoint I towards the outside endpoint O: both triangles of a shared edge compute the same vertex
VQD CVert clipVertex(const CVert& I, const CVert& O, float dI, float dO) {
    const float t = fdiv_(dI, dI - dO);
    CVert r;
    r.cx = I.cx + t * (O.cx - I.cx); r.cy = I.cy + t * (O.cy - I.cy); r.cz = I.cz + t * (O.cz - I.cz); r.cw = I.cw + t * (O.cw - I.cw);
    return r;
}
VQD bool finite_(float x) { return __builtin_fabsf(x) <= 3.4028234663852886e38f; }

VQD int64_t edgeFn(int xj, int yj, int xk, int yk, int px, int py) {
    return (int64_t)(xj - px) * (int64_t)(yk - py) - (int64_t)(xk - px) * (int64_t)(yj - py);
}
// sample s of a pixel, in 1/256 of a pixel from the pixel's corner: the centre at 1x, D3D's standard pattern at 4x
template <int S> VQD int sampleX(int s) { return S == 1 ? 128 : (s == 0 ? 96 : s == 1 ? 224 : s == 2 ? 32 : 160); }
template <int S> VQD int sampleY(int s) { return S == 1 ? 128 : 32 + 64 * s; }
// first / last pixel that holds a sample coordinate in [lo, hi] on one axis (both axes use the offsets 128, or 32 .. 224); floor division by the shift
VQD int pixelFirst(int lo, int samples) { return (lo - (samples == 1 ? 128 : 224) + 255) >> 8; }
VQD int pixelLast(int hi, int samples)  { return (hi - (samples == 1 ? 128 : 32)) >> 8; }

// MASKED (§7.19): a draw with a maskSlot also writes its triangle's side record (the unclipped clip-space x, y, w and the uv of the three vertices, the slot) and
// stamps its records with 1 + the side record's index; the opaque instantiation is the code it was.
// The mask arguments are a parameter pack so that the opaque instantiation keeps the parameter list (and the code) it had: MA = {} or {MaskArgs}.
template <class... MA>
__global__ void __launch_bounds__(kSetupLanes) k_scene_setup(const SceneDepthJob* __restrict__ jobs, int numJobs, SceneDepthArgs a, uint32_t* __restrict__ counter,
                                                             uint2* __restrict__ boxes, uint4* __restrict__ records, MA... mask) {
    constexpr bool MASKED = sizeof...(MA) != 0;
    __shared__ uint32_t sCount, sBase;
    // the block's job: the last one whose firstBlock is <= blockIdx.x (block-uniform binary search; numJobs bounds it)
    int lo = 0, hi = numJobs - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (jobs[mid].firstBlock <= blockIdx.x) lo = mid; else hi = mid - 1; }
    const SceneDepthJob job = jobs[lo];
    if (threadIdx.x == 0) sCount = 0u;
    __syncthreads();

    const uint64_t t = (uint64_t)(blockIdx.x - job.firstBlock) * kSetupLanes + threadIdx.x;
    const bool live = t < (uint64_t)job.numTris * job.numInstances;
    int sx[kMaxPoly], sy[kMaxPoly];
    float dz[kMaxPoly];                          // z / w
    int n = 0;
    uint32_t emitMask = 0;                       // bit k: fan triangle (0, k + 1, k + 2) is emitted
    const bool masked = MASKED && job.maskSlot != 0u;
    float mc[9], muv[6];                         // MASKED: the side record's fifteen floats
    if (live) {
        const uint32_t inst = (uint32_t)(t / job.numTris), tri = (uint32_t)(t % job.numTris);
        uint32_t idx[3];
        bool ok = true;
        for (int k = 0; k < 3; ++k) {
            idx[k] = job.indexBits == 16 ? (uint32_t)((const uint16_t*)job.indices)[(size_t)tri * 3 + k] : ((const uint32_t*)job.indices)[(size_t)tri * 3 + k];
            ok = ok && idx[k] < job.numVertices;                    // an index past the vertex buffer drops the triangle
        }
        CVert poly[kMaxPoly];
        if (ok) {
            const VQ_matrix& M = job.wvp[inst];
            for (int k = 0; k < 3; ++k) {
                const float* p = (const float*)(job.positions + (size_t)idx[k] * job.strideBytes);
                const float x = p[0], y = p[1] + 0.0f, z = p[2];    // the null heightmap's + 0.0f (DepthPrePass.hlsl:118)
                float c[4];
                for (int j = 0; j < 4; ++j) c[j] = ((x * M.m[0][j] + y * M.m[1][j]) + z * M.m[2][j]) + 1.0f * M.m[3][j];
                ok = ok && finite_(c[0]) && finite_(c[1]) && finite_(c[2]) && finite_(c[3]);
                poly[k] = CVert{ c[0], c[1], c[2], c[3] };
                if (masked) { mc[3 * k] = c[0]; mc[3 * k + 1] = c[1]; mc[3 * k + 2] = c[3]; muv[2 * k] = p[9]; muv[2 * k + 1] = p[10]; }    // uv at byte 36 (stride >= 44: the host checks)
            }
        }
        if (ok) {
            n = 3;
            for (int plane = 0; plane < 7; ++plane) {
                CVert out[kMaxPoly];
                int m = 0;
                for (int i = 0; i < kMaxPoly; ++i) {
                    if (i >= n) break;
                    const CVert& va = poly[i];
                    const CVert& vb = poly[i + 1 < n ? i + 1 : 0];
                    const float da = planeDist(va, plane), db = planeDist(vb, plane);
                    const bool ina = da >= 0.0f, inb = db >= 0.0f;
                    if (ina) {
                        if (m < kMaxPoly) out[m++] = va;
                        if (!inb && m < kMaxPoly) out[m++] = clipVertex(va, vb, da, db);
                    } else if (inb) {
                        if (m < kMaxPoly) out[m++] = clipVertex(vb, va, db, da);
                    }
                }
                n = m;
                for (int i = 0; i < kMaxPoly; ++i) if (i < n) poly[i] = out[i];
            }
            if (n < 3) n = 0;
            const float halfW = 0.5f * (float)a.width, halfH = 0.5f * (float)a.height;
            bool vok[kMaxPoly];
            for (int i = 0; i < kMaxPoly; ++i) {
                if (i >= n) break;
                const CVert& v = poly[i];
                const float nx = fdiv_(v.cx, v.cw), ny = fdiv_(v.cy, v.cw);
                const float fx = ((nx + 1.0f) * halfW) * 256.0f, fy = ((1.0f - ny) * halfH) * 256.0f;
                vok[i] = __builtin_fabsf(fx) <= kSnapLimit && __builtin_fabsf(fy) <= kSnapLimit;      // false for NaN
                sx[i] = vok[i] ? (int)__builtin_rintf(fx) : 0;
                sy[i] = vok[i] ? (int)__builtin_rintf(fy) : 0;
                dz[i] = fdiv_(v.cz, v.cw);
            }
            for (int k = 0; k + 2 < kMaxPoly; ++k) {
                if (k + 2 >= n) break;
                if (!(vok[0] && vok[k + 1] && vok[k + 2])) continue;
                const int64_t A = edgeFn(sx[k + 1], sy[k + 1], sx[k + 2], sy[k + 2], sx[0], sy[0]);
                if (A == 0) continue;
                if ((A > 0 && job.cullMode == VQHIP_CULL_FRONT) || (A < 0 && job.cullMode == VQHIP_CULL_BACK)) continue;
                const int xmin = min(sx[0], min(sx[k + 1], sx[k + 2])), xmax = max(sx[0], max(sx[k + 1], sx[k + 2]));
                const int ymin = min(sy[0], min(sy[k + 1], sy[k + 2])), ymax = max(sy[0], max(sy[k + 1], sy[k + 2]));
                const int i0 = max(pixelFirst(xmin, a.samples), 0), i1 = min(pixelLast(xmax, a.samples), a.width - 1);
                const int j0 = max(pixelFirst(ymin, a.samples), 0), j1 = min(pixelLast(ymax, a.samples), a.height - 1);
                if (i0 > i1 || j0 > j1) continue;                   // no sample inside the box: nothing to rasterise
                emitMask |= 1u << k;
            }
        }
    }
    const uint32_t mine = (uint32_t)__builtin_popcount(emitMask);
    uint32_t place = 0;
    if (mine) place = atomicAdd(&sCount, mine);                     // LDS
    __syncthreads();
    if (threadIdx.x == 0) sBase = sCount ? atomicAdd(counter, sCount) : 0u;
    __syncthreads();
    if (!mine) return;
    const uint32_t q = job.firstQ + (uint32_t)t;                    // first(draw) + instance * numTris + tri; below 2^32 - 1 (the host refuses more)
    uint32_t mk = 0u;
    if constexpr (MASKED) if (masked) {
        const MaskArgs& m = maskArgsOf(mask...);
        const uint64_t at = (uint64_t)job.firstMasked + t;          // below the call's masked instanced triangles = sideCap
        if (at < m.sideCap) {
            uint4* sr = (uint4*)(m.side + at);
            sr[0] = make_uint4(__float_as_uint(mc[0]), __float_as_uint(mc[1]), __float_as_uint(mc[2]), __float_as_uint(mc[3]));
            sr[1] = make_uint4(__float_as_uint(mc[4]), __float_as_uint(mc[5]), __float_as_uint(mc[6]), __float_as_uint(mc[7]));
            sr[2] = make_uint4(__float_as_uint(mc[8]), __float_as_uint(muv[0]), __float_as_uint(muv[1]), __float_as_uint(muv[2]));
            sr[3] = make_uint4(__float_as_uint(muv[3]), __float_as_uint(muv[4]), __float_as_uint(muv[5]), job.maskSlot - 1u);
            mk = (uint32_t)at + 1u;
        }
    }
    uint64_t slot = (uint64_t)sBase + place;
    for (int k = 0; k + 2 < kMaxPoly; ++k) {
        if (!(emitMask >> k & 1u)) continue;
        if (slot >= a.recCap) break;                                // cannot happen (the buffer holds eight records per instanced triangle); never write past it
        const int va = 0, vb = k + 1, vc = k + 2;
        const int xmin = min(sx[va], min(sx[vb], sx[vc])), xmax = max(sx[va], max(sx[vb], sx[vc]));
        const int ymin = min(sy[va], min(sy[vb], sy[vc])), ymax = max(sy[va], max(sy[vb], sy[vc]));
        const uint32_t i0 = (uint32_t)max(pixelFirst(xmin, a.samples), 0), i1 = (uint32_t)min(pixelLast(xmax, a.samples), a.width - 1);
        const uint32_t j0 = (uint32_t)max(pixelFirst(ymin, a.samples), 0), j1 = (uint32_t)min(pixelLast(ymax, a.samples), a.height - 1);
        boxes[slot] = make_uint2(i0 | i1 << 16, j0 | j1 << 16);
        uint4* r = records + slot * 3;
        r[0] = make_uint4((uint32_t)sx[va], (uint32_t)sy[va], (uint32_t)sx[vb], (uint32_t)sy[vb]);
        r[1] = make_uint4((uint32_t)sx[vc], (uint32_t)sy[vc], __float_as_uint(dz[va]), __float_as_uint(dz[vb]));
        r[2] = make_uint4(__float_as_uint(dz[vc]), q, mk, 0u);
        ++slot;
    }
}

// MASKED (§7.19): a sample of a stamped record that passes coverage and the < 1.0 test runs the alpha test of its pixel (M1: at the pixel centre, once per
// (primitive, pixel) — at 4x each covered sample of the pixel evaluates the same function of (side record, i, j), so the four agree) before the minimum.
template <int T, int S, class... MA>
__global__ void __launch_bounds__(kFillLanes) k_scene_fill(SceneDepthArgs a, const uint32_t* __restrict__ counter, const uint2* __restrict__ boxes,
                                                           const uint4* __restrict__ records, MA... mask) {
    constexpr bool MASKED = sizeof...(MA) != 0;
    __shared__ unsigned long long tile[T * T * S];                  // 32 KiB at (32, 4) and at (64, 1)
    __shared__ uint32_t queue[kFillLanes];
    __shared__ uint32_t qn;
    const int tilesX = (a.width + T - 1) / T;
    const int tx0 = (int)(blockIdx.x % tilesX) * T, ty0 = (int)(blockIdx.x / tilesX) * T;
    const int tx1 = min(tx0 + T, a.width) - 1, ty1 = min(ty0 + T, a.height) - 1;
    for (int i = threadIdx.x; i < T * T * S; i += kFillLanes) tile[i] = kClearKey;
    if (threadIdx.x == 0) qn = 0u;
    __syncthreads();

    const uint64_t cnt64 = *counter;
    const uint32_t count = (uint32_t)(cnt64 < a.recCap ? cnt64 : a.recCap);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (uint32_t base = 0; base < count; base += kFillLanes) {
        const uint32_t r = base + threadIdx.x;
        if (r < count) {
            const uint2 bb = boxes[r];
            const int i0 = (int)(bb.x & 0xffffu), i1 = (int)(bb.x >> 16), j0 = (int)(bb.y & 0xffffu), j1 = (int)(bb.y >> 16);
            if (i0 <= tx1 && i1 >= tx0 && j0 <= ty1 && j1 >= ty0) queue[atomicAdd(&qn, 1u)] = r;
        }
        __syncthreads();
        const uint32_t nq = qn;
        for (uint32_t qi = wave; qi < nq; qi += kFillLanes / 64) {
            const uint32_t rec = queue[qi];
            const uint2 bb = boxes[rec];
            const uint4 r0 = records[(size_t)rec * 3], r1 = records[(size_t)rec * 3 + 1], r2 = records[(size_t)rec * 3 + 2];
            const int x0 = (int)r0.x, y0 = (int)r0.y, x1 = (int)r0.z, y1 = (int)r0.w, x2 = (int)r1.x, y2 = (int)r1.y;
            const float d0 = __uint_as_float(r1.z), d1 = __uint_as_float(r1.w), d2 = __uint_as_float(r2.x);
            const uint32_t q = r2.y;
            MaskTri mt;
            bool alphaTest = false;
            if constexpr (MASKED) alphaTest = loadMaskTri(maskArgsOf(mask...), r2.z, mt);
            const int bx0 = max((int)(bb.x & 0xffffu), tx0), bx1 = min((int)(bb.x >> 16), tx1);
            const int by0 = max((int)(bb.y & 0xffffu), ty0), by1 = min((int)(bb.y >> 16), ty1);
            const int bw = bx1 - bx0 + 1, nsmp = bw * (by1 - by0 + 1) * S;                               // 1 .. T * T * S
            const int64_t A = edgeFn(x1, y1, x2, y2, x0, y0);
            const int64_t sgn = A > 0 ? 1 : -1;
            // top-left of the edge opposite each vertex, in the winding that makes the triangle clockwise on the y-down target
            auto topLeft = [&](int xa, int ya, int xb, int yb) { const int64_t dx = sgn * (xb - xa), dy = sgn * (yb - ya); return dy < 0 || (dy == 0 && dx > 0); };
            const bool tl0 = topLeft(x1, y1, x2, y2), tl1 = topLeft(x2, y2, x0, y0), tl2 = topLeft(x0, y0, x1, y1);
            const float fA = (float)A;
            for (int p = lane; p < nsmp; p += 64) {
                const int s = S == 1 ? 0 : (p & (S - 1)), pix = S == 1 ? p : p / S;
                const int i = bx0 + pix % bw, j = by0 + pix / bw;
                const int px = 256 * i + sampleX<S>(s), py = 256 * j + sampleY<S>(s);
                const int64_t E0 = edgeFn(x1, y1, x2, y2, px, py), E1 = edgeFn(x2, y2, x0, y0, px, py), E2 = edgeFn(x0, y0, x1, y1, px, py);
                const int64_t s0 = sgn * E0, s1 = sgn * E1, s2 = sgn * E2;
                if (!((s0 > 0 || (s0 == 0 && tl0)) && (s1 > 0 || (s1 == 0 && tl1)) && (s2 > 0 || (s2 == 0 && tl2)))) continue;
                const float b1 = fdiv_((float)E1, fA), b2 = fdiv_((float)E2, fA);
                const uint32_t bits = __float_as_uint(sat01((d0 + b1 * (d1 - d0)) + b2 * (d2 - d0)));
                if (bits >= 0x3f800000u) continue;                  // LESS against the clear value 1.0 fails: the sample and its id stay untouched
                if constexpr (MASKED) { if (alphaTest && maskDiscardScene(mt, i, j, a.width, a.height)) continue; }     // a discarded fragment never reaches the minimum
                atomicMin(&tile[((j - ty0) * T + (i - tx0)) * S + s], ((unsigned long long)bits << 32) | q);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) qn = 0u;
        __syncthreads();
    }
    const int w = tx1 - tx0 + 1, h = ty1 - ty0 + 1;
    for (int p = threadIdx.x; p < T * h; p += kFillLanes) {
        const int i = p % T, j = p / T;
        if (i >= w) continue;
        const size_t at = (size_t)(ty0 + j) * a.pitch + tx0 + i;
        if (S == 1) {
            const unsigned long long k = tile[j * T + i];
            a.depth[at] = __uint_as_float((uint32_t)(k >> 32));
            if (a.primitive) a.primitive[at] = (uint32_t)k;
        } else {
            uint32_t d[4], o[4];
            for (int s = 0; s < 4; ++s) { const unsigned long long k = tile[(j * T + i) * S + s]; d[s] = (uint32_t)(k >> 32); o[s] = (uint32_t)k; }
            ((uint4*)a.depth)[at] = make_uint4(d[0], d[1], d[2], d[3]);
            if (a.primitive) ((uint4*)a.primitive)[at] = make_uint4(o[0], o[1], o[2], o[3]);
            if (a.layers > 0) {
                // §7.17: walk samples 0 .. 3; a sample joins the open layer that its owner opened, or opens the next one. At most four owners, four layers.
                uint32_t lp[4] = { kNoPrimitive, kNoPrimitive, kNoPrimitive, kNoPrimitive }, mask[4] = { 0u, 0u, 0u, 0u };
                int open = 0;
                for (int s = 0; s < 4; ++s) {
                    if (o[s] == kNoPrimitive) continue;
                    int k = 0;
                    for (; k < 4; ++k) if (k >= open || lp[k] == o[s]) break;
                    if (k == open) { lp[k] = o[s]; ++open; }        // k <= s < 4
                    mask[k] |= 1u << s;
                }
                const size_t cat = (size_t)(ty0 + j) * a.coveragePitch + tx0 + i;
                for (int k = 0; k < 4; ++k) {
                    if (k >= a.layers) break;                       // owners beyond the layers asked for are dropped from the layer planes only
                    if (a.coverage[k]) a.coverage[k][cat] = (uint8_t)mask[k];
                    if (a.layerPrimitive[k]) a.layerPrimitive[k][at] = lp[k];
                }
            }
        }
    }
}

} // namespace

int scene_depth_tile(int rasterTile, int samples) { return rasterTile == 64 && samples == 1 ? 64 : 32; }   // 64 x 64 x 4 keys would be 128 KiB of LDS

hipError_t launch_scene_setup(hipStream_t s, const SceneDepthJob* jobs, int numJobs, uint32_t blocks, const SceneDepthArgs& a, uint32_t* counter, void* boxes, void* records) {
    hipLaunchKernelGGL(k_scene_setup<>, dim3(blocks), dim3(kSetupLanes), 0, s, jobs, numJobs, a, counter, (uint2*)boxes, (uint4*)records);
    return hipGetLastError();
}
hipError_t launch_scene_fill(hipStream_t s, const SceneDepthArgs& a, int tile, const uint32_t* counter, const void* boxes, const void* records) {
    const uint32_t blocks = (uint32_t)(((a.width + tile - 1) / tile) * ((a.height + tile - 1) / tile));
    if (a.samples == 4)  hipLaunchKernelGGL((k_scene_fill<32, 4>), dim3(blocks), dim3(kFillLanes), 0, s, a, counter, (const uint2*)boxes, (const uint4*)records);
    else if (tile == 64) hipLaunchKernelGGL((k_scene_fill<64, 1>), dim3(blocks), dim3(kFillLanes), 0, s, a, counter, (const uint2*)boxes, (const uint4*)records);
    else                 hipLaunchKernelGGL((k_scene_fill<32, 1>), dim3(blocks), dim3(kFillLanes), 0, s, a, counter, (const uint2*)boxes, (const uint4*)records);
    return hipGetLastError();
}

hipError_t launch_scene_setup_masked(hipStream_t s, const SceneDepthJob* jobs, int numJobs, uint32_t blocks, const SceneDepthArgs& a, uint32_t* counter, void* boxes, void* records,
                                     const MaskArgs& m) {
    hipLaunchKernelGGL(k_scene_setup<MaskArgs>, dim3(blocks), dim3(kSetupLanes), 0, s, jobs, numJobs, a, counter, (uint2*)boxes, (uint4*)records, m);
    return hipGetLastError();
}
hipError_t launch_scene_fill_masked(hipStream_t s, const SceneDepthArgs& a, int tile, const uint32_t* counter, const void* boxes, const void* records, const MaskArgs& m) {
    const uint32_t blocks = (uint32_t)(((a.width + tile - 1) / tile) * ((a.height + tile - 1) / tile));
    if (a.samples == 4)  hipLaunchKernelGGL((k_scene_fill<32, 4, MaskArgs>), dim3(blocks), dim3(kFillLanes), 0, s, a, counter, (const uint2*)boxes, (const uint4*)records, m);
    else if (tile == 64) hipLaunchKernelGGL((k_scene_fill<64, 1, MaskArgs>), dim3(blocks), dim3(kFillLanes), 0, s, a, counter, (const uint2*)boxes, (const uint4*)records, m);
    else                 hipLaunchKernelGGL((k_scene_fill<32, 1, MaskArgs>), dim3(blocks), dim3(kFillLanes), 0, s, a, counter, (const uint2*)boxes, (const uint4*)records, m);
    return hipGetLastError();
}

} // namespace vqk
