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
// vq_raster.h holds what this file shares with raster.hip: vertex stage, clipper, snap, fan walk and boxes, slot reservation, side record, binning, triangle
// setup and the coverage test. Here: the z planes' vertex, the sample pattern and q, the < 1.0 early-out before the alpha test, the 64-bit key tile, the layer walk.
#include "vq_raster.h"
#include "vq_raster_mask.h"

namespace vqk {
namespace {

constexpr int kSetupLanes = 256;
constexpr int kFillLanes = 256;
constexpr int kMaxPoly = 10;                      // a triangle against seven planes: at most 3 + 7 vertices
constexpr uint32_t kNoPrimitive = 0xffffffffu;
constexpr uint64_t kClearKey = ((uint64_t)0x3f800000u << 32) | kNoPrimitive;

struct CVert { float cx, cy, cz, cw; };

// sample s of a pixel, in 1/256 of a pixel from the pixel's corner: the centre at 1x, D3D's standard pattern at 4x
template <int S> VQD int sampleX(int s) { return S == 1 ? 128 : (s == 0 ? 96 : s == 1 ? 224 : s == 2 ? 32 : 160); }
template <int S> VQD int sampleY(int s) { return S == 1 ? 128 : 32 + 64 * s; }

// MASKED (§7.19): a draw with a maskSlot also writes its triangle's side record and stamps its records with 1 + the side record's index; the opaque
// instantiation is the code it was.
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
    uint32_t emitMask = 0;                       // bit k: fan triangle (0, k + 1, k + 2) is emitted
    const bool masked = MASKED && job.maskSlot != 0u;
    float mc[9], muv[6];                         // MASKED: the side record's fifteen floats
    if (live) {
        const uint32_t inst = (uint32_t)(t / job.numTris), tri = (uint32_t)(t % job.numTris);
        uint32_t idx[3];
        bool ok = fetchTriangle(job.indices, job.indexBits, tri, job.numVertices, idx);
        CVert poly[kMaxPoly];
        if (ok) {
            const VQ_matrix& M = job.wvp[inst];
            for (int k = 0; k < 3; ++k) {
                const float* p = (const float*)(job.positions + (size_t)idx[k] * job.strideBytes);
                float xyz[3], c[4];
                ok = clipPosition(p, M, xyz, c) && ok;
                poly[k] = CVert{ c[0], c[1], c[2], c[3] };
                if (masked) { mc[3 * k] = c[0]; mc[3 * k + 1] = c[1]; mc[3 * k + 2] = c[3]; muv[2 * k] = p[9]; muv[2 * k + 1] = p[10]; }    // uv at byte 36 (stride >= 44: the host checks)
            }
        }
        if (ok) {
            const int n = clipPolygon<7>(poly, 3, [](CVert&, const CVert&, const CVert&, float) {});
            const float halfW = 0.5f * (float)a.width, halfH = 0.5f * (float)a.height;
            bool vok[kMaxPoly];
            for (int i = 0; i < kMaxPoly; ++i) {
                if (i >= n) break;
                const CVert& v = poly[i];
                vok[i] = snapVertex(v.cx, v.cy, v.cw, halfW, halfH, sx[i], sy[i]);
                dz[i] = fdiv_(v.cz, v.cw);
            }
            emitMask = fanMask<kMaxPoly>(sx, sy, vok, n, job.cullMode, a.width, a.height, a.samples);
        }
    }
    const uint32_t mine = (uint32_t)__builtin_popcount(emitMask);
    const uint32_t place = reserveSlots(mine, counter, sCount, sBase);
    if (!mine) return;
    const uint32_t q = job.firstQ + (uint32_t)t;                    // first(draw) + instance * numTris + tri; below 2^32 - 1 (the host refuses more)
    uint32_t mk = 0u;
    if constexpr (MASKED) if (masked) mk = writeMaskSide(maskArgsOf(mask...), (uint64_t)job.firstMasked + t, mc, muv, job.maskSlot - 1u);
    uint64_t slot = (uint64_t)sBase + place;
    for (int k = 0; k + 2 < kMaxPoly; ++k) {
        if (!(emitMask >> k & 1u)) continue;
        if (slot >= a.recCap) break;                                // cannot happen (the buffer holds eight records per instanced triangle); never write past it
        const int va = 0, vb = k + 1, vc = k + 2;
        fanBox(sx, sy, k, a.width, a.height, a.samples, boxes[slot]);
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
        binRecords(boxes, count, base, tx0, ty0, tx1, ty1, queue, qn);
        __syncthreads();
        const uint32_t nq = qn;
        for (uint32_t qi = wave; qi < nq; qi += kFillLanes / 64) {
            const uint32_t rec = queue[qi];
            const uint2 bb = boxes[rec];
            const uint4 r0 = records[(size_t)rec * 3], r1 = records[(size_t)rec * 3 + 1], r2 = records[(size_t)rec * 3 + 2];
            const float d0 = __uint_as_float(r1.z), d1 = __uint_as_float(r1.w), d2 = __uint_as_float(r2.x);
            const uint32_t q = r2.y;
            MaskTri mt;
            bool alphaTest = false;
            if constexpr (MASKED) alphaTest = loadMaskTri(maskArgsOf(mask...), r2.z, mt);
            const TileBox tb(bb, tx0, ty0, tx1, ty1);
            const TriSetup ts((int)r0.x, (int)r0.y, (int)r0.z, (int)r0.w, (int)r1.x, (int)r1.y);
            for (int p = lane; p < tb.npix * S; p += 64) {                                               // 1 .. T * T * S samples
                const int s = S == 1 ? 0 : (p & (S - 1)), pix = S == 1 ? p : p / S;
                const int i = tb.bx0 + pix % tb.bw, j = tb.by0 + pix / tb.bw;
                int64_t E0, E1, E2;
                if (!ts.covers(256 * i + sampleX<S>(s), 256 * j + sampleY<S>(s), E0, E1, E2)) continue;
                const float b1 = fdiv_((float)E1, ts.fA), b2 = fdiv_((float)E2, ts.fA);
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

template <class... MA>
hipError_t launch_scene_setup(hipStream_t s, const SceneDepthJob* jobs, int numJobs, uint32_t blocks, const SceneDepthArgs& a, uint32_t* counter, void* boxes, void* records, const MA&... mask) {
    hipLaunchKernelGGL(k_scene_setup<MA...>, dim3(blocks), dim3(kSetupLanes), 0, s, jobs, numJobs, a, counter, (uint2*)boxes, (uint4*)records, mask...);
    return hipGetLastError();
}
template <class... MA>
hipError_t launch_scene_fill(hipStream_t s, const SceneDepthArgs& a, int tile, const uint32_t* counter, const void* boxes, const void* records, const MA&... mask) {
    const uint32_t blocks = (uint32_t)(((a.width + tile - 1) / tile) * ((a.height + tile - 1) / tile));
    if (a.samples == 4)  hipLaunchKernelGGL((k_scene_fill<32, 4, MA...>), dim3(blocks), dim3(kFillLanes), 0, s, a, counter, (const uint2*)boxes, (const uint4*)records, mask...);
    else if (tile == 64) hipLaunchKernelGGL((k_scene_fill<64, 1, MA...>), dim3(blocks), dim3(kFillLanes), 0, s, a, counter, (const uint2*)boxes, (const uint4*)records, mask...);
    else                 hipLaunchKernelGGL((k_scene_fill<32, 1, MA...>), dim3(blocks), dim3(kFillLanes), 0, s, a, counter, (const uint2*)boxes, (const uint4*)records, mask...);
    return hipGetLastError();
}
// the opaque and the masked form of each (capi.hip calls them with or without the trailing MaskArgs)
template hipError_t launch_scene_setup(hipStream_t, const SceneDepthJob*, int, uint32_t, const SceneDepthArgs&, uint32_t*, void*, void*);
template hipError_t launch_scene_setup(hipStream_t, const SceneDepthJob*, int, uint32_t, const SceneDepthArgs&, uint32_t*, void*, void*, const MaskArgs&);
template hipError_t launch_scene_fill(hipStream_t, const SceneDepthArgs&, int, const uint32_t*, const void*, const void*);
template hipError_t launch_scene_fill(hipStream_t, const SceneDepthArgs&, int, const uint32_t*, const void*, const void*, const MaskArgs&);

} // namespace vqk
