// raster_outline.hip — vqhip_outline: both passes of the Outline pass (Outline.hlsl through OutlinePass's two PSOs, OutlinePass.cpp:247-405; drawn last into scene
// colour by VQRenderer::RenderOutline, SceneRendering.cpp:514) at one sample per pixel. docs/DESIGN_DETAILS.md §7.21 is the contract (O1 .. O6); tests/outline_ref.py
// states it in numpy on top of tests/scene_depth_ref.py.
//   k_raster_begin (raster.hip) : zeroes the record counter
//   k_outline_setup : one lane per (draw, triangle): both vertex stages on the same three vertices — O1 (pass 0: position through the binary32 product
//                     matWorldView x matProj) and O2 (pass 1: the view-space position moved along normalize(n.xyx) by 0.5, through matProj) —, each polygon through
//                     Sutherland-Hodgman against seven planes, the W x H viewport, the snap; appends up to eight MARK records (three z/w, as §7.17's) and up to
//                     eight PAINT records (1 + the job's number) per triangle. The first lane of a job also writes the job's colour-table entry: the four
//                     pow_(Color.c, 2.2f) as halfs — once per draw, not per pixel — and the draw's index.
//   k_outline_fill  : one workgroup per tile of T x T pixels, one 32-bit LDS word per pixel, cleared to 0. A mark fragment (V5 depth below 1.0) does
//                     atomicOr(word, 0x80000000), a paint fragment atomicMax(word, 1 + job): the max leaves a marked word marked and the or keeps the low bits,
//                     so the two kinds need no barrier between them and the result does not depend on the order of the records. Then the tile is stored once:
//                     selection = word >> 31; a word that is neither 0 nor marked names the last-submitted draw that covers the pixel: its colour goes to
//                     sceneColor, its index to writer. sceneColor is touched at written pixels only.
// Every loop bound is a viewport size, a record count clamped to capacity, a draw count or a constant: nothing a vertex value can stretch. No inline assembly.
#include "vq_raster.h"

namespace vqk {
namespace {

constexpr int kSetupLanes = 256;
constexpr int kFillLanes = 256;
constexpr int kMaxPoly = 10;                      // a triangle against seven planes: at most 3 + 7 vertices
constexpr uint32_t kMarkBit = 0x80000000u;
constexpr uint32_t kNoWriter = 0xffffffffu;

struct CVert { float cx, cy, cz, cw; };

// O5: one channel of the colour as a half, round to nearest even; a NaN is 0x7E00 with its sign
VQD uint32_t colourHalf(float c) {
    const float p = pow_(c, 2.2f);
    if (p != p) return ((__float_as_uint(p) >> 16) & 0x8000u) | 0x7e00u;
    return (uint32_t)__builtin_bit_cast(uint16_t, to_f16(p));
}

__global__ void __launch_bounds__(kSetupLanes) k_outline_setup(const OutlineJob* __restrict__ jobs, int numJobs, uint32_t firstJob, OutlineArgs a,
                                                               uint32_t* __restrict__ counter, uint2* __restrict__ boxes, uint4* __restrict__ records) {
    __shared__ uint32_t sCount, sBase;
    // the block's job: the last one whose firstBlock is <= blockIdx.x (block-uniform binary search; numJobs bounds it)
    int lo = 0, hi = numJobs - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (jobs[mid].firstBlock <= blockIdx.x) lo = mid; else hi = mid - 1; }
    const OutlineJob job = jobs[lo];
    const uint32_t jobNo = firstJob + (uint32_t)lo;
    const VQ_OutlineData* __restrict__ cb = job.cb;
    if (blockIdx.x == job.firstBlock && threadIdx.x == 0 && jobNo < a.colorCap) {                    // jobNo < colorCap holds: a job has a triangle, the table an entry per triangle
        OutlineColor c;
        c.rg = colourHalf(cb->Color.x) | colourHalf(cb->Color.y) << 16;
        c.ba = colourHalf(cb->Color.z) | colourHalf(cb->Color.w) << 16;
        c.drawIndex = job.drawIndex; c.pad = 0u;
        a.colors[jobNo] = c;
    }

    const uint32_t t = (blockIdx.x - job.firstBlock) * kSetupLanes + threadIdx.x;
    const bool live = t < job.numTris;
    float clip[2][3][4];                          // [pass][vertex][xyzw]
    bool ok[2] = { false, false };
    if (live) {
        uint32_t idx[3];
        if (fetchTriangle(job.indices, job.indexBits, t, job.numVertices, idx)) {
            const VQ_matrix& WV = cb->matWorldView;
            const VQ_matrix& NV = cb->matNormalView;
            const VQ_matrix& Pr = cb->matProj;
            VQ_matrix WVP;                        // O1: the product of two matrices, every operation rounded
            for (int r = 0; r < 4; ++r)
                for (int c = 0; c < 4; ++c)
                    WVP.m[r][c] = ((WV.m[r][0] * Pr.m[0][c] + WV.m[r][1] * Pr.m[1][c]) + WV.m[r][2] * Pr.m[2][c]) + WV.m[r][3] * Pr.m[3][c];
            ok[0] = ok[1] = true;
            for (int k = 0; k < 3; ++k) {
                const float* p = (const float*)(job.positions + (size_t)idx[k] * job.strideBytes);   // normal at byte 12 (stride >= 24: the host checks)
                float P[3];
                ok[0] = clipPosition(p, WVP, P, clip[0][k]) && ok[0];                                // P = (x, y + 0.0f, z)
                // O2
                const float nx = p[3], ny = p[4], nz = p[5];
                float V[3], n[3];
                for (int j = 0; j < 3; ++j) {
                    V[j] = mulPoint(P, WV, j);
                    n[j] = ((nx * NV.m[0][j] + ny * NV.m[1][j]) + nz * NV.m[2][j]) + 0.0f * NV.m[3][j];
                }
                const f3 vn = normalize_lit(mk3(n[0], n[1], n[0]));                                  // the reference's .xyx
                const float E[3] = { V[0] + vn.x * 0.5f, V[1] + vn.y * 0.5f, V[2] + vn.z * 0.5f };
                bool fin = true;
                for (int j = 0; j < 4; ++j) { clip[1][k][j] = mulPoint(E, Pr, j); fin = fin && finite_(clip[1][k][j]); }
                ok[1] = ok[1] && fin;
            }
        }
    }
    const float halfW = 0.5f * (float)a.width, halfH = 0.5f * (float)a.height;
    for (int pass = 0; pass < 2; ++pass) {
        if (threadIdx.x == 0) sCount = 0u;
        __syncthreads();
        int sx[kMaxPoly], sy[kMaxPoly];
        float dz[kMaxPoly];                      // z / w
        uint32_t emitMask = 0;                   // bit k: fan triangle (0, k + 1, k + 2) is emitted
        if (ok[pass]) {
            CVert poly[kMaxPoly];
            for (int k = 0; k < 3; ++k) poly[k] = CVert{ clip[pass][k][0], clip[pass][k][1], clip[pass][k][2], clip[pass][k][3] };
            const int n = clipPolygon<7>(poly, 3, [](CVert&, const CVert&, const CVert&, float) {});
            bool vok[kMaxPoly];
            for (int i = 0; i < kMaxPoly; ++i) {
                if (i >= n) break;
                const CVert& v = poly[i];
                vok[i] = snapVertex(v.cx, v.cy, v.cw, halfW, halfH, sx[i], sy[i]);
                dz[i] = fdiv_(v.cz, v.cw);
            }
            emitMask = fanMask<kMaxPoly>(sx, sy, vok, n, VQHIP_CULL_NONE, a.width, a.height, 1);
        }
        const uint32_t mine = (uint32_t)__builtin_popcount(emitMask);
        const uint32_t place = reserveSlots(mine, counter, sCount, sBase);
        uint64_t slot = (uint64_t)sBase + place;
        const uint32_t kind = pass ? jobNo + 1u : 0u;
        for (int k = 0; k + 2 < kMaxPoly; ++k) {
            if (!(emitMask >> k & 1u)) continue;
            if (slot >= a.recCap) break;                            // cannot happen (the buffer holds sixteen records per triangle); never write past it
            const int va = 0, vb = k + 1, vc = k + 2;
            fanBox(sx, sy, k, a.width, a.height, 1, boxes[slot]);
            uint4* r = records + slot * 3;
            r[0] = make_uint4((uint32_t)sx[va], (uint32_t)sy[va], (uint32_t)sx[vb], (uint32_t)sy[vb]);
            r[1] = make_uint4((uint32_t)sx[vc], (uint32_t)sy[vc], __float_as_uint(dz[va]), __float_as_uint(dz[vb]));
            r[2] = make_uint4(__float_as_uint(dz[vc]), kind, 0u, 0u);
            ++slot;
        }
        __syncthreads();                                            // every lane has read sBase before the next pass reserves
    }
}

template <int T>
__global__ void __launch_bounds__(kFillLanes) k_outline_fill(OutlineArgs a, const uint32_t* __restrict__ counter, const uint2* __restrict__ boxes,
                                                             const uint4* __restrict__ records) {
    __shared__ uint32_t tile[T * T];                                // 4 KiB at 32, 16 KiB at 64
    __shared__ uint32_t queue[kFillLanes];
    __shared__ uint32_t qn;
    const int tilesX = (a.width + T - 1) / T;
    const int tx0 = (int)(blockIdx.x % tilesX) * T, ty0 = (int)(blockIdx.x / tilesX) * T;
    const int tx1 = min(tx0 + T, a.width) - 1, ty1 = min(ty0 + T, a.height) - 1;
    for (int i = threadIdx.x; i < T * T; i += kFillLanes) tile[i] = 0u;
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
            const uint32_t kind = r2.y;                             // 0: a mark record; else 1 + the job's number
            const TileBox tb(bb, tx0, ty0, tx1, ty1);
            const TriSetup ts((int)r0.x, (int)r0.y, (int)r0.z, (int)r0.w, (int)r1.x, (int)r1.y);
            for (int p = lane; p < tb.npix; p += 64) {                                                   // 1 .. T * T pixels
                const int i = tb.bx0 + p % tb.bw, j = tb.by0 + p / tb.bw;
                int64_t E0, E1, E2;
                if (!ts.covers(256 * i + 128, 256 * j + 128, E0, E1, E2)) continue;
                uint32_t* word = &tile[(j - ty0) * T + (i - tx0)];
                if (kind) { atomicMax(word, kind); continue; }      // O5: depth ALWAYS, the last-submitted draw wins
                const float b1 = fdiv_((float)E1, ts.fA), b2 = fdiv_((float)E2, ts.fA);
                const uint32_t bits = __float_as_uint(sat01((d0 + b1 * (d1 - d0)) + b2 * (d2 - d0)));
                if (bits < 0x3f800000u) atomicOr(word, kMarkBit);   // O4: LESS against the cleared depth
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
        const uint32_t word = tile[j * T + i];
        const bool marked = (word >> 31) != 0u;
        const bool written = word != 0u && !marked && word - 1u < a.colorCap;
        uint32_t who = kNoWriter;
        if (written) {
            const OutlineColor c = a.colors[word - 1u];
            ((uint2*)a.sceneColor)[(size_t)(ty0 + j) * a.pitch + tx0 + i] = make_uint2(c.rg, c.ba);
            who = c.drawIndex;
        }
        if (a.selection) a.selection[(size_t)(ty0 + j) * a.selectionPitch + tx0 + i] = marked ? (uint8_t)1 : (uint8_t)0;
        if (a.writer) a.writer[(size_t)(ty0 + j) * a.writerPitch + tx0 + i] = who;
    }
}

} // namespace

hipError_t launch_outline_setup(hipStream_t s, const OutlineJob* jobs, int numJobs, uint32_t firstJob, uint32_t blocks, const OutlineArgs& a, uint32_t* counter,
                                void* boxes, void* records) {
    hipLaunchKernelGGL(k_outline_setup, dim3(blocks), dim3(kSetupLanes), 0, s, jobs, numJobs, firstJob, a, counter, (uint2*)boxes, (uint4*)records);
    return hipGetLastError();
}

hipError_t launch_outline_fill(hipStream_t s, const OutlineArgs& a, int tile, const uint32_t* counter, const void* boxes, const void* records) {
    const uint32_t blocks = (uint32_t)(((a.width + tile - 1) / tile) * ((a.height + tile - 1) / tile));
    if (tile == 64) hipLaunchKernelGGL((k_outline_fill<64>), dim3(blocks), dim3(kFillLanes), 0, s, a, counter, (const uint2*)boxes, (const uint4*)records);
    else            hipLaunchKernelGGL((k_outline_fill<32>), dim3(blocks), dim3(kFillLanes), 0, s, a, counter, (const uint2*)boxes, (const uint4*)records);
    return hipGetLastError();
}

} // namespace vqk
