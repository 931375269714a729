// raster_unlit.hip — vqhip_unlit_draws: the unlit draws of the lit pass (Unlit.hlsl through UNLIT_PSO / UNLIT_BLEND_PSO, PipelineStateObjects.cpp:1174-1232: the
// light gizmo meshes, SceneRendering.cpp:1787-1819, and the solid half of RenderLightBounds, :1940-1989) at one sample per pixel: depth LESS without writes against
// the scene's depth, into the RGBA16F scene colour, opaque or SRC_ALPHA / INV_SRC_ALPHA blended. docs/DESIGN_DETAILS.md §7.23 is the contract (U1 .. U7);
// tests/unlit_ref.py states it in numpy on top of tests/scene_depth_ref.py. Blending is a fold over the fragments of a pixel in submission order, so — unlike every
// other fill of this library — the result depends on the order in which a pixel meets its fragments: the fill keeps that order by construction.
//   k_unlit_setup : one lane per (draw, triangle): U1's vertex stage, Sutherland-Hodgman against seven planes, the W x H viewport, the snap, the draw's cull mode.
//                   Fan piece k of triangle q goes to the FIXED slot 8 q + k (box + record); every unused slot of the triangle receives the empty box, and the
//                   triangle's own box (the union of its slots' boxes, or the empty box) goes to entry q of the triangle boxes. No append counter: memory order
//                   is submission order whatever the schedule. The first lane of a job also writes the job's colour-table entry.
//   k_unlit_fill  : one workgroup of four waves per tile of T x T pixels. Every lane OWNS T * T / 256 pixels (wave w the rows [w T / 4, (w + 1) T / 4) of the tile,
//                   a lane one column of them) and holds their scene depth, their colour (blend mode: four binary32 that are halfs exactly) and their last
//                   writer in registers, loaded once. The workgroup scans the TRIANGLE boxes in order, 256 at a time (8 B per triangle: what bounds the fill on a
//                   scene of many triangles is this scan, once per tile), and lists the triangles that touch the tile IN ORDER (ballot + prefix popcount inside
//                   a wave, the four wave counts through LDS); the listed triangles' slots are then looked at 32 triangles = 256 slots at a time, lane 8 t + k
//                   slot k of the t-th, and the slots whose box touches the tile are compacted, again in order, into an LDS queue of
//                   VQHIP_UNLIT_QUEUE_CAPACITY records; before a chunk would overflow it, the queue is drained: every lane walks the queued records front to back over its own pixels (a wave whose
//                   rows the record's box misses skips it with a scalar branch) — int64 edge functions, stepped exactly from row to row, V5's depth, U3's test,
//                   then U5's overwrite or U6's fold. One store per touched pixel at the end; no atomics: no two lanes share a pixel.
// Every loop bound is a slot count, a queue length bounded by the capacity or a constant: nothing a vertex value can stretch. No inline assembly.
#include "vq_raster.h"

namespace vqk {
namespace {

constexpr int kSetupLanes = 256;
constexpr int kFillLanes = 256;
constexpr int kMaxPoly = 10;                      // a triangle against seven planes: at most 3 + 7 vertices
constexpr uint32_t kQueueCap = VQHIP_UNLIT_QUEUE_CAPACITY;
constexpr uint32_t kNoWriter = 0xffffffffu;
static_assert(kQueueCap >= (uint32_t)kFillLanes, "a chunk of one slot per lane fits an empty queue");
static_assert(kUnlitFanMax == kMaxPoly - 2, "a slot per fan piece");

struct CVert { float cx, cy, cz, cw; };

// U5: one channel as a half, round to nearest even; a NaN is 0x7E00 with its sign (O5's conversion)
VQD uint32_t opaqueHalf(float c) {
    if (c != c) return ((__float_as_uint(c) >> 16) & 0x8000u) | 0x7e00u;
    return (uint32_t)__builtin_bit_cast(uint16_t, to_f16(c));
}
// U6: the render target holds halfs between fragments: round, and keep the half as the binary32 it equals
VQD float roundHalf(float c) { return (float)to_f16(c); }
VQD uint32_t blendHalf(float c) { return c != c ? 0x7e00u : (uint32_t)__builtin_bit_cast(uint16_t, to_f16(c)); }      // exact: c is a half already
VQD float halfValue(uint32_t bits) { return (float)__builtin_bit_cast(_Float16, (uint16_t)bits); }

__global__ void __launch_bounds__(kSetupLanes) k_unlit_setup(const UnlitJob* __restrict__ jobs, int numJobs, uint32_t firstJob, UnlitArgs a,
                                                             uint2* __restrict__ triBoxes, uint2* __restrict__ boxes, uint4* __restrict__ records) {
    // the block's job: the last one whose firstBlock is <= blockIdx.x (block-uniform binary search; numJobs bounds it)
    int lo = 0, hi = numJobs - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (jobs[mid].firstBlock <= blockIdx.x) lo = mid; else hi = mid - 1; }
    const UnlitJob job = jobs[lo];
    const uint32_t jobNo = firstJob + (uint32_t)lo;
    const VQ_UnlitData* __restrict__ cb = job.cb;
    if (blockIdx.x == job.firstBlock && threadIdx.x == 0 && jobNo < a.colorCap) {                    // jobNo < colorCap holds: a job has a triangle, the table an entry per triangle
        UnlitColor c;
        c.c[0] = cb->color.x; c.c[1] = cb->color.y; c.c[2] = cb->color.z; c.c[3] = cb->color.w;
        c.drawIndex = job.drawIndex; c.pad[0] = c.pad[1] = c.pad[2] = 0u;
        a.colors[jobNo] = c;
    }
    const uint32_t t = (blockIdx.x - job.firstBlock) * kSetupLanes + threadIdx.x;
    if (t >= job.numTris) return;
    const uint64_t slot0 = ((uint64_t)job.firstQ + t) * kUnlitFanMax;                                // U4: q = first(draw) + tri
    if (slot0 + kUnlitFanMax > a.slots) return;                                                      // cannot happen (the host sums the same triangles); never write past it

    int sx[kMaxPoly], sy[kMaxPoly];
    float dz[kMaxPoly];                          // z / w
    uint32_t emitMask = 0;                       // bit k: fan triangle (0, k + 1, k + 2) is emitted
    uint32_t idx[3];
    if (fetchTriangle(job.indices, job.indexBits, t, job.numVertices, idx)) {
        CVert poly[kMaxPoly];
        bool ok = true;
        for (int k = 0; k < 3; ++k) {
            float P[3], c[4];
            ok = clipPosition((const float*)(job.positions + (size_t)idx[k] * job.strideBytes), cb->matModelViewProj, P, c) && ok;    // U1
            poly[k] = CVert{ c[0], c[1], c[2], c[3] };
        }
        if (ok) {
            const float halfW = 0.5f * (float)a.width, halfH = 0.5f * (float)a.height;
            const int n = clipPolygon<7>(poly, 3, [](CVert&, const CVert&, const CVert&, float) {});
            bool vok[kMaxPoly];
            for (int i = 0; i < kMaxPoly; ++i) {
                if (i >= n) break;
                const CVert& v = poly[i];
                vok[i] = snapVertex(v.cx, v.cy, v.cw, halfW, halfH, sx[i], sy[i]);
                dz[i] = fdiv_(v.cz, v.cw);
            }
            emitMask = fanMask<kMaxPoly>(sx, sy, vok, n, job.cullMode, a.width, a.height, 1);
        }
    }
    int ui0 = 0xffff, ui1 = 0, uj0 = 0xffff, uj1 = 0;              // the union of the slots' boxes: the empty box when there is none
    for (int k = 0; k < (int)kUnlitFanMax; ++k) {
        const uint64_t slot = slot0 + k;
        if (!(emitMask >> k & 1u)) { boxes[slot] = make_uint2(kUnlitEmptyBox, kUnlitEmptyBox); continue; }
        const int va = 0, vb = k + 1, vc = k + 2;
        uint2 bb;
        fanBox(sx, sy, k, a.width, a.height, 1, bb);
        boxes[slot] = bb;
        ui0 = min(ui0, (int)(bb.x & 0xffffu)); ui1 = max(ui1, (int)(bb.x >> 16)); uj0 = min(uj0, (int)(bb.y & 0xffffu)); uj1 = max(uj1, (int)(bb.y >> 16));
        uint4* r = records + slot * 3;
        r[0] = make_uint4((uint32_t)sx[va], (uint32_t)sy[va], (uint32_t)sx[vb], (uint32_t)sy[vb]);
        r[1] = make_uint4((uint32_t)sx[vc], (uint32_t)sy[vc], __float_as_uint(dz[va]), __float_as_uint(dz[vb]));
        r[2] = make_uint4(__float_as_uint(dz[vc]), jobNo, 0u, 0u);
    }
    triBoxes[slot0 / kUnlitFanMax] = make_uint2((uint32_t)ui0 | (uint32_t)ui1 << 16, (uint32_t)uj0 | (uint32_t)uj1 << 16);
}

template <int T, bool BLEND>
__global__ void __launch_bounds__(kFillLanes) k_unlit_fill(UnlitArgs a, const uint2* __restrict__ triBoxes, const uint2* __restrict__ boxes,
                                                           const uint4* __restrict__ records) {
    constexpr int PPL = T * T / kFillLanes;       // pixels a lane owns: 4 at 32, 16 at 64
    constexpr int RS = 64 / T;                    // rows between two pixels of a lane: a wave's 64 lanes cover 64 / T rows at once
    constexpr int WH = T / 4;                     // rows of the tile a wave owns
    __shared__ uint4 queue[kQueueCap * 4];        // 16 KiB: per record the three record words with the box in the spare two, and the colour
    __shared__ uint32_t triList[kFillLanes];      // the triangles of the current chunk that touch the tile, in order
    __shared__ uint32_t sWave[2][kFillLanes / 64], sWave2[2][kFillLanes / 64];    // the waves' counts of the two compactions, each double-buffered by parity
    const int tilesX = (a.width + T - 1) / T;
    const int tx0 = (int)(blockIdx.x % tilesX) * T, ty0 = (int)(blockIdx.x / tilesX) * T;
    const int tx1 = min(tx0 + T, a.width) - 1, ty1 = min(ty0 + T, a.height) - 1;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int wy0 = ty0 + wave * WH, wy1 = wy0 + WH - 1;
    const int x = tx0 + lane % T, yFirst = wy0 + lane / T;
    const bool xLive = x <= tx1;

    float zd[PPL];                                // the owned pixels' scene depth; 0 outside the target: no V5 depth is below it
    float col[BLEND ? PPL : 1][4];
    uint32_t who[PPL];                            // the job of the last passing fragment
    #pragma unroll
    for (int p = 0; p < PPL; ++p) {
        const int y = yFirst + p * RS;
        const bool live = xLive && y <= ty1;
        zd[p] = live ? a.sceneDepth[(size_t)y * a.depthPitch + x] : 0.0f;
        who[p] = kNoWriter;
        if (BLEND) {
            const uint2 c = live ? ((const uint2*)a.sceneColor)[(size_t)y * a.pitch + x] : make_uint2(0u, 0u);
            col[p][0] = halfValue(c.x & 0xffffu); col[p][1] = halfValue(c.x >> 16); col[p][2] = halfValue(c.y & 0xffffu); col[p][3] = halfValue(c.y >> 16);
        }
    }

    // every lane walks the first n queued records, front to back, over its own pixels
    auto drain = [&](uint32_t n) {
        for (uint32_t qi = 0; qi < n; ++qi) {
            const uint4 r2 = queue[qi * 4 + 2];
            const uint32_t bx = __builtin_amdgcn_readfirstlane(r2.z), by = __builtin_amdgcn_readfirstlane(r2.w);
            const int j0 = (int)(by & 0xffffu), j1 = (int)(by >> 16);
            if (j1 < wy0 || j0 > wy1) continue;                     // wave-uniform: the record misses this wave's rows
            if (x < (int)(bx & 0xffffu) || x > (int)(bx >> 16)) continue;
            const uint4 r0 = queue[qi * 4], r1 = queue[qi * 4 + 1];
            const float d0 = __uint_as_float(r1.z), d1 = __uint_as_float(r1.w), d2 = __uint_as_float(r2.x);
            const uint32_t jobNo = r2.y;
            const TriSetup ts((int)r0.x, (int)r0.y, (int)r0.z, (int)r0.w, (int)r1.x, (int)r1.y);
            const int px = 256 * x + 128, py = 256 * yFirst + 128;
            int64_t E0 = edgeFn(ts.x1, ts.y1, ts.x2, ts.y2, px, py), E1 = edgeFn(ts.x2, ts.y2, ts.x0, ts.y0, px, py), E2 = edgeFn(ts.x0, ts.y0, ts.x1, ts.y1, px, py);
            // an edge function is affine in the sample: one row step of 256 RS adds (xk - xj) * 256 RS, exactly (int64)
            const int64_t s0 = (int64_t)(ts.x2 - ts.x1) * (256 * RS), s1 = (int64_t)(ts.x0 - ts.x2) * (256 * RS), s2 = (int64_t)(ts.x1 - ts.x0) * (256 * RS);
            float src[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
            if (BLEND) { const uint4 c = queue[qi * 4 + 3]; src[0] = __uint_as_float(c.x); src[1] = __uint_as_float(c.y); src[2] = __uint_as_float(c.z); src[3] = __uint_as_float(c.w); }
            const float ia = 1.0f - src[3];                         // U6
            #pragma unroll
            for (int p = 0; p < PPL; ++p) {
                const int y = yFirst + p * RS;
                const bool cover = y >= j0 && y <= j1 && TriSetup::inside(ts.sgn * E0, ts.tl0) && TriSetup::inside(ts.sgn * E1, ts.tl1) && TriSetup::inside(ts.sgn * E2, ts.tl2);
                if (cover) {
                    const float b1 = fdiv_((float)E1, ts.fA), b2 = fdiv_((float)E2, ts.fA);
                    const float d = sat01((d0 + b1 * (d1 - d0)) + b2 * (d2 - d0));                  // V5
                    if (d < zd[p]) {                                                                 // U3: LESS, no write
                        who[p] = jobNo;
                        if (BLEND) {
                            for (int c = 0; c < 3; ++c) col[p][c] = roundHalf(src[c] * src[3] + col[p][c] * ia);
                            col[p][3] = roundHalf(src[3]);
                        }
                    }
                }
                E0 += s0; E1 += s1; E2 += s2;
            }
        }
    };

    uint32_t qn = 0;                                                // the queue's length: the same number in every lane
    const uint64_t below = ((uint64_t)1 << lane) - 1u;
    const uint32_t tris = a.slots / (uint32_t)kUnlitFanMax;
    auto touches = [&](uint2 bb) {
        const int i0 = (int)(bb.x & 0xffffu), i1 = (int)(bb.x >> 16), j0 = (int)(bb.y & 0xffffu), j1 = (int)(bb.y >> 16);
        return i0 <= i1 && j0 <= j1 && i0 <= tx1 && i1 >= tx0 && j0 <= ty1 && j1 >= ty0;
    };
    auto countWaves = [&](const uint32_t* counts, uint32_t& before, uint32_t& total) {
        before = 0u; total = 0u;
        for (int w = 0; w < kFillLanes / 64; ++w) { const uint32_t c = counts[w]; if (w < wave) before += c; total += c; }
    };
    uint32_t sub = 0;                                               // sub-chunks so far: the parity of sWave2
    for (uint32_t base = 0, it = 0; base < tris; base += kFillLanes, ++it) {
        const uint32_t t = base + threadIdx.x;
        const bool hit = t < tris && touches(triBoxes[t]);
        const uint64_t hits = __ballot(hit);
        if (lane == 0) sWave[it & 1u][wave] = (uint32_t)__builtin_popcountll(hits);
        __syncthreads();
        uint32_t listBefore, listed;
        countWaves(sWave[it & 1u], listBefore, listed);
        if (listed == 0u) continue;                                 // block-uniform
        if (hit) triList[listBefore + (uint32_t)__builtin_popcountll(hits & below)] = t;             // < kFillLanes
        __syncthreads();
        for (uint32_t g = 0; g < listed; g += kFillLanes / (uint32_t)kUnlitFanMax, ++sub) {          // 32 listed triangles = 256 slots, in slot order
            const uint32_t li = g + threadIdx.x / (uint32_t)kUnlitFanMax;
            bool take = false;
            uint32_t r = 0u;
            uint2 bb = make_uint2(kUnlitEmptyBox, kUnlitEmptyBox);
            if (li < listed) {
                r = triList[li] * (uint32_t)kUnlitFanMax + threadIdx.x % (uint32_t)kUnlitFanMax;     // < a.slots: triList holds triangles below tris
                bb = boxes[r];
                take = touches(bb);
            }
            const uint64_t votes = __ballot(take);
            if (lane == 0) sWave2[sub & 1u][wave] = (uint32_t)__builtin_popcountll(votes);
            __syncthreads();                                        // also: every queue entry written so far is visible
            uint32_t before, total;
            countWaves(sWave2[sub & 1u], before, total);
            if (total == 0u) continue;                              // block-uniform
            if (qn + total > kQueueCap) {                           // block-uniform: drain before the chunk would overflow the queue
                drain(qn);
                qn = 0u;
                __syncthreads();                                    // every lane has left the queue before it is refilled
            }
            if (take) {
                const uint32_t at = qn + before + (uint32_t)__builtin_popcountll(votes & below);    // < kQueueCap: qn + total <= kQueueCap
                const uint4 r0 = records[(size_t)r * 3], r1 = records[(size_t)r * 3 + 1], r2 = records[(size_t)r * 3 + 2];
                uint4 c = make_uint4(0u, 0u, 0u, 0u);
                if (BLEND && r2.y < a.colorCap) c = *(const uint4*)a.colors[r2.y].c;
                queue[at * 4] = r0; queue[at * 4 + 1] = r1; queue[at * 4 + 2] = make_uint4(r2.x, r2.y, bb.x, bb.y); queue[at * 4 + 3] = c;
            }
            qn += total;
        }
    }
    __syncthreads();
    drain(qn);

    #pragma unroll
    for (int p = 0; p < PPL; ++p) {
        const int y = yFirst + p * RS;
        if (!(xLive && y <= ty1)) continue;
        uint32_t index = kNoWriter;
        if (who[p] < a.colorCap) {
            const UnlitColor c = a.colors[who[p]];
            index = c.drawIndex;
            uint2 h;
            if (BLEND) h = make_uint2(blendHalf(col[p][0]) | blendHalf(col[p][1]) << 16, blendHalf(col[p][2]) | blendHalf(col[p][3]) << 16);
            else       h = make_uint2(opaqueHalf(c.c[0]) | opaqueHalf(c.c[1]) << 16, opaqueHalf(c.c[2]) | opaqueHalf(c.c[3]) << 16);
            ((uint2*)a.sceneColor)[(size_t)y * a.pitch + x] = h;
        }
        if (a.writer) a.writer[(size_t)y * a.writerPitch + x] = index;
    }
}

} // namespace

hipError_t launch_unlit_setup(hipStream_t s, const UnlitJob* jobs, int numJobs, uint32_t firstJob, uint32_t blocks, const UnlitArgs& a, void* triBoxes, void* boxes,
                              void* records) {
    hipLaunchKernelGGL(k_unlit_setup, dim3(blocks), dim3(kSetupLanes), 0, s, jobs, numJobs, firstJob, a, (uint2*)triBoxes, (uint2*)boxes, (uint4*)records);
    return hipGetLastError();
}

hipError_t launch_unlit_fill(hipStream_t s, const UnlitArgs& a, int tile, const void* triBoxes, const void* boxes, const void* records) {
    const uint32_t blocks = (uint32_t)(((a.width + tile - 1) / tile) * ((a.height + tile - 1) / tile));
    const uint2* tb = (const uint2*)triBoxes;
    const uint2* b = (const uint2*)boxes;
    const uint4* r = (const uint4*)records;
    if (tile == 64) {
        if (a.blend) hipLaunchKernelGGL((k_unlit_fill<64, true>), dim3(blocks), dim3(kFillLanes), 0, s, a, tb, b, r);
        else         hipLaunchKernelGGL((k_unlit_fill<64, false>), dim3(blocks), dim3(kFillLanes), 0, s, a, tb, b, r);
    } else {
        if (a.blend) hipLaunchKernelGGL((k_unlit_fill<32, true>), dim3(blocks), dim3(kFillLanes), 0, s, a, tb, b, r);
        else         hipLaunchKernelGGL((k_unlit_fill<32, false>), dim3(blocks), dim3(kFillLanes), 0, s, a, tb, b, r);
    }
    return hipGetLastError();
}

} // namespace vqk
