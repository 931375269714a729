// raster_lines.hip — vqhip_line_draws: the line draws of the bounding-volumes pass at one sample per pixel: the WIREFRAME PSOs of Unlit.hlsl (RenderBoundingBoxes,
// SceneRendering.cpp:1853-1922, through the instanced cbuffer; the second half of RenderLightBounds, :1991-2014) and RenderDebugVertexAxes (:2018-2058,
// VertexDebug.hlsl: a point list whose geometry shader emits three coloured lines per point). Depth LESS without writes against the scene's depth, no blending, into
// the RGBA16F scene colour. docs/DESIGN_DETAILS.md §7.24 is the contract (L1 .. L8); tests/line_ref.py states it in numpy on top of tests/scene_depth_ref.py.
//   k_lines_setup : one lane per line — (draw, instance, triangle, edge) of a wireframe draw, (draw, index, axis) of a vertex-axes draw: L1 or L3's vertex stage,
//                   the segment clipped against seven planes from the inside end towards the outside end, the W x H viewport, the snap. The line goes to the
//                   FIXED slot q (box + record: the snapped ends, the two z / w, the colour-table entry, the major axis); a dropped line receives the empty
//                   box. No append counter: a slot number is L7's q. The first lane of a job writes the job's four colour-table entries (halfs + the draw's index).
//   k_lines_fill  : one workgroup per tile of T x T pixels, one 32-bit LDS word per pixel, cleared to 0. The workgroup scans the boxes in order, 256 at a time;
//                   a lane whose line touches the tile walks the line's major-axis steps inside the tile (at most T): per step the one pixel whose diamond the
//                   extended line crosses (L5's consequence; kept from step to step with one compare each way), L5's end rules in integers, L6's depth and
//                   test, then atomicMax(word, q + 1). A maximum does not depend on the order of arrival: the bits do not depend on scheduling. The tile is
//                   stored once: a non-zero word names the passing line with the largest q; its colour goes to sceneColor, its draw to writer.
// Every loop bound is a record count, T or a constant: nothing a vertex value can stretch. No inline assembly.
#include "vq_raster.h"

namespace vqk {
namespace {

constexpr int kSetupLanes = 256;
constexpr int kFillLanes = 256;
constexpr uint32_t kNoWriter = 0xffffffffu;

struct CVert { float cx, cy, cz, cw; };

// L7 = O5's conversion: one channel as a half, round to nearest even; a NaN is 0x7E00 with its sign
VQD uint32_t lineHalf(float c) {
    if (c != c) return ((__float_as_uint(c) >> 16) & 0x8000u) | 0x7e00u;
    return (uint32_t)__builtin_bit_cast(uint16_t, to_f16(c));
}
VQD LineColor lineColor(float r, float g, float b, float a, uint32_t drawIndex) {
    LineColor c;
    c.rg = lineHalf(r) | lineHalf(g) << 16; c.ba = lineHalf(b) | lineHalf(a) << 16; c.drawIndex = drawIndex; c.pad = 0u;
    return c;
}
VQD uint32_t fetchIndex(const void* indices, int indexBits, uint64_t at) {
    return indexBits == 16 ? (uint32_t)((const uint16_t*)indices)[at] : ((const uint32_t*)indices)[at];
}
// mul(M, float4(v, 0)).xyz in mulPoint's association (O2 writes the same sum)
VQD f3 mulDirection(f3 v, const VQ_matrix& M) {
    float r[3];
    for (int j = 0; j < 3; ++j) r[j] = ((v.x * M.m[0][j] + v.y * M.m[1][j]) + v.z * M.m[2][j]) + 0.0f * M.m[3][j];
    return mk3(r[0], r[1], r[2]);
}
VQD bool finite4(const float c[4]) { return finite_(c[0]) && finite_(c[1]) && finite_(c[2]) && finite_(c[3]); }

// L5: is the point (px, py) in the diamond set of the pixel centred at (cx, cy)? The open diamond, its two lower edges and its bottom corner (y grows downwards);
// for a y-major line its right corner too.
VQD bool inDiamond(int px, int py, int cx, int cy, bool yMajor) {
    const int dx = px - cx, dy = py - cy;
    const int a = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
    return a < 128 || (a == 128 && (dy > 0 || (yMajor && dx == 128)));
}

__global__ void __launch_bounds__(kSetupLanes) k_lines_setup(const LineJob* __restrict__ jobs, int numJobs, uint32_t firstJob, LineArgs a,
                                                             uint2* __restrict__ boxes, uint4* __restrict__ records) {
    // the block's job: the last one whose firstBlock is <= blockIdx.x (block-uniform binary search; numJobs bounds it)
    int lo = 0, hi = numJobs - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (jobs[mid].firstBlock <= blockIdx.x) lo = mid; else hi = mid - 1; }
    const LineJob job = jobs[lo];
    const uint32_t jobNo = firstJob + (uint32_t)lo;
    const bool axes = job.kind == VQHIP_LINES_VERTEX_AXES;
    const uint32_t colour0 = jobNo * kLineColorsPerJob;
    if (blockIdx.x == job.firstBlock && threadIdx.x == 0 && colour0 + kLineColorsPerJob <= a.colorCap) {   // holds: a job has a line, the table four entries per line
        if (axes) {                                                 // L3: the shader's emission order — tangent red, cross(N, T) BLUE, normal green
            a.colors[colour0]     = lineColor(0.6f, 0.0f, 0.0f, 1.0f, job.drawIndex);
            a.colors[colour0 + 1] = lineColor(0.0f, 0.0f, 0.6f, 1.0f, job.drawIndex);
            a.colors[colour0 + 2] = lineColor(0.0f, 0.6f, 0.0f, 1.0f, job.drawIndex);
        } else {
            const VQ_float4 c = *job.color;
            a.colors[colour0] = lineColor(c.x, c.y, c.z, c.w, job.drawIndex);
            a.colors[colour0 + 1] = a.colors[colour0 + 2] = lineColor(0.0f, 0.0f, 0.0f, 0.0f, job.drawIndex);
        }
        a.colors[colour0 + 3] = lineColor(0.0f, 0.0f, 0.0f, 0.0f, job.drawIndex);
    }
    const uint64_t t = (uint64_t)(blockIdx.x - job.firstBlock) * kSetupLanes + threadIdx.x;
    if (t >= job.numLines) return;
    const uint64_t q = (uint64_t)job.firstQ + t;                    // L7: 3 (first + instance numTris + tri) + edge, or first + 3 point + axis
    if (q >= a.lines) return;                                       // cannot happen (the host sums the same lines); never write past it

    CVert e0 = { 0.0f, 0.0f, 0.0f, 1.0f }, e1 = e0;
    bool ok = false;
    uint32_t colour = colour0;
    if (axes) {                                                     // L3
        const uint32_t point = (uint32_t)(t / 3u), axis = (uint32_t)(t % 3u);
        const uint32_t vi = fetchIndex(job.indices, job.indexBits, point);
        colour += axis;
        if (vi < job.numVertices) {
            const float* v = (const float*)(job.vertices + (size_t)vi * job.strideBytes);          // position @0, normal @12, tangent @24 (stride >= 36: the host checks)
            const VQ_VertexAxesData* __restrict__ cb = (const VQ_VertexAxesData*)job.cb;
            const float p[3] = { v[0], v[1], v[2] };
            const f3 N = mk3(v[3], v[4], v[5]), T = mk3(v[6], v[7], v[8]);
            const f3 tbn = normalize_lit(axis == 0 ? T : axis == 1 ? cross(N, T) : N);
            float P[3], E[3], c0[4], c1[4];
            for (int j = 0; j < 3; ++j) P[j] = mulPoint(p, cb->matWorld, j);
            const f3 o = normalize_lit(mulDirection(tbn, cb->matNormal));
            const float size = cb->LocalAxisSize;
            E[0] = P[0] + o.x * size; E[1] = P[1] + o.y * size; E[2] = P[2] + o.z * size;
            for (int j = 0; j < 4; ++j) { c0[j] = mulPoint(P, cb->matViewProj, j); c1[j] = mulPoint(E, cb->matViewProj, j); }
            ok = finite4(c0) && finite4(c1);
            e0 = CVert{ c0[0], c0[1], c0[2], c0[3] }; e1 = CVert{ c1[0], c1[1], c1[2], c1[3] };
        }
    } else {                                                        // L1, L2
        const uint32_t numTris = job.numPrims;
        const uint32_t it = (uint32_t)(t / 3u), edge = (uint32_t)(t % 3u);
        const uint32_t inst = it / numTris, tri = it % numTris;
        uint32_t idx[3];
        if (fetchTriangle(job.indices, job.indexBits, tri, job.numVertices, idx)) {
            const VQ_matrix& M = ((const VQ_matrix*)job.cb)[inst];
            float P[3], c0[4], c1[4];
            const bool f0 = clipPosition((const float*)(job.vertices + (size_t)idx[edge] * job.strideBytes), M, P, c0);
            const bool f1 = clipPosition((const float*)(job.vertices + (size_t)idx[edge == 2u ? 0u : edge + 1u] * job.strideBytes), M, P, c1);
            ok = f0 && f1;
            e0 = CVert{ c0[0], c0[1], c0[2], c0[3] }; e1 = CVert{ c1[0], c1[1], c1[2], c1[3] };
        }
    }
    // L4: the segment against the seven planes, from the inside end towards the outside end; the direction is kept
    for (int plane = 0; plane < 7; ++plane) {
        if (!ok) break;
        const float d0 = planeDist(e0, plane), d1 = planeDist(e1, plane);
        const bool in0 = d0 >= 0.0f, in1 = d1 >= 0.0f;
        if (!in0 && !in1) ok = false;
        else if (in0 && !in1) e1 = clipVertex(e0, e1, d0, d1, [](CVert&, const CVert&, const CVert&, float) {});
        else if (!in0 && in1) e0 = clipVertex(e1, e0, d1, d0, [](CVert&, const CVert&, const CVert&, float) {});
    }
    int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    float z0 = 0.0f, z1 = 0.0f;
    if (ok) {
        const float halfW = 0.5f * (float)a.width, halfH = 0.5f * (float)a.height;
        const bool s0 = snapVertex(e0.cx, e0.cy, e0.cw, halfW, halfH, x0, y0);
        const bool s1 = snapVertex(e1.cx, e1.cy, e1.cw, halfW, halfH, x1, y1);
        z0 = fdiv_(e0.cz, e0.cw); z1 = fdiv_(e1.cz, e1.cw);
        ok = s0 && s1 && !(x0 == x1 && y0 == y1);                   // L5: a zero-length line covers nothing
    }
    uint2 box = make_uint2(kLineEmptyBox, kLineEmptyBox);
    uint32_t yMajor = 0u;
    if (ok) {
        const int dx = x1 - x0, dy = y1 - y0;
        yMajor = (dx < 0 ? -dx : dx) >= (dy < 0 ? -dy : dy) ? 0u : 1u;
        // the pixels whose closed diamond [256 i, 256 i + 256] can meet the line's extent on each axis
        const int i0 = max(((min(x0, x1) + 255) >> 8) - 1, 0), i1 = min(max(x0, x1) >> 8, a.width - 1);
        const int j0 = max(((min(y0, y1) + 255) >> 8) - 1, 0), j1 = min(max(y0, y1) >> 8, a.height - 1);
        if (i0 <= i1 && j0 <= j1) box = make_uint2((uint32_t)i0 | (uint32_t)i1 << 16, (uint32_t)j0 | (uint32_t)j1 << 16);
    }
    boxes[q] = box;
    records[q * 2] = make_uint4((uint32_t)x0, (uint32_t)y0, (uint32_t)x1, (uint32_t)y1);
    records[q * 2 + 1] = make_uint4(__float_as_uint(z0), __float_as_uint(z1), colour, yMajor);
}

template <int T>
__global__ void __launch_bounds__(kFillLanes) k_lines_fill(LineArgs a, const uint2* __restrict__ boxes, const uint4* __restrict__ records) {
    __shared__ uint32_t tile[T * T];                                // 4 KiB at 32, 16 KiB at 64
    const int tilesX = (a.width + T - 1) / T;
    const int tx0 = (int)(blockIdx.x % tilesX) * T, ty0 = (int)(blockIdx.x / tilesX) * T;
    const int tx1 = min(tx0 + T, a.width) - 1, ty1 = min(ty0 + T, a.height) - 1;
    for (int i = threadIdx.x; i < T * T; i += kFillLanes) tile[i] = 0u;
    __syncthreads();

    for (uint32_t base = 0; base < a.lines; base += kFillLanes) {
        const uint32_t q = base + threadIdx.x;
        if (q >= a.lines) continue;
        const uint2 bb = boxes[q];
        const int bi0 = (int)(bb.x & 0xffffu), bi1 = (int)(bb.x >> 16), bj0 = (int)(bb.y & 0xffffu), bj1 = (int)(bb.y >> 16);
        if (!(bi0 <= bi1 && bj0 <= bj1 && bi0 <= tx1 && bi1 >= tx0 && bj0 <= ty1 && bj1 >= ty0)) continue;
        const uint4 r0 = records[(size_t)q * 2], r1 = records[(size_t)q * 2 + 1];
        const bool yMajor = r1.w != 0u;
        const int x0 = (int)r0.x, y0 = (int)r0.y, x1 = (int)r0.z, y1 = (int)r0.w;
        const float z0 = __uint_as_float(r1.x), z1 = __uint_as_float(r1.y);
        // (m, n): the major and the minor coordinate of the two ends
        const int m0 = yMajor ? y0 : x0, n0 = yMajor ? x0 : y0, m1 = yMajor ? y1 : x1, n1 = yMajor ? x1 : y1;
        const int s0 = yMajor ? max(bj0, ty0) : max(bi0, tx0), s1 = yMajor ? min(bj1, ty1) : min(bi1, tx1);      // the steps inside the tile: at most T
        const int k0 = yMajor ? max(bi0, tx0) : max(bj0, ty0), k1 = yMajor ? min(bi1, tx1) : min(bj1, ty1);      // the minor pixels a fragment may lie in
        if (s0 > s1 || m0 == m1) continue;                          // m0 == m1: cannot happen (a major axis has an extent)
        // L5's consequence: at the centre cm of a step the extended line has the minor coordinate num / den; the step's pixel is k with 256 k < num / den <= 256 k + 256
        const int64_t sgn = m1 > m0 ? 1 : -1;
        const int64_t den = sgn * (int64_t)(m1 - m0) * 256;         // > 0; num, den in units of 1 / |dm|: below 2^52
        const int64_t stepNum = sgn * (int64_t)(n1 - n0) * 256;
        int64_t num = sgn * ((int64_t)n0 * (m1 - m0) + (int64_t)(256 * s0 + 128 - m0) * (n1 - n0));
        int64_t k = num / den;                                      // truncated: corrected to the ceiling - 1 below
        if (k * den >= num) --k;
        if ((k + 1) * den < num) ++k;
        const float fdm = (float)(m1 - m0), dz = z1 - z0;
        for (int s = s0; s <= s1; ++s) {                            // at most T steps
            if (s != s0) {
                num += stepNum;                                     // |stepNum| <= den: k moves by one at most
                if (num > (k + 1) * den) ++k; else if (num <= k * den) --k;
            }
            if (k < k0 || k > k1) continue;
            const int cm = 256 * s + 128, cn = 256 * (int)k + 128;
            const int cx = yMajor ? cn : cm, cy = yMajor ? cm : cn;
            const bool onSeg = sgn > 0 ? (cm >= m0 && cm <= m1) : (cm <= m0 && cm >= m1);
            const bool endIn = inDiamond(x1, y1, cx, cy, yMajor);
            if (endIn || !(onSeg || inDiamond(x0, y0, cx, cy, yMajor))) continue;                    // L5: the segment meets the diamond set and does not end in it
            const float tt = sat01(fdiv_((float)(cm - m0), fdm));                                    // L6
            const float d = sat01(z0 + tt * dz);
            const int i = cx >> 8, j = cy >> 8;                     // inside the tile and the target: s in [s0, s1], k in [k0, k1]
            if (d < a.sceneDepth[(size_t)j * a.depthPitch + i]) atomicMax(&tile[(j - ty0) * T + (i - tx0)], q + 1u);
        }
    }
    __syncthreads();
    const int w = tx1 - tx0 + 1, h = ty1 - ty0 + 1;
    for (int p = threadIdx.x; p < T * h; p += kFillLanes) {
        const int i = p % T, j = p / T;
        if (i >= w) continue;
        const uint32_t word = tile[j * T + i];
        uint32_t who = kNoWriter;
        if (word != 0u && word - 1u < a.lines) {
            const uint32_t ci = records[(size_t)(word - 1u) * 2 + 1].z;
            if (ci < a.colorCap) {
                const LineColor c = a.colors[ci];
                ((uint2*)a.sceneColor)[(size_t)(ty0 + j) * a.pitch + tx0 + i] = make_uint2(c.rg, c.ba);
                who = c.drawIndex;
            }
        }
        if (a.writer) a.writer[(size_t)(ty0 + j) * a.writerPitch + tx0 + i] = who;
    }
}

} // namespace

hipError_t launch_lines_setup(hipStream_t s, const LineJob* jobs, int numJobs, uint32_t firstJob, uint32_t blocks, const LineArgs& a, void* boxes, void* records) {
    hipLaunchKernelGGL(k_lines_setup, dim3(blocks), dim3(kSetupLanes), 0, s, jobs, numJobs, firstJob, a, (uint2*)boxes, (uint4*)records);
    return hipGetLastError();
}

hipError_t launch_lines_fill(hipStream_t s, const LineArgs& a, int tile, const void* boxes, const void* records) {
    const uint32_t blocks = (uint32_t)(((a.width + tile - 1) / tile) * ((a.height + tile - 1) / tile));
    if (tile == 64) hipLaunchKernelGGL((k_lines_fill<64>), dim3(blocks), dim3(kFillLanes), 0, s, a, (const uint2*)boxes, (const uint4*)records);
    else            hipLaunchKernelGGL((k_lines_fill<32>), dim3(blocks), dim3(kFillLanes), 0, s, a, (const uint2*)boxes, (const uint4*)records);
    return hipGetLastError();
}

} // namespace vqk
