// displace.hip — vqhip_displace_meshes: the heightmap displacement of the reference's five vertex stages (CalcHeightOffset: ForwardLighting.hlsl:136-154,
// DepthPrePass.hlsl:96-100, ShadowDepthPass.hlsl:61-66, ObjectID.hlsl:70-74, Outline.hlsl:78-82), applied ONCE per (mesh, material) to a copy of the vertex stream that
// every rasteriser of this library then consumes unchanged. docs/DESIGN_DETAILS.md §7.22 H1 .. H4 is the contract; tests/displace_ref.py states it in numpy.
//   k_displace_vertices : a block = 256 consecutive vertices of one job. Phase 1, one lane per vertex: uv (dwords 9, 10) -> H1 -> H2 (four gathers of level 0) ->
//                         h = s * displacement -> y' = y + h. Phase 2 moves the block's bytes with consecutive lanes on consecutive dwords, whatever the stride:
//                         the full-stride form copies the block's 256 * stride input bytes and swaps in y' (from LDS) at dword 1 of every vertex; the 12-byte form
//                         writes the 768 position dwords that phase 1 parked in LDS.
//                         For the engine's 44-byte vertex the full-stride form's copy loads are issued before phase 1 and held in registers across the barrier.
// A 44-byte vertex is not 16-byte aligned, so every access is a dword; a block's span is contiguous, so each wave instruction of phase 2 covers 256 consecutive
// bytes. Every index is bounded by the job's numVertices; the texture taps are wrapped into level 0 for any uv (vq_tex8.h).
#include "vq_internal.h"
#include "vq_tex8.h"

namespace vqk {
namespace {

constexpr int kLanes = kDisplaceLanes;            // four waves; 3 KiB of LDS: occupancy is bounded by nothing but the wave slots

__global__ void __launch_bounds__(kLanes) k_displace_vertices(const DisplaceJob* __restrict__ jobs, int numJobs) {
    __shared__ float sPos[kLanes * 3];            // phase 1's (x, y', z) per vertex; the full-stride form reads y' alone
    // the block's job: the last one whose firstBlock is <= blockIdx.x (block-uniform binary search; numJobs bounds it)
    int lo = 0, hi = numJobs - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (jobs[mid].firstBlock <= blockIdx.x) lo = mid; else hi = mid - 1; }
    const DisplaceJob job = jobs[lo];
    const uint32_t v0 = (blockIdx.x - job.firstBlock) * (uint32_t)kLanes;         // < numVertices: the host gives a job ceil(numVertices / 256) blocks
    if (v0 >= job.numVertices) return;                                            // holds by construction; checked all the same (block-uniform)
    const uint32_t n = min(job.numVertices - v0, (uint32_t)kLanes);              // the block's vertices
    const uint32_t sw = job.strideBytes >> 2;                                     // dwords per vertex, >= 11
    const uint32_t* __restrict__ in = (const uint32_t*)job.vertices + (size_t)v0 * sw;
    const bool full = job.outStrideBytes != 12u;
    // The engine's own 44-byte vertex, full-stride form: the block's copy loads are issued BEFORE phase 1, so that they are in flight while the uv loads and the
    // gathers of H2 wait (profiles/r24a_heightmap_displacement.md). Other strides take the loop behind the barrier.
    constexpr uint32_t kEngineWords = 11;
    const bool early = full && sw == kEngineWords;                                // block-uniform
    uint32_t held[kEngineWords];
    if (early) {
#pragma unroll
        for (uint32_t k = 0; k < kEngineWords; ++k) { const uint32_t w = threadIdx.x + k * kLanes; held[k] = w < n * kEngineWords ? in[w] : 0u; }
    }

    if (threadIdx.x < n) {
        const uint32_t* __restrict__ p = in + (size_t)threadIdx.x * sw;
        const float y = __uint_as_float(p[1]);
        const float u = __uint_as_float(p[9]) * job.sx + job.ox;                  // H1: product and sum rounded separately (-ffp-contract=off)
        const float v = __uint_as_float(p[10]) * job.sy + job.oy;
        const float s = job.texels ? fetch_lane_red_level0(job.texels, job.width, job.height, u, v) : 0.0f;      // H2; the null SRV samples 0
        const float h = s * job.displacement;                                     // H3
        sPos[threadIdx.x * 3 + 1] = y + h;
        if (!full) { sPos[threadIdx.x * 3] = __uint_as_float(p[0]); sPos[threadIdx.x * 3 + 2] = __uint_as_float(p[2]); }
    }
    __syncthreads();

    if (early) {
        uint32_t* __restrict__ out = (uint32_t*)job.out + (size_t)v0 * kEngineWords;
#pragma unroll
        for (uint32_t k = 0; k < kEngineWords; ++k) {
            const uint32_t w = threadIdx.x + k * kLanes, vtx = w / kEngineWords;
            if (w < n * kEngineWords) out[w] = (w - vtx * kEngineWords == 1u) ? __float_as_uint(sPos[vtx * 3 + 1]) : held[k];
        }
    } else if (full) {
        uint32_t* __restrict__ out = (uint32_t*)job.out + (size_t)v0 * sw;
        const uint32_t words = n * sw;                                            // <= 256 * stride / 4 < 2^32: the host bounds stride * 256
        for (uint32_t w = threadIdx.x; w < words; w += kLanes) {
            const uint32_t vtx = w / sw;
            out[w] = (w - vtx * sw == 1u) ? __float_as_uint(sPos[vtx * 3 + 1]) : in[w];
        }
    } else {
        uint32_t* __restrict__ out = (uint32_t*)job.out + (size_t)v0 * 3;
        const uint32_t words = n * 3;
        for (uint32_t w = threadIdx.x; w < words; w += kLanes) out[w] = __float_as_uint(sPos[w]);
    }
}

} // namespace

hipError_t launch_displace(hipStream_t s, const DisplaceJob* jobs, int numJobs, uint32_t blocks) {
    hipLaunchKernelGGL(k_displace_vertices, dim3(blocks), dim3(kLanes), 0, s, jobs, numJobs);
    return hipGetLastError();
}

} // namespace vqk
