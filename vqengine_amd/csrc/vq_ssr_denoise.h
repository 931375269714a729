// vq_ssr_denoise.h — what the three passes of SSR's reflection denoiser share (ssr_reproject.hip, ssr_denoise.hip; docs/DESIGN_DETAILS.md §7.12, §7.13): the
// intrinsics as the contract pins them, the wave-local LDS synchronisation, the plane loads, the 9-tap kernel weights, the temporal variance, the tile-list walk and the
// persistent-grid launch.
#pragma once
#include "vq_internal.h"
#include "vq_devmath.h"

namespace vqk {
namespace dnsr {

using namespace vqd;

// min / max as §7.11 pins them: the second operand unless the first one wins
VQD float max2(float a, float b) { return (b > a || a != a) ? b : a; }
VQD float exp_(float x) { return exp2_(x * __uint_as_float(0x3FB8AA3Bu)); }                                       // the binary32 nearest log2(e): DXC's lowering
VQD float lerp_w(float a, float b, float t) { return a + t * (b - a); }
// the wave's own LDS traffic: make its stores visible to its loads (and its loads complete before the next tile's stores) without a workgroup barrier
VQD void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
VQD float rh(float x) { return (float)to_f16(x); }                                                                // through binary16 and back: what f32tof16 / f16tof32 leave
VQD f3 load_rgb(const void* img, int f32, size_t i) {
    const float4 c = f32 ? load_px<0>(img, i) : load_px<1>(img, i);
    return mk3(c.x, c.y, c.z);
}
VQD float load_r16f(const void* plane, size_t i) { return (float)((const _Float16*)plane)[i]; }
// FFX_DNSR_Reflections_LocalNeighborhoodKernelWeight(i) = exp((-3 i^2) / 25) for |i| = 0..4 under the contract's exp (tests/test_ssr_denoise_cpu.py pins the words)
VQD float kernel_weight(int i) {
    const int m = i < 0 ? -i : i;
    return __uint_as_float(m == 0 ? 0x3f800000u : m == 1 ? 0x3f630d38u : m == 2 ? 0x3f1e6897u : m == 3 ? 0x3eaddf76u : 0x3e162023u);
}
VQD float luminance(f3 c, bool dxc) { return max2(dot_rt(c, mk3(0.299f, 0.587f, 0.114f), dxc), 0.001f); }
VQD float temporal_variance(f3 history, f3 rad, bool dxc) {
    const float hl = luminance(history, dxc), l = luminance(rad, dxc);
    const float diff = fdiv_(abs_(hl - l), max2(max2(hl, l), 0.5f));
    return diff * diff;
}
VQD bool not_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }
// every CU filled once with as many workgroups as the kernel's registers and LDS admit; never more workgroups than the tile grid can list
template <typename K, typename A> hipError_t launch_tiles(hipStream_t s, K kernel, int perCU, const A& a, int nCUs) {
    if (nCUs <= 0) nCUs = 256;
    const uint32_t maxTiles = (uint32_t)a.tilesX * (uint32_t)a.tilesY;
    uint32_t blocks = (uint32_t)(perCU * nCUs);
    if (blocks > (maxTiles + 3u) / 4u) blocks = (maxTiles + 3u) / 4u;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}
template <typename K> int blocks_per_cu(K kernel) {
    int n = 0;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, 256, 0) == hipSuccess && n > 0 ? n : 2;
}
// the tile of list entry g: false when it lies beyond the tile grid (then nothing of the entry is used as an index)
VQD bool tile_origin(const uint32_t* tileList, uint32_t g, int tilesX, int tilesY, int* x0, int* y0) {
    const uint32_t e = tileList[g];
    const uint32_t tx = (e & 0xffffu) >> 3, ty = (e >> 16) >> 3;
    *x0 = (int)(tx * 8u); *y0 = (int)(ty * 8u);
    return tx < (uint32_t)tilesX && ty < (uint32_t)tilesY;
}

} // namespace dnsr
} // namespace vqk
