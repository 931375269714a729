// msaa.hip — the lit draw into the 4-sample scene colour and its resolve (vqhip_forward_lighting_msaa, docs/DESIGN_DETAILS.md §7.9): the bMSAA
// branch of RenderSceneColor (SceneRendering.cpp:1644-1650) + ResolveMSAA (:2060-2112). PSMain runs once per (pixel, primitive); its per-fragment
// arithmetic is vq_shade.h:shade_pixel, unchanged. Two kernels:
//   k_msaa_shade : one lane per pixel, laid out like k_forward_lighting. Works out the owner of each sample from the coverage bytes, shades the
//                  lowest owning layer f. A pixel whose four samples all belong to f (interiors) or to the background (sky) is resolved and written
//                  here; any other pixel gets f's SAMPLE value and is appended to the edge list (one atomic per wave).
//   k_msaa_edges : persistent, grid-stride over the edge list (the count is read on the device: the host never waits for it). Per pixel: shades
//                  every other owning layer once, reads f's sample back from `out`, fetches the background, resolves in sample order.
// An edge pixel's result does not depend on which other pixels share its wave: shade_pixel's wave-uniform forms give the same bits whatever the
// neighbours (vq_shade.h), so the run-to-run order of the list is invisible in the output.
#include "vq_shade.h"

namespace {

using vqk::MsaaArgs;

// the value a sample holds once stored in the output format, widened back to binary32 (FMT 0 = RGBA32F, 1 = RGBA16F)
template <int FMT> VQD float4 stored(float4 c) {
    if (FMT == 0) return c;
    return make_float4((float)to_f16(c.x), (float)to_f16(c.y), (float)to_f16(c.z), (float)to_f16(c.w));
}
// ResolveSubresource of a 4-sample RGBA pixel as the project states it: per channel (((s0 + s1) + s2) + s3) * 0.25 in binary32
VQD float4 resolve4(float4 s0, float4 s1, float4 s2, float4 s3) {
    return make_float4((((s0.x + s1.x) + s2.x) + s3.x) * 0.25f, (((s0.y + s1.y) + s2.y) + s3.y) * 0.25f,
                       (((s0.z + s1.z) + s2.z) + s3.z) * 0.25f, (((s0.w + s1.w) + s2.w) + s3.w) * 0.25f);
}

// own[k] = the samples of pixel (x, y) owned by layer k (lowest layer whose mask has the bit); returns the background's samples
VQD uint32_t ownership(const MsaaArgs& a, int x, int y, uint32_t own[VQHIP_MSAA_MAX_LAYERS]) {
    const size_t c = (size_t)y * a.covPitch + x;
    uint32_t rem = 0xFu;
    #pragma unroll
    for (int k = 0; k < VQHIP_MSAA_MAX_LAYERS; ++k) {
        const uint32_t m = k < a.layers ? (uint32_t)a.L[k].cov[c] : 0u;      // wave-uniform test
        own[k] = m & rem;
        rem &= ~m;
    }
    return rem;
}
// own[k] for a per-lane k, by selects (a run-time index into a register array would go through scratch)
VQD uint32_t pick(const uint32_t own[VQHIP_MSAA_MAX_LAYERS], int k) {
    return k == 0 ? own[0] : k == 1 ? own[1] : k == 2 ? own[2] : own[3];
}
// the G-buffer record of layer k (per-lane k) at (x, y)
template <bool NT>
VQD void load_record(const MsaaArgs& a, int k, int x, int y, float4& g0, float4& g1, float4& g2, float4& g3) {
    // one load block per layer under a per-lane test (constant indices into the argument block: a run-time index, or a select of its
    // addresses, puts a copy of the block in scratch)
    #pragma unroll
    for (int j = 0; j < VQHIP_MSAA_MAX_LAYERS; ++j) {
        if (k != j) continue;
        const vqk::MsaaLayer& L = a.L[j];
        const size_t i = (size_t)y * L.pitch + x;
        if (NT) {      // read once and never again: non-temporal, as k_forward_lighting does
            typedef float v4f __attribute__((ext_vector_type(4)));
            auto ntload = [](const float4* p) { const v4f v = __builtin_nontemporal_load((const v4f*)p); return make_float4(v.x, v.y, v.z, v.w); };
            g0 = ntload(&L.gb0[i]); g1 = ntload(&L.gb1[i]); g2 = ntload(&L.gb2[i]); g3 = ntload(&L.gb3[i]);
        } else {
            g0 = L.gb0[i]; g1 = L.gb1[i]; g2 = L.gb2[i]; g3 = L.gb3[i];
        }
    }
}
template <int FMT> VQD float4 background(const MsaaArgs& a, int x, int y) {
    return a.bg ? load_px<FMT>(a.bg, (size_t)y * a.bgPitch + x) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}
VQD int lowest_owner(const uint32_t own[VQHIP_MSAA_MAX_LAYERS]) {
    return own[0] ? 0 : own[1] ? 1 : own[2] ? 2 : own[3] ? 3 : -1;
}

template <bool HAS_ENV, bool HAS_CASTERS, int OUTFMT, int AR>
__global__ __launch_bounds__(256, VQ_SHADE_WAVES) void k_msaa_shade(MsaaArgs a) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    const bool in = x < a.width;
    int f = -1;
    bool edge = false;
    if (in) {
        uint32_t own[VQHIP_MSAA_MAX_LAYERS];
        const uint32_t bgm = ownership(a, x, y, own);
        f = lowest_owner(own);
        edge = (f >= 0 ? pick(own, f) : bgm) != 0xFu;                      // f < 0: every sample is background
    }
    // the wave's edge pixels go on the list BEFORE shading (less state live across shade_pixel): one atomic per wave, slots in lane order
    const uint64_t b = __builtin_amdgcn_ballot_w64(edge);
    if (b) {
        const int leader = __builtin_ctzll(b);                               // wave-uniform
        uint32_t base = 0;
        if ((int)__lane_id() == leader) base = atomicAdd(a.edgeCount, (uint32_t)__builtin_popcountll(b));
        base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
        if (edge) {
            const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
            a.edgeList[base + below] = (uint32_t)y * (uint32_t)a.width + (uint32_t)x;
        }
    }
    if (!in) return;
    float4 v;
    if (f >= 0) {
        float4 g0, g1, g2, g3;
        load_record<true>(a, f, x, y, g0, g1, g2, g3);
        v = stored<OUTFMT>(shade_pixel<HAS_ENV, HAS_CASTERS, AR>(g0, g1, g2, g3, a.fc));
    } else {
        v = background<OUTFMT>(a, x, y);
    }
    // interior / sky: the resolve of four equal samples; edge pixel: f's sample value, resolved by k_msaa_edges
    store_px<OUTFMT>(a.out, (size_t)y * a.outPitch + x, edge ? v : resolve4(v, v, v, v));
}

template <bool HAS_ENV, bool HAS_CASTERS, int OUTFMT, int AR>
__global__ __launch_bounds__(256, VQ_SHADE_WAVES) void k_msaa_edges(MsaaArgs a) {
    const uint32_t n = *a.edgeCount;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        const uint32_t p = a.edgeList[e];
        const int y = (int)(p / (uint32_t)a.width), x = (int)(p - (uint32_t)y * (uint32_t)a.width);
        uint32_t own[VQHIP_MSAA_MAX_LAYERS];
        const uint32_t bgm = ownership(a, x, y, own);
        const int f = lowest_owner(own);                                     // >= 0: an all-background pixel is never listed
        const size_t o = (size_t)y * a.outPitch + x;
        const float4 vf = load_px<OUTFMT>(a.out, o);                         // f's sample value, written by k_msaa_shade
        const float4 vb = bgm ? background<OUTFMT>(a, x, y) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float4 s[4];
        #pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = ((bgm >> j) & 1u) ? vb : vf;
        uint32_t todo = 0;                                                   // the other owning layers
        #pragma unroll
        for (int k = 0; k < VQHIP_MSAA_MAX_LAYERS; ++k) todo |= (own[k] != 0u ? 1u : 0u) << k;
        todo &= ~(1u << f);
        while (todo) {                                                       // one shade per iteration and lane: shade_pixel is inlined once
            const int k = __builtin_ctz(todo);
            todo &= todo - 1u;
            float4 g0, g1, g2, g3;
            load_record<false>(a, k, x, y, g0, g1, g2, g3);
            const float4 v = stored<OUTFMT>(shade_pixel<HAS_ENV, HAS_CASTERS, AR>(g0, g1, g2, g3, a.fc));
            const uint32_t m = pick(own, k);
            #pragma unroll
            for (int j = 0; j < 4; ++j) if ((m >> j) & 1u) s[j] = v;
        }
        store_px<OUTFMT>(a.out, o, resolve4(s[0], s[1], s[2], s[3]));
    }
}

template <bool E, bool C, int FMT, int AR>
hipError_t launch_pair(hipStream_t s, const MsaaArgs& a, dim3 grid, int wg, int nCUs, int edgeWgs) {
    hipLaunchKernelGGL((k_msaa_shade<E, C, FMT, AR>), grid, dim3(wg), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // k_msaa_edges fills every CU once: as many 256-lane workgroups per CU as its register budget admits (queried once per instantiation).
    // Option "msaa_edge_wgs" overrides the number of workgroups (tests: the grid-stride step with a list longer than the grid); edgeWgs comes
    // clamped from launch_forward_lighting_msaa.
    static const int perCU = [] {
        int n = 0;
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_msaa_edges<E, C, FMT, AR>, 256, 0) == hipSuccess && n > 0 ? n : 2;
    }();
    hipLaunchKernelGGL((k_msaa_edges<E, C, FMT, AR>), dim3(edgeWgs > 0 ? edgeWgs : perCU * nCUs), dim3(256), 0, s, a);
    return hipGetLastError();
}
template <bool E, bool C>
hipError_t launch_fmt(hipStream_t s, const MsaaArgs& a, int outFmt, int arithDxc, dim3 grid, int wg, int nCUs, int edgeWgs) {
    if (outFmt == VQHIP_FMT_RGBA32F) return arithDxc ? launch_pair<E, C, 0, 1>(s, a, grid, wg, nCUs, edgeWgs) : launch_pair<E, C, 0, 0>(s, a, grid, wg, nCUs, edgeWgs);
    return arithDxc ? launch_pair<E, C, 1, 1>(s, a, grid, wg, nCUs, edgeWgs) : launch_pair<E, C, 1, 0>(s, a, grid, wg, nCUs, edgeWgs);
}

} // namespace

namespace vqk {
hipError_t launch_forward_lighting_msaa(hipStream_t s, const MsaaArgs& a, bool hasEnv, bool hasCasters, int outFmt, int arithDxc, int nCUs, const Options& opt) {
    // k_msaa_shade: the workgroup shape of k_forward_lighting's default (shade.hip), option "shade_wg" overrides it here as there; k_msaa_edges walks the
    // list whatever its length
    int wg = (size_t)a.width * a.height < ((size_t)4 << 20) ? 64 : 256;
    if (opt.shadeWg == 64 || opt.shadeWg == 128 || opt.shadeWg == 256) wg = opt.shadeWg;
    const dim3 grid((a.width + wg - 1) / wg, a.height);
    if (nCUs <= 0) nCUs = 256;
    // "msaa_edge_wgs": never more workgroups than one lane per pixel needs (the list holds at most width * height entries), nor than 65 536 — the
    // kernel's stride gridDim.x * 256 is a 32-bit product, and a stride that wrapped to 0 would never leave the loop
    int edgeWgs = 0;
    if (opt.msaaEdgeWgs > 0) {
        const size_t perPixel = ((size_t)a.width * a.height + 255) / 256;
        const size_t cap = perPixel < 65536 ? perPixel : 65536;
        edgeWgs = (size_t)opt.msaaEdgeWgs < cap ? opt.msaaEdgeWgs : (int)cap;
    }
    if (hasEnv) return hasCasters ? launch_fmt<true, true>(s, a, outFmt, arithDxc, grid, wg, nCUs, edgeWgs) : launch_fmt<true, false>(s, a, outFmt, arithDxc, grid, wg, nCUs, edgeWgs);
    return hasCasters ? launch_fmt<false, true>(s, a, outFmt, arithDxc, grid, wg, nCUs, edgeWgs) : launch_fmt<false, false>(s, a, outFmt, arithDxc, grid, wg, nCUs, edgeWgs);
}
} // namespace vqk
