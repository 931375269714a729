// ssr_denoise.hip — passes 2 and 3 of SSR's reflection denoiser for gfx950 (docs/DESIGN_DETAILS.md §7.12):
//   k_ssr_prefilter        == Shaders/ScreenSpaceReflections/Prefilter.hlsl:CSMain + AMDFidelityFX/DNSR/ffx_denoiser_reflections_prefilter.h (the 15-tap edge-stopping filter)
//   k_ssr_resolve_temporal == Shaders/ScreenSpaceReflections/ResolveTemporal.hlsl:CSMain + ffx_denoiser_reflections_resolve_temporal.h (9 x 9 moments, history clip, blend)
// for every entry of the denoiser tile list vqhip_ssr_classify wrote. One wave64 per 8 x 8 tile, four waves per workgroup; a persistent grid strides over the
// list, whose length is read on the device. Each wave owns its 16 x 16 apron in LDS — the values the reference itself packs with f32tof16: the prefilter keeps them
// as packed halves (5 KB per wave), the temporal resolve as binary32 already rounded through binary16 (3 KB per wave); each form won its kernel's A/B
// (profiles/r10a_ssr_denoise.md) — and synchronises only with itself (waves of one workgroup run different numbers of tiles: no workgroup barrier inside the loop).
// Every expression is evaluated AS WRITTEN (products and sums rounded one by one, a / b the IEEE quotient), in the reading vqhip_set_arithmetic selects;
// min16float is binary32, exp(x) = exp2_(x * 1.44269502f).
#include "vq_internal.h"
#include "vq_devmath.h"
#include "vq_sampling.h"
#include "vq_ssr_denoise.h"

using namespace vqd;

namespace vqk {

namespace {

using namespace dnsr;

VQD uint32_t pack2(float a, float b) {
    const _Float16 ha = to_f16(a), hb = to_f16(b);
    return (uint32_t)__builtin_bit_cast(uint16_t, ha) | ((uint32_t)__builtin_bit_cast(uint16_t, hb) << 16);
}
VQD float lo16(uint32_t u) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(u & 0xffffu)); }
VQD float hi16(uint32_t u) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(u >> 16)); }

// one field of DXGI R11G11B10_FLOAT (5-bit exponent, bias 15, MB mantissa bits, unsigned) to binary32, exactly
template <int MB> VQD float small_float(uint32_t f) {
    const uint32_t e = f >> MB, m = f & ((1u << MB) - 1u);
    float r = __uint_as_float(((e + 112u) << 23) | (m << (23 - MB)));
    if (e == 31u) r = __uint_as_float(0x7f800000u | (m << (23 - MB)));
    if (e == 0u) r = (float)m * __uint_as_float((uint32_t)(127 - 14 - MB) << 23);
    return r;
}
VQD float4 load_avg(const SsrDenoiseArgs& a, int x, int y) {                                                       // x, y already clamped into the texture
    const size_t i = (size_t)y * a.avgW + x;
    if (a.avgF32) return ((const float4*)a.avg)[i];
    const uint32_t q = ((const uint32_t*)a.avg)[i];
    return make_float4(small_float<6>(q & 0x7ffu), small_float<6>((q >> 11) & 0x7ffu), small_float<5>(q >> 22), 0.0f);
}
// g_average_radiance.SampleLevel(g_linear_sampler, uv8, 0): bilinear, CLAMP, §3.4 (the rule of sample_2d_rg16f_clamp)
VQD f3 sample_average(const SsrDenoiseArgs& a, uint32_t px, uint32_t py) {
    const float u = fdiv_((float)px + 0.5f, a.roundUp8W), v = fdiv_((float)py + 0.5f, a.roundUp8H);
    int ix, iy; float wx, wy;
    fixed8(u * (float)a.avgW - 0.5f, &ix, &wx);
    fixed8(v * (float)a.avgH - 0.5f, &iy, &wy);
    const int x0 = min(max(ix, 0), a.avgW - 1), x1 = min(max(ix + 1, 0), a.avgW - 1);
    const int y0 = min(max(iy, 0), a.avgH - 1), y1 = min(max(iy + 1, 0), a.avgH - 1);
    const float4 r = blend4(load_avg(a, x0, y0), load_avg(a, x1, y0), load_avg(a, x0, y1), load_avg(a, x1, y1), wx, wy);
    return mk3(r.x, r.y, r.z);
}
VQD void store_out(const SsrDenoiseArgs& a, uint32_t x, uint32_t y, f3 c, float var) {
    if (x >= (uint32_t)a.width || y >= (uint32_t)a.height) return;                                                // a store outside the UAV is dropped
    const float4 v = make_float4(c.x, c.y, c.z, c.z);                                                             // radiance.xyzz
    if (a.outF32) store_px<0>(a.outRadiance, (size_t)y * a.outPitch + x, v); else store_px<1>(a.outRadiance, (size_t)y * a.outPitch + x, v);
    ((_Float16*)a.outVariance)[(size_t)y * a.outVariancePitch + x] = to_f16(var);
}
// FFX_DNSR_Reflections_GetRadianceWeight
VQD float radiance_weight(f3 avg, f3 rad, float variance, bool dxc) {
    return max2(exp_(-(0.6f + variance * 0.1f) * length_rt(sub(avg, rad), dxc)), 1.0e-2f);
}

// 15 offsets of ffx_denoiser_reflections_prefilter.h:111-112 as indices into the 16-wide apron: dy * 16 + dx
__device__ const int8_t kOffX[15] = { 0, -2, 2, -3, 1, -1, 3, -3, 0, -1, 2, -2, 1, 0, 3 };
__device__ const int8_t kOffY[15] = { 1, 1, -3, 0, 2, -2, 0, 3, -3, -1, 1, -2, 0, 2, -1 };

__global__ __launch_bounds__(256) void k_ssr_prefilter(SsrDenoiseArgs a) {
    __shared__ uint4 sA[4][256];                                                                                  // radiance.xy | radiance.z, variance | normal.xy | normal.z
    __shared__ float sD[4][256];                                                                                  // linear depth stays binary32
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint4* A = sA[wave];
    float* D = sD[wave];
    const uint32_t n = min(a.counters[1], (uint32_t)(a.tilesX * a.tilesY));
    const bool dxc = a.arithDxc != 0;
    const float fW = (float)a.width, fH = (float)a.height;
    for (uint32_t g = blockIdx.x * 4u + wave; g < n; g += gridDim.x * 4u) {
        int x0, y0;
        if (!tile_origin(a.tileList, g, a.tilesX, a.tilesY, &x0, &y0)) continue;                            // wave-uniform
        #pragma unroll
        for (int k = 0; k < 4; ++k) {                                                                             // FFX_DNSR_Reflections_LoadNeighborhood, Prefilter.hlsl:51-66
            const int idx = (int)lane + 64 * k, qx = x0 - 4 + (idx & 15), qy = y0 - 4 + (idx >> 4);
            f3 rad = mk3(0.0f, 0.0f, 0.0f), n01 = mk3(0.0f, 0.0f, 0.0f);
            float var = 0.0f, z = 0.0f;
            if ((uint32_t)qx < (uint32_t)a.width && (uint32_t)qy < (uint32_t)a.height) {                           // a load outside the texture reads 0
                rad = load_rgb(a.radiance, a.radF32, (size_t)qy * a.radiancePitch + qx);
                var = load_r16f(a.variance, (size_t)qy * a.variancePitch + qx);
                z = a.depth[(size_t)qy * a.depthPitch + qx];
                if (a.normF32) { const float4 q = ((const float4*)a.normals)[(size_t)qy * a.normalPitch + qx]; n01 = mk3(q.x, q.y, q.z); }
                else { const uint32_t q = ((const uint32_t*)a.normals)[(size_t)qy * a.normalPitch + qx];
                       n01 = mk3(fdiv_((float)(q & 1023u), 1023.0f), fdiv_((float)((q >> 10) & 1023u), 1023.0f), fdiv_((float)((q >> 20) & 1023u), 1023.0f)); }
            }
            const f3 nn = normalize_rt(mk3(2.0f * n01.x - 1.0f, 2.0f * n01.y - 1.0f, 2.0f * n01.z - 1.0f), dxc);
            // GetLinearDepth: |z / w| of InvProjectPosition(float3(uv, depth), invProjection), uv of this (possibly outside) pixel
            const float u = fdiv_((float)qx + 0.5f, fW), v = fdiv_((float)qy + 0.5f, fH);
            const float cy = 1.0f - v;
            const float cx2 = 2.0f * u - 1.0f, cy2 = 2.0f * cy - 1.0f;
            const float pz = ((cx2 * a.ipZ[0] + cy2 * a.ipZ[1]) + z * a.ipZ[2]) + 1.0f * a.ipZ[3];
            const float pw = ((cx2 * a.ipW[0] + cy2 * a.ipW[1]) + z * a.ipW[2]) + 1.0f * a.ipW[3];
            A[idx] = make_uint4(pack2(rad.x, rad.y), pack2(rad.z, var), pack2(nn.x, nn.y), pack2(nn.z, 0.0f));
            D[idx] = abs_(fdiv_(pz, pw));
        }
        wave_sync();
        const int lx = (int)(lane & 7u), ly = (int)(lane >> 3);
        const uint32_t px = (uint32_t)(x0 + lx), py = (uint32_t)(y0 + ly);
        const int c = (ly + 4) * 16 + lx + 4;
        const uint4 cq = A[c];
        const f3 cRad = mk3(lo16(cq.x), hi16(cq.x), lo16(cq.y)), cN = mk3(lo16(cq.z), hi16(cq.z), lo16(cq.w));
        const float cVar = hi16(cq.y), cD = D[c];
        float roughness = 0.0f;
        if (px < (uint32_t)a.width && py < (uint32_t)a.height) roughness = fdiv_((float)a.roughness[(size_t)py * a.width + px], 255.0f);
        f3 outRad = cRad;
        float outVar = cVar;
        const bool needs = cVar > 0.0f && roughness < a.roughnessThreshold && !(roughness < 0.04f);              // ffx_denoiser_reflections_prefilter.h:151
        if (needs) {
            const f3 avg = sample_average(a, px, py);
            // FFX_DNSR_Reflections_Resolve :102-136
            float aw = radiance_weight(avg, cRad, cVar, dxc);
            f3 ar = mul(cRad, aw);
            float av = (cVar * aw) * aw;
            const float vw = max2(0.1f, 1.0f - exp_(-(cVar * 4.4f)));
            #pragma unroll 1
            for (int i = 0; i < 15; ++i) {
                const int q = c + (int)kOffY[i] * 16 + (int)kOffX[i];
                const uint4 nq = A[q];
                const f3 nRad = mk3(lo16(nq.x), hi16(nq.x), lo16(nq.y)), nN = mk3(lo16(nq.z), hi16(nq.z), lo16(nq.w));
                const float nVar = hi16(nq.y), nD = D[q];
                const float wn = exp2_(512.0f * log2_(max2(dot_rt(cN, nN, dxc), 0.0f)));                          // pow(max(dot, 0), 512)
                const float wd = exp_((-abs_(cD - nD) * cD) * 4.0f);
                const float wr = radiance_weight(avg, nRad, cVar, dxc);
                const float w = (((1.0f * wn) * wd) * wr) * vw;
                aw += w;
                ar = mk3(ar.x + w * nRad.x, ar.y + w * nRad.y, ar.z + w * nRad.z);
                av += (w * w) * nVar;
            }
            outRad = mk3(fdiv_(ar.x, aw), fdiv_(ar.y, aw), fdiv_(ar.z, aw));
            outVar = fdiv_(av, aw * aw);
        }
        store_out(a, px, py, outRad, outVar);
        wave_sync();                                                                                              // the next tile overwrites the apron
    }
}

// FFX_DNSR_Reflections_ClipAABB, ffx_denoiser_reflections_common.h:105-128
VQD f3 clip_aabb(f3 lo, f3 hi, f3 prev) {
    const f3 centre = mk3(0.5f * (hi.x + lo.x), 0.5f * (hi.y + lo.y), 0.5f * (hi.z + lo.z));
    const f3 extent = mk3(0.5f * (hi.x - lo.x) + 0.001f, 0.5f * (hi.y - lo.y) + 0.001f, 0.5f * (hi.z - lo.z) + 0.001f);
    const f3 vec = sub(prev, centre);
    const float ux = abs_(fdiv_(vec.x, extent.x)), uy = abs_(fdiv_(vec.y, extent.y)), uz = abs_(fdiv_(vec.z, extent.z));
    const float mx = max2(max2(ux, uy), uz);
    if (mx > 1.0f) return mk3(centre.x + fdiv_(vec.x, mx), centre.y + fdiv_(vec.y, mx), centre.z + fdiv_(vec.z, mx));
    return prev;
}

__global__ __launch_bounds__(256) void k_ssr_resolve_temporal(SsrDenoiseArgs a) {
    __shared__ float sA[4][3][256];                                                                               // radiance x | y | z, already rounded through binary16
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    float (*A)[256] = sA[wave];
    const uint32_t n = min(a.counters[1], (uint32_t)(a.tilesX * a.tilesY));
    const bool dxc = a.arithDxc != 0;
    for (uint32_t g = blockIdx.x * 4u + wave; g < n; g += gridDim.x * 4u) {
        int x0, y0;
        if (!tile_origin(a.tileList, g, a.tilesX, a.tilesY, &x0, &y0)) continue;
        #pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int idx = (int)lane + 64 * k, qx = x0 - 4 + (idx & 15), qy = y0 - 4 + (idx >> 4);
            f3 rad = mk3(0.0f, 0.0f, 0.0f);
            if ((uint32_t)qx < (uint32_t)a.width && (uint32_t)qy < (uint32_t)a.height) rad = load_rgb(a.radiance, a.radF32, (size_t)qy * a.radiancePitch + qx);
            A[0][idx] = rh(rad.x); A[1][idx] = rh(rad.y); A[2][idx] = rh(rad.z);
        }
        wave_sync();
        const int lx = (int)(lane & 7u), ly = (int)(lane >> 3);
        const uint32_t px = (uint32_t)(x0 + lx), py = (uint32_t)(y0 + ly);
        const bool onScreen = px < (uint32_t)a.width && py < (uint32_t)a.height;
        const int c = (ly + 4) * 16 + lx + 4;
        f3 sig = mk3(A[0][c], A[1][c], A[2][c]);
        float roughness = 0.0f, var = 0.0f;
        if (onScreen) { roughness = fdiv_((float)a.roughness[(size_t)py * a.width + px], 255.0f); var = load_r16f(a.variance, (size_t)py * a.variancePitch + px); }
        if (roughness < a.roughnessThreshold) {                                                                   // ffx_denoiser_reflections_resolve_temporal.h:111
            float ns = 0.0f;
            f3 old = mk3(0.0f, 0.0f, 0.0f);
            if (onScreen) { ns = load_r16f(a.sampleCount, (size_t)py * a.sampleCountPitch + px); old = load_rgb(a.reprojected, a.reprojF32, (size_t)py * a.reprojectedPitch + px); }
            const f3 avg = sample_average(a, px, py);
            // FFX_DNSR_Reflections_EstimateLocalNeighborhoodInGroup :50-70: j outer, i inner
            f3 mean = mk3(0.0f, 0.0f, 0.0f), m2 = mk3(0.0f, 0.0f, 0.0f);
            float acc = 0.0f;
            #pragma unroll 1                                                                                      // a row of nine taps in flight; all 81 cost every register the wave has
            for (int j = -4; j <= 4; ++j) {
                const float kj = kernel_weight(j);
                #pragma unroll
                for (int i = -4; i <= 4; ++i) {
                    const int q = c + j * 16 + i;
                    const f3 r = mk3(A[0][q], A[1][q], A[2][q]);
                    const float w = kernel_weight(i) * kj;
                    acc += w;
                    mean = mk3(mean.x + r.x * w, mean.y + r.y * w, mean.z + r.z * w);
                    m2 = mk3(m2.x + (r.x * r.x) * w, m2.y + (r.y * r.y) * w, m2.z + (r.z * r.z) * w);
                }
            }
            mean = mk3(fdiv_(mean.x, acc), fdiv_(mean.y, acc), fdiv_(mean.z, acc));
            m2 = mk3(abs_(fdiv_(m2.x, acc) - mean.x * mean.x), abs_(fdiv_(m2.y, acc) - mean.y * mean.y), abs_(fdiv_(m2.z, acc) - mean.z * mean.z));
            const float ln = length_rt(sub(mean, avg), dxc);
            const f3 sd = mk3(((sqrt_(m2.x) + ln) * a.temporalStability) * 1.4f, ((sqrt_(m2.y) + ln) * a.temporalStability) * 1.4f,
                              ((sqrt_(m2.z) + ln) * a.temporalStability) * 1.4f);
            mean = mk3(lerp_w(mean.x, avg.x, 0.2f), lerp_w(mean.y, avg.y, 0.2f), lerp_w(mean.z, avg.z, 0.2f));
            const f3 oldC = clip_aabb(sub(mean, sd), add(mean, sd), old);
            const float speed = fdiv_(1.0f, max2(ns, 1.0f));
            const float weight = 1.0f - speed;
            const float t = fdiv_(1.0f, max2(ns + 1.0f, 1.0f));
            sig = mk3(lerp_w(sig.x, avg.x, t), lerp_w(sig.y, avg.y, t), lerp_w(sig.z, avg.z, t));
            const f3 sd1 = mk3(sd.x * 1.0f, sd.y * 1.0f, sd.z * 1.0f);
            sig = clip_aabb(sub(avg, sd1), add(avg, sd1), sig);
            sig = mk3(lerp_w(sig.x, oldC.x, weight), lerp_w(sig.y, oldC.y, weight), lerp_w(sig.z, oldC.z, weight));
            var = lerp_w(temporal_variance(sig, oldC, dxc), var, weight);
            if (not_finite(sig.x) || not_finite(sig.y) || not_finite(sig.z) || not_finite(var)) { sig = mk3(0.0f, 0.0f, 0.0f); var = 0.0f; }
        }
        store_out(a, px, py, sig, var);
        wave_sync();
    }
}

} // namespace

hipError_t launch_ssr_prefilter(hipStream_t s, const SsrDenoiseArgs& a, int nCUs) {
    static const int perCU = blocks_per_cu(k_ssr_prefilter);
    return launch_tiles(s, k_ssr_prefilter, perCU, a, nCUs);
}

hipError_t launch_ssr_resolve_temporal(hipStream_t s, const SsrDenoiseArgs& a, int nCUs) {
    static const int perCU = blocks_per_cu(k_ssr_resolve_temporal);
    return launch_tiles(s, k_ssr_resolve_temporal, perCU, a, nCUs);
}

} // namespace vqk
