// ssr_reproject.hip — pass 1 of SSR's reflection denoiser for gfx950 (docs/DESIGN_DETAILS.md §7.13):
//   k_ssr_reproject == Shaders/ScreenSpaceReflections/Reproject.hlsl:CSMain + AMDFidelityFX/DNSR/ffx_denoiser_reflections_reproject.h (9 x 9 local moments, the choice
//   between hit-point and surface reprojection, the 3 x 3 search and the 2 x 2 path on disocclusion, the variance / sample-count update, the 8 x 8 -> 1 average radiance)
// for every entry of the denoiser tile list. The shape is §7.12's: one wave64 per 8 x 8 tile, four waves per workgroup, a persistent grid striding over the list whose
// length is read on the device, the 16 x 16 apron in the wave's own LDS as binary32 already rounded through binary16 (3 KB per wave), wave-local synchronisation only. The
// 8 x 8 -> 1 downsample reuses the apron's space. History fetches are bilinear gathers in software: texels decoded to binary32, CLAMP, 8-bit fractions, the blend4 FMA
// chain. Every expression is evaluated AS WRITTEN, in the reading vqhip_set_arithmetic selects; the centre radiance and ray length are NOT rounded through binary16.
#include "vq_internal.h"
#include "vq_devmath.h"
#include "vq_sampling.h"
#include "vq_ssr_denoise.h"

using namespace vqd;

namespace vqk {

namespace {

using namespace dnsr;

VQD float min2(float a, float b) { return (b < a || a != a) ? b : a; }

// the four texels and the two fractions of one SampleLevel(g_linear_sampler, uv, 0) on a width x height plane: every address is clamped into the plane
struct Bil { int x0, x1, y0, y1; float wx, wy; };
VQD Bil bilinear(float u, float v, int width, int height) {
    Bil b;
    int ix, iy;
    fixed8(u * (float)width - 0.5f, &ix, &b.wx);
    fixed8(v * (float)height - 0.5f, &iy, &b.wy);
    b.x0 = min(max(ix, 0), width - 1); b.x1 = min(max(ix + 1, 0), width - 1);
    b.y0 = min(max(iy, 0), height - 1); b.y1 = min(max(iy + 1, 0), height - 1);
    return b;
}
VQD float blend1(float c00, float c10, float c01, float c11, float wx, float wy) {
    const float w00 = (1.0f - wx) * (1.0f - wy), w10 = wx * (1.0f - wy), w01 = (1.0f - wx) * wy, w11 = wx * wy;
    return fma_(w11, c11, fma_(w01, c01, fma_(w10, c10, w00 * c00)));
}
VQD f3 blend3(f3 c00, f3 c10, f3 c01, f3 c11, float wx, float wy) {
    return mk3(blend1(c00.x, c10.x, c01.x, c11.x, wx, wy), blend1(c00.y, c10.y, c01.y, c11.y, wx, wy), blend1(c00.z, c10.z, c01.z, c11.z, wx, wy));
}
VQD f3 load_normal01(const void* plane, int f32, size_t i) {
    if (f32) { const float4 q = ((const float4*)plane)[i]; return mk3(q.x, q.y, q.z); }
    const uint32_t q = ((const uint32_t*)plane)[i];
    return mk3(fdiv_((float)(q & 1023u), 1023.0f), fdiv_((float)((q >> 10) & 1023u), 1023.0f), fdiv_((float)((q >> 20) & 1023u), 1023.0f));
}
VQD f3 world_normal(f3 n01, bool dxc) { return normalize_rt(mk3(2.0f * n01.x - 1.0f, 2.0f * n01.y - 1.0f, 2.0f * n01.z - 1.0f), dxc); }
VQD float load_r8(const uint8_t* plane, size_t i) { return fdiv_((float)plane[i], 255.0f); }

#define VQ_BIL4(pitch) (size_t)b.y0 * (pitch) + b.x0, (size_t)b.y0 * (pitch) + b.x1, (size_t)b.y1 * (pitch) + b.x0, (size_t)b.y1 * (pitch) + b.x1
VQD float sample_depth_history(const SsrReprojectArgs& a, Bil b) {
    const size_t i[4] = { VQ_BIL4(a.depthHistPitch) };
    return blend1(a.depthHist[i[0]], a.depthHist[i[1]], a.depthHist[i[2]], a.depthHist[i[3]], b.wx, b.wy);
}
VQD f3 sample_normal_history(const SsrReprojectArgs& a, Bil b, bool dxc) {                                          // FFX_DNSR_Reflections_SampleWorldSpaceNormalHistory
    const size_t i[4] = { VQ_BIL4(a.normalHistPitch) };
    return world_normal(blend3(load_normal01(a.normalHist, a.normHistF32, i[0]), load_normal01(a.normalHist, a.normHistF32, i[1]),
                               load_normal01(a.normalHist, a.normHistF32, i[2]), load_normal01(a.normalHist, a.normHistF32, i[3]), b.wx, b.wy), dxc);
}
VQD f3 sample_radiance_history(const SsrReprojectArgs& a, Bil b) {
    const size_t i[4] = { VQ_BIL4(a.radianceHistPitch) };
    return blend3(load_rgb(a.radianceHist, a.radHistF32, i[0]), load_rgb(a.radianceHist, a.radHistF32, i[1]), load_rgb(a.radianceHist, a.radHistF32, i[2]),
                  load_rgb(a.radianceHist, a.radHistF32, i[3]), b.wx, b.wy);
}
VQD float sample_roughness_history(const SsrReprojectArgs& a, Bil b) {
    const size_t i[4] = { VQ_BIL4(a.roughnessHistPitch) };
    return blend1(load_r8(a.roughnessHist, i[0]), load_r8(a.roughnessHist, i[1]), load_r8(a.roughnessHist, i[2]), load_r8(a.roughnessHist, i[3]), b.wx, b.wy);
}
VQD float sample_r16f(const void* plane, int pitch, Bil b) {
    const size_t i[4] = { VQ_BIL4(pitch) };
    return blend1(load_r16f(plane, i[0]), load_r16f(plane, i[1]), load_r16f(plane, i[2]), load_r16f(plane, i[3]), b.wx, b.wy);
}
#undef VQ_BIL4

// FFX_DNSR_Reflections_GetLinearDepth(uv, depth): |z / w| of InvProjectPosition — columns 2 and 3 only
VQD float linear_depth(const SsrReprojectArgs& a, float u, float v, float z) {
    const float cy = 1.0f - v;
    const float cx2 = 2.0f * u - 1.0f, cy2 = 2.0f * cy - 1.0f;
    const VQ_matrix& M = a.invProj;
    const float pz = ((cx2 * M.m[0][2] + cy2 * M.m[1][2]) + z * M.m[2][2]) + 1.0f * M.m[3][2];
    const float pw = ((cx2 * M.m[0][3] + cy2 * M.m[1][3]) + z * M.m[2][3]) + 1.0f * M.m[3][3];
    return abs_(fdiv_(pz, pw));
}
// mul(M, float4(p, 1)) in §7.11's form
VQD float4 mul_point(const VQ_matrix& M, float x, float y, float z) {
    float o[4];
    #pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = ((x * M.m[0][j] + y * M.m[1][j]) + z * M.m[2][j]) + 1.0f * M.m[3][j];
    return make_float4(o[0], o[1], o[2], o[3]);
}
// FFX_DNSR_Reflections_GetDisocclusionFactor
VQD float disocclusion(f3 n, f3 hn, float ld, float hld, bool dxc) {
    const float wn = exp_((-abs_(1.0f - max2(0.0f, dot_rt(n, hn, dxc)))) * 1.4f);
    const float wd = exp_(fdiv_(-abs_(hld - ld), ld) * 1.0f);
    return (1.0f * wn) * wd;
}
VQD f3 mix4(f3 a, f3 b, f3 c, f3 d, float4 w) {
    return mk3(((a.x * w.x + b.x * w.y) + c.x * w.z) + d.x * w.w, ((a.y * w.x + b.y * w.y) + c.y * w.z) + d.y * w.w, ((a.z * w.x + b.z * w.y) + c.z * w.z) + d.z * w.w);
}

// one field of DXGI R11G11B10_FLOAT from binary32 in ONE rounding to nearest even: 5-bit exponent (bias 15), MB mantissa bits, denormals kept, overflow to inf,
// negative values and -0 -> 0, NaN -> exponent 31 with the top mantissa bit (§7.13; tests/ssr_reproject_ref.py:encode_r11g11b10)
template <int MB> VQD uint32_t to_small_float(float x) {
    const uint32_t bits = __float_as_uint(x), mag = bits & 0x7fffffffu;
    if (mag > 0x7f800000u) return (31u << MB) | (1u << (MB - 1));
    if (bits >> 31) return 0u;
    const int e = (int)(mag >> 23) - 112;                                                                         // the exponent re-biased to 15
    uint32_t val = mag - (112u << 23), sh = 23u - MB;                                                             // normal: exponent and mantissa as one integer, a carry runs into the exponent
    if (e < 1) { val = (mag & 0x7fffffu) | 0x800000u; sh = (uint32_t)min(23 - MB + 1 - e, 31); }                   // a denormal result drops (1 - e) more bits
    uint32_t q = val >> sh;
    const uint32_t rem = val & ((1u << sh) - 1u), half = 1u << (sh - 1u);
    if (rem > half || (rem == half && (q & 1u))) ++q;
    return min(q, 31u << MB);
}

struct TexelHistory { f3 rad, n; float ld; };
// the 2 x 2 path's Load of one history texel (outside the frame 0); the depth is linearised with the REPROJECTION uv
VQD TexelHistory load_history(const SsrReprojectArgs& a, int x, int y, float ru, float rv, bool dxc) {
    f3 rad = mk3(0.0f, 0.0f, 0.0f), n01 = mk3(0.0f, 0.0f, 0.0f);
    float z = 0.0f;
    if ((uint32_t)x < (uint32_t)a.width && (uint32_t)y < (uint32_t)a.height) {
        rad = load_rgb(a.radianceHist, a.radHistF32, (size_t)y * a.radianceHistPitch + x);
        n01 = load_normal01(a.normalHist, a.normHistF32, (size_t)y * a.normalHistPitch + x);
        z = a.depthHist[(size_t)y * a.depthHistPitch + x];
    }
    TexelHistory t;
    t.rad = rad; t.n = world_normal(n01, dxc); t.ld = linear_depth(a, ru, rv, z);
    return t;
}

// Four waves per SIMD: left alone the compiler takes 133 VGPRs (three waves); held to 128 it spills nothing and the pass runs 526 us instead of 627 us at 3840 x 2160
// (profiles/r11a_ssr_reproject.md; five waves would spill 132 B per lane).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_ssr_reproject(SsrReprojectArgs a) {
    __shared__ float sA[4][3][256];                                                                               // radiance x | y | z, already rounded through binary16
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    float (*A)[256] = sA[wave];
    float* S = &sA[wave][0][0];                                                                                   // the downsample's 4 x 64 values live in the apron's space
    const uint32_t n = min(a.counters[1], (uint32_t)(a.tilesX * a.tilesY));
    const bool dxc = a.arithDxc != 0;
    const float fW = (float)a.width, fH = (float)a.height;
    for (uint32_t g = blockIdx.x * 4u + wave; g < n; g += gridDim.x * 4u) {
        int x0, y0;
        if (!tile_origin(a.tileList, g, a.tilesX, a.tilesY, &x0, &y0)) continue;                                  // wave-uniform
        #pragma unroll
        for (int k = 0; k < 4; ++k) {                                                                             // FFX_DNSR_Reflections_InitializeGroupSharedMemory
            const int idx = (int)lane + 64 * k, qx = x0 - 4 + (idx & 15), qy = y0 - 4 + (idx >> 4);
            f3 rad = mk3(0.0f, 0.0f, 0.0f);
            if ((uint32_t)qx < (uint32_t)a.width && (uint32_t)qy < (uint32_t)a.height) rad = load_rgb(a.radiance, a.radF32, (size_t)qy * a.radiancePitch + qx);
            A[0][idx] = rh(rad.x); A[1][idx] = rh(rad.y); A[2][idx] = rh(rad.z);
        }
        wave_sync();
        const int lx = (int)(lane & 7u), ly = (int)(lane >> 3);
        const int px = x0 + lx, py = y0 + ly;
        const bool onScreen = px < a.width && py < a.height;
        const int c = (ly + 4) * 16 + lx + 4;
        f3 rad = mk3(0.0f, 0.0f, 0.0f);
        float rayLength = 0.0f, roughness = 0.0f;
        if (onScreen) {
            const float4 q = a.radF32 ? load_px<0>(a.radiance, (size_t)py * a.radiancePitch + px) : load_px<1>(a.radiance, (size_t)py * a.radiancePitch + px);
            rad = mk3(q.x, q.y, q.z); rayLength = q.w;                                                            // the centre is not rounded through binary16
            roughness = load_r8(a.roughness, (size_t)py * a.roughnessPitch + px);
        }
        // a pixel beyond the frame stores nothing and enters the average as zero: nothing of the reprojection is observable for it
        if (onScreen && roughness < a.roughnessThreshold) {                                                       // FFX_DNSR_Reflections_IsGlossyReflection
            // FFX_DNSR_Reflections_EstimateLocalNeighborhoodInGroup: j outer, i inner
            f3 mean = mk3(0.0f, 0.0f, 0.0f), m2 = mk3(0.0f, 0.0f, 0.0f);
            float acc = 0.0f;
            #pragma unroll 1                                                                                      // a row of nine taps in flight (§7.12's measurement)
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
            // FFX_DNSR_Reflections_PickReprojection
            const float u = fdiv_((float)px + 0.5f, fW), v = fdiv_((float)py + 0.5f, fH);
            const f3 normal = world_normal(load_normal01(a.normals, a.normF32, (size_t)py * a.normalPitch + px), dxc);
            float2 mv;
            if (a.motionF32) mv = ((const float2*)a.motion)[(size_t)py * a.motionPitch + px];
            else { const h2 q = ((const h2*)a.motion)[(size_t)py * a.motionPitch + px]; mv = make_float2((float)q.x, (float)q.y); }
            const float su = u - mv.x * 0.5f, sv = v - mv.y * -0.5f;                                              // GetSurfaceReprojection
            const float z = a.depth[(size_t)py * a.depthPitch + px];
            float hu, hv;
            {                                                                                                     // GetHitPositionReprojection
                const float cy = 1.0f - v;
                const float4 p = mul_point(a.invProj, 2.0f * u - 1.0f, 2.0f * cy - 1.0f, z);
                f3 ray = mk3(fdiv_(p.x, p.w), fdiv_(p.y, p.w), fdiv_(p.z, p.w));
                const float surfaceDepth = length_rt(ray, dxc);
                const float len = surfaceDepth + rayLength;
                ray = mk3(fdiv_(ray.x, surfaceDepth) * len, fdiv_(ray.y, surfaceDepth) * len, fdiv_(ray.z, surfaceDepth) * len);
                const float4 wp = mul_point(a.invView, ray.x, ray.y, ray.z);
                const float4 q = mul_point(a.prevViewProj, wp.x, wp.y, wp.z);
                hu = 0.5f * fdiv_(q.x, q.w) + 0.5f;
                hv = 1.0f - (0.5f * fdiv_(q.y, q.w) + 0.5f);
            }
            const Bil sb = bilinear(su, sv, a.width, a.height), hb = bilinear(hu, hv, a.width, a.height);
            const f3 sN = sample_normal_history(a, sb, dxc), hN = sample_normal_history(a, hb, dxc);
            const f3 sHist = sample_radiance_history(a, sb), hHist = sample_radiance_history(a, hb);
            const f3 nn = normalize_rt(normal, dxc);
            const float hSim = dot_rt(normalize_rt(hN, dxc), nn, dxc), sSim = dot_rt(normalize_rt(sN, dxc), nn, dxc);
            const float hR = sample_roughness_history(a, hb), sR = sample_roughness_history(a, sb);
            bool picked = true;
            float ru = su, rv = sv;
            f3 histN = sN, rep = sHist;
            Bil rb = sb;
            if (hSim > 0.9999f && hSim + 1.0e-3f > sSim && abs_(hR - roughness) < abs_(sR - roughness) + 1.0e-3f) {
                ru = hu; rv = hv; histN = hN; rep = hHist; rb = hb;
            } else {
                const f3 d = sub(sHist, mean);
                picked = dot_rt(d, d, dxc) < 1.5f * length_rt(m2, dxc);                                           // else: disocclusion_factor = 0; return
            }
            f3 stRep = mk3(0.0f, 0.0f, 0.0f);
            float stVar = 1.0f, stCnt = 1.0f;
            if (picked) {
                const float ld = linear_depth(a, u, v, z);
                float df = disocclusion(normal, histN, ld, linear_depth(a, ru, rv, sample_depth_history(a, rb)), dxc);
                if (df < 0.9f) {                                                                                  // exactly 0.9 takes neither the early-out nor the blocks below
                    const float du = fdiv_(1.0f, fW), dv = fdiv_(1.0f, fH);
                    #pragma unroll 1
                    for (int y = -1; y <= 1; ++y) {
                        #pragma unroll 1
                        for (int x = -1; x <= 1; ++x) {                                                           // offsets from the UPDATED reprojection_uv, as written
                            const float tu = ru + (float)x * du, tv = rv + (float)y * dv;
                            const Bil tb = bilinear(tu, tv, a.width, a.height);
                            const float w = disocclusion(normal, sample_normal_history(a, tb, dxc), ld, linear_depth(a, tu, tv, sample_depth_history(a, tb)), dxc);
                            if (w > df) { df = w; ru = tu; rv = tv; }
                        }
                    }
                    rb = bilinear(ru, rv, a.width, a.height);
                    rep = sample_radiance_history(a, rb);
                    if (df < 0.9f) {                                                                              // the 2 x 2 slow path
                        const float fx = fW * ru + 0.5f, fy = fH * rv + 0.5f;
                        const float uvx = fx - __builtin_floorf(fx), uvy = fy - __builtin_floorf(fy);
                        const int tx = f2i_trunc(fW * ru - 0.5f), ty = f2i_trunc(fH * rv - 0.5f);
                        const TexelHistory t00 = load_history(a, tx, ty, ru, rv, dxc), t10 = load_history(a, tx + 1, ty, ru, rv, dxc);
                        const TexelHistory t01 = load_history(a, tx, ty + 1, ru, rv, dxc), t11 = load_history(a, tx + 1, ty + 1, ru, rv, dxc);
                        float4 w;
                        w.x = disocclusion(normal, t00.n, ld, t00.ld, dxc) > 0.45f ? 1.0f : 0.0f;
                        w.y = disocclusion(normal, t10.n, ld, t10.ld, dxc) > 0.45f ? 1.0f : 0.0f;
                        w.z = disocclusion(normal, t01.n, ld, t01.ld, dxc) > 0.45f ? 1.0f : 0.0f;
                        w.w = disocclusion(normal, t11.n, ld, t11.ld, dxc) > 0.45f ? 1.0f : 0.0f;
                        w.x = (w.x * (1.0f - uvx)) * (1.0f - uvy);
                        w.y = (w.y * uvx) * (1.0f - uvy);
                        w.z = (w.z * (1.0f - uvx)) * uvy;
                        w.w = (w.w * uvx) * uvy;
                        const float ws = max2(((w.x + w.y) + w.z) + w.w, 1.0e-3f);
                        w = make_float4(fdiv_(w.x, ws), fdiv_(w.y, ws), fdiv_(w.z, ws), fdiv_(w.w, ws));
                        rep = mix4(t00.rad, t10.rad, t01.rad, t11.rad, w);
                        const float hld = ((t00.ld * w.x + t10.ld * w.y) + t01.ld * w.z) + t11.ld * w.w;
                        df = disocclusion(normal, mix4(t00.n, t10.n, t01.n, t11.n, w), ld, hld, dxc);            // the interpolated normal is not normalised
                    }
                    df = df < 0.9f ? 0.0f : df;
                }
                // FFX_DNSR_Reflections_Reproject :306-328
                if (ru > 0.0f && rv > 0.0f && ru < 1.0f && rv < 1.0f && !(df < 0.9f)) {
                    const float prevVar = sample_r16f(a.varianceHist, a.varianceHistPitch, rb);
                    float ns = sample_r16f(a.sampleCountHist, a.sampleCountHistPitch, rb) * df;
                    const float sMax = max2(8.0f, 32.0f * (1.0f - exp_((-roughness) * 100.0f)));
                    ns = min2(sMax, ns + 1.0f);
                    const float newVar = temporal_variance(rad, rep, dxc);                                         // (radiance, reprojection): the call site's order
                    stRep = rep; stVar = lerp_w(newVar, prevVar, fdiv_(1.0f, ns)); stCnt = ns;
                    rad = mk3(lerp_w(rad.x, rep.x, 0.3f), lerp_w(rad.y, rep.y, 0.3f), lerp_w(rad.z, rep.z, 0.3f));
                }
            }
            const float4 o = make_float4(stRep.x, stRep.y, stRep.z, 0.0f);                                        // the shader stores a float3: alpha is written as 0
            if (a.outF32) store_px<0>(a.outReprojected, (size_t)py * a.outReprojectedPitch + px, o); else store_px<1>(a.outReprojected, (size_t)py * a.outReprojectedPitch + px, o);
            ((_Float16*)a.outVariance)[(size_t)py * a.outVariancePitch + px] = to_f16(stVar);
            ((_Float16*)a.outSampleCount)[(size_t)py * a.outSampleCountPitch + px] = to_f16(stCnt);
        }
        // the 8 x 8 -> 1 average: radiance * weight and weight through binary16, three levels each summed in binary32 and stored through binary16 again
        float weight = max2(exp_((-luminance(rad, dxc)) * 0.3f), 1.0e-2f);
        rad = mul(rad, weight);
        if (!onScreen || not_finite(rad.x) || not_finite(rad.y) || not_finite(rad.z) || weight > 1.0e3f) { rad = mk3(0.0f, 0.0f, 0.0f); weight = 0.0f; }
        wave_sync();                                                                                              // every lane is done with the apron
        S[lane] = rh(rad.x); S[64 + lane] = rh(rad.y); S[128 + lane] = rh(rad.z); S[192 + lane] = rh(weight);
        wave_sync();
        #pragma unroll
        for (int i = 2; i <= 8; i *= 2) {
            const int ox = lx * i, oy = ly * i, ix = ox + i / 2, iy = oy + i / 2;
            if (ix < 8 && iy < 8) {                                                                               // (ox, oy) is read and written by this lane alone at this level
                #pragma unroll
                for (int ch = 0; ch < 4; ++ch) {
                    const float* P = S + 64 * ch;
                    const float sum = ((P[oy * 8 + ox] + P[oy * 8 + ix]) + P[iy * 8 + ox]) + P[iy * 8 + ix];
                    S[64 * ch + oy * 8 + ox] = rh(sum);
                }
            }
            wave_sync();
        }
        if (lane == 0u) {
            const float wacc = max2(S[192], 1.0e-3f);
            const float r = fdiv_(S[0], wacc), gch = fdiv_(S[64], wacc), b = fdiv_(S[128], wacc);
            const size_t t = (size_t)(y0 >> 3) * a.tilesX + (x0 >> 3);
            if (a.avgF32) ((float4*)a.outAverage)[t] = make_float4(r, gch, b, 0.0f);
            else ((uint32_t*)a.outAverage)[t] = to_small_float<6>(r) | (to_small_float<6>(gch) << 11) | (to_small_float<5>(b) << 22);
        }
        wave_sync();                                                                                              // the next tile overwrites the apron
    }
}

} // namespace

hipError_t launch_ssr_reproject(hipStream_t s, const SsrReprojectArgs& a, int nCUs) {
    static const int perCU = blocks_per_cu(k_ssr_reproject);
    return launch_tiles(s, k_ssr_reproject, perCU, a, nCUs);
}

} // namespace vqk
