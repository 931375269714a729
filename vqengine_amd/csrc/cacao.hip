// cacao.hip — FidelityFX CACAO at quality HIGH, native resolution, engine normals (vqhip_cacao; docs/DESIGN_DETAILS.md §7.14):
// AMDFidelityFX/CACAO/ffx_cacao.hlsl as FFX_CACAO_D3D12Draw dispatches it (ffx_cacao_impl.cpp:1922-2259), five kernels on the caller's stream:
//   k_cacao_prepare_depths   CSPrepareNativeDepthsAndMips            (:1331-1430)  one wave per 8 x 8 group of the half-resolution buffer
//   k_cacao_prepare_normals  CSPrepareNativeNormalsFromInputNormals  (:1619-1643)
//   k_cacao_generate         CSGenerateQ2, the four passes in one launch (blockIdx.z = pass, its own constants block)   (:803-1147)
//   k_cacao_blur             CSEdgeSensitiveBlur<p>, the four slices in one launch (blockIdx.z = slice)                  (:381-514)
//   k_cacao_apply            CSApply                                  (:1188-1242)
// The arithmetic is the source AS WRITTEN (§3.1 *_lit forms: every + - * rounded on its own — the bits rest on -ffp-contract=off —, IEEE quotients, correctly
// rounded sqrt, the contract's log2 / exp2), min16float = binary32, binary16 only in the R16F depth store and the blur's tile. No texture units: samplers are
// address arithmetic (§3.4). tests/cacao_ref.py states every stage in numpy; tests/test_gpu_cacao.py compares every plane bit for bit.
#include "vq_internal.h"
#include "vq_devmath.h"
#include "vq_sampling.h"

namespace vqk {
using namespace vqd;

namespace {

// ---- address arithmetic -------------------------------------------------------------------------------------------------------------------------
VQD int clampi(int i, int n) { return min(max(i, 0), n - 1); }
VQD int mirrori(int i, int n) {                                  // MIRROR: texel -1 reads 0, texel n reads n - 1, period 2n
    const int p = 2 * n;
    int t = i % p;
    if (t < 0) t += p;
    return t < n ? t : p - 1 - t;
}
VQD int gather_base(float u, int n) {                            // the first texel of GatherRed's footprint: the bilinear footprint in 8-bit fixed point
    int i; float w;
    fixed8(u * (float)n - 0.5f, &i, &w);
    return i;
}
VQD int point_texel(float u, int n) { return f2i_floor(u * (float)n); }

// ---- storage rules ------------------------------------------------------------------------------------------------------------------------------
VQD float unorm8f(uint32_t b) { return fdiv_((float)b, 255.0f); }
VQD int snorm8(float f) {                                        // FLOAT -> SNORM8 (D3D11.3 §3.2.3.4): NaN -> 0, clamp, scale by 127, +-0.5 by sign, truncate
    float c = (f == f) ? f : 0.0f;
    c = c < -1.0f ? -1.0f : (c > 1.0f ? 1.0f : c);
    float s = c * 127.0f;
    s = s + (s >= 0.0f ? 0.5f : -0.5f);
    return (int)s;
}
VQD f3 load_snorm8(const uint32_t* plane, size_t i) {            // SNORM8 -> float: v / 127, -128 reads -1
    const uint32_t q = plane[i];
    const int x = max((int)(int8_t)(q & 255u), -127), y = max((int)(int8_t)((q >> 8) & 255u), -127), z = max((int)(int8_t)((q >> 16) & 255u), -127);
    return mk3(fdiv_((float)x, 127.0f), fdiv_((float)y, 127.0f), fdiv_((float)z, 127.0f));
}
VQD float dot4_lit(float ax, float ay, float az, float aw, float bx, float by, float bz, float bw) { return ((ax * bx + ay * by) + az * bz) + aw * bw; }

// UnpackEdges (:173-183) / UnpackEdgesFloat16_4 (:351-361): e[0..3] = L R T B
VQD void unpack_edges(float packed, float invSharpness, float e[4]) {
    const uint32_t p = (uint32_t)f2i_trunc(packed * 255.5f);
    e[0] = saturate(fdiv_((float)((p >> 6) & 3u), 3.0f) + invSharpness);
    e[1] = saturate(fdiv_((float)((p >> 4) & 3u), 3.0f) + invSharpness);
    e[2] = saturate(fdiv_((float)((p >> 2) & 3u), 3.0f) + invSharpness);
    e[3] = saturate(fdiv_((float)(p & 3u), 3.0f) + invSharpness);
}
// PackEdges (:163-171)
VQD float pack_edges(const float e[4]) {
    const float a = __builtin_rintf(saturate(e[0]) * 3.05f), b = __builtin_rintf(saturate(e[1]) * 3.05f);
    const float c = __builtin_rintf(saturate(e[2]) * 3.05f), d = __builtin_rintf(saturate(e[3]) * 3.05f);
    return dot4_lit(a, b, c, d, (float)(64.0 / 255.0), (float)(16.0 / 255.0), (float)(4.0 / 255.0), (float)(1.0 / 255.0));
}

VQD size_t depth_slice(const CacaoArgs& a, int mip, int slice) { return a.offDepth[mip] + (size_t)slice * ((size_t)a.mw[mip] * a.mh[mip] * 2); }

// ---- stage 1 ------------------------------------------------------------------------------------------------------------------------------------
// MipSmartAverage (:1313-1320); `-1.0f / EffectRadius * EffectRadius` left to right
VQD float mip_smart_average(float x, float y, float z, float w, float falloff) {
    const float closest = min_(min_(x, y), min_(z, w));
    const float dx = x - closest, dy = y - closest, dz = z - closest, dw = w - closest;
    const float wx = saturate(dx * dx * falloff + 1.0f), wy = saturate(dy * dy * falloff + 1.0f);
    const float wz = saturate(dz * dz * falloff + 1.0f), ww = saturate(dw * dw * falloff + 1.0f);
    return fdiv_(dot4_lit(wx, wy, wz, ww, x, y, z, w), ((wx + wy) + wz) + ww);
}

__global__ __launch_bounds__(64) void k_cacao_prepare_depths(CacaoArgs a, float unpackMul, float unpackAdd, float invW, float invH, float effectRadius) {
    __shared__ float buf[4][8][8];                                // s_PrepareDepthsAndMipsBuffer[slice][x][y]
    const int gx = threadIdx.x, gy = threadIdx.y;
    const int tx = blockIdx.x * 8 + gx, ty = blockIdx.y * 8 + gy;
    // GatherRed(g_PointClampSampler, (2 tid + 0.5) * inverse dimensions): threads outside the buffer run too, on clamped texels
    const int ix = gather_base(((float)(2 * tx) + 0.5f) * invW, a.width), iy = gather_base(((float)(2 * ty) + 0.5f) * invH, a.height);
    const int x0 = clampi(ix, a.width), x1 = clampi(ix + 1, a.width), y0 = clampi(iy, a.height), y1 = clampi(iy + 1, a.height);
    const float* r0 = a.depth + (size_t)y0 * a.depthPitch;
    const float* r1 = a.depth + (size_t)y1 * a.depthPitch;
    float s[4];                                                   // slices 0..3 = samples .w .z .x .y = footprint texels (0,0) (1,0) (0,1) (1,1)
    s[0] = fdiv_(unpackMul, unpackAdd - r0[x0]);
    s[1] = fdiv_(unpackMul, unpackAdd - r0[x1]);
    s[2] = fdiv_(unpackMul, unpackAdd - r1[x0]);
    s[3] = fdiv_(unpackMul, unpackAdd - r1[x1]);
    const bool inside = (tx < a.hw) & (ty < a.hh);
    #pragma unroll
    for (int k = 0; k < 4; ++k) {
        buf[k][gx][gy] = s[k];
        if (inside) ((_Float16*)(a.work + depth_slice(a, 0, k)))[(size_t)ty * a.hw + tx] = to_f16(s[k]);
    }
    const int ox = gx & 1, oy = gy & 1, idx = 2 * oy + ox, bx = gx - ox, by = gy - oy;
    const float falloff = fdiv_(-1.0f, effectRadius) * effectRadius;
    __syncthreads();
    {
        const float avg = mip_smart_average(buf[idx][bx][by], buf[idx][bx][by + 1], buf[idx][bx + 1][by], buf[idx][bx + 1][by + 1], falloff);
        const int cx = tx >> 1, cy = ty >> 1;
        if ((cx < a.mw[1]) & (cy < a.mh[1])) ((_Float16*)(a.work + depth_slice(a, 1, idx)))[(size_t)cy * a.mw[1] + cx] = to_f16(avg);
        buf[idx][bx][by] = avg;
    }
    __syncthreads();
    if (((gx & 3) == ox) & ((gy & 3) == oy)) {
        const float avg = mip_smart_average(buf[idx][bx][by], buf[idx][bx][by + 2], buf[idx][bx + 2][by], buf[idx][bx + 2][by + 2], falloff);
        const int cx = tx >> 2, cy = ty >> 2;
        if ((cx < a.mw[2]) & (cy < a.mh[2])) ((_Float16*)(a.work + depth_slice(a, 2, idx)))[(size_t)cy * a.mw[2] + cx] = to_f16(avg);
        buf[idx][bx][by] = avg;
    }
    __syncthreads();
    // :1381 reads `depthArrayOffset.y % 8 == depthArrayOffset.y` (always true); the reading fixed in §7.14: the writer is the thread with bufferCoord == (0, 0)
    if (((gx & 7) == ox) & ((gy & 7) == oy)) {
        const float avg = mip_smart_average(buf[idx][bx][by], buf[idx][bx][by + 4], buf[idx][bx + 4][by], buf[idx][bx + 4][by + 4], falloff);
        const int cx = tx >> 3, cy = ty >> 3;
        if ((cx < a.mw[3]) & (cy < a.mh[3])) ((_Float16*)(a.work + depth_slice(a, 3, idx)))[(size_t)cy * a.mw[3] + cx] = to_f16(avg);
    }
}

// ---- stage 2 ------------------------------------------------------------------------------------------------------------------------------------
struct NormalConsts { float invW, invH, unpackMul, unpackAdd; float m[3][3]; };   // m: the block's floats as stored; the cbuffer reads them column-major

__global__ __launch_bounds__(64) void k_cacao_prepare_normals(CacaoArgs a, NormalConsts c) {
    const int tx = blockIdx.x * 8 + threadIdx.x, ty = blockIdx.y * 8 + threadIdx.y;
    if ((tx >= a.hw) | (ty >= a.hh)) return;
    #pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int px = 2 * tx + (s & 1), py = 2 * ty + (s >> 1);
        const int x = clampi(point_texel(((float)px + 0.5f) * c.invW, a.width), a.width), y = clampi(point_texel(((float)py + 0.5f) * c.invH, a.height), a.height);
        const size_t i = (size_t)y * a.normalPitch + x;
        f3 e;
        if (a.normF32) { const float4 v = ((const float4*)a.normals)[i]; e = mk3(v.x, v.y, v.z); }
        else { const uint32_t q = ((const uint32_t*)a.normals)[i];                              // UNORM10 -> float: c / 1023, correctly rounded
               e = mk3(fdiv_((float)(q & 1023u), 1023.0f), fdiv_((float)((q >> 10) & 1023u), 1023.0f), fdiv_((float)((q >> 20) & 1023u), 1023.0f)); }
        const f3 n = mk3(e.x * c.unpackMul + c.unpackAdd, e.y * c.unpackMul + c.unpackAdd, e.z * c.unpackMul + c.unpackAdd);
        uint32_t word = 127u << 24;
        #pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float v = (n.x * c.m[j][0] + n.y * c.m[j][1]) + n.z * c.m[j][2];
            word |= ((uint32_t)snorm8(v) & 255u) << (8 * j);
        }
        ((uint32_t*)(a.work + a.offNormals))[(size_t)s * a.hw * a.hh + (size_t)ty * a.hw + tx] = word;
    }
}

// ---- stage 3 ------------------------------------------------------------------------------------------------------------------------------------
// g_samplePatternMain[0 .. 32): (x, y, weight, log2(length)); HIGH takes the first 12, the adaptive base pass the first 5, the adaptive taps 5 .. 31
__device__ const float kSamplePattern[32][4] = {
    { 0.78488064f,  0.56661671f, 1.500000f, -0.126083f }, { 0.26022232f, -0.29575172f, 1.500000f, -1.064030f }, { 0.10459357f,  0.08372527f, 1.110000f, -2.730563f },
    {-0.68286800f,  0.04963045f, 1.090000f, -0.498827f }, {-0.13570161f, -0.64190155f, 1.250000f, -0.532765f }, {-0.26193795f, -0.08205118f, 0.670000f, -1.783245f },
    {-0.61177456f,  0.66664219f, 0.710000f, -0.044234f }, { 0.43675563f,  0.25119025f, 0.610000f, -1.167283f }, { 0.07884444f,  0.86618668f, 0.640000f, -0.459002f },
    {-0.12790935f, -0.29869005f, 0.600000f, -1.729424f }, {-0.04031125f,  0.02413622f, 0.600000f, -4.792042f }, { 0.16201244f, -0.52851415f, 0.790000f, -1.067055f },
    {-0.70991218f,  0.47301072f, 0.640000f, -0.335236f }, { 0.03277707f, -0.22349690f, 0.600000f, -1.982384f }, { 0.68921727f,  0.36800742f, 0.630000f, -0.266718f },
    { 0.29251814f,  0.37775412f, 0.610000f, -1.422520f }, {-0.12224089f,  0.96582592f, 0.600000f, -0.426142f }, { 0.11071457f, -0.16131058f, 0.600000f, -2.165947f },
    { 0.46562141f, -0.59747696f, 0.600000f, -0.189760f }, {-0.51548797f,  0.11804193f, 0.600000f, -1.246800f }, { 0.89141309f, -0.42090443f, 0.600000f,  0.028192f },
    {-0.32402530f, -0.01591529f, 0.600000f, -1.543018f }, { 0.60771245f,  0.41635221f, 0.600000f, -0.605411f }, { 0.02379565f, -0.08239821f, 0.600000f, -3.809046f },
    { 0.48951152f, -0.23657045f, 0.600000f, -1.189011f }, {-0.17611565f, -0.81696892f, 0.600000f, -0.513724f }, {-0.33930185f, -0.20732205f, 0.600000f, -1.698047f },
    {-0.91974425f,  0.05403209f, 0.600000f,  0.062246f }, {-0.15064627f, -0.14949332f, 0.600000f, -1.896062f }, { 0.53180975f, -0.35210401f, 0.600000f, -0.758838f },
    { 0.41487166f,  0.81442589f, 0.600000f, -0.505648f }, {-0.24106961f, -0.32721516f, 0.600000f, -1.665244f } };

// CalculatePixelObscurance (:623-631)
VQD float pixel_obscurance(f3 n, f3 d, float falloff, float horizon) {
    const float lengthSq = dot_lit(d, d);
    const float nDotD = fdiv_(dot_lit(n, d), sqrt_(lengthSq));
    const float falloffMult = max_(0.0f, lengthSq * falloff + 1.0f);
    return max_(0.0f, nDotD - horizon) * falloffMult;
}

struct CacaoPassConsts { VQ_CacaoConstants pass[4]; };

// SampleLevel(g_LinearClampSampler, uv, 0).x of an R8_UNORM plane (the importance map and its pong): §3.4, as sample_ao_bilinear below
VQD float sample_r8_bilinear(const uint8_t* plane, int w, int h, float u, float v) {
    int ix, iy; float wx, wy;
    fixed8(u * (float)w - 0.5f, &ix, &wx);
    fixed8(v * (float)h - 0.5f, &iy, &wy);
    const int x0 = clampi(ix, w), x1 = clampi(ix + 1, w), y0 = clampi(iy, h), y1 = clampi(iy + 1, h);
    const float c00 = unorm8f(plane[(size_t)y0 * w + x0]), c10 = unorm8f(plane[(size_t)y0 * w + x1]);
    const float c01 = unorm8f(plane[(size_t)y1 * w + x0]), c11 = unorm8f(plane[(size_t)y1 * w + x1]);
    const float w00 = (1.0f - wx) * (1.0f - wy), w10 = wx * (1.0f - wy), w01 = (1.0f - wx) * wy, w11 = wx * wy;
    return fma_(w11, c11, fma_(w01, c01, fma_(w10, c10, w00 * c00)));
}

// GenerateSSAOShadowsInternal (:803-1105) in its three uses. kGenHigh: (qualityLevel 2, adaptiveBase false), 12 taps through SSAOTap. kGenBase: (3, true), the first
// 5 of those taps and nothing else — no edges, no detail AO —, the result kept as (obscurance, weight / 20) in PONG. kGenAdaptive: (3, false), HIGH's front end, then the
// base values and 1 .. 27 more taps through SSAOGetSampleData / SSAOGetHits2 / SSAOAddHits, then HIGH's back end. Each is a kernel of its own: the branches are
// compile-time, so HIGH's instantiation is the code it was.
enum { kGenHigh = 0, kGenBase = 1, kGenAdaptive = 2 };
constexpr int kAdaptiveBaseTaps = 5, kAdaptiveMaxTaps = 32;          // SSAO_ADAPTIVE_TAP_BASE_COUNT, SSAO_MAX_TAPS

template <int MODE>
VQD void cacao_generate(const CacaoArgs& a, const CacaoPassConsts& all, const CacaoAdaptiveArgs& ad) {
    const int p = blockIdx.z;
    const VQ_CacaoConstants& c = all.pass[p];
    const int x = blockIdx.x * 8 + threadIdx.x, y = blockIdx.y * 8 + threadIdx.y;
    if ((x >= a.hw) | (y >= a.hh)) return;
    const int hw = a.hw, hh = a.hh;
    const _Float16* d0 = (const _Float16*)(a.work + depth_slice(a, 0, p));
    const uint32_t* nrm = (const uint32_t*)(a.work + a.offNormals) + (size_t)p * hw * hh;
    const float sx = (float)x, sy = (float)y;
    const float invDx = c.DeinterleavedDepthBufferInverseDimensions[0], invDy = c.DeinterleavedDepthBufferInverseDimensions[1];
    const float invSx = c.SSAOBufferInverseDimensions[0], invSy = c.SSAOBufferInverseDimensions[1];
    const float uvx = (sx + 0.5f) * invDx + c.DeinterleavedDepthBufferNormalisedOffset[0], uvy = (sy + 0.5f) * invDy + c.DeinterleavedDepthBufferNormalisedOffset[1];
    // the two GatherRed(g_PointMirrorSampler): footprint base g, the UL gather moved by (-1, -1)
    const int gx = gather_base(uvx, hw), gy = gather_base(uvy, hh);
    const int mx0 = mirrori(gx, hw), mxl = mirrori(gx - 1, hw), mxr = mirrori(gx + 1, hw), my0 = mirrori(gy, hh), myt = mirrori(gy - 1, hh), myb = mirrori(gy + 1, hh);
    const float pixZ = (float)d0[(size_t)my0 * hw + mx0];
    float pixL = pixZ, pixR = pixZ, pixT = pixZ, pixB = pixZ;
    if (MODE != kGenBase) {
        pixL = (float)d0[(size_t)my0 * hw + mxl]; pixR = (float)d0[(size_t)my0 * hw + mxr];
        pixT = (float)d0[(size_t)myt * hw + mx0]; pixB = (float)d0[(size_t)myb * hw + mx0];
    }
    const float nspx = (sx + 0.5f) * invSx, nspy = (sy + 0.5f) * invSy;
    f3 pc = mk3((c.NDCToViewMul[0] * nspx + c.NDCToViewAdd[0]) * pixZ, (c.NDCToViewMul[1] * nspy + c.NDCToViewAdd[1]) * pixZ, pixZ);
    const f3 n = load_snorm8(nrm, (size_t)y * hw + x);
    const float dirX = pc.z * c.NDCToViewMul[0] * invSx, dirY = pc.z * c.NDCToViewMul[1] * invSy;
    // CalculateRadiusParameters (:588-605)
    const float tooClose = saturate(length_lit(pc) * c.EffectSamplingRadiusNearLimitRec) * 0.8f + 0.2f;
    const float radius = c.EffectRadius * tooClose;
    const float lookup = fdiv_(0.85f * radius, dirX);
    const float falloff = fdiv_(-1.0f, radius * radius);
    const uint32_t rnd = (uint32_t)f2i_trunc(sy * 2.0f + sx) % 5u;
    const float r0 = c.PatternRotScaleMatrices[rnd][0] * lookup, r1 = c.PatternRotScaleMatrices[rnd][1] * lookup;
    const float r2 = c.PatternRotScaleMatrices[rnd][2] * lookup, r3 = c.PatternRotScaleMatrices[rnd][3] * lookup;
    pc = mk3(pc.x * c.DepthPrecisionOffsetMod, pc.y * c.DepthPrecisionOffsetMod, pc.z * c.DepthPrecisionOffsetMod);
    float e[4] = { 1.0f, 1.0f, 1.0f, 1.0f };
    float obsSum = 0.0f, weightSum = 0.0f;
    if (MODE != kGenBase) {
        // CalculateEdges (:213-219)
        {
            const float el = pixL - pixZ, er = pixR - pixZ, et = pixT - pixZ, eb = pixB - pixZ;
            const float al = el + er, ar = er + el, at = et + eb, ab = eb + et;
            const float den = pixZ * 0.040f;
            e[0] = saturate(1.3f - fdiv_(min_(abs_(el), abs_(al)), den));
            e[1] = saturate(1.3f - fdiv_(min_(abs_(er), abs_(ar)), den));
            e[2] = saturate(1.3f - fdiv_(min_(abs_(et), abs_(at)), den));
            e[3] = saturate(1.3f - fdiv_(min_(abs_(eb), abs_(ab)), den));
        }
        // detail AO (:877-905)
        {
            const f3 vdz = mk3(fdiv_(pc.x, pc.z), fdiv_(pc.y, pc.z), 1.0f);
            const float dl = pixL - pc.z, dr = pixR - pc.z, dt = pixT - pc.z, db = pixB - pc.z;
            const f3 dL = mk3(-dirX + vdz.x * dl, 0.0f + vdz.y * dl, 0.0f + vdz.z * dl);
            const f3 dR = mk3(dirX + vdz.x * dr, 0.0f + vdz.y * dr, 0.0f + vdz.z * dr);
            const f3 dT = mk3(0.0f + vdz.x * dt, -dirY + vdz.y * dt, 0.0f + vdz.z * dt);
            const f3 dB = mk3(0.0f + vdz.x * db, dirY + vdz.y * db, 0.0f + vdz.z * db);
            const float mf = 4.0f * falloff, hz = c.EffectHorizonAngleThreshold;
            obsSum = 0.0f + c.DetailAOStrength * dot4_lit(pixel_obscurance(n, dL, mf, hz), pixel_obscurance(n, dR, mf, hz), pixel_obscurance(n, dT, mf, hz),
                                                           pixel_obscurance(n, dB, mf, hz), e[0], e[1], e[2], e[3]);
        }
        // normal-based edges (:908-935): a Load outside the slice returns 0
        {
            const f3 zero = mk3(0.0f, 0.0f, 0.0f);
            const f3 nl = x > 0 ? load_snorm8(nrm, (size_t)y * hw + x - 1) : zero, nr = x + 1 < hw ? load_snorm8(nrm, (size_t)y * hw + x + 1) : zero;
            const f3 nt = y > 0 ? load_snorm8(nrm, (size_t)(y - 1) * hw + x) : zero, nb = y + 1 < hh ? load_snorm8(nrm, (size_t)(y + 1) * hw + x) : zero;
            e[0] = e[0] * saturate(dot_lit(n, nl) + 0.5f);
            e[1] = e[1] * saturate(dot_lit(n, nr) + 0.5f);
            e[2] = e[2] * saturate(dot_lit(n, nt) + 0.5f);
            e[3] = e[3] * saturate(dot_lit(n, nb) + 0.5f);
        }
    }
    const float mipOffset = log2_(lookup) + (-4.3f);
    const float hz = c.EffectHorizonAngleThreshold;
    if (MODE != kGenAdaptive) {
        constexpr int taps = MODE == kGenBase ? kAdaptiveBaseTaps : 12;             // SSAOTap (:658-698), g_numTaps[2]
        for (int i = 0; i < taps; ++i) {
            const float spx = kSamplePattern[i][0], spy = kSamplePattern[i][1];
            const float ox = __builtin_rintf(r0 * spx + r1 * spy), oy = __builtin_rintf(r2 * spx + r3 * spy);
            const float lod = kSamplePattern[i][3] + mipOffset;
            const int level = min(max(f2i_floor(lod + 0.5f), 0), 3);                  // the point mip filter; NaN -> 0
            const float weightMod = 1.0f * kSamplePattern[i][2];
            const int mw = a.mw[level], mh = a.mh[level];
            const _Float16* dm = (const _Float16*)(a.work + depth_slice(a, level, p));
            #pragma unroll
            for (int t = 0; t < 2; ++t) {
                const float tx = (t ? -ox : ox) * invDx + uvx, ty = (t ? -oy : oy) * invDy + uvy;
                const float z = (float)dm[(size_t)clampi(point_texel(ty, mh), mh) * mw + clampi(point_texel(tx, mw), mw)];
                const f3 hit = mk3((c.DepthBufferUVToViewMul[0] * tx + c.DepthBufferUVToViewAdd[0]) * z, (c.DepthBufferUVToViewMul[1] * ty + c.DepthBufferUVToViewAdd[1]) * z, z);
                const f3 delta = sub(hit, pc);
                const float obs = pixel_obscurance(n, delta, falloff, hz);
                const float reduct = saturate(max_(0.0f, -delta.z) * c.NegRecEffectRadius + 2.0f);
                const float weight = (0.6f * reduct + 0.4f) * weightMod;                 // (1.0 - 0.6) folds to the binary32 nearest 0.4
                obsSum = obsSum + obs * weight;
                weightSum = weightSum + weight;
            }
        }
    } else {
        // the adaptive branch (:995-1048)
        const uint8_t* imp = a.work + ad.offImportance;
        float importance = sample_r8_bilinear(imp, ad.iw, ad.ih, nspx + c.PerPassFullResUVOffset[0], nspy + c.PerPassFullResUVOffset[1]);
        obsSum = obsSum * (0.15625f + fdiv_(importance * 27.0f, 32.0f));              // 5 / (float)32 + importance * 27 / (float)32, left to right
        const uint32_t base = ((const uint16_t*)(a.work + a.offPong))[(size_t)p * hw * hh + (size_t)y * hw + x];
        weightSum = weightSum + unorm8f(base >> 8) * 20.0f;                            // (float)(5 * 4.0)
        obsSum = obsSum + unorm8f(base & 255u) * weightSum;
        const float avgImportance = (float)*(const uint32_t*)(a.work + ad.offCounter) * c.LoadCounterAvgDiv;
        importance = importance * saturate(fdiv_(c.AdaptiveSampleCountLimit, avgImportance));   // x / 0 = +inf -> 1; 0 / 0 = NaN -> 0
        const int to = min(kAdaptiveMaxTaps, f2i_trunc(27.0f * importance + 1.5f) + kAdaptiveBaseTaps);
        // The source's software pipeline: tap i + 1's two depths are fetched before tap i's arithmetic. The trip count is per lane (1 .. 27 taps); the loop
        // stays rolled and the wave runs to its longest lane. g_samplePatternMain[i + 2] (:1033) is read one tap ahead of its use, at index 32 for nothing:
        // the pattern is read here where it is used.
        struct Tap { float u0, v0, z0, u1, v1, z1; };
        auto fetch = [&](int i) {                                                       // SSAOGetSampleData (:742-757) + SSAOGetHits2 (:759-768)
            const float spx = kSamplePattern[i][0], spy = kSamplePattern[i][1];
            const float ox = __builtin_rintf(r0 * spx + r1 * spy) * invDx, oy = __builtin_rintf(r2 * spx + r3 * spy) * invDy;
            const float lod = kSamplePattern[i][3] + mipOffset;
            const int level = min(max(f2i_floor(lod + 0.5f), 0), 3);
            const int mw = a.mw[level], mh = a.mh[level];
            const _Float16* dm = (const _Float16*)(a.work + depth_slice(a, level, p));
            Tap t;
            t.u0 = uvx + ox; t.v0 = uvy + oy;
            t.z0 = (float)dm[(size_t)clampi(point_texel(t.v0, mh), mh) * mw + clampi(point_texel(t.u0, mw), mw)];
            t.u1 = uvx - ox; t.v1 = uvy - oy;
            t.z1 = (float)dm[(size_t)clampi(point_texel(t.v1, mh), mh) * mw + clampi(point_texel(t.u1, mw), mw)];
            return t;
        };
        auto add = [&](float u, float v, float z) {                                     // SSAOAddHits (:770-792): the weight is overwritten per hit, weightMod never enters
            const f3 hit = mk3((c.DepthBufferUVToViewMul[0] * u + c.DepthBufferUVToViewAdd[0]) * z, (c.DepthBufferUVToViewMul[1] * v + c.DepthBufferUVToViewAdd[1]) * z, z);
            const f3 delta = sub(hit, pc);
            const float obs = pixel_obscurance(n, delta, falloff, hz);
            const float reduct = saturate(max_(0.0f, -delta.z) * c.NegRecEffectRadius + 2.0f);
            const float weight = 0.6f * reduct + 0.4f;
            obsSum = obsSum + obs * weight;
            weightSum = weightSum + weight;
        };
        Tap hits = fetch(kAdaptiveBaseTaps);
        #pragma clang loop unroll(disable)
        for (int i = kAdaptiveBaseTaps; i < to - 1; ++i) {
            const Tap next = fetch(i + 1);
            add(hits.u0, hits.v0, hits.z0);
            add(hits.u1, hits.v1, hits.z1);
            hits = next;
        }
        add(hits.u0, hits.v0, hits.z0);
        add(hits.u1, hits.v1, hits.z1);
    }
    float obscurance = fdiv_(obsSum, weightSum);
    if (MODE == kGenBase) {                                                             // CSGenerateQ3Base (:1150-1161): R8G8_UNORM, the store saturates
        uint8_t* out = a.work + a.offPong + ((size_t)p * hw * hh + (size_t)y * hw + x) * 2;
        *(uint16_t*)out = (uint16_t)(unorm8(obscurance) | (unorm8(fdiv_(weightSum, 20.0f)) << 8));
        return;
    }
    float fade = saturate(pc.z * c.EffectFadeOutMul + c.EffectFadeOutAdd);
    const float edgeFade = saturate((1.0f - e[0] - e[1]) * 0.35f) + saturate((1.0f - e[2] - e[3]) * 0.35f);
    fade = fade * saturate(1.0f - edgeFade);
    obscurance = min_(c.EffectShadowStrength * obscurance, c.EffectShadowClamp) * fade;
    const float occlusion = pow_(saturate(1.0f - obscurance), c.EffectShadowPow);
    uint8_t* out = a.work + a.offPing + ((size_t)p * hw * hh + (size_t)y * hw + x) * 2;
    *(uint16_t*)out = (uint16_t)(unorm8(occlusion) | (unorm8(pack_edges(e)) << 8));
}

__global__ __launch_bounds__(64) void k_cacao_generate(CacaoArgs a, CacaoPassConsts all) { cacao_generate<kGenHigh>(a, all, CacaoAdaptiveArgs{}); }
__global__ __launch_bounds__(64) void k_cacao_generate_base(CacaoArgs a, CacaoPassConsts all) { cacao_generate<kGenBase>(a, all, CacaoAdaptiveArgs{}); }
__global__ __launch_bounds__(64) void k_cacao_generate_adaptive(CacaoArgs a, CacaoPassConsts all, CacaoAdaptiveArgs ad) { cacao_generate<kGenAdaptive>(a, all, ad); }

// ---- the importance map (:1645-1747): R8_UNORM at quarter resolution, 8 x 8 groups over iw x ih ---------------------------------------------------------------
struct ImportanceConsts { float invSx, invSy, strength, shadowPow, invIx, invIy; };

// CSGenerateImportanceMap (:1651-1682). `avg` (:1658, :1673) feeds nothing. Threads outside the map would only have their store dropped. Lane 0 of group (0, 0)
// clears the load counter: stream order puts this store two launches before CSPostprocessImportanceMapB's adds.
__global__ __launch_bounds__(64) void k_cacao_importance(CacaoArgs a, CacaoAdaptiveArgs ad, ImportanceConsts k) {
    const int tx = blockIdx.x * 8 + threadIdx.x, ty = blockIdx.y * 8 + threadIdx.y;
    if ((blockIdx.x | blockIdx.y | threadIdx.x | threadIdx.y) == 0) *(uint32_t*)(a.work + ad.offCounter) = 0u;
    if ((tx >= ad.iw) | (ty >= ad.ih)) return;
    const int hw = a.hw, hh = a.hh;
    const int ix = gather_base(((float)(2 * tx) + 0.5f) * k.invSx, hw), iy = gather_base(((float)(2 * ty) + 0.5f) * k.invSy, hh);
    const int x0 = clampi(ix, hw), x1 = clampi(ix + 1, hw), y0 = clampi(iy, hh), y1 = clampi(iy + 1, hh);
    float minV = 1.0f, maxV = 0.0f;
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint16_t* base = (const uint16_t*)(a.work + a.offPong) + (size_t)i * hw * hh;
        float v[4] = { unorm8f(base[(size_t)y1 * hw + x0] & 255u), unorm8f(base[(size_t)y1 * hw + x1] & 255u),     // GatherRed .x .y .z .w
                       unorm8f(base[(size_t)y0 * hw + x1] & 255u), unorm8f(base[(size_t)y0 * hw + x0] & 255u) };
        #pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = pow_(saturate(1.0f - k.strength * v[j]), k.shadowPow);
        maxV = max_(maxV, max_(max_(v[0], v[1]), max_(v[2], v[3])));
        minV = min_(minV, min_(min_(v[0], v[1]), min_(v[2], v[3])));
    }
    (a.work + ad.offImportance)[(size_t)ty * ad.iw + tx] = (uint8_t)unorm8(pow_(saturate((maxV - minV) * 2.0f), 0.8f));
}

// CSPostprocessImportanceMapA (:1689-1710) and B (:1716-1747): the centre and four bilinear taps at +-1/2 and +-3/2 texels, B with the mirrored pattern;
// lerp(maxVal, avgVal, cSmoothenImportance = 1.0) is the contract's a + t * (b - a), which is not avgVal. B has no bounds test in the source: the threads of
// its last groups that lie outside the map sample clamped texels, lose their store, and still add to the load counter when tid.x % 3 + tid.y % 3 == 0 (§7.15).
template <bool B>
VQD float importance_postprocess(const uint8_t* in, int iw, int ih, int tx, int ty, float invIx, float invIy) {
    const float u = ((float)tx + 0.5f) * invIx, v = ((float)ty + 0.5f) * invIy;
    const float centre = sample_r8_bilinear(in, iw, ih, u, v);
    const float hx = 0.5f * invIx, hy = 0.5f * invIy;
    float s[4];
    if (!B) {
        s[0] = sample_r8_bilinear(in, iw, ih, u + -hx * 3.0f, v + -hy);
        s[1] = sample_r8_bilinear(in, iw, ih, u + hx, v + -hy * 3.0f);
        s[2] = sample_r8_bilinear(in, iw, ih, u + hx * 3.0f, v + hy);
        s[3] = sample_r8_bilinear(in, iw, ih, u + -hx, v + hy * 3.0f);
    } else {
        s[0] = sample_r8_bilinear(in, iw, ih, u + -hx, v + -hy * 3.0f);
        s[1] = sample_r8_bilinear(in, iw, ih, u + hx * 3.0f, v + -hy);
        s[2] = sample_r8_bilinear(in, iw, ih, u + hx, v + hy * 3.0f);
        s[3] = sample_r8_bilinear(in, iw, ih, u + -hx * 3.0f, v + hy);
    }
    const float avgVal = dot4_lit(s[0], s[1], s[2], s[3], 0.25f, 0.25f, 0.25f, 0.25f);
    const float maxVal = max_(centre, max_(max_(s[0], s[2]), max_(s[1], s[3])));
    return lerp_lit(maxVal, avgVal, 1.0f);
}

__global__ __launch_bounds__(64) void k_cacao_importance_a(CacaoArgs a, CacaoAdaptiveArgs ad, ImportanceConsts k) {
    const int tx = blockIdx.x * 8 + threadIdx.x, ty = blockIdx.y * 8 + threadIdx.y;
    if ((tx >= ad.iw) | (ty >= ad.ih)) return;
    const float r = importance_postprocess<false>(a.work + ad.offImportance, ad.iw, ad.ih, tx, ty, k.invIx, k.invIy);
    (a.work + ad.offImportancePong)[(size_t)ty * ad.iw + tx] = (uint8_t)unorm8(r);
}

// B's threads are the source's — ceil(iw / 8) x ceil(ih / 8) groups of 8 x 8 —, carried by groups of 16 x 16 (four waves) so that one atomic serves four of the source's
// groups: every wave's atomic lands on the one counter, and with one per 8 x 8 group they were nine tenths of this kernel's time (profiles/r13a_cacao_adaptive.md).
// The sum is an integer: neither the grouping nor the order of the adds changes it.
__global__ __launch_bounds__(256) void k_cacao_importance_b(CacaoArgs a, CacaoAdaptiveArgs ad, ImportanceConsts k) {
    __shared__ uint32_t waveSum[4];
    const int tx = blockIdx.x * 16 + threadIdx.x, ty = blockIdx.y * 16 + threadIdx.y;
    const bool runs = (tx < (ad.iw + 7) / 8 * 8) & (ty < (ad.ih + 7) / 8 * 8);               // a thread of the source's dispatch
    const float r = importance_postprocess<true>(a.work + ad.offImportancePong, ad.iw, ad.ih, tx, ty, k.invIx, k.invIy);
    if ((tx < ad.iw) & (ty < ad.ih)) (a.work + ad.offImportance)[(size_t)ty * ad.iw + tx] = (uint8_t)unorm8(r);
    uint32_t sum = (runs & (tx % 3 + ty % 3 == 0)) ? (uint32_t)f2i_trunc(saturate(r) * 255.0f + 0.5f) : 0u;
    #pragma unroll
    for (int m = 32; m > 0; m >>= 1) sum += (uint32_t)__shfl_xor((int)sum, m, 64);            // the wave's 64 contributions
    const int lane = threadIdx.y * 16 + threadIdx.x;
    if ((lane & 63) == 0) waveSum[lane >> 6] = sum;
    __syncthreads();
    if (lane == 0) {
        const uint32_t total = (waveSum[0] + waveSum[1]) + (waveSum[2] + waveSum[3]);
        if (total) atomicAdd((uint32_t*)(a.work + ad.offCounter), total);                      // adding 0 changes nothing: flat regions stay off the counter
    }
}

// ---- stage 4 ------------------------------------------------------------------------------------------------------------------------------------
// LDSEdgeSensitiveBlur (:381-514): 16 x 16 threads, each owning 4 x 3 texels of a 64 x 48 tile kept as binary16 in group-shared memory (two copies, a one-texel
// border the source never writes: it only reaches texels that are not stored, and reads 0 here). Rows are padded to 68 halves.
constexpr int kBlurW = 64, kBlurH = 48, kBlurRow = 68;

struct BlurConsts { float invW[4], invH[4], invSharpness[4]; };        // each slice is blurred with its own pass's constants block

__global__ __launch_bounds__(256) void k_cacao_blur(CacaoArgs a, BlurConsts bc) {
    __shared__ _Float16 tile[2][kBlurH + 2][kBlurRow];
    const int p = a.blurPasses, slice = blockIdx.z;
    const float invW = bc.invW[slice], invH = bc.invH[slice], invSharpness = bc.invSharpness[slice];
    const int hw = a.hw, hh = a.hh;
    const int lx = 4 * threadIdx.x, ly = 3 * threadIdx.y;                          // the thread's texels inside the tile
    const int ox = (int)blockIdx.x * (kBlurW - 2 * p) - p + lx, oy = (int)blockIdx.y * (kBlurH - 2 * p) - p + ly;   // imageCoord
    const uint16_t* src = (const uint16_t*)(a.work + a.offPing) + (size_t)slice * hw * hh;
    uint16_t* dst = (uint16_t*)(a.work + a.offPong) + (size_t)slice * hw * hh;
    for (int i = threadIdx.y * 16 + threadIdx.x; i < 2 * (kBlurH + 2) * kBlurRow; i += 256) (&tile[0][0][0])[i] = (_Float16)0.0f;
    __syncthreads();
    float e[3][4][4];
    uint8_t eb[3][4];
    #pragma unroll
    for (int y = 0; y < 3; ++y) {
        const int ty = mirrori(point_texel(((float)(oy + y) + 0.5f) * invH, hh), hh);
        #pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int tx = mirrori(point_texel(((float)(ox + x) + 0.5f) * invW, hw), hw);
            const uint32_t v = src[(size_t)ty * hw + tx];
            tile[0][ly + y + 1][lx + x + 1] = to_f16(unorm8f(v & 255u));
            eb[y][x] = (uint8_t)(v >> 8);
            unpack_edges(unorm8f(v >> 8), invSharpness, e[y][x]);
        }
    }
    __syncthreads();
    for (int it = 0; it < p; ++it) {
        const int s = it & 1, d = s ^ 1;
        #pragma unroll
        for (int y = 0; y < 3; ++y) {
            #pragma unroll
            for (int x = 0; x < 4; ++x) {
                const int cy = ly + y + 1, cx = lx + x + 1;
                float sum = (float)tile[s][cy][cx] * 0.5f, weight = 0.5f;
                sum = sum + (float)tile[s][cy][cx - 1] * e[y][x][0]; weight = weight + e[y][x][0];
                sum = sum + (float)tile[s][cy][cx + 1] * e[y][x][1]; weight = weight + e[y][x][1];
                sum = sum + (float)tile[s][cy - 1][cx] * e[y][x][2]; weight = weight + e[y][x][2];
                sum = sum + (float)tile[s][cy + 1][cx] * e[y][x][3]; weight = weight + e[y][x][3];
                tile[d][cy][cx] = to_f16(fdiv_(sum, weight));
            }
        }
        __syncthreads();
    }
    const int r = p & 1;
    #pragma unroll
    for (int y = 0; y < 3; ++y) {
        #pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int tx = lx + x, ty = ly + y, gx = ox + x, gy = oy + y;
            if ((tx >= p) & (tx < kBlurW - p) & (ty >= p) & (ty < kBlurH - p) & (gx >= 0) & (gx < hw) & (gy >= 0) & (gy < hh))
                dst[(size_t)gy * hw + gx] = (uint16_t)(unorm8((float)tile[r][ty + 1][tx + 1]) | ((uint32_t)eb[y][x] << 8));   // the edge byte survives its own UNORM8 round trip
        }
    }
}

// ---- stage 5 ------------------------------------------------------------------------------------------------------------------------------------
VQD float sample_ao_bilinear(const uint16_t* plane, int hw, int hh, float u, float v) {   // SampleLevel(g_LinearClampSampler, uv, 0).x: §3.4
    int ix, iy; float wx, wy;
    fixed8(u * (float)hw - 0.5f, &ix, &wx);
    fixed8(v * (float)hh - 0.5f, &iy, &wy);
    const int x0 = clampi(ix, hw), x1 = clampi(ix + 1, hw), y0 = clampi(iy, hh), y1 = clampi(iy + 1, hh);
    const float c00 = unorm8f(plane[(size_t)y0 * hw + x0] & 255u), c10 = unorm8f(plane[(size_t)y0 * hw + x1] & 255u);
    const float c01 = unorm8f(plane[(size_t)y1 * hw + x0] & 255u), c11 = unorm8f(plane[(size_t)y1 * hw + x1] & 255u);
    const float w00 = (1.0f - wx) * (1.0f - wy), w10 = wx * (1.0f - wy), w01 = (1.0f - wx) * wy, w11 = wx * wy;
    return fma_(w11, c11, fma_(w01, c01, fma_(w10, c10, w00 * c00)));
}

__global__ __launch_bounds__(64) void k_cacao_apply(CacaoArgs a, float invW, float invH, float invSharpness) {
    const int x = blockIdx.x * 8 + threadIdx.x, y = blockIdx.y * 8 + threadIdx.y;
    if ((x >= a.width) | (y >= a.height)) return;
    const int hw = a.hw, hh = a.hh;
    const size_t sliceTexels = (size_t)hw * hh;
    const uint16_t* fin = (const uint16_t*)(a.work + (a.blurPasses ? a.offPong : a.offPing));
    const int mx = x & 1, my = y & 1;
    const int ic = mx + my * 2, ih = (1 - mx) + my * 2, iv = mx + (1 - my) * 2, id = (1 - mx) + (1 - my) * 2;
    const uint32_t centre = fin[ic * sliceTexels + (size_t)(y >> 1) * hw + (x >> 1)];
    float ao = unorm8f(centre & 255u);
    float e[4];
    unpack_edges(unorm8f(centre >> 8), invSharpness, e);
    const float fx = (float)x, fy = (float)y, fmx = (float)mx, fmy = (float)my;
    const float fmxe = e[1] - e[0], fmye = e[3] - e[2];
    const float aoH = sample_ao_bilinear(fin + ih * sliceTexels, hw, hh, (fx + (fmx + fmxe - 0.5f)) * 0.5f * invW, (fy + (0.5f - fmy)) * 0.5f * invH);
    const float aoV = sample_ao_bilinear(fin + iv * sliceTexels, hw, hh, (fx + (0.5f - fmx)) * 0.5f * invW, (fy + (fmy - 0.5f + fmye)) * 0.5f * invH);
    const float aoD = sample_ao_bilinear(fin + id * sliceTexels, hw, hh, (fx + (fmx - 0.5f + fmxe)) * 0.5f * invW, (fy + (fmy - 0.5f + fmye)) * 0.5f * invH);
    const float bw1 = (e[0] + e[1]) * 0.5f, bw2 = (e[2] + e[3]) * 0.5f, bw3 = (bw1 + bw2) * 0.5f;
    const float total = ((1.0f + bw1) + bw2) + bw3;
    ao = fdiv_(dot4_lit(ao, aoH, aoV, aoD, 1.0f, bw1, bw2, bw3), total);
    a.ao[(size_t)y * a.aoPitch + x] = (uint8_t)unorm8(ao);
}

void launch_prepare(hipStream_t s, const CacaoArgs& a, const VQ_CacaoConstants& shared, dim3 halfGrid) {
    const dim3 wave(8, 8);
    k_cacao_prepare_depths<<<halfGrid, wave, 0, s>>>(a, shared.DepthUnpackConsts[0], shared.DepthUnpackConsts[1], shared.DepthBufferInverseDimensions[0],
                                                      shared.DepthBufferInverseDimensions[1], shared.EffectRadius);
    NormalConsts nc;
    nc.invW = shared.InputOutputBufferInverseDimensions[0]; nc.invH = shared.InputOutputBufferInverseDimensions[1];
    nc.unpackMul = shared.NormalsUnpackMul; nc.unpackAdd = shared.NormalsUnpackAdd;
    for (int j = 0; j < 3; ++j) for (int i = 0; i < 3; ++i) nc.m[j][i] = shared.NormalsWorldToViewspaceMatrix.m[j][i];
    k_cacao_prepare_normals<<<halfGrid, wave, 0, s>>>(a, nc);
}
void launch_blur_apply(hipStream_t s, const CacaoArgs& a, const VQ_CacaoConstants& shared, const VQ_CacaoConstants perPass[4]) {
    if (a.blurPasses) {
        const int sw = kBlurW - 2 * a.blurPasses, sh = kBlurH - 2 * a.blurPasses;
        BlurConsts bc;
        for (int i = 0; i < 4; ++i) { bc.invW[i] = perPass[i].SSAOBufferInverseDimensions[0]; bc.invH[i] = perPass[i].SSAOBufferInverseDimensions[1]; bc.invSharpness[i] = perPass[i].InvSharpness; }
        k_cacao_blur<<<dim3((a.hw + sw - 1) / sw, (a.hh + sh - 1) / sh, 4), dim3(16, 16), 0, s>>>(a, bc);
    }
    k_cacao_apply<<<dim3((a.width + 7) / 8, (a.height + 7) / 8), dim3(8, 8), 0, s>>>(a, shared.SSAOBufferInverseDimensions[0], shared.SSAOBufferInverseDimensions[1],
                                                                                    shared.InvSharpness);
}
} // namespace

hipError_t launch_cacao(hipStream_t s, const CacaoArgs& a, const VQ_CacaoConstants& shared, const VQ_CacaoConstants perPass[4]) {
    const dim3 wave(8, 8);
    const dim3 halfGrid((a.hw + 7) / 8, (a.hh + 7) / 8);
    launch_prepare(s, a, shared, halfGrid);
    CacaoPassConsts all;
    for (int i = 0; i < 4; ++i) all.pass[i] = perPass[i];
    k_cacao_generate<<<dim3(halfGrid.x, halfGrid.y, 4), wave, 0, s>>>(a, all);
    launch_blur_apply(s, a, shared, perPass);
    return hipGetLastError();
}

// Quality HIGHEST (FFX_CACAO_D3D12Draw's adaptive branch, ffx_cacao_impl.cpp:1950-2150): ten launches, or nine when the blur is skipped
hipError_t launch_cacao_adaptive(hipStream_t s, const CacaoArgs& a, const CacaoAdaptiveArgs& ad, const VQ_CacaoConstants& shared, const VQ_CacaoConstants perPass[4]) {
    const dim3 wave(8, 8);
    const dim3 halfGrid((a.hw + 7) / 8, (a.hh + 7) / 8), mapGrid((ad.iw + 7) / 8, (ad.ih + 7) / 8);
    launch_prepare(s, a, shared, halfGrid);
    CacaoPassConsts all;
    for (int i = 0; i < 4; ++i) all.pass[i] = perPass[i];
    k_cacao_generate_base<<<dim3(halfGrid.x, halfGrid.y, 4), wave, 0, s>>>(a, all);
    const ImportanceConsts k = { shared.SSAOBufferInverseDimensions[0], shared.SSAOBufferInverseDimensions[1], shared.EffectShadowStrength, shared.EffectShadowPow,
                                 shared.ImportanceMapInverseDimensions[0], shared.ImportanceMapInverseDimensions[1] };
    k_cacao_importance<<<mapGrid, wave, 0, s>>>(a, ad, k);
    k_cacao_importance_a<<<mapGrid, wave, 0, s>>>(a, ad, k);
    k_cacao_importance_b<<<dim3((ad.iw + 15) / 16, (ad.ih + 15) / 16), dim3(16, 16), 0, s>>>(a, ad, k);
    k_cacao_generate_adaptive<<<dim3(halfGrid.x, halfGrid.y, 4), wave, 0, s>>>(a, all, ad);
    launch_blur_apply(s, a, shared, perPass);
    return hipGetLastError();
}

} // namespace vqk
