// ssr_trace.hip — SSR's ray list and hierarchical march for gfx950 (docs/DESIGN_DETAILS.md §7.11):
//   k_ssr_classify_count / k_ssr_classify_scan / k_ssr_classify_scatter
//                     == the ray decision of Shaders/ScreenSpaceReflections/ClassifyReflectionTiles.hlsl:ClassifyTiles :96-145,157-161 (IsBaseRay :65-74,
//                        PackRayCoords Common.hlsl:62-71, FFX_DNSR_Reflections_RemapLane8x8 ffx_denoiser_reflections_common.h:38-51) in ONE reproducible order:
//                        8 x 8 tiles row-major, lanes 0..63 of the remap inside a tile. count -> scan -> scatter: three launches, no workgroup waits for another.
//   k_ssr_intersect   == Shaders/ScreenSpaceReflections/Intersect.hlsl:CSMain :145-216 + AMDFidelityFX/SSSR/ffx_sssr.h for every entry of the list. One lane per
//                        ray, one wave per 64 consecutive rays (a persistent grid strides over the 64-ray groups, so the low-occupancy exit of :116 sees the
//                        waves the list fixes, whatever the launch shape). The march is one dependent pyramid load per iteration: its live state is origin,
//                        direction, inverse direction, position, t, mip and the two resolutions; the per-level offset / size come from a 16-entry LDS table;
//                        hit validation and the environment sample run after the loop.
// Every expression is evaluated AS WRITTEN (products and sums rounded one by one, a / b the IEEE quotient), in the reading vqhip_set_arithmetic selects.
#include "vq_internal.h"
#include "vq_devmath.h"
#include "vq_sampling.h"

using namespace vqd;

namespace vqk {

namespace {

// ---- classification ---------------------------------------------------------------------------------------------------------------------------
struct Cls { bool needsRay, tileHit; uint32_t packed; };

// lane `lane` of tile `tile`; all 64 lanes of the wave call it together (the copy flags read the quad neighbours' decision through a ballot)
VQD Cls classify_lane(const SsrClassifyArgs& a, uint32_t tile, uint32_t lane) {
    const uint32_t ty = tile / (uint32_t)a.tilesX, tx = tile - ty * (uint32_t)a.tilesX;
    const uint32_t x = tx * 8u + ((lane & 1u) | ((lane >> 2) & 6u)), y = ty * 8u + (((lane >> 1) & 3u) | ((lane >> 3) & 4u));   // RemapLane8x8
    const bool onScreen = x < (uint32_t)a.width && y < (uint32_t)a.height;
    float roughness = 0.0f, depth = 0.0f;                                                                           // a load outside the texture reads 0
    if (onScreen) {
        if (a.sceneF32) roughness = ((const float4*)a.scene)[(size_t)y * a.scenePitch + x].w;
        else            roughness = (float)((const _Float16*)a.scene)[((size_t)y * a.scenePitch + x) * 4 + 3];
        depth = a.depth[(size_t)y * a.depthPitch + x];
    }
    const bool reflective = depth < 1.0f;                                                                          // IsReflectiveSurface :59-63
    const bool glossy = roughness < a.roughnessThreshold;                                                          // Common.hlsl:108-110
    bool needsRay = onScreen && glossy && reflective;                                                              // :103-108
    const bool needsDenoiser = needsRay && !(roughness < 0.04f);                                                   // :111, Common.hlsl:112-114
    const uint32_t spq = a.samplesPerQuad;
    const bool base = spq == 1u ? ((x & 1u) | (y & 1u)) == 0u : spq == 2u ? (x & 1u) == (y & 1u) : true;           // IsBaseRay :65-74
    needsRay = needsRay && (!needsDenoiser || base);                                                               // :115
    if (a.varianceGuided && needsDenoiser && !needsRay) {                                                          // :117-120
        const float var = a.variance ? (float)((const _Float16*)a.variance)[(size_t)y * a.variancePitch + x] : 0.0f;
        needsRay = needsRay || (var > a.varianceThreshold);
    }
    const bool requireCopy = !needsRay && needsDenoiser;                                                           // :129
    const uint64_t rc = __ballot(requireCopy);
    const bool ch = (spq != 4u) && base && ((rc >> (lane ^ 1u)) & 1u);                                             // :130-132
    const bool cv = (spq == 1u) && base && ((rc >> (lane ^ 2u)) & 1u);
    const bool cd = (spq == 1u) && base && ((rc >> (lane ^ 3u)) & 1u);
    Cls c;
    c.needsRay = needsRay;
    c.tileHit = glossy && reflective;                                                                              // :126, as written: not masked by the screen test
    c.packed = ((uint32_t)cd << 31) | ((uint32_t)cv << 30) | ((uint32_t)ch << 29) | ((y & 0x3fffu) << 15) | (x & 0x7fffu);
    return c;
}

// a wave per tile, four tiles per workgroup
__global__ __launch_bounds__(256) void k_ssr_classify_count(SsrClassifyArgs a) {
    const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (tile >= (uint32_t)(a.tilesX * a.tilesY)) return;
    const Cls c = classify_lane(a, tile, lane);
    const uint64_t rays = __ballot(c.needsRay), hit = __ballot(c.tileHit);
    if (lane == 0) { a.tileRays[tile] = (uint32_t)__popcll(rays); a.tileFlag[tile] = hit ? 1u : 0u; }
}

// ONE workgroup: exclusive scan of the per-tile ray counts and tile flags, in place, then the two counters. <= 512 x 512 tiles: a lane owns a run of at most 256
// consecutive tiles, a multiple of 4 long, and walks it with 16-byte loads and stores (lane-strided dword accesses are one cache line per lane and made this kernel
// the longest of the three). The last vector of the last run may reach past the tile count: both arrays are kMaxSsrTiles long, and those elements are never read.
__global__ __launch_bounds__(1024) void k_ssr_classify_scan(SsrClassifyArgs a) {
    __shared__ uint32_t sR[1024], sF[1024];
    const uint32_t n = (uint32_t)(a.tilesX * a.tilesY), t = threadIdx.x;
    const uint32_t per = (((n + 1023u) / 1024u) + 3u) & ~3u;
    const uint32_t i0 = t * per, i1 = min(i0 + per, n);
    uint32_t r = 0, f = 0;
    for (uint32_t i = i0; i < i1; i += 4) {
        const uint4 r4 = *(const uint4*)(a.tileRays + i), f4 = *(const uint4*)(a.tileFlag + i);
        const uint32_t rv[4] = { r4.x, r4.y, r4.z, r4.w }, fv[4] = { f4.x, f4.y, f4.z, f4.w };
        #pragma unroll
        for (uint32_t k = 0; k < 4; ++k) if (i + k < i1) { r += rv[k]; f += fv[k]; }
    }
    sR[t] = r; sF[t] = f;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint32_t pr = t >= d ? sR[t - d] : 0u, pf = t >= d ? sF[t - d] : 0u;
        __syncthreads();
        sR[t] += pr; sF[t] += pf;
        __syncthreads();
    }
    uint32_t br = sR[t] - r, bf = sF[t] - f;                                                                       // exclusive
    for (uint32_t i = i0; i < i1; i += 4) {
        const uint4 r4 = *(const uint4*)(a.tileRays + i), f4 = *(const uint4*)(a.tileFlag + i);
        const uint32_t rv[4] = { r4.x, r4.y, r4.z, r4.w }, fv[4] = { f4.x, f4.y, f4.z, f4.w };
        uint32_t ro[4], fo[4];
        #pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const bool in = i + k < i1;
            ro[k] = br; fo[k] = (in && fv[k]) ? bf : 0xffffffffu;
            if (in) { br += rv[k]; bf += fv[k]; }
        }
        *(uint4*)(a.tileRays + i) = make_uint4(ro[0], ro[1], ro[2], ro[3]);
        *(uint4*)(a.tileFlag + i) = make_uint4(fo[0], fo[1], fo[2], fo[3]);
    }
    if (t == 1023u) { a.counters[0] = sR[t]; a.counters[1] = sF[t]; }
}

__global__ __launch_bounds__(256) void k_ssr_classify_scatter(SsrClassifyArgs a) {
    const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (tile >= (uint32_t)(a.tilesX * a.tilesY)) return;
    const Cls c = classify_lane(a, tile, lane);
    const uint64_t rays = __ballot(c.needsRay);
    const uint32_t at = a.tileRays[tile] + (uint32_t)__popcll(rays & ((1ull << lane) - 1ull));
    if (c.needsRay && at < (uint32_t)a.width * (uint32_t)a.height) a.rayList[at] = c.packed;                       // every ray is an on-screen pixel: the bound never cuts
    if (lane == 0 && a.tileList) {
        const uint32_t slot = a.tileFlag[tile];
        const uint32_t ty = tile / (uint32_t)a.tilesX, tx = tile - ty * (uint32_t)a.tilesX;
        if (slot != 0xffffffffu) a.tileList[slot] = (((ty * 8u) & 0xffffu) << 16) | ((tx * 8u) & 0xffffu);          // StoreDenoiserTile :55-57
    }
}

// ---- intersection -----------------------------------------------------------------------------------------------------------------------------
// min / max as selects (HLSL min / max = minNum / maxNum; the tie of +0 and -0 is pinned here): the second operand unless the first one wins
VQD float min2(float a, float b) { return (b < a || a != a) ? b : a; }
VQD float max2(float a, float b) { return (b > a || a != a) ? b : a; }

VQD float4 mulM(const VQ_matrix& M, float x, float y, float z, float w) {                                          // mul(M_hlsl, float4(v, w)), as ssr.hip:mul_M_v4
    float o[4];
    #pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = ((x * M.m[0][j] + y * M.m[1][j]) + z * M.m[2][j]) + w * M.m[3][j];
    return make_float4(o[0], o[1], o[2], o[3]);
}
VQD f3 inv_project(const VQ_matrix& M, float u, float v, float z) {                                                // InvProjectPosition, Common.hlsl:98-104
    const float cy = 1.0f - v;
    const float px = 2.0f * u - 1.0f, py = 2.0f * cy - 1.0f;
    const float4 p = mulM(M, px, py, z, 1.0f);
    return mk3(fdiv_(p.x, p.w), fdiv_(p.y, p.w), fdiv_(p.z, p.w));
}
VQD float smoothstep_(float lo, float hi, float x) { const float t = saturate(fdiv_(x - lo, hi - lo)); return (t * t) * (3.0f - 2.0f * t); }

struct Levels { const uint32_t* off; const int* w; const int* h; };
VQD float load_depth(const float* mips, const Levels& L, int x, int y, int mip) {                                  // Texture.Load: outside the level, or no such level: 0
    const uint32_t m = (uint32_t)mip > 15u ? 15u : (uint32_t)mip;
    const int w = L.w[m], h = L.h[m];
    float v = 0.0f;
    if ((uint32_t)x < (uint32_t)w && (uint32_t)y < (uint32_t)h) v = mips[L.off[m] + (uint32_t)y * (uint32_t)w + (uint32_t)x];
    return v;
}
VQD f3 load_normal01(const SsrTraceArgs& a, int x, int y) {
    f3 n = mk3(0.0f, 0.0f, 0.0f);
    if ((uint32_t)x < (uint32_t)a.width && (uint32_t)y < (uint32_t)a.height) {
        if (a.normF32) { const float4 q = ((const float4*)a.normals)[(size_t)y * a.normalPitch + x]; n = mk3(q.x, q.y, q.z); }
        else { const uint32_t q = ((const uint32_t*)a.normals)[(size_t)y * a.normalPitch + x];
               n = mk3(fdiv_((float)(q & 1023u), 1023.0f), fdiv_((float)((q >> 10) & 1023u), 1023.0f), fdiv_((float)((q >> 20) & 1023u), 1023.0f)); }
    }
    return n;
}
VQD f3 world_normal(const SsrTraceArgs& a, int x, int y, bool dxc) {                                               // FFX_SSSR_LoadWorldSpaceNormal, Intersect.hlsl:42-44
    const f3 n = load_normal01(a, x, y);
    return normalize_rt(mk3(2.0f * n.x - 1.0f, 2.0f * n.y - 1.0f, 2.0f * n.z - 1.0f), dxc);
}
VQD void store_out(const SsrTraceArgs& a, uint32_t x, uint32_t y, float4 v) {
    if (x >= (uint32_t)a.width || y >= (uint32_t)a.height) return;                                                // a store outside the UAV is dropped
    if (a.outF32) store_px<0>(a.out, (size_t)y * a.outPitch + x, v); else store_px<1>(a.out, (size_t)y * a.outPitch + x, v);
}

// 8 waves per SIMD (64 VGPRs, 72 B of scratch per lane outside the loop) against 6 (80) and 5 (90, the compiler's own choice): measured, profiles/r9a_ssr_trace.md
__global__ __launch_bounds__(256, 8) void k_ssr_intersect(SsrTraceArgs a) {
    __shared__ uint32_t sOff[16];
    __shared__ int sW[16], sH[16];
    if (threadIdx.x < 16) {                                                                                        // level l: max(1, W >> l) x max(1, H >> l), densely packed
        const int l = (int)threadIdx.x;
        uint32_t off = 0;
        for (int k = 0; k < l && k < a.levels; ++k) off += (uint32_t)max(1, a.width >> k) * (uint32_t)max(1, a.height >> k);
        const bool in = l < a.levels;
        sOff[l] = in ? off : 0u; sW[l] = in ? max(1, a.width >> l) : 0; sH[l] = in ? max(1, a.height >> l) : 0;
    }
    __syncthreads();
    const Levels L = { sOff, sW, sH };
    const uint32_t cap = (uint32_t)a.width * (uint32_t)a.height;
    const uint32_t n = min(a.counters[0], cap);
    const uint32_t groups = (n + 63u) / 64u, lane = threadIdx.x & 63u;
    const bool dxc = a.arithDxc != 0;
    const float fW = (float)a.width, fH = (float)a.height;
    for (uint32_t g = blockIdx.x * 4u + (threadIdx.x >> 6); g < groups; g += gridDim.x * 4u) {
        const uint32_t ray = g * 64u + lane;
        const bool live = ray < n;                                                                                 // CSMain :149
        const uint32_t packed = live ? a.rayList[ray] : 0u;
        const int cx = (int)(packed & 0x7fffu), cy = (int)((packed >> 15) & 0x3fffu);                              // UnpackRayCoords, Common.hlsl:73-79
        const float u = ((float)cx + 0.5f) * a.invDimX, v = ((float)cy + 0.5f) * a.invDimY;                        // :160
        const f3 wn = world_normal(a, cx, cy, dxc);                                                                // :162
        float roughness = 0.0f;                                                                                    // :163, R8_UNORM: c / 255
        if ((uint32_t)cx < (uint32_t)a.width && (uint32_t)cy < (uint32_t)a.height) roughness = fdiv_((float)a.roughness[(size_t)cy * a.width + cx], 255.0f);
        const bool mirror = roughness < 0.041f;                                                                    // :139-141
        const int mdm = mirror ? 0 : (int)a.mostDetailedMip;                                                       // :166
        const float scale0 = __uint_as_float((uint32_t)(127 - mdm) << 23);                                         // pow(0.5, mip) == 2^-mip exactly
        float resX = fW * scale0, resY = fH * scale0;                                                              // FFX_SSSR_GetMipResolution
        const float z = load_depth(a.mips, L, f2i_trunc(u * resX), f2i_trunc(v * resY), mdm);                      // :168
        const f3 vray = inv_project(a.invProj, u, v, z);                                                           // :171
        const f3 dirV = normalize_rt(vray, dxc);                                                                   // :172
        const float4 nv4 = mulM(a.view, wn.x, wn.y, wn.z, 0.0f);                                                   // :174
        const f3 N = mk3(nv4.x, nv4.y, nv4.z);
        // SampleReflectionVector :114-130. CreateTBN :92-108: rows U, cross(N, U), N
        f3 U;
        if (abs_(N.z) > 0.0f) { const float k = sqrt_(N.y * N.y + N.z * N.z); U = mk3(0.0f, fdiv_(-N.z, k), fdiv_(N.y, k)); }
        else                  { const float k = sqrt_(N.x * N.x + N.y * N.y); U = mk3(fdiv_(N.y, k), fdiv_(-N.x, k), 0.0f); }
        const f3 B = cross(N, U);
        const f3 nd = neg(dirV);
        const f3 Ve = mk3(dot_lit(nd, U), dot_lit(nd, B), dot_lit(nd, N));                                         // mul(-view_direction, tbn_transform)
        const uint32_t nz = ((uint32_t)(cy & 127) * 128u + (uint32_t)(cx & 127)) * 2u;                             // SampleRandomVector2D :110-112
        const float U1 = fdiv_((float)a.noise[nz], 255.0f), U2 = fdiv_((float)a.noise[nz + 1], 255.0f);
        // SampleGGXVNDF :63-82, alpha_x = alpha_y = roughness
        const f3 Vh = normalize_rt(mk3(roughness * Ve.x, roughness * Ve.y, Ve.z), dxc);
        const float lensq = Vh.x * Vh.x + Vh.y * Vh.y;
        f3 T1 = mk3(1.0f, 0.0f, 0.0f);
        if (lensq > 0.0f) { const float rs = rsqrt(lensq); T1 = mk3(-Vh.y * rs, Vh.x * rs, 0.0f * rs); }
        const f3 T2 = cross(Vh, T1);
        const float rr = sqrt_(U1);
        const float phi = 6.28318548202514648f * U2;                                                               // 2.0 * M_PI, M_PI = 3.14159265358979f
        float sn, cs;
        sincos_(phi, &sn, &cs);
        const float t1 = rr * cs;
        float t2 = rr * sn;
        const float sh = 0.5f * (1.0f + Vh.z);
        t2 = (1.0f - sh) * sqrt_(1.0f - t1 * t1) + sh * t2;
        const float nhz = sqrt_(max2(0.0f, (1.0f - t1 * t1) - t2 * t2));
        const f3 Nh = mk3((t1 * T1.x + t2 * T2.x) + nhz * Vh.x, (t1 * T1.y + t2 * T2.y) + nhz * Vh.y, (t1 * T1.z + t2 * T2.z) + nhz * Vh.z);
        const f3 Ne = normalize_rt(mk3(roughness * Nh.x, roughness * Nh.y, max2(0.0f, Nh.z)), dxc);
        const f3 Rt = reflect_rt(neg(Ve), Ne, dxc);                                                                // :125
        const f3 Rv = mk3((Rt.x * U.x + Rt.y * B.x) + Rt.z * N.x, (Rt.x * U.y + Rt.y * B.y) + Rt.z * N.y, (Rt.x * U.z + Rt.y * B.z) + Rt.z * N.z);   // :128-129
        // ProjectDirection, Common.hlsl:83-95
        const float4 pp = mulM(a.proj, vray.x + Rv.x, vray.y + Rv.y, vray.z + Rv.z, 1.0f);
        const float ppx = 0.5f * fdiv_(pp.x, pp.w) + 0.5f, ppy = 1.0f - (0.5f * fdiv_(pp.y, pp.w) + 0.5f), ppz = fdiv_(pp.z, pp.w);
        const float ox = u, oy = v, oz = z;
        const float dx = ppx - ox, dy = ppy - oy, dz = ppz - oz;

        // FFX_SSSR_HierarchicalRaymarch, ffx_sssr.h:86-127
        const float ix = dx != 0.0f ? fdiv_(1.0f, dx) : 3.402823466e+38f, iy = dy != 0.0f ? fdiv_(1.0f, dy) : 3.402823466e+38f,
                    iz = dz != 0.0f ? fdiv_(1.0f, dz) : 3.402823466e+38f;
        int mip = mdm;
        float rinvX = fdiv_(1.0f, resX), rinvY = fdiv_(1.0f, resY);
        const float e2 = 0.005f * __uint_as_float((uint32_t)(127 + mdm) << 23);                                    // 0.005 * exp2(most_detailed_mip)
        float uoX = fdiv_(e2, fW), uoY = fdiv_(e2, fH);
        uoX = dx < 0.0f ? -uoX : uoX; uoY = dy < 0.0f ? -uoY : uoY;
        const float foX = dx < 0.0f ? 0.0f : 1.0f, foY = dy < 0.0f ? 0.0f : 1.0f;
        float t, px, py, pz;
        {   // FFX_SSSR_InitialAdvanceRay :27-38
            const float plX = (__builtin_floorf(resX * ox) + foX) * rinvX + uoX, plY = (__builtin_floorf(resY * oy) + foY) * rinvY + uoY;
            const float tx = plX * ix - ox * ix, ty = plY * iy - oy * iy;
            t = min2(tx, ty);
            px = ox + t * dx; py = oy + t * dy; pz = oz + t * dz;
        }
        uint32_t i = 0;
        bool lowOcc = false;
        bool in = live && i < a.maxIter && mip >= mdm;                                                             // the while condition :113
        for (;;) {
            const uint64_t act = __ballot(in);                                                                     // the lanes of this wave inside the loop at this iteration
            if (!act) break;
            if (in) {
                const float mpx = resX * px, mpy = resY * py;
                const float sz = load_depth(a.mips, L, f2i_trunc(mpx), f2i_trunc(mpy), mip);                       // :115
                lowOcc = !mirror && (uint32_t)__popcll(act) <= a.minOcc;                                           // :116
                // FFX_SSSR_AdvanceRay :40-79
                const float plX = (__builtin_floorf(mpx) + foX) * rinvX + uoX, plY = (__builtin_floorf(mpy) + foY) * rinvY + uoY;
                const float tx = plX * ix - ox * ix, ty = plY * iy - oy * iy;
                float tz = sz * iz - oz * iz;
                tz = dz > 0.0f ? tz : 3.402823466e+38f;
                const float tmin = min2(min2(tx, ty), tz);
                const bool above = sz > pz;
                const bool skipped = (__float_as_uint(tmin) != __float_as_uint(tz)) && above;
                t = above ? tmin : t;
                px = ox + t * dx; py = oy + t * dy; pz = oz + t * dz;
                mip += skipped ? 1 : -1;
                resX *= skipped ? 0.5f : 2.0f; resY *= skipped ? 0.5f : 2.0f;
                rinvX *= skipped ? 2.0f : 0.5f; rinvY *= skipped ? 2.0f : 0.5f;
                ++i;
                in = i < a.maxIter && mip >= mdm && !lowOcc;
            }
        }
        if (!live) continue;
        const bool validHit = i <= a.maxIter;                                                                      // :124, as the reference has it

        const f3 wo = inv_project(a.invViewProj, ox, oy, oz), wh = inv_project(a.invViewProj, px, py, pz);         // :182-184
        const f3 wray = sub(wh, wo);
        float conf = 0.0f;                                                                                         // FFX_SSSR_ValidateHit :129-173
        bool sample = validHit && !((px < 0.0f) || (py < 0.0f) || (px > 1.0f) || (py > 1.0f));
        sample = sample && !((abs_(px - u) < fdiv_(2.0f, fW)) && (abs_(py - v) < fdiv_(2.0f, fH)));
        const int hx = f2i_trunc(fW * px), hy = f2i_trunc(fH * py);
        if (sample) {
            const float sz = load_depth(a.mips, L, hx / 2, hy / 2, 1);
            const f3 hn = world_normal(a, hx, hy, dxc);
            if (!(sz == 1.0f) && !(dot_rt(hn, wray, dxc) > 0.0f)) {
                const f3 vs = inv_project(a.invProj, px, py, sz), vh = inv_project(a.invProj, px, py, pz);
                const float dist = length_rt(sub(vs, vh), dxc);
                const float fovX = 0.05f * fdiv_(fH, fW), fovY = 0.05f * 1.0f;
                const float bx = smoothstep_(0.0f, fovX, px) * (1.0f - smoothstep_(1.0f - fovX, 1.0f, px));
                const float by = smoothstep_(0.0f, fovY, py) * (1.0f - smoothstep_(1.0f - fovY, 1.0f, py));
                const float vignette = bx * by;
                float c = 1.0f - smoothstep_(0.0f, a.thickness, dist);
                c *= c;
                conf = vignette * c;
            }
        }
        const float rayLen = max2(0.0f, length_rt(wray, dxc));                                                     // :187
        f3 rad = mk3(0.0f, 0.0f, 0.0f);
        if (conf > 0.0f && (uint32_t)hx < (uint32_t)a.width && (uint32_t)hy < (uint32_t)a.height) {                // :190-193
            const float4 c = a.litF32 ? load_px<0>(a.lit, (size_t)hy * a.litPitch + hx) : load_px<1>(a.lit, (size_t)hy * a.litPitch + hx);
            rad = mk3(c.x, c.y, c.z);
        }
        // SampleEnvironmentMap :132-137 (level 0), EnvironmentBRDF as ssr.hip
        const float4 rw4 = mulM(a.invView, Rv.x, Rv.y, Rv.z, 0.0f);                                                // :196
        const float NdotV = saturate(dot_rt(N, neg(dirV), dxc));
        const f3 d = mk3((rw4.x * a.rot[0][0] + rw4.y * a.rot[1][0]) + rw4.z * a.rot[2][0],
                         (rw4.x * a.rot[0][1] + rw4.y * a.rot[1][1]) + rw4.z * a.rot[2][1],
                         (rw4.x * a.rot[0][2] + rw4.y * a.rot[1][2]) + rw4.z * a.rot[2][2]);
        const float4 pre = sample_cube_lod_rgba16f(a.env.specular_cube, a.env.spec_res0, a.env.spec_mips, d, 0.0f);
        const float2 sb = sample_2d_rg16f_clamp(a.env.brdf_lut, a.env.lut_size, a.env.lut_size, NdotV, roughness);
        const float F0 = lerp_lit(0.04f, 0.0f, 1.0f);
        const float p5 = a.pow5ExpLog ? pow5_explog(1.0f - NdotV) : pow5(1.0f - NdotV);
        const float Ks = F0 + (max_(1.0f - roughness, F0) - F0) * p5;
        const float Kd = (1.0f - Ks) * (1.0f - 1.0f);
        const float diffuse = 0.0f * 0.0f;
        const float k = Ks * sb.x + sb.y;
        const f3 env = mk3(Kd * diffuse + pre.x * k, Kd * diffuse + pre.y * k, Kd * diffuse + pre.z * k);
        const float4 outv = make_float4(env.x + conf * (rad.x - env.x), env.y + conf * (rad.y - env.y), env.z + conf * (rad.z - env.z), rayLen);   // :198-200
        const uint32_t ux = (uint32_t)cx, uy = (uint32_t)cy;
        store_out(a, ux, uy, outv);                                                                                // :201-215
        if ((packed >> 29) & 1u) store_out(a, ux ^ 1u, uy, outv);
        if ((packed >> 30) & 1u) store_out(a, ux, uy ^ 1u, outv);
        if ((packed >> 31) & 1u) store_out(a, ux ^ 1u, uy ^ 1u, outv);
    }
}

} // namespace

hipError_t launch_ssr_classify(hipStream_t s, const SsrClassifyArgs& a) {
    const int tiles = a.tilesX * a.tilesY;
    const dim3 grid((tiles + 3) / 4);
    hipLaunchKernelGGL(k_ssr_classify_count, grid, dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ssr_classify_scan, dim3(1), dim3(1024), 0, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ssr_classify_scatter, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_ssr_intersect(hipStream_t s, const SsrTraceArgs& a, int nCUs) {
    // the grid fills every CU once with as many 256-lane workgroups as the kernel's register budget admits; it never exceeds the list's possible groups
    static const int perCU = [] {
        int n = 0;
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_ssr_intersect, 256, 0) == hipSuccess && n > 0 ? n : 2;
    }();
    if (nCUs <= 0) nCUs = 256;
    const uint32_t maxGroups = ((uint32_t)a.width * (uint32_t)a.height + 63u) / 64u;
    uint32_t blocks = (uint32_t)(perCU * nCUs);
    if (blocks > (maxGroups + 3u) / 4u) blocks = (maxGroups + 3u) / 4u;
    hipLaunchKernelGGL(k_ssr_intersect, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace vqk
