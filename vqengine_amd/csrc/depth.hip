// depth.hip — the two compute passes between the 4x MSAA pre-pass / lit draw and the screen-space consumers (docs/DESIGN_DETAILS.md §7.10):
//   k_resolve_surfaces : Shaders/DepthResolve.hlsl:CSMain :36-100 (VQRenderer::ResolveMSAA_DepthPrePass, SceneRendering.cpp:1455-1471) — one lane per pixel:
//                        min of the four depth samples, the averaged + renormalised normal, the roughness (scene-colour alpha) of the nearest sample.
//                        Templated on the live outputs: the depth-only permutation reads the 16 B of depth samples per pixel and nothing else.
//   k_depth_hierarchy  : VQRenderer::DownsampleDepth (SceneRendering.cpp:2151-2183) == Shaders/DownsampleDepth.hlsl + FidelityFX SPD with min as the reduction.
//                        A workgroup of 256 lanes owns a 64 x 64 tile of level 0 (a lane: a 4 x 4 block), reduces it to the tile's single level-6 texel
//                        (registers, then lanes of a wave, then LDS) storing every level as it appears: levels 0-6 in one launch.
//                        MS = true takes "min of the pixel's four samples" as its level-0 load (resolve + level 0 + chain fused: 16 B/px in, 4 * 4/3 B/px out).
//   k_depth_tail       : one workgroup: level 6 (<= 64 x 64) is its tile, levels 7.. follow the same way. A second launch, not a hand-off inside the first:
//                        the in-kernel form (every workgroup releases at agent scope and counts itself in, the last arrival carries on) gave the same bits
//                        and measured 2.2x slower at 3840 x 2160 — 2040 L2 write-backs — and 2-3 us faster at 1280 x 720 (profiles/r8a_depth_chain.md).
// Contract of a level (tests/depth_ref.py:hierarchy): texel (x, y) of level l = min(min(a, b), min(c, d)) over level l-1 at (2x, 2y), (2x+1, 2y), (2x, 2y+1),
// (2x+1, 2y+1); a coordinate outside level l-1 reads 0.0; min is fminf (a NaN operand is dropped, the order of +0 / -0 is not specified: DESIGN.md §3).
#include "vq_internal.h"
#include "vq_devmath.h"

using namespace vqd;

namespace vqk {

namespace {

// ------------------------------------------------------------------------------------------------------------------------------------------------
// DepthResolve.hlsl
// ------------------------------------------------------------------------------------------------------------------------------------------------
VQD float min4_seq(float4 d) { return min_(min_(min_(d.x, d.y), d.z), d.w); }                         // :56

// texNormalsMS.Load(..).rgb of layer k's plane: UNORM10 -> float = c / 1023 correctly rounded (as ssr.hip reads Tex_SceneNormals), or the float planes as they are
VQD f3 load_normal01(const void* p, size_t i, bool f32) {
    if (f32) { const float4 n = ((const float4*)p)[i]; return mk3(n.x, n.y, n.z); }
    const uint32_t q = ((const uint32_t*)p)[i];
    return mk3(fdiv_((float)(q & 1023u), 1023.0f), fdiv_((float)((q >> 10) & 1023u), 1023.0f), fdiv_((float)((q >> 20) & 1023u), 1023.0f));
}
VQD uint32_t unorm10(float c) { return (uint32_t)(int)(saturate(c) * 1023.0f + 0.5f); }               // the store of k_scene_normals_from_materials; NaN -> 0

template <bool D, bool N, bool R>
__global__ __launch_bounds__(256) void k_resolve_surfaces(SurfArgs a) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= a.width) return;
    const float4 d = a.depthMS[(size_t)y * a.depthPitch + x];                                         // :50-53, `half` is float in this PSO
    const float minDepth = min4_seq(d);
    if (D) a.outDepth[(size_t)y * a.outDepthPitch + x] = minDepth;                                    // :92
    if (!N && !R) return;
    // sample ownership, as vqhip_forward_lighting_msaa: the lowest layer whose mask has the bit; what is left is background
    uint32_t own[VQHIP_MSAA_MAX_LAYERS];
    uint32_t bgm = 0xFu;
    #pragma unroll
    for (int k = 0; k < VQHIP_MSAA_MAX_LAYERS; ++k) {
        const uint32_t m = k < a.layers ? (uint32_t)a.L[k].cov[(size_t)y * a.covPitch + x] : 0u;      // wave-uniform test
        own[k] = m & bgm;
        bgm &= ~m;
    }
    if (N) {
        // :74-78. One decode per OWNING layer (an interior pixel: one), then the four-sample arithmetic exactly as written: (n + n) + n is not 3n.
        f3 s[4];
        #pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = mk3(-1.0f, -1.0f, -1.0f);                                  // background: the clear value 0 -> 0 * 2 - 1
        #pragma unroll
        for (int k = 0; k < VQHIP_MSAA_MAX_LAYERS; ++k) {
            if (own[k] == 0u) continue;
            const f3 n01 = load_normal01(a.L[k].normals, (size_t)y * a.L[k].nPitch + x, a.nInF32 != 0);
            const f3 n = mk3(n01.x * 2.0f - 1.0f, n01.y * 2.0f - 1.0f, n01.z * 2.0f - 1.0f);
            #pragma unroll
            for (int j = 0; j < 4; ++j) if ((own[k] >> j) & 1u) s[j] = n;
        }
        const f3 sum = add(add(add(s[0], s[1]), s[2]), s[3]);
        const f3 nn = normalize_rt(mul(sum, 0.25f), a.arithDxc != 0);                                  // a zero sum: 0 / 0 | 0 * inf = NaN in both readings
        const float ox = (nn.x + 1.0f) * 0.5f, oy = (nn.y + 1.0f) * 0.5f, oz = (nn.z + 1.0f) * 0.5f;
        const size_t o = (size_t)y * a.outNormalsPitch + x;
        // a float3 written to a four-channel UAV: alpha undefined in the reference, 1 here (as vqhip_fsr_rcas)
        if (a.nOutF32) ((float4*)a.outNormals)[o] = make_float4(ox, oy, oz, 1.0f);
        else           ((uint32_t*)a.outNormals)[o] = unorm10(ox) | (unorm10(oy) << 10) | (unorm10(oz) << 20) | (3u << 30);
    }
    if (R) {
        int iSample = 0;                                                                               // :59-62: on a tie the highest equal index wins
        if (minDepth == d.y) iSample = 1;
        if (minDepth == d.z) iSample = 2;
        if (minDepth == d.w) iSample = 3;
        const uint32_t bit = 1u << iSample;
        // the alpha Tex_SceneColorMSAA holds at that sample: the owner's gb1.w as PSMain's output stores it, or the background's alpha
        float alpha = 0.0f;
        if (bgm & bit) {
            if (a.bg) alpha = a.sceneF32 ? ((const float4*)a.bg)[(size_t)y * a.bgPitch + x].w : (float)((const _Float16*)a.bg)[((size_t)y * a.bgPitch + x) * 4 + 3];
        } else {
            #pragma unroll
            for (int k = 0; k < VQHIP_MSAA_MAX_LAYERS; ++k)
                if (own[k] & bit) alpha = a.L[k].gb1[(size_t)y * a.L[k].rPitch + x].w;
        }
        const size_t o = (size_t)y * a.scenePitch + x;                                                 // :98: rgb stays as it is
        if (a.sceneF32) ((float*)a.scene)[o * 4 + 3] = alpha;
        else            ((_Float16*)a.scene)[o * 4 + 3] = to_f16(alpha);                               // exact for a background alpha that was widened from binary16
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// DownsampleDepth.hlsl + SPD
// ------------------------------------------------------------------------------------------------------------------------------------------------
VQD float red4(float a, float b, float c, float d) { return min_(min_(a, b), min_(c, d)); }          // SpdReduce4, DownsampleDepth.hlsl:72
VQD float lane_val(float v, int lane) { return __shfl(v, lane, 64); }

// Morton order of the 256 lanes over the tile's 16 x 16 blocks: the four lanes 4q .. 4q+3 hold a 2 x 2 group (a = +0, b = +1, c = +2, d = +3), so do
// the four quads 16r .. 16r+15 one level up, and so on: levels 3-5 are lane reads inside a wave, level 6 joins the four waves through LDS.
VQD int compact_even_bits(uint32_t t) { t &= 0x55u; t = (t | (t >> 1)) & 0x33u; t = (t | (t >> 2)) & 0x0Fu; return (int)t; }

struct Level { float* p; int w, h; };
VQD Level level_of(const HierArgs& a, int l) {
    Level r;
    r.p = a.mips + a.off[l];
    r.w = max(1, a.width >> l); r.h = max(1, a.height >> l);
    return r;
}
VQD void store1(const Level& L, bool live, int x, int y, float v) { if (live && x < L.w && y < L.h) L.p[(size_t)y * L.w + x] = v; }

// Reduces the 64 x 64 tile (tx, ty) of level B whose texels the lane holds in v[4][4] (block origin (X0, Y0), outside the level: 0) to levels B+1 .. B+6,
// storing each texel that lies inside a level < a.levels. `top` follows what lane 0 of tile (0, 0) holds for level a.levels - 1.
template <int B, bool VEC>
VQD void reduce_tile(const HierArgs& a, const float v[4][4], int t, int X0, int Y0, float* lds4, float& top) {
    const int L = a.levels, lane = t & 63;
    if (B == L - 1) top = v[0][0];
    float l1[2][2];
    #pragma unroll
    for (int j = 0; j < 2; ++j)
        #pragma unroll
        for (int i = 0; i < 2; ++i) l1[j][i] = red4(v[2 * j][2 * i], v[2 * j][2 * i + 1], v[2 * j + 1][2 * i], v[2 * j + 1][2 * i + 1]);
    if (B + 1 < L) {
        const Level o = level_of(a, B + 1);
        const int x = X0 >> 1, y = Y0 >> 1;
        #pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (VEC) { if (x < o.w && y + j < o.h) *(float2*)(o.p + (size_t)(y + j) * o.w + x) = make_float2(l1[j][0], l1[j][1]); }   // VEC: o.w is even
            else     { store1(o, true, x, y + j, l1[j][0]); store1(o, true, x + 1, y + j, l1[j][1]); }
        }
        if (B + 1 == L - 1) top = l1[0][0];
    }
    const float l2 = red4(l1[0][0], l1[0][1], l1[1][0], l1[1][1]);
    if (B + 2 < L) { store1(level_of(a, B + 2), true, X0 >> 2, Y0 >> 2, l2); if (B + 2 == L - 1) top = l2; }
    const int q = lane & ~3;
    const float l3 = red4(lane_val(l2, q), lane_val(l2, q + 1), lane_val(l2, q + 2), lane_val(l2, q + 3));
    if (B + 3 < L) { store1(level_of(a, B + 3), (t & 3) == 0, X0 >> 3, Y0 >> 3, l3); if (B + 3 == L - 1) top = l3; }
    const int r = lane & ~15;
    const float l4 = red4(lane_val(l3, r), lane_val(l3, r + 4), lane_val(l3, r + 8), lane_val(l3, r + 12));
    if (B + 4 < L) { store1(level_of(a, B + 4), (t & 15) == 0, X0 >> 4, Y0 >> 4, l4); if (B + 4 == L - 1) top = l4; }
    const float l5 = red4(lane_val(l4, 0), lane_val(l4, 16), lane_val(l4, 32), lane_val(l4, 48));
    if (B + 5 < L) { store1(level_of(a, B + 5), lane == 0, X0 >> 5, Y0 >> 5, l5); if (B + 5 == L - 1) top = l5; }
    if (B + 6 < L) {                                                                                    // wave-uniform
        if (lane == 0) lds4[t >> 6] = l5;
        __syncthreads();
        const float l6 = red4(lds4[0], lds4[1], lds4[2], lds4[3]);
        store1(level_of(a, B + 6), t == 0, X0 >> 6, Y0 >> 6, l6);
        if (B + 6 == L - 1) top = l6;
    }
}

// wave-wide min over the lanes, then over the four waves (every lane gets the result)
VQD float block_min(float m, int t, float* lds4) {
    #pragma unroll
    for (int s = 32; s > 0; s >>= 1) m = min_(m, __shfl_xor(m, s, 64));
    __syncthreads();                                                                                    // lds4 may still be read by the level-6 step
    if ((t & 63) == 0) lds4[t >> 6] = m;
    __syncthreads();
    m = min_(min_(lds4[0], lds4[1]), min_(lds4[2], lds4[3]));
    __syncthreads();
    return m;
}

// The tail: level 6 (<= 64 x 64) is the source tile — lane order and tile (0, 0) as before — and levels 7 .. follow; TRUE_TOP: the frame's minimum out of the
// tiles' minima.
VQD void finish_chain(const HierArgs& a, int t, int numTiles, bool trueTop, float* lds4, float& top, float& inMin) {
    float v[4][4];
    const Level s6 = level_of(a, 6);
    const int bx = compact_even_bits((uint32_t)t) * 4, by = compact_even_bits((uint32_t)t >> 1) * 4;
    #pragma unroll
    for (int j = 0; j < 4; ++j)
        #pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int x = bx + i, y = by + j;
            v[j][i] = (a.levels > 6 && x < s6.w && y < s6.h) ? s6.p[(size_t)y * s6.w + x] : 0.0f;
        }
    reduce_tile<6, false>(a, v, t, bx, by, lds4, top);
    if (trueTop) {
        float m = __builtin_inff();
        for (int i = t; i < numTiles; i += 256) m = min_(m, a.tileMin[i]);
        inMin = block_min(m, t, lds4);
    }
}

// The 1 x 1 top level. Default: what the reference's dispatch leaves there — SPD is handed the number of LEVELS as its number of reductions, and the surplus
// reduction (top texel + three out-of-extent neighbours) lands on the last subresource: min(top, 0) whenever the chain has <= 12 levels. TRUE_TOP: the frame's minimum.
VQD void store_top(const HierArgs& a, bool trueTop, float top, float inMin) {
    float* p = a.mips + a.off[a.levels - 1];
    if (trueTop) *p = inMin;
    else if (a.levels <= 12) *p = min_(top, 0.0f);
}

template <bool MS, bool VEC>
__global__ __launch_bounds__(256) void k_depth_hierarchy(HierArgs a) {
    __shared__ float lds4[4];
    const int t = threadIdx.x;
    const int tilesX = (a.width + 63) >> 6, tilesY = (a.height + 63) >> 6, numTiles = tilesX * tilesY;
    const int tx = (int)blockIdx.x % tilesX, ty = (int)blockIdx.x / tilesX;
    const int X0 = tx * 64 + compact_even_bits((uint32_t)t) * 4, Y0 = ty * 64 + compact_even_bits((uint32_t)t >> 1) * 4;
    const bool trueTop = (a.flags & VQHIP_DEPTH_HIERARCHY_TRUE_TOP) != 0;
    // ---- level 0: load (plain, or the min of the four samples), copy, the lane's share of the frame's true minimum
    float v[4][4];
    float inMin = __builtin_inff();
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = Y0 + j;
        #pragma unroll
        for (int i = 0; i < 4; ++i) v[j][i] = 0.0f;                                                     // outside the frame: D3D's out-of-bounds typed load
        if (y >= a.height) continue;
        if (MS) {
            const float4* row = (const float4*)a.src + (size_t)y * a.srcPitch;
            #pragma unroll
            for (int i = 0; i < 4; ++i) if (X0 + i < a.width) v[j][i] = min4_seq(row[X0 + i]);
        } else if (VEC) {
            if (X0 < a.width) { const float4 r = *(const float4*)(a.src + (size_t)y * a.srcPitch + X0); v[j][0] = r.x; v[j][1] = r.y; v[j][2] = r.z; v[j][3] = r.w; }
        } else {
            #pragma unroll
            for (int i = 0; i < 4; ++i) if (X0 + i < a.width) v[j][i] = a.src[(size_t)y * a.srcPitch + X0 + i];
        }
        float* o = a.mips + (size_t)y * a.width;
        if (VEC) { if (X0 < a.width) *(float4*)(o + X0) = make_float4(v[j][0], v[j][1], v[j][2], v[j][3]); }      // VEC: width % 4 == 0, a block is inside or outside as a whole
        else {
            #pragma unroll
            for (int i = 0; i < 4; ++i) if (X0 + i < a.width) o[X0 + i] = v[j][i];
        }
        #pragma unroll
        for (int i = 0; i < 4; ++i) if (X0 + i < a.width) inMin = min_(inMin, v[j][i]);
    }
    float top = 0.0f;
    reduce_tile<0, VEC>(a, v, t, X0, Y0, lds4, top);
    if (trueTop) inMin = block_min(inMin, t, lds4);
    if (numTiles > 1) {                                                                                 // levels 7+ and the top level: k_depth_tail
        if (trueTop && t == 0) a.tileMin[blockIdx.x] = inMin;
        return;
    }
    if (t == 0) store_top(a, trueTop, top, inMin);
}

__global__ __launch_bounds__(256) void k_depth_tail(HierArgs a) {
    __shared__ float lds4[4];
    const int t = threadIdx.x;
    const int numTiles = ((a.width + 63) >> 6) * ((a.height + 63) >> 6);
    const bool trueTop = (a.flags & VQHIP_DEPTH_HIERARCHY_TRUE_TOP) != 0;
    float top = 0.0f, inMin = 0.0f;
    finish_chain(a, t, numTiles, trueTop, lds4, top, inMin);
    if (t == 0) store_top(a, trueTop, top, inMin);
}

template <bool D, bool N> hipError_t launch_resolve_r(hipStream_t s, const SurfArgs& a, dim3 grid) {
    if (a.scene) hipLaunchKernelGGL((k_resolve_surfaces<D, N, true>), grid, dim3(256), 0, s, a);
    else         hipLaunchKernelGGL((k_resolve_surfaces<D, N, false>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace

hipError_t launch_resolve_surfaces(hipStream_t s, const SurfArgs& a) {
    const dim3 grid((a.width + 255) / 256, a.height);
    if (a.outDepth) return a.outNormals ? launch_resolve_r<true, true>(s, a, grid) : launch_resolve_r<true, false>(s, a, grid);
    return a.outNormals ? launch_resolve_r<false, true>(s, a, grid) : launch_resolve_r<false, false>(s, a, grid);
}

hipError_t launch_depth_hierarchy(hipStream_t s, const HierArgs& a, bool ms) {
    const int tiles = ((a.width + 63) / 64) * ((a.height + 63) / 64);
    // wide loads / stores: every 4-texel block of level 0 and 2-texel block of level 1 is inside or outside as a whole and naturally aligned
    const bool vec = a.width % 4 == 0 && ((uintptr_t)a.mips & 15u) == 0 && (ms || (a.srcPitch % 4 == 0 && ((uintptr_t)a.src & 15u) == 0));
    if (ms) { if (vec) hipLaunchKernelGGL((k_depth_hierarchy<true, true>), dim3(tiles), dim3(256), 0, s, a);
              else     hipLaunchKernelGGL((k_depth_hierarchy<true, false>), dim3(tiles), dim3(256), 0, s, a); }
    else    { if (vec) hipLaunchKernelGGL((k_depth_hierarchy<false, true>), dim3(tiles), dim3(256), 0, s, a);
              else     hipLaunchKernelGGL((k_depth_hierarchy<false, false>), dim3(tiles), dim3(256), 0, s, a); }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || tiles == 1) return e;
    hipLaunchKernelGGL(k_depth_tail, dim3(1), dim3(256), 0, s, a);                                      // levels 7+, the top level
    return hipGetLastError();
}

} // namespace vqk
