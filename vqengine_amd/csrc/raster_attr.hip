// raster_attr.hip — vqhip_scene_interpolants: the lit draw's PSInput planes from meshes and the owner plane of vqhip_scene_depth (a visibility-buffer resolve).
// The vertex stage is ForwardLighting.hlsl:TransformVertex (:143-188), the interpolation D3D's perspective-correct evaluation at the pixel centre.
// docs/DESIGN_DETAILS.md §7.18 is the contract (I0 owner lookup, I1 vertex stage in binary32, I2 weights and I3 attributes in binary64);
// tests/scene_interp_ref.py states it in numpy.
//   k_table_copy          : one ring slot's part of the draw table into the work buffer (uint4 copies)
//   k_scene_interpolants  : one lane per pixel, a wave = an 8 x 8 pixel block (neighbouring lanes share owners: the index, vertex and matrix fetches hit in
//                           cache). Owner q -> draw (per-lane binary search of the table, bounded by the number of draws) -> instance, triangle -> three vertices
//                           through the vertex stage -> weights -> 11 or 19 attributes; float4 stores, one plane at a time.
// Every index is checked before it is used: q against the call's instanced triangles, the three indices against numVertices. Nothing an owner plane or a mesh
// holds can move a load or a store out of bounds.
// vqhip_scene_quad_interpolants (§7.20 Q1) launches the QUAD instantiations of the same kernel: one more float4 plane, the owner triangle's uv at the two helper
// lanes' centres (i ^ 1, j) and (i, j ^ 1), evaluated by vq_raster_mask.h's maskUvAt — the statement of I2 / I3 the masked depth fill already uses for its helper lanes.
#include "vq_raster_mask.h"

namespace vqk {
using namespace vqd;
namespace {

constexpr int kLanes = 256;                       // four waves: a 16 x 16 pixel block
constexpr uint32_t kNoPrimitive = 0xffffffffu;
constexpr uint32_t kCanonicalNaN = 0x7fc00000u;

__global__ void __launch_bounds__(256) k_table_copy(const uint4* __restrict__ src, uint4* __restrict__ dst, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

struct Vert { float a[19]; };                     // world 3, N 3, T 3, uv 2, clip 4, prev 4 (§7.18 I1: 19 scalars, 11 without the sv planes)

// I1: ForwardLighting.hlsl:153-184 in the literal binary32 reading. `vPosition.xyz += float3(0, 0.0f, 0)` is a float3 add: all three components lose a -0.
template <bool SV>
VQD Vert vertexStage(const float* __restrict__ v, const VQ_matrix& wvp, const VQ_matrix& world, const VQ_matrix& nrm, const VQ_matrix* __restrict__ prev) {
    Vert r;
    const float x = v[0] + 0.0f, y = v[1] + 0.0f, z = v[2] + 0.0f;
    const float nx = v[3], ny = v[4], nz = v[5], tx = v[6], ty = v[7], tz = v[8];
    for (int j = 0; j < 3; ++j) {
        r.a[j] = ((x * world.m[0][j] + y * world.m[1][j]) + z * world.m[2][j]) + 1.0f * world.m[3][j];
        r.a[3 + j] = (nx * nrm.m[0][j] + ny * nrm.m[1][j]) + nz * nrm.m[2][j];
        r.a[6 + j] = (tx * nrm.m[0][j] + ty * nrm.m[1][j]) + tz * nrm.m[2][j];
    }
    r.a[9] = v[9]; r.a[10] = v[10];
    for (int j = 0; j < 4; ++j) {
        r.a[11 + j] = ((x * wvp.m[0][j] + y * wvp.m[1][j]) + z * wvp.m[2][j]) + 1.0f * wvp.m[3][j];
        r.a[15 + j] = SV ? ((x * prev->m[0][j] + y * prev->m[1][j]) + z * prev->m[2][j]) + 1.0f * prev->m[3][j] : 0.0f;
    }
    return r;
}

// I2: D(a, b) with (x, y, w) of two vertices; products of widened binary32 values are exact, every other operation rounds once
VQD double det(double X, double Y, double xa, double ya, double wa, double xb, double yb, double wb) {
    return (X * (ya * wb - wa * yb) - Y * (xa * wb - wa * xb)) + (xa * yb - ya * xb);
}

VQD uint32_t roundBits(double d) {
    const float f = (float)d;                     // one RNE rounding
    return f != f ? kCanonicalNaN : __float_as_uint(f);
}

// I0 .. I3 for the owner q of pixel (i, j): the record's words into out[] (left as they are when q owns nothing). Called with the lane's own q, or — from a wave whose
// 64 pixels share one owner — with that q as a wave-uniform value: the table entry, the indices, the vertices and the matrices then have uniform addresses and
// travel through the scalar cache, one fetch per wave instead of one per lane. The arithmetic is the same instruction sequence either way: identical bits.
// QUAD: also quad[0 .. 3] = (u_h, v_h, u_v, v_v), the owner's uv at the centres of pixels (i ^ 1, j) and (i, j ^ 1) — which may lie outside the viewport and outside
// the triangle. The three sub-determinants of each weight depend on the triangle alone and are shared by the two centres; with -ffp-contract=off that is the
// expression of det() bit for bit.
template <bool SV, bool QUAD>
VQD void resolveOwner(const SceneInterpArgs& a, const SurfaceJob* __restrict__ table, uint32_t q, int i, int j, uint32_t* out, uint32_t* quad) {
    int lo = 0, hi = a.numJobs - 1;               // the last job whose firstQ is <= q; numJobs >= 1 since totalTris > 0
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (table[mid].firstQ <= q) lo = mid; else hi = mid - 1; }
    const SurfaceJob& J = table[lo];
    const uint32_t r = q - J.firstQ, numTris = J.numTris;
    const uint32_t inst = r / numTris, tri = r % numTris;
    uint32_t idx[3];
    if (!fetchTriangle(J.indices, J.indexBits, tri, J.numVertices, idx) || inst >= J.numInstances) return;      // the latter holds by construction of firstQ; checked all the same
    const VQ_matrix& wvp = J.wvp[inst];
    const VQ_matrix& world = J.world[inst];
    const VQ_matrix& nrm = J.normal[inst];
    const VQ_matrix* prev = SV ? J.wvpPrev + inst : nullptr;
    const uint8_t* vb = J.vertices;
    const size_t stride = J.strideBytes;
    const Vert v0 = vertexStage<SV>((const float*)(vb + idx[0] * stride), wvp, world, nrm, prev);
    const Vert v1 = vertexStage<SV>((const float*)(vb + idx[1] * stride), wvp, world, nrm, prev);
    const Vert v2 = vertexStage<SV>((const float*)(vb + idx[2] * stride), wvp, world, nrm, prev);
    // I2
    const double X = pixelCentreX(i, a.width), Y = pixelCentreY(j, a.height);
    const double x0 = v0.a[11], y0 = v0.a[12], w0 = v0.a[14], x1 = v1.a[11], y1 = v1.a[12], w1 = v1.a[14], x2 = v2.a[11], y2 = v2.a[12], w2 = v2.a[14];
    const double k0 = det(X, Y, x1, y1, w1, x2, y2, w2), k1 = det(X, Y, x2, y2, w2, x0, y0, w0), k2 = det(X, Y, x0, y0, w0, x1, y1, w1);
    const double den = (k0 + k1) + k2;
    const double l1 = k1 / den, l2 = k2 / den;
    // I3
    for (int k = 0; k < (SV ? 19 : 11); ++k) {
        const double a0 = v0.a[k], a1 = v1.a[k], a2 = v2.a[k];
        const uint32_t bits = roundBits((a0 + l1 * (a1 - a0)) + l2 * (a2 - a0));
        // world -> ip0.xyz, N -> ip1.xyz, T -> ip2.xyz, uv -> ip0.w / ip1.w, clip -> sv[0], prev -> sv[1]
        const int at = k < 9 ? (k / 3) * 4 + k % 3 : k == 9 ? 3 : k == 10 ? 7 : k + 1;
        out[at] = bits;
    }
    out[11] = (uint32_t)J.materialIndex;
    if constexpr (QUAD) {                         // after I3: of the 57 vertex scalars only the nine of (x, y, w) and the six of uv are still live
        MaskUv t;
        t.P[0] = y1 * w2 - w1 * y2; t.Q[0] = x1 * w2 - w1 * x2; t.R[0] = x1 * y2 - y1 * x2;
        t.P[1] = y2 * w0 - w2 * y0; t.Q[1] = x2 * w0 - w2 * x0; t.R[1] = x2 * y0 - y2 * x0;
        t.P[2] = y0 * w1 - w0 * y1; t.Q[2] = x0 * w1 - w0 * x1; t.R[2] = x0 * y1 - y0 * x1;
        t.u[0] = v0.a[9]; t.v[0] = v0.a[10]; t.u[1] = v1.a[9]; t.v[1] = v1.a[10]; t.u[2] = v2.a[9]; t.v[2] = v2.a[10];
        const float2 h = maskUvAt(t, pixelCentreX(i ^ 1, a.width), Y), v = maskUvAt(t, X, pixelCentreY(j ^ 1, a.height));
        auto canon = [](float f) { return f != f ? kCanonicalNaN : __float_as_uint(f); };
        quad[0] = canon(h.x); quad[1] = canon(h.y); quad[2] = canon(v.x); quad[3] = canon(v.y);
    }
}

// QA: empty, or the one QuadPlane of vqhip_scene_quad_interpolants (the existing instantiations keep their parameter list)
VQD const QuadPlane& quadPlaneOf(const QuadPlane& p) { return p; }
template <bool SV, bool WAVE, class... QA>
__global__ void __launch_bounds__(kLanes) k_scene_interpolants(SceneInterpArgs a, const SurfaceJob* __restrict__ table, QA... quadPlane) {
    constexpr bool QUAD = sizeof...(QA) != 0;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), j = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (i >= a.width || j >= a.height) return;
    const uint32_t q = a.owner[(size_t)j * a.ownerPitch + i];

    uint32_t out[SV ? 20 : 12];
    for (int k = 0; k < (SV ? 20 : 12); ++k) out[k] = 0u;
    out[11] = kNoPrimitive;                       // asfloat(int32 -1)
    if constexpr (SV) { out[15] = 0x3f800000u; out[19] = 0x3f800000u; }
    uint32_t quad[4] = { 0u, 0u, 0u, 0u };

    // I0: q at or beyond the call's instanced triangles (0xFFFFFFFF included: the host refuses 2^29 or more) owns nothing
    const uint32_t q0 = __builtin_amdgcn_readfirstlane(q);
    if (WAVE && __builtin_amdgcn_ballot_w64(q != q0) == 0ull) {       // the wave's live lanes share one owner
        if (q0 < a.totalTris) resolveOwner<SV, QUAD>(a, table, q0, i, j, out, quad);
    } else if (q < a.totalTris) {
        resolveOwner<SV, QUAD>(a, table, q, i, j, out, quad);
    }
    const size_t at = (size_t)j * a.pitch + i;
    ((uint4*)a.ip[0])[at] = make_uint4(out[0], out[1], out[2], out[3]);
    ((uint4*)a.ip[1])[at] = make_uint4(out[4], out[5], out[6], out[7]);
    ((uint4*)a.ip[2])[at] = make_uint4(out[8], out[9], out[10], out[11]);
    if constexpr (SV) {
        const size_t sat = (size_t)j * a.svPitch + i;
        ((uint4*)a.sv[0])[sat] = make_uint4(out[12], out[13], out[14], out[15]);
        ((uint4*)a.sv[1])[sat] = make_uint4(out[16], out[17], out[18], out[19]);
    }
    if constexpr (QUAD) {
        const QuadPlane& qp = quadPlaneOf(quadPlane...);
        ((uint4*)qp.uv)[(size_t)j * qp.pitch + i] = make_uint4(quad[0], quad[1], quad[2], quad[3]);
    }
}

} // namespace

hipError_t launch_table_copy(hipStream_t s, const void* src, void* dst, uint32_t numUint4) {
    hipLaunchKernelGGL(k_table_copy, dim3((numUint4 + 255u) / 256u), dim3(256), 0, s, (const uint4*)src, (uint4*)dst, numUint4);
    return hipGetLastError();
}

hipError_t launch_scene_interpolants(hipStream_t s, const SceneInterpArgs& a, const SurfaceJob* table, bool waveForm) {
    const dim3 grid((uint32_t)((a.width + 15) / 16), (uint32_t)((a.height + 15) / 16));
    if (a.sv[0]) {
        if (waveForm) hipLaunchKernelGGL((k_scene_interpolants<true, true>), grid, dim3(kLanes), 0, s, a, table);
        else          hipLaunchKernelGGL((k_scene_interpolants<true, false>), grid, dim3(kLanes), 0, s, a, table);
    } else {
        if (waveForm) hipLaunchKernelGGL((k_scene_interpolants<false, true>), grid, dim3(kLanes), 0, s, a, table);
        else          hipLaunchKernelGGL((k_scene_interpolants<false, false>), grid, dim3(kLanes), 0, s, a, table);
    }
    return hipGetLastError();
}

hipError_t launch_scene_quad_interpolants(hipStream_t s, const SceneInterpArgs& a, const SurfaceJob* table, bool waveForm, const QuadPlane& quad) {
    const dim3 grid((uint32_t)((a.width + 15) / 16), (uint32_t)((a.height + 15) / 16));
    if (a.sv[0]) {
        if (waveForm) hipLaunchKernelGGL((k_scene_interpolants<true, true, QuadPlane>), grid, dim3(kLanes), 0, s, a, table, quad);
        else          hipLaunchKernelGGL((k_scene_interpolants<true, false, QuadPlane>), grid, dim3(kLanes), 0, s, a, table, quad);
    } else {
        if (waveForm) hipLaunchKernelGGL((k_scene_interpolants<false, true, QuadPlane>), grid, dim3(kLanes), 0, s, a, table, quad);
        else          hipLaunchKernelGGL((k_scene_interpolants<false, false, QuadPlane>), grid, dim3(kLanes), 0, s, a, table, quad);
    }
    return hipGetLastError();
}

} // namespace vqk
