// raster_ids.hip — vqhip_object_ids: the ObjectID pass's R32G32B32A32_SINT target (ObjectID.hlsl:PSMain) from the owner plane of the pass's own cull-NONE depth
// call (vqhip_scene_depth / vqhip_scene_masked_depth at one sample): a visibility-buffer resolve, as raster_attr.hip's, that needs no vertex at all.
// docs/DESIGN_DETAILS.md §7.21 P0 is the contract; tests/object_ids_ref.py states it in numpy.
//   k_object_ids : one lane per pixel, a wave = an 8 x 8 pixel block. Owner q -> draw (binary search of the table, bounded by the number of draws) -> instance ->
//                  (objID[instance].x, meshID, materialID, objID[instance].w); one int4 store per pixel. A pixel that owns nothing stores the clear colour.
// Every index is checked before it is used: q against the call's instanced triangles, the instance against the draw's count. Nothing an owner plane holds can
// move a load or a store out of bounds.
#include "vq_internal.h"

namespace vqk {
namespace {

constexpr int kLanes = 256;                       // four waves: a 16 x 16 pixel block

// P0 for the owner q (below the call's instanced triangles). Called with the lane's own q, or — from a wave whose 64 pixels share one owner — with that q as a
// wave-uniform value: the table entries and the objID row then have uniform addresses and travel through the scalar cache, one fetch per wave.
__device__ __forceinline__ int4 resolveIds(const ObjectIdArgs& a, const ObjectIdJob* __restrict__ table, uint32_t q) {
    int lo = 0, hi = a.numJobs - 1;               // the last job whose firstQ is <= q; numJobs >= 1 since totalTris > 0
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (table[mid].firstQ <= q) lo = mid; else hi = mid - 1; }
    const ObjectIdJob& J = table[lo];
    const uint32_t inst = (q - J.firstQ) / J.numTris;               // numTris >= 1: empty draws are not in the table
    if (inst >= J.numInstances) return make_int4(0, 0, 0, 0);       // holds by construction of firstQ; checked all the same
    const int32_t* id = J.objID + (size_t)inst * 4;
    return make_int4(id[0], J.meshID, J.materialID, id[3]);
}

template <bool WAVE>
__global__ void __launch_bounds__(kLanes) k_object_ids(ObjectIdArgs a, const ObjectIdJob* __restrict__ table) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), j = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (i >= a.width || j >= a.height) return;
    const uint32_t q = a.owner[(size_t)j * a.ownerPitch + i];
    int4 out = make_int4(0, 0, 0, 0);             // the pass's clear colour
    // q at or beyond the call's instanced triangles (0xFFFFFFFF included: the host refuses 2^29 or more) owns nothing
    const uint32_t q0 = __builtin_amdgcn_readfirstlane(q);
    if (WAVE && __builtin_amdgcn_ballot_w64(q != q0) == 0ull) {     // the wave's live lanes share one owner
        if (q0 < a.totalTris) out = resolveIds(a, table, q0);
    } else if (q < a.totalTris) {
        out = resolveIds(a, table, q);
    }
    ((int4*)a.ids)[(size_t)j * a.idsPitch + i] = out;
}

} // namespace

hipError_t launch_object_ids(hipStream_t s, const ObjectIdArgs& a, const ObjectIdJob* table, bool waveForm) {
    const dim3 grid((uint32_t)((a.width + 15) / 16), (uint32_t)((a.height + 15) / 16));
    if (waveForm) hipLaunchKernelGGL((k_object_ids<true>), grid, dim3(kLanes), 0, s, a, table);
    else          hipLaunchKernelGGL((k_object_ids<false>), grid, dim3(kLanes), 0, s, a, table);
    return hipGetLastError();
}

} // namespace vqk
