// Policy-ready observations on the device (include/procgen2_vec.h pgv_policy_obs_enable): the u8 [N][64][64][3] slab the
// render kernels leave, turned into what a policy network reads — planar, scaled, frame-stacked:
//     out [N][K*C][64][64], contiguous; C = 3 (planes R, G, B) or 1 (gray); slot 0 the oldest frame, slot K-1 the newest;
//     channel slot*C + c.
// Values, the lane's share of a frame, units and the wave's exchange are pg_planes.h's.  What is this header's own:
//
// The push kernel: one workgroup of 256 lanes per env; a lane makes its 16 values per plane from the slab, 16·ES bytes.
//   * dense form (the default): the wave exchanges the units through LDS, so that store instruction k (k < ES) of lane l
//     writes unit 64k + l;
//   * strided form (pgv_set_debug bit 26, kept to be measured against: docs/OPTLOG.md): lane l stores its own units
//     l·ES + k — lanes 16·ES bytes apart.
// Either way policy_unit() maps (lane, k) to a unit, the same in every plane and every slot: a unit of the output has one
// owner.  The stack moves in place — slots 1 .. K-1 to 0 .. K-2, then the new frame into slot K-1 — by each lane loading
// every unit it owns of slot s+1 before it stores any into slot s, slot by slot upwards: the only lane that ever reads or
// writes a byte is its owner, in program order, so there is no cross-lane hazard and no barrier round the moves (the two
// barriers per plane fence the LDS exchange alone).  An env whose restart flag is set gets the new frame into all K slots
// and reads nothing of its stack; the flag is read by every lane in front of the first barrier and cleared by lane 0
// behind it.  An env whose mask byte is 0 is left before anything is read or written: no move, no flag change
// (workgroup-uniform, in front of the barriers).
// Plain vector loads and stores, no atomics.
// Bounds: the grid is n workgroups, env = blockIdx.x < n; a lane reads obs[env·12 288 + 48t .. + 47], t < 256; it writes
// channel ch < K·C, wave w < 4, unit u < 64·ES at  env·K·C·4096·ES + (ch·4096 + w·1024)·ES + 16u  <  (env + 1)·K·C·4096·ES.
// Offsets are size_t: 65 536 envs, K = 4, RGB, f32 are 12.9 GB.  The table has 256 words and is indexed by a byte.
// The flag kernels: a lane per env (or per index) over an array of flag bytes u8[n] — this feature's restart flags, the
// frame history's pending flags; an index outside 0 .. n-1 is skipped.
#pragma once

#include "pg_carve.h"
#include "pg_planes.h"

namespace pg {

constexpr int kPolicyFlagBlock = 256;

// The engine's own block behind the feature (pg_carve.h): the pending restart flags and the value table.
struct PolicyObsBuffers {
    uint8_t* restart;  // [n]
    uint32_t* table;   // [256]
};
inline void list_policy_obs(Carve& c, PolicyObsBuffers& b, int n) {
    c.take(b.restart, size_t(n));
    c.take(b.table, 256 * 4);
}

// One push.
struct PolicyPush {
    int n, stack, planes, dense;  // K; C = 3 or 1 (the gray rule); the store form
    const uint8_t* obs;           // the engine's slab (StepIO), 16-byte aligned
    uint8_t* out;                 // [n][K*C][64][64] elements, 16-byte aligned
    const uint8_t* mask;          // [n] or nullptr = all
    PolicyObsBuffers b;
};

#if defined(__HIPCC__)
template <int ES, int C>  // element bytes; planes
__global__ void __launch_bounds__(kPolicyBlock) policy_push_kernel(PolicyPush q) {
    __shared__ uint32_t table[256];
    __shared__ PolicyVec16 exchange[ES > 1 ? kPolicyBlock * ES : 1];  // a wave's units of one plane, in the wave's own quarter
    const int env = static_cast<int>(blockIdx.x);
    if (q.mask && !q.mask[env]) return;  // (workgroup-uniform)
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const bool dense = q.dense != 0;
    table[tid] = q.b.table[tid];
    const bool restart = q.b.restart[env] != 0;
    const SlabWords slab = slab_load(q.obs, env, tid);
    __syncthreads();  // the table is whole; every lane has read the flag
    if (tid == 0 && restart) q.b.restart[env] = 0;

    const int K = q.stack;
    uint8_t* const out = q.out + size_t(env) * policy_bytes_per_env(K, C, ES);
    int unit[ES];
#pragma unroll
    for (int k = 0; k < ES; k++) unit[k] = policy_unit(dense, ES, lane, k);
    if (!restart) {  // the stack moves down one slot
        for (int s = 0; s + 1 < K; s++) {
            PolicyVec16 held[C * ES];
#pragma unroll
            for (int p = 0; p < C; p++)
#pragma unroll
                for (int k = 0; k < ES; k++)
                    held[p * ES + k] = *reinterpret_cast<const PolicyVec16*>(out + policy_unit_offset(ES, (s + 1) * C + p, wave, unit[k]));
#pragma unroll
            for (int p = 0; p < C; p++)
#pragma unroll
                for (int k = 0; k < ES; k++)
                    *reinterpret_cast<PolicyVec16*>(out + policy_unit_offset(ES, s * C + p, wave, unit[k])) = held[p * ES + k];
        }
    }
#pragma unroll
    for (int p = 0; p < C; p++) {
        uint32_t v[kPolicyLanePixels];
        slab_plane_bytes<C>(slab, p, v);
#pragma unroll
        for (int j = 0; j < kPolicyLanePixels; j++) v[j] = table[v[j]];
        PolicyVec16 mine[ES];
        policy_pack<ES>(v, mine);
        if (ES > 1 && dense) wave_exchange<ES>(exchange, wave, lane, mine);  // (workgroup-uniform)
        for (int s = restart ? 0 : K - 1; s < K; s++)
#pragma unroll
            for (int k = 0; k < ES; k++) *reinterpret_cast<PolicyVec16*>(out + policy_unit_offset(ES, s * C + p, wave, unit[k])) = mine[k];
    }
}

// flags[i] |= done[i]: the done row as a step finds it (an env whose row is set has its reset served by that step).
__global__ void __launch_bounds__(kPolicyFlagBlock) policy_flag_done_kernel(uint8_t* flags, int n, const uint8_t* done) {
    const int i = static_cast<int>(blockIdx.x) * kPolicyFlagBlock + static_cast<int>(threadIdx.x);
    if (i < n && done[i]) flags[i] = 1;
}
// Set under a mask (nullptr = all).
__global__ void __launch_bounds__(kPolicyFlagBlock) policy_flag_mask_kernel(uint8_t* flags, int n, const uint8_t* mask) {
    const int i = static_cast<int>(blockIdx.x) * kPolicyFlagBlock + static_cast<int>(threadIdx.x);
    if (i < n && (!mask || mask[i])) flags[i] = 1;
}
// Set over a list of indices, for the slots a load wrote: the load kernel's own tests (pg_records.h) — an index outside the
// batch is skipped, and so is a record whose first word is not `full`.
__global__ void __launch_bounds__(kPolicyFlagBlock) policy_flag_list_kernel(uint8_t* flags, int n, const int32_t* indices, int count,
                                                                            const uint8_t* records, uint32_t record_bytes, uint32_t full) {
    const int k = static_cast<int>(blockIdx.x) * kPolicyFlagBlock + static_cast<int>(threadIdx.x);
    if (k >= count) return;
    const int env = indices ? indices[k] : k;
    if (env < 0 || env >= n) return;
    if (records && *reinterpret_cast<const uint32_t*>(records + size_t(k) * record_bytes) != full) return;
    flags[env] = 1;
}

inline void launch_policy_push(hipStream_t st, const PolicyPush& q, int es) {
    const dim3 grid(q.n), block(kPolicyBlock);
    for_es_planes(es, q.planes, [&](auto es_c, auto planes_c) {
        hipLaunchKernelGGL((policy_push_kernel<decltype(es_c)::value, decltype(planes_c)::value>), grid, block, 0, st, q);
    });
}
inline dim3 policy_flag_grid(int count) { return dim3((count + kPolicyFlagBlock - 1) / kPolicyFlagBlock); }
inline void launch_policy_flag_done(hipStream_t st, uint8_t* flags, int n, const uint8_t* done) {
    hipLaunchKernelGGL(policy_flag_done_kernel, policy_flag_grid(n), dim3(kPolicyFlagBlock), 0, st, flags, n, done);
}
inline void launch_policy_flag_mask(hipStream_t st, uint8_t* flags, int n, const uint8_t* mask) {
    hipLaunchKernelGGL(policy_flag_mask_kernel, policy_flag_grid(n), dim3(kPolicyFlagBlock), 0, st, flags, n, mask);
}
inline void launch_policy_flag_list(hipStream_t st, uint8_t* flags, int n, const int32_t* indices, int count, const uint8_t* records,
                                    uint32_t record_bytes, uint32_t full) {
    hipLaunchKernelGGL(policy_flag_list_kernel, policy_flag_grid(count), dim3(kPolicyFlagBlock), 0, st, flags, n, indices, count, records, record_bytes, full);
}
#endif

}  // namespace pg
