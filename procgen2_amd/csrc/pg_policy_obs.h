// Policy-ready observations on the device (include/procgen2_vec.h pgv_policy_obs_enable): the u8 [N][64][64][3] slab the
// render kernels leave, turned into what a policy network reads — planar, scaled, frame-stacked:
//     out [N][K*C][64][64], contiguous; C = 3 (planes R, G, B) or 1 (gray); slot 0 the oldest frame, slot K-1 the newest;
//     channel slot*C + c.
// The VALUE of a byte is a table look-up: 256 output bit patterns, made on the host when the feature is enabled
// (policy_table_entry), so the kernel knows the element size (1, 2 or 4 bytes) and nothing of the number format.
//
// The push kernel: one workgroup of 256 lanes per env.  Lane t owns the 16 consecutive pixels 16t .. 16t+15: it reads their
// 48 bytes as three 16-byte loads (the slab is 16-byte aligned, 12 288 and 48 are multiples of 16) and makes 16 values per
// plane, 16·ES bytes.  A wave's 64 lanes so hold 1 024·ES consecutive bytes of a plane, cut into 64·ES units of 16 bytes:
//   * dense form (the default): the wave exchanges the units through LDS, so that store instruction k (k < ES) of lane l
//     writes unit 64k + l — lanes 16 bytes apart, 1 KiB per instruction;
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
// The flag kernels: a lane per env (or per index) over restart u8[n]; an index outside 0 .. n-1 is skipped.
#pragma once

#include "pg_carve.h"
#include "pg_defs.h"

namespace pg {

constexpr int kPolicyBlock = 256;        // lanes a workgroup = pixels of a frame / kPolicyLanePixels
constexpr int kPolicyLanePixels = 16;
constexpr int kPolicyPlane = kObsW * kObsH;  // elements a plane
constexpr int kPolicyMaxStack = 8;
constexpr int kPolicyFlagBlock = 256;
static_assert(kPolicyBlock * kPolicyLanePixels == kPolicyPlane, "a lane per 16 pixels");

// include/procgen2_vec.h PGV_POLICY_*
constexpr int kPolicyU8 = 0, kPolicyF16 = 1, kPolicyBF16 = 2, kPolicyF32 = 3;

PG_HD int policy_element_bytes(int dtype) { return dtype == kPolicyU8 ? 1 : dtype == kPolicyF32 ? 4 : 2; }

PG_HD uint32_t policy_f32_bits(float f) {
    union { float f; uint32_t u; } x;
    x.f = f;
    return x.u;
}
// float32 → binary16, round to nearest even: for +0 and values whose half is normal (2^-14 <= x < 65 520) — the table's
// lie in {0} ∪ [1/255, 1].
PG_HD uint32_t policy_f16_of(uint32_t f32) {
    if (f32 == 0u) return 0u;
    const uint32_t r = f32 + 0xFFFu + ((f32 >> 13) & 1u);
    return ((r >> 13) - (112u << 10)) & 0xFFFFu;
}
// float32 → bfloat16, round to nearest even (finite values).
PG_HD uint32_t policy_bf16_of(uint32_t f32) { return (f32 + 0x7FFFu + ((f32 >> 16) & 1u)) >> 16; }

// The value rule: the output bit pattern of byte v, in the low policy_element_bytes(dtype) bytes of the word.
PG_HD uint32_t policy_table_entry(int dtype, uint32_t v) {
    if (dtype == kPolicyU8) return v;
    const uint32_t f32 = policy_f32_bits(static_cast<float>(v) / 255.0f);  // one correctly rounded IEEE division
    if (dtype == kPolicyF16) return policy_f16_of(f32);
    if (dtype == kPolicyBF16) return policy_bf16_of(f32);
    return f32;
}

// The gray rule, in integers: the weights sum to 256, so white stays 255.
PG_HD uint32_t policy_gray(uint32_t r, uint32_t g, uint32_t b) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; }

// Who owns what.  Unit u (16 bytes) of wave w's share of a plane: store k (k < ES) of lane l.
PG_HD int policy_unit(bool dense, int es, int lane, int k) { return dense ? 64 * k + lane : lane * es + k; }
// Byte offset, inside one env's block, of unit u of wave w in channel ch.
PG_HD size_t policy_unit_offset(int es, int ch, int wave, int unit) {
    return (size_t(ch) * kPolicyPlane + size_t(wave) * 1024) * size_t(es) + size_t(unit) * 16;
}
PG_HD size_t policy_bytes_per_env(int stack, int planes, int es) { return size_t(stack) * planes * kPolicyPlane * es; }

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
typedef uint32_t PolicyVec16 __attribute__((ext_vector_type(4)));  // 16 bytes a lane: one load or store instruction
// 16 table words → ES vectors of 16 bytes (the low ES bytes of each word, in pixel order).
template <int ES>
PG_D void policy_pack(const uint32_t (&v)[kPolicyLanePixels], PolicyVec16 (&to)[ES]) {
    uint32_t w[4 * ES];
    if (ES == 1) {
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] = v[4 * k] | (v[4 * k + 1] << 8) | (v[4 * k + 2] << 16) | (v[4 * k + 3] << 24);
    } else if (ES == 2) {
#pragma unroll
        for (int k = 0; k < 8; k++) w[k] = v[2 * k] | (v[2 * k + 1] << 16);
    } else {
#pragma unroll
        for (int k = 0; k < 16; k++) w[k] = v[k];
    }
#pragma unroll
    for (int k = 0; k < ES; k++) to[k] = PolicyVec16{w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]};
}

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
    const PolicyVec16* from = reinterpret_cast<const PolicyVec16*>(q.obs + size_t(env) * kObsBytes + size_t(tid) * 48);
    const PolicyVec16 in0 = from[0], in1 = from[1], in2 = from[2];
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
    const uint32_t word[12] = {in0.x, in0.y, in0.z, in0.w, in1.x, in1.y, in1.z, in1.w, in2.x, in2.y, in2.z, in2.w};
#pragma unroll
    for (int p = 0; p < C; p++) {  // (unrolled: every byte position is a constant)
        uint32_t v[kPolicyLanePixels];
#pragma unroll
        for (int j = 0; j < kPolicyLanePixels; j++) {
            const int at = 3 * j;
            const uint32_t r = (word[at >> 2] >> (8 * (at & 3))) & 0xFFu, g = (word[(at + 1) >> 2] >> (8 * ((at + 1) & 3))) & 0xFFu,
                           b = (word[(at + 2) >> 2] >> (8 * ((at + 2) & 3))) & 0xFFu;
            v[j] = table[C == 1 ? policy_gray(r, g, b) : p == 0 ? r : p == 1 ? g : b];
        }
        PolicyVec16 mine[ES];
        policy_pack<ES>(v, mine);
        if (ES > 1 && dense) {  // (workgroup-uniform)
            PolicyVec16* share = exchange + wave * 64 * ES;
#pragma unroll
            for (int k = 0; k < ES; k++) share[lane * ES + k] = mine[k];
            __syncthreads();
#pragma unroll
            for (int k = 0; k < ES; k++) mine[k] = share[64 * k + lane];
            __syncthreads();  // before the next plane overwrites the share
        }
        for (int s = restart ? 0 : K - 1; s < K; s++)
#pragma unroll
            for (int k = 0; k < ES; k++) *reinterpret_cast<PolicyVec16*>(out + policy_unit_offset(ES, s * C + p, wave, unit[k])) = mine[k];
    }
}

// restart[i] |= done[i]: the done row as a step finds it (an env whose row is set has its reset served by that step).
__global__ void __launch_bounds__(kPolicyFlagBlock) policy_flag_done_kernel(PolicyObsBuffers b, int n, const uint8_t* done) {
    const int i = static_cast<int>(blockIdx.x) * kPolicyFlagBlock + static_cast<int>(threadIdx.x);
    if (i < n && done[i]) b.restart[i] = 1;
}
// Set under a mask (nullptr = all).
__global__ void __launch_bounds__(kPolicyFlagBlock) policy_flag_mask_kernel(PolicyObsBuffers b, int n, const uint8_t* mask) {
    const int i = static_cast<int>(blockIdx.x) * kPolicyFlagBlock + static_cast<int>(threadIdx.x);
    if (i < n && (!mask || mask[i])) b.restart[i] = 1;
}
// Set over a list of indices, for the slots a load wrote: the load kernel's own tests (pg_records.h) — an index outside the
// batch is skipped, and so is a record whose first word is not `full`.
__global__ void __launch_bounds__(kPolicyFlagBlock) policy_flag_list_kernel(PolicyObsBuffers b, int n, const int32_t* indices, int count,
                                                                            const uint8_t* records, uint32_t record_bytes, uint32_t full) {
    const int k = static_cast<int>(blockIdx.x) * kPolicyFlagBlock + static_cast<int>(threadIdx.x);
    if (k >= count) return;
    const int env = indices ? indices[k] : k;
    if (env < 0 || env >= n) return;
    if (records && *reinterpret_cast<const uint32_t*>(records + size_t(k) * record_bytes) != full) return;
    b.restart[env] = 1;
}

inline void launch_policy_push(hipStream_t st, const PolicyPush& q, int es) {
    const dim3 grid(q.n), block(kPolicyBlock);
    void (*kernel)(PolicyPush) = nullptr;
    if (q.planes == 1)
        kernel = es == 1 ? policy_push_kernel<1, 1> : es == 2 ? policy_push_kernel<2, 1> : policy_push_kernel<4, 1>;
    else
        kernel = es == 1 ? policy_push_kernel<1, 3> : es == 2 ? policy_push_kernel<2, 3> : policy_push_kernel<4, 3>;
    hipLaunchKernelGGL(kernel, grid, block, 0, st, q);
}
inline dim3 policy_flag_grid(int count) { return dim3((count + kPolicyFlagBlock - 1) / kPolicyFlagBlock); }
inline void launch_policy_flag_done(hipStream_t st, const PolicyObsBuffers& b, int n, const uint8_t* done) {
    hipLaunchKernelGGL(policy_flag_done_kernel, policy_flag_grid(n), dim3(kPolicyFlagBlock), 0, st, b, n, done);
}
inline void launch_policy_flag_mask(hipStream_t st, const PolicyObsBuffers& b, int n, const uint8_t* mask) {
    hipLaunchKernelGGL(policy_flag_mask_kernel, policy_flag_grid(n), dim3(kPolicyFlagBlock), 0, st, b, n, mask);
}
inline void launch_policy_flag_list(hipStream_t st, const PolicyObsBuffers& b, int n, const int32_t* indices, int count, const uint8_t* records,
                                    uint32_t record_bytes, uint32_t full) {
    hipLaunchKernelGGL(policy_flag_list_kernel, policy_flag_grid(count), dim3(kPolicyFlagBlock), 0, st, b, n, indices, count, records, record_bytes, full);
}
#endif

}  // namespace pg
