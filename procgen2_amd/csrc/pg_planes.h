// From a frame to a tensor, a lane's share at a time: what the policy observations (pg_policy_obs.h), the frame history
// (pg_history.h) and the augmented gathers (pg_history_aug.h) have in common, each piece stated once.
//     a frame is the u8 [64][64][3] slab row the render kernels leave; a PLANE is one colour of it (C = 3: R, G, B) or its
//     gray (C = 1, policy_gray), 4096 bytes; a tensor row is [K*C][64][64] elements of ES = 1, 2 or 4 bytes, channel
//     slot*C + c, slot K-1 the newest frame.
// The VALUE of a byte is a table look-up: 256 output bit patterns per number format, made on the host
// (policy_table_entry), so a kernel knows the element size and nothing of the format.
// A workgroup is 256 lanes, and lane t owns the 16 consecutive pixels 16t .. 16t+15 of a frame: 48 bytes of the slab (three
// 16-byte loads: the slab is 16-byte aligned, 12 288 and 48 are multiples of 16), 16 bytes of a stored plane, 16·ES bytes
// of a tensor's channel.  A wave's 64 lanes so hold 1 024·ES consecutive bytes of a channel, cut into 64·ES UNITS of 16 bytes.
// Bounds are each kernel's own to state; the helpers here index the slab by (env, t), a table by a byte, and the exchange
// buffer of 256·ES units by wave·64·ES + 0 .. 64·ES - 1.
#pragma once

#include <type_traits>

#include "pg_defs.h"

namespace pg {

constexpr int kPolicyBlock = 256;        // lanes a workgroup = pixels of a frame / kPolicyLanePixels
constexpr int kPolicyLanePixels = 16;
constexpr int kPolicyPlane = kObsW * kObsH;  // elements a plane
constexpr int kPolicyMaxStack = 8;
static_assert(kPolicyBlock * kPolicyLanePixels == kPolicyPlane, "a lane per 16 pixels");

// include/procgen2_vec.h PGV_POLICY_*
constexpr int kPolicyU8 = 0, kPolicyF16 = 1, kPolicyBF16 = 2, kPolicyF32 = 3;
constexpr int kPolicyTables = 4;  // one table of 256 words per dtype

PG_HD bool policy_dtype_known(int dtype) { return dtype >= 0 && dtype < kPolicyTables; }
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

// f(ES, C) with the element bytes and the planes as compile-time constants (std::integral_constant): the launchers pick
// their kernel's instantiation through it.
template <class F>
inline void for_es_planes(int es, int planes, F&& f) {
    auto with_es = [&](auto c) {
        es == 1 ? f(std::integral_constant<int, 1>{}, c) : es == 2 ? f(std::integral_constant<int, 2>{}, c) : f(std::integral_constant<int, 4>{}, c);
    };
    planes == 1 ? with_es(std::integral_constant<int, 1>{}) : with_es(std::integral_constant<int, 3>{});
}

#if defined(__HIPCC__)
typedef uint32_t PolicyVec16 __attribute__((ext_vector_type(4)));  // 16 bytes a lane: one load or store instruction

// Lane tid's 48 bytes of env's slab row, as 12 words.
struct SlabWords { uint32_t word[12]; };
PG_D SlabWords slab_load(const uint8_t* obs, int env, int tid) {
    const PolicyVec16* from = reinterpret_cast<const PolicyVec16*>(obs + size_t(env) * kObsBytes + size_t(tid) * 48);
    const PolicyVec16 in0 = from[0], in1 = from[1], in2 = from[2];
    return SlabWords{{in0.x, in0.y, in0.z, in0.w, in1.x, in1.y, in1.z, in1.w, in2.x, in2.y, in2.z, in2.w}};
}
// Plane p's 16 bytes of those words (C = 1: their gray).  For unrolled callers: every byte position is then a constant.
template <int C>
PG_D void slab_plane_bytes(const SlabWords& s, int p, uint32_t (&v)[kPolicyLanePixels]) {
#pragma unroll
    for (int j = 0; j < kPolicyLanePixels; j++) {
        const int at = 3 * j;
        const uint32_t r = (s.word[at >> 2] >> (8 * (at & 3))) & 0xFFu, g = (s.word[(at + 1) >> 2] >> (8 * ((at + 1) & 3))) & 0xFFu,
                       b = (s.word[(at + 2) >> 2] >> (8 * ((at + 2) & 3))) & 0xFFu;
        v[j] = C == 1 ? policy_gray(r, g, b) : p == 0 ? r : p == 1 ? g : b;
    }
}
// 16 stored plane bytes → 16 table words.
PG_D void plane_values(const uint32_t* table, const PolicyVec16& in, uint32_t (&v)[kPolicyLanePixels]) {
#pragma unroll
    for (int i = 0; i < kPolicyLanePixels; i++) v[i] = table[(in[i >> 2] >> (8 * (i & 3))) & 0xFFu];
}

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

// The wave's exchange of one plane's units through its own quarter of `exchange` (LDS, 256·ES units): lane l's units
// l·ES + k out, units 64k + l in.  Two workgroup barriers, the second before the next plane overwrites the quarter: every
// call sits under a workgroup-uniform condition, so that they are met by all lanes or none.
template <int ES>
PG_D void wave_exchange(PolicyVec16* exchange, int wave, int lane, PolicyVec16 (&mine)[ES]) {
    PolicyVec16* share = exchange + wave * 64 * ES;
#pragma unroll
    for (int k = 0; k < ES; k++) share[lane * ES + k] = mine[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ES; k++) mine[k] = share[64 * k + lane];
    __syncthreads();
}

// A row of zero bytes: `channels` channels of `channel` bytes = `units` Units each; lane tid writes units tid, tid + 256, …
template <class Unit>
PG_D void zero_row(uint8_t* out, int channels, size_t channel, int units, int tid) {
    const Unit zero{};
    for (int ch = 0; ch < channels; ch++)
        for (int u = tid; u < units; u += kPolicyBlock) *reinterpret_cast<Unit*>(out + ch * channel + size_t(u) * sizeof(Unit)) = zero;
}
#endif

}  // namespace pg
