// Frame codes and visit counts over the frame ring (include/procgen2_vec.h pgv_frame_codes_enable): SimHash of stored frames —
// project a frame onto k directions, keep the signs, count the code — for count-based exploration bonuses.
//     w      int8 [k][D], D = C·4096 in the ring's plane order, k = 32 .. 256 in steps of 32; frame_code_weight unless the caller's
//     proj   int32 [B][k]: proj[b][j] = sum over d of w[j][d] · (frame_b[d] - 128), exact: |proj| <= 12 288 · 128 · 128 =
//            201 326 592 < 2^31.  A stored byte becomes the signed operand by ^ 0x80.
//     code   uint32 [B][k/32]: bit j % 32 of word j / 32 is proj[b][j] >= 0 (frame_code_word)
//     key    uint64, frame_code_key over the words and the row's salt, never 0: 0 marks an empty slot
//     table  keys uint64 [cap], visits uint32 [cap], cap a power of two; a key's slots are frame_code_slot(key, i, cap), i <
//            frame_code_probes(cap) = min(cap, 128); counters used, dropped uint32 [1]
// Entry b is the one stored frame (pushes[b], envs[b]), valid as a gather's entry is (pg_history.h) and with no walk; an entry
// that is not valid has valid = 0, zero proj and zero words, and never touches the table.
//
// frame_project_kernel<C, NB, RB>: a workgroup of 256 lanes owns a tile of 32·RB entries and all k = 32·NB columns; its four
// waves split D (split-K), wave w taking the 128-byte steps w, w + 4, ..., so a frame byte is fetched once a call.  The matrix
// instruction is v_mfma_i32_32x32x32_i8: operand A is 16 bytes of frame row (lane % 32) of a row block, operand B 16 bytes of
// weight row (lane % 32) of a column block, both at the same d, straight from global memory with dwordx4 loads — frames and
// weights are row-major in d, so nothing is rearranged in LDS.  The sum does not care in which order d is walked as long as
// both operands walk alike: in a step half-wave h = lane / 32 takes bytes [64h, 64h + 64) of the step's 128, four loads and
// four instructions, so two lanes cover a whole line of a row.  The next step's frame loads are issued before the current
// step's matrix instructions.  An invalid row loads nothing: its operand is zero.  The accumulators, 16·NB·RB registers, are
// D[i][j] with j = lane % 32 and i = 8·(v / 4) + 4·(lane / 32) + v % 4 for register v.
// The four waves' partial sums meet in LDS by integer atomic adds into one zeroed [32·RB][k] array (order-free, 32 KB a row
// block at k = 256) — not four arrays and a pass over them.  Then one pass, 64 consecutive columns a wave: proj is stored
// where asked for, a ballot of (valid and sum >= 0) gives two code words, kept in LDS and stored where asked for.  Then a
// lane per row: valid, the key from the row's words, and the count: `look` probes and stores the visits; `add` claims a slot
// by a 64-bit compare-and-swap on the key, adds 1 and stores the SLOT in visits_out, which frame_count_read_kernel, a second
// launch and a lane per entry, replaces by the slot's visits — the key's total behind the whole batch, whatever the order of
// the atomics.  The key so never leaves the kernel: there is no per-row key array to allocate.  No scratch memory.
// frame_weights_kernel, frame_table_clear_kernel: grid-stride, a lane per byte / per slot.
// Bounds.  Project: the grid is ceil(count / (32·RB)) workgroups; entry = tile·32·RB + row < count or nothing of the entry is
// read or stored; pushes[entry], envs[entry], salts[entry]; a frame is read only where the head's verdict holds (0 <= env < n,
// push held, so slot < T): bytes frame offset + d .. + 15 with d + 15 <= D - 1 < C·4096, the largest offset (T·n·C·4096) - 1 in
// size_t as in pg_history.h; weights at j·D + d .. + 15 with j < k: < k·D <= 3 145 728.  LDS: sum[row][col], row < 32·RB, col <
// k; words[row][word], word < NB.  proj[entry·k + col], codes[entry·NB + word], valid[entry], visits[entry], entry < count, in
// size_t.  Table: slot = (key + i) & (cap - 1) < cap, i < min(cap, 128): every loop is bounded by the probe limit.  Read: entry
// < count, slot < cap or the row reports 0.  Weights: idx < k·D.  Clear: slot < cap.
#pragma once

#include "pg_history.h"

#ifndef PG_FC_ROW_BLOCKS
#define PG_FC_ROW_BLOCKS 2  // 64 rows a tile up to 128 bits, 32 above; 1 = 32 rows always (docs/OPTLOG.md has both measured)
#endif

namespace pg {

constexpr int kFcBlock = 256;
constexpr int kFcRowBlocks = PG_FC_ROW_BLOCKS;
constexpr int kFcMinBits = 32, kFcMaxBits = 256, kFcMaxWords = kFcMaxBits / 32;
constexpr int kFcMinCapacity = 8, kFcMaxCapacity = 1 << 28, kFcMaxProbes = 128;
constexpr int kFcStep = 128;  // bytes of d a wave takes per step
constexpr int kFcCountNone = 0, kFcCountLook = 1, kFcCountAdd = 2;
constexpr uint32_t kFcNoSlot = 0xFFFFFFFFu;
constexpr int64_t kFcProjBound = int64_t(3 * kPolicyPlane) * 128 * 128;
static_assert(kFcProjBound == 201326592 && kFcProjBound < (int64_t(1) << 31), "the projection fits int32");

// Generated weights: +1 or -1 by one hash bit of (seed, direction, position).
PG_HD int8_t frame_code_weight(uint32_t seed, uint32_t j, uint32_t d) {
    return (mix32(mix32(seed ^ (j * 0x9E3779B9u)) + d) & 1u) ? int8_t(1) : int8_t(-1);
}
// A code word of 32 projections: bit i is proj[i] >= 0.
PG_HD uint32_t frame_code_word(const int32_t* proj) {
    uint32_t w = 0;
    for (int i = 0; i < 32; i++) w |= uint32_t(proj[i] >= 0) << i;
    return w;
}
PG_HD uint64_t frame_code_key_of(uint32_t hi, uint32_t lo) {
    const uint64_t key = uint64_t(hi) << 32 | lo;
    return key ? key : 1u;  // 0 marks an empty slot
}
// The table key of a code: two chains of mix32 over the words, both started from the salt; hi << 32 | lo, 0 mapped to 1.
PG_HD uint64_t frame_code_key(const uint32_t* words, int count, uint32_t salt) {
    uint32_t lo = mix32(salt + 0x9E3779B9u), hi = mix32(salt ^ 0x85EBCA6Bu);
    for (int i = 0; i < count; i++) {
        lo = mix32(lo ^ words[i]);
        hi = mix32(hi + (words[i] ^ 0xC2B2AE35u));
    }
    return frame_code_key_of(hi, lo);
}
PG_HD int frame_code_probes(int capacity) { return capacity < kFcMaxProbes ? capacity : kFcMaxProbes; }
PG_HD uint32_t frame_code_slot(uint64_t key, int i, int capacity) { return (uint32_t(key) + uint32_t(i)) & uint32_t(capacity - 1); }

// The engine's block behind the feature (pg_carve.h): the weights unless the caller brought them, and the table where asked for.
struct FrameCodeBuffers {
    int bits, capacity, planes, own_weights;
    int8_t* weights;   // [k][D]
    uint64_t* keys;    // [cap]
    uint32_t* visits;  // [cap]
    uint32_t* used;    // [1]
    uint32_t* dropped; // [1]
};
inline void list_frame_codes(Carve& c, FrameCodeBuffers& b, int) {
    if (b.own_weights) c.take(b.weights, size_t(b.bits) * size_t(b.planes) * kPolicyPlane);
    c.take(b.keys, size_t(b.capacity) * 8);
    c.take(b.visits, size_t(b.capacity) * 4);
    c.take(b.used, b.capacity ? 4 : 0);
    c.take(b.dropped, b.capacity ? 4 : 0);
}

struct FrameCodes {
    int n, count, count_mode;
    int64_t head;
    const int64_t* pushes;  // [count]
    const int32_t* envs;    // [count]
    const int32_t* salts;   // [count] or nullptr = 0
    int32_t* proj;          // [count][k] or nullptr
    uint32_t* codes;        // [count][k/32] or nullptr
    uint8_t* valid;         // [count] or nullptr
    uint32_t* visits;       // [count] or nullptr
    HistoryBuffers ring;
    FrameCodeBuffers b;
};

#if defined(__HIPCC__)
typedef int fc_v4i __attribute__((ext_vector_type(4)));
typedef int fc_v16i __attribute__((ext_vector_type(16)));

// The slot of `key`, claiming an empty one on the way; kFcNoSlot when the probes run out.  `used` counts the claims.
PG_D uint32_t frame_count_claim(const FrameCodeBuffers& b, uint64_t key) {
    const int probes = frame_code_probes(b.capacity);
    for (int i = 0; i < probes; i++) {
        const uint32_t slot = frame_code_slot(key, i, b.capacity);
        unsigned long long* const at = reinterpret_cast<unsigned long long*>(b.keys + slot);
        unsigned long long cur = __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            cur = atomicCAS(at, 0ull, static_cast<unsigned long long>(key));
            if (cur == 0) {
                atomicAdd(b.used, 1u);
                return slot;
            }
        }
        if (cur == key) return slot;
    }
    return kFcNoSlot;
}
// The slot of `key` where the table has it.  An empty slot ends the search: nothing is ever removed but by a clear.
PG_D uint32_t frame_count_find(const FrameCodeBuffers& b, uint64_t key) {
    const int probes = frame_code_probes(b.capacity);
    for (int i = 0; i < probes; i++) {
        const uint32_t slot = frame_code_slot(key, i, b.capacity);
        const uint64_t cur = b.keys[slot];
        if (cur == key) return slot;
        if (cur == 0) break;
    }
    return kFcNoSlot;
}

// A lane's 64 bytes of a frame row as four int8 operands (byte - 128), zero for a row that is not held.
PG_D void frame_code_load(const uint8_t* row, bool on, fc_v4i (&a)[4]) {
#pragma unroll
    for (int m = 0; m < 4; m++) {
        a[m] = on ? *reinterpret_cast<const fc_v4i*>(row + m * 16) : fc_v4i{0, 0, 0, 0};
        if (on) a[m] ^= fc_v4i{int(0x80808080u), int(0x80808080u), int(0x80808080u), int(0x80808080u)};  // byte - 128, as int8
    }
}

template <int C, int NB, int RB>  // planes; column blocks of 32 (k = 32·NB); row blocks of 32 a tile
__global__ void __launch_bounds__(kFcBlock) frame_project_kernel(FrameCodes q) {
    constexpr int kRows = 32 * RB, kCols = 32 * NB, kD = C * kPolicyPlane, kSteps = kD / kFcStep / 4;  // steps a wave
    __shared__ int32_t sum[kRows][kCols];
    __shared__ uint32_t words[kRows][NB];
    __shared__ size_t base[kRows];
    __shared__ uint8_t held[kRows];
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const size_t row0 = size_t(blockIdx.x) * kRows;
    if (tid < kRows) {
        const size_t entry = row0 + tid;
        int ok = 0;
        size_t at = 0;
        if (entry < size_t(q.count)) {
            const int env = q.envs[entry];
            const int64_t push = q.pushes[entry];
            ok = env >= 0 && env < q.n && history_held(push, q.head, q.ring.capacity);
            if (ok) at = history_frame_offset(history_slot(push, q.ring.capacity), q.n, env, C);
        }
        base[tid] = at, held[tid] = uint8_t(ok);
    }
    for (int i = tid; i < kRows * kCols; i += kFcBlock) (&sum[0][0])[i] = 0;
    __syncthreads();

    const uint8_t* frame[RB];
    bool on[RB];
#pragma unroll
    for (int rb = 0; rb < RB; rb++) {
        on[rb] = held[rb * 32 + r] != 0;
        frame[rb] = q.ring.frames + base[rb * 32 + r] + wave * kFcStep + h * 64;
    }
    const int8_t* const wrow = q.b.weights + size_t(r) * kD + wave * kFcStep + h * 64;
    fc_v16i acc[RB][NB];
#pragma unroll
    for (int rb = 0; rb < RB; rb++)
#pragma unroll
        for (int cb = 0; cb < NB; cb++)
#pragma unroll
            for (int v = 0; v < 16; v++) acc[rb][cb][v] = 0;
    fc_v4i a[RB][4], next[RB][4];
#pragma unroll
    for (int rb = 0; rb < RB; rb++) frame_code_load(frame[rb], on[rb], a[rb]);
    for (int s = 0; s < kSteps; s++) {
        const size_t d = size_t(s) * (4 * kFcStep);
        if (s + 1 < kSteps) {
#pragma unroll
            for (int rb = 0; rb < RB; rb++) frame_code_load(frame[rb] + d + 4 * kFcStep, on[rb], next[rb]);
        }
#pragma unroll
        for (int cb = 0; cb < NB; cb++) {
            fc_v4i b[4];
#pragma unroll
            for (int m = 0; m < 4; m++) b[m] = *reinterpret_cast<const fc_v4i*>(wrow + size_t(cb) * 32 * kD + d + m * 16);
#pragma unroll
            for (int m = 0; m < 4; m++)
#pragma unroll
                for (int rb = 0; rb < RB; rb++) acc[rb][cb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[rb][m], b[m], acc[rb][cb], 0, 0, 0);
        }
        if (s + 1 < kSteps) {
#pragma unroll
            for (int rb = 0; rb < RB; rb++)
#pragma unroll
                for (int m = 0; m < 4; m++) a[rb][m] = next[rb][m];
        }
    }
#pragma unroll
    for (int rb = 0; rb < RB; rb++)
#pragma unroll
        for (int cb = 0; cb < NB; cb++)
#pragma unroll
            for (int v = 0; v < 16; v++) atomicAdd(&sum[rb * 32 + 8 * (v / 4) + 4 * h + (v % 4)][cb * 32 + r], acc[rb][cb][v]);
    __syncthreads();

    for (int i = tid; i < kRows * kCols; i += kFcBlock) {  // (kRows·kCols is a multiple of 1024: every wave makes every round)
        const int row = i / kCols, col = i % kCols;
        const size_t entry = row0 + row;
        const int32_t v = sum[row][col];
        const unsigned long long signs = __ballot(held[row] != 0 && v >= 0);
        if (entry < size_t(q.count)) {
            if (q.proj) q.proj[entry * kCols + col] = v;
            if ((lane & 31) == 0) {
                const uint32_t word = uint32_t(signs >> (lane & 32));
                words[row][col / 32] = word;
                if (q.codes) q.codes[entry * NB + col / 32] = word;
            }
        }
    }
    __syncthreads();

    const size_t entry = row0 + tid;
    if (tid >= kRows || entry >= size_t(q.count)) return;
    const bool ok = held[tid] != 0;
    if (q.valid) q.valid[entry] = uint8_t(ok);
    if (q.count_mode == kFcCountNone) return;
    uint32_t out = q.count_mode == kFcCountAdd ? kFcNoSlot : 0u;
    if (ok) {
        const uint64_t key = frame_code_key(words[tid], NB, q.salts ? uint32_t(q.salts[entry]) : 0u);
        if (q.count_mode == kFcCountAdd) {
            out = frame_count_claim(q.b, key);
            if (out != kFcNoSlot) atomicAdd(q.b.visits + out, 1u);
            else atomicAdd(q.b.dropped, 1u);
        } else {
            const uint32_t slot = frame_count_find(q.b, key);
            out = slot != kFcNoSlot ? q.b.visits[slot] : 0u;
        }
    }
    if (q.visits) q.visits[entry] = out;
}

// Behind an `add`: visits_out holds each row's slot; the slot's visits take its place, 0 where the row has none.
__global__ void __launch_bounds__(kFcBlock) frame_count_read_kernel(FrameCodes q) {
    const size_t entry = size_t(blockIdx.x) * kFcBlock + threadIdx.x;
    if (entry >= size_t(q.count)) return;
    const uint32_t slot = q.visits[entry];
    q.visits[entry] = slot < uint32_t(q.b.capacity) ? q.b.visits[slot] : 0u;
}

__global__ void __launch_bounds__(kFcBlock) frame_weights_kernel(FrameCodeBuffers b, uint32_t seed) {
    const size_t D = size_t(b.planes) * kPolicyPlane, total = size_t(b.bits) * D;
    for (size_t i = size_t(blockIdx.x) * kFcBlock + threadIdx.x; i < total; i += size_t(gridDim.x) * kFcBlock)
        b.weights[i] = frame_code_weight(seed, uint32_t(i / D), uint32_t(i % D));
}

__global__ void __launch_bounds__(kFcBlock) frame_table_clear_kernel(FrameCodeBuffers b) {
    const size_t first = size_t(blockIdx.x) * kFcBlock + threadIdx.x;
    for (size_t i = first; i < size_t(b.capacity); i += size_t(gridDim.x) * kFcBlock) b.keys[i] = 0, b.visits[i] = 0;
    if (first == 0) *b.used = 0, *b.dropped = 0;
}

template <int C, int RB, int NB = 1>
inline void launch_frame_project(hipStream_t st, const FrameCodes& q) {
    if constexpr (NB <= kFcMaxWords) {
        if (q.b.bits != 32 * NB) return launch_frame_project<C, RB, NB + 1>(st, q);
        constexpr int rb = NB <= 4 ? RB : 1;  // 64 rows hold 16·NB·2 accumulators: up to 128 bits
        hipLaunchKernelGGL((frame_project_kernel<C, NB, rb>), dim3((q.count + 32 * rb - 1) / (32 * rb)), dim3(kFcBlock), 0, st, q);
    }
}
inline void launch_frame_table_clear(hipStream_t st, const FrameCodeBuffers& b) {
    const int blocks = b.capacity / kFcBlock < 4096 ? (b.capacity + kFcBlock - 1) / kFcBlock : 4096;
    hipLaunchKernelGGL(frame_table_clear_kernel, dim3(blocks), dim3(kFcBlock), 0, st, b);
}
inline void launch_frame_weights(hipStream_t st, const FrameCodeBuffers& b, uint32_t seed) {
    hipLaunchKernelGGL(frame_weights_kernel, dim3(1024), dim3(kFcBlock), 0, st, b, seed);
}
// A call: clear, project (with `look` or the adds inside), and behind an `add` whose visits are wanted the read.
inline void launch_frame_codes(hipStream_t st, const FrameCodes& q, bool clear) {
    if (clear) launch_frame_table_clear(st, q.b);
    if (q.count == 0) return;
    if (q.b.planes == 1) launch_frame_project<1, kFcRowBlocks>(st, q);
    else launch_frame_project<3, kFcRowBlocks>(st, q);
    if (q.count_mode == kFcCountAdd && q.visits)
        hipLaunchKernelGGL(frame_count_read_kernel, dim3((q.count + kFcBlock - 1) / kFcBlock), dim3(kFcBlock), 0, st, q);
}
#endif

}  // namespace pg
