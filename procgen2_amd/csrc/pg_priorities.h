// Prioritised sampling over the transition ring (include/procgen2_vec.h pgv_priorities_enable): the engine hands out the
// (push, env) pairs a replay learner reads, drawn in proportion to a fixed-point priority over exactly the rows that
// pgv_transitions_gather would call VALID.
//     priority u32 [T][N], laid out as the transitions' flags are: row q lives in slot q % T.  max u32 [1]: the running
//     maximum, what a new row is opened at.  chunk_sum u64 [chunks], chunk_count u32 [chunks], totals u64 [2] = {S, M}: the
//     sampler's scratch, chunks = ceil(T·N / 4096).
// Priorities are integers (fix(), 16 fraction bits), so every sum is exact and a parallel scan is the sequential one bit
// for bit; no tree is kept between calls: flags and priority are 5 bytes a row, and a scan on demand is one streaming read.
//
// The chunk kernel: a workgroup of 256 lanes per 4096 consecutive flat rows j = slot·N + env, 16 rows a lane — four
// dwordx4 loads of priority and one of flags —, slot and env carried along the run with a wrap at N; a wave reduction by
// shuffles, four partials through LDS, one sum and one count per chunk.
// The scan kernel: one workgroup turns the chunk sums into exclusive prefixes in place, 256 a pass (one a lane, a wave
// scan by shuffles, the waves' totals through LDS) with the total carried from pass to pass; it writes S and M.
// The sample kernel: a wavefront per sample, four to a workgroup.  Every lane computes target_k; the chunk is found by a
// 64-way search over the prefixes (a pivot a lane, a ballot narrows the range: about log64(chunks) rounds); the chunk is
// walked 64 rows a round, coalesced: a wave-inclusive scan of the weights, a ballot for the first lane whose running sum
// passes what is left of the target.  Every exit is wave-uniform; lane 0 stores with plain vector stores.
// The open kernel: a lane per env, behind the record kernel of the same call.  The set kernel: a lane per entry, one vector
// atomicMax on `max` — integer max is order-independent.  Nothing allocated, no host synchronisation.
// Bounds.  rows = T·N < 2^31 by the enable, so every flat index and every chunk number fits an int.  Chunk: the grid is
// `chunks`; a lane's run starts at j0 = chunk·4096 + tid·16 <= rows + 4095: where j0 + 16 <= rows the five vector loads read
// [j0, j0 + 16) of both arrays (priority and flags begin on 256-byte boundaries and j0 is a multiple of 16, so each is
// aligned), else each row is read alone and only where j < rows; writes [chunk] of the two chunk arrays.  Scan: reads and
// writes chunk_sum[c], reads chunk_count[c], only where c < chunks; totals[0 .. 1].  Sample: k = blockIdx·4 + wave < count
// or the wave leaves; a pivot is read only where it is < hi <= chunks; the walk reads row j = chunk·4096 + t·64 + lane, t <
// 64, only where j < rows; the outputs go to [k] of arrays of `count`, totals to [0 .. 1].  Fill (the enable's): j < rows.  Open: i < n, slot < T by the host.
// Set: entry < count; a row is written only where 0 <= env < n and the push is held with its successor, so its slot is
// push % T < T.
#pragma once

#include "pg_transitions.h"

namespace pg {

constexpr int kPrBlock = 256;                         // lanes a workgroup, every kernel here
constexpr int kPrLaneRows = 16;                       // rows a lane of the chunk kernel
constexpr int kPrChunk = kPrBlock * kPrLaneRows;      // 4096 rows a chunk
constexpr int kPrWaves = kPrBlock / 64;               // samples a workgroup
constexpr int kPrMaxCount = 1 << 20;                  // samples a call: k · (S % count) stays far below 2^64
constexpr uint32_t kPrOne = 65536u;                   // priority 1.0
constexpr uint32_t kPrTop = 2147483647u;

PG_HD int priority_chunks(int64_t rows) { return static_cast<int>((rows + kPrChunk - 1) / kPrChunk); }

// A caller's float32 priority in fixed point: NaN and everything below 2^-16 is the smallest weight, not zero — a row the
// caller named stays drawable.
PG_HD uint32_t priority_fix(float p) {
    const float t = p * 65536.0f;
    if (!(t >= 1.0f)) return 1u;
    if (t >= 2147483648.0f) return kPrTop;
    return static_cast<uint32_t>(rintf(t));  // nearest-even
}

// Which slots hold a row that is held with its successor, by head and T alone: the slots written so far but the newest
// push's (whose row is not made yet) — transition_held(row, head, T) for the row of slot s, without a division per slot.
struct PriorityWindow {
    int filled, newest;  // slots 0 .. filled-1 were written; `newest` is push head - 1's (-1: none)
};
PG_HD PriorityWindow priority_window(int64_t head, int capacity) {
    return {static_cast<int>(head < capacity ? head : capacity), head > 0 ? history_slot(head - 1, capacity) : -1};
}
PG_HD bool priority_slot_held(const PriorityWindow& w, int slot) { return slot < w.filled && slot != w.newest; }
// The row that lives in a held slot: the newest q < head with q % T = slot.
PG_HD int64_t priority_slot_row(int slot, int64_t head, int capacity) { return head - 1 - (head - 1 - slot) % capacity; }
// w(s, i) of a row's bytes.
PG_HD uint32_t priority_weight(bool held, uint8_t flags, uint32_t priority) { return transition_usable(held, flags) ? priority : 0u; }

// Sample k's target in [0, S), S > 0: 64-bit unsigned arithmetic throughout.
PG_HD uint64_t priority_target(uint64_t S, uint32_t count, uint32_t k, uint32_t seed, bool stratified) {
    const uint64_t word = mix32(mix32(seed + 0x9E3779B9u * (k + 1u)) ^ 0xC2B2AE35u);
    uint64_t lo = 0, width = S;
    if (stratified) {
        const uint64_t base = S / count, rem = S % count;
        lo = k * base + (k * rem) / count;
        width = (k + 1u) * base + ((k + 1u) * rem) / count - lo;
    }
    return lo + word * (width >> 32) + ((word * (width & 0xFFFFFFFFu)) >> 32);
}

struct PriorityBuffers {
    int capacity;
    uint32_t* priority;     // [T][n]
    uint32_t* max;          // [1]
    uint64_t* chunk_sum;    // [chunks]: the chunks' sums, then their exclusive prefixes
    uint32_t* chunk_count;  // [chunks]
    uint64_t* totals;       // [2]: S, M
};
inline void list_priorities(Carve& c, PriorityBuffers& b, int n) {
    const size_t rows = size_t(b.capacity) * size_t(n), chunks = size_t(priority_chunks(int64_t(rows)));
    c.take(b.priority, rows * 4);
    c.take(b.max, 4);
    c.take(b.chunk_sum, chunks * 8);
    c.take(b.chunk_count, chunks * 4);
    c.take(b.totals, 16);
}

// What the scan and the sample read of the two rings.
struct PriorityRing {
    int n, capacity;
    int64_t head;
    const uint8_t* flags;  // the transitions'
    PriorityBuffers b;
};
struct PriorityOpen {
    int n, slot;
    PriorityBuffers b;
};
struct PrioritySet {
    int n, count;
    int64_t head;
    const int64_t* pushes;
    const int32_t* envs;
    const float* values;
    PriorityBuffers b;
};
struct PrioritySample {
    PriorityRing ring;
    uint32_t count, seed;
    int stratified;
    int64_t* pushes;
    int32_t* envs;
    uint32_t* priority;
    float* prob;
    uint64_t* totals;
};

}  // namespace pg

#if defined(__HIPCC__)
#include "pg_engine.h"

namespace pg {

// A 64-bit value from another lane, as two 32-bit shuffles.
__device__ inline uint64_t priority_shfl(uint64_t v, int lane) {
    const uint32_t lo = __shfl(static_cast<uint32_t>(v), lane, 64), hi = __shfl(static_cast<uint32_t>(v >> 32), lane, 64);
    return (static_cast<uint64_t>(hi) << 32) | lo;
}
// The wave's inclusive prefix sums of v, lane order.
__device__ inline uint64_t priority_wave_scan(uint64_t v, int lane) {
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t below = priority_shfl(v, lane >= off ? lane - off : lane);
        if (lane >= off) v += below;
    }
    return v;
}

// The enable's one launch: every row, and the maximum, at 1.0 — rows recorded before it are drawable like new ones.
__global__ void __launch_bounds__(kPrBlock) priority_fill_kernel(PriorityBuffers b, int64_t rows) {
    const int64_t first = int64_t(blockIdx.x) * kPrBlock + threadIdx.x;
    if (first == 0) *b.max = kPrOne;
    for (int64_t j = first; j < rows; j += int64_t(gridDim.x) * kPrBlock) b.priority[j] = kPrOne;
}

__global__ void __launch_bounds__(kPrBlock) priority_open_kernel(PriorityOpen q) {
    const int i = static_cast<int>(blockIdx.x) * kPrBlock + static_cast<int>(threadIdx.x);
    if (i >= q.n) return;
    q.b.priority[history_began_offset(q.slot, q.n, i)] = *q.b.max;
}

__global__ void __launch_bounds__(kPrBlock) priority_set_kernel(PrioritySet q) {
    const int entry = static_cast<int>(blockIdx.x) * kPrBlock + static_cast<int>(threadIdx.x);
    if (entry >= q.count) return;
    const int64_t p = q.pushes[entry];
    const int env = q.envs[entry];
    if (env < 0 || env >= q.n || !transition_held(p, q.head, q.b.capacity)) return;
    const uint32_t v = priority_fix(q.values[entry]);
    q.b.priority[history_began_offset(history_slot(p, q.b.capacity), q.n, env)] = v;
    atomicMax(q.b.max, v);
}

__global__ void __launch_bounds__(kPrBlock) priority_chunk_kernel(PriorityRing q) {
    __shared__ uint64_t wave_sum[kPrWaves];
    __shared__ uint32_t wave_count[kPrWaves];
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63;
    const int64_t rows = int64_t(q.capacity) * q.n;
    const int64_t j0 = int64_t(blockIdx.x) * kPrChunk + int64_t(tid) * kPrLaneRows;
    uint32_t w[kPrLaneRows];
    uint8_t f[kPrLaneRows];
    if (j0 + kPrLaneRows <= rows) {
        const uint4* pv = reinterpret_cast<const uint4*>(q.b.priority + j0);
        for (int v = 0; v < 4; v++) {
            const uint4 x = pv[v];
            w[4 * v] = x.x, w[4 * v + 1] = x.y, w[4 * v + 2] = x.z, w[4 * v + 3] = x.w;
        }
        const uint4 fl = *reinterpret_cast<const uint4*>(q.flags + j0);
        const uint32_t words[4] = {fl.x, fl.y, fl.z, fl.w};
        for (int k = 0; k < kPrLaneRows; k++) f[k] = static_cast<uint8_t>(words[k >> 2] >> (8 * (k & 3)));
    } else {
        for (int k = 0; k < kPrLaneRows; k++) {
            const bool in = j0 + k < rows;
            w[k] = in ? q.b.priority[j0 + k] : 0u;
            f[k] = in ? q.flags[j0 + k] : uint8_t(0);  // (not recorded: no weight)
        }
    }
    const PriorityWindow win = priority_window(q.head, q.capacity);
    int slot = static_cast<int>(j0 / q.n), env = static_cast<int>(j0 % q.n);  // (one division a lane)
    bool held = priority_slot_held(win, slot);
    uint64_t sum = 0;
    uint32_t count = 0;
    for (int k = 0; k < kPrLaneRows; k++) {
        sum += priority_weight(held, f[k], w[k]);
        count += transition_usable(held, f[k]);
        if (++env == q.n) {
            env = 0;
            held = priority_slot_held(win, ++slot);  // (past the ring: not held)
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        sum += priority_shfl(sum, lane ^ off);
        count += __shfl(count, lane ^ off, 64);
    }
    if (lane == 0) wave_sum[tid >> 6] = sum, wave_count[tid >> 6] = count;
    __syncthreads();
    if (tid == 0) {
        q.b.chunk_sum[blockIdx.x] = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
        q.b.chunk_count[blockIdx.x] = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
    }
}

__global__ void __launch_bounds__(kPrBlock) priority_scan_kernel(PriorityBuffers b, int chunks) {
    __shared__ uint64_t wave_sum[kPrWaves];
    __shared__ uint32_t wave_count[kPrWaves];
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    uint64_t carry = 0;  // the total of the passes so far (the same in every lane)
    uint32_t count = 0;  // this lane's share of M
    for (int first = 0; first < chunks; first += kPrBlock) {  // (workgroup-uniform)
        const int c = first + tid;
        const uint64_t mine = c < chunks ? b.chunk_sum[c] : 0;
        count += c < chunks ? b.chunk_count[c] : 0u;
        const uint64_t upto = priority_wave_scan(mine, lane);
        __syncthreads();  // (the pass before has read wave_sum)
        if (lane == 63) wave_sum[wave] = upto;
        __syncthreads();
        uint64_t before = carry + upto - mine;
        for (int k = 0; k < wave; k++) before += wave_sum[k];
        if (c < chunks) b.chunk_sum[c] = before;
        carry += wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
    }
    for (int off = 32; off > 0; off >>= 1) count += __shfl(count, lane ^ off, 64);
    __syncthreads();
    if (lane == 0) wave_count[wave] = count;
    __syncthreads();
    if (tid == 0) {
        b.totals[0] = carry;
        b.totals[1] = uint64_t(wave_count[0]) + wave_count[1] + wave_count[2] + wave_count[3];
    }
}

__global__ void __launch_bounds__(kPrBlock) priority_sample_kernel(PrioritySample q) {
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const uint32_t k = blockIdx.x * kPrWaves + (threadIdx.x >> 6);
    if (k >= q.count) return;  // (wave-uniform, as every branch below that leaves or loops)
    const PriorityRing& g = q.ring;
    const uint64_t S = g.b.totals[0];
    if (k == 0 && lane == 0 && q.totals) q.totals[0] = S, q.totals[1] = g.b.totals[1];
    int64_t push = -1;
    int32_t env_out = -1;
    uint32_t weight = 0;
    if (S != 0) {
        const uint64_t target = priority_target(S, q.count, k, q.seed, q.stratified != 0);
        const int64_t rows = int64_t(g.capacity) * g.n;
        // the last chunk whose prefix is <= target: prefix[lo] <= target throughout, and prefix[hi] > target or hi = chunks
        int lo = 0, hi = priority_chunks(rows);
        while (hi - lo > 1) {
            const int step = (hi - lo + 63) / 64;
            const int64_t pivot = int64_t(lo) + int64_t(lane) * step;  // (lane 0's is lo: its answer is yes)
            const uint64_t yes = __ballot(pivot < hi && g.b.chunk_sum[pivot] <= target);  // (the prefixes do not fall: a run of ones)
            const int ones = __popcll(yes);
            hi = lo + ones * step < hi ? lo + ones * step : hi;
            lo = lo + (ones - 1) * step;
        }
        uint64_t left = target - g.b.chunk_sum[lo];  // < the chunk's sum
        const PriorityWindow win = priority_window(g.head, g.capacity);
        const int64_t j0 = int64_t(lo) * kPrChunk + lane;
        int slot = static_cast<int>(j0 / g.n), env = static_cast<int>(j0 % g.n);
        const int slots_round = 64 / g.n, envs_round = 64 % g.n;  // what 64 rows further means
        for (int t = 0; t < kPrChunk / 64; t++) {
            const int64_t j = j0 + t * 64;
            uint32_t w = 0;
            if (j < rows) w = priority_weight(priority_slot_held(win, slot), g.flags[j], g.b.priority[j]);
            const uint64_t upto = priority_wave_scan(w, lane);
            const uint64_t passed = __ballot(upto > left);
            if (passed) {
                const int at = __builtin_ctzll(passed);  // its weight is > 0: the lane below it has not passed
                push = priority_slot_row(__shfl(slot, at, 64), g.head, g.capacity);
                env_out = __shfl(env, at, 64);
                weight = __shfl(w, at, 64);
                break;
            }
            left -= priority_shfl(upto, 63);
            slot += slots_round, env += envs_round;
            if (env >= g.n) env -= g.n, slot++;
        }
    }
    if (lane != 0) return;
    if (q.pushes) q.pushes[k] = push;
    if (q.envs) q.envs[k] = env_out;
    if (q.priority) q.priority[k] = weight;
    if (q.prob) q.prob[k] = weight ? static_cast<float>(static_cast<uint64_t>(weight)) / static_cast<float>(S) : 0.0f;
}

inline dim3 priority_grid(int lanes) { return dim3((lanes + kPrBlock - 1) / kPrBlock); }
inline void launch_priority_fill(hipStream_t st, const PriorityBuffers& b, int n) {
    const int64_t rows = int64_t(b.capacity) * n;
    hipLaunchKernelGGL(priority_fill_kernel, dim3(priority_chunks(rows)), dim3(kPrBlock), 0, st, b, rows);
}
inline void launch_priority_open(hipStream_t st, const PriorityOpen& q) {
    hipLaunchKernelGGL(priority_open_kernel, priority_grid(q.n), dim3(kPrBlock), 0, st, q);
}
inline void launch_priority_set(hipStream_t st, const PrioritySet& q) {
    hipLaunchKernelGGL(priority_set_kernel, priority_grid(q.count), dim3(kPrBlock), 0, st, q);
}
// The three launches of a sample call.
inline void launch_priority_sample(hipStream_t st, const PrioritySample& q) {
    const int chunks = priority_chunks(int64_t(q.ring.capacity) * q.ring.n);
    hipLaunchKernelGGL(priority_chunk_kernel, dim3(chunks), dim3(kPrBlock), 0, st, q.ring);
    hipLaunchKernelGGL(priority_scan_kernel, dim3(1), dim3(kPrBlock), 0, st, q.ring.b, chunks);
    hipLaunchKernelGGL(priority_sample_kernel, dim3((q.count + kPrWaves - 1) / kPrWaves), dim3(kPrBlock), 0, st, q);
}

}  // namespace pg
#endif
