// Level replay scores on the device (include/procgen2_vec.h pgv_level_scores_enable): which level every ring row was played
// on, and a table of per-level scores folded from a caller's per-step signal over a stretch of the transition ring.
//     level u32 [T][N], known u8 [T][N], laid out as `began` is: push p lives in slot p % T and holds pgv_level_numbers /
//     pgv_level_known as they stood where the push's frame was filed.  score f32, episodes u32, max_return f32, stamp int64
//     [K]: the table.  sum u64, steps u32, segments u32 [K] and totals u64 [2]: scratch, zero between calls.
// The rule is stated once below (level_score_fix, _accept, _live, _closes, _cell, _step, _files, _raises, _finish); the kernels and
// tests/cpp/test_level_scores.cpp share the text.  Signals are fixed point (16 fraction bits), so every sum is an exact
// integer and any order of the adds gives the sequential bits; a maximum is order-free as well.
//
// The words kernel: a lane per env, behind the history push of the same call, under the same mask.
// The update kernel: a workgroup of 256 lanes owns a tile of 64 consecutive envs and walks the stretch from the front in
// chunks of R = kLsRows rows; the ragged chunk, L % R rows, is the stretch's end.
//     A  all four waves.  Wave w takes rows w·R/4 .. of the chunk, lane = env: R/4 cells a lane, each flags, reward, level,
//        known and signal, and R/4 + 1 began bytes (the row's own says `whole`, the one behind it says CUT).  The loads of a
//        whole chunk are issued into registers first (level_score_load); then the cell is made — fix(signal), the table
//        index, one byte of verdicts — and goes to an LDS slab [R][64] (level_score_fill): 13 bytes a cell.
//     B  wave 0, lane = env: the chunk's rows in order out of LDS, the open segment (sum, steps, ret, index, verdicts) in
//        registers across chunks.  A close adds into the workgroup's table.
// Two slabs, one barrier a chunk: every wave issues the loads of chunk j + 1, wave 0 walks B of chunk j while they are in
// flight, every wave fills slab (j+1) & 1, BARRIER (B has left slab j & 1 before the fill of chunk j + 2 writes it; the
// cells of chunk j + 1 are visible).  So the load latency is paid once a chunk, under B.
// Where the closes go (template argument): K <= kLsLdsLevels — a table of the workgroup's own in LDS, 20 bytes a level
// (sum, steps, segments, max), LDS atomics, and one pass at the end that adds the entries with segments != 0 into global
// memory; above it, global atomics straight away.  Integer adds and a maximum: both give the same bytes.
// The finish kernel: a lane per level, level_score_finish where scratch steps > 0, the scratch it read cleared; lane 0 of
// block 0 hands the call's totals over and clears them.  No float atomics (the maximum is two integer ones on the float's
// bits), nothing allocated, no host synchronisation.
// Bounds.  Words: i < n, slot < T by the host, writes [slot·n + i] of both arrays.  Update: the grid is ceil(n / 64);
// env = blockIdx·64 + lane, every global access under env < n and local row < the chunk's rows.  t <= L - 1: flags, reward,
// level, known, began at [slot(first + t)·n + env] and began at [slot(first + t + 1)·n + env], both rows held by the
// host's check, so slot < T (one wrap a step); signal at [t·n + env] <= L·n - 1.  A table index is written only where
// level_score_accept said k < K; the LDS table is used only where K <= kLsLdsLevels and is indexed by that k or by j < K.
// LDS: two slabs of R·64·13 = 13 312 bytes, the table's 20 480 and 16 of totals: 47 120 bytes.  Finish: k < K.
#pragma once

#include "pg_transitions.h"

namespace pg {

// include/procgen2_vec.h PGV_SCORE_*
constexpr int kScoreAbs = 0, kScorePositive = 1;
constexpr int kLsMaxLevels = 1 << 24;  // K of the enable
constexpr uint32_t kLsMaskSeeded = 2u, kLsMaskCustom = 4u;  // known_mask: bit `level_known`

constexpr int kLsRows = 16;   // R: rows a chunk (procgen2_amd/lib.py LEVEL_SCORE_ROWS)
constexpr int kLsEnvs = 64;   // envs a workgroup: a wave a row (procgen2_amd/lib.py LEVEL_SCORE_ENVS)
constexpr int kLsBlock = 256;
constexpr int kLsLaneRows = kLsRows / (kLsBlock / kLsEnvs);  // cells a lane a chunk
constexpr int kLsLdsLevels = 1024;  // the largest K served by the workgroup's own table (procgen2_amd/lib.py LEVEL_SCORE_LDS_LEVELS)
// a cell's verdicts
constexpr uint8_t kLsLive = 1, kLsComplete = 2, kLsPartial = 4, kLsWhole = 8, kLsAccepted = 16;

// The caller's per-step quantity in fixed point, 16 fraction bits.
PG_HD uint32_t level_score_fix(int kind, float x) {
    const float v = kind == kScoreAbs ? fabsf(x) : (x > 0.0f ? x : 0.0f);
    const float t = v * 65536.0f;
    if (t != t) return 0u;
    if (t >= 2147483648.0f) return 2147483647u;
    return static_cast<uint32_t>(rintf(t));  // nearest-even
}
// May a segment opened on (level, known) be filed, and where.
PG_HD bool level_score_accept(uint32_t known_mask, uint32_t first_level, uint32_t levels, uint32_t level, uint8_t known, uint32_t& k) {
    k = level - first_level;  // (wrapping)
    return known < 32 && ((known_mask >> known) & 1u) != 0 && k < levels;
}
PG_HD bool level_score_live(uint8_t flags) { return (flags & kTrRecorded) != 0 && (flags & kTrVoid) == 0; }
// What closes behind a live row: 0 nothing, kLsComplete (TERMINATED or TRUNCATED) or kLsPartial (CUT).
PG_HD uint8_t level_score_closes(uint8_t flags, uint8_t began_next) {
    const uint8_t ends = transition_ends(flags, began_next);
    return ends == 0 ? uint8_t(0) : ends == kTrCut ? kLsPartial : kLsComplete;
}
// Everything about a row that no other row decides, one byte: live, what closes behind it, and — read only where the row
// opens a segment — `whole` and `accepted`.
PG_HD uint8_t level_score_cell(uint8_t flags, uint8_t began, uint8_t began_next, bool accepted) {
    if (!level_score_live(flags)) return 0;
    return uint8_t(kLsLive | level_score_closes(flags, began_next) | (began ? kLsWhole : 0) | (accepted ? kLsAccepted : 0));
}
// Is a closing segment added to the table (`opened`: the verdicts of the row that opened it), and may it raise max_return.
PG_HD bool level_score_files(uint8_t opened, bool complete, bool include_partial) { return (opened & kLsAccepted) != 0 && (complete || include_partial); }
PG_HD bool level_score_raises(uint8_t opened, bool complete, float ret) { return complete && (opened & kLsWhole) != 0 && ret == ret; }
// The table's row once the call's adds are in: every operation its own float32 rounding (the build forms no fused multiply-add).
PG_HD float level_score_finish(float score, uint32_t episodes, uint64_t sum, uint32_t steps, float alpha) {
    const float a = static_cast<float>(sum), b = static_cast<float>(steps);
    const float d = a / b;
    const float m = d * (1.0f / 65536.0f);
    if (episodes == 0) return m;
    const float keep = 1.0f - alpha;
    const float old = keep * score;
    const float fresh = alpha * m;
    return old + fresh;
}

// The walk of one env, a row at a time: the statement phase B of the kernel is.
struct LevelSegment {
    uint64_t sum;
    uint32_t steps, k;
    float ret;
    uint8_t opened;  // 0: nothing open; else the opening row's verdicts
};
// Takes row (cell, fix, reward, k); returns 0, or kLsComplete / kLsPartial when `seg` closed — it then still holds what closed.
PG_HD uint8_t level_score_step(LevelSegment& seg, bool& open, uint8_t cell, uint32_t fix, float reward, uint32_t k) {
    if ((cell & kLsLive) == 0) {
        const bool was = open;
        open = false;
        return was ? kLsPartial : uint8_t(0);
    }
    if (!open) {
        seg = LevelSegment{0, 0, k, 0.0f, cell};
        open = true;
    }
    seg.sum += fix;
    seg.steps += 1;
    seg.ret = seg.ret + reward;
    const uint8_t closes = cell & (kLsComplete | kLsPartial);
    if (closes) open = false;
    return closes;
}

struct LevelScoreBuffers {
    int capacity;  // T
    int levels;    // K
    uint32_t first_level, known_mask;
    uint32_t* level;       // [T][n]
    uint8_t* known;        // [T][n]
    float* score;          // [K]
    uint32_t* episodes;    // [K]
    float* max_return;     // [K]
    int64_t* stamp;        // [K]
    uint64_t* sum;         // [K] scratch
    uint32_t* steps;       // [K] scratch
    uint32_t* segments;    // [K] scratch
    uint64_t* totals;      // [2] scratch: segments and steps filed by the call
};
inline void list_level_scores(Carve& c, LevelScoreBuffers& b, int n) {
    const size_t rows = size_t(b.capacity) * size_t(n), K = size_t(b.levels);
    c.take(b.level, rows * 4);
    c.take(b.known, rows);
    c.take(b.score, K * 4);
    c.take(b.episodes, K * 4);
    c.take(b.max_return, K * 4);
    c.take(b.stamp, K * 8);
    c.take(b.sum, K * 8);
    c.take(b.steps, K * 4);
    c.take(b.segments, K * 4);
    c.take(b.totals, 16);
}

struct LevelWords {
    int n, slot;
    const uint8_t* mask;  // [n] or nullptr = all
    const uint32_t* number;  // the engine's level words (LevelPlan)
    const uint8_t* known;
    LevelScoreBuffers b;
};
struct LevelScoreUpdate {
    int n, length;
    int64_t first;
    int kind, include_partial;
    float alpha;
    int64_t stamp;
    const float* signal;
    uint64_t* totals;  // the caller's, or nullptr
    TransitionRing ring;
    LevelScoreBuffers b;
};

}  // namespace pg

#if defined(__HIPCC__)

namespace pg {

__global__ void __launch_bounds__(kTrBlock) level_words_kernel(LevelWords q) {
    const int i = static_cast<int>(blockIdx.x) * kTrBlock + static_cast<int>(threadIdx.x);
    if (i >= q.n || (q.mask && !q.mask[i])) return;
    const size_t at = history_began_offset(q.slot, q.n, i);
    q.b.level[at] = q.number[i];
    q.b.known[at] = q.known[i];
}

// The enable's launch behind its clear: the two columns that do not start as zero bytes.
__global__ void __launch_bounds__(kLsBlock) level_score_init_kernel(LevelScoreBuffers b) {
    const int k = static_cast<int>(blockIdx.x) * kLsBlock + static_cast<int>(threadIdx.x);
    if (k >= b.levels) return;
    b.max_return[k] = -__builtin_inff();
    b.stamp[k] = -1;
}

// *at = max(*at, v) for a float that is not NaN, by integer atomics on its bits: order-free, and the same word in LDS and in
// global memory.  A value >= 0 (-0 taken as +0) is raised as a signed integer — every negative float is a negative integer
// —, a value < 0 lowered as an unsigned one: among negative floats the larger has the smaller bits, and a word >= 0 is
// smaller than all of them.
__device__ __forceinline__ void level_score_raise(float* at, float v) {
    if (v >= 0.0f)
        atomicMax(reinterpret_cast<int*>(at), __float_as_int(v + 0.0f));
    else
        atomicMin(reinterpret_cast<unsigned int*>(at), __float_as_uint(v));
}

struct LevelScoreSlab {
    uint32_t fix[kLsRows][kLsEnvs], k[kLsRows][kLsEnvs];
    float reward[kLsRows][kLsEnvs];
    uint8_t cell[kLsRows][kLsEnvs];
};
template <int K>
struct LevelScoreTable {  // a workgroup's own, K = kLsLdsLevels (1: the kernel that does without)
    unsigned long long sum[K];
    uint32_t steps[K], segments[K];
    float max_return[K];
};
// A lane's cells of one chunk as loaded: rows row0 .. row0 + kLsLaneRows - 1 of the chunk, those below `rows` only.
struct LevelScoreLoads {
    uint8_t flags[kLsLaneRows], known[kLsLaneRows], began[kLsLaneRows + 1];
    uint32_t level[kLsLaneRows];
    float reward[kLsLaneRows], signal[kLsLaneRows];
};
__device__ __forceinline__ void level_score_load(const LevelScoreUpdate& q, int lo, int rows, int row0, int env, LevelScoreLoads& c) {
    if (row0 >= rows) return;  // (wave-uniform)
    const TransitionRing& g = q.ring;
    int slot = history_slot(q.first + lo + row0, g.capacity);
    c.began[0] = g.began[history_began_offset(slot, g.n, env)];
#pragma unroll
    for (int i = 0; i < kLsLaneRows; i++) {
        if (row0 + i >= rows) break;
        const int next = slot + 1 == g.capacity ? 0 : slot + 1;
        const size_t at = history_began_offset(slot, g.n, env);
        c.flags[i] = g.b.flags[at];
        c.reward[i] = g.b.reward[at];
        c.level[i] = q.b.level[at];
        c.known[i] = q.b.known[at];
        c.began[i + 1] = g.began[history_began_offset(next, g.n, env)];
        c.signal[i] = q.signal[size_t(lo + row0 + i) * size_t(q.n) + env];
        slot = next;
    }
}
__device__ __forceinline__ void level_score_fill(const LevelScoreUpdate& q, int rows, int row0, int lane, const LevelScoreLoads& c, LevelScoreSlab& s) {
#pragma unroll
    for (int i = 0; i < kLsLaneRows; i++) {
        const int r = row0 + i;
        if (r >= rows) break;
        uint32_t k;
        const bool accepted = level_score_accept(q.b.known_mask, q.b.first_level, uint32_t(q.b.levels), c.level[i], c.known[i], k);
        s.cell[r][lane] = level_score_cell(c.flags[i], c.began[i], c.began[i + 1], accepted);
        s.fix[r][lane] = level_score_fix(q.kind, c.signal[i]);
        s.k[r][lane] = k;
        s.reward[r][lane] = c.reward[i];
    }
}

template <bool kLds>
__global__ void __launch_bounds__(kLsBlock) level_score_update_kernel(LevelScoreUpdate q) {
    __shared__ LevelScoreSlab slab[2];
    __shared__ LevelScoreTable<kLds ? kLsLdsLevels : 1> table;
    __shared__ unsigned long long filed[2];  // the workgroup's segments and steps
    const int tid = static_cast<int>(threadIdx.x), lane = tid & (kLsEnvs - 1), wave = tid / kLsEnvs;
    const int env = static_cast<int>(blockIdx.x) * kLsEnvs + lane;
    const bool inside = env < q.n;
    const int L = q.length, chunks = (L + kLsRows - 1) / kLsRows, row0 = wave * kLsLaneRows;
    const int K = q.b.levels;
    if (tid < 2) filed[tid] = 0;
    if constexpr (kLds) {
        for (int k = tid; k < K; k += kLsBlock) {
            table.sum[k] = 0, table.steps[k] = 0, table.segments[k] = 0;
            table.max_return[k] = -__builtin_inff();
        }
    }
    LevelScoreLoads loads;
    if (inside) {
        const int rows = L < kLsRows ? L : kLsRows;
        level_score_load(q, 0, rows, row0, env, loads);
        level_score_fill(q, rows, row0, lane, loads, slab[0]);
    }
    __syncthreads();
    LevelSegment seg{0, 0, 0, 0.0f, 0};
    bool open = false;
    uint32_t my_segments = 0;
    unsigned long long my_steps = 0;
    auto close = [&](bool complete) {  // (wave 0; `seg` as level_score_step left it)
        if (!level_score_files(seg.opened, complete, q.include_partial != 0)) return;
        my_segments += 1, my_steps += seg.steps;
        if constexpr (kLds) {
            atomicAdd(&table.sum[seg.k], static_cast<unsigned long long>(seg.sum));
            atomicAdd(&table.steps[seg.k], seg.steps);
            atomicAdd(&table.segments[seg.k], 1u);
            if (level_score_raises(seg.opened, complete, seg.ret)) level_score_raise(&table.max_return[seg.k], seg.ret);
        } else {
            atomicAdd(reinterpret_cast<unsigned long long*>(&q.b.sum[seg.k]), static_cast<unsigned long long>(seg.sum));
            atomicAdd(&q.b.steps[seg.k], seg.steps);
            atomicAdd(&q.b.segments[seg.k], 1u);
            if (level_score_raises(seg.opened, complete, seg.ret)) level_score_raise(&q.b.max_return[seg.k], seg.ret);
        }
    };
    for (int j = 0; j < chunks; j++) {
        const int lo = j * kLsRows, rows = L - lo < kLsRows ? L - lo : kLsRows;
        const int next_lo = lo + kLsRows, next_rows = L - next_lo < kLsRows ? L - next_lo : kLsRows;  // chunk j + 1, where there is one
        const LevelScoreSlab& s = slab[j & 1];
        const bool more = inside && j + 1 < chunks;
        if (more) level_score_load(q, next_lo, next_rows, row0, env, loads);
        if (wave == 0 && inside) {  // phase B
#pragma unroll
            for (int r = 0; r < kLsRows; r++) {
                if (r < rows) {
                    const uint8_t closed = level_score_step(seg, open, s.cell[r][lane], s.fix[r][lane], s.reward[r][lane], s.k[r][lane]);
                    if (closed) close(closed == kLsComplete);
                }
            }
        }
        if (more) level_score_fill(q, next_rows, row0, lane, loads, slab[(j + 1) & 1]);
        __syncthreads();
    }
    if (wave == 0 && inside) {
        if (open) close(false);  // behind the last row: partial
        if (my_segments) atomicAdd(&filed[0], static_cast<unsigned long long>(my_segments)), atomicAdd(&filed[1], my_steps);
    }
    __syncthreads();
    if constexpr (kLds) {
        for (int k = tid; k < K; k += kLsBlock) {
            const uint32_t segments = table.segments[k];
            if (segments == 0) continue;
            atomicAdd(reinterpret_cast<unsigned long long*>(&q.b.sum[k]), table.sum[k]);
            atomicAdd(&q.b.steps[k], table.steps[k]);
            atomicAdd(&q.b.segments[k], segments);
            const float top = table.max_return[k];
            if (top != -__builtin_inff()) level_score_raise(&q.b.max_return[k], top);
        }
    }
    if (tid < 2 && filed[tid]) atomicAdd(reinterpret_cast<unsigned long long*>(&q.b.totals[tid]), filed[tid]);
}

__global__ void __launch_bounds__(kLsBlock) level_score_finish_kernel(LevelScoreUpdate q) {
    const int k = static_cast<int>(blockIdx.x) * kLsBlock + static_cast<int>(threadIdx.x);
    if (k < 2) {  // (K >= 1: block 0 exists)
        if (q.totals) q.totals[k] = q.b.totals[k];
        q.b.totals[k] = 0;
    }
    if (k >= q.b.levels) return;
    const uint32_t steps = q.b.steps[k];
    if (steps == 0) return;
    const uint32_t episodes = q.b.episodes[k];
    q.b.score[k] = level_score_finish(q.b.score[k], episodes, q.b.sum[k], steps, q.alpha);
    q.b.episodes[k] = episodes + q.b.segments[k];
    q.b.stamp[k] = q.stamp;
    q.b.sum[k] = 0, q.b.steps[k] = 0, q.b.segments[k] = 0;
}

inline void launch_level_words(hipStream_t st, const LevelWords& q) {
    hipLaunchKernelGGL(level_words_kernel, transition_grid(q.n), dim3(kTrBlock), 0, st, q);
}
inline void launch_level_score_init(hipStream_t st, const LevelScoreBuffers& b) {
    hipLaunchKernelGGL(level_score_init_kernel, dim3((b.levels + kLsBlock - 1) / kLsBlock), dim3(kLsBlock), 0, st, b);
}
// The two launches of an update.  `global_adds`: the closes go straight to global memory whatever K is (pgv_set_debug).
inline void launch_level_score_update(hipStream_t st, const LevelScoreUpdate& q, bool global_adds) {
    const dim3 grid((q.n + kLsEnvs - 1) / kLsEnvs);
    if (q.b.levels <= kLsLdsLevels && !global_adds)
        hipLaunchKernelGGL(level_score_update_kernel<true>, grid, dim3(kLsBlock), 0, st, q);
    else
        hipLaunchKernelGGL(level_score_update_kernel<false>, grid, dim3(kLsBlock), 0, st, q);
    hipLaunchKernelGGL(level_score_finish_kernel, dim3((q.b.levels + kLsBlock - 1) / kLsBlock), dim3(kLsBlock), 0, st, q);
}

}  // namespace pg
#endif
