// Steps without frames (include/procgen2_vec.h pgv_step_sequence): T sub-steps in one call, of which at most the last is
// drawn.  A sub-step is the step's logic launches and nothing of its render path (engine.hip step_impl, frame = false);
// behind it one small launch, a lane per env, settles the sub-step's row: it copies the engine's own reward / done rows
// — which the logic kernels, and in chaser the level kernel on its own stream, have written by then — into row t of the
// caller's [T][N] buffers, and folds them into the env's summary by sequence_fold() below.  The engine's own rows stay
// where pgv_bind_outputs put them and are the last sub-step's without a copy.
// The summary's running values live in a block of the engine's own (SequenceBuffers: 9 bytes an env, allocated by
// pgv_make) so that any of the caller's three summary pointers may be NULL; the last sub-step writes the caller's.
// Plain vector loads and stores, no atomics, no cross-lane traffic.  Bounds: lane i < n; row t < T of buffers the caller
// sized [T][N].
#pragma once

#include "pg_carve.h"
#include "pg_defs.h"

namespace pg {

constexpr int kSequenceBlock = 256;

// The per-env rule.  Starting from {0.0f, 0, 0}: until the env's first done, every sub-step — one that serves a reset
// included — adds its reward (one float32 addition a sub-step, in step order) and one to the length; the sub-step that
// reports done is the last one counted.
struct SequenceFold {
    float ret;
    int32_t len;
    uint8_t done;
};
PG_HD SequenceFold sequence_fold(SequenceFold acc, float reward, uint8_t done) {
    if (acc.done) return acc;
    acc.ret = acc.ret + reward;
    acc.len = acc.len + 1;
    acc.done = done != 0;
    return acc;
}

// The engine's own block behind the running values (pg_carve.h).
struct SequenceBuffers {
    float* ret;     // [n]
    int32_t* len;   // [n]
    uint8_t* done;  // [n]
};
inline void list_sequence(Carve& c, SequenceBuffers& b, int n) {
    c.take(b.ret, size_t(n) * 4);
    c.take(b.len, size_t(n) * 4);
    c.take(b.done, size_t(n));
}

// One sub-step's row.
struct SequenceRow {
    int n;
    int first, last, fold;  // sub-step 0 / T - 1 of the call; the caller asked for a summary
    const float* reward;    // the engine's own rows (StepIO)
    const uint8_t* done;
    float* row_reward;      // rewards + t·N, dones + t·N, or nullptr
    uint8_t* row_done;
    SequenceBuffers acc;
    float* seq_return;      // the caller's, or nullptr
    int32_t* seq_length;
    uint8_t* seq_done;
};

#if defined(__HIPCC__)
__global__ void __launch_bounds__(kSequenceBlock) sequence_row_kernel(SequenceRow q) {
    const int i = static_cast<int>(blockIdx.x) * kSequenceBlock + static_cast<int>(threadIdx.x);
    if (i >= q.n) return;
    const float r = q.reward[i];
    const uint8_t d = q.done[i];
    if (q.row_reward) q.row_reward[i] = r;
    if (q.row_done) q.row_done[i] = d;
    if (!q.fold) return;
    SequenceFold acc{0.0f, 0, 0};
    if (!q.first) acc = SequenceFold{q.acc.ret[i], q.acc.len[i], q.acc.done[i]};
    acc = sequence_fold(acc, r, d);
    if (!q.last) {
        q.acc.ret[i] = acc.ret;
        q.acc.len[i] = acc.len;
        q.acc.done[i] = acc.done;
        return;
    }
    if (q.seq_return) q.seq_return[i] = acc.ret;
    if (q.seq_length) q.seq_length[i] = acc.len;
    if (q.seq_done) q.seq_done[i] = acc.done;
}

inline void launch_sequence_row(hipStream_t st, const SequenceRow& q) {
    hipLaunchKernelGGL(sequence_row_kernel, dim3((q.n + kSequenceBlock - 1) / kSequenceBlock), dim3(kSequenceBlock), 0, st, q);
}
#endif

}  // namespace pg
