// Transitions on the device (include/procgen2_vec.h pgv_transitions_enable): the other half of a rollout beside the frame
// history (pg_history.h) — a ring of what every call did, and the two folds a learner makes of it:
//     action int32 [T][N], reward f32 [T][N], flags u8 [T][N]; row q lives in slot q % T and describes the call that made
//     push q + 1: the action taken on frame q, what it earned, how it ended.  pending [N]: "this step found the env's done
//     row set" (VOID), filed by the flag kernel in front of the step and consumed by the row's write.
// Row q is COMPLETE when pushes q and q + 1 are both held and RECORDED is set; CUT when it is complete, none of TERMINATED,
// TRUNCATED, VOID is set and began[q + 1][env] is: somebody outside ended the episode (a reset, a load, new levels).
//
// The record kernel: a lane per env, in front of the history push of the same call.  Plain loads and stores.
// The gather kernel: a workgroup of 256 lanes per (entry, which of the two rows).  Lane k < 64 of wave 0 loads row p + k's
// flags, reward and the began byte behind it, side by side; two ballots find where the walk stops; the fold then runs in
// row order over the lanes' rewards (every lane of the wave computes it, lane 0 stores it).  The frame part is the plain
// gather's: gather_entry_at, gather_row (pg_history.h) with the push p, or p + steps.
// The GAE kernel: a lane per env walks t = L-1 .. 0; the rows of one t are coalesced across envs.
// No atomics, nothing allocated, no host synchronisation.
// Bounds.  Record: i = blockIdx·256 + tid < n; slot < T by the host (or < 0: only the pending byte is cleared); writes
// [slot·n + i] of the three arrays and pending[i].  Gather: the grid is (count, 1 or 2); pushes[entry], envs[entry]; a ring
// byte is read only where 0 <= env < n and 0 <= p < head and row p + k is held with the push behind it (p + k <= head + 63:
// no overflow), so every slot is (p + k) % T and (p + k + 1) % T < T; the scalars go to [entry] of arrays of `count`; a row
// to entry·K·C·4096·ES .. as gather_row states.  GAE: i < n; t < L; row first + t is held with its successor by the host's
// check, so its slots are < T; values[(t + 1)·n + i] with t + 1 <= L: the array has L + 1 rows.
#pragma once

#include "pg_history.h"

namespace pg {

// include/procgen2_vec.h PGV_TR_*
constexpr uint8_t kTrRecorded = 1, kTrTerminated = 2, kTrTruncated = 4, kTrVoid = 8, kTrCut = 16;
constexpr uint8_t kTrValid = 1;  // bit 0 of a gathered status
constexpr int kTrMaxSteps = 64;  // n of a gather: one row a lane of a wave
constexpr int kTrBlock = 256;    // envs a workgroup (record, GAE)

// Row q with its successor frame: pushes q and q + 1 both held.
PG_HD bool transition_held(int64_t q, int64_t head, int capacity) { return history_held(q, head, capacity) && q + 1 < head; }
// A held row's bytes → may the walk take it (complete and not VOID), and what ends behind it (TERMINATED | TRUNCATED | CUT).
PG_HD bool transition_usable(bool held, uint8_t flags) { return held && (flags & kTrRecorded) != 0 && (flags & kTrVoid) == 0; }
PG_HD uint8_t transition_ends(uint8_t flags, uint8_t began_next) {
    const uint8_t own = flags & (kTrTerminated | kTrTruncated);
    return (own == 0 && (flags & kTrVoid) == 0 && began_next != 0) ? kTrCut : own;
}
// One row of the n-step fold: three float32 roundings, in this order (the build forms no fused multiply-add).
PG_HD void transition_fold(float& ret, float& disc, float reward, float gamma) {
    const float t = disc * reward;
    ret = ret + t;
    disc = disc * gamma;
}

struct TransitionBuffers {
    int capacity;
    uint8_t* pending;  // [n]
    uint8_t* flags;    // [T][n]
    int32_t* action;   // [T][n]
    float* reward;     // [T][n]
};
inline void list_transitions(Carve& c, TransitionBuffers& b, int n) {
    const size_t rows = size_t(b.capacity) * size_t(n);
    c.take(b.pending, size_t(n));
    c.take(b.flags, rows);
    c.take(b.action, rows * 4);
    c.take(b.reward, rows * 4);
}

// What the walk reads, and what it gives.
struct TransitionRing {
    int n, capacity;
    int64_t head;
    const uint8_t* began;  // the history's
    TransitionBuffers b;
};
struct TransitionResult {
    int32_t action, steps;
    float ret, discount;
    uint8_t status;
};
// What the walk leaves once it stopped behind `steps` rows, the last of which ended `ends`; steps = 0: an invalid entry.
PG_HD TransitionResult transition_result(int32_t action, int steps, float ret, float disc, uint8_t ends) {
    if (steps == 0) return TransitionResult{0, 0, 0.0f, 0.0f, 0};
    return TransitionResult{action, steps, ret, (ends & kTrTerminated) ? 0.0f : disc, uint8_t(kTrValid | ends)};
}
// The walk of entry (p, env), row after row: the statement the gather kernel's lanes are held to (tests/cpp/test_transitions.cpp).
PG_HD TransitionResult transition_walk(const TransitionRing& g, int64_t p, int env, int n, float gamma) {
    if (env < 0 || env >= g.n || p < 0 || p >= g.head) return transition_result(0, 0, 0.0f, 1.0f, 0);
    int m = 0;
    float ret = 0.0f, disc = 1.0f;
    uint8_t ends = 0;
    for (int k = 0; k < n; k++) {
        const int64_t q = p + k;
        const bool held = transition_held(q, g.head, g.capacity);
        const size_t at = held ? history_began_offset(history_slot(q, g.capacity), g.n, env) : 0;
        const uint8_t flags = held ? g.b.flags[at] : uint8_t(0);
        if (!transition_usable(held, flags)) break;
        transition_fold(ret, disc, g.b.reward[at], gamma);
        m++;
        ends = transition_ends(flags, g.began[history_began_offset(history_slot(q + 1, g.capacity), g.n, env)]);
        if (ends) break;
    }
    const int32_t action = m ? g.b.action[history_began_offset(history_slot(p, g.capacity), g.n, env)] : 0;
    return transition_result(action, m, ret, disc, ends);
}

// One row of the GAE recurrence, t = L-1 .. 0, `carry` the advantage of row t + 1 (0 behind the stretch).  c = gamma * lambda,
// computed once by the caller.  Every product and sum is its own float32 rounding.
struct GaeStep {
    float adv, ret;
};
PG_HD GaeStep gae_step(uint8_t flags, uint8_t began_next, float reward, float v, float v_next, float v_trunc, float gamma, float c, float carry) {
    if ((flags & kTrRecorded) == 0 || (flags & kTrVoid) != 0) return GaeStep{0.0f, v};
    const uint8_t ends = transition_ends(flags, began_next);
    const float nv = ends == 0 ? v_next : ends == kTrTruncated ? v_trunc : 0.0f;  // (TERMINATED wins where both are set)
    const float a = gamma * nv;
    const float b = reward + a;
    const float delta = b - v;
    float adv = delta;
    if (ends == 0) {
        const float d = c * carry;
        adv = delta + d;
    }
    return GaeStep{adv, adv + v};
}

struct TransitionRecord {
    int n, slot;   // slot < 0: no row to write, the pending bytes are cleared all the same
    int recorded;  // 0: the row is flags = 0 (a push that no single step made)
    uint32_t run_seed, step_index, env_offset;  // the synthetic action, where `actions` is nullptr
    const int32_t* actions;
    const float* reward;
    const uint8_t* terminated;  // the done row, or the episode outputs' terminated
    const uint8_t* truncated;   // nullptr: never
    TransitionBuffers b;
};

struct TransitionGather {
    HistoryGather g;  // out: unused — the two rows below
    int steps;        // n, 1 .. 64
    float gamma;
    TransitionRing ring;
    uint8_t *obs, *next_obs;
    int32_t* action;
    float* nstep_return;
    float* discount;
    int32_t* step_count;
    uint8_t* status;
};

struct TransitionGae {
    int n, length;
    int64_t first;
    float gamma, lambda;
    const float *values, *trunc_values;
    float *advantages, *returns;
    TransitionRing ring;
};

}  // namespace pg

#if defined(__HIPCC__)
#include "pg_engine.h"

namespace pg {

__global__ void __launch_bounds__(kTrBlock) transition_record_kernel(TransitionRecord q) {
    const int i = static_cast<int>(blockIdx.x) * kTrBlock + static_cast<int>(threadIdx.x);
    if (i >= q.n) return;
    const uint8_t found_done = q.b.pending[i];
    q.b.pending[i] = 0;
    if (q.slot < 0) return;
    const size_t at = history_began_offset(q.slot, q.n, i);
    int32_t action = 0;
    float reward = 0.0f;
    uint8_t flags = 0;
    if (q.recorded) {
        action = q.actions ? q.actions[i] : synthetic_action(q.run_seed, q.step_index, q.env_offset + uint32_t(i));
        reward = q.reward[i];
        flags = kTrRecorded;
        if (q.terminated[i]) flags |= kTrTerminated;
        if (q.truncated && q.truncated[i]) flags |= kTrTruncated;
        if (found_done) flags |= kTrVoid;
    }
    q.b.action[at] = action;
    q.b.reward[at] = reward;
    q.b.flags[at] = flags;
}

template <int ES, int C>
__global__ void __launch_bounds__(kHistoryBlock) transition_gather_kernel(TransitionGather q) {
    __shared__ uint32_t table[256];
    __shared__ int64_t frame[kPolicyMaxStack];
    __shared__ int valid;
    __shared__ int walked;  // steps, 0 = an invalid entry
    __shared__ PolicyVec16 exchange[ES > 1 ? kHistoryBlock * ES : 1];
    const int tid = static_cast<int>(threadIdx.x);
    const size_t entry = blockIdx.x;
    const int which = static_cast<int>(blockIdx.y);  // 0: the scalars and obs; 1: next_obs
    const int64_t p = q.g.pushes[entry];
    const int env = q.g.envs[entry];
    if (tid < 64) {  // (wave 0, whole)
        const TransitionRing& g = q.ring;
        const bool inside = env >= 0 && env < g.n && p >= 0 && p < g.head;  // (wave-uniform)
        const int64_t row = inside ? p + tid : 0;
        const bool held = inside && tid < q.steps && transition_held(row, g.head, g.capacity);
        uint8_t flags = 0, began_next = 0;
        float reward = 0.0f;
        if (held) {
            const size_t at = history_began_offset(history_slot(row, g.capacity), g.n, env);
            flags = g.b.flags[at];
            reward = g.b.reward[at];
            began_next = g.began[history_began_offset(history_slot(row + 1, g.capacity), g.n, env)];
        }
        const bool usable = transition_usable(held, flags);  // (false from lane n on)
        const int ends = usable ? transition_ends(flags, began_next) : 0;
        const uint64_t stop_before = __ballot(!usable), stop_behind = __ballot(ends != 0);
        const int first_bad = stop_before ? __builtin_ctzll(stop_before) : 64;
        const int first_end = stop_behind ? __builtin_ctzll(stop_behind) : 64;
        const int m = first_end < first_bad ? first_end + 1 : first_bad;  // <= n
        float ret = 0.0f, disc = 1.0f;
        for (int k = 0; k < m; k++) transition_fold(ret, disc, __shfl(reward, k, 64), q.gamma);  // (m is wave-uniform)
        const int last_ends = __shfl(ends, m > 0 ? m - 1 : 0, 64);
        if (tid == 0) {
            walked = m;
            if (which == 0) {
                const int32_t action = m ? g.b.action[history_began_offset(history_slot(p, g.capacity), g.n, env)] : 0;
                const TransitionResult r = transition_result(action, m, ret, disc, m ? uint8_t(last_ends) : uint8_t(0));
                if (q.action) q.action[entry] = r.action;
                if (q.nstep_return) q.nstep_return[entry] = r.ret;
                if (q.discount) q.discount[entry] = r.discount;
                if (q.step_count) q.step_count[entry] = r.steps;
                if (q.status) q.status[entry] = r.status;
            }
        }
    }
    uint8_t* const rows = which == 0 ? q.obs : q.next_obs;
    if (!rows) return;  // (workgroup-uniform)
    __syncthreads();
    const int m = walked;
    // a valid entry's two pushes are held: p by row p, p + m by row p + m - 1; an invalid one gets the zero row through env = -1
    const bool ok = gather_entry_at(q.g, which == 0 ? p : p + m, m ? env : -1, tid, table, frame, &valid);
    gather_row<ES, C>(q.g, ok, env, tid, table, frame, exchange, rows + entry * policy_bytes_per_env(q.g.stack, C, ES));
}

__global__ void __launch_bounds__(kTrBlock) transition_gae_kernel(TransitionGae q) {
    const int i = static_cast<int>(blockIdx.x) * kTrBlock + static_cast<int>(threadIdx.x);
    if (i >= q.n) return;
    const TransitionRing& g = q.ring;
    const size_t n = size_t(q.n);
    const float c = q.gamma * q.lambda;
    float carry = 0.0f;
    float v_next = q.values[size_t(q.length) * n + i];
    for (int t = q.length - 1; t >= 0; t--) {
        const int64_t row = q.first + t;
        const size_t at = history_began_offset(history_slot(row, g.capacity), g.n, i);
        const uint8_t began_next = g.began[history_began_offset(history_slot(row + 1, g.capacity), g.n, i)];
        const size_t cell = size_t(t) * n + i;
        const float v = q.values[cell];
        const GaeStep s = gae_step(g.b.flags[at], began_next, g.b.reward[at], v, v_next, q.trunc_values ? q.trunc_values[cell] : 0.0f, q.gamma, c, carry);
        q.advantages[cell] = s.adv;
        if (q.returns) q.returns[cell] = s.ret;
        carry = s.adv;
        v_next = v;
    }
}

inline dim3 transition_grid(int n) { return dim3((n + kTrBlock - 1) / kTrBlock); }
inline void launch_transition_record(hipStream_t st, const TransitionRecord& q) {
    hipLaunchKernelGGL(transition_record_kernel, transition_grid(q.n), dim3(kTrBlock), 0, st, q);
}
inline void launch_transition_gather(hipStream_t st, const TransitionGather& q, int es) {
    for_es_planes(es, q.g.b.planes, [&](auto es_c, auto planes_c) {
        hipLaunchKernelGGL((transition_gather_kernel<decltype(es_c)::value, decltype(planes_c)::value>), dim3(q.g.count, q.next_obs ? 2 : 1),
                           dim3(kHistoryBlock), 0, st, q);
    });
}
inline void launch_transition_gae(hipStream_t st, const TransitionGae& q) {
    hipLaunchKernelGGL(transition_gae_kernel, transition_grid(q.n), dim3(kTrBlock), 0, st, q);
}

}  // namespace pg
#endif
