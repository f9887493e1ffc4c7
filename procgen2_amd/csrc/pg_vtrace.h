// V-trace over the transition ring (include/procgen2_vec.h pgv_transitions_vtrace): value targets and policy-gradient
// advantages of a stretch of rows under clipped importance ratios, one launch.  The rule is vtrace_step below, made of the
// three pieces the kernel's phases are: vtrace_cell (everything about a cell that no other row decides), vtrace_carry (the
// recurrence: one product and one sum a row) and vtrace_vs / vtrace_pg (what a cell gives once x and the row above are known).
//
// The kernel: a workgroup of 256 lanes owns a tile of 64 consecutive envs and walks the stretch from the back in chunks of
// R = kVtRows rows; chunk j holds rows [max(0, L - (j+1)·R), L - j·R), so the ragged one, L % R rows, is the stretch's front.
//     A  all four waves.  Wave w takes rows w·R/4 .. of the chunk, lane = env: R/4 cells a lane, each flags, began[q+1],
//        reward, rho, trunc and V — R/4 + 1 loads of V, the row above a cell being the lane's own next load.  The loads of a
//        whole chunk are issued into registers first (vtrace_load), then vtrace_cell runs and the cell goes to an LDS slab
//        [R][64] (vtrace_fill): delta, k, v, r, nv, pr and the mode byte (dead, ends, plain).
//     B  wave 0, lane = env: the chunk's rows from the last to the first, delta, k and mode from LDS, x written over delta;
//        carry stays in a register across chunks.  No global memory.  A dead or ending row gives x = delta by its mode, never
//        by 0 * carry.
//     C  all four waves, the cells as in A: vs = x + v (v where dead), the row above's vs made the same way from its slab
//        entries — the chunk's last row takes the edge row instead: V[L], then the vs of the first row of the chunk walked
//        before —, pg where asked (workgroup-uniform).  Coalesced stores.
// Two slabs and two edge rows.  Per chunk j: every wave issues the loads of chunk j + 1; wave 0 walks B of chunk j while they
// are in flight; every wave fills slab (j+1) & 1; BARRIER 1 (B's x of slab j & 1 and A's cells of the other slab are
// visible); C of chunk j reads slab j & 1 and edge j & 1, writes edge (j+1) & 1; BARRIER 2 (C has left slab j & 1 before the
// fill of chunk j + 2 writes it, and its edge row is visible).  So the load latency is paid once a chunk, under B, and not
// once a row.  No atomics, nothing allocated, no host synchronisation.
// Bounds.  The grid is ceil(n / 64) workgroups; env = blockIdx·64 + lane, every access under env < n and local row < the
// chunk's rows, masked and not padded.  t <= L - 1: flags, reward at [slot(first + t)·n + env] and began at [slot(first + t
// + 1)·n + env], both rows held by the host's check, so slot < T (one wrap a step: slot + 1 == T → 0); rhos, trunc_values, vs,
// pg at [t·n + env] <= L·n - 1; values at [(t + 1)·n + env] <= (L + 1)·n - 1: the array has L + 1 rows.  LDS: two slabs of
// R·64·(6·4 + 1) = 25 600 bytes and two edge rows of 256: 51 712 bytes, slab row < R, column = lane < 64.
#pragma once

#include "pg_transitions.h"

namespace pg {

constexpr int kVtRows = 16;   // R: rows a chunk (procgen2_amd/lib.py VTRACE_ROWS)
constexpr int kVtEnvs = 64;   // envs a workgroup: a wave a row
constexpr int kVtBlock = 256;
constexpr int kVtLaneRows = kVtRows / (kVtBlock / kVtEnvs);  // cells a lane a chunk
constexpr uint8_t kVtDead = 0, kVtEnds = 1, kVtPlain = 2;    // a cell's mode

struct VtraceRule {
    float gamma, lambda, rho_bar, c_bar, pg_rho_bar, reward_scale, reward_clip;
};
struct VtraceCell {
    float delta, k, v, r, nv, pr;
    uint8_t mode;
};
// Every product, sum and difference below is its own float32 rounding (the build forms no fused multiply-add).
PG_HD VtraceCell vtrace_cell(const VtraceRule& p, uint8_t flags, uint8_t began_next, float reward, float v, float v_next, float v_trunc, float rho) {
    if ((flags & kTrRecorded) == 0 || (flags & kTrVoid) != 0) return VtraceCell{0.0f, 0.0f, v, 0.0f, 0.0f, 0.0f, kVtDead};
    const uint8_t ends = transition_ends(flags, began_next);
    const float nv = ends == 0 ? v_next : ends == kTrTruncated ? v_trunc : 0.0f;  // (as gae_step has it)
    const float s = reward * p.reward_scale;
    const float clip = p.reward_clip;
    const float r = clip <= 0.0f ? s : s > clip ? clip : s < -clip ? -clip : s;
    const float rc = rho < p.rho_bar ? rho : p.rho_bar;
    const float cm = rho < p.c_bar ? rho : p.c_bar;
    const float cc = p.lambda * cm;
    const float pr = rho < p.pg_rho_bar ? rho : p.pg_rho_bar;
    const float a = p.gamma * nv;
    const float b = r + a;
    const float d = b - v;
    const float delta = rc * d;
    const float k = p.gamma * cc;
    return VtraceCell{delta, k, v, r, nv, pr, ends ? kVtEnds : kVtPlain};
}
// x of a row from the carry of the row above (a dead cell's delta is 0: its x, and the carry it hands on).
PG_HD float vtrace_carry(uint8_t mode, float delta, float k, float carry) {
    if (mode != kVtPlain) return delta;
    const float e = k * carry;
    return delta + e;
}
PG_HD float vtrace_vs(uint8_t mode, float x, float v) { return mode == kVtDead ? v : x + v; }
PG_HD float vtrace_pg(const VtraceRule& p, uint8_t mode, float v, float r, float nv, float pr, float vs_next) {
    if (mode == kVtDead) return 0.0f;
    const float qn = mode == kVtPlain ? vs_next : nv;
    const float pa = p.gamma * qn;
    const float pb = r + pa;
    const float pd = pb - v;
    return pr * pd;
}
// One row of the walk t = L-1 .. 0: `carry` the x and `vs_next` the vs of row t + 1 (0 and V[L] behind the stretch); the caller
// carries x and vs on.  The statement the kernel's phases and tests/cpp/test_vtrace.cpp share.
struct VtraceStep {
    float x, vs, pg;
};
PG_HD VtraceStep vtrace_step(const VtraceRule& p, uint8_t flags, uint8_t began_next, float reward, float v, float v_next, float v_trunc, float rho,
                             float carry, float vs_next) {
    const VtraceCell c = vtrace_cell(p, flags, began_next, reward, v, v_next, v_trunc, rho);
    const float x = vtrace_carry(c.mode, c.delta, c.k, carry);
    return VtraceStep{x, vtrace_vs(c.mode, x, v), vtrace_pg(p, c.mode, c.v, c.r, c.nv, c.pr, vs_next)};
}

struct TransitionVtrace {
    int n, length;
    int64_t first;
    VtraceRule rule;
    const float *values, *rhos, *trunc_values;
    float *vs, *pg;
    TransitionRing ring;
};

}  // namespace pg

#if defined(__HIPCC__)
#include "pg_engine.h"

namespace pg {

struct VtraceSlab {
    float x[kVtRows][kVtEnvs];  // delta until phase B has passed
    float k[kVtRows][kVtEnvs], v[kVtRows][kVtEnvs], r[kVtRows][kVtEnvs], nv[kVtRows][kVtEnvs], pr[kVtRows][kVtEnvs];
    uint8_t mode[kVtRows][kVtEnvs];
};
// A lane's cells of one chunk as loaded: rows row0 .. row0 + kVtLaneRows - 1 of the chunk, those below `rows` only.
struct VtraceLoads {
    uint8_t flags[kVtLaneRows], began[kVtLaneRows];
    float reward[kVtLaneRows], rho[kVtLaneRows], trunc[kVtLaneRows], v[kVtLaneRows + 1];
};
__device__ __forceinline__ void vtrace_load(const TransitionVtrace& q, int lo, int rows, int row0, int env, VtraceLoads& c) {
    if (row0 >= rows) return;  // (wave-uniform)
    const TransitionRing& g = q.ring;
    const size_t n = size_t(q.n);
    int slot = history_slot(q.first + lo + row0, g.capacity);
    c.v[0] = q.values[size_t(lo + row0) * n + env];
#pragma unroll
    for (int i = 0; i < kVtLaneRows; i++) {
        if (row0 + i >= rows) break;
        const int next = slot + 1 == g.capacity ? 0 : slot + 1;
        const size_t at = history_began_offset(slot, g.n, env), cell = size_t(lo + row0 + i) * n + env;
        c.flags[i] = g.b.flags[at];
        c.reward[i] = g.b.reward[at];
        c.began[i] = g.began[history_began_offset(next, g.n, env)];
        c.rho[i] = q.rhos ? q.rhos[cell] : 1.0f;
        c.trunc[i] = q.trunc_values ? q.trunc_values[cell] : 0.0f;
        c.v[i + 1] = q.values[cell + n];
        slot = next;
    }
}
__device__ __forceinline__ void vtrace_fill(const TransitionVtrace& q, int rows, int row0, int lane, const VtraceLoads& c, VtraceSlab& s) {
#pragma unroll
    for (int i = 0; i < kVtLaneRows; i++) {
        const int r = row0 + i;
        if (r >= rows) break;
        const VtraceCell cell = vtrace_cell(q.rule, c.flags[i], c.began[i], c.reward[i], c.v[i], c.v[i + 1], c.trunc[i], c.rho[i]);
        s.x[r][lane] = cell.delta, s.k[r][lane] = cell.k, s.v[r][lane] = cell.v, s.r[r][lane] = cell.r;
        s.nv[r][lane] = cell.nv, s.pr[r][lane] = cell.pr, s.mode[r][lane] = cell.mode;
    }
}

__global__ void __launch_bounds__(kVtBlock) transition_vtrace_kernel(TransitionVtrace q) {
    __shared__ VtraceSlab slab[2];
    __shared__ float edge[2][kVtEnvs];  // vs of the row above a chunk's last
    const int lane = static_cast<int>(threadIdx.x) & (kVtEnvs - 1), wave = static_cast<int>(threadIdx.x) / kVtEnvs;
    const int env = static_cast<int>(blockIdx.x) * kVtEnvs + lane;
    const bool inside = env < q.n;
    const int L = q.length, chunks = (L + kVtRows - 1) / kVtRows, row0 = wave * kVtLaneRows;
    const size_t n = size_t(q.n);
    VtraceLoads loads;
    float carry = 0.0f;
    {
        const int lo = L > kVtRows ? L - kVtRows : 0;
        if (inside) {
            vtrace_load(q, lo, L - lo, row0, env, loads);
            if (wave == 0) edge[0][lane] = q.values[size_t(L) * n + env];
            vtrace_fill(q, L - lo, row0, lane, loads, slab[0]);
        }
    }
    __syncthreads();
    for (int j = 0; j < chunks; j++) {
        const int hi = L - j * kVtRows, lo = hi > kVtRows ? hi - kVtRows : 0, rows = hi - lo;
        const int next_lo = lo > kVtRows ? lo - kVtRows : 0;  // chunk j + 1 is rows [next_lo, lo), where there is one
        VtraceSlab& s = slab[j & 1];
        const bool more = inside && j + 1 < chunks;
        if (more) vtrace_load(q, next_lo, lo - next_lo, row0, env, loads);
        if (wave == 0 && inside) {  // phase B
#pragma unroll
            for (int r = kVtRows - 1; r >= 0; r--) {
                if (r < rows) {
                    carry = vtrace_carry(s.mode[r][lane], s.x[r][lane], s.k[r][lane], carry);
                    s.x[r][lane] = carry;
                }
            }
        }
        if (more) vtrace_fill(q, lo - next_lo, row0, lane, loads, slab[(j + 1) & 1]);
        __syncthreads();  // barrier 1
        if (inside) {     // phase C
#pragma unroll
            for (int i = 0; i < kVtLaneRows; i++) {
                const int r = row0 + i;
                if (r >= rows) break;
                const uint8_t mode = s.mode[r][lane];
                const float v = s.v[r][lane];
                const float vs = vtrace_vs(mode, s.x[r][lane], v);
                const size_t cell = size_t(lo + r) * n + env;
                q.vs[cell] = vs;
                if (r == 0) edge[(j + 1) & 1][lane] = vs;
                if (q.pg) {
                    const float above = r + 1 < rows ? vtrace_vs(s.mode[r + 1][lane], s.x[r + 1][lane], s.v[r + 1][lane]) : edge[j & 1][lane];
                    q.pg[cell] = vtrace_pg(q.rule, mode, v, s.r[r][lane], s.nv[r][lane], s.pr[r][lane], above);
                }
            }
        }
        __syncthreads();  // barrier 2
    }
}

inline void launch_transition_vtrace(hipStream_t st, const TransitionVtrace& q) {
    hipLaunchKernelGGL(transition_vtrace_kernel, dim3((q.n + kVtEnvs - 1) / kVtEnvs), dim3(kVtBlock), 0, st, q);
}

}  // namespace pg
#endif
