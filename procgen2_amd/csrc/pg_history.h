// Frame history on the device (include/procgen2_vec.h pgv_history_enable): a ring of the last T frames of every env, each
// stored once as planar u8, and a gather that turns (push number, env) pairs into what pg_policy_obs.h keeps for "now" —
// stacked, scaled, channel-first rows — only when somebody reads them:
//     frames [T][N][C][64][64] u8; C = 3 (planes R, G, B) or 1 (policy_gray); push number p lives in slot p % T;
//     began  [T][N] u8: 1 where the frame is the first an env shows of an episode; pending [N]: the flag the next push files;
//     a gathered row [K*C][64][64] elements; slot K-1 the newest frame; values by policy_table_entry.
// Push p is HELD while head - T <= p < head (head: the pushes so far, a host counter handed to every launch by value).
//
// Values, the lane's share of a frame, units, the wave's exchange and the row of zero bytes are pg_planes.h's.
//
// The push kernel: one workgroup of 256 lanes per env.  A lane reads its 48 bytes of the slab and stores 16 bytes per plane: at
// one byte per element the lanes of a plane lie 16 bytes apart as they are, so nothing is exchanged.  Lane 0 files the env's
// pending flag as the slot's began byte and clears it; no other lane touches either byte.  An env whose mask byte is 0 is left
// before anything is read or written.  The form pgv_reset uses (`reset` set) writes into the newest slot and files began = 1.
//
// The gather kernel: one workgroup of 256 lanes per entry, begun by gather_entry and fed by history_fetch (both shared with
// pg_history_aug.h); its body behind the head is gather_row, which pg_transitions.h calls for its two rows as well.  Per frame and plane a lane looks its 16 stored bytes up: 16·ES bytes, which at ES = 2 and 4 the wave
// exchanges (measured against each lane storing its own units as they lie: -7 % at 2 bytes, -36 % at 4, docs/OPTLOG.md).
// Where the walk repeats a frame the values already in registers are stored again.  An entry that is not held, or whose env
// is outside the batch, gets a row of zero bytes.
// Plain vector loads and stores, no atomics.
// Bounds.  Push: the grid is n workgroups, env = blockIdx.x < n, slot < T by the host; a lane reads obs[env·12 288 + 48t ..
// + 47] and writes frames[((slot·n + env)·C + c)·4096 + 16t .. + 15], c < C, t < 256  <  T·n·C·4096; began[slot·n + env],
// pending[env].  Gather: the grid is `count` workgroups, entry = blockIdx.x < count; pushes[entry], envs[entry]; nothing of
// the ring is read unless 0 <= env < n and max(0, head - T) <= p < head, and the walk only ever moves to a held push, so
// every slot is f % T < T with f >= 0; a lane writes channel ch < K·C, wave w < 4, unit u < 64·ES at
// entry·K·C·4096·ES + policy_unit_offset(ES, ch, w, u) .. + 15  <  (entry + 1)·K·C·4096·ES; the zero row writes units
// u < 256·ES of 16 bytes of every channel, the same bytes.  The table is indexed by a byte.
// Offsets are size_t: 65 536 envs, T = 32, RGB are 25.8 GB.
#pragma once

#include "pg_carve.h"
#include "pg_defs.h"
#include "pg_policy_obs.h"

namespace pg {

constexpr int kHistoryBlock = kPolicyBlock;  // lanes a workgroup, 16 pixels a lane

PG_HD int history_slot(int64_t push, int capacity) { return static_cast<int>(push % capacity); }  // (push >= 0)
PG_HD bool history_held(int64_t push, int64_t head, int capacity) { return push >= 0 && push < head && push >= head - capacity; }
// Byte offset of env's frame in a slot, and of its began byte.
PG_HD size_t history_frame_offset(int slot, int n, int env, int planes) {
    return (size_t(slot) * size_t(n) + size_t(env)) * size_t(planes) * kPolicyPlane;
}
PG_HD size_t history_began_offset(int slot, int n, int env) { return size_t(slot) * size_t(n) + size_t(env); }
PG_HD size_t history_frames_bytes(int capacity, int n, int planes) { return history_frame_offset(capacity, n, 0, planes); }

// The walk of a gathered entry (push, env), both valid: f[0] = push; f[j] = f[j-1] where that frame began an episode or the
// push in front of it is no longer held, else f[j-1] - 1.  Row slot K-1-j shows frame f[j].
PG_HD void history_walk(const uint8_t* began, int n, int capacity, int64_t head, int64_t push, int env, int stack, int64_t* f) {
    f[0] = push;
    for (int j = 1; j < stack; j++) {
        const int64_t at = f[j - 1];
        const bool stop = began[history_began_offset(history_slot(at, capacity), n, env)] != 0 || !history_held(at - 1, head, capacity);
        f[j] = stop ? at : at - 1;
    }
}

// The engine's own block behind the feature (pg_carve.h): the pending flags, the began bytes, the four value tables and,
// unless the caller brought them, the frames.  The listing reads its sizes from the struct.
struct HistoryBuffers {
    int capacity, planes, own_frames;
    uint8_t* pending;  // [n]
    uint8_t* began;    // [T][n]
    uint32_t* table;   // [4][256]
    uint8_t* frames;   // [T][n][C][64][64]
};
inline void list_history(Carve& c, HistoryBuffers& b, int n) {
    c.take(b.pending, size_t(n));
    c.take(b.began, size_t(b.capacity) * size_t(n));
    c.take(b.table, kPolicyTables * 256 * 4);
    if (b.own_frames) c.take(b.frames, history_frames_bytes(b.capacity, n, b.planes));
}

struct HistoryPush {
    int n, planes, slot, reset;  // reset: pgv_reset's form — began = 1 whatever the flag
    const uint8_t* obs;          // the engine's slab (StepIO), 16-byte aligned
    const uint8_t* mask;         // [n] or nullptr = all
    HistoryBuffers b;
};

struct HistoryGather {
    int n, stack, count;
    int64_t head;
    const int64_t* pushes;  // [count]
    const int32_t* envs;    // [count]
    const uint32_t* table;  // the dtype's 256 words
    uint8_t* out;           // [count][K*C][64][64] elements, 16-byte aligned
    HistoryBuffers b;
};

#if defined(__HIPCC__)
template <int C>
__global__ void __launch_bounds__(kHistoryBlock) history_push_kernel(HistoryPush q) {
    const int env = static_cast<int>(blockIdx.x);
    if (q.mask && !q.mask[env]) return;  // (workgroup-uniform)
    const int tid = static_cast<int>(threadIdx.x);
    const SlabWords slab = slab_load(q.obs, env, tid);
    if (tid == 0) {
        q.b.began[history_began_offset(q.slot, q.n, env)] = q.reset ? uint8_t(1) : q.b.pending[env];
        q.b.pending[env] = 0;
    }
    uint8_t* const to = q.b.frames + history_frame_offset(q.slot, q.n, env, C) + size_t(tid) * kPolicyLanePixels;
#pragma unroll
    for (int p = 0; p < C; p++) {
        uint32_t v[kPolicyLanePixels];
        slab_plane_bytes<C>(slab, p, v);
        PolicyVec16 mine[1];
        policy_pack<1>(v, mine);
        *reinterpret_cast<PolicyVec16*>(to + size_t(p) * kPolicyPlane) = mine[0];
    }
}

// The head of a gather kernel: all lanes copy the dtype's 256 table words into `table` while lane 0 validates the entry and,
// where it is valid, walks back from its push (history_walk: at most K-1 dependent byte loads of began) into `frame`; one
// barrier shares both (all three in LDS).  Returns the verdict (workgroup-uniform).  gather_entry_at: the entry's push and env
// are the caller's (pg_transitions.h: the push behind an n-step walk); gather_entry reads them from the lists, and hands back `env`.
PG_D bool gather_entry_at(const HistoryGather& q, int64_t push, int env, int tid, uint32_t* table, int64_t* frame, int* valid) {
    table[tid] = q.table[tid];
    if (tid == 0) {
        const int ok = env >= 0 && env < q.n && history_held(push, q.head, q.b.capacity);
        *valid = ok;
        if (ok) history_walk(q.b.began, q.n, q.b.capacity, q.head, push, env, q.stack, frame);
    }
    __syncthreads();  // the table is whole; the walk is shared
    return *valid != 0;
}
PG_D bool gather_entry(const HistoryGather& q, size_t entry, int tid, uint32_t* table, int64_t* frame, int* valid, int& env) {
    env = q.envs[entry];
    return gather_entry_at(q, q.pushes[entry], env, tid, table, frame, valid);
}
// Lane tid's 16 stored bytes of each of the C planes of env's frame f (a held push).
template <int C>
PG_D void history_fetch(const HistoryGather& q, int64_t f, int env, int tid, PolicyVec16 (&in)[C]) {
    const uint8_t* from = q.b.frames + history_frame_offset(history_slot(f, q.b.capacity), q.n, env, C) + size_t(tid) * kPolicyLanePixels;
#pragma unroll
    for (int p = 0; p < C; p++) in[p] = *reinterpret_cast<const PolicyVec16*>(from + size_t(p) * kPolicyPlane);
}

// The body of a gather kernel behind its head: the row of an entry whose verdict is `ok` (workgroup-uniform) and whose walk
// lies in `frame`, at `out` — the K frames through the value table, or the row of zero bytes.
template <int ES, int C>  // element bytes; planes
PG_D void gather_row(const HistoryGather& q, bool ok, int env, int tid, const uint32_t* table, const int64_t* frame, PolicyVec16* exchange,
                     uint8_t* out) {
    const int lane = tid & 63, wave = tid >> 6;
    const int K = q.stack;
    const size_t channel = size_t(kPolicyPlane) * ES;
    if (!ok) {  // (workgroup-uniform)
        zero_row<PolicyVec16>(out, K * C, channel, kHistoryBlock * ES, tid);
        return;
    }
    size_t unit[ES];  // byte offset, inside a channel of this wave, of the units this lane stores
#pragma unroll
    for (int k = 0; k < ES; k++) unit[k] = policy_unit_offset(ES, 0, wave, policy_unit(true, ES, lane, k));
    PolicyVec16 held[C * ES];
    for (int j = 0; j < K; j++) {
        const int64_t f = frame[j];
        if (j == 0 || f != frame[j - 1]) {  // (workgroup-uniform)
            PolicyVec16 in[C];
            history_fetch<C>(q, f, env, tid, in);
#pragma unroll
            for (int p = 0; p < C; p++) {
                uint32_t v[kPolicyLanePixels];
                plane_values(table, in[p], v);
                PolicyVec16 mine[ES];
                policy_pack<ES>(v, mine);
                if (ES > 1) wave_exchange<ES>(exchange, wave, lane, mine);
#pragma unroll
                for (int k = 0; k < ES; k++) held[p * ES + k] = mine[k];
            }
        }
        uint8_t* const to = out + size_t(K - 1 - j) * C * channel;
#pragma unroll
        for (int p = 0; p < C; p++)
#pragma unroll
            for (int k = 0; k < ES; k++) *reinterpret_cast<PolicyVec16*>(to + p * channel + unit[k]) = held[p * ES + k];
    }
}

template <int ES, int C>
__global__ void __launch_bounds__(kHistoryBlock) history_gather_kernel(HistoryGather q) {
    __shared__ uint32_t table[256];
    __shared__ int64_t frame[kPolicyMaxStack];
    __shared__ int valid;
    __shared__ PolicyVec16 exchange[ES > 1 ? kHistoryBlock * ES : 1];  // a wave's units of one plane, in the wave's own quarter
    const int tid = static_cast<int>(threadIdx.x);
    const size_t entry = blockIdx.x;
    int env = 0;
    const bool ok = gather_entry(q, entry, tid, table, frame, &valid, env);
    gather_row<ES, C>(q, ok, env, tid, table, frame, exchange, q.out + entry * policy_bytes_per_env(q.stack, C, ES));
}

inline void launch_history_push(hipStream_t st, const HistoryPush& q) {
    hipLaunchKernelGGL(q.planes == 1 ? history_push_kernel<1> : history_push_kernel<3>, dim3(q.n), dim3(kHistoryBlock), 0, st, q);
}
inline void launch_history_gather(hipStream_t st, const HistoryGather& q, int es) {
    for_es_planes(es, q.b.planes, [&](auto es_c, auto planes_c) {
        hipLaunchKernelGGL((history_gather_kernel<decltype(es_c)::value, decltype(planes_c)::value>), dim3(q.count), dim3(kHistoryBlock), 0, st, q);
    });
}
#endif

}  // namespace pg
