// Per-env state records (include/procgen2_vec.h pgv_save_envs / pgv_load_envs): one env's complete state as a fixed-size
// block of bytes in device memory, gathered from and scattered to the per-env regions of the state block (pg_engine.h
// Carve, describe mode) and the engine's own per-env data (the level plan's arrays, reward, done, the observation row).
//
// A record:  [ 16-byte header | region 0 | region 1 | … ],  every region's share — its F pieces of E bytes one after the
// other, piece f at f·E — rounded up to 16 bytes and the padding written as zeros, so equal states give equal bytes.
// Header: word 0 kRecordFull or kRecordEmpty (an index outside the batch was saved; a load skips it, as it skips a record
// of zeros), word 1 bit 0 "a reset is due in the env's next step" (StepIO::pending, freed of the step parity and of the
// two games' encodings), words 2-3 zero.
//
// One gather and one scatter kernel for every game.  A workgroup of 256 lanes serves (64 consecutive records) × (one
// region), and the two shapes of region get opposite lane mappings:
//   * blocks — E a multiple of 4 and at least 64 bytes: a wavefront per record, lanes along the bytes of a piece, 16
//     bytes a lane where E is a multiple of 16 (the piece then starts 16-byte aligned on both sides: the region's base is
//     256-byte aligned, the record's share 16-byte), 4 bytes otherwise (`mt`: 2 500 B);
//   * fields (E = 4 or 1, F of them) and the small odd blocks (a byte a slot): lanes along the 64 RECORDS, a wavefront
//     per field — a save of consecutive env indices reads whole lines — staged through LDS (row stride 65 words: no bank
//     conflict either way round) and moved to and from the records in 16-byte vectors, lanes along a record's bytes.
// Plain loads and stores; nothing here is faster than memory allows and nothing needs to be.
#pragma once

#include "pg_engine.h"
#include "pg_prefetch.h"

namespace pg {

constexpr int kRecordHeaderBytes = 16;
constexpr int kMaxRecordRegions = 40;
constexpr uint32_t kRecordLayoutVersion = 3;  // part of pgv_env_record_tag: bump with the layout above (2: the level plan's assignment arrays travel; 3: the plan's regions in list_plan's order)

struct RecordRegion {
    uint8_t* base;
    uint32_t pieces, piece_bytes;  // F, E
    uint32_t offset;               // of the region's share in a record (a multiple of 16)
};
struct RecordTable {
    RecordRegion r[kMaxRecordRegions];
    int regions;
    int n;                   // envs of the engine
    uint32_t record_bytes;   // a multiple of 16
    uint8_t* pending;        // StepIO::pending
    uint8_t* selectors;      // Game::stream_selectors or nullptr: zeroed for a loaded slot
    int due_mark, due_code;  // save: pending == 1 or == due_mark means "reset due"; load: what "reset due" is written as
};

#if defined(__HIPCC__)
constexpr int kRecordGroup = 64;     // records per workgroup
constexpr int kRecordChunk = 256;    // bytes of a record's share staged at a time
constexpr int kRecordStride = 65;    // words a staged row
static_assert(kRecordChunk % 16 == 0 && kRecordStride * 4 >= kRecordChunk + 4, "staging rows");

PG_D bool record_block_shape(const RecordRegion& r) { return r.piece_bytes % 4 == 0 && r.piece_bytes >= 64; }
PG_D uint32_t record_share(const RecordRegion& r) { return (r.pieces * r.piece_bytes + 15u) / 16u * 16u; }

// kLoad = false: gather (engine → records); true: scatter (records → engine).
template <bool kLoad>
__global__ void __launch_bounds__(256) records_kernel(RecordTable t, const int32_t* indices, int count, uint8_t* records) {
    __shared__ uint32_t stage[kRecordGroup * kRecordStride];
    __shared__ int32_t env_of[kRecordGroup];  // the env of each record of the group, or -1: nothing to move
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int first = static_cast<int>(blockIdx.x) * kRecordGroup;
    const RecordRegion r = t.r[blockIdx.y];
    if (tid < kRecordGroup) {
        const int k = first + tid;
        int env = -1;
        if (k < count) {
            env = indices ? indices[k] : k;
            if (env < 0 || env >= t.n) env = -1;
            uint32_t* head = reinterpret_cast<uint32_t*>(records + size_t(k) * t.record_bytes);
            if (kLoad) {
                if (env >= 0 && head[0] != kRecordFull) env = -1;
                if (env >= 0 && blockIdx.y == 0) {
                    t.pending[env] = (head[1] & 1u) ? static_cast<uint8_t>(t.due_code) : 0;
                    if (t.selectors) t.selectors[env] = 0;  // the stream is at home, nothing is made ahead
                }
            } else if (blockIdx.y == 0) {
                uint32_t due = 0u;
                if (env >= 0) {
                    const int p = t.pending[env];
                    due = (p == 1 || p == t.due_mark) ? 1u : 0u;
                }
                *reinterpret_cast<uint4*>(head) = make_uint4(env >= 0 ? kRecordFull : kRecordEmpty, due, 0u, 0u);
            }
        }
        env_of[tid] = env;
    }
    __syncthreads();
    const uint32_t E = r.piece_bytes, F = r.pieces, bytes = F * E, share = record_share(r);
    const size_t plane = size_t(t.n) * E;  // from one piece of an env to its next

    if (record_block_shape(r)) {
        for (int q = wave; q < kRecordGroup && first + q < count; q += 4) {  // (wave-uniform)
            const int env = env_of[q];
            uint8_t* rec = records + size_t(first + q) * t.record_bytes + r.offset;
            if (env < 0) {
                if (!kLoad)
                    for (uint32_t k = lane; k < share / 16; k += 64) reinterpret_cast<uint4*>(rec)[k] = make_uint4(0u, 0u, 0u, 0u);
                continue;
            }
            for (uint32_t f = 0; f < F; f++) {
                uint8_t* mem = r.base + f * plane + size_t(env) * E;
                uint8_t* in_rec = rec + f * E;
                if (E % 16 == 0) {
                    uint4* a = reinterpret_cast<uint4*>(kLoad ? mem : in_rec);
                    const uint4* b = reinterpret_cast<const uint4*>(kLoad ? in_rec : mem);
                    for (uint32_t k = lane; k < E / 16; k += 64) a[k] = b[k];
                } else {
                    uint32_t* a = reinterpret_cast<uint32_t*>(kLoad ? mem : in_rec);
                    const uint32_t* b = reinterpret_cast<const uint32_t*>(kLoad ? in_rec : mem);
                    for (uint32_t k = lane; k < E / 4; k += 64) a[k] = b[k];
                }
            }
            if (!kLoad)
                for (uint32_t k = bytes / 4 + lane; k < share / 4; k += 64) reinterpret_cast<uint32_t*>(rec)[k] = 0u;
        }
        return;
    }

    // fields and small odd blocks: a unit is a word where E is a multiple of 4, a byte otherwise
    const uint32_t unit = E % 4 == 0 ? 4u : 1u;
    const int env = env_of[lane];
    for (uint32_t c0 = 0; c0 < share; c0 += kRecordChunk) {  // (workgroup-uniform)
        const uint32_t cb = share - c0 < kRecordChunk ? share - c0 : kRecordChunk;  // a multiple of 16
        const uint32_t vecs = cb / 16;
        if (kLoad) {
            for (uint32_t v = tid; v < kRecordGroup * vecs; v += 256) {
                const uint32_t q = v / vecs, k = v - q * vecs;
                if (env_of[q] < 0) continue;
                const uint4 w = *reinterpret_cast<const uint4*>(records + size_t(first + q) * t.record_bytes + r.offset + c0 + k * 16);
                uint32_t* row = stage + q * kRecordStride + k * 4;
                row[0] = w.x, row[1] = w.y, row[2] = w.z, row[3] = w.w;
            }
            __syncthreads();
        }
        for (uint32_t u = wave; u < cb / unit; u += 4) {  // lanes along the records
            const uint32_t b = c0 + u * unit;  // byte of the share
            const bool real = b < bytes;
            const uint32_t f = b / E, rest = b - f * E;
            uint8_t* mem = r.base + f * plane + size_t(env < 0 ? 0 : env) * E + rest;
            if (unit == 4) {
                uint32_t* cell = stage + lane * kRecordStride + u;
                if (kLoad) {
                    if (env >= 0 && real) *reinterpret_cast<uint32_t*>(mem) = *cell;
                } else {
                    *cell = (env >= 0 && real) ? *reinterpret_cast<const uint32_t*>(mem) : 0u;
                }
            } else {
                uint8_t* cell = reinterpret_cast<uint8_t*>(stage + lane * kRecordStride) + u;
                if (kLoad) {
                    if (env >= 0 && real) *mem = *cell;
                } else {
                    *cell = (env >= 0 && real) ? *mem : 0;
                }
            }
        }
        __syncthreads();
        if (!kLoad) {
            for (uint32_t v = tid; v < kRecordGroup * vecs; v += 256) {
                const uint32_t q = v / vecs, k = v - q * vecs;
                if (first + static_cast<int>(q) >= count) continue;
                const uint32_t* row = stage + q * kRecordStride + k * 4;
                *reinterpret_cast<uint4*>(records + size_t(first + q) * t.record_bytes + r.offset + c0 + k * 16) =
                    make_uint4(row[0], row[1], row[2], row[3]);
            }
            __syncthreads();
        }
    }
}

// (a grid's x is the groups of 64 records, its y the regions; 65 536 records are 1 024 groups)
inline void launch_records(hipStream_t st, const RecordTable& t, bool load, const int32_t* d_indices, int count, void* d_records) {
    const dim3 grid((count + kRecordGroup - 1) / kRecordGroup, t.regions);
    if (load)
        hipLaunchKernelGGL(records_kernel<true>, grid, dim3(256), 0, st, t, d_indices, count, static_cast<uint8_t*>(d_records));
    else
        hipLaunchKernelGGL(records_kernel<false>, grid, dim3(256), 0, st, t, d_indices, count, static_cast<uint8_t*>(d_records));
}
#endif

}  // namespace pg
