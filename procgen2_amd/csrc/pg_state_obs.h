// Symbolic observations (include/procgen2_vec.h pgv_state_rows / pgv_tile_rows): every env's oracle state dump as a row
// of floats, and its tile map as a row of bytes, in device memory.
//
// A game states its row once, as a `Row` type beside its State:
//     using State;                       the game's device view
//     kWidth, kFixed, kRecord, kMaxRecords   the layout (kWidth == kFixed + kRecord * kMaxRecords)
//     kEnvCols                           the leading columns whose sources are [field][n] arrays
//     length(s, env)                     floats of this env's dump
//     value(s, env, col)                 column col of it, col < length(s, env)
//     names()                            host only: the columns' names, "<fixed names>|<record names>", space-separated
//     map(s)                             host only, tile games: the game's TileMaps (pg_paths.h)
// and state_rows_kernel<Row> lays the rows out.  It is the engine's only statement of the layout — the oracle's dump_state is
// the other one — and the debug taps read one row through it (engine.hip pgv_dump_state), so whatever test holds a tap to
// the oracle holds this.  ViewedGame, below, derives a game's host functions for these views from the Row.
//
// One kernel for every game, the shape of pg_records.h: a workgroup of 256 lanes takes 64 consecutive rows.  The two kinds
// of source get opposite lane mappings:
//   * columns below kEnvCols come from the [field][n] arrays: lanes along the ROWS, so that NULL or consecutive indices
//     read whole lines of a field;
//   * the columns behind them come from the per-env blocks (chaser's and caveflyer's entity tables, bossfight's shots,
//     jumper's puffs and spike cells): lanes along the ELEMENTS of one row.
// Both write a staging area in LDS whose rows are kWidth | 1 words apart — odd, so neither of the two WRITES has a bank
// conflict — and the staged rows leave over the FLAT output, padding included: 16-byte stores from the first 16-byte boundary
// of the staged range to its last, single words for the at most three floats at either end (a range starts at a multiple of
// kWidth floats, which need not be one of four).  The store phase reads its four words one at a time with neighbouring lanes
// four words apart: a 4-way conflict on the 64 banks, and the odd stride rules a single 128-bit LDS read out (a row's words
// are not 16-byte aligned in the stage).  Measured on chaser: the stage and the stores together are under a quarter of the
// kernel (docs/OPTLOG.md), so the reads were left as they are.
// 64 rows of the widest game (chaser, extreme: 1 597 floats) do not fit a workgroup's LDS, so a group is staged kRows rows
// at a time.
//
// Tiles are a strided copy with a mask, kTileStride → cells, and their rows end off the word grid (625, 121, 361 bytes):
// a lane makes one 16-byte vector of the FLAT output — it may span the end of one row and the start of the next — and
// stores it whole; the last vector of the call, where it is short, goes byte by byte.
// Plain loads and stores: the calls are read-only and on demand.
#pragma once

#include <initializer_list>
#include <string>
#include <type_traits>

#include "pg_engine.h"
#include "pg_frame.h"

namespace pg {

#if defined(__HIPCC__)
constexpr int kStateGroup = 64;          // rows per workgroup
constexpr int kStateStageWords = 8192;   // 32 KiB of LDS: two workgroups a CU beside a step's kernels

template <class Row>
__global__ void __launch_bounds__(256) state_rows_kernel(typename Row::State s, int n, const int32_t* indices, int count,
                                                          float* rows, int32_t* lengths) {
    constexpr int kW = Row::kWidth, kStride = kW | 1, kEnvCols = Row::kEnvCols, kRest = kW - kEnvCols;
    constexpr int kRows = kStateStageWords / kStride < kStateGroup ? kStateStageWords / kStride : kStateGroup;
    static_assert(kRows >= 1, "a row does not fit the staging area");
    static_assert(Row::kWidth == Row::kFixed + Row::kRecord * Row::kMaxRecords && kEnvCols <= kW, "layout");
    __shared__ float stage[kRows * kStride];
    __shared__ int32_t env_of[kStateGroup], len_of[kStateGroup];  // the env of each row of the group (-1: a row of zeros), its dump's length
    const int tid = threadIdx.x;
    const int first = static_cast<int>(blockIdx.x) * kStateGroup;
    const int here = count - first < kStateGroup ? count - first : kStateGroup;
    if (tid < here) {
        int env = indices ? indices[first + tid] : first + tid;
        if (env < 0 || env >= n) env = -1;
        const int len = env >= 0 ? Row::length(s, env) : 0;
        if (lengths) lengths[first + tid] = len;
        env_of[tid] = env;
        len_of[tid] = len;
    }
    __syncthreads();
    for (int q0 = 0; q0 < here; q0 += kRows) {  // (workgroup-uniform)
        const int R = here - q0 < kRows ? here - q0 : kRows;
        for (int t = tid; t < R * kEnvCols; t += 256) {  // lanes along the rows
            const int c = t / R, q = t - c * R;
            stage[q * kStride + c] = c < len_of[q0 + q] ? Row::value(s, env_of[q0 + q], c) : 0.0f;
        }
        for (int t = tid; t < R * kRest; t += 256) {  // lanes along a row's elements
            const int q = t / kRest, c = kEnvCols + (t - q * kRest);
            stage[q * kStride + c] = c < len_of[q0 + q] ? Row::value(s, env_of[q0 + q], c) : 0.0f;
        }
        __syncthreads();
        // the staged rows are floats [a, b) of the flat output; a4 .. b4 is the part on the 16-byte grid (the base is on it)
        const size_t a = size_t(first + q0) * kW;
        const uint32_t total = static_cast<uint32_t>(R) * kW;
        uint32_t head = static_cast<uint32_t>((4u - static_cast<uint32_t>(a & 3u)) & 3u);
        if (head > total) head = total;
        const uint32_t vecs = (total - head) / 4u, tail = head + vecs * 4u;
        auto staged = [&](uint32_t j) {
            const uint32_t q = j / kW;
            return stage[q * kStride + (j - q * kW)];
        };
        for (uint32_t v = tid; v < vecs; v += 256) {
            const uint32_t j = head + v * 4u;
            *reinterpret_cast<float4*>(rows + a + j) = make_float4(staged(j), staged(j + 1), staged(j + 2), staged(j + 3));
        }
        if (tid < 8) {  // lanes 0-3: the floats in front of the grid; 4-7: those behind it
            const uint32_t j = tid < 4 ? static_cast<uint32_t>(tid) : tail + static_cast<uint32_t>(tid - 4);
            if (tid < 4 ? j < head : j < total) rows[a + j] = staged(j);
        }
        __syncthreads();
    }
}

static __global__ void __launch_bounds__(256) tile_rows_kernel(const uint8_t* tiles, uint32_t stride, uint32_t cells, uint32_t mask,
                                                         int n, const int32_t* indices, int count, uint8_t* out) {
    const size_t total = size_t(count) * cells;
    const size_t at = (size_t(blockIdx.x) * 256 + threadIdx.x) * 16;
    if (at >= total) return;
    uint32_t k = static_cast<uint32_t>(at / cells), c = static_cast<uint32_t>(at - size_t(k) * cells);
    auto row_of = [&](uint32_t row) -> const uint8_t* {  // nullptr: a row of zeros
        const int env = indices ? indices[row] : static_cast<int>(row);
        return env < 0 || env >= n ? nullptr : tiles + size_t(env) * stride;
    };
    const uint8_t* src = row_of(k);
    const int m = total - at < 16 ? static_cast<int>(total - at) : 16;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    for (int b = 0; b < m; b++) {
        const uint32_t v = src ? (src[c] & mask) : 0u;
        w[b >> 2] |= v << (8 * (b & 3));
        if (++c == cells && b + 1 < m) {
            c = 0;
            src = row_of(++k);
        }
    }
    if (m == 16) {
        *reinterpret_cast<uint4*>(out + at) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (int b = 0; b < m; b++) out[at + b] = static_cast<uint8_t>(w[b >> 2] >> (8 * (b & 3)));
    }
}

// (65 536 rows are 1 024 groups: one grid)
template <class Row>
void launch_state_rows_of(hipStream_t st, const typename Row::State& s, int n, const int32_t* d_indices, int count, float* d_rows,
                          int32_t* d_lengths) {
    const uint32_t groups = (static_cast<uint32_t>(count) + kStateGroup - 1u) / kStateGroup;  // (unsigned: any count up to INT_MAX)
    hipLaunchKernelGGL(state_rows_kernel<Row>, dim3(groups), dim3(256), 0, st, s, n, d_indices, count, d_rows, d_lengths);
}
inline void launch_tile_rows_of(hipStream_t st, const TileMaps& m, int n, const int32_t* d_indices, int count, uint8_t* d_tiles) {
    const size_t vecs = (size_t(count) * m.cells + 15) / 16;
    hipLaunchKernelGGL(tile_rows_kernel, dim3(static_cast<uint32_t>((vecs + 255) / 256)), dim3(256), 0, st, m.tiles,
                       static_cast<uint32_t>(m.stride), static_cast<uint32_t>(m.cells), static_cast<uint32_t>(m.mask), n, d_indices,
                       count, d_tiles);
}

template <class Row>
constexpr StateLayout state_layout_of(const TileMaps& m) {
    return {Row::kWidth, Row::kFixed, Row::kRecord, Row::kMaxRecords, m.cells, m.w, m.h};
}

// Whether a Row states a tile map (bossfight's does not).
template <class Row, class = void>
struct HasTileMap {
    static constexpr bool value = false;
};
template <class Row>
struct HasTileMap<Row, decltype(static_cast<void>(&Row::map))> {
    static constexpr bool value = true;
};

// The host side of the read-only views, written once: a game's class derives from ViewedGame<Base, its StateRow, its PathRow
// or void, its Frames> — Base: whatever it derived from otherwise, a BoundGame (pg_engine.h) — and has all six, and the
// human-size frames (pg_frame.h), which are one more read-only view of the state.
template <class Base, class Row, class Points, class Frames>
class ViewedGame : public Base {
   public:
    bool launch_frame(hipStream_t st, int env, uint32_t* d_px, int w, int h) override {
        launch_frame_of<Frames>(st, this->s_, this->atlas_, env, d_px, w, h);
        return true;
    }
    void launch_frames(hipStream_t st, const int32_t* d_indices, int count, uint8_t* d_rgb, int w, int h) override {
        launch_frames_of<Frames>(st, this->s_, this->atlas_, d_indices, count, d_rgb, w, h);
    }
    StateLayout state_layout() const override { return state_layout_of<Row>(map()); }
    std::string state_names() const override { return Row::names(); }
    void launch_state_rows(hipStream_t st, const int32_t* d_indices, int count, float* d_rows, int32_t* d_lengths) override {
        launch_state_rows_of<Row>(st, this->s_, this->s_.n, d_indices, count, d_rows, d_lengths);
    }
    void launch_tile_rows(hipStream_t st, const int32_t* d_indices, int count, uint8_t* d_tiles) override {
        if constexpr (HasTileMap<Row>::value) launch_tile_rows_of(st, map(), this->s_.n, d_indices, count, d_tiles);
    }
    PathPoints path_points() const override {
        if constexpr (std::is_void<Points>::value) return Game::path_points();
        else return path_points_of<Points>();
    }
    void launch_tile_paths(hipStream_t st, const TilePaths& q) override {
        if constexpr (!std::is_void<Points>::value) launch_tile_paths_of<Points>(st, this->s_, map(), this->s_.n, q);
    }

   private:
    TileMaps map() const {
        if constexpr (HasTileMap<Row>::value) return Row::map(this->s_);
        else return TileMaps{nullptr, 0, 0, 0, 0, 0};
    }
};
#endif

// "p0_x p0_y p0_life p1_x …": the names of `count` slots of `fields` floats each, with a space in front of every one.
inline std::string slot_names(const char* prefix, int count, std::initializer_list<const char*> fields) {
    std::string out;
    for (int k = 0; k < count; k++)
        for (const char* f : fields) out += std::string(" ") + prefix + std::to_string(k) + "_" + f;
    return out;
}

}  // namespace pg
