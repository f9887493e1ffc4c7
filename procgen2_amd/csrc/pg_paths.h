// Path distances (include/procgen2_vec.h pgv_tile_paths_rows): the breadth-first distance field of every named env's tile
// map from one source cell, int16 [count][cells] laid out as the tile rows are, and what a second cell — the probe — sees
// of it: its distance and the neighbour that is one step nearer.
//
// A tile map is at most 64 × 64 and lies column-major (cell (x, y) at y + x * tile_h), so a whole board is one uint64 a
// lane of a wavefront: lane = column x, bit = y.  Three boards: `open` (the passable cells), `seen` (reached so far) and
// `front` (reached in the last level).  One level is
//     next = (front << 1 | front >> 1 | front of lane x-1 | front of lane x+1) & open & ~seen
// — two shifts inside the lane, two neighbour-lane exchanges, an and, an and-not — and the loop ends when a ballot finds
// `next` empty in every lane.  Lanes >= tile_w and bits >= tile_h are never in `open`, so nothing has to be masked at the
// right and bottom edges; the neighbour-lane exchange is a DPP shift of the whole wavefront by one lane (wave_shr:1,
// wave_shl:1 with bound_ctrl: two v_mov a direction, no LDS round trip), which hands lane 0 a 0 for its lower neighbour
// and lane 63 a 0 for its upper one, so nothing wraps; every shift is by 1, by a bit number or by a column offset below 64.
//
// The row routine (path_row, path_probe) is written once over a `Wave`: WaveLanes is the wavefront itself — a board is one
// register pair, each() runs its body once for the calling lane — and EmulatedLanes is 64 lanes in arrays on the host, for
// tests/cpp/test_tile_paths.cpp, where each() loops.  Values that differ between lanes live in a Wave::Board and are only
// touched inside each(); everything else in the routine is wave-uniform.
//
// The kernel: one wavefront a row, a workgroup of 256 lanes takes four consecutive rows.  A row's distances are made in
// an int16 stage in LDS — -1 everywhere first, then each cell's level when it is reached — at most 8 KiB a row.  The
// probe's answers are read from the stage.  Rows are 242, 1 250, 3 200 … bytes long and end off the 16-byte grid, so the
// four staged rows leave over the FLAT output as tile_rows_kernel's do (pg_state_obs.h): 16-byte stores
// from the first 16-byte boundary of the staged range to its last, single int16s for the at most seven in front and
// behind.  The stage starts (a mod 8) int16s into the LDS block, a the group's first element of the flat output, so that a
// 16-byte store's source is 16-byte aligned in LDS too (one ds_read_b128; the dynamic block is the kernel's only LDS, so
// its base is aligned).  Plain loads and stores: the call is read-only and on demand.
// Bounds.  Row k < count; env = indices[k] is used only where 0 <= env < n, and then tiles[env * stride + c], c < cells.
// A cell index is used only where 0 <= cell < cells (path_cell_of, path_given_cell).  The stage is written at shift +
// wave * cells + c, c < cells, shift < 8: below 4 * cells + 8 int16s, the block's size.  The flat store writes elements
// a .. a + R * cells - 1 of dist, R = the group's rows inside count.  Offsets into dist are size_t.
#pragma once

#include "pg_defs.h"

namespace pg {

// include/procgen2_vec.h PGV_PATH_*
constexpr int kPathNone = 0, kPathAgent = 1, kPathGoal = 2, kPathCells = 3;
constexpr int kPathMaxSide = 64;   // lanes a wavefront, bits a board word
constexpr int kPathGroupRows = 4;  // rows a workgroup: one a wavefront
constexpr int kPathBatch = 8;      // words of 64 cells whose loads are in flight together while the board is built

// The cell of a world point, -1 where it has none: x = floor(wx), y = tile_h - 1 - floor(wy).  (The comparisons come
// first: they are false for a NaN, and inside them the conversion is exact and truncation is floor.)
PG_HD int path_cell_of(float wx, float wy, int tile_w, int tile_h) {
    if (!(wx >= 0.0f && wx < static_cast<float>(tile_w) && wy >= 0.0f && wy < static_cast<float>(tile_h))) return -1;
    return (tile_h - 1 - static_cast<int>(wy)) + static_cast<int>(wx) * tile_h;
}
PG_HD int path_given_cell(int32_t cell, int cells) { return cell >= 0 && cell < cells ? cell : -1; }
PG_HD bool path_passable(uint32_t passable, uint32_t tile) { return tile < 32u && ((passable >> tile) & 1u) != 0u; }

// 64 lanes in arrays.
struct EmulatedLanes {
    static constexpr int kHeld = kPathMaxSide;
    struct Board { uint64_t v[kHeld]; };
    template <class F>
    void each(F&& f) const {
        for (int lane = 0; lane < kPathMaxSide; lane++) f(lane, lane);
    }
    Board from_lower(const Board& b) const {  // lane x: the value of lane x - 1
        Board r;
        for (int lane = 0; lane < kPathMaxSide; lane++) r.v[lane] = lane > 0 ? b.v[lane - 1] : 0u;
        return r;
    }
    Board from_upper(const Board& b) const {  // lane x: the value of lane x + 1
        Board r;
        for (int lane = 0; lane < kPathMaxSide; lane++) r.v[lane] = lane < kPathMaxSide - 1 ? b.v[lane + 1] : 0u;
        return r;
    }
    uint64_t ballot(const Board& b) const {  // bit l: lane l's word is not 0
        uint64_t r = 0u;
        for (int lane = 0; lane < kPathMaxSide; lane++) r |= uint64_t(b.v[lane] != 0u) << lane;
        return r;
    }
};

#if defined(__HIPCC__)
// The wavefront itself: the calling lane holds its own word of a board.
struct WaveLanes {
    static constexpr int kHeld = 1;
    struct Board { uint64_t v[kHeld]; };
    int lane;
    template <class F>
    __device__ __forceinline__ void each(F&& f) const { f(lane, 0); }
    // A DPP shift of the whole wavefront by one lane, one 32-bit half at a time: wave_shr:1 (0x138) hands lane x the value of
    // lane x - 1, wave_shl:1 (0x130) that of lane x + 1, and with bound_ctrl the lane without a partner gets 0.
    template <int kCtrl>
    static __device__ __forceinline__ uint64_t shifted(uint64_t v) {
        const uint32_t lo = __builtin_amdgcn_update_dpp(0, static_cast<int>(static_cast<uint32_t>(v)), kCtrl, 0xf, 0xf, true);
        const uint32_t hi = __builtin_amdgcn_update_dpp(0, static_cast<int>(static_cast<uint32_t>(v >> 32)), kCtrl, 0xf, 0xf, true);
        return uint64_t(hi) << 32 | lo;
    }
    __device__ __forceinline__ Board from_lower(const Board& b) const { return Board{{shifted<0x138>(b.v[0])}}; }
    __device__ __forceinline__ Board from_upper(const Board& b) const { return Board{{shifted<0x130>(b.v[0])}}; }
    __device__ __forceinline__ uint64_t ballot(const Board& b) const { return __ballot(b.v[0] != 0u); }
};
#endif

// One row: the distance of every cell of the map from cell `source` into row[0 .. tile_w * tile_h - 1].  tiles: the env's
// tile bytes, each taken & tile_mask as pgv_tile_rows gives them, or nullptr (then source must be -1).  source -1: no
// source, every cell -1.
template <class Wave>
PG_HD void path_row(const Wave& w, const uint8_t* tiles, int tile_w, int tile_h, uint32_t tile_mask, uint32_t passable, int source,
                    int16_t* row) {
    typename Wave::Board open, seen, front;
    const int sx = source >= 0 ? source / tile_h : -1, sy = source >= 0 ? source - sx * tile_h : 0;
    const int cells = tile_w * tile_h;
    // Every cell starts at -1, in the row's own order: 64 consecutive int16s an instruction, no two lanes on one bank (a
    // lane writing its own column puts all 64 lanes on one bank where tile_h is 64).  The cells that are reached are
    // written once more.
    w.each([&](int lane, int L) {
        open.v[L] = 0u;
        for (int c = lane; c < cells; c += kPathMaxSide) row[c] = -1;
    });
    // The passable board.  The lanes read the row 64 consecutive cells at a time — cell base + lane, whole lines — and a
    // ballot makes the 64 flags one word; lane x's column is bits x * tile_h .. + tile_h - 1 of the row, so it takes from
    // every word that holds some of them those bits, shifted to its own bit 0 (by less than 64 either way).
    // kPathBatch words' loads are issued together: one at a time, a row of 4 096 cells waited for memory 64 times over.
    for (int first = 0; source >= 0 && first < cells; first += kPathMaxSide * kPathBatch) {
        typename Wave::Board flag[kPathBatch];
        w.each([&](int lane, int L) {
            uint32_t tile[kPathBatch];
            for (int j = 0; j < kPathBatch; j++) {  // (unconditional loads, behind the row's end the last cell again: no wait between them)
                const int c = first + j * kPathMaxSide + lane;
                tile[j] = tiles[c < cells ? c : cells - 1];
            }
            for (int j = 0; j < kPathBatch; j++)
                flag[j].v[L] = first + j * kPathMaxSide + lane < cells && path_passable(passable, tile[j] & tile_mask) ? 1u : 0u;
        });
        for (int j = 0; j < kPathBatch; j++) {
            const int base = first + j * kPathMaxSide;
            if (base >= cells) break;
            const uint64_t word = w.ballot(flag[j]);
            w.each([&](int lane, int L) {
                const int lo = lane * tile_h - base;  // where the column starts in this word
                if (lane < tile_w && lo > -kPathMaxSide && lo < kPathMaxSide) open.v[L] |= lo >= 0 ? word >> lo : word << -lo;
            });
        }
    }
    const uint64_t column = tile_h < kPathMaxSide ? (uint64_t(1) << tile_h) - 1u : ~uint64_t(0);  // (a column's cells: the bits above are its neighbours')
    w.each([&](int lane, int L) {
        open.v[L] &= column;
        seen.v[L] = front.v[L] = lane == sx ? uint64_t(1) << sy : 0u;
        if (lane == sx) row[source] = 0;
    });
    for (int level = 1; w.ballot(front) != 0u; level++) {  // (each level with a cell adds it to `seen`: at most cells levels)
        const typename Wave::Board lower = w.from_lower(front), upper = w.from_upper(front);
        w.each([&](int lane, int L) {
            const uint64_t f = front.v[L];
            const uint64_t next = ((f << 1) | (f >> 1) | lower.v[L] | upper.v[L]) & open.v[L] & ~seen.v[L];
            seen.v[L] |= next;
            front.v[L] = next;
            for (uint64_t left = next; left; left &= left - 1) row[lane * tile_h + __builtin_ctzll(left)] = static_cast<int16_t>(level);
        });
    }
}

// What the probe cell sees of a finished row: its distance (-1: not reached, or no probe cell) and the step code — 0 where
// the distance is <= 0, else the first of x-1 (1), x+1 (2), y-1 (3), y+1 (4) whose distance is one less.
PG_HD void path_probe(const int16_t* row, int tile_w, int tile_h, int probe, int32_t& dist, uint8_t& step) {
    dist = probe >= 0 ? row[probe] : -1;
    step = 0;
    if (dist <= 0) return;
    const int px = probe / tile_h, py = probe - px * tile_h, want = dist - 1;
    if (px > 0 && row[probe - tile_h] == want) step = 1;
    else if (px < tile_w - 1 && row[probe + tile_h] == want) step = 2;
    else if (py > 0 && row[probe - 1] == want) step = 3;
    else if (py < tile_h - 1 && row[probe + 1] == want) step = 4;
}

// A game's tile maps as its read-only views take them (the tile rows of pg_state_obs.h, the path distances here): stated
// once per tile game, as the host function map(State) of its StateRow.  w and h need no bound state.
struct TileMaps {
    const uint8_t* tiles;  // [n][stride] bytes, a map in the first `cells` of each
    int stride, cells;
    int mask;              // what a tile byte is taken & with
    int w, h;
};

// pgv_tile_paths (include/procgen2_vec.h) with what the game knows of its map, as the kernel takes it.
struct TilePaths {
    const uint8_t* tiles;  // [n][stride] bytes, a map in the first `cells` of each
    uint32_t stride, cells, tile_mask;
    int tile_w, tile_h;
    uint32_t passable;
    int source, probe;  // kPath*
    const int32_t* source_cells;
    const int32_t* probe_cells;
    int16_t* dist;
    int32_t* probe_dist;
    uint8_t* probe_step;
    int32_t* cells_out;
    int n;
    const int32_t* indices;
    int count;
};
// (pgv_path_layout's part that a game states itself)
struct PathPoints {
    bool has_goal;
    float agent_dx, agent_dy;
};

#if defined(__HIPCC__)
// A game states beside its StateRow where its points are, as a `Points` type:
//     using Row;                 its StateRow: the agent's point is columns 0 and 1 of it
//     kAgentDy                   the centre of the agent's body box lies at (agent_x, agent_y + kAgentDy)
//     kGoalX, kGoalY             the columns of the goal's point; -1: the game has no goal.  A row whose dump is too short
//                                to hold them (caveflyer without entities) has no goal cell.
template <class Points>
__device__ __forceinline__ int path_point_cell(const typename Points::Row::State& s, const TilePaths& q, int kind, const int32_t* given,
                                                int row, int env) {
    using Row = typename Points::Row;
    if (kind == kPathAgent) return path_cell_of(Row::value(s, env, 0), Row::value(s, env, 1) + Points::kAgentDy, q.tile_w, q.tile_h);
    if (kind == kPathGoal) {
        if (Points::kGoalY < 0 || Points::kGoalY >= Row::length(s, env)) return -1;
        constexpr int gx = Points::kGoalX < 0 ? 0 : Points::kGoalX, gy = Points::kGoalY < 0 ? 0 : Points::kGoalY;
        return path_cell_of(Row::value(s, env, gx), Row::value(s, env, gy), q.tile_w, q.tile_h);
    }
    if (kind == kPathCells) return path_given_cell(given[row], static_cast<int>(q.cells));
    return -1;
}

template <class Points>
__global__ void __launch_bounds__(256) tile_paths_kernel(typename Points::Row::State s, TilePaths q) {
    extern __shared__ __attribute__((aligned(16))) int16_t path_stage[];  // 4 * cells + 8 int16s
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int first = static_cast<int>(blockIdx.x) * kPathGroupRows, row = first + wave;
    const int cells = static_cast<int>(q.cells);
    const size_t a = size_t(first) * q.cells;  // the group's first element of the flat output
    const uint32_t shift = static_cast<uint32_t>(a & 7u);
    int16_t* const mine = path_stage + shift + wave * cells;
    int source = -1, probe = -1;
    if (row < q.count) {  // (wave-uniform, as is everything below but `lane`)
        const int env = q.indices ? q.indices[row] : row;
        const uint8_t* tiles = nullptr;
        if (env >= 0 && env < q.n) {
            tiles = q.tiles + size_t(env) * q.stride;
            source = path_point_cell<Points>(s, q, q.source, q.source_cells, row, env);
            probe = path_point_cell<Points>(s, q, q.probe, q.probe_cells, row, env);
        }
        path_row(WaveLanes{lane}, tiles, q.tile_w, q.tile_h, q.tile_mask, q.passable, source, mine);
    }
    __syncthreads();
    if (row < q.count && lane == 0) {
        int32_t dist;
        uint8_t step;
        path_probe(mine, q.tile_w, q.tile_h, probe, dist, step);
        if (q.probe_dist) q.probe_dist[row] = dist;
        if (q.probe_step) q.probe_step[row] = step;
        if (q.cells_out) q.cells_out[2 * size_t(row)] = source, q.cells_out[2 * size_t(row) + 1] = probe;
    }
    if (!q.dist) return;
    // the staged rows are int16s [a, a + total) of the flat output; head .. tail is the part on the 16-byte grid
    const int here = q.count - first < kPathGroupRows ? q.count - first : kPathGroupRows;
    const uint32_t total = static_cast<uint32_t>(here) * q.cells;
    uint32_t head = (8u - shift) & 7u;
    if (head > total) head = total;
    const uint32_t vecs = (total - head) / 8u, tail = head + vecs * 8u;
    const int16_t* const staged = path_stage + shift;
    for (uint32_t v = tid; v < vecs; v += 256) {
        const uint32_t j = head + v * 8u;
        *reinterpret_cast<uint4*>(q.dist + a + j) = *reinterpret_cast<const uint4*>(staged + j);
    }
    if (tid < 16) {  // lanes 0-7: the int16s in front of the grid; 8-15: those behind it
        const uint32_t j = tid < 8 ? static_cast<uint32_t>(tid) : tail + static_cast<uint32_t>(tid - 8);
        if (tid < 8 ? j < head : j < total) q.dist[a + j] = staged[j];
    }
}

// (65 536 rows are 16 384 groups: one grid)
template <class Points>
void launch_tile_paths_of(hipStream_t st, const typename Points::Row::State& s, const TileMaps& m, int n, const TilePaths& asked) {
    static_assert(Points::kGoalX < Points::Row::kWidth && Points::kGoalY < Points::Row::kWidth, "the goal's columns");
    TilePaths q = asked;
    q.tiles = m.tiles, q.stride = static_cast<uint32_t>(m.stride), q.cells = static_cast<uint32_t>(m.cells);
    q.tile_mask = static_cast<uint32_t>(m.mask), q.tile_w = m.w, q.tile_h = m.h, q.n = n;
    const uint32_t groups = (static_cast<uint32_t>(q.count) + kPathGroupRows - 1u) / kPathGroupRows;  // (unsigned: any count up to INT_MAX)
    const size_t lds = ((size_t(kPathGroupRows) * q.cells + 8) * sizeof(int16_t) + 15) & ~size_t(15);
    hipLaunchKernelGGL(tile_paths_kernel<Points>, dim3(groups), dim3(256), lds, st, s, q);
}
template <class Points>
constexpr PathPoints path_points_of() {
    return {Points::kGoalY >= 0, 0.0f, Points::kAgentDy};
}
#endif

}  // namespace pg
