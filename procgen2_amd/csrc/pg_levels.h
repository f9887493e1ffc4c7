// Caller-made levels (include/procgen2_vec.h pgv_get_levels / pgv_set_levels): a level as a value — a tile row, the agent's
// and the goal's cell, the floor picture and its shift — read out of any envs and installed into any envs as the start of a
// new episode, on the device.
//
// A game states its level once, as a `Custom` type beside its State:
//     using State, using Level               the game's device view; one level as its generator leaves it (tiles first)
//     kW, kH, kStride, kBackgrounds           the map, the bytes between two envs' tile blocks, the floor pictures
//     kOpen, kPad                             the tile id an agent may stand on; the byte behind a level's cells
//     tiles(s)                                the live tile blocks, [n][kStride]
//     read(s, env, agent, goal, bg, shift)    the level of env as it stands, the points as cells
//     fill(lv, agent, goal, bg, shift)        the same fields into a Level whose tiles are in place
//     install(s, env, lv, lane)               lv becomes env's live state: the generator's own install()
// and set_levels_kernel<Custom> / get_levels_kernel<Custom> do the rest.  Only maze has one so far.
//
// Both kernels: one wavefront a row.  The caller's rows are kCells bytes apart — 225, 625, 961 — so a row's base is on no
// grid at all: the bytes in front of the first 4-byte boundary and behind the last go one at a time, the words between them
// as words (the address of the first such word is base + head, which is on the grid; the base itself is never taken for
// anything wider than a byte).  The env's side is kStride bytes apart and dense: words throughout.
//
// Install.  The row is staged in LDS as a Level — bytes from the caller's words, since head shifts them off the word grid of
// the stage — and judged there: a lane's verdict on its own bytes goes through a ballot, the points are looked up in the
// stage, and only a row that passes everything reaches the first store.  So a refused row writes its status and nothing
// else.  An accepted one claims its env (an atomic exchange on the call's claim words: of two rows that name one env the
// first to arrive is installed whole and the other is dropped), installs through the game's install(), and marks the env in
// the call's mask, which the engine hands to the render path and the other consumers of a masked reset.
// Bounds.  Row k < count; env = indices[k] is used only where 0 <= env < n.  The caller's row is read at k * kCells + c,
// c < kCells; a cell index is used only where 0 <= cell < kCells.  The stage is a Level: kStride >= kCells bytes of tiles.
// Offsets into the caller's buffers are size_t.
#pragma once

#include "pg_carve.h"
#include "pg_defs.h"

namespace pg {

// pgv_level_layout without its struct_size.
struct LevelLayout {
    int supported, cells, tile_w, tile_h, backgrounds;
};

// include/procgen2_vec.h pgv_set_levels: what a row's status says.
enum LevelStatus : int32_t {
    kLevelInstalled = 0,
    kLevelNoEnv = 1,
    kLevelBadTile = 2,
    kLevelBadAgent = 3,
    kLevelBadGoal = 4,
    kLevelBadFloor = 5,
};
constexpr uint8_t kLevelKnownCustom = 2;  // pgv_level_known: the caller's label

// pgv_level_rows with the indices: device pointers, any of which may be nullptr where the header says so.
struct LevelRows {
    const int32_t* indices;
    int count;
    uint8_t* tiles;
    int32_t* agent_cell;
    int32_t* goal_cell;
    int32_t* background;
    float* background_shift;
    uint32_t* ids;
    int32_t* status;
};

// What an install writes besides the game's state: the engine's rows and level words of the env, and the call's scratch.
struct LevelInstall {
    int n;
    float* reward;
    uint8_t* done;
    uint8_t* pending;
    uint32_t* number;  // LevelPlan::number, known
    uint8_t* known;
    uint32_t* claim;   // [n]  0, or 1 + the row that installs the env
    uint8_t* mask;     // [n]  1: installed by this call
};

// The engine's own block behind an install (pg_carve.h): zeroed in front of every call, as one range.
struct LevelBuffers {
    uint32_t* claim;  // [n]
    uint8_t* mask;    // [n]
};
inline void list_levels(Carve& c, LevelBuffers& b, int n) {
    c.take(b.claim, size_t(n) * 4);
    c.take(b.mask, size_t(n));
}

// (x, y) of a cell and back: cell = y + x * tile_h, y counted as the tile map counts it; a point's centre in world units.
PG_HD float level_point_x(int cell, int tile_h) { return static_cast<float>(cell / tile_h) + 0.5f; }
PG_HD float level_point_y(int cell, int tile_h) { return static_cast<float>(tile_h - 1 - cell % tile_h) + 0.5f; }
PG_HD bool level_shift_ok(float shift) { return shift >= 0.0f && shift < 1.0f; }  // (false for a NaN, and for ±inf)

#if defined(__HIPCC__)
template <class C>
__global__ void __launch_bounds__(64) set_levels_kernel(typename C::State s, LevelRows in, LevelInstall to) {
    constexpr int kCells = C::kW * C::kH;
    __shared__ typename C::Level lv;
    const int lane = threadIdx.x;
    const int k = static_cast<int>(blockIdx.x);  // (block-uniform from here on)
    int env = in.indices ? in.indices[k] : k;
    if (env < 0 || env >= to.n) {
        if (lane == 0 && in.status) in.status[k] = kLevelNoEnv;
        return;
    }
    // the caller's row into the stage, each lane judging the bytes it carries
    const uint8_t* row = in.tiles + size_t(k) * kCells;
    const int head = static_cast<int>((4u - static_cast<uint32_t>(reinterpret_cast<uintptr_t>(row) & 3u)) & 3u);
    const int words = (kCells - head) / 4, tail = head + words * 4;
    bool bad = false;
    const uint32_t* mid = reinterpret_cast<const uint32_t*>(row + head);
    for (int j = lane; j < words; j += 64) {
        const uint32_t w = mid[j];
        bad |= (w & 0xfefefefeu) != 0u;
        for (int b = 0; b < 4; b++) lv.tiles[head + 4 * j + b] = static_cast<uint8_t>(w >> (8 * b));
    }
    if (lane < 8) {  // lanes 0-3: the bytes in front of the words; 4-7: those behind them
        const int c = lane < 4 ? lane : tail + lane - 4;
        if (lane < 4 ? c < head : c < kCells) {
            const uint8_t v = row[c];
            bad |= v > 1u;
            lv.tiles[c] = v;
        }
    }
    for (int c = kCells + lane; c < C::kStride; c += 64) lv.tiles[c] = C::kPad;
    const bool bad_tile = __ballot(bad) != 0ull;
    __syncthreads();
    // the points and the floor (wave-uniform: every lane reads the same words)
    const int agent = in.agent_cell[k], goal = in.goal_cell[k];
    int now_agent, now_goal, bg;
    float shift;
    C::read(s, env, now_agent, now_goal, bg, shift);
    if (in.background) bg = in.background[k];
    if (in.background_shift) shift = in.background_shift[k];
    int32_t status = kLevelInstalled;
    if (bad_tile)
        status = kLevelBadTile;
    else if (agent < 0 || agent >= kCells || lv.tiles[agent] != C::kOpen)
        status = kLevelBadAgent;
    else if (goal < 0 || goal >= kCells || lv.tiles[goal] != C::kOpen || goal == agent)
        status = kLevelBadGoal;
    else if (bg < 0 || bg >= C::kBackgrounds || !level_shift_ok(shift))
        status = kLevelBadFloor;
    if (status == kLevelInstalled) {  // of two rows that name the env, the first to arrive
        uint32_t before = 0u;
        if (lane == 0) before = atomicExch(&to.claim[env], static_cast<uint32_t>(k) + 1u);
        before = __builtin_amdgcn_readfirstlane(before);
        if (before != 0u) {  // (dropped: the env holds the other row's level, and this row says so)
            if (lane == 0 && in.status) in.status[k] = kLevelInstalled;
            return;
        }
    }
    if (status != kLevelInstalled) {
        if (lane == 0 && in.status) in.status[k] = status;
        return;
    }
    if (lane == 0) C::fill(lv, agent, goal, bg, shift);
    __syncthreads();
    C::install(s, env, lv, lane);
    if (lane == 0) {
        to.number[env] = in.ids ? in.ids[k] : 0u;
        to.known[env] = kLevelKnownCustom;
        to.reward[env] = 0.0f;
        to.done[env] = 0;
        to.pending[env] = 0;
        to.mask[env] = 1;
        if (in.status) in.status[k] = kLevelInstalled;
    }
}

template <class C>
__global__ void __launch_bounds__(64) get_levels_kernel(typename C::State s, LevelRows out, int n) {
    constexpr int kCells = C::kW * C::kH;
    __shared__ uint32_t stage[C::kStride / 4];
    static_assert(C::kStride % 4 == 0 && C::kStride >= kCells, "an env's tile block is whole words");
    const int lane = threadIdx.x;
    const int k = static_cast<int>(blockIdx.x);
    int env = out.indices ? out.indices[k] : k;
    if (env < 0 || env >= n) env = -1;
    if (lane == 0) {
        int agent = -1, goal = -1, bg = 0;
        float shift = 0.0f;
        if (env >= 0) C::read(s, env, agent, goal, bg, shift);
        if (out.agent_cell) out.agent_cell[k] = agent;
        if (out.goal_cell) out.goal_cell[k] = goal;
        if (out.background) out.background[k] = bg;
        if (out.background_shift) out.background_shift[k] = shift;
    }
    if (!out.tiles) return;
    const uint32_t* src = env >= 0 ? reinterpret_cast<const uint32_t*>(C::tiles(s) + size_t(env) * C::kStride) : nullptr;
    for (int j = lane; j < C::kStride / 4; j += 64) stage[j] = src ? src[j] : 0u;
    __syncthreads();
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(stage);
    uint8_t* row = out.tiles + size_t(k) * kCells;
    const int head = static_cast<int>((4u - static_cast<uint32_t>(reinterpret_cast<uintptr_t>(row) & 3u)) & 3u);
    const int words = (kCells - head) / 4, tail = head + words * 4;
    uint32_t* mid = reinterpret_cast<uint32_t*>(row + head);
    for (int j = lane; j < words; j += 64) {
        const uint8_t* b = bytes + head + 4 * j;
        mid[j] = uint32_t(b[0]) | uint32_t(b[1]) << 8 | uint32_t(b[2]) << 16 | uint32_t(b[3]) << 24;
    }
    if (lane < 8) {
        const int c = lane < 4 ? lane : tail + lane - 4;
        if (lane < 4 ? c < head : c < kCells) row[c] = bytes[c];
    }
}

template <class C>
void launch_set_levels_of(hipStream_t st, const typename C::State& s, const LevelRows& in, const LevelInstall& to) {
    hipLaunchKernelGGL(set_levels_kernel<C>, dim3(static_cast<uint32_t>(in.count)), dim3(64), 0, st, s, in, to);
}
template <class C>
void launch_get_levels_of(hipStream_t st, const typename C::State& s, const LevelRows& out, int n) {
    hipLaunchKernelGGL(get_levels_kernel<C>, dim3(static_cast<uint32_t>(out.count)), dim3(64), 0, st, s, out, n);
}
template <class C>
constexpr LevelLayout level_layout_of() {
    return {1, C::kW * C::kH, C::kW, C::kH, C::kBackgrounds};
}
#endif

}  // namespace pg
