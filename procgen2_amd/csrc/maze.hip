// maze on gfx950: integer grid physics, randomised-Kruskal level generation.
//
// Reference:
//   step   games/maze/maze.cpp:279-330, common_systems.cpp:69-136
//   render games/maze/maze.cpp:386-414, tilemap.cpp:111-133, common_systems.cpp:41-63,138-150
//   reset  games/maze/maze.cpp:416-438, tilemap.cpp:31-109, maze_generator.cpp:55-139,183-195
// Config: one compiled variant per distribution mode (below); variant 0 = the reference's compile-time default,
// hard_mode: 25×25 world, all visible, fixed camera
// (maze/tilemap.h:40-42, tilemap.cpp:35-38).
// Machine mapping: logic one lane per env (SoA across envs), render two waves per env, level generation one wave per
// env on LDS.  The game draws no random numbers during an episode and every episode ends within 500 steps, so
// resets are frequent and bursty; the next maze of every env is carved ahead of time on a side stream and copied
// in at reset (pg_prefetch.h).
#include "pg_engine.h"
#include "pg_frame.h"
#include "pg_geom.h"
#include "pg_kruskal.h"
#include "pg_prefetch.h"
#include "pg_render.h"
#include "pg_prepass.h"
#include "pg_rng.h"
#include "pg_state_obs.h"

namespace pg {
namespace PG_VARIANT_NS {
namespace maze {

// tilemap.cpp:31-48: world side, visible side (the zoom, maze.cpp:397), camera on the agent or on the world centre
#if PG_VARIANT == 0  // hard_mode — the reference's compile-time default (tilemap.h:41)
constexpr int W = 25, kVisible = 25;
constexpr bool kCentred = false;
#elif PG_VARIANT == 1  // easy_mode
constexpr int W = 15, kVisible = 15;
constexpr bool kCentred = false;
#elif PG_VARIANT == 2  // memory_mode
constexpr int W = 31, kVisible = 8;
constexpr bool kCentred = true;
#else
#error "maze: unknown PG_VARIANT"
#endif
constexpr int H = W, kCells = W * H;
constexpr int kTileStride = (kCells + 127) / 128 * 128;  // 625 → 640
constexpr int kTimeout = 500;     // maze.cpp:49
enum Cell : uint8_t { kOpen = 0, kWall = 1 };

enum Tex { kTexWall = 0, kTexCheese = 1, kTexMouse = 2, kTexFloor = 3, kTexCount = 12 };

enum { F_AX, F_AY, F_GX, F_GY, F_BGSHIFT, F_CAMX, F_CAMY, F_COUNT };
enum { I_FLAGS, I_STEPS, I_BG, I_COUNT };
constexpr int kFlagForward = 1, kFlagListed = 2;

// One generated level, as the generator leaves it in LDS and as it waits in the shadow slot.
struct Level {
    uint8_t tiles[kTileStride];
    float ax, ay, gx, gy, bgshift;
    int32_t bg;
};

struct State {
    int n;
    Level* shadow;   // [n]  next level of each env (pg_prefetch.h)
    int32_t* slot;   // [n]  SlotState
    uint32_t* mt;    // [n][625]  generator chain: the stream position after the newest generated level
    uint8_t* tiles;  // [n][kTileStride], column-major y + x*H
    // !kCentred: the camera rests on the world centre and shows all of it, so the row composer's span and hand-over
    // tables are the same in every frame: worked out once (prepare_kernel), read from here (pg_render.h compose_prepare)
    ComposeHand* prepared;
    float* f;        // [F_COUNT][n]
    int32_t* i;      // [I_COUNT][n]
    // The render pre-pass's hand-over (scratch memory, not state): the frame's two draws and the background's two axes, worked
    // out by four lanes an env of a dense kernel (setup_kernel) instead of by 2 + 1 lanes of each of the env's two render
    // wavefronts — a quarter of what those executed.
    struct Prep {
        uint32_t* draws;  // [n][2][kBlitWords]  cheese, mouse (pg_render.h BlitWords; word 1 = 0: not drawn)
        uint32_t* bg;     // [n][8]              background, x axis then y axis: d0 | dn << 16, s0 | sn << 16, first texel, width
    } prep;
};

PG_D float& SF(const State& s, int field, int env) { return s.f[size_t(field) * s.n + env]; }
PG_D int32_t& SI(const State& s, int field, int env) { return s.i[size_t(field) * s.n + env]; }

PG_D int tile_at(const uint8_t* t, int x, int y) {
    if (x < 0 || y < 0 || x >= W || y >= H) return kWall;  // maze/tilemap.h:79-84
    return t[y + x * H];
}

using MazeLds = KruskalLdsT<(W > 25 ? W : 25)>;
struct GenLds {
    uint32_t mt[kMtWords];
    MazeLds k;
};

// reset() (maze.cpp:416-438 + tilemap.cpp:31-109) for one env by one wavefront: advances the env's generator chain
// (s.mt) and leaves the level in `lv` (LDS).
PG_D void generate(const State& s, int env, GenLds& L, Level& lv, bool reseed, uint32_t seed, int lane) {
    uint32_t* gmt = s.mt + size_t(env) * kMtWords;
    if (reseed) {
        if (lane == 0) mt_seed(L.mt, seed);
    } else {
        for (int k = lane; k < kMtWords; k += 64) L.mt[k] = gmt[k];
    }
    for (int k = lane; k < kTileStride; k += 64) lv.tiles[k] = kWall;
    __syncthreads();
    uint32_t* mt = L.mt;
    const int dim = wave_rng_int(mt, 0, (W - 1) / 2 - 1, lane) * 2 + 3;
    const int margin = (W - dim) / 2;
    CarverT<MazeLds> carver{L.k, 0, 0, 0, 0};
    carver.carve(dim, mt, lane);
    carver.drop(2, mt, lane);
    for (int c = lane; c < dim * dim; c += 64) {
        const int a = c / dim, b = c % dim;
        const int t = carver.get(a + 1, b + 1);
        lv.tiles[(b + margin) + (a + margin) * H] = (t == 1) ? kWall : kOpen;
        if (t == 2) {
            lv.gx = static_cast<float>(a + margin) + 0.5f;
            lv.gy = static_cast<float>(H - 1 - (b + margin)) + 0.5f;
        }
    }
    const int bg = wave_rng_int(mt, 0, 8, lane);
    const float shift = wave_rng_real(mt, 0.0f, 1.0f, lane);
    if (lane == 0) {
        lv.ax = static_cast<float>(margin) + 0.5f;
        lv.ay = static_cast<float>(H - 1 - margin) + 0.5f;
        lv.bg = bg;
        lv.bgshift = shift;
    }
    __syncthreads();
    for (int k = lane; k < kMtWords; k += 64) gmt[k] = L.mt[k];
    __syncthreads();
}

// The level becomes the env's live state.
PG_D void install(const State& s, int env, const Level& lv, int lane) {
    uint32_t* tiles = reinterpret_cast<uint32_t*>(s.tiles + size_t(env) * kTileStride);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(lv.tiles);
    for (int k = lane; k < kTileStride / 4; k += 64) tiles[k] = src[k];
    if (lane == 0) {
        SF(s, F_GX, env) = lv.gx;
        SF(s, F_GY, env) = lv.gy;
        SF(s, F_AX, env) = lv.ax;
        SF(s, F_AY, env) = lv.ay;
        SI(s, I_STEPS, env) = 0;
        SI(s, I_BG, env) = lv.bg;
        SF(s, F_BGSHIFT, env) = lv.bgshift;
        SI(s, I_FLAGS, env) = kFlagForward;  // face_forward = true; draw list cleared (D2)
        SF(s, F_CAMX, env) = W * 0.5f * kUnitPx;  // maze.cpp:436-437
        SF(s, F_CAMY, env) = H * 0.5f * kUnitPx;
    }
}

// What cenv_make leaves in an env besides the seeded RNG, split by owner: the generator chain (bucket counts of
// the sets that survive clear()) and the live state.  Level-seed mode (pg_engine.h LevelPlan) rebuilds every
// level from here.
PG_D void fresh_chain(const State& s, int env) {
}
PG_D void fresh_live(const State& s, int env) {
}

struct Gen {  // pg_prefetch.h level_kernel<Gen>
    using State = maze::State;
    using Level = maze::Level;
    using GenLds = maze::GenLds;
    PG_D static void generate(const State& s, int env, GenLds& L, Level& lv, bool reseed, uint32_t seed, int lane) {
        maze::generate(s, env, L, lv, reseed, seed, lane);
    }
    PG_D static void install(const State& s, int env, const Level& lv, int lane) { maze::install(s, env, lv, lane); }
    PG_D static void fresh_chain(const State& s, int env) { maze::fresh_chain(s, env); }
    PG_D static void fresh_live(const State& s, int env) { maze::fresh_live(s, env); }
};

PG_D void advance(const State& s, int env, int action, float& reward_out, bool& terminated_out) {
    const uint8_t* tiles = s.tiles + size_t(env) * kTileStride;
    float ax = SF(s, F_AX, env), ay = SF(s, F_AY, env);
    int flags = SI(s, I_FLAGS, env);
    const int mx = action / 3 - 1;  // actions 9..14 give 2/3-cell jumps (D6)
    const int my = mx ? 0 : -(action % 3 - 1);
    if (mx) {
        if (tile_at(tiles, static_cast<int>(ax + mx), H - 1 - static_cast<int>(ay)) == kOpen)
            ax = static_cast<int>(ax + mx) + 0.5f;
    } else if (my) {
        if (tile_at(tiles, static_cast<int>(ax), H - 1 - static_cast<int>(ay + my)) == kOpen)
            ay = static_cast<int>(ay + my) + 0.5f;
    }
    const Box body{ax + -0.5f, ay + -0.5f, 1.0f, 1.0f};
    const Box goal{SF(s, F_GX, env) + -0.5f, SF(s, F_GY, env) + -0.5f, 1.0f, 1.0f};
    const bool reached = box_hit(body, goal);
    if (mx > 0)
        flags |= kFlagForward;
    else if (mx < 0)
        flags &= ~kFlagForward;
    flags |= kFlagListed;
    const int steps = SI(s, I_STEPS, env) + 1;
    SF(s, F_AX, env) = ax;
    SF(s, F_AY, env) = ay;
    if (kCentred) {  // common_systems.cpp:119-123: the camera follows the agent
        SF(s, F_CAMX, env) = ax * kUnitPx;
        SF(s, F_CAMY, env) = ay * kUnitPx;
    }
    SI(s, I_FLAGS, env) = flags;
    SI(s, I_STEPS, env) = steps;
    reward_out = reached * 10.0f;
    terminated_out = reached || steps >= kTimeout;  // maze.cpp:302-310: the cap sets `terminated` (D5)
}

struct Step {  // pg_prefetch.h logic_step<Gen, Step>: a lane per env, nothing in LDS
    static constexpr int kGang = 1;
    struct Lds {};
    PG_D static void advance(const State& s, Lds&, int, int env, int action, float& reward, bool& terminated) {
        maze::advance(s, env, action, reward, terminated);
    }
};

__global__ void __launch_bounds__(64) logic_kernel(State s, const int32_t* actions, uint32_t run_seed,
                                                   uint32_t step_index, int env_offset, StepIO io, int prefetch, LevelPlan plan) {
    logic_step<Gen, Step>(s, actions, run_seed, step_index, env_offset, io, prefetch, plan);
}

constexpr int kGrid = kVisible + 3 <= 20 ? 20 : 28;  // visible tiles + the border cells of the inclusive window; as small as it
// may be: the composer tables are LDS, and LDS decides how many envs a CU holds (28: 7 per CU, 32: 6)
constexpr int kSpan = 64 / kVisible + 2 <= kMaxSpan ? kMaxSpan : 16;  // pixels a tile covers (+ seam padding)

// the wall window of a camera (tilemap.cpp:111-121)
struct Window {
    int x0, y0, cols, rows;
};
PG_D Window window_of(const Camera& cam) {
    const TileWindow w = tile_window(cam);
    return Window{w.x0, w.y0, w.x1 - w.x0 + 1, w.y1 - w.y0 + 1};
}
// The draw list of maze.cpp:402-420 after the walls, each kind of draw stated once, for setup_kernel, render_kernel and
// frame_draws, given the texture's descriptor (y: width): the cheese sprite (tilemap.cpp:88: offset (-0.48,-0.5), scale
// 0.95, z = 1), once it is listed; the mouse (common_systems.cpp:138-150), flipped when it faces forward.
PG_D DrawCall cheese_draw(int sflags, float gx, float gy, const int4& d) {
    const float scale = 1.0f * 0.95f;
    return DrawCall{(sflags & kFlagListed) != 0, false, false, kTexCheese, (gx + -0.48f) * kUnitPx, (gy + -0.5f) * kUnitPx,
                    scale * kUnitPx / d.y, 1.0f, 0.0f};
}
PG_D DrawCall mouse_draw(int sflags, float ax, float ay, const int4& d) {
    return DrawCall{true, (sflags & kFlagForward) != 0, false, kTexMouse, (ax + -0.5f) * kUnitPx, (ay + -0.5f) * kUnitPx,
                    kUnitPx / d.y * 1.0f, 1.0f, 0.0f};
}
PG_D float zoom_of_obs() { return 64.0f / (kUnitPx * static_cast<float>(kVisible)); }  // maze.cpp:397-400

// Once per engine (!kCentred): the composer's tables for the camera on the world centre (State::prepared).
__global__ void __launch_bounds__(128) prepare_kernel(State s, AtlasView atlas) {
    __shared__ alignas(16) uint32_t fb[kFbWords];
    __shared__ ComposeLds<kGrid> L;
    const int lane = threadIdx.x & 63, half = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const Camera cam{W * 0.5f * kUnitPx, H * 0.5f * kUnitPx, 64.0f, 64.0f, zoom_of_obs()};  // maze.cpp:436-437
    const Window w = window_of(cam);
    const int4 wall = atlas.desc[kTexWall];
    compose_spans<kGrid, kSpan>(fb, L, cam, w.x0, w.y0, w.cols, w.rows, wall.y, wall.z, kUnitPx / wall.y, lane, 0, half, 2,
                                soft_rows_of(0, wall.w), hard_rows_of(0, wall.w));
    __syncthreads();
    compose_hand_build<kGrid, false, false>(fb, L, BgAxis{}, wall.y, lane, 0, half, make_int4(0, -1, 0, -1));
    compose_prepare<kGrid>(fb, L, s.prepared, lane, half);
}

// flags bit 0: force the draw-list replay for background + walls (fallback path).
// The render pre-pass: four lanes an env — cheese, mouse (tilemap.cpp:88, common_systems.cpp:138-150 as render_kernel states
// them), the background's x and y axis (maze.cpp:402-408; pg_render.h bg_axis).
__global__ void __launch_bounds__(256) setup_kernel(State s, AtlasView atlas) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int env = gid >> 2, item = gid & 3;
    if (env >= s.n) return;
    const Camera cam{kCentred ? SF(s, F_CAMX, env) : W * 0.5f * kUnitPx, kCentred ? SF(s, F_CAMY, env) : H * 0.5f * kUnitPx,
                     64.0f, 64.0f, zoom_of_obs()};
    if (item < 2) {
        const bool cheese = item == 0;
        const int sflags = SI(s, I_FLAGS, env);
        const int4 d = atlas.desc[cheese ? kTexCheese : kTexMouse];
        const DrawCall c = cheese ? cheese_draw(sflags, SF(s, F_GX, env), SF(s, F_GY, env), d) : mouse_draw(sflags, SF(s, F_AX, env), SF(s, F_AY, env), d);
        bool has = c.go;
        Blit b;
        if (has) has = resolve_draw(cam, d.y, d.z, d.x, c.wx, c.wy, c.scale, 1.0f, c.flip_h, false, b);
        BlitWords w{};
        if (has) w = blit_pack(b);
        uint2* at = reinterpret_cast<uint2*>(s.prep.draws + (size_t(env) * 2 + item) * kBlitWords);
        at[0] = make_uint2(w.w[0], w.w[1]);
        at[1] = make_uint2(w.w[2], w.w[3]);
        at[2] = make_uint2(w.w[4], w.w[5]);
    } else {
        const int axis = item - 2;
        const int4 d = atlas.desc[kTexFloor + SI(s, I_BG, env)];
        const BgDraw bg = backdrop_draw(d, SF(s, F_BGSHIFT, env));
        const BgAxis a = bg_axis(cam, d, bg.px, bg.py, bg.scale, axis);
        uint4* at = reinterpret_cast<uint4*>(s.prep.bg + size_t(env) * 8 + axis * 4);
        *at = make_uint4(pack_halves(a.d0, a.dn), pack_halves(a.s0, a.sn), static_cast<uint32_t>(a.tex_off), static_cast<uint32_t>(a.tex_w));
    }
}

// kPrepped: the two draws and (camera at rest) the background's axes come from the pre-pass; false: the debug paths.
template <bool kPrepped>
__global__ void __launch_bounds__(128, 4) render_kernel(State s, AtlasView atlas, const uint8_t* mask, StepIO io,
                                                    int flags) {
    const int env = blockIdx.x;
    if (mask && !mask[env]) return;
    const int lane = threadIdx.x & 63, half = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // two wavefronts per env (pg_render.h)
    constexpr int halves = 2;
    __shared__ alignas(16) uint32_t fb[kFbWords];
    __shared__ ComposeLds<kGrid> L;

    // maze.cpp:397-400, 436-437: zoom = 64 / (16 * visible_width); camera at the world centre, or on the agent
    const float zoom = zoom_of_obs();
    const Camera cam{kCentred ? SF(s, F_CAMX, env) : W * 0.5f * kUnitPx, kCentred ? SF(s, F_CAMY, env) : H * 0.5f * kUnitPx,
                     64.0f, 64.0f, zoom};
    const int sflags = SI(s, I_FLAGS, env);
    const uint8_t* tiles = s.tiles + size_t(env) * kTileStride;
    Blit mine;

    int bg_soft = 0;  // the backdrop has texels that are not opaque (descriptor .w)
    // the background draw (maze.cpp:402-408) — each wave resolves the axis it needs (pg_render.h BgAxis)
    const BgDraw bg_draw = backdrop_draw(atlas.desc[kTexFloor + SI(s, I_BG, env)], SF(s, F_BGSHIFT, env));
    const int4& bg_d = bg_draw.desc;
    const float bg_px = bg_draw.px, bg_py = bg_draw.py, bg_sc = bg_draw.scale;
    bg_soft = bg_d.w;
    const Window win = window_of(cam);
    const int x0 = win.x0, y0 = win.y0, cols = win.cols, rows = win.rows, cells = cols * rows;
    const int4 wall = atlas.desc[kTexWall];

    BgAxis bga{};  // this wave's axis of it (wave 0: x, wave 1: y), resolved along with the tile spans
    bool composed = false;
    if (!(flags & 1) && cols <= kGrid && rows <= kGrid) {
        if (kCentred) {
            compose_spans<kGrid, kSpan>(fb, L, cam, x0, y0, cols, rows, wall.y, wall.z, kUnitPx / wall.y, lane, 0, half, halves,
                                        soft_rows_of(bg_soft, wall.w), hard_rows_of(bg_soft, wall.w), &bg_draw, &bga);
        } else {  // the tile spans are the prepared ones: only this wave's axis of the background is resolved
            if (kPrepped) {
                const uint32_t* w = s.prep.bg + size_t(env) * 8 + half * 4;
                bga = BgAxis{static_cast<int32_t>(w[0] << 16) >> 16, static_cast<int32_t>(w[0]) >> 16, static_cast<int32_t>(w[1] & 0xffffu),
                             static_cast<int32_t>(w[1] >> 16), static_cast<int32_t>(w[2]), static_cast<int32_t>(w[3])};
            } else {
                bga = bg_axis(cam, bg_d, bg_px, bg_py, bg_sc, half);
            }
            if (half == 0 && lane < 2) L.base[kGrid * kGrid + lane] = static_cast<int32_t>(kNoTexel);
        }
        for (int cell = lane + 64 * half; cell < cells; cell += 64 * halves) {
            const int r = cell / cols, c = cell - r * cols;
            L.base[r * kGrid + c] =
                tile_at(tiles, x0 + c, H - 1 - (y0 + r)) == kOpen ? static_cast<int32_t>(kNoTexel) : wall.x * 4;
        }
        __syncthreads();
        composed = kCentred ? compose_rows<kGrid>(fb, L, atlas, bga, cols, rows, wall.y, lane, flags, half, halves)
                            : compose_rows<kGrid, false, false, true>(fb, L, atlas, bga, cols, rows, wall.y, lane, flags, half, halves,
                                                                      make_int4(0, -1, 0, -1), s.prepared, bg_soft);
    }
    if (!composed) {  // draw-list replay (tilemap.cpp:111-133)
        wave_clear(fb, lane, half, halves);
        const bool has_bg = resolve_draw(cam, bg_d.y, bg_d.z, bg_d.x, bg_px, bg_py, bg_sc, 1.0f, false, false, mine);
        wave_replay(fb, atlas, mine, has_bg ? 1ull : 0ull, lane, half, halves);
        for (int base = 0; base < cells; base += 64) {
            const int cell = base + lane;
            bool has = false;
            if (cell < cells) {
                const int row = cell / cols;
                const int x = x0 + (cell - row * cols), y = y0 + row;
                if (tile_at(tiles, x, H - 1 - y) != kOpen)
                    has = resolve_draw(cam, wall.y, wall.z, wall.x, x * kUnitPx, y * kUnitPx, kUnitPx / wall.y, 1.0f,
                                       false, false, mine);
            }
            wave_replay(fb, atlas, mine, __ballot(has), lane, half, halves);
        }
    }
    if (kPrepped) {  // lane 0: the cheese, lane 1: the mouse, as the pre-pass resolved them
        mine = prep_draw_load(s.prep.draws + (size_t(env) * 2 + (lane & 1)) * kBlitWords, lane < 2);
        wave_replay_rows(fb, atlas, mine, __ballot(lane < 2 && mine.dw > 0), lane, half * (kObsH / halves), (half + 1) * (kObsH / halves));
    } else {
        // lane 0: the cheese sprite (tilemap.cpp:88): offset (-0.48,-0.5), scale 0.95, z = 1, once it is listed;
        // lane 1: the mouse (common_systems.cpp:138-150); flip = face_forward.  The two differ in their parameters
        // only: one pass through resolve_draw, one replay, in this order.
        const bool cheese = lane == 0;
        const int4 d = atlas.desc[cheese ? kTexCheese : kTexMouse];
        const DrawCall c = cheese ? cheese_draw(sflags, SF(s, F_GX, env), SF(s, F_GY, env), d) : mouse_draw(sflags, SF(s, F_AX, env), SF(s, F_AY, env), d);
        bool has = c.go && lane < 2;
        if (has) has = resolve_draw(cam, d.y, d.z, d.x, c.wx, c.wy, c.scale, 1.0f, c.flip_h, false, mine);
        wave_replay_rows(fb, atlas, mine, __ballot(has), lane, half * (kObsH / halves), (half + 1) * (kObsH / halves));
    }
    // each wave stores the rows it owns (pg_render.h wave_replay_rows): no barrier
    wave_store_rows(fb, io.obs + size_t(env) * kObsBytes, lane, half * (kObsH / halves), (half + 1) * (kObsH / halves));
}

// cenv_render's frame (render_game(false)): the draw list of render_kernel, one draw at a time, for either painter of pg_frame.h.
template <class Painter>
__device__ void frame_draws(const State& s, const AtlasView& atlas, int env, Painter& P) {
    const float fw = P.width(), fh = P.height();
    const float zoom = fw / (kUnitPx * static_cast<float>(kVisible));  // maze.cpp:397-400
    P.begin(atlas, Camera{SF(s, F_CAMX, env), SF(s, F_CAMY, env), fw, fh, zoom});
    const int sflags = SI(s, I_FLAGS, env);
    const uint8_t* tiles = s.tiles + size_t(env) * kTileStride;
    P.clear();
    const int floor_tex = kTexFloor + SI(s, I_BG, env);
    const BgDraw bg = backdrop_draw(P.desc(floor_tex), SF(s, F_BGSHIFT, env));
    P.draw(floor_tex, bg.px, bg.py, bg.scale);
    const TileWindow win = P.window();
    for (int y = win.y0; y <= win.y1; y++)
        for (int x = win.x0; x <= win.x1; x++)
            if (tile_at(tiles, x, H - 1 - y) != kOpen) P.draw(kTexWall, x * kUnitPx, y * kUnitPx, kUnitPx / P.desc(kTexWall).y);
    P.draw(cheese_draw(sflags, SF(s, F_GX, env), SF(s, F_GY, env), P.desc(kTexCheese)));
    P.draw(mouse_draw(sflags, SF(s, F_AX, env), SF(s, F_AY, env), P.desc(kTexMouse)));
}

struct Frames {  // pg_frame.h frame_kernel<Frames> / frames_kernel<Frames>
    using State = maze::State;
    template <class Painter>
    static __device__ void draws(const State& s, const AtlasView& atlas, int env, Painter& P) { frame_draws(s, atlas, env, P); }
};

// The state row (pg_state_obs.h): oracle/pgo_maze.cpp Maze::dump_state, column by column.  Every source is a field array.
struct StateRow {
    using State = maze::State;
    static constexpr int kFixed = 10, kRecord = 0, kMaxRecords = 0, kWidth = kFixed, kEnvCols = kWidth;
    static __device__ int length(const State&, int) { return kFixed; }
    static __device__ float value(const State& s, int env, int col) {
        switch (col) {
            case 0: return SF(s, F_AX, env);
            case 1: return SF(s, F_AY, env);
            case 2: return (SI(s, I_FLAGS, env) & kFlagForward) ? 1.0f : 0.0f;
            case 3: return SF(s, F_GX, env);
            case 4: return SF(s, F_GY, env);
            case 5: return static_cast<float>(SI(s, I_STEPS, env));
            case 6: return static_cast<float>(SI(s, I_BG, env));
            case 7: return SF(s, F_BGSHIFT, env);
            case 8: return SF(s, F_CAMX, env);
            default: return SF(s, F_CAMY, env);
        }
    }
    static std::string names() { return "agent_x agent_y agent_forward goal_x goal_y steps floor floor_shift cam_x cam_y|"; }
    static TileMaps map(const State& s) { return {s.tiles, kTileStride, kCells, 0xff, W, H}; }
};

// The points of the path distances (pg_paths.h): the mouse fills its cell; the goal is the cheese.
struct PathRow {
    using Row = StateRow;
    static constexpr float kAgentDy = 0.0f;
    static constexpr int kGoalX = 3, kGoalY = 4;
};

// A level as a value (pg_levels.h): `Level` is all of it.  The floor pictures are the nine generate() draws from.
struct Custom {
    using State = maze::State;
    using Level = maze::Level;
    static constexpr int kW = W, kH = H, kStride = kTileStride, kBackgrounds = 9;
    static constexpr uint8_t kOpen = maze::kOpen, kPad = kWall;  // (generate() fills the whole block with walls first)
    static __device__ const uint8_t* tiles(const State& s) { return s.tiles; }
    static __device__ void read(const State& s, int env, int& agent, int& goal, int& bg, float& shift) {
        agent = path_cell_of(SF(s, F_AX, env), SF(s, F_AY, env), W, H);
        goal = path_cell_of(SF(s, F_GX, env), SF(s, F_GY, env), W, H);
        bg = SI(s, I_BG, env);
        shift = SF(s, F_BGSHIFT, env);
    }
    static __device__ void fill(Level& lv, int agent, int goal, int bg, float shift) {
        lv.ax = level_point_x(agent, H);
        lv.ay = level_point_y(agent, H);
        lv.gx = level_point_x(goal, H);
        lv.gy = level_point_y(goal, H);
        lv.bg = bg;
        lv.bgshift = shift;
    }
    static __device__ void install(const State& s, int env, const Level& lv, int lane) { maze::install(s, env, lv, lane); }
};

class MazeGame final : public ViewedGame<PrefetchingGame<Gen>, StateRow, PathRow, Frames> {
   public:
    const char* name() const override { return "maze"; }
    std::vector<std::string> texture_names() const override {
        std::vector<std::string> v = {"kenney/Ground/Sand/sandCenter.png", "misc_assets/cheese.png",
                                      "kenney/Enemies/mouse_move.png", "topdown_backgrounds/floortiles.png"};
        for (int k = 1; k <= 8; k++) v.push_back("topdown_backgrounds/backgrounddetailed" + std::to_string(k) + ".png");
        return v;
    }
    // The state block, in order (state_bytes and bind).
    static void carve(Carve& c, State& s, int n) {
        c.take_env(s.shadow, n, 1, sizeof(Level));
        c.take_env(s.slot, n, 1, 4);
        c.take_env(s.mt, n, 1, kMtWords * 4);
        c.take_env(s.tiles, n, 1, kTileStride);
        c.take_env(s.f, n, F_COUNT, 4);
        c.take_env(s.i, n, I_COUNT, 4);
        c.take_shared(s.prepared, sizeof(ComposeHand));
    }
    size_t state_bytes(int n) const override { return Carve::size(carve, n); }
    void bind(void* d_state, int n, AtlasView atlas) override {
        Carve::bind(carve, d_state, s_, n, &regions);
        s_.n = n;
        atlas_ = atlas;
    }
    void launch_make(hipStream_t st, uint32_t seed_base, int env_offset) override {
        make_levels<false>(st, seed_base, env_offset);  // (fresh_chain and fresh_live, above, leave nothing)
        if (!kCentred) hipLaunchKernelGGL(prepare_kernel, dim3(1), dim3(128), 0, st, s_, atlas_);
    }
    int pregen_every() const override { return 2; }  // (pg_engine.h)
    void launch_logic(hipStream_t st, const int32_t* actions, uint32_t run_seed, uint32_t step_index, int env_offset,
                      StepIO io) override {
        launch_fused_logic(logic_kernel, Step::kGang, st, actions, run_seed, step_index, env_offset, io);
    }
    // (the draw-list replay and kDebugNoPrepass take the kernel that resolves its own draws)
    bool lean() const { return !(debug_flags & (1 | kDebugNoPrepass)); }
    void launch_prepass(hipStream_t st, const uint8_t* mask) override {
        (void)mask;  // (every env: a lane's work, and the frames of the others are not drawn)
        if (lean()) hipLaunchKernelGGL(setup_kernel, dim3((s_.n * 4 + 255) / 256), dim3(256), 0, st, s_, atlas_);
    }
    void launch_render(hipStream_t st, const uint8_t* mask, StepIO io) override {
        if (lean())
            hipLaunchKernelGGL(render_kernel<true>, dim3(s_.n), dim3(128), 0, st, s_, atlas_, mask, io, debug_flags);
        else
            hipLaunchKernelGGL(render_kernel<false>, dim3(s_.n), dim3(128), 0, st, s_, atlas_, mask, io, debug_flags);
    }
    static void carve_scratch(Carve& c, State::Prep& p, int n) {
        c.take(p.draws, size_t(n) * 2 * kBlitWords * 4);
        c.take(p.bg, size_t(n) * 8 * 4);
    }
    size_t scratch_bytes(int n) const override { return Carve::size(carve_scratch, n); }
    void bind_scratch(void* d_scratch, int n) override { Carve::bind(carve_scratch, d_scratch, s_.prep, n); }
    LevelLayout level_layout() const override { return level_layout_of<Custom>(); }
    void launch_get_levels(hipStream_t st, const LevelRows& out) override { launch_get_levels_of<Custom>(st, s_, out, s_.n); }
    void launch_set_levels(hipStream_t st, const LevelRows& in, const LevelInstall& to) override {
        launch_set_levels_of<Custom>(st, s_, in, to);
    }
};

}  // namespace maze

}  // namespace PG_VARIANT_NS

std::unique_ptr<Game> PG_FACTORY(make_maze)() { return std::make_unique<PG_VARIANT_NS::maze::MazeGame>(); }

}  // namespace pg
