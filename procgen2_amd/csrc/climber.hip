// climber on gfx950: vertical platformer, patrol mobs, collectible crystals.
//
// Reference:
//   step   games/climber/climber.cpp:323-376, common_systems.cpp:184-270 (agent), :109-168 (mobs), :66-107 (points),
//          :8-39 (sprite list)
//   render games/climber/climber.cpp:431-459, tilemap.cpp:172-198, common_systems.cpp:41-63, :272-298
//   reset  games/climber/climber.cpp:461-497, tilemap.cpp:40-70, :75-170
// Config = the reference's compile-time default (easy_mode = false, climber/tilemap.h:32-34).
//
// Machine mapping as in coinrun.hip: logic one lane per env over struct-of-arrays state, render one wavefront per
// env.  Collected crystals are destroyed entities in the reference: they leave the sprite System's
// std::unordered_set, and the z-sorted draw list is rebuilt from that set every sub-step.  Erasing from the
// libstdc++ node list keeps the relative order of the survivors, so the device keeps the episode's insertion-built
// order (pg_order.h, computed at reset) plus an alive bit per entity, and re-runs the introsort emulation over the
// survivors whenever the set changed.
#include "pg_engine.h"
#include "pg_frame.h"
#include "pg_gang.h"
#include "pg_geom.h"
#include "pg_order.h"
#include "pg_prefetch.h"
#include "pg_prepass.h"
#include "pg_render.h"
#include "pg_rng.h"
#include "pg_state_obs.h"
#include "pg_tiles.h"

namespace pg {
namespace PG_VARIANT_NS {
namespace climber {

// climber/tilemap.cpp:118 `enemy_prob = cfg.easy_mode ? .2 : .5` (tilemap.h:33: easy_mode = false is the default)
#if PG_VARIANT == 0
constexpr float kEnemyProb = 0.5f;
#elif PG_VARIANT == 1  // easy_mode
constexpr float kEnemyProb = 0.2f;
#else
#error "climber: unknown PG_VARIANT"
#endif

constexpr int W = 20, H = 64;
constexpr int kMaxEnt = 34, kEntStride = 48;  // ≤ 17 platforms (difficulty 3), each at most one mob and one crystal (tilemap.cpp:98-105)
enum Tile : uint8_t { kEmpty = 0, kWallTop, kWallMid };  // tilemap.h:12-17

enum Tex {
    kTexTop = 0,    // 4 themes
    kTexMid = 4,    // 4 themes
    kTexStand = 8,  // 4 suits each
    kTexJump = 12,
    kTexWalk1 = 16,
    kTexWalk2 = 20,
    kTexFish = 24,  // 2 frames
    kTexGem = 26,
    kTexBackdrop = 27,  // 10
    kTexCount = 37
};

enum { F_AX, F_AY, F_AVX, F_AVY, F_APHASE, F_CAMY, F_BGSHIFT, F_COUNT };
enum { I_FLAGS, I_THEMES, I_NENT, I_NDRAW, I_HASH_SPRITE, I_COUNT };
constexpr int kFlagGround = 1, kFlagForward = 2, kFlagListed = 4;
enum { EF_X, EF_Y, EF_VX, EF_ANIM_T, EF_COUNT };
enum { EB_INFO, EB_SPAWN_X, EB_ORDER, EB_DRAW, EB_COUNT };
// EB_INFO bits
constexpr int kMob = 1, kAlive = 2, kFrame = 4, kFlip = 8, kTexSet = 16;

// One generated level, as the generator leaves it in LDS and as it waits in the shadow slot (pg_prefetch.h).
struct Level {
    uint8_t tiles[W * H];
    float bgshift;
    int32_t themes, n_ent;
    float ex[kMaxEnt], ey[kMaxEnt], evx[kMaxEnt];
    uint8_t info[kMaxEnt], spawn_x[kMaxEnt], order[kMaxEnt];
    uint8_t pad[2];
};

struct GenLds {
    uint32_t mt[kMtWords];
};

struct State {
    int n;
    Level* shadow;   // [n]  next level of each env
    int32_t* slot;   // [n]  SlotState
    uint32_t* mt;    // [n][625]  generator chain: the stream position after the newest generated level
    uint8_t* tiles;  // [n][1280]  column-major y + x*H
    float* f;        // [F_COUNT][n]
    int32_t* i;      // [I_COUNT][n]
    float* ef;       // [n][EF_COUNT][kEntStride]  per-env contiguous: a gang's and the render wavefronts' lanes index them by entity
    uint8_t* eb;     // [n][EB_COUNT][kEntStride]
    const uint8_t* ranks;  // pg_order.h equal-key sort ranks
    PrepOut prep;          // what setup_kernel leaves for render_kernel (pg_prepass.h); not part of the state blob
};

PG_D float& SF(const State& s, int field, int env) { return s.f[size_t(field) * s.n + env]; }
PG_D int32_t& SI(const State& s, int field, int env) { return s.i[size_t(field) * s.n + env]; }
PG_D float& EF(const State& s, int field, int e, int env) { return s.ef[(size_t(env) * EF_COUNT + field) * kEntStride + e]; }
PG_D uint8_t& EB(const State& s, int field, int e, int env) { return s.eb[(size_t(env) * EB_COUNT + field) * kEntStride + e]; }

using Win = TileWinT<W, H, kWallMid>;  // out of bounds is a wall (tilemap.h:66-68)

// Tile writes by the whole wavefront into the map under construction (LDS); later fills overwrite earlier ones, so
// each ends with a barrier.
PG_D void fill(uint8_t* t, int x, int y, int w, int h, int id, int lane) {
    const int total = (w > 0 && h > 0) ? w * h : 0;
    for (int k = lane; k < total; k += 64) {
        const int a = udiv_small(k, h), b = k - a * h;
        const int px = x + a, py = y + b;
        if (!(px < 0 || py < 0 || px >= W || py >= H)) t[py + px * H] = static_cast<uint8_t>(id);
    }
    __syncthreads();
}
PG_D void fill_capped(uint8_t* t, int x, int y, int w, int h, int body, int cap, int lane) {
    fill(t, x, y, w, h - 1, body, lane);
    fill(t, x, y + h - 1, w, 1, cap, lane);
}

// The sprite System's set order for this episode: ids 0..n-1 inserted in creation order into a set that kept its
// bucket array across clear() (packed = buckets | next_resize << 16).
PG_D void episode_order(int32_t& packed, int n, uint8_t* out) {
    int16_t next[kMaxEnt];
    int16_t before[64];
    HashOrder h;
    h.next = next;
    h.before = before;
    h.head = kNil;
    h.buckets = packed & 0xffff;
    h.next_resize = packed >> 16;
    h.count = 0;
    if (h.buckets == 0) h.buckets = 1;
    for (int b = 0; b < h.buckets; b++) before[b] = kNil;
    for (int k = 0; k < n; k++) hash_insert(h, k);
    int16_t p = static_cast<int16_t>(h.head);
    for (int k = 0; k < n; k++) {
        out[k] = static_cast<uint8_t>(p);
        p = next[p];
    }
    packed = h.buckets | (h.next_resize << 16);
}

// reset() (climber.cpp:461-497 + tilemap.cpp:75-170) for one env by one wavefront: every lane walks the generator
// (the draws are wave-uniform), lane 0 records the entities.  Advances the env's generator chain (s.mt, the sprite
// set's bucket count) and leaves the level in `lv` (LDS).
PG_D void generate(const State& s, int env, GenLds& L, Level& lv, bool reseed, uint32_t seed, int lane) {
    uint32_t* gmt = s.mt + size_t(env) * kMtWords;
    if (reseed) {
        if (lane == 0) mt_seed(L.mt, seed);
    } else {
        for (int k = lane; k < kMtWords; k += 64) L.mt[k] = gmt[k];
    }
    __syncthreads();
    uint32_t* mt = L.mt;
    uint8_t* tiles = lv.tiles;
    const float max_jump = 1.5f, gravity = 0.2f;
    fill(tiles, 0, 0, W, H, kEmpty, lane);
    fill_capped(tiles, 0, 0, W, 1, kWallMid, kWallTop, lane);
    fill(tiles, 0, 0, 1, H, kWallMid, lane);
    fill(tiles, W - 1, 0, 1, H, kWallMid, lane);
    fill(tiles, 0, H - 1, W, 1, kWallMid, lane);
    const int difficulty = wave_rng_int(mt, 1, 3, lane);
    const int platforms = wave_rng_int(mt, difficulty * difficulty + 1, (difficulty + 1) * (difficulty + 1) + 1, lane);
    int cx = wave_rng_int(mt, 2, W - 3, lane), cy = 1;
    const int margin = 3;
    const float enemy_prob = kEnemyProb;
    const float reach_y = max_jump * max_jump / (2.0f * gravity);
    const int max_dy = static_cast<int>(reach_y - 0.5f);
    int n_ent = 0;
    auto spawn = [&](int x, int y, int info, float vx) {
        const int e = n_ent++;
        if (lane == 0) {
            lv.ex[e] = static_cast<float>(x) + 0.5f;
            lv.ey[e] = static_cast<float>(H - 1 - y) + 0.5f;
            lv.evx[e] = vx;
            lv.info[e] = static_cast<uint8_t>(info | kAlive);
            lv.spawn_x[e] = static_cast<uint8_t>(x);
        }
    };
    for (int p = 0; p < platforms; p++) {
        const int dy = wave_rng_int(mt, 3, max_dy - 1, lane);
        const bool roomy = (cx >= margin) && (cx <= W - 1 - margin);
        if (roomy && (wave_rng_real(mt, 0.0f, 1.0f, lane) < enemy_prob)) {
            const int my = cy + wave_rng_int(mt, 0, 1, lane) + 2;
            const float vx = 0.15f * (wave_rng_int(mt, 0, 1, lane) * 2.0f - 1.0f);  // tilemap.cpp:55
            spawn(cx, my, kMob, vx);
        }
        cy += dy;
        const int len = 2 + wave_rng_int(mt, 0, 9, lane);
        int vx = wave_rng_int(mt, 0, 1, lane) * 2 - 1;
        if (cx < margin) vx = 1;
        if (cx > W - margin) vx = -1;
        int spots[12];
        int n_spots = 0;
        for (int j = 0; j < len; j++) {
            const int nx = cx + (j + 1) * vx;
            if (nx <= 0 || nx >= W - 1) break;
            spots[n_spots++] = nx;
            fill_capped(tiles, nx, cy, 1, 1, kWallMid, kWallTop, lane);
        }
        if (wave_rng_real(mt, 0.0f, 1.0f, lane) < 0.5f || p == platforms - 1)
            spawn(spots[wave_rng_int(mt, 0, n_spots - 1, lane)], cy + 1, kTexSet, 0.0f);  // crystal: textured from the start
        cx = spots[wave_rng_int(mt, 0, n_spots - 1, lane)];
    }
    const int backdrop = wave_rng_int(mt, 0, 9, lane);
    const float shift = wave_rng_real(mt, 0.0f, 1.0f, lane);
    const int suit = wave_rng_int(mt, 0, 3, lane);
    const int theme = wave_rng_int(mt, 0, 3, lane);
    if (lane == 0) {
        lv.bgshift = shift;
        lv.themes = backdrop | (suit << 8) | (theme << 16);
        lv.n_ent = n_ent;
        int32_t packed = SI(s, I_HASH_SPRITE, env);
        episode_order(packed, n_ent, lv.order);
        SI(s, I_HASH_SPRITE, env) = packed;
    }
    __syncthreads();
    for (int k = lane; k < kMtWords; k += 64) gmt[k] = L.mt[k];
    __syncthreads();
}

// The level becomes the env's live state (what reset() and the component constructors initialise).
PG_D void install(const State& s, int env, const Level& lv, int lane) {
    uint32_t* tiles = reinterpret_cast<uint32_t*>(s.tiles + size_t(env) * (W * H));
    const uint32_t* src = reinterpret_cast<const uint32_t*>(lv.tiles);
    for (int k = lane; k < W * H / 4; k += 64) tiles[k] = src[k];
    const int n_ent = lv.n_ent;
    if (lane < n_ent) {
        EF(s, EF_X, lane, env) = lv.ex[lane];
        EF(s, EF_Y, lane, env) = lv.ey[lane];
        EF(s, EF_VX, lane, env) = lv.evx[lane];
        EF(s, EF_ANIM_T, lane, env) = 0.0f;
        EB(s, EB_INFO, lane, env) = lv.info[lane];
        EB(s, EB_SPAWN_X, lane, env) = lv.spawn_x[lane];
        EB(s, EB_ORDER, lane, env) = lv.order[lane];
    }
    if (lane == 0) {
        SF(s, F_BGSHIFT, env) = lv.bgshift;
        SF(s, F_AX, env) = 1.5f;
        SF(s, F_AY, env) = H - 2 + 1.0f;
        SF(s, F_AVX, env) = 0.0f;
        SF(s, F_AVY, env) = 0.0f;
        SF(s, F_APHASE, env) = 0.0f;
        SI(s, I_FLAGS, env) = kFlagForward;  // on_ground = false, face_forward = true, draw list cleared (D2)
        SI(s, I_THEMES, env) = lv.themes;
        SI(s, I_NENT, env) = n_ent;
        SI(s, I_NDRAW, env) = 0;
        // camera x is fixed (climber.cpp:466); camera y keeps the previous episode's value (D3)
    }
}

// What cenv_make leaves in an env besides the seeded RNG, split by owner: the generator chain (bucket counts of
// the sets that survive clear()) and the live state.  Level-seed mode (pg_engine.h LevelPlan) rebuilds every
// level from here.
PG_D void fresh_chain(const State& s, int env) {
    SI(s, I_HASH_SPRITE, env) = 1;
}
PG_D void fresh_live(const State& s, int env) {
    SF(s, F_CAMY, env) = 0.0f;  // Renderer::camera_position{0} (renderer.h:18)
}

struct Gen {  // pg_prefetch.h level_kernel<Gen>
    using State = climber::State;
    using Level = climber::Level;
    using GenLds = climber::GenLds;
    PG_D static void generate(const State& s, int env, GenLds& L, Level& lv, bool reseed, uint32_t seed, int lane) {
        climber::generate(s, env, L, lv, reseed, seed, lane);
    }
    PG_D static void install(const State& s, int env, const Level& lv, int lane) { climber::install(s, env, lv, lane); }
    PG_D static void fresh_chain(const State& s, int env) { climber::fresh_chain(s, env); }
    PG_D static void fresh_live(const State& s, int env) { climber::fresh_live(s, env); }
    PG_D static void chain_counts(const State& s, int env, uint32_t* w, bool put) {  // (pg_prefetch.h chain_keep: what fresh_chain empties)
        if (put) SI(s, I_HASH_SPRITE, env) = static_cast<int>(w[0]); else w[0] = static_cast<uint32_t>(SI(s, I_HASH_SPRITE, env));
    }
};

PG_D bool is_wall(int t) { return t == kWallMid || t == kWallTop; }

// A level has at most 17 platforms (difficulty 3: (3+1)² + 1, tilemap.cpp:98-105), each with at most one mob and one
// crystal.
constexpr int kMaxMobs = 17, kMaxGems = 17;

// One env = one gang of kGang adjacent lanes (pg_gang.h).  What costs in this game is get_collision — the agent's box
// and one probe per mob, every sub-step — so those are the gang's parallel work: collider 0 is the agent, collider
// 1 + m the m-th alive mob, kGang of them per pass through ONE copy of the collision code.  Everything else about the
// agent is uniform over the gang; mobs and crystals (alive ones, compacted in id order) live in LDS for the step.
#ifndef PG_CLIMBER_GANG
#define PG_CLIMBER_GANG 8
#endif
#ifndef PG_CLIMBER_WAVES
#define PG_CLIMBER_WAVES 4  // wavefronts per SIMD the logic kernel's registers are capped for
#endif
constexpr int kGang = PG_CLIMBER_GANG;
using Q = Gang<kGang>;

struct StepLds {  // one per gang
    float m_x[kMaxMobs], m_vx[kMaxMobs], m_t[kMaxMobs];
    unsigned long long m_win[kMaxMobs];
    int8_t m_ax[kMaxMobs], m_ay[kMaxMobs];
    uint8_t m_row[kMaxMobs], m_spawn[kMaxMobs], m_id[kMaxMobs], m_info[kMaxMobs];
    uint8_t g_col[kMaxGems], g_row[kMaxGems], g_id[kMaxGems], g_info[kMaxGems];
};

// System_Sprite_Render::update's list: the surviving sprites in set order, then std::sort on z (all 1.0).
PG_D void rebuild_draw_list(const State& s, Q q, int env, int n_ent) {
    int n = 0;
    for (int k0 = 0; k0 < n_ent; k0 += kGang) {
        const int k = k0 + q.g;
        n += __popc(q.ballot(k < n_ent && (EB(s, EB_INFO, k, env) & kAlive)));
    }
    const uint8_t* rank = s.ranks + rank_offset(n);  // equal keys: the sort is a fixed permutation for each n
    int r = 0;
    for (int k0 = 0; k0 < n_ent; k0 += kGang) {
        const int k = k0 + q.g;
        const int e = k < n_ent ? EB(s, EB_ORDER, k, env) : 0;
        const bool alive = k < n_ent && (EB(s, EB_INFO, e, env) & kAlive);
        const uint32_t m = q.ballot(alive);
        if (alive) EB(s, EB_DRAW, rank[r + __popc(m & ((1u << q.g) - 1u))], env) = static_cast<uint8_t>(e);
        r += __popc(m);
    }
    if (q.g == 0) SI(s, I_NDRAW, env) = n;
}

PG_D void advance(const State& s, StepLds& L, Q q, int env, int action, float& reward_out, bool& terminated_out) {
    const uint8_t* tiles = s.tiles + size_t(env) * (W * H);
    const int n_ent = SI(s, I_NENT, env);
    const float dt = 1.0f / 4;
    const uint32_t below = (1u << q.g) - 1u;

    // --- stage the alive entities (reference loop: `if (!alive) continue`): mobs and crystals in id order
    int n_mobs = 0, n_gems = 0;
    for (int e0 = 0; e0 < n_ent; e0 += kGang) {
        const int e = e0 + q.g;
        const bool ok = e < n_ent;
        const int info = ok ? EB(s, EB_INFO, e, env) : 0;
        const int spawn = ok ? EB(s, EB_SPAWN_X, e, env) : 0;
        const float x = ok ? EF(s, EF_X, e, env) : 0.0f, y = ok ? EF(s, EF_Y, e, env) : 0.0f;
        const float vx = ok ? EF(s, EF_VX, e, env) : 0.0f, t = ok ? EF(s, EF_ANIM_T, e, env) : 0.0f;
        const bool alive = (info & kAlive) != 0, mob = alive && (info & kMob), gem = alive && !(info & kMob);
        const uint32_t mobs = q.ballot(mob), gems = q.ballot(gem);
        const int row = H - 1 - static_cast<int>(y);  // y = (H-1-row) + 0.5 exactly (generate(): spawn)
        if (mob) {
            const int m = n_mobs + __popc(mobs & below);
            if (m >= kMaxMobs) __builtin_trap();
            L.m_x[m] = x;
            L.m_vx[m] = vx;
            L.m_t[m] = t;
            L.m_row[m] = static_cast<uint8_t>(row);
            L.m_spawn[m] = static_cast<uint8_t>(spawn);
            L.m_id[m] = static_cast<uint8_t>(e);
            L.m_info[m] = static_cast<uint8_t>(info);
            // its tile window for the step, around the probe of the first sub-step, spare column on the side it is heading
            // (mobs drift 0.15 tiles a step; `at()` falls back to a direct load outside the window: a cache, not an assumption)
            const float my = static_cast<float>(H - 1 - row) + 0.5f;
            const Box probe{x + vx * dt - 0.5f, my - 0.6f, 1.0f, 0.5f};
            const Win w = Win::around(tiles, probe, vx, 0.0f);
            L.m_win[m] = w.bits;
            L.m_ax[m] = static_cast<int8_t>(w.ax);
            L.m_ay[m] = static_cast<int8_t>(w.ay);
        }
        if (gem) {
            const int k = n_gems + __popc(gems & below);
            if (k >= kMaxGems) __builtin_trap();
            L.g_col[k] = static_cast<uint8_t>(static_cast<int>(x));  // x = col + 0.5 exactly
            L.g_row[k] = static_cast<uint8_t>(row);
            L.g_id[k] = static_cast<uint8_t>(e);
            L.g_info[k] = static_cast<uint8_t>(info);
        }
        n_mobs += __popc(mobs);
        n_gems += __popc(gems);
    }
    wave_order();

    int flags = SI(s, I_FLAGS, env);
    float ax = SF(s, F_AX, env), ay = SF(s, F_AY, env);
    float avx = SF(s, F_AVX, env), avy = SF(s, F_AVY, env);
    float phase = SF(s, F_APHASE, env), camy = SF(s, F_CAMY, env);
    bool ground = (flags & kFlagGround) != 0, forward = (flags & kFlagForward) != 0;
    const float max_jump = 1.55f, gravity = 0.2f, max_speed = 0.5f, mix = 0.2f, air_control = 0.15f;
    const float move_x = static_cast<float>((action == 6 || action == 7 || action == 8) -
                                            (action == 0 || action == 1 || action == 2));
    const bool jump = (action == 2 || action == 5 || action == 8);

    float reward = 0.0f;
    bool terminated = false, set_changed = (flags & kFlagListed) == 0;
    Win awin{tiles, 0, 0, 0};
    for (int ss = 0; ss < 4; ss++) {
        // --- System_Agent::update (common_systems.cpp:184-270), up to its get_collision
        const float mix_x = ground ? mix : (mix * air_control);
        avx += mix_x * (max_speed * move_x - avx) * dt;
        if (fabsf(avx) < mix_x * max_speed * dt) avx = 0.0f;
        if (jump && ground) avy = -max_jump;
        avy += gravity * dt;
        if (fabsf(avy) > max_jump) avy = (avy > 0.0f ? 1.0f : -1.0f) * max_jump;
        ax += avx * dt;
        ay += avy * dt;
        const Box body{ax + -0.5f, ay + -1.0f, 1.0f, 1.0f};
        if (ss == 0 || !awin.holds(body)) awin = Win::around(tiles, body, avx, avy);

        // --- the agent's get_collision: the same box in every lane of the gang, so the walk's nine cells go side by side
        // (pg_tiles.h collide_plain_gang8; until round 6 the agent was lane 0 of the mobs' pass and every lane walked)
        bool dead = false;
        Box agent{0.0f, 0.0f, 1.0f, 1.0f};
        {
            static_assert(kGang == 8, "collide_plain_gang8");
            const TileHit h = collide_plain_gang8(q, awin, body, is_wall);
            const float moved_x = h.x - body.x, moved_y = h.y - body.y;
            ground = moved_y < 0.0f && h.any;
            ax = h.x - -0.5f;
            ay = h.y - -1.0f;
            if (moved_x != 0.0f) avx = 0.0f;
            if (ground) avy = 0.0f;
            camy = (ay - 8 - 0.5f) * kUnitPx;
            phase += 0.1f * dt;
            phase = fmodf(phase, 1.0f);
            if (move_x > 0.0f)
                forward = true;
            else if (move_x < 0.0f)
                forward = false;
            agent = Box{ax + -0.5f, ay + -1.0f, 1.0f, 1.0f};
        }
        // --- the mobs, kGang per pass (common_systems.cpp:109-168; order-free per entity).  Their walk skips the cells no
        // mob of the wavefront meets (pg_tiles.h PG_WALK_SKIP: 96 -> 88 µs); a whether-test in front of it as in coinrun
        // (collide_any) then buys nothing more here — of the ≈ 60 mobs of a pass one usually does touch — and is not made.
        for (int m0 = 0; m0 < n_mobs; m0 += kGang) {
            const int m = m0 + q.g;
            const bool is_mob = m < n_mobs;
            float x = 0.0f, vx = 0.0f, y = 0.0f;
            Box probe = body;
            Win win = awin;
            if (is_mob) {
                x = L.m_x[m];
                vx = L.m_vx[m];
                y = static_cast<float>(H - 1 - L.m_row[m]) + 0.5f;
                x += vx * dt;
                probe = Box{x - 0.5f, y - 0.6f, 1.0f, 0.5f};
                win = Win{tiles, L.m_ax[m], L.m_ay[m], L.m_win[m]};
            }
            TileHit h{probe.x, probe.y, false};
            if (is_mob) h = collide_plain<true>(win, probe, is_wall);
            bool bitten = false;
            if (is_mob) {
                int info = L.m_info[m];
                x = h.x + 0.5f;
                bitten = box_hit(agent, Box{x + -0.4f, y + -0.4f, 0.8f, 0.8f});
                const int spawn_x = L.m_spawn[m];
                const bool end_patrol = x > spawn_x + 4 || x < spawn_x - 4;
                if (h.any || end_patrol) vx *= -1.0f;
                info = (info & ~kFlip) | (vx < 0.0f ? kFlip : 0);
                float t = L.m_t[m] + dt;
                const int adv = static_cast<int>(t * 0.2f);
                t -= adv / 0.2f;
                const int frame = (((info & kFrame) ? 1 : 0) + adv) % 2;
                info = (info & ~kFrame) | (frame ? kFrame : 0) | kTexSet;
                L.m_x[m] = x;
                L.m_vx[m] = vx;
                L.m_t[m] = t;
                L.m_info[m] = static_cast<uint8_t>(info);
            }
            if (q.any(bitten)) dead = true;
        }
        // --- points (:66-107)
        int delta = 0, available = 0;
        for (int k0 = 0; k0 < n_gems; k0 += kGang) {
            const int k = k0 + q.g;
            const int info = k < n_gems ? L.g_info[k] : 0;
            const bool alive = (info & kAlive) != 0;
            const float x = static_cast<float>(k < n_gems ? L.g_col[k] : 0) + 0.5f;
            const float y = static_cast<float>(H - 1 - (k < n_gems ? L.g_row[k] : 0)) + 0.5f;
            const bool taken = alive && box_hit(agent, Box{x + -0.5f, y + -0.5f, 1.0f, 1.0f});
            if (taken) L.g_info[k] = static_cast<uint8_t>(info & ~kAlive);  // destroy_entity
            delta += __popc(q.ballot(taken));
            available += __popc(q.ballot(alive && !taken));
        }
        if (delta) set_changed = true;
        reward = delta + (available == 0) * 10.0f;
        terminated = dead || (available == 0);
        if (terminated) break;
    }
    // Note: in the reference the mob loop runs before the point loop within a sub-step; the two never read each
    // other's data, so two loops per sub-step yield the same state.
    for (int m0 = 0; m0 < n_mobs; m0 += kGang) {
        const int m = m0 + q.g;
        if (m < n_mobs) {
            const int e = L.m_id[m];
            EF(s, EF_X, e, env) = L.m_x[m];
            EF(s, EF_VX, e, env) = L.m_vx[m];
            EF(s, EF_ANIM_T, e, env) = L.m_t[m];
            EB(s, EB_INFO, e, env) = L.m_info[m];
        }
    }
    if (set_changed)
        for (int k0 = 0; k0 < n_gems; k0 += kGang) {
            const int k = k0 + q.g;
            if (k < n_gems) EB(s, EB_INFO, L.g_id[k], env) = L.g_info[k];
        }
    if (q.g == 0) {
        SF(s, F_AX, env) = ax;
        SF(s, F_AY, env) = ay;
        SF(s, F_AVX, env) = avx;
        SF(s, F_AVY, env) = avy;
        SF(s, F_APHASE, env) = phase;
        SF(s, F_CAMY, env) = camy;
        SI(s, I_FLAGS, env) = kFlagListed | (ground ? kFlagGround : 0) | (forward ? kFlagForward : 0);
    }
    if (set_changed) {
        gang_fence();  // the info bytes just written, for the lanes that read them below
        rebuild_draw_list(s, q, env, n_ent);
    }
    reward_out = reward;
    terminated_out = terminated;
}

struct Step {  // pg_prefetch.h logic_step<Gen, Step>: a gang per env
    static constexpr int kGang = climber::kGang;
    using Lds = StepLds;
    PG_D static void advance(const State& s, Lds& L, int tid, int env, int action, float& reward, bool& terminated) {
        climber::advance(s, L, Q::at(tid), env, action, reward, terminated);
    }
};

__global__ void __launch_bounds__(64, PG_CLIMBER_WAVES) logic_kernel(State s, const int32_t* actions, uint32_t run_seed,
                                                                     uint32_t step_index, int env_offset, StepIO io, int prefetch, LevelPlan plan) {
    logic_step<Gen, Step>(s, actions, run_seed, step_index, env_offset, io, prefetch, plan);
}

// render_game(true) (climber.cpp:431-459): one workgroup of two wavefronts per env (pg_render.h).
constexpr int kGrid = 24;  // 64 px / 3.2 px per tile = 20 tiles → at most 22 columns/rows in view (24² = 9·64 cells; LDS: 7 envs per CU instead of 6)

// The draw list of climber.cpp:431-459, each kind of draw stated once, for render_full, setup_kernel and frame_draws:
// which texture, then the draw call given that texture's descriptor (x: first texel, y: width, z: height).
PG_D int tile_tex(int tile, int theme) { return (tile == kWallTop ? kTexTop : kTexMid) + theme; }  // tilemap.cpp:183-198
// positive-z sprites (common_systems.cpp:41-63): fish or gem
PG_D int entity_tex(int info) { return (info & kMob) ? kTexFish + ((info & kFrame) ? 1 : 0) : kTexGem; }
PG_D DrawCall entity_draw(int info, float x, float y, int tex, const int4& d) {
    if (!(info & kTexSet)) return kNoDraw;
    const float off = (info & kMob) ? -0.4f : -0.5f;  // tilemap.cpp:53,66
    const float scale = 1.0f * 1.0f;
    return DrawCall{true, (info & kFlip) != 0, false, tex, (x + off) * kUnitPx, (y + off) * kUnitPx, scale * kUnitPx / d.y, 1.0f, 0.0f};
}
// the agent (common_systems.cpp:272-298)
PG_D int agent_tex(int sflags, float avx, float aphase, int suit) {
    const bool ground = (sflags & kFlagGround) != 0;
    if (fabsf(avx) < 0.01f && ground) return kTexStand + suit;
    if (!ground) return kTexJump + suit;
    return (aphase > 0.5f ? kTexWalk2 : kTexWalk1) + suit;
}
PG_D DrawCall agent_draw(int sflags, float ax, float ay, int tex, const int4& d) {
    const float px = ax - 0.5f, py = ay - 1.0f;
    return DrawCall{true, (sflags & kFlagForward) == 0, false, tex, px * kUnitPx, py * kUnitPx, 0.8f * kUnitPx / d.y, 1.0f, 0.0f};
}

// The complete frame of one env by its workgroup, set-up included: the frames the pre-pass marks fat, the draw-list
// replay (flags bit 0) and kDebugNoPrepass.
PG_D void render_full(const State& s, const AtlasView& atlas, const StepIO& io, int flags, int env, uint32_t* fb,
                      ComposeLds<kGrid>& L) {
    const int lane = threadIdx.x & 63, half = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // two wavefronts per env (pg_render.h)
    constexpr int halves = 2;

    const Camera cam{W / 2.0f * kUnitPx, SF(s, F_CAMY, env), 64.0f, 64.0f, 0.2f * 64.0f / 64.0f};
    const int themes = SI(s, I_THEMES, env), sflags = SI(s, I_FLAGS, env);
    const int backdrop = themes & 0xff, suit = (themes >> 8) & 0xff, theme = (themes >> 16) & 0xff;
    const int n_draw = (sflags & kFlagListed) ? SI(s, I_NDRAW, env) : 0;  // empty right after a reset (D2)
    const uint8_t* tiles = s.tiles + size_t(env) * (W * H);
    const DescRegs descs = DescRegs::load(atlas, lane);
    Blit mine;

    // sprite-pass inputs, requested early
    const bool is_sprite = lane < n_draw, is_agent = lane == n_draw;
    int spr_info = 0;
    float spr_x = 0.0f, spr_y = 0.0f;
    if (is_sprite) {
        const int e = EB(s, EB_DRAW, lane, env);
        spr_info = EB(s, EB_INFO, e, env);
        spr_x = EF(s, EF_X, e, env);
        spr_y = EF(s, EF_Y, e, env);
    }

    int bg_soft = 0;  // the backdrop has texels that are not opaque (descriptor .w)
    // the background draw, climber.cpp:447-452 — each wave resolves the axis it needs (pg_render.h BgAxis)
    const BgDraw bg_draw = backdrop_draw(descs.uniform(kTexBackdrop + backdrop), SF(s, F_BGSHIFT, env));
    bg_soft = bg_draw.desc.w;
    const TileWindow win = tile_window(cam);  // tilemap.cpp:172-181
    const int x0 = win.x0, y0 = win.y0;
    const int cols = win.x1 - x0 + 1, rows = win.y1 - y0 + 1, cells = cols * rows;
    const int4 top_d = descs.uniform(kTexTop + theme), mid_d = descs.uniform(kTexMid + theme);

    BgAxis bga{};  // this wave's axis of it (wave 0: x, wave 1: y), resolved along with the tile spans
    bool composed = false;
    // The brown theme's cap tile is 64×53 next to 64×64 bodies (assets/platformer/tileBrown_06.png): the composer's
    // two-texture mode; a cap taller than the body, or of another width, would take the draw-list replay.
    const bool two = top_d.z != mid_d.z;
    if (!(flags & 1) && cols <= kGrid && rows <= kGrid && top_d.y == mid_d.y && top_d.z <= mid_d.z) {
        compose_spans(fb, L, cam, x0, y0, cols, rows, mid_d.y, mid_d.z, kUnitPx / mid_d.y, lane, two ? top_d.z : 0, half, halves,
                      soft_rows_of(bg_soft, top_d.w | mid_d.w), hard_rows_of(bg_soft, mid_d.w), &bg_draw, &bga);  // (cap tiles are few: always worth the attempt)
#pragma unroll
        for (int k = half; k < kGrid * kGrid / 64; k += halves) {
            const int cell = k * 64 + lane;
            const int r = cell / kGrid, c = cell % kGrid;
            const int t = (c < cols && r < rows) ? Win::direct(tiles, x0 + c, y0 + r) : kEmpty;
            L.base[cell] = (t == kEmpty) ? static_cast<int32_t>(kNoTexel)
                                         : (t == kWallTop ? (top_d.x * 4) | (two ? 1 : 0) : mid_d.x * 4);
        }
        __syncthreads();
        composed = two ? compose_rows<kGrid, true>(fb, L, atlas, bga, cols, rows, mid_d.y, lane, flags, half, halves)
                       : compose_rows<kGrid, false>(fb, L, atlas, bga, cols, rows, mid_d.y, lane, flags, half, halves);
    }
    if (!composed) {  // draw-list replay (tilemap.cpp:172-198)
        wave_clear(fb, lane, half, halves);
        const bool has_bg = resolve_draw(cam, bg_draw.desc.y, bg_draw.desc.z, bg_draw.desc.x, bg_draw.px, bg_draw.py, bg_draw.scale, 1.0f, false, false, mine);
        wave_replay(fb, atlas, mine, has_bg ? 1ull : 0ull, lane, half, halves);
        for (int base = 0; base < cells; base += 64) {
            const int cell = base + lane;
            bool has = false;
            if (cell < cells) {
                const int row = cell / cols;
                const int x = x0 + (cell - row * cols), y = y0 + row;
                const int t = Win::direct(tiles, x, y);
                if (t != kEmpty) {
                    const int4 d = (t == kWallTop) ? top_d : mid_d;
                    has = resolve_draw(cam, d.y, d.z, d.x, x * kUnitPx, y * kUnitPx, kUnitPx / d.y, 1.0f, false, false,
                                       mine);
                }
            }
            wave_replay(fb, atlas, mine, __ballot(has), lane, half, halves);
        }
    }

    {  // positive-z sprites (common_systems.cpp:41-63), then the agent (:272-298): one draw per lane
        int want_tex = 0;
        if (is_sprite)
            want_tex = entity_tex(spr_info);
        else if (is_agent)
            want_tex = agent_tex(sflags, SF(s, F_AVX, env), SF(s, F_APHASE, env), suit);
        const int4 d = descs.at(want_tex);
        // sprites and the agent differ in their parameters only: pick per lane, resolve once (a resolve_draw per kind
        // in its own branch is executed by the whole wave once per kind)
        DrawCall c = kNoDraw;
        if (is_sprite)
            c = entity_draw(spr_info, spr_x, spr_y, want_tex, d);
        else if (is_agent)
            c = agent_draw(sflags, SF(s, F_AX, env), SF(s, F_AY, env), want_tex, d);
        bool has = false;
        if (c.go) has = resolve_draw(cam, d.y, d.z, d.x, c.wx, c.wy, c.scale, 1.0f, c.flip_h, false, mine);
        wave_replay_rows(fb, atlas, mine, __ballot(has), lane, half * (kObsH / halves), (half + 1) * (kObsH / halves));
    }
    // each wave stores the rows it owns (pg_render.h wave_replay_rows): no barrier
    wave_store_rows(fb, io.obs + size_t(env) * kObsBytes, lane, half * (kObsH / halves), (half + 1) * (kObsH / halves));
}

// ------------------------------------------------------------------------------------------------
// The render pre-pass (pg_prepass.h prep_setup: the kernel; here what is climber's own): tile spans, per-pixel
// candidates, the cell table and the resolved, culled draws of kPrepEnvs envs per workgroup.
// Reference arithmetic moved here unchanged: tilemap.cpp:172-198 (the window), common_systems.cpp:41-63,272-298
// (sprites, agent).
// ------------------------------------------------------------------------------------------------
struct PrepEnv {
    int32_t sflags, n_draw, suit;
    float avx, aphase, ax, ay;
};
struct Setup : PrepPlain {
    using State = climber::State;
    static constexpr int kGrid = climber::kGrid, kSpan = kMaxSpan, kW = W, kH = H, kTexCount = climber::kTexCount, kOob = kWallMid;
    static constexpr bool kTwo = true;
    struct Lds {
        PrepEnv env[kPrepEnvs];
        uint32_t draw_order[kPrepEnvs][kEntStride / 4];  // EB_DRAW of every env
    };
    struct Regs {
        Camera cam;
        int themes;
        float bgshift;
    };
    static PG_D void stage(Lds& L, const State& s, int env0, int tid) {
        static_assert(kPrepEnvs * (kEntStride / 4) <= kPrepThreads, "one word per thread");
        if (tid < kPrepEnvs * (kEntStride / 4)) {
            const int e = tid / (kEntStride / 4), w = tid - e * (kEntStride / 4);
            if (env0 + e < s.n) L.draw_order[e][w] = reinterpret_cast<const uint32_t*>(&EB(s, EB_DRAW, 0, env0 + e))[w];
        }
    }
    static PG_D void load(const State& s, int env, Regs& r, PrepEnv& out) {
        r.cam = Camera{W / 2.0f * kUnitPx, SF(s, F_CAMY, env), 64.0f, 64.0f, 0.2f * 64.0f / 64.0f};
        r.themes = SI(s, I_THEMES, env);
        r.bgshift = SF(s, F_BGSHIFT, env);
        PrepEnv pe{};
        pe.sflags = SI(s, I_FLAGS, env);
        pe.n_draw = (pe.sflags & kFlagListed) ? SI(s, I_NDRAW, env) : 0;  // empty right after a reset (D2)
        pe.suit = (r.themes >> 8) & 0xff;
        pe.avx = SF(s, F_AVX, env);
        pe.aphase = SF(s, F_APHASE, env);
        pe.ax = SF(s, F_AX, env);
        pe.ay = SF(s, F_AY, env);
        out = pe;
    }
    static PG_D bool view(const int4* desc, const Regs& r, int, PrepView& v, uint32_t& soft, uint32_t& hard, uint32_t* meta, Lds&, int) {
        const int backdrop = r.themes & 0xff, theme = (r.themes >> 16) & 0xff;
        const int4 d = desc[kTexBackdrop + backdrop];
        v.bg = backdrop_draw(d, r.bgshift);  // climber.cpp:447-452
        return prep_view_cap_body(d, desc[kTexTop + theme], desc[kTexMid + theme], v, soft, hard, meta);
    }
    static PG_D const uint8_t* tiles(const State& s, int env) { return s.tiles + size_t(env) * (W * H); }
    static PG_D uint32_t kinds(uint32_t raw, const Lds&, int, uint32_t& kind_bytes) {  // kEmpty 0, kWallTop 1, kWallMid 2
        kind_bytes = prep_kinds_cap_body(raw);
        return 0u;
    }
    // The draws in the reference's order: the positive-z sprites (common_systems.cpp:41-63), then the agent (:272-298).
    static PG_D int count(const PrepEnv& pe) { return pe.n_draw + 1; }
    static PG_D DrawCall draw(const State& s, const Lds& L, const int4* desc, int e, int env, int slot) {
        const PrepEnv& pe = L.env[e];
        if (slot < pe.n_draw) {
            const int ent = (L.draw_order[e][slot >> 2] >> (8 * (slot & 3))) & 0xffu;
            const int info = EB(s, EB_INFO, ent, env);
            const float ex = EF(s, EF_X, ent, env), ey = EF(s, EF_Y, ent, env);
            const int tex = entity_tex(info);
            return entity_draw(info, ex, ey, tex, desc[tex]);
        }
        const int tex = agent_tex(pe.sflags, pe.avx, pe.aphase, pe.suit);
        return agent_draw(pe.sflags, pe.ax, pe.ay, tex, desc[tex]);
    }
};

__global__ void __launch_bounds__(kPrepThreads) setup_kernel(State s, AtlasView atlas, const uint8_t* mask, int flags) {
    __shared__ SetupLds<Setup> S;
    prep_setup<Setup>(S, s, atlas, mask, flags);
}

// render_game(true) (climber.cpp:431-459): one workgroup of two wavefronts per env; a lean frame starts from what
// setup_kernel left (coinrun.hip's render_kernel is the commented model).
__global__ void __launch_bounds__(128, 4) render_kernel(State s, AtlasView atlas, const uint8_t* mask, StepIO io,
                                                    int flags) {
    const int env = blockIdx.x;
    if (mask && !mask[env]) return;
    const int lane = threadIdx.x & 63, half = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int halves = 2;
    __shared__ alignas(16) uint32_t fb[kFbWords];
    __shared__ ComposeLds<kGrid> L;
    const PrepMeta M{s.prep.meta + size_t(env) * kPrepMetaWords};
    const uint32_t colw = s.prep.axes[size_t(env) * 128 + lane], roww = s.prep.axes[size_t(env) * 128 + 64 + lane];
    const uint32_t roww2 = s.prep.axes2[size_t(env) * 64 + lane];
    const uint32_t kind_off = M.w[PM_KINDS + (lane & (kPrepKinds - 1))];
    const int n_draws = M.draws();
    const bool has = lane < n_draws;
    const Blit mine = prep_draw_load(s.prep.draws + (size_t(env) * kPrepDraws + lane) * kBlitWords, has);
    prep_cells_expand_any<kGrid>(L, s.prep.cells + size_t(env) * (kGrid * kGrid), kind_off, half, lane);
    const ComposeRegs R = prep_regs<kGrid>(M, colw, roww, roww2, lane);
    __syncthreads();  // the cell table is complete
    if ((flags & (1 | kDebugNoPrepass)) || M.fat()) {  // (wave-uniform)
        render_full(s, atlas, io, flags, env, fb, L);
        return;
    }
    const int row_lo = half * (kObsH / halves), row_hi = (half + 1) * (kObsH / halves);
    if (M.flags() & 2u)
        compose_rows_from<kGrid, true, false>(fb, L, atlas, R, lane, flags, half, halves);
    else
        compose_rows_from<kGrid, false, false>(fb, L, atlas, R, lane, flags, half, halves);
    wave_replay_rows(fb, atlas, mine, __ballot(has), lane, row_lo, row_hi);
    wave_store_rows(fb, io.obs + size_t(env) * kObsBytes, lane, row_lo, row_hi);
}

// cenv_render's frame (render_game(false)): the draw list of render_kernel, one draw at a time, for either painter of pg_frame.h.
template <class Painter>
__device__ void frame_draws(const State& s, const AtlasView& atlas, int env, Painter& P) {
    const float fw = P.width(), fh = P.height();
    P.begin(atlas, Camera{W / 2.0f * kUnitPx, SF(s, F_CAMY, env), fw, fh, 0.2f * fw / 64.0f});
    const int themes = SI(s, I_THEMES, env), sflags = SI(s, I_FLAGS, env);
    const int backdrop = themes & 0xff, suit = (themes >> 8) & 0xff, theme = (themes >> 16) & 0xff;
    const int n_draw = (sflags & kFlagListed) ? SI(s, I_NDRAW, env) : 0;
    const uint8_t* tiles = s.tiles + size_t(env) * (W * H);
    P.clear();
    const BgDraw bg = backdrop_draw(P.desc(kTexBackdrop + backdrop), SF(s, F_BGSHIFT, env));
    P.draw(kTexBackdrop + backdrop, bg.px, bg.py, bg.scale);
    const TileWindow win = P.window();
    for (int y = win.y0; y <= win.y1; y++)
        for (int x = win.x0; x <= win.x1; x++) {
            const int tile = Win::direct(tiles, x, y);
            if (tile == kEmpty) continue;
            const int tex = tile_tex(tile, theme);
            P.draw(tex, x * kUnitPx, y * kUnitPx, kUnitPx / P.desc(tex).y);
        }
    for (int k = 0; k < n_draw; k++) {
        const int e = EB(s, EB_DRAW, k, env);
        const int info = EB(s, EB_INFO, e, env);
        const int tex = entity_tex(info);
        P.draw(entity_draw(info, EF(s, EF_X, e, env), EF(s, EF_Y, e, env), tex, P.desc(tex)));
    }
    const int tex = agent_tex(sflags, SF(s, F_AVX, env), SF(s, F_APHASE, env), suit);
    P.draw(agent_draw(sflags, SF(s, F_AX, env), SF(s, F_AY, env), tex, P.desc(tex)));
}

struct Frames {  // pg_frame.h frame_kernel<Frames> / frames_kernel<Frames>
    using State = climber::State;
    template <class Painter>
    static __device__ void draws(const State& s, const AtlasView& atlas, int env, Painter& P) { frame_draws(s, atlas, env, P); }
};

// The state row (pg_state_obs.h): oracle/pgo_climber.cpp Climber::dump_state, column by column.  The 14 scalars come from
// the field arrays, the entity records from each env's own tables.
struct StateRow {
    using State = climber::State;
    static constexpr int kFixed = 14, kRecord = 6, kMaxRecords = kMaxEnt, kWidth = kFixed + kRecord * kMaxRecords, kEnvCols = kFixed;
    static __device__ int length(const State& s, int env) { return kFixed + kRecord * SI(s, I_NENT, env); }
    static __device__ float value(const State& s, int env, int col) {
        if (col >= kFixed) {
            const int e = (col - kFixed) / kRecord, k = (col - kFixed) - e * kRecord;
            const uint8_t info = EB(s, EB_INFO, e, env);
            switch (k) {
                case 0: return (info & kAlive) ? 1.0f : 0.0f;
                case 1: return EF(s, EF_X, e, env);
                case 2: return EF(s, EF_Y, e, env);
                case 3: return (info & kMob) ? EF(s, EF_VX, e, env) : 0.0f;
                case 4: return (info & kFrame) ? 1.0f : 0.0f;
                default: return EF(s, EF_ANIM_T, e, env);
            }
        }
        const int themes = SI(s, I_THEMES, env);
        switch (col) {
            case 0: return SF(s, F_AX, env);
            case 1: return SF(s, F_AY, env);
            case 2: return SF(s, F_AVX, env);
            case 3: return SF(s, F_AVY, env);
            case 4: return (SI(s, I_FLAGS, env) & kFlagGround) ? 1.0f : 0.0f;
            case 5: return (SI(s, I_FLAGS, env) & kFlagForward) ? 1.0f : 0.0f;
            case 6: return SF(s, F_APHASE, env);
            case 7: return W / 2.0f * kUnitPx;  // (the camera never moves sideways)
            case 8: return SF(s, F_CAMY, env);
            case 9: return static_cast<float>(themes & 0xff);
            case 10: return SF(s, F_BGSHIFT, env);
            case 11: return static_cast<float>((themes >> 8) & 0xff);
            case 12: return static_cast<float>((themes >> 16) & 0xff);
            default: return static_cast<float>(SI(s, I_NENT, env));
        }
    }
    static std::string names() {
        return "agent_x agent_y agent_vel_x agent_vel_y agent_ground agent_forward agent_phase cam_x cam_y backdrop backdrop_shift "
               "suit theme n_things|alive x y vel_x frame anim_t";
    }
    static TileMaps map(const State& s) { return {s.tiles, W * H, W * H, 0xff, W, H}; }
};

// The points of the path distances (pg_paths.h): the body box spans agent_y - 1 .. agent_y; the game has no goal point.
struct PathRow {
    using Row = StateRow;
    static constexpr float kAgentDy = -0.5f;
    static constexpr int kGoalX = -1, kGoalY = -1;
};

class ClimberGame final : public ViewedGame<PrefetchingGame<Gen>, StateRow, PathRow, Frames> {
   public:
    const char* name() const override { return "climber"; }
    std::vector<std::string> texture_names() const override {
        std::vector<std::string> v;
        for (const char* t : {"tileBlue_05", "tileGreen_05", "tileYellow_06", "tileBrown_06", "tileBlue_08",
                              "tileGreen_08", "tileYellow_09", "tileBrown_09"})
            v.push_back(std::string("platformer/") + t + ".png");
        for (const char* pose : {"_stand", "_walk4", "_walk1", "_walk2"})  // jump = walk4 (common_systems.cpp:178)
            for (const char* suit : {"Blue", "Green", "Grey", "Red"})
                v.push_back(std::string("platformer/player") + suit + pose + ".png");
        v.push_back("platformer/enemySwimming_1.png");
        v.push_back("platformer/enemySwimming_2.png");
        v.push_back("misc_assets/yellowCrystal.png");
        for (const char* b : {"platform_backgrounds/alien_bg", "platform_backgrounds/another_world_bg",
                              "platform_backgrounds_2/fantasy1", "platform_backgrounds_2/fantasy2",
                              "platform_backgrounds_2/fantasy3", "platform_backgrounds_2/fantasy4",
                              "platform_backgrounds_2/candy1", "platform_backgrounds_2/candy2",
                              "platform_backgrounds_2/candy3", "platform_backgrounds_2/candy4"})
            v.push_back(std::string(b) + ".png");
        return v;
    }
    std::string check_atlas(const std::vector<std::pair<int, int>>& sizes) const override {
        return static_cast<int>(sizes.size()) == kTexCount ? "" : "climber: unexpected texture count";
    }
    // The state block, in order (state_bytes and bind).
    static void carve(Carve& c, State& s, int n) {
        c.take_env(s.shadow, n, 1, sizeof(Level));
        c.take_env(s.slot, n, 1, 4);
        c.take_env(s.mt, n, 1, kMtWords * 4);
        c.take_env(s.tiles, n, 1, W * H);
        c.take_env(s.f, n, F_COUNT, 4);
        c.take_env(s.i, n, I_COUNT, 4);
        c.take_env(s.ef, n, 1, EF_COUNT * kEntStride * 4);
        c.take_env(s.eb, n, 1, EB_COUNT * kEntStride);
    }
    size_t state_bytes(int n) const override { return Carve::size(carve, n); }
    void bind(void* d_state, int n, AtlasView atlas) override {
        Carve::bind(carve, d_state, s_, n, &regions);
        s_.n = n;
        s_.ranks = atlas.sort_ranks;
        atlas_ = atlas;
    }
    void launch_make(hipStream_t st, uint32_t seed_base, int env_offset) override {
        make_levels(st, seed_base, env_offset);
    }
    void launch_logic(hipStream_t st, const int32_t* actions, uint32_t run_seed, uint32_t step_index, int env_offset,
                      StepIO io) override {
        launch_fused_logic(logic_kernel, Step::kGang, st, actions, run_seed, step_index, env_offset, io);
    }
    static void carve_scratch(Carve& c, PrepOut& p, int n) { prep_carve(c, p, n, kGrid, kBlitWords, true); }
    size_t scratch_bytes(int n) const override { return Carve::size(carve_scratch, n); }
    void bind_scratch(void* d_scratch, int n) override { Carve::bind(carve_scratch, d_scratch, s_.prep, n); }
    void launch_prepass(hipStream_t st, const uint8_t* mask) override {
        prep_launch(setup_kernel, st, s_, atlas_, mask, debug_flags);
    }
    void launch_render(hipStream_t st, const uint8_t* mask, StepIO io) override {
        hipLaunchKernelGGL(render_kernel, dim3(s_.n), dim3(128), 0, st, s_, atlas_, mask, io, debug_flags);
    }
};

}  // namespace climber

}  // namespace PG_VARIANT_NS

std::unique_ptr<Game> PG_FACTORY(make_climber)() { return std::make_unique<PG_VARIANT_NS::climber::ClimberGame>(); }

}  // namespace pg
