// Engine-internal interfaces: device sprite atlas, per-game kernel launchers, and the vector env
// object behind the C ABI of include/procgen2_vec.h.  Nothing here is exported.
#pragma once

#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "pg_carve.h"
#include "pg_defs.h"
#include "pg_levels.h"
#include "pg_paths.h"

namespace pg {

// Device view of the atlas: all textures of one game packed into one RGBA8 array in HBM.
// desc[t] = {texel offset, width, height, 0}.  Replaces Asset_Texture / manager_texture
// (games/*/common_assets.h, asset_manager.h) — SURVEY.md rows A1, E4.
struct AtlasView {
    const uint32_t* texels;
    const int4* desc;
    int count;
    uint32_t texel_bytes;  // size of `texels` in bytes (< 256 MiB: pg_render.h kRank, kNoTexel)
    const uint8_t* sort_ranks;  // pg_order.h equal_key_ranks table (kRankTableBytes), uploaded with the atlas
};

class Atlas {
   public:
    ~Atlas();
    // names are reference asset paths relative to the asset root ("kenney/Items/coinGold.png").
    bool load(const std::string& root, const std::vector<std::string>& names, std::string& err);
    bool upload(std::string& err);
    AtlasView view() const {
        return {d_texels_, d_desc_, static_cast<int>(desc_.size()), static_cast<uint32_t>(texels_.size() * 4), d_ranks_};
    }
    size_t texel_bytes() const { return texels_.size() * 4; }
    // Host-side access for Game::extend_atlas: the decoded textures, and room for derived data behind them (returns
    // the word offset of the appended block; the atlas is one flat array of 32-bit words on the device).
    const uint32_t* texels_host(int tex) const { return texels_.data() + desc_[tex].x; }
    int4 desc_host(int tex) const { return desc_[tex]; }
    uint32_t append_words(const std::vector<uint32_t>& words) {
        const uint32_t at = static_cast<uint32_t>(texels_.size());
        texels_.insert(texels_.end(), words.begin(), words.end());
        return at;
    }
    std::vector<std::pair<int, int>> sizes() const {
        std::vector<std::pair<int, int>> v;
        for (const auto& d : desc_) v.emplace_back(d.y, d.z);
        return v;
    }

   private:
    std::vector<uint32_t> texels_;
    std::vector<int4> desc_;
    uint32_t* d_texels_ = nullptr;
    int4* d_desc_ = nullptr;
    uint8_t* d_ranks_ = nullptr;
};

// Buffers every game writes: the contiguous observation slab and the per-env scalars.
struct StepIO {
    uint8_t* obs;      // [n][64][64][3]
    float* reward;     // [n]
    uint8_t* done;     // [n]  terminated (truncated is always false in the reference: coinrun.cpp:367)
    // [n]  1: the env terminated last step → the next step performs the reset instead: the level kernel serves it and
    // leaves 2, the logic kernel skips it and puts 0 back.  A game whose logic kernel runs BESIDE the level kernel
    // (Game::resets_beside_logic) cannot hand the flag over like that: there the logic kernel skips every env that is
    // not 0 and writes 3 — not 1, which the level kernel running next to it would take for last step's — for an env that
    // terminates now, and the step's render kernel, which runs after both, turns 2 into 0 and 3 into 1.
    // Between steps: 0 or 1 either way.  The games that install prefetched levels inside their one logic launch
    // (pg_prefetch.h install_prefetched: maze, jumper, climber, caveflyer) keep the step's parity in the byte instead:
    // 4 | t mod 2 = reset due in step t, 2 | t mod 2 = reset served in step t, anything else = step.
    uint8_t* pending;
};

// pgv_state_layout (include/procgen2_vec.h) without its struct_size: width == fixed + record * max_records floats a state
// row, cells == tile_w * tile_h bytes a tile row (all three 0 for a game without a tile map).
struct StateLayout {
    int width, fixed, record, max_records, cells, tile_w, tile_h;
};

// The debug taps' buffer (include/procgen2_vec.h pgv_dump_state / pgv_dump_tiles): room for ONE env's rows, the
// engine's own, so a tap allocates nothing.  `width` and `cells`: the game's StateLayout, set before the listing runs.
struct TapBuffers {
    int32_t* index;   // the env asked for: the launches' d_indices
    int32_t* length;  // its dump's length
    float* row;       // [width], at a 16-byte boundary as the row kernels want their outputs
    uint8_t* tiles;   // [cells], likewise
    int width, cells;
};
inline void list_tap(Carve& c, TapBuffers& b, int) {
    c.take(b.index, 4, 8);
    c.take(b.length, 4, 8);
    c.take(b.row, size_t(b.width) * 4, 16);
    c.take(b.tiles, size_t(b.cells), 16);
}

// Word 0 of a record (pg_records.h: here because a game's records_loaded looks at it too).
constexpr uint32_t kRecordFull = 0x31524750u;  // "PGR1"
constexpr uint32_t kRecordEmpty = 0u;

class Game {
   public:
    virtual ~Game() = default;
    virtual const char* name() const = 0;
    virtual std::vector<std::string> texture_names() const = 0;
    virtual size_t state_bytes(int n) const = 0;
    virtual void bind(void* d_state, int n, AtlasView atlas) = 0;
    // cenv_make: seed rng with seed_base + env_offset + i, build and discard level 0 (D1).
    virtual void launch_make(hipStream_t s, uint32_t seed_base, int env_offset) = 0;
    // cenv_reset for envs where mask != 0 (nullptr = all); seeds nullptr = keep the stream (no reseed).
    virtual void launch_reset(hipStream_t s, const uint8_t* mask, const int32_t* seeds, StepIO io) = 0;
    // cenv_step with next-step auto-reset; actions nullptr = synthetic hash(run_seed, step, env).
    virtual void launch_logic(hipStream_t s, const int32_t* actions, uint32_t run_seed, uint32_t step_index,
                              int env_offset, StepIO io) = 0;
    // render_game(true) + RGB pack into io.obs for envs where mask != 0 (nullptr = all).  A game with a render pre-pass
    // (pg_prepass.h) has it launched right before, by the engine: launch_prepass, same mask — a launch of its own so that
    // the engine's render events (pgv_step_times, bench.py's roofline leg) bracket the render kernel alone.
    virtual void launch_render(hipStream_t s, const uint8_t* mask, StepIO io) = 0;
    virtual void launch_prepass(hipStream_t s, const uint8_t* mask) { (void)s; (void)mask; }
    // Level prefetch (pg_prefetch.h): launch the generator that fills queued shadow slots on the side stream.
    // bulk = most envs are expected to be queued (after make / a full reset).  False = game has no prefetch.
    virtual bool launch_pregen(hipStream_t side, bool bulk) { return false; }
    // While the side stream is busy the engine launches the generator again only every this-many steps: an env whose
    // episode ends before its slot is refilled generates its level inside the step, on the main stream, and one such env
    // costs the step a whole level's latency.  Four suits the games whose episodes last hundreds of steps; maze's
    // smallest mazes are solved in a few (two: 160 -> 195 M env-steps/s; one: 191), caveflyer gains 4 % at two,
    // coinrun, climber and jumper lose 1-2 %.
    virtual int pregen_every() const { return 4; }
    // The slot words of the game's shadow slots (pg_prefetch.h), or nullptr for a game without any: pgv_assign_levels puts
    // a ready slot that no longer holds what the env builds next back in the queue.
    virtual int32_t* prefetch_slots() const { return nullptr; }
    // cenv_render's human-size frame (render_game(false)) of one env into a w×h target of 0x00BBGGRR words in device
    // memory (pg_frame.h).  False = not implemented for this game.
    virtual bool launch_frame(hipStream_t s, int env, uint32_t* d_px, int w, int h) { return false; }
    // The same frames for `count` envs at once, as packed RGB into d_rgb = u8 [count][h][w][3] in device memory, tile by
    // tile (pg_frame.h TilePainter).  d_indices: device int32[count] or nullptr for envs 0 .. count-1; an index outside
    // the batch gives a frame of zeros.  Every game has it; a batch too big for one grid goes out in several launches.
    virtual void launch_frames(hipStream_t s, const int32_t* d_indices, int count, uint8_t* d_rgb, int w, int h) = 0;
    // Symbolic observations (include/procgen2_vec.h pgv_state_rows / pgv_tile_rows; pg_state_obs.h): the oracle's state
    // dump and tile map of `count` envs at once into device memory, d_rows = f32 [count][width] (+0.0f behind a dump's end),
    // d_lengths = int32 [count] or nullptr, d_tiles = u8 [count][cells].  d_indices as launch_frames takes them; an index
    // outside the batch gives a row of zero bytes and length 0.  Read-only, on the given stream.  state_layout / state_names
    // are host-only and need neither a bound state nor a GPU (pgv_state_layout_of asks a Game fresh from its factory).
    // The parity tests' debug taps (pgv_dump_state / pgv_dump_tiles) are the engine's: one row through these two launches.
    // Every game has the six functions from here to launch_tile_paths from ViewedGame (pg_state_obs.h).
    virtual StateLayout state_layout() const = 0;
    virtual std::string state_names() const = 0;  // "<fixed names>|<record names>", space-separated
    virtual void launch_state_rows(hipStream_t s, const int32_t* d_indices, int count, float* d_rows, int32_t* d_lengths) = 0;
    virtual void launch_tile_rows(hipStream_t s, const int32_t* d_indices, int count, uint8_t* d_tiles) = 0;
    // Path distances (include/procgen2_vec.h pgv_tile_paths_rows; pg_paths.h): the breadth-first distance field of `q.count`
    // envs' tile maps, with the map's own fields of q (tiles .. tile_h, n) filled in by the game.  Read-only, on the given
    // stream.  path_points is host-only, as state_layout is.  A game without a tile map (bossfight) has neither.
    virtual PathPoints path_points() const { return {false, 0.0f, 0.0f}; }
    virtual void launch_tile_paths(hipStream_t s, const TilePaths& q) { (void)s; (void)q; }
    // Caller-made levels (include/procgen2_vec.h pgv_get_levels / pgv_set_levels; pg_levels.h): the levels of `count` envs
    // read into the caller's rows, and the caller's rows installed as the named envs' live state (`to`: the engine's rows,
    // level words and scratch of the call).  level_layout is host-only, as state_layout is; supported = 0 (every other field 0)
    // for a game whose levels are more than a tile map and two points, and the engine then never calls the launches.
    virtual LevelLayout level_layout() const { return {0, 0, 0, 0, 0}; }
    virtual void launch_get_levels(hipStream_t s, const LevelRows& out) { (void)s; (void)out; }
    virtual void launch_set_levels(hipStream_t s, const LevelRows& in, const LevelInstall& to) { (void)s; (void)in; (void)to; }
    // pgv_config.game_flags (include/procgen2_vec.h); false = this game does not know these switches.
    virtual bool set_game_flags(uint32_t flags) { return flags == 0; }
    // Called once between loading and uploading the atlas: a game may append data derived from its textures (jumper:
    // its compass ring as it lands on the 64×64 observation — the same pixels in every frame of every env).
    virtual void extend_atlas(Atlas& atlas) { (void)atlas; }
    // Called by pgv_save_state before it copies the state blob: a game that keeps part of what a rollout depends on
    // outside the blob for speed (chaser: the random streams' second buffers) puts it back first.  The engine
    // synchronises the stream afterwards.
    virtual void prepare_save(hipStream_t st) { (void)st; }
    // Host-side sanity check of the loaded atlas (sizes[i] = {w, h} of texture i); empty string = fine.
    virtual std::string check_atlas(const std::vector<std::pair<int, int>>& sizes) const { return ""; }

    // A game that generates its levels inside the step (chaser: 0.2 ms a step) can have the level kernel's auto-reset
    // (pg_prefetch.h mode 2) run beside its logic kernel — the envs being reset sit the logic out — on `reset_stream`,
    // which the engine forks off its main stream before launch_logic and joins before the render launch.  The hand-over
    // between the streams costs about 25 µs, so games whose auto-reset only installs a prefetched level do not ask.
    virtual bool resets_beside_logic() const { return false; }
    hipStream_t reset_stream = nullptr;
    // Such a game may go further and keep the reset stream apart until AFTER the step's render launch: the envs being
    // reset are a per cent of the batch, their levels one long chain per wavefront — beside the render kernel that
    // chain is hidden altogether.  launch_render_step() then renders every env that is not being reset,
    // launch_render_late() — called once the reset stream has joined — the few that were.  Default: one launch.
    virtual void launch_render_step(hipStream_t s, StepIO io) { launch_render(s, nullptr, io); }
    virtual bool launch_render_late(hipStream_t s, StepIO io) { return false; }
    // A step that has no frame (pgv_step_sequence: every sub-step but a rendered last one): called where launch_prepass and
    // launch_render_step would have been, for whatever those launches do beside drawing that later steps or frames need:
    // coinrun's render wavefront finishes the entity table of a step that ended early (its redo_kernel does that here),
    // bossfight's pre-pass makes the random streams' next blocks ahead.  The pending bytes are not its business — the logic
    // kernels settle them, or the late pass, which a frameless step keeps (launch_render_late).  Default: nothing.
    virtual void launch_no_frame(hipStream_t s, StepIO io) { (void)s; (void)io; }

    // Called after pgv_load_state has replaced the state blob: whatever a game derives from its state and keeps OUTSIDE the
    // blob (chaser: the base layer of every env's frame, pg chaser.hip) is stale from here on.  An error fails the load.
    virtual hipError_t state_loaded(hipStream_t st) { (void)st; return hipSuccess; }

    // Per-env records (include/procgen2_vec.h pgv_save_envs / pgv_load_envs; pg_records.h).  `regions`: the per-env regions
    // of the state block, left by bind() (Carve, describe mode).  What a game keeps per env OUTSIDE the block:
    //   * stream_selectors(): the selector bytes of random streams that live in two buffers (bossfight, chaser: mt_sel), or
    //     nullptr.  A save is preceded by prepare_save (every stream at home), a load zeroes the loaded slots' bytes: at
    //     home, nothing made ahead.
    //   * pending_has_parity(): StepIO::pending carries the parity of the step it is about (pg_prefetch.h reset_due_mark)
    //     instead of 0 / 1.  A record holds "reset due: yes / no"; the load encodes it for the destination's next step.
    //   * records_loaded(): called behind the scatter, on the env's stream, for whatever else is derived from the state of
    //     the loaded slots (chaser: their base layers, the due list).  d_indices / count / d_records as given to
    //     pgv_load_envs; obs_offset: where a record keeps the observation row; next_step: the index of the next step.
    // The render pre-pass tables, coinrun's hazard hand-off and jumper's `fat` list are rebuilt every frame, and coinrun's
    // `scratch` rows inside the block are a hand-off within one step (they travel, harmlessly): nothing to put right.
    EnvRegions regions;
    virtual uint8_t* stream_selectors() const { return nullptr; }
    virtual bool pending_has_parity() const { return false; }
    virtual void records_loaded(hipStream_t st, const int32_t* d_indices, int count, const uint8_t* d_records, size_t record_bytes,
                                size_t obs_offset, uint32_t next_step, StepIO io) {
        (void)st; (void)d_indices; (void)count; (void)d_records; (void)record_bytes; (void)obs_offset; (void)next_step; (void)io;
    }

    // Device memory a game's kernels hand results to each other through within one frame (the render pre-pass,
    // pg_prepass.h): allocated by the engine beside the state, never part of a snapshot.
    virtual size_t scratch_bytes(int n) const { (void)n; return 0; }
    virtual void bind_scratch(void* d_scratch, int n) { (void)d_scratch; (void)n; }

    // Bit 0: render background + tiles by draw-list replay instead of the row composer (fallback path).
    // Bit 8: no level prefetch — every reset generates its level synchronously inside the step.
    // Bit 21: no render pre-pass — every frame's workgroup does its own set-up (the complete path; pg_prepass.h).
    // Bit 23: the pre-pass leaves every third env's frame to the complete path (`fat`), as it does by itself for the frames
    //         its tables do not hold — which some games never have in a normal run: the tests' way to that path.
    // Bit 24: coinrun — the entity lanes' hazard pre-selection assumes an agent that does not move (coinrun.hip hazard_near):
    //         the agent's own check of that assumption fails and resolve_kernel works the hazards out the long way.
    // Bit 27: coinrun — the render launch has no early blocks: a handed-back frame is drawn by its env's own block.
    int debug_flags = 0;
    LevelPlan plan{};  // set by the engine after bind()
};

constexpr int kDebugNoPrefetch = 1 << 8;
constexpr int kDebugNoPrepass = 1 << 21;  // (clear of the -DPG_ABLATE experiment bits the games use)
constexpr int kDebugFatThirds = 1 << 23;
constexpr int kDebugCoinrunNoReach = 1 << 24;
constexpr int kDebugChaserSerialMobs = 1 << 25;  // chaser: the enemies one after the other on the stream itself (chaser.hip advance)
constexpr int kDebugPolicyStrided = 1 << 26;     // policy observations: each lane stores its own units (pg_policy_obs.h), no exchange
constexpr int kDebugFatInPlace = 1 << 27;        // coinrun: no early blocks in the render launch — a handed-back frame is drawn by its env's own block (coinrun.hip render_kernel)

// What every game's host class keeps: its device view and the atlas, left there by its bind().
template <class S>
class BoundGame : public Game {
   protected:
    S s_{};
    AtlasView atlas_{};
};

// Factories, one per compiled variant of a game (pg_defs.h PG_VARIANT; v0 = the reference's compile-time default).
std::unique_ptr<Game> make_coinrun_v0();
std::unique_ptr<Game> make_maze_v0();
std::unique_ptr<Game> make_maze_v1();
std::unique_ptr<Game> make_maze_v2();
std::unique_ptr<Game> make_bossfight_v0();
std::unique_ptr<Game> make_bossfight_v1();
std::unique_ptr<Game> make_climber_v0();
std::unique_ptr<Game> make_climber_v1();
std::unique_ptr<Game> make_caveflyer_v0();
std::unique_ptr<Game> make_caveflyer_v1();
std::unique_ptr<Game> make_caveflyer_v2();
std::unique_ptr<Game> make_chaser_v0();
std::unique_ptr<Game> make_chaser_v1();
std::unique_ptr<Game> make_chaser_v2();
std::unique_ptr<Game> make_jumper_v0();
std::unique_ptr<Game> make_jumper_v1();
std::unique_ptr<Game> make_jumper_v2();

// Level numbers, and the counter-based synthetic action shared with the oracle (oracle/pgo_api.cpp pgo_synthetic_action).
PG_HD uint32_t level_number(int32_t num_levels, int32_t start_level, uint32_t chain_seed, uint32_t k) {
    return static_cast<uint32_t>(start_level) + mix32(mix32(chain_seed) + k) % static_cast<uint32_t>(num_levels);
}
#if defined(__HIPCC__)
// What env builds next, decided by ONE lane on behalf of whoever generates the level (pg_prefetch.h level_serve, bossfight's
// begin_level).  restart: the env's own sequence starts over from chain_seed; `drop` (a reset WITH seeds) also drops a
// pending assignment.  Returns whether the level has a number — then it is built as a fresh cenv_make(seed = number)
// builds its level 0, in either mode — and leaves the number and whether it came from an assignment.
PG_D bool plan_next_level(const LevelPlan& plan, int env, bool restart, bool drop, uint32_t chain_seed, uint32_t& number,
                          bool& from_assignment) {
    if (restart) {
        plan.chain_seed[env] = chain_seed;
        plan.drawn[env] = 0;
    }
    if (drop) plan.assigned_on[env] = 0;
    from_assignment = false;
    if (plan.assigned_on[env]) {
        plan.assigned_on[env] = 0;
        number = plan.assigned[env];
        from_assignment = true;
        return true;
    }
    if (plan.num_levels > 0) {
        const uint32_t k = plan.drawn[env];
        plan.drawn[env] = k + 1;
        number = level_number(plan.num_levels, plan.start_level, plan.chain_seed[env], k);
        return true;
    }
    number = 0u;
    return false;
}
// … and what the lane that installs a level leaves for pgv_level_numbers / pgv_level_known.
PG_D void plan_note_level(const LevelPlan& plan, int env, bool known, uint32_t number) {
    plan.number[env] = known ? number : 0u;
    plan.known[env] = known ? 1 : 0;
}
#endif
PG_HD int synthetic_action(uint32_t run_seed, uint32_t step, uint32_t env) {
    uint32_t h = mix32(mix32(step * 0x9E3779B9u + run_seed) ^ (env * 0x85EBCA6Bu + 0xC2B2AE35u));
    return static_cast<int>((static_cast<uint64_t>(h) * 15u) >> 32);
}
// The two ends of an env's step in a logic kernel: its action — the caller's, or the synthetic one — and what the step
// leaves in StepIO.  `mark`: what a terminated env leaves in `pending` (StepIO::pending: 1, 3, or the parity mark of
// pg_prefetch.h reset_due_mark).
PG_D int step_action(const int32_t* actions, uint32_t run_seed, uint32_t step_index, int env_offset, int env) {
    return actions ? actions[env] : synthetic_action(run_seed, step_index, static_cast<uint32_t>(env_offset + env));
}
PG_D void step_results(const StepIO& io, int env, float reward, bool terminated, int mark) {
    io.reward[env] = reward;
    io.done[env] = terminated ? 1 : 0;
    io.pending[env] = terminated ? static_cast<uint8_t>(mark) : 0;
}

}  // namespace pg
