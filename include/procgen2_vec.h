/* procgen2_vec.h — vector extension of the cenv ABI for the MI355X engine.
 *
 * The reference ABI (cenv/cenv.h:122-133) is single-env with process-global state and host buffers;
 * at 65 536 envs one step's observations are 805 MB, which cannot cross PCIe at the target rate
 * (SURVEY.md §7 hard part 5, §8b "Consequence for a vector engine").  This extension keeps the same
 * life cycle — make / reset / step / close, games/<g>/<g>.cpp cenv_make:127, cenv_reset:308,
 * cenv_step:341, cenv_close:413 — but for N envs at once, with explicit handles and DEVICE pointers.
 *
 * Plain C ABI: pointers and sizes only.  Pointers documented as "device" are HIP device pointers on
 * the env's GPU.  All work is enqueued on the env's stream (its own, or the one given at make);
 * pgv_sync waits for it.  Every function returns 0 on success; on failure the message is in
 * pgv_last_error().  There is no CPU fallback: without a usable GPU pgv_make fails.
 *
 * Semantics that mirror the reference:
 *   - env i is seeded with seed_base + env_offset + i and builds one level that is never observed
 *     (cenv_make calls reset(), coinrun.cpp:235,303 — SURVEY.md D1);
 *   - pgv_reset ≙ cenv_reset on the selected envs (optional reseed), renders the reset frame;
 *   - pgv_step ≙ cenv_step.  An env that reported terminated performs its reset on the NEXT
 *     pgv_step instead of stepping (action ignored, reward 0, done 0, observation = reset frame),
 *     i.e. the observation sequence equals the reference caller's `if term: env.reset()` loop
 *     (game_test.py:36-40) with the per-env mt19937 stream continuing;
 *   - truncated is always false in the reference games (coinrun.cpp:367) and is not materialised.
 */
#ifndef PROCGEN2_VEC_H
#define PROCGEN2_VEC_H

#ifdef __cplusplus
extern "C" {
#endif

#include <stdint.h>

#define PGV_API __attribute__((__visibility__("default")))

#define PGV_OBS_BYTES 12288 /* 64*64*3, coinrun.cpp:24-25,185 */
#define PGV_NUM_ACTIONS 15  /* coinrun.cpp:26 */

typedef struct pgv_env pgv_env;

/* Games available in this build: 0 "coinrun", 1 "maze", 2 "bossfight", 3 "climber", 4 "caveflyer", 5 "chaser", 6 "jumper".  Returns NULL past the end. */
PGV_API const char* pgv_game_name(int32_t game_id);
PGV_API int32_t pgv_game_id(const char* name); /* -1 if unknown */

/* Create N envs of `game` on HIP device `device`.  `stream` is a hipStream_t to enqueue on, or NULL
 * for an internally created stream.  Asset root: $PROCGEN2_ASSETS, else <dir of the .so>/../assets. */
PGV_API int32_t pgv_make(const char* game, int32_t num_envs, int32_t device, uint32_t seed_base, int32_t env_offset,
                         void* stream, pgv_env** out);
/* Same with a finite level set (the reference has no such option, the semantics follow the
 * original procgen's num_levels / start_level).  num_levels = 0 is pgv_make: every level is new.  With
 * num_levels > 0 the k-th level an env builds since it was made / reseeded is level number
 *     start_level + mix32(mix32(seed of the env) + k) % num_levels      (mix32: the hash of pgv_synthetic_action)
 * and level number L is exactly what a fresh cenv_make(seed = L) of the reference builds as its level 0 (fresh
 * containers and camera, rng.seed(L): coinrun.cpp:130-152,219-262), so equal numbers give equal levels. */
PGV_API int32_t pgv_make_levels(const char* game, int32_t num_envs, int32_t device, uint32_t seed_base,
                                int32_t env_offset, void* stream, int32_t num_levels, int32_t start_level,
                                pgv_env** out);

/* The general form.  Distribution modes are compile-time `System_Tilemap::Config` constants in the
 * reference (e.g. maze/tilemap.h:13-17,40-42, chaser/tilemap.cpp:85-99, climber/tilemap.h:33); PGV_MODE_DEFAULT is the
 * one each reference game is compiled with.  pgv_game_modes(game_id) = bit mask (1 << mode) of what a game offers;
 * asking for anything else fails.  Zero-initialise the struct and set struct_size = sizeof(pgv_config). */
#define PGV_MODE_DEFAULT 0
#define PGV_MODE_EASY 1
#define PGV_MODE_HARD 2
#define PGV_MODE_MEMORY 3
#define PGV_MODE_EXTREME 4
typedef struct pgv_config {
    uint32_t struct_size;
    int32_t num_envs;
    const char* game;
    void* stream; /* hipStream_t or NULL */
    int32_t device;
    uint32_t seed_base;
    int32_t env_offset;
    int32_t num_levels, start_level; /* pgv_make_levels */
    int32_t mode;                    /* PGV_MODE_* */
    uint32_t game_flags;             /* game-specific generator switches, 0 = the reference's defaults (below) */
} pgv_config;
/* coinrun: System_Tilemap::Config's allow_pit / allow_crate / allow_dy / allow_mobs (coinrun/tilemap.h:42-45, all true
 * in the reference; tilemap.cpp:158,174,250,258), as switches that turn a feature OFF. */
#define PGV_COINRUN_NO_PIT 1u
#define PGV_COINRUN_NO_CRATE 2u
#define PGV_COINRUN_NO_DY 4u
#define PGV_COINRUN_NO_MOBS 8u
/* chaser, jumper: how the reference's unqualified `abs(<float>)` calls resolve (games/chaser/common_systems.cpp:165-166,
 * 206,346-420; games/jumper/common_systems.cpp:198).  0 (default): glibc's `int abs(int)` — the argument is truncated
 * first — which is what g++/libstdc++ picks when no header of the translation unit includes <stdlib.h> or <math.h>
 * (SDL3's SDL_stdinc.h stopped including them).  1: `float std::abs(float)`, what the same sources mean as soon as any
 * header pulls libstdc++'s <stdlib.h> wrapper in, and on libc++ / MSVC always.  Both readings have recorded traces of
 * the unmodified reference (tests/golden/appendix_c.json). */
#define PGV_CHASER_FLOAT_ABS 1u
#define PGV_JUMPER_FLOAT_ABS 1u
PGV_API int32_t pgv_make_config(const pgv_config* config, pgv_env** out);
PGV_API uint32_t pgv_game_modes(int32_t game_id);
PGV_API int32_t pgv_mode(pgv_env* env); /* the resolved mode (never PGV_MODE_DEFAULT) */
PGV_API void pgv_close(pgv_env* env);

/* Reset the envs whose mask byte is non-zero (device u8[N]; NULL = all).  seeds: device int32[N] to
 * reseed each selected env's mt19937 (coinrun.cpp:313-317), or NULL to keep the streams running. */
PGV_API int32_t pgv_reset(pgv_env* env, const uint8_t* d_mask, const int32_t* d_seeds);

/* One step of every env.  d_actions: device int32[N], values 0..14 (others are no-ops except in maze,
 * SURVEY.md D6/D20). */
PGV_API int32_t pgv_step(pgv_env* env, const int32_t* d_actions);

/* Same, with actions generated on the device: a = (mix(run_seed, step_index, env_offset+i) * 15) >> 32
 * where step_index counts pgv_step/pgv_step_synthetic calls since make.  Used by the benchmark so
 * the CPU oracle sees identical streams without a host transfer. */
PGV_API int32_t pgv_step_synthetic(pgv_env* env, uint32_t run_seed);
PGV_API int32_t pgv_synthetic_action(uint32_t run_seed, uint32_t step_index, uint32_t global_env);

/* Host-pointer conveniences (synchronous upload, then the calls above): for callers without device
 * memory of their own, e.g. the cenv shim and the parity tests.  h_mask / h_seeds may be NULL. */
/* `steps` synthetic steps of `count` envs side by side — step s of every env is enqueued (each on its own stream) before
 * step s+1 of any: the launch loop of a mixed workload (several games on one device) without a host round trip through
 * the caller's language per env and step.  Nothing is synchronised; pgv_sync the envs afterwards. */
PGV_API int32_t pgv_step_synthetic_many(pgv_env* const* envs, int32_t count, int32_t steps, uint32_t run_seed);

PGV_API int32_t pgv_step_host(pgv_env* env, const int32_t* h_actions);
PGV_API int32_t pgv_reset_host(pgv_env* env, const uint8_t* h_mask, const int32_t* h_seeds);

/* PNG → RGBA8 through the engine's own decoder (host only, no GPU needed): lets tests compare the
 * atlas loader with an independent decoder.  Returns 0 and fills w/h; copies min(cap, w*h*4) bytes. */
PGV_API int32_t pgv_decode_png(const char* path, int32_t* w, int32_t* h, uint8_t* h_rgba, int64_t cap);

PGV_API int32_t pgv_sync(pgv_env* env);

/* How many times the level generator has been launched on the env's side stream since make (pg_prefetch.h).  The cadence
 * is a function of the step count alone — every Game::pregen_every()-th step, plus one launch per make / reset — whatever
 * the caller's synchronisation pattern: a measurement / test tap, -1 for a NULL env. */
PGV_API int64_t pgv_generator_launches(pgv_env* env);

/* Result buffers (device pointers, valid until pgv_close or the next pgv_bind_outputs):
 *   obs    u8 [N][64][64][3]   row-major HWC, one contiguous slab
 *   reward f32[N]
 *   done   u8 [N]              terminated flag of the last step */
PGV_API uint8_t* pgv_obs(pgv_env* env);
PGV_API float* pgv_reward(pgv_env* env);
PGV_API uint8_t* pgv_done(pgv_env* env);
/* Let the caller own the result buffers (e.g. torch tensors): any pointer may be NULL to keep the
 * engine's own allocation. */
PGV_API int32_t pgv_bind_outputs(pgv_env* env, uint8_t* d_obs, float* d_reward, uint8_t* d_done);

PGV_API int32_t pgv_num_envs(pgv_env* env);
PGV_API int32_t pgv_device(pgv_env* env);
PGV_API void* pgv_stream(pgv_env* env);

/* Synchronous copies to host memory (any pointer may be NULL). */
PGV_API int32_t pgv_copy_out(pgv_env* env, uint8_t* h_obs, float* h_reward, uint8_t* h_done);

/* Whole-batch snapshot / restore: game state (incl. RNG streams and prefetched levels), reward, done, the pending
 * auto-resets, the step counter and the observations, as one HOST buffer of pgv_snapshot_bytes().  A snapshot loads
 * only into an env made with the same game, num_envs and env_offset.  The reference has no counterpart (its state
 * lives in process globals, games/coinrun/coinrun.cpp:22-70); this is the vector engine's checkpoint/resume. */
PGV_API int64_t pgv_snapshot_bytes(pgv_env* env);
PGV_API int32_t pgv_save_state(pgv_env* env, void* h_buffer, int64_t capacity);
PGV_API int32_t pgv_load_state(pgv_env* env, const void* h_buffer, int64_t size);

/* Per-env state records: save, load and fork ANY envs, on the device.  (The original procgen's get_state / set_state; the
 * reference has no counterpart.)  A record is one env's complete state as a fixed-size, opaque, position-independent
 * block of pgv_env_record_bytes() bytes (a multiple of 16) in DEVICE memory.  Its size and its tag are functions of the
 * engine's configuration — game, mode, game_flags, num_levels, start_level, the record layout's version — and of nothing
 * else: not num_envs, env_offset, seed_base, the step counter or what the engine did before.  pgv_env_record_tag() is a
 * fingerprint of that configuration, never 0.  Records are for this process and this device: the caller may copy the
 * bytes wherever it likes, but the layout is not a file format (the tag ties a record to a layout version on purpose).
 *
 *   1. Saving is transparent: the engine that saved goes on exactly as one that never did.
 *   2. A record resumes in any slot of any engine of the same configuration on the same device — another num_envs,
 *      env_offset or seed_base, fresh or mid-rollout, at a step counter of either parity.  From the load on the slot
 *      produces, given the actions the source env would have been given, the observations, rewards and dones the source
 *      env would have produced, bit for bit, through any number of later auto-resets: its mt19937 stream, generator
 *      chain, prefetched level, position in the level set and (bossfight) camera size travel.  Right after the load the
 *      slot's rows of obs / reward / done — through the bound output pointers — are the source's at the save, and a
 *      reset that was pending for the source is pending for the slot.
 *   3. Envs that a load does not name are untouched, in state and in outputs.
 *   4. Two saves of one env with nothing in between are byte-equal (padding is written), so records can be hashed.
 *   5. What does NOT travel: the engine-wide step counter and the env's global index.  The actions pgv_step_synthetic
 *      makes on the device hash both, so a moved env gets the actions of the SLOT it now sits in, at its new engine's
 *      step count; a caller who wants an env's own trajectory back feeds explicit actions (pgv_step).
 *
 * d_records: device u8 [count][pgv_env_record_bytes], 16-byte aligned.  d_indices: device int32[count], or NULL for envs
 * 0 .. count-1.  Both calls are enqueued on the env's stream; nothing is allocated, the host is not synchronised (the
 * level generator's side stream is ordered by events).  count = 0 succeeds and does nothing; count < 0, or a NULL record
 * pointer with count > 0, fails.  pgv_load_envs checks `tag` on the host before anything is enqueued: records of another
 * configuration are refused and the engine is left as it was.
 * An index outside the batch: save writes a record marked empty, load skips it; load also skips every record marked
 * empty, and a zero-filled buffer is all empty records.  A save may name the same env several times.  The indices of
 * one load must be distinct: a slot named twice ends up with one of its records or a mixture of them (nothing faults).
 * Fork = save, then load under other indices.  Cost beside the copy itself: a save first brings home the random streams
 * that bossfight and chaser keep in two buffers (one small launch over the batch), a load launches the level generator
 * for the loaded slots whose next level was still queued (pgv_generator_launches counts it). */
PGV_API int64_t pgv_env_record_bytes(pgv_env* env);
PGV_API uint64_t pgv_env_record_tag(pgv_env* env);
PGV_API int32_t pgv_save_envs(pgv_env* env, const int32_t* d_indices, int32_t count, void* d_records);
PGV_API int32_t pgv_load_envs(pgv_env* env, const int32_t* d_indices, int32_t count, const void* d_records, uint64_t tag);
/* Host-pointer conveniences (synchronous; allocate and free their device buffers), as pgv_step_host is to pgv_step. */
PGV_API int32_t pgv_save_envs_host(pgv_env* env, const int32_t* h_indices, int32_t count, void* h_records);
PGV_API int32_t pgv_load_envs_host(pgv_env* env, const int32_t* h_indices, int32_t count, const void* h_records,
                                   uint64_t tag);

/* Assigned levels: choose, on the device, the level an env plays next, and read the level each env is in.  (The original
 * procgen's info["level_seed"], and what level replay, curricula and "evaluate these levels" are built on; the reference
 * has no counterpart.)
 *
 *   1. "Level number L" is what level-seed mode (pgv_make_levels) means by it, in ANY engine — num_levels = 0 or > 0, any
 *      mode, any game_flags: what a fresh cenv_make(seed = L) builds as its level 0 — fresh containers and camera,
 *      rng.seed(L).  d_levels[k] is read as its 32-bit pattern, as pgv_reset's seeds are.
 *   2. An assignment names the next level the env BUILDS: the auto-reset after its current episode, or a pgv_reset
 *      WITHOUT seeds that names the env, whichever comes first.
 *   3. One pending assignment per env.  A later one overwrites an unconsumed one; it is consumed when the level is built;
 *      a pgv_reset WITH seeds drops the pending assignment of the envs it names and behaves as it always did — also where
 *      the level generator had already built the assigned level on a fresh chain: the container state the env's own
 *      history left is kept until the next level is installed, and such a reset goes back to it.  There is no cancel call,
 *      on purpose: in free mode a prefetched assigned level has already replaced the env's mt19937 stream.
 *   4. After the assigned episode — level-seed mode: the env's own sequence goes on where it was; an assigned level takes
 *      no place in it (k does not move, and a level of the sequence that was prefetched and is discarded is not counted).
 *      Free mode (num_levels = 0): the env goes on as a reference env made with seed L goes on — its mt19937 stream and
 *      containers continue from the assigned episode.
 *   5. Timing does not show in results: an assignment made right after the env's reset (the generator's side stream has
 *      rebuilt the shadow slot long before it is needed) and one made the step before the reset is due (the level is
 *      generated inside the step) give the same bytes, with and without level prefetch (pgv_set_debug bit 8).
 *   6. Envs not named are untouched.  d_indices: device int32[count], or NULL for envs 0 .. count-1; the indices of one
 *      call must be distinct — of two entries that name one env, one wins (nothing faults); an index outside the batch is
 *      skipped.  count = 0 succeeds and does nothing; count < 0, or NULL levels with count > 0, fails.
 *   7. The call is enqueued on the env's stream and allocates nothing; the host is not synchronised (the level generator's
 *      side stream is ordered by events, as for pgv_load_envs).  Cost: one small launch over the indices and one launch of
 *      the level generator on its side stream — made by EVERY call with count > 0, however many slots it put back in the
 *      queue, none included (pgv_generator_launches counts it; measurements: docs/OPTLOG.md).
 *   8. pgv_level_numbers()[i] / pgv_level_known()[i] (device u32[N] / u8[N], valid from pgv_make until pgv_close, written
 *      on the env's stream): the number of the level env i is IN, and whether it has one — 1 in level-seed mode and for an
 *      assigned level, 0 (with number 0) for a free-mode level, 2 for a caller-made level with the caller's label as its
 *      number (pgv_set_levels).  Whatever installs a level writes them: at the step that
 *      reports `done` they still name the level that just ended — what a scorer needs — and they change in the step that
 *      shows the new level's first frame.
 *   9. The pending assignment, the current number and its flag, and what the shadow slot knows about the level it holds
 *      travel in pgv_save_state and in the per-env records: a loaded slot goes on as its source would have.
 * pgv_assign_levels_host: host pointers, synchronous (allocates and frees a device buffer), as pgv_step_host is to pgv_step. */
PGV_API int32_t pgv_assign_levels(pgv_env* env, const int32_t* d_indices, int32_t count, const int32_t* d_levels);
PGV_API int32_t pgv_assign_levels_host(pgv_env* env, const int32_t* h_indices, int32_t count, const int32_t* h_levels);
PGV_API const uint32_t* pgv_level_numbers(pgv_env* env);
PGV_API const uint8_t* pgv_level_known(pgv_env* env);

/* Episodes on the device: same-step autoreset, time limits and episode results, decided without a look from the host.
 * (Gymnasium's autoreset modes and TimeLimit, and the original procgen's episode info; the reference has no counterpart:
 * it never truncates, coinrun.cpp:367, and leaves the reset to its caller.)  Opt-in per engine: one that never calls
 * pgv_episodes_enable launches nothing new and gives the same bytes as before at every entry point.
 *
 *   1. pgv_episodes_enable allocates every buffer below, once per env; a second call fails.  It fails, with a message and
 *      the engine left as it was, for an unknown mode, max_episode_steps < 0, final_capacity outside 0 .. num_envs, and a
 *      step limit with PGV_AUTORESET_NEXT_STEP.  Without it pgv_step_episodes* and pgv_episode_outputs_get fail with a
 *      message.  pgv_step_episodes* allocates nothing and does not synchronise the host; it is enqueued on the env's stream
 *      (and the level generator on its side stream at its usual cadence).  With final_capacity > 0 the observation buffer
 *      (pgv_bind_outputs) must be 16-byte aligned.
 *   2. PGV_AUTORESET_NEXT_STEP: pgv_step_episodes is pgv_step for obs, the engine's own reward / done rows and all state;
 *      the episode outputs come on top.  The step that serves an env's auto-reset (reward 0, done 0, the reset frame) — any
 *      step that finds the env's `done` row set — is not an episode step: nothing is added to length or return.  The
 *      terminal frame is the env's obs row itself; final_obs is filled all the same where capacity allows.
 *   3. PGV_AUTORESET_SAME_STEP: an env that ends in this step — terminated by the game, or truncated: it played the
 *      max_episode_steps-th step of its episode without terminating — is reset inside the same call, exactly as
 *      pgv_reset(mask = ended, seeds = NULL) does it: the mt19937 stream continues, a pending level assignment is consumed,
 *      the level words are written, the env's pending auto-reset is cleared.  Its obs row is then the first frame of the new
 *      episode; its terminal frame is in final_obs, its terminal reward and flags in the episode outputs' reward /
 *      terminated / truncated; the engine's own reward / done rows of it are what pgv_reset leaves: 0.  The call equals the
 *      caller's loop pgv_step; read done and count steps; pgv_reset(mask) — except that the level generator keeps its
 *      step-count cadence: the launch pgv_reset forces is not made per step.
 *   4. ended_env lists the envs that ended in this step in ascending order; counts[0], anything from 0 to N, says how
 *      many.  ended_return / ended_length / ended_level / ended_level_known are listed for all of them — the level words as
 *      they stood before the reset — the frames for the first counts[1] = min(counts[0], final_capacity).  Entries past the
 *      counts are unspecified.  Lists and ring hold one step's results until the next pgv_step_episodes*.
 *   5. ended_return is the float32 sum of the episode's rewards in step order (ret = ret + r, one rounding a step),
 *      ended_length the number of its steps.  running_return / running_length are those of the episode each env is IN; a
 *      pgv_reset zeroes them for the envs it names.  pgv_load_envs and pgv_load_state leave them as they are — they travel
 *      neither in records nor in snapshots — and the caller may write them (after a fork, with its own indexing).  A loaded
 *      slot whose source had a reset pending has its next step recognised as the reset step: the `done` row travels.
 *      pgv_step and pgv_step_episodes may be mixed on one engine; steps taken through pgv_step are not counted. */
#define PGV_AUTORESET_NEXT_STEP 0
#define PGV_AUTORESET_SAME_STEP 1
typedef struct pgv_episode_config {
    uint32_t struct_size;
    int32_t autoreset;         /* PGV_AUTORESET_* */
    int32_t max_episode_steps; /* 0: no limit.  > 0 only with PGV_AUTORESET_SAME_STEP */
    int32_t final_capacity;    /* rows of the final-observation ring, 0 .. num_envs */
} pgv_episode_config;
typedef struct pgv_episode_outputs { /* device pointers, valid until pgv_close */
    uint32_t struct_size;
    float* reward;              /* [N]  this step's reward (same-step: the terminal step's, kept across the reset) */
    uint8_t* terminated;        /* [N] */
    uint8_t* truncated;         /* [N] */
    uint8_t* ended;             /* [N]  terminated | truncated */
    int32_t* counts;            /* [2]  episodes that ended in this step; how many of them have a row in final_obs */
    int32_t* ended_env;         /* [N]  their env indices, ascending */
    float* ended_return;        /* [N]  parallel to ended_env */
    int32_t* ended_length;      /* [N] */
    uint32_t* ended_level;      /* [N]  pgv_level_numbers / pgv_level_known of the level that just ended */
    uint8_t* ended_level_known; /* [N] */
    uint8_t* final_obs;         /* [final_capacity][PGV_OBS_BYTES]  terminal frame of ended_env[k], k < counts[1]; NULL at capacity 0 */
    float* running_return;      /* [N]  of the episode each env is IN; the caller may write */
    int32_t* running_length;    /* [N] */
} pgv_episode_outputs;
PGV_API int32_t pgv_episodes_enable(pgv_env* env, const pgv_episode_config* config);
PGV_API int32_t pgv_episode_outputs_get(pgv_env* env, pgv_episode_outputs* out); /* set struct_size first */
PGV_API int32_t pgv_step_episodes(pgv_env* env, const int32_t* d_actions);
PGV_API int32_t pgv_step_episodes_synthetic(pgv_env* env, uint32_t run_seed); /* same action hash and step counter as pgv_step_synthetic */
PGV_API int32_t pgv_step_episodes_host(pgv_env* env, const int32_t* h_actions); /* as pgv_step_host */
/* Measurement: `steps` calls of pgv_step_episodes_synthetic with HIP events on the env's stream — h_step_ms[s] the whole call,
 * h_episode_ms[s] the two episode launches behind the step alone (host arrays of `steps` floats, either may be NULL). */
PGV_API int32_t pgv_step_episodes_times(pgv_env* env, int32_t steps, uint32_t run_seed, float* h_step_ms, float* h_episode_ms);

/* Steps without frames: play a sequence of T sub-steps in one call and render only the last of them, or none.  (Look-ahead
 * over forked envs, fast-forwarding a batch, open-loop evaluation, action repeat, any consumer of rewards and dones that
 * does not look at pixels; the reference and the original procgen draw every step.)
 *
 *   1. pgv_step_sequence with T sub-steps leaves the engine as T calls of pgv_step would — of pgv_step_synthetic when
 *      `actions` is NULL — with the same rows, bit for bit, through any number of auto-resets inside the sequence: the game
 *      state, the random streams, the prefetched levels and pending resets, the level words and pending assignments, the
 *      step counter, the engine's own reward / done rows (the last sub-step's), pgv_generator_launches and, with
 *      PGV_FRAMES_LAST, the whole observation slab.
 *   2. rewards[t][i] / dones[t][i] are what pgv_reward()[i] / pgv_done()[i] would have held after sub-step t.  An env that
 *      reports done in sub-step t serves its reset in sub-step t + 1 (reward 0, done 0) and plays on: the engine's own
 *      next-step policy.  The call is NOT a frame-skip wrapper that freezes ended envs; the caller cuts at the first done,
 *      and seq_* does that cutting on the device.
 *   3. seq_length[i] is the index of env i's first sub-step with done set, plus 1, or T if there is none; seq_done[i] says
 *      whether there is one; seq_return[i] is the float32 sum of rewards[0 .. seq_length - 1][i] in step order from 0.0f, one
 *      rounding a step (ret = ret + r, the rule of ended_return).  Pure functions of the rows, available with rewards / dones
 *      NULL; a sub-step that serves a reset counts like any other.
 *   4. PGV_FRAMES_NONE: nothing is drawn for the envs that play.  Where a game needs frames of its own inside a frameless
 *      step (chaser's late pass over the envs just reset) it makes them, which is why obs is unspecified and not untouched.
 *      pgv_render_obs(NULL) afterwards leaves exactly the slab PGV_FRAMES_LAST would have left; pgv_render_obs(mask) does so
 *      for the rows whose mask byte is non-zero and leaves the others' bytes alone.  pgv_render_obs changes no state, at any
 *      time between steps: an engine that called it goes on exactly as one that did not, and twice gives the same bytes.
 *   5. Everything is enqueued on the env's stream; nothing is allocated per call and the host is not synchronised.  The
 *      _host forms take HOST pointers for every pointer of the struct, allocate and free their staging and synchronise.
 *   6. Every check is made on the host before anything is enqueued; a refusal leaves a message and the engine as it was:
 *      steps < 0, an unknown `frames`, a struct_size too small, with actions a stride that is neither 0 nor >= N.
 *      steps = 0 succeeds and does nothing (no output is written).
 *   7. On an engine with episodes enabled the call behaves as pgv_step does: its steps are not counted. */
#define PGV_FRAMES_LAST 0 /* the last sub-step is a complete pgv_step: its frame is rendered */
#define PGV_FRAMES_NONE 1 /* no sub-step renders; obs is unspecified until pgv_render_obs or the next rendering call */
typedef struct pgv_sequence {
    uint32_t struct_size;
    int32_t steps;          /* T >= 0; 0 succeeds and does nothing */
    const int32_t* actions; /* device int32; sub-step t reads row actions + t*action_stride; NULL: synthetic */
    int64_t action_stride;  /* elements; 0 = the same row every sub-step (action repeat), else >= N */
    uint32_t run_seed;      /* synthetic actions only: same hash, same step counter as pgv_step_synthetic */
    int32_t frames;         /* PGV_FRAMES_* */
    float* rewards;         /* device f32[T][N] or NULL */
    uint8_t* dones;         /* device u8 [T][N] or NULL */
    float* seq_return;      /* device f32[N] or NULL */
    int32_t* seq_length;    /* device i32[N] or NULL */
    uint8_t* seq_done;      /* device u8 [N] or NULL */
} pgv_sequence;
PGV_API int32_t pgv_step_sequence(pgv_env* env, const pgv_sequence* seq);
PGV_API int32_t pgv_step_sequence_host(pgv_env* env, const pgv_sequence* seq); /* every pointer a HOST pointer; synchronous, as pgv_step_host */
PGV_API int32_t pgv_render_obs(pgv_env* env, const uint8_t* d_mask);           /* device u8[N] or NULL = all */
PGV_API int32_t pgv_render_obs_host(pgv_env* env, const uint8_t* h_mask);

/* Policy-ready observations on the device: the frame a policy network reads — channel-first, scaled, frame-stacked,
 * optionally gray — made by the engine behind the render launch, where the facts it needs are known: which envs served a
 * reset, resets inside a frameless sequence included.  (Gymnasium's FrameStackObservation / GrayscaleObservation and the
 * permute-convert-divide every consumer of the u8 [N][64][64][3] slab writes; the reference has no counterpart.)  Opt-in
 * per engine: one that never calls pgv_policy_obs_enable launches nothing new and gives the same bytes as before at every
 * entry point.
 *
 * The tensor: [N][K*C][64][64], contiguous, C = 3 (planes R, G, B) or 1 (gray); slot 0 is the oldest frame, slot K-1 the
 * newest, channel slot*C + c.  The value of byte v: PGV_POLICY_U8 v; PGV_POLICY_F32 the float32 float(v) / 255.0f (one
 * correctly rounded division); PGV_POLICY_F16 / PGV_POLICY_BF16 that float32 rounded to nearest-even binary16 / bfloat16.
 * Gray: y = (77*R + 150*G + 29*B + 128) >> 8 in integers (white stays 255), then the value rule on y.
 *
 *   1. pgv_policy_obs_enable may be called once per env, at any time.  Everything is checked on the host before anything is
 *      enqueued; a refusal leaves a message and the engine as it was: a second call, stack outside 1 .. 8, gray outside
 *      0 .. 1, an unknown dtype, an `out` that is not 16-byte aligned, a struct_size too small.  It sets every env's restart
 *      flag and pushes nothing: the first push after it fills every stack with that env's frame.  Until then the engine's
 *      own tensor is zero and a caller's is as the caller left it.
 *   2. A PUSH converts the obs slab as it stands at that point of the env's stream: an env whose restart flag is set gets
 *      the new frame into all K slots and its flag cleared; any other env has slots 1 .. K-1 moved to 0 .. K-2 and the new
 *      frame put into slot K-1.  With a mask, an env whose mask byte is 0 is not touched: no move, no flag change.  A push
 *      is enqueued on the env's stream, allocates nothing and does not synchronise the host.  It needs the obs slab 16-byte
 *      aligned (pgv_bind_outputs may move the slab): pgv_policy_obs_push and every call of point 4 that ends with a push
 *      check that on the host before they enqueue anything, and fail with a message and the engine as it was — no step
 *      taken, no flag set, the step counter where it stood.  The calls that do not push do not check.
 *   3. An env's restart flag is set by: every step, however taken — the measurement entry points and the sub-steps of
 *      pgv_step_sequence included — that finds the env's `done` row set (that step serves its reset); pgv_reset, for the
 *      envs it names; a same-step auto-reset, for the envs that ended; pgv_load_envs, for the slots it actually wrote (an
 *      index outside the batch and an empty record set nothing); pgv_load_state, for all envs.  Only a push that touches
 *      the env clears it.  The stack travels neither in records nor in snapshots: pgv_snapshot_bytes and
 *      pgv_env_record_bytes are what they were.
 *   4. Who pushes, once per call and behind everything else the call enqueues: pgv_step, pgv_step_synthetic and
 *      pgv_step_host, all envs; pgv_step_episodes, pgv_step_episodes_synthetic and pgv_step_episodes_host, all envs, after
 *      the same-step reset has redrawn the ended envs — an ended env's stack is then K copies of its new episode's first
 *      frame, its terminal frame is in final_obs as before, and the stacked view of the terminal step is not kept;
 *      pgv_reset and pgv_reset_host, under their mask (envs not named keep their bytes); pgv_step_sequence and
 *      pgv_step_sequence_host with PGV_FRAMES_LAST, all envs, once, behind the last sub-step: an env that served a reset in
 *      any sub-step has its stack restarted with the drawn frame, so the call is a frame-skip whose stack never mixes
 *      episodes.  Who does not push: PGV_FRAMES_NONE, pgv_render_obs and pgv_render_obs_host, pgv_step_synthetic_many,
 *      pgv_timed_steps, pgv_step_times, pgv_step_phases, pgv_step_phases_many, pgv_step_episodes_times.  Flags still
 *      accumulate there, so a later push is right.
 *   5. PGV_FRAMES_NONE, then pgv_render_obs(NULL), then pgv_policy_obs_push(NULL) leaves exactly what PGV_FRAMES_LAST would
 *      have left: the obs slab, the policy tensor and the flags. */
#define PGV_POLICY_U8 0
#define PGV_POLICY_F16 1
#define PGV_POLICY_BF16 2
#define PGV_POLICY_F32 3
typedef struct pgv_policy_obs_config {
    uint32_t struct_size;
    int32_t stack; /* K, 1 .. 8 */
    int32_t gray;  /* 0: three planes R, G, B; 1: one plane, the gray rule */
    int32_t dtype; /* PGV_POLICY_* */
    void* out;     /* device, 16-byte aligned, N * pgv_policy_obs_bytes_per_env bytes; NULL: the engine allocates (zeroed) */
} pgv_policy_obs_config;
PGV_API int32_t pgv_policy_obs_enable(pgv_env* env, const pgv_policy_obs_config* config);
PGV_API void* pgv_policy_obs(pgv_env* env);                       /* the tensor; NULL before enable */
PGV_API int64_t pgv_policy_obs_bytes_per_env(pgv_env* env);       /* K*C*4096*element size; 0 before enable */
PGV_API const uint8_t* pgv_policy_obs_restart(pgv_env* env);      /* device u8[N]: the pending restart flags; NULL before enable */
PGV_API int32_t pgv_policy_obs_push(pgv_env* env, const uint8_t* d_mask); /* device u8[N] or NULL = all */
PGV_API int32_t pgv_policy_obs_push_host(pgv_env* env, const uint8_t* h_mask);

/* Frame history on the device: the last T frames of every env, each stored once as planar u8 with one `began` byte, and a
 * gather that builds stacked, scaled, channel-first rows — what the policy observations keep for "now" — for any list of
 * (push number, env) pairs, only when somebody reads them: the acting batch, or a training minibatch over T x N.  A push
 * writes one frame per env instead of moving K; a rollout's observations cost C*4096 bytes per (step, env) instead of
 * K*C*4096*element size.  Opt-in per engine: one that never calls pgv_history_enable launches nothing new and gives the same
 * bytes as before at every entry point.  Independent of the policy observations: either may be enabled without the other.
 *
 *   1. Slots.  Push number p (0, 1, 2, ...) lives in slot p % T of `frames`, u8 [T][N][C][64][64], C = 3 (planes R, G, B) or
 *      1 (gray: (77*R + 150*G + 29*B + 128) >> 8, the policy observations' rule), and of `began`, u8 [T][N].  Push p is HELD
 *      while head - T <= p < head, head being the number of pushes so far (pgv_history_head: a host counter that moves when a
 *      push is enqueued, read without synchronisation).
 *   2. A PUSH converts the obs slab as it stands at that point of the env's stream into slot head % T, all envs, writes
 *      began[slot][i] = env i's pending flag, clears the flag, and head moves.  It is enqueued on the env's stream, allocates
 *      nothing and does not synchronise the host.  It needs the obs slab 16-byte aligned (pgv_bind_outputs may move the
 *      slab): pgv_history_push and every call of point 4 or 5 check that on the host before they enqueue anything, and fail
 *      with a message and the engine as it was — no step taken, no flag set, head and the step counter where they stood.
 *   3. An env's pending flag is set by exactly the events of point 3 of the policy observations: any step, however taken,
 *      that finds the env's `done` row set; pgv_reset, for the envs it names; a same-step auto-reset, for the envs that
 *      ended; pgv_load_envs, for the slots it actually wrote; pgv_load_state, for all envs; and pgv_history_enable itself,
 *      for all envs.  The flags are the feature's own array (pgv_history_pending).  The ring travels neither in records nor
 *      in snapshots: pgv_snapshot_bytes and pgv_env_record_bytes are what they were.
 *   4. Who pushes a new slot, once per call and behind everything else the call enqueues: the callers of point 4 of the
 *      policy observations — pgv_step, pgv_step_synthetic, pgv_step_host; pgv_step_episodes, pgv_step_episodes_synthetic,
 *      pgv_step_episodes_host, after the same-step reset has redrawn the ended envs; pgv_step_sequence and
 *      pgv_step_sequence_host with PGV_FRAMES_LAST.  Who does not push: the same list as there.  After PGV_FRAMES_NONE and
 *      pgv_render_obs(NULL), pgv_history_push leaves what PGV_FRAMES_LAST would have left.
 *   5. pgv_reset (and pgv_reset_host) opens no slot of its own: the newest slot is "what pgv_obs showed when the caller next
 *      acts", and after a reset that is the reset frame.  It rewrites, in slot (head - 1) % T, the rows of the envs it names
 *      with the frame it drew, began = 1, and clears their pending flags; rows and flags of envs it does not name keep their
 *      bytes.  At head == 0 it opens slot 0 first (head becomes 1): the rows of envs it does not name are then what `frames`
 *      held — zeros in the engine's own — and their flags stay set, so their first pushed frame begins their history.
 *   6. pgv_history_gather writes `count` rows of [K*C][64][64] elements of `dtype`, K = stack in 1 .. 8, slot K-1 the newest
 *      frame, values by the policy observations' value rule.  For an entry (p, i): f_0 = p; for j = 1 .. K-1, f_j = f_(j-1)
 *      if began[f_(j-1)][i] is set or push f_(j-1) - 1 is not held, else f_(j-1) - 1; row slot K-1-j is frame f_j.  So a stack
 *      never mixes episodes, an env that just began holds K copies of its first frame, and a walk that reaches the oldest
 *      held push repeats that push.  An entry whose p is not held, or whose env is outside 0 .. N-1, gives a row of zero
 *      bytes; nothing faults for any index values, and an entry may appear more than once.  "Held" is judged by head as
 *      it stands when the call is made.  count = 0 succeeds and does nothing.  Checked on the host before anything is
 *      enqueued: stack, dtype, count < 0, d_out 16-byte aligned, NULL pointers with count > 0.
 *   7. pgv_history_enable may be called once per env, at any time.  Each refusal leaves a message and the engine as it was:
 *      a second call, capacity < 1, gray outside 0 .. 1, a `frames` that is not 16-byte aligned, a struct_size too small, a
 *      failed allocation.  It sets every pending flag and pushes nothing.  The engine's own `frames` start as zeros; a
 *      caller's are as the caller left them.
 *
 * The law that ties the two features: on an engine with both enabled at the same moment, the same `gray`, and T >= K,
 * gather(p = head - 1, envs 0 .. N-1, K, dtype) equals pgv_policy_obs bit for bit after every call of point 4 and after
 * every pgv_reset.  (pgv_policy_obs_push under a mask by hand has no counterpart here.) */
typedef struct pgv_history_config {
    uint32_t struct_size;
    int32_t capacity; /* T >= 1 time slots */
    int32_t gray;     /* 0: planes R, G, B; 1: one plane, the gray rule of the policy observations */
    void* frames;     /* device, 16-byte aligned, T*N*C*4096 bytes; NULL: the engine allocates (zeroed) */
} pgv_history_config;
PGV_API int32_t pgv_history_enable(pgv_env* env, const pgv_history_config* config);
PGV_API uint8_t* pgv_history_frames(pgv_env* env);        /* device u8 [T][N][C][64][64]; NULL before enable */
PGV_API const uint8_t* pgv_history_began(pgv_env* env);   /* device u8 [T][N]; NULL before enable */
PGV_API const uint8_t* pgv_history_pending(pgv_env* env); /* device u8 [N]: the pending "began" flags; NULL before enable */
PGV_API int64_t pgv_history_head(pgv_env* env);           /* pushes so far (host counter, no synchronisation); 0 before enable, -1 for NULL */
PGV_API int32_t pgv_history_capacity(pgv_env* env);       /* T; 0 before enable */
PGV_API int32_t pgv_history_push(pgv_env* env);           /* by hand: all envs, a new slot */
PGV_API int32_t pgv_history_gather(pgv_env* env, const int64_t* d_pushes, const int32_t* d_envs, int32_t count, int32_t stack,
                                   int32_t dtype /* PGV_POLICY_* */, void* d_out);

/* Augmented gathers: pgv_history_gather with a random shift or crop (RAD, DrAC, DrQ's pad-and-shift) and a cutout (RAD's
 * cutout and cutout-color) worked into the same pass — on the stored u8 bytes, in front of the value rule, so the result is
 * exact and can be held bit for bit to a model.  The gather reads the stored bytes once and writes the row once either way:
 * a window only changes which stored byte an element reads, a cutout replaces some bytes.
 *
 *   1. Output.  `count` rows of [K*C][H'][W'] elements of `dtype`, contiguous, H' = out_height, W' = out_width; slot K-1 the
 *      newest frame.  The frames f_0 .. f_(K-1) of an entry are those of point 6 of the frame history: the same walk, the
 *      same began bytes, "held" judged by head at the call.
 *   2. The draws of entry e (its position in the call), all arithmetic uint32 and wrapping, mix32 the engine's hash
 *      (x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16):
 *          word(j)   = mix32( mix32(seed + 0x9E3779B9*(e+1)) ^ (j*0x85EBCA6B + 0xC2B2AE35) )
 *          draw(m,j) = (uint64(word(j)) * m) >> 32                                  (pgv_synthetic_action's rule)
 *          oy = -pad + draw(64 + 2*pad - H' + 1, 0)      ox = -pad + draw(64 + 2*pad - W' + 1, 1)
 *      and with cutout_max > 0
 *          ch = min(H', cutout_min + draw(max-min+1, 2))    cw = min(W', cutout_min + draw(max-min+1, 3))
 *          cy = draw(H' - ch + 1, 4)    cx = draw(W' - cw + 1, 5)    colour = word(6), 0 with PGV_AUG_CUTOUT_BLACK;
 *      without, ch = cw = cy = cx = colour = 0.  Plane c of an RGB ring uses byte c of colour, the gray plane byte 0.  They
 *      are a function of (aug, e) and of nothing else: not of count, of the other entries, or of whether the entry is held.
 *   3. The element at (slot s, plane c, y, x): where cy <= y < cy+ch and cx <= x < cx+cw the byte is the plane's colour byte;
 *      else, with sy = oy+y and sx = ox+x both in 0 .. 63, the stored byte of frame f_(K-1-s), plane c, at (sy, sx); outside
 *      the frame that byte at the coordinates clamped to 0 .. 63 (PGV_AUG_EDGE_REPLICATE) or byte 0 (PGV_AUG_EDGE_ZERO).  The
 *      element is the policy observations' value of that byte.  One window and one rectangle per entry, shared by its K
 *      frames and all planes.  An entry that is not held, or whose env is outside the batch, gives a row of zero bytes,
 *      cutout or not.
 *   4. `params`, where not NULL, receives {oy, ox, cy, cx, ch, cw, colour & 0xFFFFFF, 0} per entry, held or not; on a gray
 *      ring the seventh word is colour & 0xFF, the one byte it used.  pgv_gather_aug_params gives the same row on the host,
 *      in the RGB form (it knows no ring).
 *   5. Laws.  With H' = W' = 64, pad = 0 and cutout_max = 0 the output equals pgv_history_gather's bit for bit, for any seed
 *      and edge.  The call changes nothing — ring, began bytes, pending flags, head, engine state — and a second call gives
 *      the same bytes.
 *   6. Checked on the host before anything is enqueued, each refusal leaving a message and the engine as it was: everything
 *      pgv_history_gather refuses; aug NULL or its struct_size too small; H' outside 1 .. 64; W' outside 8 .. 64 or no
 *      multiple of 8; pad outside 0 .. 16; an unknown edge or colour mode; cutout sides outside 0 .. 64, min > max, min = 0
 *      with max > 0; d_out not 16-byte aligned; params not 4-byte aligned.  count = 0 succeeds and does nothing.  The call
 *      is enqueued on the env's stream, allocates nothing and does not synchronise.  pgv_gather_aug_params makes the same
 *      checks of `aug` and refuses entry < 0. */
#define PGV_AUG_EDGE_REPLICATE 0 /* a source pixel outside the frame is the nearest pixel of the frame (DrQ's replicate pad) */
#define PGV_AUG_EDGE_ZERO 1      /* ... is byte 0 */
#define PGV_AUG_CUTOUT_BLACK 0   /* the rectangle is byte 0 in every plane (RAD cutout) */
#define PGV_AUG_CUTOUT_RANDOM 1  /* one drawn byte per plane (RAD cutout-color) */
typedef struct pgv_gather_aug {
    uint32_t struct_size;
    int32_t out_height, out_width;  /* H' in 1 .. 64; W' in 8 .. 64 and a multiple of 8 */
    int32_t pad;                    /* 0 .. 16: how far the window may hang over each edge of the frame */
    int32_t edge;                   /* PGV_AUG_EDGE_* */
    int32_t cutout_min, cutout_max; /* side lengths; max = 0 (then min = 0): no cutout; else 1 <= min <= max <= 64 */
    int32_t cutout_color;           /* PGV_AUG_CUTOUT_* */
    uint32_t seed;
    int32_t* params;                /* device int32 [count][8] or NULL: what was drawn for each entry */
} pgv_gather_aug;
PGV_API int32_t pgv_history_gather_aug(pgv_env* env, const int64_t* d_pushes, const int32_t* d_envs, int32_t count,
                                       int32_t stack, int32_t dtype, const pgv_gather_aug* aug, void* d_out);
/* The draws of entry `entry` under `aug` (host, pure, no GPU, env not needed): h_params8[0..7] as `params` rows are. */
PGV_API int32_t pgv_gather_aug_params(const pgv_gather_aug* aug, int32_t entry, int32_t* h_params8);

/* Transitions on the device: the other half of a rollout beside the frame history — a ring of what every call did (the
 * action, the reward, how it ended), the n-step transition gather of replay learners and the GAE recurrence of on-policy
 * ones, each one launch.  The engine is the only party that knows, without a look from the host, the action of a synthetic
 * step, the terminal reward a same-step reset wipes from the reward row, terminated against truncated, and the step that
 * only served an auto-reset.  Opt-in per engine, on top of the frame history: an engine that never enables it launches
 * nothing new and gives the same bytes as before at every entry point.
 *
 *   1. Rows.  `action` int32 [T][N], `reward` float32 [T][N], `flags` u8 [T][N], T the history's capacity.  Row q lives in
 *      slot q % T and describes the call that made push q + 1: the action taken on frame q, what it earned, how it ended —
 *      obs[t], action[t], reward[t], done[t].  Flag bits: PGV_TR_RECORDED, PGV_TR_TERMINATED, PGV_TR_TRUNCATED, PGV_TR_VOID.
 *      VOID: the step found the env's `done` row set and only served its auto-reset; its action was ignored and it is no
 *      step of an episode.  It is the event that sets the history's pending flag "from the `done` row as the step finds it",
 *      filed by the same flag kernel into a pending byte of the feature's own, which the row's write reads and clears.
 *   2. Who writes row head - 1, in front of the history push of the same call (head as the call finds it; at head = 0
 *      there is no row and only the pending bytes are cleared): the single steps, with the caller's action as given — for a
 *      synthetic step the value pgv_synthetic_action gives for (run_seed, the step's index, env_offset + i), evaluated on the
 *      device —, the engine's reward row, TERMINATED from the `done` row, VOID from the pending byte, never TRUNCATED; the
 *      three episode steps, with reward, TERMINATED and TRUNCATED from the episode outputs (the terminal step's values, which a
 *      same-step reset has wiped from the engine's own rows) and VOID as above (it occurs in next-step mode, and after a load
 *      of an env whose reset was due).  Every other call that opens a slot — the push by hand, and the drawn sequences —
 *      writes action 0, reward 0, flags 0 for all envs: not recorded, so a stale row of push q - T is never taken for
 *      row q.  pgv_reset writes no row: it rewrites the newest frame with began = 1, and that byte is how an interruption
 *      from outside shows (a reset, a load of envs or of a snapshot, new levels).  A sequence without frames writes no row and
 *      clears the pending bytes behind its last sub-step.  The measurement calls that step without pushing (pgv_timed_steps,
 *      pgv_step_times, pgv_step_phases, pgv_step_synthetic_many, pgv_step_episodes_times) write no row and leave the pending
 *      bytes they set: they are not for the middle of a recorded rollout.
 *   3. Row q is COMPLETE when pushes q and q + 1 are both held, judged by head as the call is made, and RECORDED is set.  It
 *      is CUT when it is complete, none of TERMINATED, TRUNCATED, VOID is set and began[q + 1][i] is.  The ring travels neither
 *      in records nor in snapshots: pgv_snapshot_bytes and pgv_env_record_bytes are what they were.
 *   4. pgv_transitions_gather, entry (p, i), n = `n` in 1 .. 64.  The entry is VALID when 0 <= i < N and row p is complete
 *      and not VOID; an invalid entry gives rows of zero bytes and zero scalars, nothing faults for any index values, and an
 *      entry may appear more than once.  The walk: m = 0, ret = 0, disc = 1; for k = 0 .. n-1: stop in front of row p + k if
 *      it is not complete or is VOID; else t = disc * r; ret = ret + t; disc = disc * gamma; m = m + 1 — three float32
 *      roundings, no fused multiply-add, the rule of `ended_return` —; then stop behind the row if it is TERMINATED,
 *      TRUNCATED or CUT.  Outputs, each device pointer optional (NULL: not written): `action` row p's; `nstep_return` ret;
 *      `steps` m; `discount` 0 if the last row walked was TERMINATED, else disc; `status` bit 0 = valid, and
 *      PGV_TR_TERMINATED, PGV_TR_TRUNCATED, PGV_TR_CUT of the last row walked; `obs` exactly the row of
 *      pgv_history_gather for (p, i, stack, dtype) and `next_obs` the row for (p + m, i, stack, dtype): the same walk over
 *      `began`, the same value rule, the same zero row.  Under TRUNCATED or CUT the status says that next_obs is not the
 *      successor state; under a same-step TERMINATED it is the new episode's first frame, and discount = 0 masks it.
 *      Checked on the host before anything is enqueued: the query and its struct_size, n, stack, dtype, count < 0, obs and
 *      next_obs 16-byte aligned, the int32 and float outputs 4-byte aligned, NULL index lists with count > 0.  count = 0
 *      succeeds and does nothing.  One launch; the call changes nothing of the engine.
 *   5. pgv_transitions_gae over rows first .. first + L - 1, L >= 1, all of which must have head - T <= q and q + 1 < head
 *      (else refused): values f32 [L+1][N], optional trunc_values f32 [L][N], advantages f32 [L][N], optional returns f32
 *      [L][N].  Per env, t = L-1 .. 0, carry = 0: a row that is not RECORDED or is VOID gives adv = 0, carry = 0, ret =
 *      V[t]; else nv = V[t+1] if the row ends nothing, 0 if TERMINATED or CUT, trunc_values[t] (0 without the array) if
 *      TRUNCATED; a = gamma * nv; b = r + a; delta = b - V[t]; adv = delta + c * carry with c = gamma * lambda computed
 *      once if the row ends nothing, else delta — the product and the sum separate roundings —; carry = adv; ret = adv +
 *      V[t].  One launch, nothing allocated, no atomics, no host synchronisation.
 *   6. pgv_transitions_enable needs pgv_history_enable first and a capacity T >= 2, and may be called once, at any time; the
 *      rows start as zeros (not recorded).  Each refusal leaves a message and the engine as it was. */
#define PGV_TR_RECORDED 1
#define PGV_TR_TERMINATED 2
#define PGV_TR_TRUNCATED 4
#define PGV_TR_VOID 8
#define PGV_TR_CUT 16 /* in a gathered status only */
typedef struct pgv_transitions_config {
    uint32_t struct_size;
    uint32_t reserved; /* 0 */
} pgv_transitions_config;
typedef struct pgv_transition_query {
    uint32_t struct_size;
    int32_t n;     /* 1 .. 64 */
    float gamma;
    int32_t stack; /* K, 1 .. 8 */
    int32_t dtype; /* PGV_POLICY_* */
    void* obs;           /* device [count][K*C][64][64] elements, 16-byte aligned, or NULL */
    void* next_obs;      /* the same */
    int32_t* action;     /* device [count] or NULL, and so on */
    float* nstep_return;
    float* discount;
    int32_t* steps;
    uint8_t* status;
} pgv_transition_query;
typedef struct pgv_gae {
    uint32_t struct_size;
    float gamma, lambda;
    const float* values;       /* device f32 [L+1][N] */
    const float* trunc_values; /* device f32 [L][N] or NULL */
    float* advantages;         /* device f32 [L][N] */
    float* returns;            /* device f32 [L][N] or NULL */
} pgv_gae;
PGV_API int32_t pgv_transitions_enable(pgv_env* env, const pgv_transitions_config* config);
PGV_API const int32_t* pgv_transitions_action(pgv_env* env); /* device int32 [T][N]; NULL before enable */
PGV_API const float* pgv_transitions_reward(pgv_env* env);   /* device f32 [T][N]; NULL before enable */
PGV_API const uint8_t* pgv_transitions_flags(pgv_env* env);  /* device u8 [T][N]; NULL before enable */
PGV_API int32_t pgv_transitions_gather(pgv_env* env, const int64_t* d_pushes, const int32_t* d_envs, int32_t count,
                                       const pgv_transition_query* query);
PGV_API int32_t pgv_transitions_gae(pgv_env* env, int64_t first, int32_t length, const pgv_gae* gae);

/* cenv_render for one env of the batch (games/coinrun/coinrun.cpp:393-411, render_game(false)): the human-size frame,
 * width x height x 3 bytes row-major RGB into a HOST buffer.  Synchronises the env's stream.  Debug / viewer path. */
PGV_API int32_t pgv_render_frame(pgv_env* env, int32_t index, int32_t width, int32_t height, uint8_t* h_rgb);

/* The W x H human frames (cenv_render, render_game(false)) of `count` envs of the batch into DEVICE memory:
 * u8 [count][height][width][3], row-major RGB.  d_indices: device int32[count], or NULL for envs 0 .. count-1; the same
 * env may be named more than once, and an index outside the batch gives a frame of zeros.  1 <= width, height <= 4096;
 * count = 0 succeeds and does nothing.  Enqueued on the env's stream; nothing is synchronised, nothing allocated.  One
 * workgroup paints one 64x64 tile of one frame (pg_frame.h), so the whole device works on a batch at any size. */
PGV_API int32_t pgv_render_frames(pgv_env* env, const int32_t* d_indices, int32_t count, int32_t width, int32_t height,
                                  uint8_t* d_rgb);
/* Host-pointer convenience (synchronous; allocates and frees its device buffers), as pgv_step_host is to pgv_step. */
PGV_API int32_t pgv_render_frames_host(pgv_env* env, const int32_t* h_indices, int32_t count, int32_t width,
                                       int32_t height, uint8_t* h_rgb);

/* Symbolic observations: what the games know, for every env at once, in device memory — the agent, every entity's kind,
 * position and liveness, the goal, the tile map — as rows of floats and bytes (the parity taps below read one env's rows
 * through the same kernels).  For privileged critics, probes and auxiliary losses, scripted and planning agents; with
 * pgv_step_sequence's frameless steps such an agent runs without a frame being drawn.
 *
 *   1. Layout.  pgv_state_layout_of(game_id, mode) is host-only and pure: no GPU, no env.  PGV_MODE_DEFAULT stands for the
 *      mode the game is compiled with; a mode pgv_game_modes does not offer is refused, as are an unknown game id, out NULL
 *      and a struct_size that is too small.  A state row is `width` floats: `fixed` floats that every row has, then up to
 *      max_records records of `record` floats (record = 0: every row is `fixed` long).  A tile row is `cells` = tile_w *
 *      tile_h bytes, cell (x, y) at byte y + x * tile_h, y counted as the game's tile map counts it; all three are 0 for a
 *      game without a tile map (bossfight).  The layout is a function of (game, mode) alone.
 *   2. Names.  pgv_state_names writes the names of the `fixed` floats, then '|', then the names of one record's floats,
 *      names separated by single spaces, NUL-terminated and cut to cap bytes where cap is short, and returns the length the
 *      whole string needs without its NUL (-1 where pgv_state_layout_of would refuse; buf may be NULL).  The names are
 *      unique within a game and the first two are agent_x agent_y in every game.  INTEGRATION.md lists the columns of every
 *      game, the rule from a cell index to (x, y), and the tile ids.
 *   3. Rows.  d_rows is device f32 [count][width], contiguous.  Row k holds the state dump of env indices[k] — bit for bit
 *      the oracle's, and what pgv_dump_state copies out of such a row — followed by +0.0f up to width; d_lengths[k] (device
 *      int32 [count], or NULL) is the dump's length.  d_tiles is device u8 [count][cells], contiguous: the env's tile ids, as
 *      pgv_dump_tiles copies them out.
 *   4. Indices.  d_indices is device int32 [count], or NULL for envs 0 .. count-1.  The same env may be named more than once;
 *      an index outside the batch gives a row of zero bytes and length 0; nothing faults for any index value.
 *   5. Ordering and state.  The calls read the state as it stands at that point of the env's stream: behind a step, a reset,
 *      a same-step auto-reset (the new episode, as the observation shows), a frameless pgv_step_sequence; between any two
 *      calls.  They change nothing — an engine that called them goes on exactly as one that did not, and a second call
 *      gives the same bytes.  They are enqueued on the env's stream, allocate nothing and do not synchronise the host.
 *      Nothing is written per step: an engine that never calls them launches nothing for them.
 *   6. Checked on the host before anything is enqueued, each refusal leaving a message and the engine as it was: env NULL;
 *      count < 0; with count > 0 an output that is NULL or whose base is not 16-byte aligned (d_lengths: 4-byte).  count = 0
 *      succeeds and writes nothing; pgv_tile_rows on a game without a tile map succeeds and writes nothing.
 *   7. The _host forms take host pointers, allocate and free their device buffers and are synchronous, as
 *      pgv_render_frames_host is; they ask no alignment. */
typedef struct pgv_state_layout {
    uint32_t struct_size;
    int32_t width;          /* floats per row: the longest dump this configuration can produce */
    int32_t fixed;          /* floats every row has */
    int32_t record;         /* floats per variable record behind them; 0: every row is `fixed` long */
    int32_t max_records;    /* width == fixed + record * max_records */
    int32_t cells;          /* bytes per tile row; 0 for a game without a tile map (bossfight) */
    int32_t tile_w, tile_h; /* cells == tile_w * tile_h */
} pgv_state_layout;
PGV_API int32_t pgv_state_layout_of(int32_t game_id, int32_t mode, pgv_state_layout* out); /* set struct_size first */
PGV_API int64_t pgv_state_names(int32_t game_id, int32_t mode, char* buf, int64_t cap);
PGV_API int32_t pgv_state_rows(pgv_env* env, const int32_t* d_indices, int32_t count, float* d_rows, int32_t* d_lengths);
PGV_API int32_t pgv_tile_rows(pgv_env* env, const int32_t* d_indices, int32_t count, uint8_t* d_tiles);
PGV_API int32_t pgv_state_rows_host(pgv_env* env, const int32_t* h_indices, int32_t count, float* h_rows, int32_t* h_lengths);
PGV_API int32_t pgv_tile_rows_host(pgv_env* env, const int32_t* h_indices, int32_t count, uint8_t* h_tiles);

/* Path distances: the breadth-first distance field of every named env's tile map from one source cell, and what a second
 * cell — the probe — sees of it.  The first thing a scripted or planning agent, a privileged critic or a level-scoring
 * curriculum computes from a tile map: the distance from the mouse to the cheese and the move that shortens it, from a
 * chaser enemy to the agent, the optimal episode length of a maze.  The field is a geometric distance over cells: in the
 * platformers it knows nothing of jumps or gravity.
 *
 *   1. Cells.  Cell (x, y) is index y + x * tile_h, exactly as in pgv_tile_rows.  The cell of a world point (wx, wy) is
 *      x = floor(wx), y = tile_h - 1 - floor(wy); a point whose cell is outside the map has no cell.
 *   2. The agent's cell is the cell of the centre of the agent's body box, (agent_x, agent_y + agent_dy), the sum one
 *      float32 addition: agent_dy is 0 in maze, chaser and caveflyer, -0.5f in coinrun and climber, -0.4f in jumper.
 *      The goal's cell is the cell of (goal_x, goal_y) in maze and jumper and of record 0's (x, y) in caveflyer (entity 0
 *      is the goal); the other games have no goal.  pgv_path_layout_of gives both facts, and the map's size, on the host:
 *      no GPU, no env, refusals as pgv_state_layout_of.  cells is 0 for a game without a tile map (bossfight).
 *   3. Passable.  Bit t of `passable` set: a cell whose tile id, as pgv_tile_rows gives it, is t may be entered.  Ids >= 32
 *      are never passable; a mask of 0 is legal.  INTEGRATION.md lists the tile ids and a sensible set for every game.
 *   4. Distance.  The source cell has distance 0 whatever its tile.  A cell has distance d + 1 when it is passable, is not
 *      yet reached, and has a 4-neighbour at distance d.  There is no wrap at any edge.  Any other cell is -1.  dist is
 *      device int16 [count][cells], laid out as the tile rows are (the longest path is below 4 096); a row with no source
 *      is all -1.
 *   5. Probe.  probe_dist[k] is the distance at the probe cell, -1 when it is not reached or the row has no probe cell.
 *      probe_step[k] is 0 when that distance is <= 0, otherwise the first of x-1 (code 1), x+1 (2), y-1 (3), y+1 (4)
 *      whose distance is one less.  cells_out[k] = {source cell, probe cell}, -1 for none.
 *   6. Source and probe are each PGV_PATH_AGENT, PGV_PATH_GOAL or PGV_PATH_CELLS — caller-given cells, device int32 [count],
 *      a value outside 0 .. cells-1 meaning no cell; the probe may also be PGV_PATH_NONE.
 *   7. Indices, ordering and state are points 4 and 5 of the symbolic observations: d_indices may be NULL, may repeat and
 *      may name an env outside the batch — such a row is -1 everywhere, with a -1 probe distance, step 0 and cells -1.
 *      The call is enqueued on the env's stream, allocates nothing, does not synchronise and changes nothing; an engine
 *      that never calls it launches nothing for it.  count = 0 succeeds and writes nothing.
 *   8. Checked on the host before anything is enqueued, each refusal leaving a message and the engine as it was: env or
 *      struct NULL; struct_size too small; count < 0; an unknown source or probe, or source = PGV_PATH_NONE;
 *      PGV_PATH_GOAL on a game without a goal; PGV_PATH_CELLS with a NULL cell pointer and count > 0; dist not 16-byte
 *      aligned, probe_dist or cells_out not 4-byte aligned; every output NULL with count > 0; a game without a tile map.
 *   9. The _host form takes host pointers throughout (indices, cells, outputs), allocates and frees its device buffers and
 *      is synchronous, as pgv_tile_rows_host is; it asks no alignment. */
#define PGV_PATH_NONE 0 /* probe only */
#define PGV_PATH_AGENT 1
#define PGV_PATH_GOAL 2
#define PGV_PATH_CELLS 3
typedef struct pgv_tile_paths {
    uint32_t struct_size;
    uint32_t passable;           /* bit t: tile id t may be entered */
    int32_t source;              /* PGV_PATH_AGENT, _GOAL or _CELLS */
    const int32_t* source_cells; /* [count], for PGV_PATH_CELLS */
    int32_t probe;               /* PGV_PATH_NONE, _AGENT, _GOAL or _CELLS */
    const int32_t* probe_cells;  /* [count], for PGV_PATH_CELLS */
    int16_t* dist;               /* [count][cells], base 16-byte aligned, or NULL */
    int32_t* probe_dist;         /* [count] or NULL */
    uint8_t* probe_step;         /* [count] or NULL */
    int32_t* cells_out;          /* [count][2]: source cell, probe cell, -1 for none; or NULL */
} pgv_tile_paths;
PGV_API int32_t pgv_tile_paths_rows(pgv_env* env, const int32_t* d_indices, int32_t count, const pgv_tile_paths* paths);
PGV_API int32_t pgv_tile_paths_rows_host(pgv_env* env, const int32_t* h_indices, int32_t count, const pgv_tile_paths* paths);
typedef struct pgv_path_layout {
    uint32_t struct_size;
    int32_t cells, tile_w, tile_h; /* as pgv_state_layout has them */
    int32_t has_goal;              /* 1: PGV_PATH_GOAL is served */
    float agent_dx, agent_dy;      /* the agent's cell is the cell of (agent_x + agent_dx, agent_y + agent_dy); agent_dx is 0 */
} pgv_path_layout;
PGV_API int32_t pgv_path_layout_of(int32_t game_id, int32_t mode, pgv_path_layout* out); /* set struct_size first */

/* Caller-made levels: levels as values.  pgv_get_levels reads the level of any envs into device memory, the caller edits it
 * there, pgv_set_levels installs rows into any envs as the start of a new episode.  (What unsupervised environment design —
 * PAIRED, ACCEL, robust PLR — maze interpretability and hand-built evaluation sets need; pgv_assign_levels only names a
 * generator seed.  The reference has no counterpart.)  For maze, in every mode it has; the other games' levels carry entity
 * lists and are refused.
 *
 * A level is a row of pgv_level_rows: the tile row as pgv_tile_rows lays it out (cells bytes, 0 open, 1 wall), the agent's
 * and the goal's cell by the rule of point 1 of the path distances (cell (x, y) = y + x * tile_h; a point stands on its
 * cell's centre, agent_x = x + 0.5, agent_y = tile_h - 1 - y + 0.5), the floor picture (0 .. backgrounds - 1) and its shift.
 * pgv_level_layout_of is host-only and pure — no GPU, no env, refusals as pgv_state_layout_of — and says supported = 1 with
 * the map's size for maze in each of its modes, supported = 0 and zeros for the six other games.
 *
 * pgv_get_levels is the read-only form: the level of each named env as it stands, the agent's current cell included; it
 * changes nothing and a second call gives the same bytes.  Every field equals what pgv_tile_rows and pgv_state_rows give
 * (background, background_shift: columns floor, floor_shift).  d_indices as for pgv_tile_rows: NULL for envs 0 .. count-1,
 * repeats allowed, an index outside the batch gives a zero tile row, cells of -1, background 0 and shift +0.0f.  Any output
 * pointer may be NULL; ids and status are not written.
 *
 * pgv_set_levels:
 *   1. Every row is judged on the device and its status written to status[k] (where status is not NULL); nothing is
 *      reported through the host.  A row that is refused leaves its env untouched.  The first that applies:
 *        PGV_LEVEL_INSTALLED  0  installed;
 *        PGV_LEVEL_NO_ENV     1  the index is outside the batch (a caller's way to a fixed-size call, as for
 *                                pgv_assign_levels);
 *        PGV_LEVEL_BAD_TILE   2  a tile byte is neither 0 (open) nor 1 (wall);
 *        PGV_LEVEL_BAD_AGENT  3  the agent's cell is outside the map, or is a wall;
 *        PGV_LEVEL_BAD_GOAL   4  the goal's cell is outside the map, is a wall, or is the agent's cell;
 *        PGV_LEVEL_BAD_FLOOR  5  background is outside 0 .. backgrounds - 1, or background_shift is not a finite value in
 *                                [0, 1).
 *      With background or background_shift NULL every env keeps the value it has: an edited level keeps its look.
 *   2. An accepted row is a pgv_reset of its env with the caller's level in place of a generated one.  The live state is
 *      what the generator's own install leaves: the tiles (and the block's padding bytes), the two points, the floor, steps
 *      0, facing forward, the camera on the world centre.  The env's obs row is the level's first frame, its reward 0, its
 *      done 0, and an auto-reset that was pending for it is cleared.  Everything pgv_reset does for the envs it names is
 *      done for the installed envs and for no other: the policy observations restart and are pushed under the mask (point 4
 *      there), the frame history's newest slot is rewritten (point 5 there), the episodes' running return and length are
 *      zeroed.
 *   3. What an install does NOT touch: the env's mt19937 stream, its generator chain, its shadow slot, a pending level
 *      assignment, its place in its level sequence.  When the custom episode ends, the auto-reset builds the level the env
 *      would have built anyway; a caller who wants another custom level installs one on the envs that ended — behind a
 *      same-step pgv_step_episodes that is indices = where(ended, arange, -1), with no look from the host.
 *   4. Labels.  pgv_level_numbers[i] = ids[k], or 0 with ids NULL, and pgv_level_known[i] = 2, "the caller's label": so
 *      ended_level / ended_level_known say which custom level an episode's return belongs to.  Nothing else writes 2.
 *   5. The indices of one call must be distinct; d_indices NULL stands for envs 0 .. count-1.  Of two rows that name one
 *      env, one is installed whole and the other is dropped, both with status 0 (nothing faults).
 *   6. count = 0 succeeds and writes nothing.  Checked on the host before anything is enqueued, each refusal leaving a
 *      message and the engine as it was: env or struct NULL; struct_size too small; count < 0; a game without caller-made
 *      levels ("no caller-made levels for this game", pgv_get_levels too); tiles, agent_cell or goal_cell NULL with
 *      count > 0; a pointer to 4-byte elements that is not 4-byte aligned (tiles may lie anywhere); with the policy
 *      observations or the frame history enabled, an obs slab that is not 16-byte aligned.
 *   7. The call is enqueued on the env's stream, allocates nothing and does not synchronise the host.  It touches nothing
 *      the level generator's side stream reads or writes, so it is not ordered against it and launches no generator.  Cost:
 *      one clear of the call's scratch, one launch of a wavefront a row, and pgv_reset's render and bookkeeping launches
 *      under the mask (measurements: docs/OPTLOG.md).
 *   8. Records and snapshots: a custom level is live state and nothing else, so it travels in pgv_save_envs and
 *      pgv_save_state as any level does; neither layout changed.
 * The _host forms take host pointers throughout (indices and every pointer of the struct), allocate and free their device
 * buffers and are synchronous, as pgv_tile_rows_host is; they ask no alignment. */
#define PGV_LEVEL_INSTALLED 0
#define PGV_LEVEL_NO_ENV 1
#define PGV_LEVEL_BAD_TILE 2
#define PGV_LEVEL_BAD_AGENT 3
#define PGV_LEVEL_BAD_GOAL 4
#define PGV_LEVEL_BAD_FLOOR 5
typedef struct pgv_level_layout {
    uint32_t struct_size;
    int32_t supported;       /* 1: pgv_get_levels / pgv_set_levels serve this game in this mode */
    int32_t cells;           /* bytes per tile row */
    int32_t tile_w, tile_h;  /* cells == tile_w * tile_h */
    int32_t backgrounds;     /* floor pictures: background is 0 .. backgrounds - 1 */
} pgv_level_layout;
PGV_API int32_t pgv_level_layout_of(int32_t game_id, int32_t mode, pgv_level_layout* out); /* set struct_size first */
typedef struct pgv_level_rows { /* device pointers; [count] rows parallel to the indices */
    uint32_t struct_size;
    uint8_t* tiles;          /* [count][cells], laid out as pgv_tile_rows */
    int32_t* agent_cell;     /* [count]  cell index y + x * tile_h */
    int32_t* goal_cell;      /* [count] */
    int32_t* background;     /* [count]  floor picture; may be NULL */
    float* background_shift; /* [count]  may be NULL */
    uint32_t* ids;           /* [count]  the caller's labels, install only; may be NULL */
    int32_t* status;         /* [count]  install only: PGV_LEVEL_* per row; may be NULL */
} pgv_level_rows;
PGV_API int32_t pgv_get_levels(pgv_env* env, const int32_t* d_indices, int32_t count, const pgv_level_rows* out);
PGV_API int32_t pgv_set_levels(pgv_env* env, const int32_t* d_indices, int32_t count, const pgv_level_rows* in);
PGV_API int32_t pgv_get_levels_host(pgv_env* env, const int32_t* h_indices, int32_t count, const pgv_level_rows* out);
PGV_API int32_t pgv_set_levels_host(pgv_env* env, const int32_t* h_indices, int32_t count, const pgv_level_rows* in);

/* Measurement helper for bench.py: runs `steps` synthetic steps and returns, from HIP events recorded
 * on the env's stream, the total time of the region and the summed time of the dominant (render)
 * kernel launches inside it. */
PGV_API int32_t pgv_timed_steps(pgv_env* env, int32_t steps, uint32_t run_seed, double* total_ms,
                                double* render_kernel_ms);
/* render_kernel_ms == NULL: the region holds nothing but the steps between its two events (no per-launch events): the
 * form `value` is measured with.  render_kernel_ms is the render KERNEL's launches alone: a game's render pre-pass
 * (setup_kernel, since round 4 a launch of its own in front of the render kernel) is NOT in it — pgv_step_phases
 * reports that one beside it.
 *
 * Per-step detail for the same kind of run: h_step_ms[s] = time from the start of step s to the start of step s+1 (to
 * the end of the run for the last), h_render_ms[s] = its render launch (again without the pre-pass), both from HIP events
 * on the env's stream (host arrays of `steps` floats, either may be NULL).  For latency percentiles and the roofline
 * window — never for `value`: events sit inside the region. */
PGV_API int32_t pgv_step_times(pgv_env* env, int32_t steps, uint32_t run_seed, float* h_step_ms, float* h_render_ms);
/* The same run with a step cut into its four phases by events on the env's stream (any pointer may be NULL):
 *   h_logic_ms    the logic kernels (level install / auto-reset, agent, entities, resolve — whatever the game launches
 *                 in front of its frame), including the side-stream launch of the level generator;
 *   h_prepass_ms  the render pre-pass (setup_kernel; 0 for a game or debug mode without one);
 *   h_render_ms   the render kernel (jumper: + the list kernel that walks the frames the pre-pass handed back);
 *   h_late_ms     what follows the render launch inside the step (chaser: the join with its reset stream and the late
 *                 pass over the envs that were reset).
 * logic + prepass + render + late = step.  bench.py's roofline.render_path is prepass + render + late. */
PGV_API int32_t pgv_step_phases(pgv_env* env, int32_t steps, uint32_t run_seed, float* h_step_ms, float* h_logic_ms,
                                float* h_prepass_ms, float* h_render_ms, float* h_late_ms);
/* … of `count` envs stepping side by side, each on its own stream (the mixed workload: step s of every env is enqueued
 * before step s+1 of any, as pgv_step_synthetic_many does).  h_ms: host floats [count][5][steps] — per env: step, logic,
 * prepass, render, late.  The streams overlap on the device, so an env's phases are what ITS stream saw, not a share of
 * the wall clock. */
PGV_API int32_t pgv_step_phases_many(pgv_env* const* envs, int32_t count, int32_t steps, uint32_t run_seed, float* h_ms);

/* Debug switches (tests only); none changes a result.  Bit 0: render the background and tile layer by replaying the
 * draw list one blit at a time instead of the fused row composer.  Bit 8: no level prefetch — every reset generates its
 * level inside the step.  Bit 21: no render pre-pass — every frame's workgroup does its own set-up, as the frames the
 * pre-pass hands back do anyway.  Bit 23: the pre-pass hands back every third env's frame (the way for tests to the
 * hand-back path of games that never take it in a normal run).  Bit 24: coinrun works every hazard's boxes out behind
 * the agent instead of the few its entity lanes pre-selected (the fallback a normal run never takes).  Bit 25: chaser's
 * enemies take their turns one after the other on the env's random stream itself instead of side by side on outputs
 * peeked from it (what the last few words of a 624-word block take in a normal run).  Bit 26: a push of the policy
 * observations stores each lane's own 16 values per plane as they lie (lanes 32 or 64 bytes apart for 2- and 4-byte elements)
 * instead of exchanging them inside the wave for dense stores.  Bit 27: coinrun draws a frame its pre-pass hands back in
 * that env's own block of the render launch instead of in one of the early blocks in front of the grid (what a frame
 * does anyway that finds the list of such frames full).  Any other bit is refused. */
PGV_API int32_t pgv_set_debug(pgv_env* env, int32_t flags);

/* Parity taps (host pointers): the state row / tile row of one env, read through the launches behind pgv_state_rows /
 * pgv_tile_rows: row k = 0 of a call with indices = {index}, without its padding.  Return the dump's full length, whatever
 * cap is, and copy min(cap, length) items (cap <= 0: nothing is written, h_out may be NULL); pgv_dump_tiles of a game
 * without a tile map returns 0.  -1 for a NULL env or an index outside 0 .. n-1 — and for a HIP error inside the call,
 * which then leaves its text in pgv_last_error.  Synchronous; a tap waits for the env's stream alone and allocates
 * nothing. */
PGV_API int32_t pgv_dump_state(pgv_env* env, int32_t index, float* h_out, int32_t cap);
PGV_API int32_t pgv_dump_tiles(pgv_env* env, int32_t index, uint8_t* h_out, int32_t cap);

PGV_API const char* pgv_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* PROCGEN2_VEC_H */
