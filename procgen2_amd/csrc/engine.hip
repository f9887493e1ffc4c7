// Vector env engine + the two C ABIs (include/procgen2_vec.h, include/procgen2_cenv.h).
#include <dirent.h>
#include <dlfcn.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <array>
#include <atomic>
#include <cstring>
#include <mutex>

#include "../../include/procgen2_cenv.h"
#include "../../include/procgen2_vec.h"
#include "pg_engine.h"
#include "pg_episodes.h"
#include "pg_order.h"
#include "pg_history.h"
#include "pg_history_aug.h"
#include "pg_transitions.h"
#include "pg_policy_obs.h"
#include "pg_records.h"
#include "pg_sequence.h"
#include "png_decode.h"

#ifndef PG_DEFAULT_GAME
#define PG_DEFAULT_GAME 0
#endif

namespace pg {

static thread_local std::string g_error;

static int fail(const std::string& msg) {
    g_error = msg;
    return 1;
}

#define PG_HIP(call)                                                                             \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) return fail(std::string(#call) + ": " + hipGetErrorString(e_));    \
    } while (0)

// ------------------------------------------------------------------------------------------------
// Atlas
// ------------------------------------------------------------------------------------------------
Atlas::~Atlas() {
    if (d_texels_) hipFree(d_texels_);
    if (d_desc_) hipFree(d_desc_);
    if (d_ranks_) hipFree(d_ranks_);
}

bool Atlas::load(const std::string& root, const std::vector<std::string>& names, std::string& err) {
    texels_.clear();
    desc_.clear();
    for (const auto& name : names) {
        Image img;
        if (!decode_png_file(root + "/" + name, img, err)) return false;
        int4 d;
        d.x = static_cast<int>(texels_.size());
        d.y = img.w;
        d.z = img.h;
        // .w bit 0: some texel is not opaque (alpha < 255) — under this texture something else can show, and the row
        // composer may have to blend; bit 1: more than 3 % of them are not — a frame that shows this texture is unlikely
        // to get away with its one-texel-per-pixel attempt (pg_render.h compose_rows), so it does not try.
        d.w = 0;
        size_t not_opaque = 0;
        for (size_t k = 3; k < img.rgba.size(); k += 4) not_opaque += img.rgba[k] != 255;
        if (not_opaque) d.w |= 1;
        if (not_opaque * 100 > size_t(img.w) * img.h * 3) d.w |= 2;
        // bit 2: some texel is translucent (alpha neither 0 nor 255); bit 3: every texel outside the central half of
        // the texture (rows and columns [size/4, 3·size/4)) is fully transparent — what chaser.hip asks of its point
        // sprite before it lets the points join the tile layer.
        bool clear_rim = true;
        for (int y = 0; y < img.h; y++)
            for (int x = 0; x < img.w; x++) {
                const uint8_t a = img.rgba[(size_t(y) * img.w + x) * 4 + 3];
                if (a != 0 && a != 255) d.w |= 4;
                const bool inner = y >= img.h / 4 && y < img.h - img.h / 4 && x >= img.w / 4 && x < img.w - img.w / 4;
                if (!inner && a != 0) clear_rim = false;
            }
        if (clear_rim) d.w |= 8;
        desc_.push_back(d);
        size_t base = texels_.size();
        texels_.resize(base + size_t(img.w) * img.h);
        std::memcpy(&texels_[base], img.rgba.data(), size_t(img.w) * img.h * 4);
        // A texel with alpha 0 never reaches a pixel (raster spec S4), whatever colour the PNG left in it: store it as
        // the word 0, so that "nothing here" is one value (pg_render.h compose_rows picks the last drawn candidate
        // with an unsigned maximum).
        for (size_t k = base; k < texels_.size(); k++)
            if ((texels_[k] >> 24) == 0) texels_[k] = 0;
    }
    return true;
}

bool Atlas::upload(std::string& err) {
    if (texels_.size() * 4 >= 0x10000000ull) {  // byte offsets share their word with two rank bits (pg_render.h kRank)
        err = "atlas exceeds 256 MiB (pg_render.h kRank, kNoTexel)";
        return false;
    }
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d_texels_), texels_.size() * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_desc_), desc_.size() * sizeof(int4));
    if (e == hipSuccess) e = hipMemcpy(d_texels_, texels_.data(), texels_.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_desc_, desc_.data(), desc_.size() * sizeof(int4), hipMemcpyHostToDevice);
    std::vector<uint8_t> ranks(kRankTableBytes);
    build_equal_key_ranks(ranks.data());
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_ranks_), ranks.size());
    if (e == hipSuccess) e = hipMemcpy(d_ranks_, ranks.data(), ranks.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        err = std::string("atlas upload: ") + hipGetErrorString(e);
        return false;
    }
    return true;
}

// Several engines on one GPU want more hardware queues than the HIP runtime's default of four (streams that share a
// queue run their kernels one after the other: the mixed seven-game workload, fourteen streams, gains 9.5 % with twelve
// or more).  The runtime reads GPU_MAX_HW_QUEUES when it initialises, at the first HIP call of the process; loading this
// library is usually earlier.  A value the caller has set is left alone.
// When the runtime is up already (the embedding process made a HIP call first, or rocprofv3's preloaded tool did) the
// default comes too late and is silently without effect: that is noticed here — an initialised ROCm runtime holds
// /dev/kfd open — and said once, on stderr, by the first pgv_make that would have profited (the third engine on a
// device: a single game's two streams are served by the runtime's own four queues).
static bool g_queue_default_too_late = false;
static bool rocm_runtime_is_up() {
    DIR* d = opendir("/proc/self/fd");
    if (!d) return false;
    bool up = false;
    while (dirent* ent = readdir(d)) {
        char link[64], target[64];
        std::snprintf(link, sizeof link, "/proc/self/fd/%s", ent->d_name);
        const ssize_t n = readlink(link, target, sizeof target - 1);
        if (n > 0) {
            target[n] = 0;
            if (!std::strcmp(target, "/dev/kfd")) up = true;
        }
    }
    closedir(d);
    return up;
}
__attribute__((constructor)) static void runtime_defaults() {
    if (std::getenv("GPU_MAX_HW_QUEUES")) return;  // the caller's choice
    g_queue_default_too_late = rocm_runtime_is_up();
    setenv("GPU_MAX_HW_QUEUES", "16", /*overwrite=*/0);
}
static std::atomic<int> g_live_engines[16];
static void note_engine_made(int device) {
    if (device < 0 || device >= 16) return;
    static std::atomic<bool> said{false};
    if (++g_live_engines[device] >= 3 && g_queue_default_too_late && !said.exchange(true))
        std::fprintf(stderr,
                     "procgen2_hip: %d engines on device %d, but the HIP runtime was initialised before this library was "
                     "loaded, so its default GPU_MAX_HW_QUEUES=16 came too late and the streams of these engines share the "
                     "runtime's default hardware queues (kernels of different engines run in turn; measured: -9 %% on the "
                     "seven-game workload).  Export GPU_MAX_HW_QUEUES=16 before the process starts.\n",
                     g_live_engines[device].load(), device);
}

static std::string asset_root() {
    if (const char* env = std::getenv("PROCGEN2_ASSETS")) return env;
    Dl_info info;
    if (dladdr(reinterpret_cast<void*>(&asset_root), &info) && info.dli_fname) {
        std::string p = info.dli_fname;
        size_t slash = p.rfind('/');
        std::string dir = slash == std::string::npos ? "." : p.substr(0, slash);
        return dir + "/../assets";
    }
    return "assets";
}

static const char* const kGameNames[kNumGames] = {"coinrun", "maze", "bossfight", "climber", "caveflyer", "chaser", "jumper"};

// (game, distribution mode) → compiled variant.  The first row of a game is its PGV_MODE_DEFAULT, i.e. the reference's
// compile-time `Config` (SURVEY.md §5 "config / flags").  coinrun: `easy_mode` only feeds `allow_monsters`, which
// nothing reads (coinrun/tilemap.cpp:148), so both modes are the same game.
struct Variant {
    int game, mode;
    std::unique_ptr<Game> (*make)();
};
static const Variant kVariants[] = {
    {kGameCoinrun, PGV_MODE_HARD, make_coinrun_v0},     {kGameCoinrun, PGV_MODE_EASY, make_coinrun_v0},
    {kGameMaze, PGV_MODE_HARD, make_maze_v0},           {kGameMaze, PGV_MODE_EASY, make_maze_v1},
    {kGameMaze, PGV_MODE_MEMORY, make_maze_v2},
    {kGameBossfight, PGV_MODE_HARD, make_bossfight_v0}, {kGameBossfight, PGV_MODE_EASY, make_bossfight_v1},
    {kGameClimber, PGV_MODE_HARD, make_climber_v0},     {kGameClimber, PGV_MODE_EASY, make_climber_v1},
    {kGameCaveflyer, PGV_MODE_HARD, make_caveflyer_v0}, {kGameCaveflyer, PGV_MODE_EASY, make_caveflyer_v1},
    {kGameCaveflyer, PGV_MODE_MEMORY, make_caveflyer_v2},
    {kGameChaser, PGV_MODE_EASY, make_chaser_v0},       {kGameChaser, PGV_MODE_HARD, make_chaser_v1},
    {kGameChaser, PGV_MODE_EXTREME, make_chaser_v2},
    {kGameJumper, PGV_MODE_HARD, make_jumper_v0},       {kGameJumper, PGV_MODE_EASY, make_jumper_v1},
    {kGameJumper, PGV_MODE_MEMORY, make_jumper_v2},
};

static const Variant* find_variant(int game, int mode) {
    for (const Variant& v : kVariants)
        if (v.game == game && (mode == PGV_MODE_DEFAULT || v.mode == mode)) return &v;
    return nullptr;
}

// Device buffers for one call of a host-pointer entry point, filled from and read back to host memory on the env's stream.
// The first error is kept and what follows it skipped; on every way out the stream is drained before the buffers are freed.
struct Staged {
    hipStream_t stream;
    hipError_t err = hipSuccess;
    std::vector<void*> held;
    ~Staged() {
        (void)hipStreamSynchronize(stream);
        for (void* p : held) (void)hipFree(p);
    }
    template <class T>
    T* alloc(size_t count, const T* h_from = nullptr) {  // device T[count], with a copy of h_from[count] where given
        void* p = nullptr;
        if (err == hipSuccess) err = hipMalloc(&p, count * sizeof(T));
        if (p) held.push_back(p);
        if (h_from) upload(p, h_from, count * sizeof(T));
        return static_cast<T*>(p);
    }
    void upload(void* d_to, const void* h_from, size_t bytes) {
        if (err == hipSuccess) err = hipMemcpyAsync(d_to, h_from, bytes, hipMemcpyHostToDevice, stream);
    }
    void finish() { err = err == hipSuccess ? hipStreamSynchronize(stream) : err; }
    void fetch(void* h_to, const void* d_from, size_t bytes) {  // behind everything the stream holds
        finish();
        if (err == hipSuccess) err = hipMemcpy(h_to, d_from, bytes, hipMemcpyDeviceToHost);
    }
};

}  // namespace pg

// ------------------------------------------------------------------------------------------------
// The vector env object
// ------------------------------------------------------------------------------------------------
struct pgv_env {
    int n = 0, device = 0, env_offset = 0, mode = 0;
    uint32_t game_flags = 0;
    uint32_t step_index = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::unique_ptr<pg::Game> game;
    pg::Atlas atlas;
    void* d_state = nullptr;
    bool counted = false;       // among g_live_engines (note_engine_made)
    void* d_scratch = nullptr;  // Game::scratch_bytes: per-frame hand-over between a game's kernels, not part of any snapshot
    uint8_t* d_obs = nullptr;
    float* d_reward = nullptr;
    uint8_t* d_done = nullptr;
    uint8_t* d_pending = nullptr;
    int32_t* d_host_i32 = nullptr;  // staging for the *_host entry points
    uint8_t* d_host_u8 = nullptr;
    bool own_obs = false, own_reward = false, own_done = false;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // level prefetch (pg_prefetch.h): generator launches on a side stream, ordered behind the main stream by events
    hipStream_t side = nullptr;
    hipEvent_t side_ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int side_ev_next = 0, since_pregen = 0;
    int64_t generator_launches = 0;  // pgv_generator_launches
    // auto-resets beside the logic kernels (pg_engine.h Game::reset_stream)
    hipStream_t reset_stream = nullptr;
    hipEvent_t reset_fork = nullptr, reset_join = nullptr;
    // per-env records (pg_records.h): the region table as far as pgv_make knows it — the output rows' addresses are filled
    // in per call, pgv_bind_outputs may move them — the configuration's fingerprint, and the event that orders the env's
    // stream behind the generator's before records are read or written
    pg::RecordTable rec{};
    int rec_reward = 0, rec_done = 0, rec_obs = 0;
    uint64_t rec_tag = 0;
    hipEvent_t rec_ev = nullptr;
    // episode bookkeeping (pg_episodes.h; pgv_episodes_enable): off unless asked for.  One device block holds every buffer;
    // the engine's own rows and level words are filled in per call (pgv_bind_outputs may move the rows).
    bool episodes = false;
    int ep_autoreset = 0;
    void* d_episodes = nullptr;
    pg::EpisodeBuffers ep{};
    // steps without frames (pg_sequence.h; pgv_step_sequence): the running values of the summary, one block
    void* d_sequence = nullptr;
    pg::SequenceBuffers seq{};
    // caller-made levels (pg_levels.h; pgv_set_levels): an install's claim words and mask, one block, for a game that has them
    void* d_levels = nullptr;
    pg::LevelBuffers lev{};
    // the debug taps (pgv_dump_state / pgv_dump_tiles): room for one env's state row and tile row, one block
    void* d_tap = nullptr;
    pg::TapBuffers tap{};
    // policy-ready observations (pg_policy_obs.h; pgv_policy_obs_enable): off unless asked for.  One device block holds the
    // restart flags and the value table; the tensor is the caller's, or the engine's own.
    bool policy = false, own_policy_out = false;
    int policy_stack = 0, policy_planes = 0, policy_es = 0;
    void* d_policy = nullptr;
    uint8_t* d_policy_out = nullptr;
    pg::PolicyObsBuffers pol{};
    // frame history (pg_history.h; pgv_history_enable): off unless asked for.  One device block holds the pending flags, the
    // began bytes, the value tables and — unless the caller brought them — the frames.  `history_head` counts the pushes.
    bool history = false;
    int64_t history_head = 0;
    void* d_history = nullptr;
    pg::HistoryBuffers hist{};
    // transitions (pg_transitions.h; pgv_transitions_enable): off unless asked for, on top of the frame history.  One device
    // block holds the pending bytes and the three [T][N] arrays; a row's slot follows `history_head`.
    bool transitions = false;
    void* d_transitions = nullptr;
    pg::TransitionBuffers tr{};
    // both features' value tables, dtype by dtype (pg_planes.h): the uploads' source, so they live as long as the env
    uint32_t value_tables[pg::kPolicyTables][256];  // (filled where the env is made)

    pg::StepIO io() const { return {d_obs, d_reward, d_done, d_pending}; }
    // The per-env output rows, in the order a snapshot holds them behind the state blob.  Separate allocations:
    // pgv_bind_outputs replaces them one at a time.
    struct Row { void** d; size_t bytes_per_env; };
    std::array<Row, 4> rows() {
        return {{{reinterpret_cast<void**>(&d_reward), 4}, {reinterpret_cast<void**>(&d_done), 1},
                 {reinterpret_cast<void**>(&d_pending), 1}, {reinterpret_cast<void**>(&d_obs), size_t(pg::kObsBytes)}}};
    }
};

// Queue one generator launch behind everything the main stream holds so far.  In the step loop: every
// pregen_every()-th step (pg_engine.h: the game says how long a queued slot may wait) — one launch serves every slot
// queued by then, and a launch costs its single-env latency (ms) even for one env, so launching per step would only pile
// launches up.  The cadence is a count of steps and nothing else: until round 5 a launch was also made whenever the
// HOST saw the side stream idle (hipStreamQuery), which a benchmark loop that runs hundreds of steps ahead of the device
// never does and a caller that synchronises every step always does — two callers, two cadences, and the second one
// the slower for coinrun, climber and jumper (tests/test_levels.py::test_generator_cadence_…).
static void pregen(pgv_env* e, bool bulk, bool force) {
    if (!e->side) return;
    e->since_pregen++;
    if (!force && e->since_pregen < e->game->pregen_every()) return;
    hipEvent_t ev = e->side_ev[e->side_ev_next];
    e->side_ev_next = (e->side_ev_next + 1) % 8;
    if (hipEventRecord(ev, e->stream) != hipSuccess || hipStreamWaitEvent(e->side, ev, 0) != hipSuccess) return;
    if (!e->game->launch_pregen(e->side, bulk)) {
        hipStreamDestroy(e->side);  // this game generates its levels inside the step
        e->side = nullptr;
        return;
    }
    e->generator_launches++;
    e->since_pregen = 0;
}

using pg::fail;

extern "C" {

const char* pgv_last_error(void) { return pg::g_error.c_str(); }

const char* pgv_game_name(int32_t id) { return (id >= 0 && id < pg::kNumGames) ? pg::kGameNames[id] : nullptr; }

int32_t pgv_game_id(const char* name) {
    for (int i = 0; i < pg::kNumGames; i++)
        if (name && !std::strcmp(name, pg::kGameNames[i])) return i;
    return -1;
}

int32_t pgv_synthetic_action(uint32_t run_seed, uint32_t step_index, uint32_t global_env) {
    return pg::synthetic_action(run_seed, step_index, global_env);
}

void pgv_close(pgv_env* e) {
    if (!e) return;
    if (e->counted && e->device >= 0 && e->device < 16) --pg::g_live_engines[e->device];
    hipSetDevice(e->device);
    if (e->stream) hipStreamSynchronize(e->stream);
    if (e->side) {
        hipStreamSynchronize(e->side);
        hipStreamDestroy(e->side);
    }
    for (auto& ev : e->side_ev)
        if (ev) hipEventDestroy(ev);
    for (auto& ev : e->ev)
        if (ev) hipEventDestroy(ev);
    if (e->reset_stream) {
        hipStreamSynchronize(e->reset_stream);
        hipStreamDestroy(e->reset_stream);
    }
    if (e->reset_fork) hipEventDestroy(e->reset_fork);
    if (e->reset_join) hipEventDestroy(e->reset_join);
    if (e->rec_ev) hipEventDestroy(e->rec_ev);
    if (e->d_state) hipFree(e->d_state);
    if (e->d_scratch) hipFree(e->d_scratch);
    if (e->own_obs && e->d_obs) hipFree(e->d_obs);
    if (e->own_reward && e->d_reward) hipFree(e->d_reward);
    if (e->own_done && e->d_done) hipFree(e->d_done);
    if (e->d_pending) hipFree(e->d_pending);
    if (e->d_episodes) hipFree(e->d_episodes);
    if (e->d_sequence) hipFree(e->d_sequence);
    if (e->d_levels) hipFree(e->d_levels);
    if (e->d_tap) hipFree(e->d_tap);
    if (e->d_policy) hipFree(e->d_policy);
    if (e->own_policy_out && e->d_policy_out) hipFree(e->d_policy_out);
    if (e->d_history) hipFree(e->d_history);
    if (e->d_transitions) hipFree(e->d_transitions);
    if (e->d_host_i32) hipFree(e->d_host_i32);
    if (e->d_host_u8) hipFree(e->d_host_u8);
    if (e->own_stream && e->stream) hipStreamDestroy(e->stream);
    delete e;
}

// The device state blob: the game's SoA state followed by the level plan's per-env arrays (pg_carve.h list_plan), so that
// a snapshot of the blob carries them.
static size_t game_state_bytes(const pgv_env* e) { return (e->game->state_bytes(e->n) + 255) / 256 * 256; }
static size_t state_blob_bytes(const pgv_env* e) { return game_state_bytes(e) + pg::Carve::size(pg::list_plan, e->n); }

// The record layout of this engine (pg_records.h): the game's per-env regions as its state listing describes them, then the
// level plan's as list_plan describes them (`planned`), then the engine's output rows.  The game's listing is checked
// here, on the host: every byte of the state block is either an env's or declared engine-wide — a region added later
// without saying which fails pgv_make instead of dropping out of records.
static int32_t plan_records(pgv_env* e, const pg::EnvRegions& planned) {
    const pg::EnvRegions& listed = e->game->regions;
    const std::string who = std::string("pgv_make: ") + e->game->name() + "'s state listing ";
    if (listed.unlisted_bytes)
        return fail(who + "takes " + std::to_string(listed.unlisted_bytes) + " bytes with a plain take(): say take_env or take_shared (pg_engine.h Carve)");
    size_t sum = listed.shared_bytes;
    for (const pg::EnvRegion& r : listed.v) sum += (size_t(e->n) * r.pieces * r.piece_bytes + 255) / 256 * 256;
    if (sum != e->game->state_bytes(e->n))
        return fail(who + "describes " + std::to_string(sum) + " bytes of a block of " + std::to_string(e->game->state_bytes(e->n)));
    std::vector<pg::EnvRegion> all = listed.v;
    all.insert(all.end(), planned.v.begin(), planned.v.end());
    for (auto [index, bytes] : {std::pair<int*, uint32_t>{&e->rec_reward, 4}, {&e->rec_done, 1}, {&e->rec_obs, pg::kObsBytes}}) {
        *index = static_cast<int>(all.size());  // (the rows' bases: records_table, per call)
        all.push_back({nullptr, 1, bytes});
    }
    if (all.size() > size_t(pg::kMaxRecordRegions)) return fail(who + "has more per-env regions than a record table holds");
    pg::RecordTable& t = e->rec;
    t = pg::RecordTable{};
    uint32_t at = pg::kRecordHeaderBytes;
    for (const pg::EnvRegion& r : all) {
        t.r[t.regions++] = pg::RecordRegion{r.base, r.pieces, r.piece_bytes, at};
        at += (r.pieces * r.piece_bytes + 15u) / 16u * 16u;
    }
    t.n = e->n;
    t.record_bytes = at;
    t.selectors = e->game->stream_selectors();
    // the fingerprint: FNV-1a over the configuration and the layout (every region's shape: they differ between variants)
    uint64_t h = 0xcbf29ce484222325ull;
    auto mix = [&](uint32_t w) {
        for (int k = 0; k < 4; k++) h = (h ^ ((w >> (8 * k)) & 0xffu)) * 0x100000001b3ull;
    };
    mix(pg::kRecordLayoutVersion);
    mix(static_cast<uint32_t>(pgv_game_id(e->game->name())));
    mix(static_cast<uint32_t>(e->mode));
    mix(e->game_flags);
    mix(static_cast<uint32_t>(e->game->plan.num_levels));
    mix(static_cast<uint32_t>(e->game->plan.start_level));
    for (int k = 0; k < t.regions; k++) mix(t.r[k].pieces), mix(t.r[k].piece_bytes);
    mix(t.record_bytes);
    e->rec_tag = h ? h : 1;
    return 0;
}

int32_t pgv_make(const char* game, int32_t num_envs, int32_t device, uint32_t seed_base, int32_t env_offset,
                 void* stream, pgv_env** out) {
    return pgv_make_levels(game, num_envs, device, seed_base, env_offset, stream, 0, 0, out);
}

int32_t pgv_make_levels(const char* game, int32_t num_envs, int32_t device, uint32_t seed_base, int32_t env_offset,
                        void* stream, int32_t num_levels, int32_t start_level, pgv_env** out) {
    pgv_config cfg{};
    cfg.struct_size = sizeof(pgv_config);
    cfg.game = game;
    cfg.num_envs = num_envs;
    cfg.device = device;
    cfg.seed_base = seed_base;
    cfg.env_offset = env_offset;
    cfg.stream = stream;
    cfg.num_levels = num_levels;
    cfg.start_level = start_level;
    cfg.mode = PGV_MODE_DEFAULT;
    return pgv_make_config(&cfg, out);
}

uint32_t pgv_game_modes(int32_t game_id) {
    uint32_t bits = 0;
    for (const pg::Variant& v : pg::kVariants)
        if (v.game == game_id) bits |= 1u << v.mode;
    return bits;
}

int32_t pgv_mode(pgv_env* e) { return e ? e->mode : -1; }

int32_t pgv_make_config(const pgv_config* cfg, pgv_env** out) {
    if (!out) return fail("pgv_make: out is NULL");
    *out = nullptr;
    if (!cfg || cfg->struct_size < sizeof(pgv_config)) return fail("pgv_make_config: config is NULL or struct_size too small");
    const char* game = cfg->game;
    const int32_t num_envs = cfg->num_envs, device = cfg->device, env_offset = cfg->env_offset;
    const uint32_t seed_base = cfg->seed_base;
    void* stream = cfg->stream;
    const int32_t num_levels = cfg->num_levels, start_level = cfg->start_level;
    if (num_levels < 0) return fail("pgv_make: num_levels must be >= 0 (0 = every level is new)");
    const int gid = pgv_game_id(game);
    if (gid < 0) return fail(std::string("pgv_make: unknown game '") + (game ? game : "(null)") + "'");
    const pg::Variant* variant = pg::find_variant(gid, cfg->mode);
    if (!variant)
        return fail(std::string("pgv_make: game '") + game + "' has no distribution mode " + std::to_string(cfg->mode) +
                    " (see pgv_game_modes)");
    if (num_envs <= 0) return fail("pgv_make: num_envs must be positive");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail("pgv_make: no HIP device available (the engine has no CPU path)");
    if (device < 0 || device >= count) return fail("pgv_make: device index out of range");
    PG_HIP(hipSetDevice(device));

    // every failure path below releases what was created so far (streams, events, atlas, device memory)
    std::unique_ptr<pgv_env, void (*)(pgv_env*)> e(new pgv_env(), pgv_close);
    e->n = num_envs;
    e->device = device;
    e->env_offset = env_offset;
    e->game = variant->make();
    e->mode = variant->mode;
    e->game_flags = cfg->game_flags;
    for (int dtype = 0; dtype < pg::kPolicyTables; dtype++)
        for (uint32_t v = 0; v < 256; v++) e->value_tables[dtype][v] = pg::policy_table_entry(dtype, v);
    if (!e->game->set_game_flags(cfg->game_flags))
        return fail(std::string("pgv_make: game '") + game + "' does not take game_flags " + std::to_string(cfg->game_flags));
    if (stream) {
        e->stream = static_cast<hipStream_t>(stream);
    } else {
        PG_HIP(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
        e->own_stream = true;
    }
    for (auto& ev : e->ev) PG_HIP(hipEventCreate(&ev));
    PG_HIP(hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking));  // the level generator's stream
    for (auto& ev : e->side_ev) PG_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    PG_HIP(hipEventCreateWithFlags(&e->rec_ev, hipEventDisableTiming));
    if (e->game->resets_beside_logic()) {
        {   // the few long wavefronts of the in-step level kernel go first; the logic kernel's many short ones fill in around them
            int least = 0, greatest = 0;
            PG_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
            PG_HIP(hipStreamCreateWithPriority(&e->reset_stream, hipStreamNonBlocking, greatest));
        }
        PG_HIP(hipEventCreateWithFlags(&e->reset_fork, hipEventDisableTiming));
        PG_HIP(hipEventCreateWithFlags(&e->reset_join, hipEventDisableTiming));
        e->game->reset_stream = e->reset_stream;
    }

    std::string err;
    if (!e->atlas.load(pg::asset_root(), e->game->texture_names(), err)) return fail("pgv_make: " + err);
    err = e->game->check_atlas(e->atlas.sizes());
    if (!err.empty()) return fail("pgv_make: " + err);
    e->game->extend_atlas(e->atlas);
    if (!e->atlas.upload(err)) return fail("pgv_make: " + err);
    const size_t sb = state_blob_bytes(e.get());
    PG_HIP(hipMalloc(&e->d_state, sb));
    PG_HIP(hipMemsetAsync(e->d_state, 0, sb, e->stream));
    e->own_obs = e->own_reward = e->own_done = true;
    for (const pgv_env::Row& row : e->rows()) {
        PG_HIP(hipMalloc(row.d, size_t(num_envs) * row.bytes_per_env));
        PG_HIP(hipMemsetAsync(*row.d, 0, size_t(num_envs) * row.bytes_per_env, e->stream));
    }

    PG_HIP(hipMalloc(&e->d_sequence, pg::Carve::size(pg::list_sequence, num_envs)));  // (written before it is read: pg_sequence.h)
    pg::Carve::bind(pg::list_sequence, e->d_sequence, e->seq, num_envs);
    if (e->game->level_layout().supported) {  // (zeroed in front of every install)
        PG_HIP(hipMalloc(&e->d_levels, pg::Carve::size(pg::list_levels, num_envs)));
        pg::Carve::bind(pg::list_levels, e->d_levels, e->lev, num_envs);
    }

    e->game->bind(e->d_state, num_envs, e->atlas.view());
    if (const size_t scratch = e->game->scratch_bytes(num_envs)) {
        PG_HIP(hipMalloc(&e->d_scratch, scratch));
        PG_HIP(hipMemsetAsync(e->d_scratch, 0, scratch, e->stream));
        e->game->bind_scratch(e->d_scratch, num_envs);
    }
    pg::EnvRegions planned;
    e->game->plan = pg::LevelPlan{num_levels, start_level};
    pg::Carve::bind(pg::list_plan, static_cast<uint8_t*>(e->d_state) + game_state_bytes(e.get()), e->game->plan, num_envs, &planned);
    if (plan_records(e.get(), planned)) return 1;
    // (the last allocation of the call: a debug buffer does not move the addresses of what the step works on)
    e->tap.width = e->game->state_layout().width, e->tap.cells = e->game->state_layout().cells;
    PG_HIP(hipMalloc(&e->d_tap, pg::Carve::size(pg::list_tap, 1, e->tap)));  // (written before it is read, by every tap)
    pg::Carve::bind(pg::list_tap, e->d_tap, e->tap, 1);
    e->game->launch_make(e->stream, seed_base, env_offset);
    PG_HIP(hipGetLastError());
    PG_HIP(hipStreamSynchronize(e->stream));
    pregen(e.get(), true, true);
    pg::note_engine_made(device);
    e->counted = true;
    *out = e.release();
    return 0;
}

// What a call that ends with a push of the policy observations or of the frame history asks of the host, BEFORE it enqueues
// anything: a slab the push kernels' 16-byte loads can read (pgv_bind_outputs may have moved it).  A refusal leaves the
// engine as it was — no step taken, no flag set, the step counter and the ring's head where they stood.  An engine with
// neither feature passes.
static int32_t slab_ready(const char* who, const pgv_env* e) {
    if ((e->policy || e->history) && (reinterpret_cast<uintptr_t>(e->d_obs) & 15u))
        return fail(std::string(who) + ": the observation buffer must be 16-byte aligned for the " +
                    (e->policy ? "policy observations" : "frame history"));
    return 0;
}

// The flag array of every enabled feature — the policy observations' restart flags, then the frame history's pending flags;
// nullptr for one that is off: the stacks and the ring begin afresh at the same events, told by the same flag kernels.
// `found_done`: the event is a step that finds the `done` row set — the one event the transitions' pending bytes (VOID) are
// filed at, by the same kernel; at every other event their place is nullptr.
static std::array<uint8_t*, 3> flag_arrays(const pgv_env* e, bool found_done = false) {
    return {{e->policy ? e->pol.restart : nullptr, e->history ? e->hist.pending : nullptr,
             found_done && e->transitions ? e->tr.pending : nullptr}};
}

// A push of the policy observations (pg_policy_obs.h) on the env's stream, for the calls that end with one: the obs slab as
// it stands there.  Its callers have asked slab_ready() first.
static int32_t policy_push(const char* who, pgv_env* e, const uint8_t* d_mask) {
    pg::PolicyPush q{};
    q.n = e->n;
    q.stack = e->policy_stack;
    q.planes = e->policy_planes;
    q.dense = (e->game->debug_flags & pg::kDebugPolicyStrided) ? 0 : 1;
    q.obs = e->d_obs;
    q.out = e->d_policy_out;
    q.mask = d_mask;
    q.b = e->pol;
    pg::launch_policy_push(e->stream, q, e->policy_es);
    PG_HIP(hipGetLastError());
    return 0;
}

// A push of the frame history (pg_history.h) on the env's stream: the obs slab as it stands there into a new slot, all envs
// — or, for pgv_reset (`reset`), into the newest slot under the mask (slot 0, opened, where there is none yet).  Its callers
// have asked slab_ready() first.
static int32_t history_push(pgv_env* e, bool reset, const uint8_t* d_mask) {
    const bool open = !reset || e->history_head == 0;
    pg::HistoryPush q{};
    q.n = e->n;
    q.planes = e->hist.planes;
    q.slot = pg::history_slot(open ? e->history_head : e->history_head - 1, e->hist.capacity);
    q.reset = reset ? 1 : 0;
    q.obs = e->d_obs;
    q.mask = d_mask;
    q.b = e->hist;
    pg::launch_history_push(e->stream, q);
    PG_HIP(hipGetLastError());
    if (open) e->history_head++;
    return 0;
}

// What a call that opens a slot of the frame history says of itself for the transitions' row (pg_transitions.h): nothing
// (`recorded` 0: the push by hand, a drawn sequence), or the single step it took — its actions (nullptr: synthetic, by
// run_seed) and, for an episode step, that the episode outputs hold its reward and how it ended.
struct RowOf {
    int recorded = 0, episodes = 0;
    const int32_t* actions = nullptr;
    uint32_t run_seed = 0;
};
// The row head - 1, in front of the history push that makes push `head` (at head = 0 there is none: the pending bytes are
// cleared all the same).  A step's index is the one step_impl just used.
static int32_t transition_record(pgv_env* e, const RowOf& row) {
    pg::TransitionRecord q{};
    q.n = e->n;
    q.slot = e->history_head > 0 ? pg::history_slot(e->history_head - 1, e->hist.capacity) : -1;
    q.recorded = row.recorded;
    q.run_seed = row.run_seed, q.step_index = e->step_index - 1u, q.env_offset = static_cast<uint32_t>(e->env_offset);
    q.actions = row.actions;
    q.reward = row.episodes ? e->ep.reward : e->d_reward;
    q.terminated = row.episodes ? e->ep.terminated : e->d_done;
    q.truncated = row.episodes ? e->ep.truncated : nullptr;
    q.b = e->tr;
    pg::launch_transition_record(e->stream, q);
    PG_HIP(hipGetLastError());
    return 0;
}

// The pushes that end a call of point 4: the policy observations, then — behind the transitions' row of the call — the
// frame history, whichever is enabled.
static int32_t end_with_pushes(const char* who, pgv_env* e, const RowOf& row = RowOf{}) {
    if (e->policy && policy_push(who, e, nullptr)) return 1;
    if (e->transitions && transition_record(e, row)) return 1;
    return e->history ? history_push(e, false, nullptr) : 0;
}

// What a reset does for the envs of `d_mask` once their new levels are the live state: the first frame, the episodes'
// running values, the stacks and the frame history.  `generated`: the levels came from the generator (pgv_reset), whose next
// launch is then due; a caller's levels (pgv_set_levels) took nothing from it.
static int32_t reset_shows(const char* who, pgv_env* e, const uint8_t* d_mask, bool generated) {
    e->game->launch_prepass(e->stream, d_mask);
    e->game->launch_render(e->stream, d_mask, e->io());
    if (e->episodes) pg::launch_episode_clear(e->stream, e->ep, d_mask);  // the named envs start their episodes afresh
    if (generated) pregen(e, true, true);
    PG_HIP(hipGetLastError());
    if (e->policy) {  // the named envs' stacks restart with the frame just drawn
        pg::launch_policy_flag_mask(e->stream, e->pol.restart, e->n, d_mask);
        if (policy_push(who, e, d_mask)) return 1;
    }
    if (e->history) return history_push(e, true, d_mask);  // … and their rows of the newest slot are that frame, began = 1
    return 0;
}

int32_t pgv_reset(pgv_env* e, const uint8_t* d_mask, const int32_t* d_seeds) {
    if (!e) return fail("pgv_reset: env is NULL");
    if (slab_ready("pgv_reset", e)) return 1;
    PG_HIP(hipSetDevice(e->device));
    e->game->launch_reset(e->stream, d_mask, d_seeds, e->io());
    return reset_shows("pgv_reset", e, d_mask, true);
}

// One step's launches.  The launch status is read after each group of launches: hipGetLastError reports (and clears)
// only the most recent error.
// `after_logic` / `before_render` / `after_render`: optional events (measurement only) — behind the logic kernels (and the
// level generator's launch on the side stream), behind the render pre-pass = in front of the render kernel, behind the
// render launch (jumper: its list kernel included).  What follows after_render inside a step is the late pass of a game
// that resets beside its render kernel (chaser).
// `frame` = false: a step without a frame (pgv_step_sequence) — neither the pre-pass nor the render launch; the game's
// launch_no_frame in their place, and the late pass all the same (chaser: the pending bytes, the due list and the reset
// envs' base layers depend on it).
static int32_t step_impl(pgv_env* e, const int32_t* d_actions, uint32_t run_seed, hipEvent_t before_render = nullptr,
                         hipEvent_t after_render = nullptr, hipEvent_t after_logic = nullptr, bool frame = true) {
    // hipGetLastError is sticky and per thread: whatever the embedding application left behind (a stream query's
    // NotReady, say) is not this step's; start clean.
    (void)hipGetLastError();
    // (policy observations, frame history: the done row as this step finds it — in front of the fork, so no reset kernel is at the row yet)
    for (uint8_t* flags : flag_arrays(e, /*found_done=*/true))
        if (flags) pg::launch_policy_flag_done(e->stream, flags, e->n, e->d_done);
    const bool forked = e->reset_stream != nullptr;
    if (forked) {  // fork: the auto-resets of this step go beside its logic and render kernels
        PG_HIP(hipEventRecord(e->reset_fork, e->stream));
        PG_HIP(hipStreamWaitEvent(e->reset_stream, e->reset_fork, 0));
    }
    hipError_t status = hipSuccess;
    auto launched = [&]() {  // the status of the launches since the last call
        const hipError_t now = hipGetLastError();
        if (status == hipSuccess && now != hipSuccess) status = now;
    };
    // The step counter moves as soon as the logic launch has been issued, whatever becomes of the rest: the logic kernels
    // write "reset due in step index + 1" into the pending bytes (pg_prefetch.h reset_due_mark), and a counter that stayed
    // behind after a failed later launch would have the next call read those marks as another step's.
    const uint32_t step_index = e->step_index++;
    e->game->launch_logic(e->stream, d_actions, run_seed, step_index, e->env_offset, e->io());
    launched();
    pregen(e, false, false);  // before the render launch: the generator overlaps it
    launched();
    if (after_logic && status == hipSuccess) status = hipEventRecord(after_logic, e->stream);
    if (frame && status == hipSuccess) {
        e->game->launch_prepass(e->stream, nullptr);
        launched();
    }
    if (before_render && status == hipSuccess) status = hipEventRecord(before_render, e->stream);
    if (status == hipSuccess) {
        if (frame)
            e->game->launch_render_step(e->stream, e->io());
        else
            e->game->launch_no_frame(e->stream, e->io());
        launched();
    }
    if (after_render && status == hipSuccess) status = hipEventRecord(after_render, e->stream);
    if (forked) {  // join — on every way out, so the two streams stay consistent — and the late frames of the reset envs
        hipError_t j = hipEventRecord(e->reset_join, e->reset_stream);
        if (j == hipSuccess) j = hipStreamWaitEvent(e->stream, e->reset_join, 0);
        if (status == hipSuccess) status = j;
        if (status == hipSuccess) {
            e->game->launch_render_late(e->stream, e->io());
            launched();
        }
    }
    if (status != hipSuccess) return fail(std::string("step: ") + hipGetErrorString(status));
    return 0;
}

// A step without a frame, by name: the flag sits behind three event pointers.
static int32_t step_no_frame(pgv_env* e, const int32_t* d_actions, uint32_t run_seed) {
    return step_impl(e, d_actions, run_seed, nullptr, nullptr, nullptr, /*frame=*/false);
}

int32_t pgv_step(pgv_env* e, const int32_t* d_actions) {
    if (!e) return fail("pgv_step: env is NULL");
    if (!d_actions) return fail("pgv_step: actions is NULL");
    if (slab_ready("pgv_step", e)) return 1;
    PG_HIP(hipSetDevice(e->device));
    if (step_impl(e, d_actions, 0)) return 1;
    return end_with_pushes("pgv_step", e, RowOf{1, 0, d_actions, 0});
}

int32_t pgv_step_synthetic(pgv_env* e, uint32_t run_seed) {
    if (!e) return fail("pgv_step_synthetic: env is NULL");
    if (slab_ready("pgv_step_synthetic", e)) return 1;
    PG_HIP(hipSetDevice(e->device));
    if (step_impl(e, nullptr, run_seed)) return 1;
    return end_with_pushes("pgv_step_synthetic", e, RowOf{1, 0, nullptr, run_seed});
}

int32_t pgv_step_synthetic_many(pgv_env* const* envs, int32_t count, int32_t steps, uint32_t run_seed) {
    if (!envs || count < 1 || steps < 1) return fail("pgv_step_synthetic_many: bad arguments");
    for (int32_t k = 0; k < count; k++)
        if (!envs[k]) return fail("pgv_step_synthetic_many: env is NULL");
    for (int32_t s = 0; s < steps; s++)
        for (int32_t k = 0; k < count; k++) {
            PG_HIP(hipSetDevice(envs[k]->device));
            if (step_impl(envs[k], nullptr, run_seed))  // (the envs before k have taken step s, those from k on have not)
                return fail(pg::g_error + " (pgv_step_synthetic_many: env " + std::to_string(k) + " of " + std::to_string(count) +
                            ", step " + std::to_string(s) + " of " + std::to_string(steps) + ")");
        }
    return 0;
}

static int32_t ensure_staging(pgv_env* e) {
    if (!e->d_host_i32) PG_HIP(hipMalloc(reinterpret_cast<void**>(&e->d_host_i32), size_t(e->n) * 4));
    if (!e->d_host_u8) PG_HIP(hipMalloc(reinterpret_cast<void**>(&e->d_host_u8), size_t(e->n)));
    return 0;
}

int32_t pgv_step_host(pgv_env* e, const int32_t* h_actions) {
    if (!e) return fail("pgv_step_host: env is NULL");
    if (!h_actions) return fail("pgv_step_host: actions is NULL");
    if (slab_ready("pgv_step_host", e)) return 1;
    PG_HIP(hipSetDevice(e->device));
    if (ensure_staging(e)) return 1;
    PG_HIP(hipMemcpyAsync(e->d_host_i32, h_actions, size_t(e->n) * 4, hipMemcpyHostToDevice, e->stream));
    PG_HIP(hipStreamSynchronize(e->stream));  // the host buffer is the caller's: do not keep reading it
    return pgv_step(e, e->d_host_i32);
}

int32_t pgv_reset_host(pgv_env* e, const uint8_t* h_mask, const int32_t* h_seeds) {
    if (!e) return fail("pgv_reset_host: env is NULL");
    if (slab_ready("pgv_reset_host", e)) return 1;
    PG_HIP(hipSetDevice(e->device));
    if (ensure_staging(e)) return 1;
    if (h_mask) PG_HIP(hipMemcpyAsync(e->d_host_u8, h_mask, size_t(e->n), hipMemcpyHostToDevice, e->stream));
    if (h_seeds) PG_HIP(hipMemcpyAsync(e->d_host_i32, h_seeds, size_t(e->n) * 4, hipMemcpyHostToDevice, e->stream));
    PG_HIP(hipStreamSynchronize(e->stream));
    int rc = pgv_reset(e, h_mask ? e->d_host_u8 : nullptr, h_seeds ? e->d_host_i32 : nullptr);
    if (rc) return rc;
    PG_HIP(hipStreamSynchronize(e->stream));  // staging buffers are reused by the next *_host call
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Episodes on the device (pg_episodes.h): same-step autoreset, time limits, episode results
// ------------------------------------------------------------------------------------------------
int32_t pgv_episodes_enable(pgv_env* e, const pgv_episode_config* cfg) {
    if (!e) return fail("pgv_episodes_enable: env is NULL");
    if (!cfg || cfg->struct_size < sizeof(pgv_episode_config)) return fail("pgv_episodes_enable: config is NULL or struct_size too small");
    if (e->episodes) return fail("pgv_episodes_enable: episodes are enabled already (once per env)");
    if (cfg->autoreset != PGV_AUTORESET_NEXT_STEP && cfg->autoreset != PGV_AUTORESET_SAME_STEP)
        return fail("pgv_episodes_enable: unknown autoreset mode " + std::to_string(cfg->autoreset));
    if (cfg->max_episode_steps < 0) return fail("pgv_episodes_enable: max_episode_steps must be >= 0 (0 = no limit)");
    if (cfg->max_episode_steps > 0 && cfg->autoreset != PGV_AUTORESET_SAME_STEP)
        return fail("pgv_episodes_enable: a step limit needs PGV_AUTORESET_SAME_STEP (a truncated env must be reset by the engine)");
    if (cfg->final_capacity < 0 || cfg->final_capacity > e->n)
        return fail("pgv_episodes_enable: final_capacity must be in 0 .. num_envs");
    PG_HIP(hipSetDevice(e->device));
    pg::EpisodeBuffers b{};
    b.n = e->n;
    b.max_steps = cfg->max_episode_steps;
    b.capacity = cfg->final_capacity;
    b.level_number = e->game->plan.number;
    b.level_known = e->game->plan.known;
    const size_t bytes = pg::Carve::size(pg::list_episodes, e->n, b);
    void* mem = nullptr;
    PG_HIP(hipMalloc(&mem, bytes));
    hipError_t err = hipMemsetAsync(mem, 0, bytes, e->stream);
    if (err != hipSuccess) {
        (void)hipFree(mem);
        return fail(std::string("pgv_episodes_enable: ") + hipGetErrorString(err));
    }
    pg::Carve::bind(pg::list_episodes, mem, b, e->n);
    e->d_episodes = mem;
    e->ep = b;
    e->ep_autoreset = cfg->autoreset;
    e->episodes = true;
    return 0;
}

int32_t pgv_episode_outputs_get(pgv_env* e, pgv_episode_outputs* out) {
    if (!e) return fail("pgv_episode_outputs_get: env is NULL");
    if (!out || out->struct_size < sizeof(pgv_episode_outputs)) return fail("pgv_episode_outputs_get: outputs is NULL or struct_size too small");
    if (!e->episodes) return fail("pgv_episode_outputs_get: call pgv_episodes_enable first");
    const pg::EpisodeBuffers& b = e->ep;
    out->reward = b.reward;
    out->terminated = b.terminated;
    out->truncated = b.truncated;
    out->ended = b.ended;
    out->counts = b.counts;
    out->ended_env = b.ended_env;
    out->ended_return = b.ended_return;
    out->ended_length = b.ended_length;
    out->ended_level = b.ended_level;
    out->ended_level_known = b.ended_level_known;
    out->final_obs = b.final_obs;
    out->running_return = b.running_return;
    out->running_length = b.running_length;
    return 0;
}

// step_impl, then the episode launches and — same-step — the masked reset of the envs that ended: pgv_reset(ended, NULL)
// without its forced generator launch (the generator keeps the cadence of pregen(e, false, false) inside the step).
// `before_episodes` / `after_episodes`: optional events (measurement only) round the two launches behind the step.
static int32_t step_episodes_impl(const char* who, pgv_env* e, const int32_t* d_actions, uint32_t run_seed, hipEvent_t before_episodes = nullptr,
                                  hipEvent_t after_episodes = nullptr) {
    if (!e->episodes) return fail(std::string(who) + ": call pgv_episodes_enable first");
    if (e->ep.capacity > 0 && (reinterpret_cast<uintptr_t>(e->d_obs) & 15u))
        return fail(std::string(who) + ": the observation buffer must be 16-byte aligned for the final-observation ring");
    pg::EpisodeBuffers& b = e->ep;
    b.obs = e->d_obs;
    b.step_reward = e->d_reward;
    b.done = e->d_done;
    (void)hipGetLastError();
    pg::launch_episode_before(e->stream, b);
    PG_HIP(hipGetLastError());
    if (step_impl(e, d_actions, run_seed)) return 1;
    if (before_episodes) PG_HIP(hipEventRecord(before_episodes, e->stream));
    pg::launch_episode_after(e->stream, b);
    PG_HIP(hipGetLastError());
    if (after_episodes) PG_HIP(hipEventRecord(after_episodes, e->stream));
    if (e->ep_autoreset == PGV_AUTORESET_SAME_STEP) {
        e->game->launch_reset(e->stream, b.ended, nullptr, e->io());
        e->game->launch_prepass(e->stream, b.ended);
        e->game->launch_render(e->stream, b.ended, e->io());
        // their stacks restart, and their history begins afresh, with the new first frame
        for (uint8_t* flags : flag_arrays(e))
            if (flags) pg::launch_policy_flag_mask(e->stream, flags, e->n, b.ended);
        PG_HIP(hipGetLastError());
    }
    return 0;
}
// … and, for the entry points that are not measurements, the push behind everything.
static int32_t step_episodes_push(const char* who, pgv_env* e, const int32_t* d_actions, uint32_t run_seed) {
    if (slab_ready(who, e)) return 1;
    if (step_episodes_impl(who, e, d_actions, run_seed)) return 1;
    return end_with_pushes(who, e, RowOf{1, 1, d_actions, run_seed});
}

int32_t pgv_step_episodes(pgv_env* e, const int32_t* d_actions) {
    if (!e) return fail("pgv_step_episodes: env is NULL");
    if (!d_actions) return fail("pgv_step_episodes: actions is NULL");
    PG_HIP(hipSetDevice(e->device));
    return step_episodes_push("pgv_step_episodes", e, d_actions, 0);
}

int32_t pgv_step_episodes_synthetic(pgv_env* e, uint32_t run_seed) {
    if (!e) return fail("pgv_step_episodes_synthetic: env is NULL");
    PG_HIP(hipSetDevice(e->device));
    return step_episodes_push("pgv_step_episodes_synthetic", e, nullptr, run_seed);
}

int32_t pgv_step_episodes_host(pgv_env* e, const int32_t* h_actions) {
    if (!e) return fail("pgv_step_episodes_host: env is NULL");
    if (!h_actions) return fail("pgv_step_episodes_host: actions is NULL");
    if (!e->episodes) return fail("pgv_step_episodes_host: call pgv_episodes_enable first");
    if (slab_ready("pgv_step_episodes_host", e)) return 1;
    PG_HIP(hipSetDevice(e->device));
    if (ensure_staging(e)) return 1;
    PG_HIP(hipMemcpyAsync(e->d_host_i32, h_actions, size_t(e->n) * 4, hipMemcpyHostToDevice, e->stream));
    PG_HIP(hipStreamSynchronize(e->stream));  // the host buffer is the caller's: do not keep reading it
    return step_episodes_push("pgv_step_episodes_host", e, e->d_host_i32, 0);
}

// ------------------------------------------------------------------------------------------------
// Steps without frames (pg_sequence.h)
// ------------------------------------------------------------------------------------------------
static int32_t sequence_arguments(const char* who, pgv_env* e, const pgv_sequence* q) {
    if (!e) return fail(std::string(who) + ": env is NULL");
    if (!q || q->struct_size < sizeof(pgv_sequence)) return fail(std::string(who) + ": sequence is NULL or struct_size too small");
    if (q->steps < 0) return fail(std::string(who) + ": steps is negative");
    if (q->frames != PGV_FRAMES_LAST && q->frames != PGV_FRAMES_NONE) return fail(std::string(who) + ": unknown frames mode " + std::to_string(q->frames));
    if (q->actions && q->action_stride != 0 && q->action_stride < e->n)
        return fail(std::string(who) + ": action_stride must be 0 (the same row every sub-step) or >= num_envs");
    return 0;
}

int32_t pgv_step_sequence(pgv_env* e, const pgv_sequence* q) {
    if (sequence_arguments("pgv_step_sequence", e, q)) return 1;
    if (q->steps == 0) return 0;
    if (q->frames == PGV_FRAMES_LAST && slab_ready("pgv_step_sequence", e)) return 1;
    PG_HIP(hipSetDevice(e->device));
    pg::SequenceRow row{};
    row.n = e->n;
    row.fold = (q->seq_return || q->seq_length || q->seq_done) ? 1 : 0;
    row.acc = e->seq;
    row.seq_return = q->seq_return;
    row.seq_length = q->seq_length;
    row.seq_done = q->seq_done;
    const bool rows = q->rewards || q->dones;
    for (int32_t t = 0; t < q->steps; t++) {
        const bool last = t == q->steps - 1;
        const int32_t* actions = q->actions ? q->actions + int64_t(t) * q->action_stride : nullptr;
        const bool frame = last && q->frames == PGV_FRAMES_LAST;
        if (frame ? step_impl(e, actions, q->run_seed) : step_no_frame(e, actions, q->run_seed))
            return fail(pg::g_error + " (pgv_step_sequence: sub-step " + std::to_string(t) + " of " + std::to_string(q->steps) + "; the ones before it were taken)");
        if (!row.fold && !rows) continue;
        row.first = t == 0;
        row.last = last;
        row.reward = e->d_reward;
        row.done = e->d_done;
        row.row_reward = q->rewards ? q->rewards + size_t(t) * e->n : nullptr;
        row.row_done = q->dones ? q->dones + size_t(t) * e->n : nullptr;
        pg::launch_sequence_row(e->stream, row);
        PG_HIP(hipGetLastError());
    }
    if (q->frames == PGV_FRAMES_LAST) return end_with_pushes("pgv_step_sequence", e);  // once, behind the drawn sub-step (its row: not recorded)
    if (e->transitions) PG_HIP(hipMemsetAsync(e->tr.pending, 0, size_t(e->n), e->stream));  // no slot, no row: what the sub-steps found is nobody's
    return 0;
}

int32_t pgv_step_sequence_host(pgv_env* e, const pgv_sequence* q) {
    if (sequence_arguments("pgv_step_sequence_host", e, q)) return 1;
    if (q->steps == 0) return 0;
    if (q->frames == PGV_FRAMES_LAST && slab_ready("pgv_step_sequence_host", e)) return 1;
    PG_HIP(hipSetDevice(e->device));
    const size_t n = size_t(e->n), rows = size_t(q->steps) * n;
    pg::Staged dev{e->stream};
    pgv_sequence d = *q;
    if (q->actions) d.actions = dev.alloc(q->action_stride ? size_t(q->steps - 1) * size_t(q->action_stride) + n : n, q->actions);
    if (q->rewards) d.rewards = dev.alloc<float>(rows);
    if (q->dones) d.dones = dev.alloc<uint8_t>(rows);
    if (q->seq_return) d.seq_return = dev.alloc<float>(n);
    if (q->seq_length) d.seq_length = dev.alloc<int32_t>(n);
    if (q->seq_done) d.seq_done = dev.alloc<uint8_t>(n);
    if (dev.err == hipSuccess) {
        if (const int32_t rc = pgv_step_sequence(e, &d)) return rc;
        if (q->rewards) dev.fetch(q->rewards, d.rewards, rows * 4);
        if (q->dones) dev.fetch(q->dones, d.dones, rows);
        if (q->seq_return) dev.fetch(q->seq_return, d.seq_return, n * 4);
        if (q->seq_length) dev.fetch(q->seq_length, d.seq_length, n * 4);
        if (q->seq_done) dev.fetch(q->seq_done, d.seq_done, n);
        dev.finish();
    }
    if (dev.err != hipSuccess) return fail(std::string("pgv_step_sequence_host: ") + hipGetErrorString(dev.err));
    return 0;
}

// The frames of the state as it stands, by the launches pgv_reset draws its frames with: the pre-pass and the render launch
// under the mask.  Between steps a pending byte is 0 or 1 (or carries a parity), which no render launch touches.
// "Changes no state" means everything a result, a record or a snapshot can see.  Two things outside that do move, and are
// harmless only because of what they are: bossfight's pre-pass also makes the random streams' next blocks ahead (mt_other /
// mt_sel: the same words a gang would make in place), and chaser's complete path rewrites the base layers of the envs it
// draws and, with a NULL mask, sets base_valid_ (the layers depend on the level alone).  Nothing a step's outcome depends on
// may be hung on launch_prepass or launch_render.
int32_t pgv_render_obs(pgv_env* e, const uint8_t* d_mask) {
    if (!e) return fail("pgv_render_obs: env is NULL");
    PG_HIP(hipSetDevice(e->device));
    (void)hipGetLastError();
    e->game->launch_prepass(e->stream, d_mask);
    e->game->launch_render(e->stream, d_mask, e->io());
    PG_HIP(hipGetLastError());
    return 0;
}

int32_t pgv_render_obs_host(pgv_env* e, const uint8_t* h_mask) {
    if (!e) return fail("pgv_render_obs_host: env is NULL");
    PG_HIP(hipSetDevice(e->device));
    pg::Staged dev{e->stream};
    const uint8_t* d_mask = h_mask ? dev.alloc(size_t(e->n), h_mask) : nullptr;
    if (dev.err == hipSuccess) {
        if (const int32_t rc = pgv_render_obs(e, d_mask)) return rc;
        dev.finish();
    }
    if (dev.err != hipSuccess) return fail(std::string("pgv_render_obs_host: ") + hipGetErrorString(dev.err));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Policy-ready observations (pg_policy_obs.h)
// ------------------------------------------------------------------------------------------------
int32_t pgv_policy_obs_enable(pgv_env* e, const pgv_policy_obs_config* cfg) {
    if (!e) return fail("pgv_policy_obs_enable: env is NULL");
    if (!cfg || cfg->struct_size < sizeof(pgv_policy_obs_config)) return fail("pgv_policy_obs_enable: config is NULL or struct_size too small");
    if (e->policy) return fail("pgv_policy_obs_enable: policy observations are enabled already (once per env)");
    if (cfg->stack < 1 || cfg->stack > pg::kPolicyMaxStack) return fail("pgv_policy_obs_enable: stack must be in 1 .. 8");
    if (cfg->gray != 0 && cfg->gray != 1) return fail("pgv_policy_obs_enable: gray must be 0 or 1");
    if (!pg::policy_dtype_known(cfg->dtype)) return fail("pgv_policy_obs_enable: unknown dtype " + std::to_string(cfg->dtype));
    if (reinterpret_cast<uintptr_t>(cfg->out) & 15u) return fail("pgv_policy_obs_enable: out must be 16-byte aligned");
    PG_HIP(hipSetDevice(e->device));
    const int planes = cfg->gray ? 1 : 3, es = pg::policy_element_bytes(cfg->dtype);
    const size_t out_bytes = size_t(e->n) * pg::policy_bytes_per_env(cfg->stack, planes, es);
    void* mem = nullptr;
    void* out = cfg->out;
    pg::PolicyObsBuffers b{};
    hipError_t err = hipMalloc(&mem, pg::Carve::size(pg::list_policy_obs, e->n));
    if (err == hipSuccess && !out) err = hipMalloc(&out, out_bytes);
    if (err == hipSuccess && !cfg->out) err = hipMemsetAsync(out, 0, out_bytes, e->stream);
    if (err == hipSuccess) {
        pg::Carve::bind(pg::list_policy_obs, mem, b, e->n);
        err = hipMemsetAsync(b.restart, 1, size_t(e->n), e->stream);  // the first push fills every stack
    }
    if (err == hipSuccess) err = hipMemcpyAsync(b.table, e->value_tables[cfg->dtype], sizeof(e->value_tables[0]), hipMemcpyHostToDevice, e->stream);
    if (err != hipSuccess) {
        (void)hipStreamSynchronize(e->stream);
        if (mem) (void)hipFree(mem);
        if (out && !cfg->out) (void)hipFree(out);
        return fail(std::string("pgv_policy_obs_enable: ") + hipGetErrorString(err));
    }
    e->d_policy = mem;
    e->pol = b;
    e->d_policy_out = static_cast<uint8_t*>(out);
    e->own_policy_out = !cfg->out;
    e->policy_stack = cfg->stack;
    e->policy_planes = planes;
    e->policy_es = es;
    e->policy = true;
    return 0;
}

void* pgv_policy_obs(pgv_env* e) { return e && e->policy ? e->d_policy_out : nullptr; }
int64_t pgv_policy_obs_bytes_per_env(pgv_env* e) {
    return e && e->policy ? static_cast<int64_t>(pg::policy_bytes_per_env(e->policy_stack, e->policy_planes, e->policy_es)) : 0;
}
const uint8_t* pgv_policy_obs_restart(pgv_env* e) { return e && e->policy ? e->pol.restart : nullptr; }

int32_t pgv_policy_obs_push(pgv_env* e, const uint8_t* d_mask) {
    if (!e) return fail("pgv_policy_obs_push: env is NULL");
    if (!e->policy) return fail("pgv_policy_obs_push: call pgv_policy_obs_enable first");
    PG_HIP(hipSetDevice(e->device));
    if (slab_ready("pgv_policy_obs_push", e)) return 1;
    (void)hipGetLastError();
    return policy_push("pgv_policy_obs_push", e, d_mask);
}

int32_t pgv_policy_obs_push_host(pgv_env* e, const uint8_t* h_mask) {
    if (!e) return fail("pgv_policy_obs_push_host: env is NULL");
    if (!e->policy) return fail("pgv_policy_obs_push_host: call pgv_policy_obs_enable first");
    PG_HIP(hipSetDevice(e->device));
    pg::Staged dev{e->stream};
    const uint8_t* d_mask = h_mask ? dev.alloc(size_t(e->n), h_mask) : nullptr;
    if (dev.err == hipSuccess) {
        if (const int32_t rc = pgv_policy_obs_push(e, d_mask)) return rc;
        dev.finish();
    }
    if (dev.err != hipSuccess) return fail(std::string("pgv_policy_obs_push_host: ") + hipGetErrorString(dev.err));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Frame history (pg_history.h)
// ------------------------------------------------------------------------------------------------
int32_t pgv_history_enable(pgv_env* e, const pgv_history_config* cfg) {
    if (!e) return fail("pgv_history_enable: env is NULL");
    if (!cfg || cfg->struct_size < sizeof(pgv_history_config)) return fail("pgv_history_enable: config is NULL or struct_size too small");
    if (e->history) return fail("pgv_history_enable: the frame history is enabled already (once per env)");
    if (cfg->capacity < 1) return fail("pgv_history_enable: capacity must be >= 1");
    if (cfg->gray != 0 && cfg->gray != 1) return fail("pgv_history_enable: gray must be 0 or 1");
    if (reinterpret_cast<uintptr_t>(cfg->frames) & 15u) return fail("pgv_history_enable: frames must be 16-byte aligned");
    PG_HIP(hipSetDevice(e->device));
    pg::HistoryBuffers b{};
    b.capacity = cfg->capacity;
    b.planes = cfg->gray ? 1 : 3;
    b.own_frames = cfg->frames ? 0 : 1;
    const size_t bytes = pg::Carve::size(pg::list_history, e->n, b);
    void* mem = nullptr;
    hipError_t err = hipMalloc(&mem, bytes);
    if (err == hipSuccess) {
        pg::Carve::bind(pg::list_history, mem, b, e->n);
        err = hipMemsetAsync(mem, 0, bytes, e->stream);  // began, and the engine's own frames
    }
    if (err == hipSuccess) err = hipMemsetAsync(b.pending, 1, size_t(e->n), e->stream);  // every env's first frame begins its history
    if (err == hipSuccess) err = hipMemcpyAsync(b.table, e->value_tables, sizeof(e->value_tables), hipMemcpyHostToDevice, e->stream);
    if (err != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(e->stream);
        if (mem) (void)hipFree(mem);
        return fail(std::string("pgv_history_enable: ") + hipGetErrorString(err));
    }
    if (cfg->frames) b.frames = static_cast<uint8_t*>(cfg->frames);
    e->d_history = mem;
    e->hist = b;
    e->history_head = 0;
    e->history = true;
    return 0;
}

uint8_t* pgv_history_frames(pgv_env* e) { return e && e->history ? e->hist.frames : nullptr; }
const uint8_t* pgv_history_began(pgv_env* e) { return e && e->history ? e->hist.began : nullptr; }
const uint8_t* pgv_history_pending(pgv_env* e) { return e && e->history ? e->hist.pending : nullptr; }
int64_t pgv_history_head(pgv_env* e) { return e ? e->history_head : -1; }
int32_t pgv_history_capacity(pgv_env* e) { return e && e->history ? e->hist.capacity : 0; }

int32_t pgv_history_push(pgv_env* e) {
    if (!e) return fail("pgv_history_push: env is NULL");
    if (!e->history) return fail("pgv_history_push: call pgv_history_enable first");
    if (slab_ready("pgv_history_push", e)) return 1;
    PG_HIP(hipSetDevice(e->device));
    (void)hipGetLastError();
    if (e->transitions && transition_record(e, RowOf{})) return 1;  // the slot's row: not recorded
    return history_push(e, false, nullptr);
}

// What both augmented calls check of `aug`, the same way; `who` heads the message.
static int32_t gather_aug_config(const char* who, const pgv_gather_aug* aug, pg::AugConfig& cfg) {
    if (!aug || aug->struct_size < sizeof(pgv_gather_aug)) return fail(std::string(who) + ": aug is NULL or struct_size too small");
    cfg = pg::AugConfig{aug->out_height, aug->out_width, aug->pad, aug->edge, aug->cutout_min, aug->cutout_max, aug->cutout_color, aug->seed};
    if (const char* why = pg::aug_config_error(cfg)) return fail(std::string(who) + ": " + why);
    if (reinterpret_cast<uintptr_t>(aug->params) & 3u) return fail(std::string(who) + ": params must be 4-byte aligned");
    return 0;
}

// What both gathers check of their arguments, in the order they check it, and the entry list they hand their kernel.  `cfg`
// (the augmented gather): its config is checked between the count and the tensor.  Leaves q.count = 0 where nothing is asked for.
// `out_optional` (the transition gather, whose rows are): a NULL tensor passes.
static int32_t gather_arguments(const char* who, pgv_env* e, const int64_t* d_pushes, const int32_t* d_envs, int32_t count, int32_t stack,
                                int32_t dtype, void* d_out, pg::HistoryGather& q, const pgv_gather_aug* aug = nullptr, pg::AugConfig* cfg = nullptr,
                                bool out_optional = false) {
    if (!e) return fail(std::string(who) + ": env is NULL");
    if (!e->history) return fail(std::string(who) + ": call pgv_history_enable first");
    if (stack < 1 || stack > pg::kPolicyMaxStack) return fail(std::string(who) + ": stack must be in 1 .. 8");
    if (!pg::policy_dtype_known(dtype)) return fail(std::string(who) + ": unknown dtype " + std::to_string(dtype));
    if (count < 0) return fail(std::string(who) + ": count is negative");
    if (cfg && gather_aug_config(who, aug, *cfg)) return 1;
    if (reinterpret_cast<uintptr_t>(d_out) & 15u) return fail(std::string(who) + ": out must be 16-byte aligned");
    if (count == 0) return 0;
    if (!d_pushes || !d_envs || (!d_out && !out_optional)) return fail(std::string(who) + ": pushes, envs or out is NULL");
    PG_HIP(hipSetDevice(e->device));
    (void)hipGetLastError();
    q.n = e->n, q.stack = stack, q.count = count, q.head = e->history_head;
    q.pushes = d_pushes, q.envs = d_envs, q.table = e->hist.table + dtype * 256, q.out = static_cast<uint8_t*>(d_out);
    q.b = e->hist;
    return 0;
}

int32_t pgv_history_gather(pgv_env* e, const int64_t* d_pushes, const int32_t* d_envs, int32_t count, int32_t stack, int32_t dtype, void* d_out) {
    pg::HistoryGather q{};
    if (gather_arguments("pgv_history_gather", e, d_pushes, d_envs, count, stack, dtype, d_out, q)) return 1;
    if (q.count == 0) return 0;
    pg::launch_history_gather(e->stream, q, pg::policy_element_bytes(dtype));
    PG_HIP(hipGetLastError());
    return 0;
}

int32_t pgv_gather_aug_params(const pgv_gather_aug* aug, int32_t entry, int32_t* h_params8) {
    pg::AugConfig cfg{};
    if (gather_aug_config("pgv_gather_aug_params", aug, cfg)) return 1;
    if (entry < 0) return fail("pgv_gather_aug_params: entry is negative");
    if (!h_params8) return fail("pgv_gather_aug_params: params8 is NULL");
    pg::aug_params_row(pg::aug_params(cfg, static_cast<uint32_t>(entry)), 3, h_params8);
    return 0;
}

int32_t pgv_history_gather_aug(pgv_env* e, const int64_t* d_pushes, const int32_t* d_envs, int32_t count, int32_t stack, int32_t dtype,
                               const pgv_gather_aug* aug, void* d_out) {
    pg::HistoryGatherAug q{};
    if (gather_arguments("pgv_history_gather_aug", e, d_pushes, d_envs, count, stack, dtype, d_out, q.g, aug, &q.cfg)) return 1;
    if (q.g.count == 0) return 0;
    q.params = aug->params;
    pg::launch_history_gather_aug(e->stream, q, pg::policy_element_bytes(dtype));
    PG_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Transitions (pg_transitions.h)
// ------------------------------------------------------------------------------------------------
int32_t pgv_transitions_enable(pgv_env* e, const pgv_transitions_config* cfg) {
    if (!e) return fail("pgv_transitions_enable: env is NULL");
    if (!cfg || cfg->struct_size < sizeof(pgv_transitions_config)) return fail("pgv_transitions_enable: config is NULL or struct_size too small");
    if (cfg->reserved != 0) return fail("pgv_transitions_enable: reserved must be 0");
    if (e->transitions) return fail("pgv_transitions_enable: transitions are enabled already (once per env)");
    if (!e->history) return fail("pgv_transitions_enable: call pgv_history_enable first");
    if (e->hist.capacity < 2) return fail("pgv_transitions_enable: the frame history's capacity must be >= 2 (a row needs two held pushes)");
    PG_HIP(hipSetDevice(e->device));
    pg::TransitionBuffers b{};
    b.capacity = e->hist.capacity;
    const size_t bytes = pg::Carve::size(pg::list_transitions, e->n, b);
    void* mem = nullptr;
    hipError_t err = hipMalloc(&mem, bytes);
    if (err == hipSuccess) err = hipMemsetAsync(mem, 0, bytes, e->stream);  // no row recorded, no reset found
    if (err != hipSuccess) {
        (void)hipGetLastError();
        if (mem) (void)hipFree(mem);
        return fail(std::string("pgv_transitions_enable: ") + hipGetErrorString(err));
    }
    pg::Carve::bind(pg::list_transitions, mem, b, e->n);
    e->d_transitions = mem;
    e->tr = b;
    e->transitions = true;
    return 0;
}

const int32_t* pgv_transitions_action(pgv_env* e) { return e && e->transitions ? e->tr.action : nullptr; }
const float* pgv_transitions_reward(pgv_env* e) { return e && e->transitions ? e->tr.reward : nullptr; }
const uint8_t* pgv_transitions_flags(pgv_env* e) { return e && e->transitions ? e->tr.flags : nullptr; }

static pg::TransitionRing transition_ring(const pgv_env* e) { return {e->n, e->hist.capacity, e->history_head, e->hist.began, e->tr}; }

int32_t pgv_transitions_gather(pgv_env* e, const int64_t* d_pushes, const int32_t* d_envs, int32_t count, const pgv_transition_query* query) {
    const char* who = "pgv_transitions_gather";
    if (!e) return fail(std::string(who) + ": env is NULL");
    if (!e->transitions) return fail(std::string(who) + ": call pgv_transitions_enable first");
    if (!query || query->struct_size < sizeof(pgv_transition_query)) return fail(std::string(who) + ": query is NULL or struct_size too small");
    if (query->n < 1 || query->n > pg::kTrMaxSteps) return fail(std::string(who) + ": n must be in 1 .. 64");
    if (reinterpret_cast<uintptr_t>(query->next_obs) & 15u) return fail(std::string(who) + ": next_obs must be 16-byte aligned");
    for (const void* p : {static_cast<const void*>(query->action), static_cast<const void*>(query->nstep_return),
                          static_cast<const void*>(query->discount), static_cast<const void*>(query->steps)})
        if (reinterpret_cast<uintptr_t>(p) & 3u) return fail(std::string(who) + ": action, nstep_return, discount and steps must be 4-byte aligned");
    pg::TransitionGather q{};
    // (what pgv_history_gather checks, the way it checks it)
    if (gather_arguments(who, e, d_pushes, d_envs, count, query->stack, query->dtype, query->obs, q.g, nullptr, nullptr, /*out_optional=*/true)) return 1;
    if (q.g.count == 0) return 0;
    q.g.out = nullptr;  // (the two rows below)
    q.steps = query->n;
    q.gamma = query->gamma;
    q.ring = transition_ring(e);
    q.obs = static_cast<uint8_t*>(query->obs), q.next_obs = static_cast<uint8_t*>(query->next_obs);
    q.action = query->action, q.nstep_return = query->nstep_return, q.discount = query->discount, q.step_count = query->steps, q.status = query->status;
    pg::launch_transition_gather(e->stream, q, pg::policy_element_bytes(query->dtype));
    PG_HIP(hipGetLastError());
    return 0;
}

int32_t pgv_transitions_gae(pgv_env* e, int64_t first, int32_t length, const pgv_gae* gae) {
    const char* who = "pgv_transitions_gae";
    if (!e) return fail(std::string(who) + ": env is NULL");
    if (!e->transitions) return fail(std::string(who) + ": call pgv_transitions_enable first");
    if (!gae || gae->struct_size < sizeof(pgv_gae)) return fail(std::string(who) + ": gae is NULL or struct_size too small");
    if (length < 1) return fail(std::string(who) + ": length must be >= 1");
    const int64_t head = e->history_head;
    // rows first .. first + length - 1, each with head - T <= q and q + 1 < head (length < T then, and nothing overflows)
    if (first < 0 || first < head - e->hist.capacity || first >= head || int64_t(length) > head - 1 - first)
        return fail(std::string(who) + ": rows " + std::to_string(first) + " .. + " + std::to_string(length) + " are not all held with their successors (head " +
                    std::to_string(head) + ", capacity " + std::to_string(e->hist.capacity) + ")");
    if (!gae->values || !gae->advantages) return fail(std::string(who) + ": values or advantages is NULL");
    for (const void* p : {static_cast<const void*>(gae->values), static_cast<const void*>(gae->trunc_values),
                          static_cast<const void*>(gae->advantages), static_cast<const void*>(gae->returns)})
        if (reinterpret_cast<uintptr_t>(p) & 3u) return fail(std::string(who) + ": values, trunc_values, advantages and returns must be 4-byte aligned");
    PG_HIP(hipSetDevice(e->device));
    (void)hipGetLastError();
    pg::TransitionGae q{};
    q.n = e->n, q.length = length, q.first = first;
    q.gamma = gae->gamma, q.lambda = gae->lambda;
    q.values = gae->values, q.trunc_values = gae->trunc_values, q.advantages = gae->advantages, q.returns = gae->returns;
    q.ring = transition_ring(e);
    pg::launch_transition_gae(e->stream, q);
    PG_HIP(hipGetLastError());
    return 0;
}

int32_t pgv_decode_png(const char* path, int32_t* w, int32_t* h, uint8_t* h_rgba, int64_t cap) {
    pg::Image img;
    std::string err;
    if (!path || !pg::decode_png_file(path, img, err)) return fail("pgv_decode_png: " + err);
    if (w) *w = img.w;
    if (h) *h = img.h;
    if (h_rgba && cap > 0) {
        size_t nbytes = img.rgba.size() < static_cast<size_t>(cap) ? img.rgba.size() : static_cast<size_t>(cap);
        std::memcpy(h_rgba, img.rgba.data(), nbytes);
    }
    return 0;
}

int64_t pgv_generator_launches(pgv_env* e) { return e ? e->generator_launches : -1; }

int32_t pgv_sync(pgv_env* e) {
    if (!e) return fail("pgv_sync: env is NULL");
    PG_HIP(hipSetDevice(e->device));
    PG_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

// Whole-batch snapshot / restore (SURVEY.md §8f-4, §5 checkpoint/resume): everything a rollout depends on — the game
// state blob (live state, generator chains, prefetched levels and their slot words), reward / done / pending, the
// step counter and the observation slab — as one host buffer.  Both streams are drained first, so no slot is busy.
struct SnapshotHeader {
    uint32_t magic, game;
    int32_t n, env_offset;
    uint64_t state_bytes;
    uint32_t step_index;
    int32_t num_levels, start_level, mode;
    uint32_t game_flags, reserved;
};
// "PGN" + the version of the state-blob layouts: bump it whenever any game's State / Level / field enums change — equal
// state_bytes does not mean equal layout (sizes are rounded to 256 bytes), and an old blob would load silently.
// 2: round 2.  3: round 3 (per-env contiguous rings and entity tables in bossfight, caveflyer, chaser, climber; caveflyer's
// wall-bit columns and hazard places).  4: round 5/6 (the pending byte carries the parity of the step it is about —
// pg_prefetch.h reset_due_mark / reset_served_mark — where it used to be 0 / 1; coinrun's hazard hand-off left the blob).
// 5: the level plan's assignment arrays lie behind the game's state (pg_carve.h LevelPlan; pgv_assign_levels).
static constexpr uint32_t kSnapshotMagic = 0x50474e35u;

static size_t snapshot_bytes(pgv_env* e) {
    size_t bytes = sizeof(SnapshotHeader) + state_blob_bytes(e);
    for (const pgv_env::Row& row : e->rows()) bytes += size_t(e->n) * row.bytes_per_env;
    return bytes;
}
// What follows the header: the state blob, then the output rows — device to host (save) or back (load).
static int32_t snapshot_copy(pgv_env* e, uint8_t* h_body, size_t blob_bytes, bool load) {
    std::vector<std::pair<void*, size_t>> parts{{e->d_state, blob_bytes}};
    for (const pgv_env::Row& row : e->rows()) parts.push_back({*row.d, size_t(e->n) * row.bytes_per_env});
    for (const auto& [d, bytes] : parts) {
        PG_HIP(load ? hipMemcpy(d, h_body, bytes, hipMemcpyHostToDevice) : hipMemcpy(h_body, d, bytes, hipMemcpyDeviceToHost));
        h_body += bytes;
    }
    return 0;
}

int64_t pgv_snapshot_bytes(pgv_env* e) { return e ? static_cast<int64_t>(snapshot_bytes(e)) : -1; }

int32_t pgv_save_state(pgv_env* e, void* h_buffer, int64_t capacity) {
    if (!e || !h_buffer) return fail("pgv_save_state: NULL argument");
    if (capacity < static_cast<int64_t>(snapshot_bytes(e))) return fail("pgv_save_state: buffer too small");
    PG_HIP(hipSetDevice(e->device));
    e->game->prepare_save(e->stream);
    PG_HIP(hipGetLastError());
    PG_HIP(hipStreamSynchronize(e->stream));
    if (e->side) PG_HIP(hipStreamSynchronize(e->side));
    uint8_t* out = static_cast<uint8_t*>(h_buffer);
    SnapshotHeader hd{kSnapshotMagic, static_cast<uint32_t>(pgv_game_id(e->game->name())), e->n, e->env_offset,
                      state_blob_bytes(e), e->step_index, e->game->plan.num_levels, e->game->plan.start_level, e->mode, e->game_flags, 0};
    std::memcpy(out, &hd, sizeof(hd));
    return snapshot_copy(e, out + sizeof(hd), hd.state_bytes, false);
}

int32_t pgv_load_state(pgv_env* e, const void* h_buffer, int64_t size) {
    if (!e || !h_buffer) return fail("pgv_load_state: NULL argument");
    if (size < static_cast<int64_t>(snapshot_bytes(e))) return fail("pgv_load_state: buffer too small for this env");
    const uint8_t* in = static_cast<const uint8_t*>(h_buffer);
    SnapshotHeader hd;
    std::memcpy(&hd, in, sizeof(hd));
    if (hd.magic != kSnapshotMagic || hd.game != static_cast<uint32_t>(pgv_game_id(e->game->name())) || hd.n != e->n ||
        hd.env_offset != e->env_offset || hd.state_bytes != state_blob_bytes(e) ||
        hd.num_levels != e->game->plan.num_levels || hd.start_level != e->game->plan.start_level || hd.mode != e->mode ||
        hd.game_flags != e->game_flags)
        return fail("pgv_load_state: snapshot of a different env (game, mode, size, shard or level set)");
    PG_HIP(hipSetDevice(e->device));
    PG_HIP(hipStreamSynchronize(e->stream));
    if (e->side) PG_HIP(hipStreamSynchronize(e->side));
    if (snapshot_copy(e, const_cast<uint8_t*>(in) + sizeof(hd), hd.state_bytes, true)) return 1;
    e->step_index = hd.step_index;
    PG_HIP(e->game->state_loaded(e->stream));  // (on the env's stream: ordered in front of the next step)
    // neither the stacks nor the ring travel: every env restarts
    for (uint8_t* flags : flag_arrays(e))
        if (flags) pg::launch_policy_flag_mask(e->stream, flags, e->n, nullptr);
    pregen(e, true, true);  // queued shadow slots of the snapshot get their generator launch
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Per-env records (pg_records.h)
// ------------------------------------------------------------------------------------------------
int64_t pgv_env_record_bytes(pgv_env* e) { return e ? static_cast<int64_t>(e->rec.record_bytes) : -1; }
uint64_t pgv_env_record_tag(pgv_env* e) { return e ? e->rec_tag : 0; }

// The env's stream waits for what the generator's stream holds so far, so no prefetch slot is kSlotBusy while records are
// read or written: a slot is then idle, queued or ready, and travels as it is (a generator launched later waits for an
// event the env's stream records later: pregen).  Events only; the host goes on.
static int32_t records_behind_generator(pgv_env* e) {
    if (!e->side) return 0;
    PG_HIP(hipEventRecord(e->rec_ev, e->side));
    PG_HIP(hipStreamWaitEvent(e->stream, e->rec_ev, 0));
    return 0;
}
static pg::RecordTable records_table(const pgv_env* e) {
    pg::RecordTable t = e->rec;
    t.r[e->rec_reward].base = reinterpret_cast<uint8_t*>(e->d_reward);
    t.r[e->rec_done].base = e->d_done;
    t.r[e->rec_obs].base = e->d_obs;
    t.pending = e->d_pending;
    // "a reset is due" as the pending byte says it for the step that comes next in THIS engine
    t.due_mark = t.due_code = e->game->pending_has_parity() ? pg::reset_due_mark(e->step_index) : 1;
    return t;
}
static int32_t records_arguments(const char* who, pgv_env* e, int32_t count, const void* records) {
    if (!e) return fail(std::string(who) + ": env is NULL");
    if (count < 0) return fail(std::string(who) + ": count is negative");
    if (count > 0 && !records) return fail(std::string(who) + ": the record buffer is NULL");
    return 0;
}

int32_t pgv_save_envs(pgv_env* e, const int32_t* d_indices, int32_t count, void* d_records) {
    if (records_arguments("pgv_save_envs", e, count, d_records)) return 1;
    if (count == 0) return 0;
    if (reinterpret_cast<uintptr_t>(d_records) & 15u) return fail("pgv_save_envs: the record buffer must be 16-byte aligned");
    PG_HIP(hipSetDevice(e->device));
    (void)hipGetLastError();
    e->game->prepare_save(e->stream);  // random streams that live in two buffers come home (a no-op elsewhere)
    if (records_behind_generator(e)) return 1;
    pg::launch_records(e->stream, records_table(e), false, d_indices, count, d_records);
    PG_HIP(hipGetLastError());
    return 0;
}

int32_t pgv_load_envs(pgv_env* e, const int32_t* d_indices, int32_t count, const void* d_records, uint64_t tag) {
    if (records_arguments("pgv_load_envs", e, count, d_records)) return 1;
    if (tag != e->rec_tag)
        return fail("pgv_load_envs: records of another configuration (game, mode, game_flags, level set or record layout): tag " +
                    std::to_string(tag) + ", this engine's is " + std::to_string(e->rec_tag));
    if (count == 0) return 0;
    if (reinterpret_cast<uintptr_t>(d_records) & 15u) return fail("pgv_load_envs: the record buffer must be 16-byte aligned");
    PG_HIP(hipSetDevice(e->device));
    (void)hipGetLastError();
    if (records_behind_generator(e)) return 1;
    const pg::RecordTable t = records_table(e);
    pg::launch_records(e->stream, t, true, d_indices, count, const_cast<void*>(d_records));
    e->game->records_loaded(e->stream, d_indices, count, static_cast<const uint8_t*>(d_records), t.record_bytes, t.r[e->rec_obs].offset,
                            e->step_index, e->io());
    for (uint8_t* flags : flag_arrays(e))  // the slots actually written restart their stacks and begin their history afresh
        if (flags) pg::launch_policy_flag_list(e->stream, flags, e->n, d_indices, count, static_cast<const uint8_t*>(d_records), t.record_bytes, pg::kRecordFull);
    PG_HIP(hipGetLastError());
    pregen(e, size_t(count) * 2 >= size_t(e->n), true);  // loaded slots that are queued get their generator launch
    return 0;
}

// Host-pointer forms: device buffers for the call, a synchronous copy either way.
static int32_t records_host(pgv_env* e, const int32_t* h_indices, int32_t count, void* h_records, bool load, uint64_t tag) {
    const char* who = load ? "pgv_load_envs_host" : "pgv_save_envs_host";
    if (records_arguments(who, e, count, h_records)) return 1;
    if (load && tag != e->rec_tag) return pgv_load_envs(e, nullptr, count, h_records, tag);  // (refused there, before anything is touched)
    if (count == 0) return 0;
    PG_HIP(hipSetDevice(e->device));
    const size_t bytes = size_t(count) * e->rec.record_bytes;
    pg::Staged dev{e->stream};
    uint8_t* d_records = dev.alloc<uint8_t>(bytes);
    const int32_t* d_indices = h_indices ? dev.alloc(size_t(count), h_indices) : nullptr;
    if (load) dev.upload(d_records, h_records, bytes);
    if (dev.err == hipSuccess) {
        if (const int32_t rc = load ? pgv_load_envs(e, d_indices, count, d_records, tag) : pgv_save_envs(e, d_indices, count, d_records)) return rc;
        if (load) dev.finish(); else dev.fetch(h_records, d_records, bytes);
    }
    if (dev.err != hipSuccess) return fail(std::string(who) + ": " + hipGetErrorString(dev.err));
    return 0;
}
int32_t pgv_save_envs_host(pgv_env* e, const int32_t* h_indices, int32_t count, void* h_records) {
    return records_host(e, h_indices, count, h_records, false, 0);
}
int32_t pgv_load_envs_host(pgv_env* e, const int32_t* h_indices, int32_t count, const void* h_records, uint64_t tag) {
    return records_host(e, h_indices, count, const_cast<void*>(h_records), true, tag);
}

// ------------------------------------------------------------------------------------------------
// Assigned levels (pg_carve.h LevelPlan)
// ------------------------------------------------------------------------------------------------
}  // extern "C"

namespace pg {
// Lanes along the indices.  Runs on the env's stream behind everything the generator's stream held (records_behind_generator),
// so no slot is kSlotBusy, and between the kernels of the env's stream, so none is kSlotSync: a slot is idle, queued or
// ready.  A ready slot holds the level the env WOULD have built next; unless that is the very level now assigned it goes
// back into the queue — the generator, launched behind this kernel, consumes the assignment — and where it was a level of
// the env's own sequence, the sequence steps back to it (level-seed mode: k).  In free mode the chain has moved past the
// discarded level; an assigned level starts the chain afresh, so nothing is lost that anything would read.
__global__ void __launch_bounds__(256) assign_levels_kernel(LevelPlan plan, int32_t* slot, int n, const int32_t* indices, int count,
                                                            const int32_t* levels) {
    const int k = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= count) return;
    const int env = indices ? indices[k] : k;
    if (env < 0 || env >= n) return;
    const uint32_t number = static_cast<uint32_t>(levels[k]);
    if (slot && slot_load(&slot[env]) == kSlotReady) {
        const bool was_assigned = plan.slot_assigned[env] != 0;
        if (was_assigned && plan.slot_number[env] == number) return;  // (its assignment was consumed: none is pending)
        // (the exchange decides between two lanes that name the same env: one of them steps the sequence back)
        if (slot_cas(&slot[env], kSlotReady, kSlotQueued) && !was_assigned && plan.num_levels > 0) plan.drawn[env] -= 1u;
    }
    plan.assigned[env] = number;
    plan.assigned_on[env] = 1;
}
}  // namespace pg

extern "C" {

int32_t pgv_assign_levels(pgv_env* e, const int32_t* d_indices, int32_t count, const int32_t* d_levels) {
    if (!e) return fail("pgv_assign_levels: env is NULL");
    if (count < 0) return fail("pgv_assign_levels: count is negative");
    if (count > 0 && !d_levels) return fail("pgv_assign_levels: the level buffer is NULL");
    if (count == 0) return 0;
    PG_HIP(hipSetDevice(e->device));
    (void)hipGetLastError();
    if (records_behind_generator(e)) return 1;
    hipLaunchKernelGGL(pg::assign_levels_kernel, dim3((count + 255) / 256), dim3(256), 0, e->stream, e->game->plan,
                       e->game->prefetch_slots(), e->n, d_indices, count, d_levels);
    PG_HIP(hipGetLastError());
    // The slots put back in the queue get their generator launch.  Not the bulk shape, whatever `count` is: a call may name
    // every env and mean few (indices outside the batch are skipped: a caller's way to a fixed-size call), and few is the
    // common case — the envs that just finished.
    pregen(e, false, true);
    return 0;
}

int32_t pgv_assign_levels_host(pgv_env* e, const int32_t* h_indices, int32_t count, const int32_t* h_levels) {
    if (!e) return fail("pgv_assign_levels_host: env is NULL");
    if (count < 0) return fail("pgv_assign_levels_host: count is negative");
    if (count > 0 && !h_levels) return fail("pgv_assign_levels_host: the level buffer is NULL");
    if (count == 0) return 0;
    PG_HIP(hipSetDevice(e->device));
    pg::Staged dev{e->stream};  // (a call may name more indices than the batch has envs: not the staging buffers)
    const int32_t* d_levels = dev.alloc(size_t(count), h_levels);
    const int32_t* d_indices = h_indices ? dev.alloc(size_t(count), h_indices) : nullptr;
    if (dev.err != hipSuccess) return fail(std::string("pgv_assign_levels_host: ") + hipGetErrorString(dev.err));
    return pgv_assign_levels(e, d_indices, count, d_levels);  // (the host buffers are the caller's: drained on the way out)
}

const uint32_t* pgv_level_numbers(pgv_env* e) { return e ? e->game->plan.number : nullptr; }
const uint8_t* pgv_level_known(pgv_env* e) { return e ? e->game->plan.known : nullptr; }

uint8_t* pgv_obs(pgv_env* e) { return e ? e->d_obs : nullptr; }
float* pgv_reward(pgv_env* e) { return e ? e->d_reward : nullptr; }
uint8_t* pgv_done(pgv_env* e) { return e ? e->d_done : nullptr; }
int32_t pgv_num_envs(pgv_env* e) { return e ? e->n : 0; }
int32_t pgv_device(pgv_env* e) { return e ? e->device : -1; }
void* pgv_stream(pgv_env* e) { return e ? static_cast<void*>(e->stream) : nullptr; }

int32_t pgv_bind_outputs(pgv_env* e, uint8_t* d_obs, float* d_reward, uint8_t* d_done) {
    if (!e) return fail("pgv_bind_outputs: env is NULL");
    PG_HIP(hipSetDevice(e->device));
    PG_HIP(hipStreamSynchronize(e->stream));
    if (d_obs) {
        PG_HIP(hipMemcpy(d_obs, e->d_obs, size_t(e->n) * pg::kObsBytes, hipMemcpyDeviceToDevice));
        if (e->own_obs) hipFree(e->d_obs);
        e->d_obs = d_obs;
        e->own_obs = false;
    }
    if (d_reward) {
        PG_HIP(hipMemcpy(d_reward, e->d_reward, size_t(e->n) * 4, hipMemcpyDeviceToDevice));
        if (e->own_reward) hipFree(e->d_reward);
        e->d_reward = d_reward;
        e->own_reward = false;
    }
    if (d_done) {
        PG_HIP(hipMemcpy(d_done, e->d_done, size_t(e->n), hipMemcpyDeviceToDevice));
        if (e->own_done) hipFree(e->d_done);
        e->d_done = d_done;
        e->own_done = false;
    }
    return 0;
}

int32_t pgv_copy_out(pgv_env* e, uint8_t* h_obs, float* h_reward, uint8_t* h_done) {
    if (!e) return fail("pgv_copy_out: env is NULL");
    PG_HIP(hipSetDevice(e->device));
    PG_HIP(hipStreamSynchronize(e->stream));
    if (h_obs) PG_HIP(hipMemcpy(h_obs, e->d_obs, size_t(e->n) * pg::kObsBytes, hipMemcpyDeviceToHost));
    if (h_reward) PG_HIP(hipMemcpy(h_reward, e->d_reward, size_t(e->n) * 4, hipMemcpyDeviceToHost));
    if (h_done) PG_HIP(hipMemcpy(h_done, e->d_done, size_t(e->n), hipMemcpyDeviceToHost));
    return 0;
}

// Per-step events of a run of synthetic steps, created before the region starts and destroyed on every way out; they are
// read back after the region so the host never stalls the stream inside it.
namespace {
struct StepEvents {
    std::vector<hipEvent_t> v;
    ~StepEvents() {
        for (hipEvent_t p : v)
            if (p) hipEventDestroy(p);
    }
};
}  // namespace

namespace pg {
// `steps` synthetic steps of `count` envs side by side (step s of every env enqueued before step s + 1 of any, each on
// its own stream, as pgv_step_synthetic_many), every step cut into its phases by events on the env's stream.
// out[5 * k + j]: `steps` floats of env k — j = 0 the whole step, 1 logic, 2 pre-pass, 3 render, 4 late — or NULL.
static int32_t step_phases_many(pgv_env* const* envs, int count, int steps, uint32_t run_seed, float* const* out) {
    if (steps < 1 || steps > (1 << 20)) return fail("pgv_step_phases: steps must be in 1..1048576");
    std::vector<StepEvents> ev(static_cast<size_t>(count));  // per step: start, after logic, before render, after render; one more at the end
    for (int k = 0; k < count; k++) {
        PG_HIP(hipSetDevice(envs[k]->device));
        ev[k].v.assign(size_t(steps) * 4 + 1, nullptr);
        for (auto& p : ev[k].v) PG_HIP(hipEventCreate(&p));
    }
    for (int s = 0; s < steps; s++)
        for (int k = 0; k < count; k++) {
            pgv_env* e = envs[k];
            PG_HIP(hipSetDevice(e->device));
            PG_HIP(hipEventRecord(ev[k].v[4 * s], e->stream));
            if (step_impl(e, nullptr, run_seed, ev[k].v[4 * s + 2], ev[k].v[4 * s + 3], ev[k].v[4 * s + 1])) return 1;
        }
    for (int k = 0; k < count; k++) {
        PG_HIP(hipSetDevice(envs[k]->device));
        PG_HIP(hipEventRecord(ev[k].v[size_t(steps) * 4], envs[k]->stream));
    }
    static const int kFrom[5] = {0, 0, 1, 2, 3}, kTo[5] = {4, 1, 2, 3, 4};
    for (int k = 0; k < count; k++) {
        PG_HIP(hipSetDevice(envs[k]->device));
        PG_HIP(hipEventSynchronize(ev[k].v[size_t(steps) * 4]));
        for (int j = 0; j < 5; j++) {
            float* to = out[5 * k + j];
            if (!to) continue;
            for (int s = 0; s < steps; s++) PG_HIP(hipEventElapsedTime(&to[s], ev[k].v[4 * s + kFrom[j]], ev[k].v[4 * s + kTo[j]]));
        }
    }
    return 0;
}
}  // namespace pg

int32_t pgv_timed_steps(pgv_env* e, int32_t steps, uint32_t run_seed, double* total_ms, double* render_kernel_ms) {
    if (!e) return fail("pgv_timed_steps: env is NULL");
    if (steps < 1 || steps > (1 << 20)) return fail("pgv_timed_steps: steps must be in 1..1048576");
    PG_HIP(hipSetDevice(e->device));
    // render_kernel_ms == NULL: nothing but the steps between the region's two events (the form bench.py's `value` uses).
    StepEvents pairs;
    if (render_kernel_ms) {
        pairs.v.assign(size_t(steps) * 2, nullptr);
        for (auto& p : pairs.v) PG_HIP(hipEventCreate(&p));
    }
    PG_HIP(hipEventRecord(e->ev[0], e->stream));  // whole region on the env's stream
    for (int s = 0; s < steps; s++)
        if (step_impl(e, nullptr, run_seed, render_kernel_ms ? pairs.v[2 * s] : nullptr,
                      render_kernel_ms ? pairs.v[2 * s + 1] : nullptr))
            return 1;
    PG_HIP(hipEventRecord(e->ev[1], e->stream));
    PG_HIP(hipEventSynchronize(e->ev[1]));
    float ms = 0.0f;
    PG_HIP(hipEventElapsedTime(&ms, e->ev[0], e->ev[1]));
    if (total_ms) *total_ms = ms;
    if (render_kernel_ms) {
        double render_sum = 0.0;
        for (int s = 0; s < steps; s++) {
            float k = 0.0f;
            PG_HIP(hipEventElapsedTime(&k, pairs.v[2 * s], pairs.v[2 * s + 1]));
            render_sum += k;
        }
        *render_kernel_ms = render_sum;
    }
    return 0;
}

int32_t pgv_step_times(pgv_env* e, int32_t steps, uint32_t run_seed, float* h_step_ms, float* h_render_ms) {
    return pgv_step_phases(e, steps, run_seed, h_step_ms, nullptr, nullptr, h_render_ms, nullptr);
}

int32_t pgv_step_phases(pgv_env* e, int32_t steps, uint32_t run_seed, float* h_step_ms, float* h_logic_ms, float* h_prepass_ms,
                        float* h_render_ms, float* h_late_ms) {
    if (!e) return fail("pgv_step_phases: env is NULL");
    float* out[5] = {h_step_ms, h_logic_ms, h_prepass_ms, h_render_ms, h_late_ms};
    return pg::step_phases_many(&e, 1, steps, run_seed, out);
}

int32_t pgv_step_phases_many(pgv_env* const* envs, int32_t count, int32_t steps, uint32_t run_seed, float* h_ms) {
    if (!envs || count < 1 || !h_ms) return fail("pgv_step_phases_many: bad arguments");
    for (int32_t k = 0; k < count; k++)
        if (!envs[k]) return fail("pgv_step_phases_many: env is NULL");
    std::vector<float*> out(size_t(count) * 5);
    for (size_t k = 0; k < out.size(); k++) out[k] = h_ms + k * size_t(steps > 0 ? steps : 0);
    return pg::step_phases_many(envs, count, steps, run_seed, out.data());
}

int32_t pgv_step_episodes_times(pgv_env* e, int32_t steps, uint32_t run_seed, float* h_step_ms, float* h_episode_ms) {
    if (!e) return fail("pgv_step_episodes_times: env is NULL");
    if (steps < 1 || steps > (1 << 20)) return fail("pgv_step_episodes_times: steps must be in 1..1048576");
    PG_HIP(hipSetDevice(e->device));
    StepEvents ev;  // per step: start, before the episode launches, behind them; one more at the end
    ev.v.assign(size_t(steps) * 3 + 1, nullptr);
    for (auto& p : ev.v) PG_HIP(hipEventCreate(&p));
    for (int s = 0; s < steps; s++) {
        PG_HIP(hipEventRecord(ev.v[3 * s], e->stream));
        if (step_episodes_impl("pgv_step_episodes_times", e, nullptr, run_seed, ev.v[3 * s + 1], ev.v[3 * s + 2])) return 1;
    }
    PG_HIP(hipEventRecord(ev.v[size_t(steps) * 3], e->stream));
    PG_HIP(hipEventSynchronize(ev.v[size_t(steps) * 3]));
    for (int s = 0; s < steps; s++) {
        if (h_step_ms) PG_HIP(hipEventElapsedTime(&h_step_ms[s], ev.v[3 * s], ev.v[3 * s + 3]));
        if (h_episode_ms) PG_HIP(hipEventElapsedTime(&h_episode_ms[s], ev.v[3 * s + 1], ev.v[3 * s + 2]));
    }
    return 0;
}

int32_t pgv_render_frame(pgv_env* e, int32_t index, int32_t width, int32_t height, uint8_t* h_rgb) {
    if (!e) return fail("pgv_render_frame: env is NULL");
    if (index < 0 || index >= e->n) return fail("pgv_render_frame: env index out of range");
    if (width < 1 || height < 1 || width > 4096 || height > 4096 || !h_rgb)
        return fail("pgv_render_frame: bad frame size or NULL buffer");
    PG_HIP(hipSetDevice(e->device));
    const size_t px = size_t(width) * height;
    pg::Staged dev{e->stream};
    uint32_t* d_px = dev.alloc<uint32_t>(px);
    if (dev.err == hipSuccess && !e->game->launch_frame(e->stream, index, d_px, width, height))
        return fail(std::string("pgv_render_frame: not implemented for ") + e->game->name());
    std::vector<uint32_t> host(px);
    if (dev.err == hipSuccess) dev.err = hipGetLastError();
    dev.fetch(host.data(), d_px, px * 4);
    if (dev.err != hipSuccess) return fail(std::string("pgv_render_frame: ") + hipGetErrorString(dev.err));
    for (size_t k = 0; k < px; k++) {  // RGBA → RGB, row-major (coinrun.cpp:401-407)
        h_rgb[3 * k + 0] = static_cast<uint8_t>(host[k]);
        h_rgb[3 * k + 1] = static_cast<uint8_t>(host[k] >> 8);
        h_rgb[3 * k + 2] = static_cast<uint8_t>(host[k] >> 16);
    }
    return 0;
}

int32_t pgv_render_frames(pgv_env* e, const int32_t* d_indices, int32_t count, int32_t width, int32_t height, uint8_t* d_rgb) {
    if (!e) return fail("pgv_render_frames: env is NULL");
    if (count < 0) return fail("pgv_render_frames: count is negative");
    if (width < 1 || height < 1 || width > 4096 || height > 4096 || !d_rgb)
        return fail("pgv_render_frames: bad frame size or NULL buffer");
    if (count == 0) return 0;
    PG_HIP(hipSetDevice(e->device));
    e->game->launch_frames(e->stream, d_indices, count, d_rgb, width, height);
    PG_HIP(hipGetLastError());
    return 0;
}

int32_t pgv_render_frames_host(pgv_env* e, const int32_t* h_indices, int32_t count, int32_t width, int32_t height,
                               uint8_t* h_rgb) {
    if (!e) return fail("pgv_render_frames_host: env is NULL");
    if (count < 0) return fail("pgv_render_frames_host: count is negative");
    if (width < 1 || height < 1 || width > 4096 || height > 4096 || !h_rgb)
        return fail("pgv_render_frames_host: bad frame size or NULL buffer");
    if (count == 0) return 0;
    PG_HIP(hipSetDevice(e->device));
    const size_t bytes = size_t(count) * size_t(height) * size_t(width) * 3;
    pg::Staged dev{e->stream};
    uint8_t* d_rgb = dev.alloc<uint8_t>(bytes);
    const int32_t* d_indices = h_indices ? dev.alloc(size_t(count), h_indices) : nullptr;
    if (dev.err == hipSuccess) {
        if (const int32_t rc = pgv_render_frames(e, d_indices, count, width, height, d_rgb)) return rc;
        dev.fetch(h_rgb, d_rgb, bytes);
    }
    if (dev.err != hipSuccess) return fail(std::string("pgv_render_frames_host: ") + hipGetErrorString(dev.err));
    return 0;
}

int32_t pgv_set_debug(pgv_env* e, int32_t flags) {
    if (!e) return fail("pgv_set_debug: env is NULL");
#ifndef PG_ABLATE
    if (flags & ~(1 | pg::kDebugNoPrefetch | pg::kDebugNoPrepass | pg::kDebugFatThirds | pg::kDebugCoinrunNoReach | pg::kDebugChaserSerialMobs | pg::kDebugPolicyStrided | pg::kDebugFatInPlace))
        return fail("pgv_set_debug: only bit 0 (draw-list replay), bit 8 (no level prefetch), bit 21 (no render pre-pass), bit 23 (every third frame by the complete path), bit 24 (coinrun: hazards the long way), bit 25 (chaser: enemies the long way), bit 26 (policy observations: lane-strided stores) and bit 27 (coinrun: handed-back frames in their own blocks) exist in this build");
#endif
    if (e->side) hipStreamSynchronize(e->side);
    e->game->debug_flags = flags;
    return 0;
}

// The debug taps: one env's row through the launches behind pgv_state_rows / pgv_tile_rows into the engine's tap buffer,
// and as much of it out as `cap` allows.  On the env's stream and no other: nothing is allocated or freed here, so a tap
// waits neither for the level generator's stream nor for the reset stream.
namespace pg {
static int32_t tap_failed(const char* who, hipError_t err) {
    g_error = std::string(who) + ": " + hipGetErrorString(err);
    return -1;
}
}  // namespace pg

int32_t pgv_dump_state(pgv_env* e, int32_t index, float* h_out, int32_t cap) {
    if (!e || index < 0 || index >= e->n) return -1;
    const pg::TapBuffers& t = e->tap;
    int32_t length = 0;
    hipError_t err = hipSetDevice(e->device);
    if (err == hipSuccess) err = hipMemsetD32Async(t.index, index, 1, e->stream);
    if (err == hipSuccess) {
        e->game->launch_state_rows(e->stream, t.index, 1, t.row, t.length);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipMemcpyAsync(&length, t.length, 4, hipMemcpyDeviceToHost, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    const int32_t m = std::min(cap, length);
    if (err == hipSuccess && m > 0 && h_out) err = hipMemcpy(h_out, t.row, size_t(m) * 4, hipMemcpyDeviceToHost);
    return err == hipSuccess ? length : pg::tap_failed("pgv_dump_state", err);
}

int32_t pgv_dump_tiles(pgv_env* e, int32_t index, uint8_t* h_out, int32_t cap) {
    if (!e || index < 0 || index >= e->n) return -1;
    const pg::TapBuffers& t = e->tap;
    const int32_t m = h_out ? std::min(cap, t.cells) : 0;
    hipError_t err = hipSetDevice(e->device);
    if (m > 0) {
        if (err == hipSuccess) err = hipMemsetD32Async(t.index, index, 1, e->stream);
        if (err == hipSuccess) {
            e->game->launch_tile_rows(e->stream, t.index, 1, t.tiles);
            err = hipGetLastError();
        }
    }
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    if (err == hipSuccess && m > 0) err = hipMemcpy(h_out, t.tiles, size_t(m), hipMemcpyDeviceToHost);
    return err == hipSuccess ? t.cells : pg::tap_failed("pgv_dump_tiles", err);
}

// ------------------------------------------------------------------------------------------------
// Symbolic observations (include/procgen2_vec.h; pg_state_obs.h and every game's StateRow).
// ------------------------------------------------------------------------------------------------
namespace pg {
// A Game fresh from its factory answers for its layout: host only, nothing bound, no GPU.
static std::unique_ptr<Game> layout_game(const char* who, int32_t game_id, int32_t mode) {
    if (game_id < 0 || game_id >= kNumGames) {
        fail(std::string(who) + ": unknown game id " + std::to_string(game_id));
        return nullptr;
    }
    const Variant* variant = find_variant(game_id, mode);
    if (!variant) {
        fail(std::string(who) + ": game '" + kGameNames[game_id] + "' has no distribution mode " + std::to_string(mode) +
             " (see pgv_game_modes)");
        return nullptr;
    }
    return variant->make();
}
}  // namespace pg

int32_t pgv_state_layout_of(int32_t game_id, int32_t mode, pgv_state_layout* out) {
    if (!out || out->struct_size < sizeof(pgv_state_layout)) return fail("pgv_state_layout_of: out is NULL or struct_size too small");
    const std::unique_ptr<pg::Game> game = pg::layout_game("pgv_state_layout_of", game_id, mode);
    if (!game) return 1;
    const pg::StateLayout l = game->state_layout();
    out->width = l.width, out->fixed = l.fixed, out->record = l.record, out->max_records = l.max_records;
    out->cells = l.cells, out->tile_w = l.tile_w, out->tile_h = l.tile_h;
    return 0;
}

int64_t pgv_state_names(int32_t game_id, int32_t mode, char* buf, int64_t cap) {
    const std::unique_ptr<pg::Game> game = pg::layout_game("pgv_state_names", game_id, mode);
    if (!game) return -1;
    const std::string names = game->state_names();
    if (buf && cap > 0) {
        const size_t m = std::min(names.size(), static_cast<size_t>(cap - 1));
        std::memcpy(buf, names.data(), m);
        buf[m] = 0;
    }
    return static_cast<int64_t>(names.size());
}

int32_t pgv_state_rows(pgv_env* e, const int32_t* d_indices, int32_t count, float* d_rows, int32_t* d_lengths) {
    if (!e) return fail("pgv_state_rows: env is NULL");
    if (count < 0) return fail("pgv_state_rows: count is negative");
    if (count == 0) return 0;
    if (!d_rows) return fail("pgv_state_rows: the output buffer is NULL");
    if (reinterpret_cast<uintptr_t>(d_rows) % 16) return fail("pgv_state_rows: d_rows is not 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_lengths) % 4) return fail("pgv_state_rows: d_lengths is not 4-byte aligned");
    PG_HIP(hipSetDevice(e->device));
    e->game->launch_state_rows(e->stream, d_indices, count, d_rows, d_lengths);
    PG_HIP(hipGetLastError());
    return 0;
}

int32_t pgv_tile_rows(pgv_env* e, const int32_t* d_indices, int32_t count, uint8_t* d_tiles) {
    if (!e) return fail("pgv_tile_rows: env is NULL");
    if (count < 0) return fail("pgv_tile_rows: count is negative");
    if (e->game->state_layout().cells == 0 || count == 0) return 0;  // (a game without a tile map: nothing to write)
    if (!d_tiles) return fail("pgv_tile_rows: the output buffer is NULL");
    if (reinterpret_cast<uintptr_t>(d_tiles) % 16) return fail("pgv_tile_rows: d_tiles is not 16-byte aligned");
    PG_HIP(hipSetDevice(e->device));
    e->game->launch_tile_rows(e->stream, d_indices, count, d_tiles);
    PG_HIP(hipGetLastError());
    return 0;
}

int32_t pgv_state_rows_host(pgv_env* e, const int32_t* h_indices, int32_t count, float* h_rows, int32_t* h_lengths) {
    if (!e) return fail("pgv_state_rows_host: env is NULL");
    if (count < 0) return fail("pgv_state_rows_host: count is negative");
    if (count == 0) return 0;
    if (!h_rows) return fail("pgv_state_rows_host: the output buffer is NULL");
    PG_HIP(hipSetDevice(e->device));
    const size_t floats = size_t(count) * size_t(e->game->state_layout().width);
    pg::Staged dev{e->stream};
    float* d_rows = dev.alloc<float>(floats);
    int32_t* d_lengths = h_lengths ? dev.alloc<int32_t>(size_t(count)) : nullptr;
    const int32_t* d_indices = h_indices ? dev.alloc(size_t(count), h_indices) : nullptr;
    if (dev.err == hipSuccess) {
        if (const int32_t rc = pgv_state_rows(e, d_indices, count, d_rows, d_lengths)) return rc;
        dev.fetch(h_rows, d_rows, floats * 4);
        if (h_lengths) dev.fetch(h_lengths, d_lengths, size_t(count) * 4);
    }
    if (dev.err != hipSuccess) return fail(std::string("pgv_state_rows_host: ") + hipGetErrorString(dev.err));
    return 0;
}

int32_t pgv_tile_rows_host(pgv_env* e, const int32_t* h_indices, int32_t count, uint8_t* h_tiles) {
    if (!e) return fail("pgv_tile_rows_host: env is NULL");
    if (count < 0) return fail("pgv_tile_rows_host: count is negative");
    const size_t bytes = size_t(count > 0 ? count : 0) * size_t(e->game->state_layout().cells);
    if (bytes == 0) return 0;
    if (!h_tiles) return fail("pgv_tile_rows_host: the output buffer is NULL");
    PG_HIP(hipSetDevice(e->device));
    pg::Staged dev{e->stream};
    uint8_t* d_tiles = dev.alloc<uint8_t>(bytes);
    const int32_t* d_indices = h_indices ? dev.alloc(size_t(count), h_indices) : nullptr;
    if (dev.err == hipSuccess) {
        if (const int32_t rc = pgv_tile_rows(e, d_indices, count, d_tiles)) return rc;
        dev.fetch(h_tiles, d_tiles, bytes);
    }
    if (dev.err != hipSuccess) return fail(std::string("pgv_tile_rows_host: ") + hipGetErrorString(dev.err));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Path distances (include/procgen2_vec.h; pg_paths.h and every tile game's PathRow).
// ------------------------------------------------------------------------------------------------
int32_t pgv_path_layout_of(int32_t game_id, int32_t mode, pgv_path_layout* out) {
    if (!out || out->struct_size < sizeof(pgv_path_layout)) return fail("pgv_path_layout_of: out is NULL or struct_size too small");
    const std::unique_ptr<pg::Game> game = pg::layout_game("pgv_path_layout_of", game_id, mode);
    if (!game) return 1;
    const pg::StateLayout l = game->state_layout();
    const pg::PathPoints p = game->path_points();
    out->cells = l.cells, out->tile_w = l.tile_w, out->tile_h = l.tile_h;
    out->has_goal = p.has_goal ? 1 : 0, out->agent_dx = p.agent_dx, out->agent_dy = p.agent_dy;
    return 0;
}

namespace pg {
// Points 8 of the path distances that do not depend on where the pointers live: nullptr, or why the call is refused.
static const char* tile_paths_error(const pgv_env* e, int32_t count, const pgv_tile_paths* p) {
    if (!e) return "env is NULL";
    if (!p) return "the pgv_tile_paths struct is NULL";
    if (p->struct_size < sizeof(pgv_tile_paths)) return "struct_size is too small";
    if (count < 0) return "count is negative";
    if (e->game->state_layout().cells == 0) return "this game has no tile map";
    if (p->source != PGV_PATH_AGENT && p->source != PGV_PATH_GOAL && p->source != PGV_PATH_CELLS)
        return "source must be PGV_PATH_AGENT, PGV_PATH_GOAL or PGV_PATH_CELLS";
    if (p->probe != PGV_PATH_NONE && p->probe != PGV_PATH_AGENT && p->probe != PGV_PATH_GOAL && p->probe != PGV_PATH_CELLS)
        return "unknown probe";
    if ((p->source == PGV_PATH_GOAL || p->probe == PGV_PATH_GOAL) && !e->game->path_points().has_goal)
        return "PGV_PATH_GOAL: this game has no goal";
    if (count > 0 && p->source == PGV_PATH_CELLS && !p->source_cells) return "source_cells is NULL";
    if (count > 0 && p->probe == PGV_PATH_CELLS && !p->probe_cells) return "probe_cells is NULL";
    if (count > 0 && !p->dist && !p->probe_dist && !p->probe_step && !p->cells_out) return "every output is NULL";
    return nullptr;
}
}  // namespace pg

int32_t pgv_tile_paths_rows(pgv_env* e, const int32_t* d_indices, int32_t count, const pgv_tile_paths* p) {
    if (const char* why = pg::tile_paths_error(e, count, p)) return fail(std::string("pgv_tile_paths_rows: ") + why);
    if (reinterpret_cast<uintptr_t>(p->dist) % 16) return fail("pgv_tile_paths_rows: dist is not 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(p->probe_dist) % 4) return fail("pgv_tile_paths_rows: probe_dist is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(p->cells_out) % 4) return fail("pgv_tile_paths_rows: cells_out is not 4-byte aligned");
    if (count == 0) return 0;
    PG_HIP(hipSetDevice(e->device));
    pg::TilePaths q{};
    q.passable = p->passable, q.source = p->source, q.probe = p->probe;
    q.source_cells = p->source_cells, q.probe_cells = p->probe_cells;
    q.dist = p->dist, q.probe_dist = p->probe_dist, q.probe_step = p->probe_step, q.cells_out = p->cells_out;
    q.indices = d_indices, q.count = count;
    e->game->launch_tile_paths(e->stream, q);
    PG_HIP(hipGetLastError());
    return 0;
}

int32_t pgv_tile_paths_rows_host(pgv_env* e, const int32_t* h_indices, int32_t count, const pgv_tile_paths* p) {
    if (const char* why = pg::tile_paths_error(e, count, p)) return fail(std::string("pgv_tile_paths_rows_host: ") + why);
    if (count == 0) return 0;
    PG_HIP(hipSetDevice(e->device));
    const size_t rows = size_t(count), dists = rows * size_t(e->game->state_layout().cells);
    pg::Staged dev{e->stream};
    pgv_tile_paths d = *p;
    d.source_cells = p->source == PGV_PATH_CELLS ? dev.alloc(rows, p->source_cells) : nullptr;
    d.probe_cells = p->probe == PGV_PATH_CELLS ? dev.alloc(rows, p->probe_cells) : nullptr;
    d.dist = p->dist ? dev.alloc<int16_t>(dists) : nullptr;
    d.probe_dist = p->probe_dist ? dev.alloc<int32_t>(rows) : nullptr;
    d.probe_step = p->probe_step ? dev.alloc<uint8_t>(rows) : nullptr;
    d.cells_out = p->cells_out ? dev.alloc<int32_t>(rows * 2) : nullptr;
    const int32_t* d_indices = h_indices ? dev.alloc(rows, h_indices) : nullptr;
    if (dev.err == hipSuccess) {
        if (const int32_t rc = pgv_tile_paths_rows(e, d_indices, count, &d)) return rc;
        if (p->dist) dev.fetch(p->dist, d.dist, dists * 2);
        if (p->probe_dist) dev.fetch(p->probe_dist, d.probe_dist, rows * 4);
        if (p->probe_step) dev.fetch(p->probe_step, d.probe_step, rows);
        if (p->cells_out) dev.fetch(p->cells_out, d.cells_out, rows * 8);
    }
    if (dev.err != hipSuccess) return fail(std::string("pgv_tile_paths_rows_host: ") + hipGetErrorString(dev.err));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Caller-made levels (include/procgen2_vec.h; pg_levels.h and maze's Custom).
// ------------------------------------------------------------------------------------------------
int32_t pgv_level_layout_of(int32_t game_id, int32_t mode, pgv_level_layout* out) {
    if (!out || out->struct_size < sizeof(pgv_level_layout)) return fail("pgv_level_layout_of: out is NULL or struct_size too small");
    const std::unique_ptr<pg::Game> game = pg::layout_game("pgv_level_layout_of", game_id, mode);
    if (!game) return 1;
    const pg::LevelLayout l = game->level_layout();
    out->supported = l.supported, out->cells = l.cells, out->tile_w = l.tile_w, out->tile_h = l.tile_h, out->backgrounds = l.backgrounds;
    return 0;
}

namespace pg {
// The host's refusals that do not depend on where the pointers live: nullptr, or why the call is refused.
static const char* level_rows_error(const pgv_env* e, int32_t count, const pgv_level_rows* rows, bool install) {
    if (!e) return "env is NULL";
    if (!rows) return "the pgv_level_rows struct is NULL";
    if (rows->struct_size < sizeof(pgv_level_rows)) return "struct_size is too small";
    if (count < 0) return "count is negative";
    if (!e->game->level_layout().supported) return "no caller-made levels for this game";
    if (install && count > 0 && !rows->tiles) return "tiles is NULL";
    if (install && count > 0 && !rows->agent_cell) return "agent_cell is NULL";
    if (install && count > 0 && !rows->goal_cell) return "goal_cell is NULL";
    return nullptr;
}
static const char* level_rows_misaligned(const pgv_level_rows* rows) {
    for (auto [p, name] : {std::pair<const void*, const char*>{rows->agent_cell, "agent_cell"}, {rows->goal_cell, "goal_cell"},
                           {rows->background, "background"}, {rows->background_shift, "background_shift"}, {rows->ids, "ids"},
                           {rows->status, "status"}})
        if (reinterpret_cast<uintptr_t>(p) % 4) return name;
    return nullptr;
}
static LevelRows level_rows(const int32_t* d_indices, int32_t count, const pgv_level_rows* r) {
    return LevelRows{d_indices, count, r->tiles, r->agent_cell, r->goal_cell, r->background, r->background_shift, r->ids, r->status};
}
}  // namespace pg

int32_t pgv_get_levels(pgv_env* e, const int32_t* d_indices, int32_t count, const pgv_level_rows* out) {
    if (const char* why = pg::level_rows_error(e, count, out, false)) return fail(std::string("pgv_get_levels: ") + why);
    if (const char* name = pg::level_rows_misaligned(out)) return fail(std::string("pgv_get_levels: ") + name + " is not 4-byte aligned");
    if (count == 0) return 0;
    PG_HIP(hipSetDevice(e->device));
    e->game->launch_get_levels(e->stream, pg::level_rows(d_indices, count, out));
    PG_HIP(hipGetLastError());
    return 0;
}

int32_t pgv_set_levels(pgv_env* e, const int32_t* d_indices, int32_t count, const pgv_level_rows* in) {
    if (const char* why = pg::level_rows_error(e, count, in, true)) return fail(std::string("pgv_set_levels: ") + why);
    if (const char* name = pg::level_rows_misaligned(in)) return fail(std::string("pgv_set_levels: ") + name + " is not 4-byte aligned");
    if (count == 0) return 0;
    if (slab_ready("pgv_set_levels", e)) return 1;
    PG_HIP(hipSetDevice(e->device));
    (void)hipGetLastError();
    // The install writes the live state, the engine's rows and the level words of the envs it names, all of them the env's
    // stream's: the generator's side stream reads and writes the shadow slots, the chains and the slot words alone, so there
    // is nothing to order against it (a reset waits for it through the slot word it consumes; an install consumes none).
    PG_HIP(hipMemsetAsync(e->d_levels, 0, pg::Carve::size(pg::list_levels, e->n), e->stream));
    pg::LevelInstall to{e->n, e->d_reward, e->d_done, e->d_pending, e->game->plan.number, e->game->plan.known, e->lev.claim, e->lev.mask};
    e->game->launch_set_levels(e->stream, pg::level_rows(d_indices, count, in), to);
    PG_HIP(hipGetLastError());
    return reset_shows("pgv_set_levels", e, e->lev.mask, false);
}

int32_t pgv_get_levels_host(pgv_env* e, const int32_t* h_indices, int32_t count, const pgv_level_rows* out) {
    if (const char* why = pg::level_rows_error(e, count, out, false)) return fail(std::string("pgv_get_levels_host: ") + why);
    if (count == 0) return 0;
    PG_HIP(hipSetDevice(e->device));
    const size_t rows = size_t(count), bytes = rows * size_t(e->game->level_layout().cells);
    pg::Staged dev{e->stream};
    pgv_level_rows d = *out;
    d.tiles = out->tiles ? dev.alloc<uint8_t>(bytes) : nullptr;
    d.agent_cell = out->agent_cell ? dev.alloc<int32_t>(rows) : nullptr;
    d.goal_cell = out->goal_cell ? dev.alloc<int32_t>(rows) : nullptr;
    d.background = out->background ? dev.alloc<int32_t>(rows) : nullptr;
    d.background_shift = out->background_shift ? dev.alloc<float>(rows) : nullptr;
    d.ids = nullptr, d.status = nullptr;
    const int32_t* d_indices = h_indices ? dev.alloc(rows, h_indices) : nullptr;
    if (dev.err == hipSuccess) {
        if (const int32_t rc = pgv_get_levels(e, d_indices, count, &d)) return rc;
        if (out->tiles) dev.fetch(out->tiles, d.tiles, bytes);
        if (out->agent_cell) dev.fetch(out->agent_cell, d.agent_cell, rows * 4);
        if (out->goal_cell) dev.fetch(out->goal_cell, d.goal_cell, rows * 4);
        if (out->background) dev.fetch(out->background, d.background, rows * 4);
        if (out->background_shift) dev.fetch(out->background_shift, d.background_shift, rows * 4);
    }
    if (dev.err != hipSuccess) return fail(std::string("pgv_get_levels_host: ") + hipGetErrorString(dev.err));
    return 0;
}

int32_t pgv_set_levels_host(pgv_env* e, const int32_t* h_indices, int32_t count, const pgv_level_rows* in) {
    if (const char* why = pg::level_rows_error(e, count, in, true)) return fail(std::string("pgv_set_levels_host: ") + why);
    if (count == 0) return 0;
    if (slab_ready("pgv_set_levels_host", e)) return 1;
    PG_HIP(hipSetDevice(e->device));
    const size_t rows = size_t(count), bytes = rows * size_t(e->game->level_layout().cells);
    pg::Staged dev{e->stream};
    pgv_level_rows d = *in;
    d.tiles = dev.alloc(bytes, in->tiles);
    d.agent_cell = dev.alloc(rows, in->agent_cell);
    d.goal_cell = dev.alloc(rows, in->goal_cell);
    d.background = in->background ? dev.alloc(rows, in->background) : nullptr;
    d.background_shift = in->background_shift ? dev.alloc(rows, in->background_shift) : nullptr;
    d.ids = in->ids ? dev.alloc(rows, in->ids) : nullptr;
    d.status = in->status ? dev.alloc<int32_t>(rows) : nullptr;
    const int32_t* d_indices = h_indices ? dev.alloc(rows, h_indices) : nullptr;
    if (dev.err == hipSuccess) {
        if (const int32_t rc = pgv_set_levels(e, d_indices, count, &d)) return rc;
        if (in->status) dev.fetch(in->status, d.status, rows * 4);
        dev.finish();  // (the host buffers are the caller's)
    }
    if (dev.err != hipSuccess) return fail(std::string("pgv_set_levels_host: ") + hipGetErrorString(dev.err));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// cenv ABI (include/procgen2_cenv.h) on top of one process-global vector env.
// ------------------------------------------------------------------------------------------------
cenv_make_data make_data;
cenv_reset_data reset_data;
cenv_step_data step_data;
cenv_render_data render_data;

}  // extern "C"

namespace {

struct CenvGlobal {
    pgv_env* env = nullptr;
    int n = 0;
    int window_w = 512, window_h = 512;  // coinrun.cpp:29-30
    cenv_key_value obs_space{}, act_space{};
    cenv_key_value observations[3]{};
    float box_bounds[2] = {0.0f, 255.0f};
    int32_t nvec[1] = {pg::kNumActions};
    std::vector<uint8_t> h_obs, h_done, h_frame;
    std::vector<float> h_reward;
    int32_t* d_actions = nullptr;
    int32_t* d_seeds = nullptr;
    std::vector<int32_t> h_actions;
};
CenvGlobal g;

const int kVersion = 100;  // coinrun.cpp:9

int opt_int(const cenv_option& o, int* out) {
    if (o.value_type == CENV_VALUE_TYPE_INT) {
        *out = o.value.i;
        return 0;
    }
    if (o.value_type == CENV_VALUE_TYPE_DOUBLE) {  // python float → DOUBLE (cenv.py:39-42)
        *out = static_cast<int>(o.value.d);
        return 0;
    }
    return 1;
}

void publish_results(bool from_step) {
    pgv_copy_out(g.env, g.h_obs.data(), g.h_reward.data(), g.h_done.data());
    if (from_step) {
        double sum = 0.0;
        bool all = true;
        for (int i = 0; i < g.n; i++) {
            sum += g.h_reward[i];
            all = all && g.h_done[i];
        }
        step_data.reward.f = static_cast<float>(g.n == 1 ? g.h_reward[0] : sum / g.n);
        step_data.terminated = g.n == 1 ? (g.h_done[0] != 0) : all;
        step_data.truncated = false;
    }
}

}  // namespace

extern "C" {

int32_t cenv_get_env_version(void) { return kVersion; }

int32_t cenv_make(const char* render_mode, cenv_option* options, int32_t options_size) {
    (void)render_mode;
    if (g.env) cenv_close();
    g.window_w = g.window_h = 512;               // coinrun.cpp:29-30; a previous make's size does not carry over
    int seed = static_cast<int>(time(nullptr));  // coinrun.cpp:130
    int num_envs = 1, game = PG_DEFAULT_GAME, device = 0, env_offset = 0, num_levels = 0, start_level = 0, mode = 0, game_flags = 0;
    for (int i = 0; i < options_size; i++) {
        const std::string name(options[i].name ? options[i].name : "");
        int v = 0;
        if (name == "seed" || name == "width" || name == "height" || name == "num_envs" || name == "game" ||
            name == "device" || name == "env_offset" || name == "num_levels" || name == "start_level" ||
            name == "distribution_mode" || name == "game_flags") {
            if (opt_int(options[i], &v)) return fail("cenv_make: option '" + name + "' must be INT");
        }
        if (name == "seed")
            seed = v;
        else if (name == "width")
            g.window_w = v;
        else if (name == "height")
            g.window_h = v;
        else if (name == "num_envs")
            num_envs = v;
        else if (name == "game")
            game = v;
        else if (name == "device")
            device = v;
        else if (name == "env_offset")
            env_offset = v;
        else if (name == "num_levels")
            num_levels = v;
        else if (name == "start_level")
            start_level = v;
        else if (name == "distribution_mode")
            mode = v;
        else if (name == "game_flags")
            game_flags = v;
    }
    const char* gname = pgv_game_name(game);
    if (!gname) return fail("cenv_make: unknown game id");
    pgv_config cfg{};
    cfg.struct_size = sizeof(pgv_config);
    cfg.game = gname;
    cfg.num_envs = num_envs;
    cfg.device = device;
    cfg.seed_base = static_cast<uint32_t>(seed);
    cfg.env_offset = env_offset;
    cfg.num_levels = num_levels;
    cfg.start_level = start_level;
    cfg.mode = mode;
    cfg.game_flags = static_cast<uint32_t>(game_flags);
    int rc = pgv_make_config(&cfg, &g.env);
    if (rc) return rc;
    g.n = num_envs;
    g.h_obs.assign(size_t(num_envs) * pg::kObsBytes, 0);
    g.h_reward.assign(num_envs, 0.0f);
    g.h_done.assign(num_envs, 0);
    g.h_actions.assign(num_envs, 0);
    g.h_frame.assign(size_t(g.window_w) * g.window_h * 3, 0);
    if (hipMalloc(reinterpret_cast<void**>(&g.d_actions), size_t(num_envs) * 4) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&g.d_seeds), size_t(num_envs) * 4) != hipSuccess) {
        cenv_close();
        return fail("cenv_make: hipMalloc failed");
    }

    // Spaces (coinrun.cpp:154-172): "screen" Box(0,255), "action" MultiDiscrete([15]).
    g.obs_space.key = "screen";
    g.obs_space.value_type = CENV_SPACE_TYPE_BOX;
    g.obs_space.value_buffer_size = 2;
    g.obs_space.value_buffer.f = g.box_bounds;
    g.act_space.key = "action";
    g.act_space.value_type = CENV_SPACE_TYPE_MULTI_DISCRETE;
    g.act_space.value_buffer_size = 1;
    g.act_space.value_buffer.i = g.nvec;
    make_data.observation_spaces_size = 1;
    make_data.observation_spaces = &g.obs_space;
    make_data.action_spaces_size = 1;
    make_data.action_spaces = &g.act_space;

    g.observations[0].key = "screen";
    g.observations[0].value_type = CENV_VALUE_TYPE_BYTE;
    g.observations[0].value_buffer_size = num_envs * pg::kObsBytes;
    g.observations[0].value_buffer.b = g.h_obs.data();
    g.observations[1].key = "reward";
    g.observations[1].value_type = CENV_VALUE_TYPE_FLOAT;
    g.observations[1].value_buffer_size = num_envs;
    g.observations[1].value_buffer.f = g.h_reward.data();
    g.observations[2].key = "terminated";
    g.observations[2].value_type = CENV_VALUE_TYPE_BYTE;
    g.observations[2].value_buffer_size = num_envs;
    g.observations[2].value_buffer.b = g.h_done.data();
    const int nobs = num_envs == 1 ? 1 : 3;
    reset_data.observations_size = nobs;
    reset_data.observations = g.observations;
    reset_data.infos_size = 0;
    reset_data.infos = nullptr;
    step_data.observations_size = nobs;
    step_data.observations = g.observations;
    step_data.reward.f = 0.0f;
    step_data.terminated = false;
    step_data.truncated = false;
    step_data.infos_size = 0;
    step_data.infos = nullptr;
    render_data.value_type = CENV_VALUE_TYPE_BYTE;
    render_data.value_buffer_width = g.window_w;
    render_data.value_buffer_height = g.window_h;
    render_data.value_buffer_channels = 3;
    render_data.value_buffer.b = g.h_frame.data();
    return 0;
}

int32_t cenv_reset(cenv_option* options, int32_t options_size) {
    if (!g.env) return fail("cenv_reset: cenv_make has not been called");
    const int32_t* seeds = nullptr;
    for (int i = 0; i < options_size; i++) {
        const std::string name(options[i].name ? options[i].name : "");
        if (name == "seed") {
            int v = 0;
            if (opt_int(options[i], &v)) return fail("cenv_reset: option 'seed' must be INT");
            for (int k = 0; k < g.n; k++) g.h_actions[k] = v + k;
            if (hipMemcpy(g.d_seeds, g.h_actions.data(), size_t(g.n) * 4, hipMemcpyHostToDevice) != hipSuccess)
                return fail("cenv_reset: seed upload failed");
            seeds = g.d_seeds;
        }
    }
    int rc = pgv_reset(g.env, nullptr, seeds);
    if (rc) return rc;
    publish_results(false);
    return 0;
}

int32_t cenv_step(cenv_key_value* actions, int32_t actions_size) {
    if (!g.env) return fail("cenv_step: cenv_make has not been called");
    for (int k = 0; k < g.n; k++) g.h_actions[k] = 0;  // `int action = 0;` (coinrun.cpp:342)
    for (int i = 0; i < actions_size; i++) {
        if (!actions[i].key || std::strcmp(actions[i].key, "action")) continue;
        if (actions[i].value_type != CENV_VALUE_TYPE_INT) return fail("cenv_step: 'action' must be INT");
        const int m = actions[i].value_buffer_size < g.n ? actions[i].value_buffer_size : g.n;
        for (int k = 0; k < m; k++) g.h_actions[k] = actions[i].value_buffer.i[k];
    }
    if (hipMemcpy(g.d_actions, g.h_actions.data(), size_t(g.n) * 4, hipMemcpyHostToDevice) != hipSuccess)
        return fail("cenv_step: action upload failed");
    if (g.n == 1) {
        // Reference semantics: no auto-reset — stepping a terminated env keeps stepping it.  The vector
        // engine's pending flag is cleared so the single-env path never resets on its own.
        uint8_t zero = 0;
        hipMemcpy(g.env->d_pending, &zero, 1, hipMemcpyHostToDevice);
    }
    int rc = pgv_step(g.env, g.d_actions);
    if (rc) return rc;
    publish_results(true);
    return 0;
}

int32_t cenv_render(void) {
    // Human-size frame (coinrun.cpp:393-411): render_game(false) of env 0 on the GPU (pg_frame.h).
    if (!g.env) return fail("cenv_render: cenv_make has not been called");
    if (pgv_render_frame(g.env, 0, g.window_w, g.window_h, g.h_frame.data()) == 0) return 0;
    // a game without a frame kernel: the 64×64 observation of env 0, nearest-neighbour enlarged
    for (int y = 0; y < g.window_h; y++)
        for (int x = 0; x < g.window_w; x++) {
            const int sx = x * pg::kObsW / g.window_w, sy = y * pg::kObsH / g.window_h;
            for (int c = 0; c < 3; c++) g.h_frame[c + 3 * (x + g.window_w * y)] = g.h_obs[c + 3 * (sx + pg::kObsW * sy)];
        }
    return 0;
}

void cenv_close(void) {
    if (!g.env) return;
    if (g.d_actions) hipFree(g.d_actions);
    if (g.d_seeds) hipFree(g.d_seeds);
    g.d_actions = g.d_seeds = nullptr;
    pgv_close(g.env);
    g.env = nullptr;
}

}  // extern "C"
