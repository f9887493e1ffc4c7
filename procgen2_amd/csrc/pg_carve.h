// Device memory listed once (Carve), and the engine's level plan listed with it.  No HIP: g++ compiles it for the CPU tests.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace pg {

// The per-env regions of a state block, as its listing describes them (Carve, below).
struct EnvRegion {
    uint8_t* base;
    uint32_t pieces, piece_bytes;  // F, E
};
struct EnvRegions {
    std::vector<EnvRegion> v;
    size_t shared_bytes = 0, unlisted_bytes = 0;  // (rounded, as they lie in the block)
};

// A block of device memory listed as consecutive regions, each rounded up to 256 bytes (or to `align`).  A game writes
// its listing once, as a function list(c, s, n) that takes every region into a pointer of s; run without a base it only
// adds up the bytes (state_bytes, scratch_bytes), with one it also hands out the addresses (bind, bind_scratch), so the
// size and the binding cannot disagree.  A region of no bytes gets nullptr.  A listing whose sizes depend on more than n
// reads them from s (pg_episodes.h list_episodes: the ring's capacity): size() then starts from a copy of the caller's.
//
// A STATE listing also says which regions are per env and what an env's share of one looks like: take_env(p, n, F, E) is
// a region of n·F·E bytes in which env i owns F pieces of E bytes at  base + f·n·E + i·E  — F = 1 for an env-major block
// (`mt`, `tiles`, a shadow level), E = 4 or 1 and F = the field count for struct-of-arrays fields; take_shared is a
// region the whole engine has once (a list, a counter, a prepared table).  Bound with a table (third mode: describe), the
// listing leaves the per-env regions there: what one env's record is gathered from and scattered to (pg_records.h).  A
// plain take() in a state listing is counted as unlisted, and pgv_make refuses an engine whose table has any: a region
// somebody adds later must say what it is, or it would silently drop out of the records.
struct Carve {
    uint8_t* base = nullptr;
    size_t bytes = 0;
    EnvRegions* table = nullptr;
    template <class T>
    void take(T*& p, size_t len, size_t align = 256) {
        const size_t before = bytes;
        place(p, len, align);
        if (table) table->unlisted_bytes += bytes - before;
    }
    template <class T>
    void take_env(T*& p, int n, size_t pieces, size_t piece_bytes, size_t align = 256) {
        const size_t at = bytes;
        place(p, size_t(n) * pieces * piece_bytes, align);
        if (table) table->v.push_back({base + at, static_cast<uint32_t>(pieces), static_cast<uint32_t>(piece_bytes)});
    }
    template <class T>
    void take_shared(T*& p, size_t len) {
        const size_t before = bytes;
        place(p, len, 256);
        if (table) table->shared_bytes += bytes - before;
    }
    template <class S>
    static size_t size(void (*list)(Carve&, S&, int), int n, S s = S{}) {
        Carve c;
        list(c, s, n);
        return c.bytes;
    }
    template <class S>
    static void bind(void (*list)(Carve&, S&, int), void* base, S& s, int n, EnvRegions* table = nullptr) {
        Carve c{static_cast<uint8_t*>(base)};
        if (table) *table = EnvRegions{};
        c.table = table;
        list(c, s, n);
    }

   private:
    template <class T>
    void place(T*& p, size_t len, size_t align) {
        p = base && len ? reinterpret_cast<T*>(base + bytes) : nullptr;
        bytes += (len + align - 1) / align * align;
    }
};

// Level-seed mode (absent from the reference, modelled on the original procgen's
// num_levels / start_level).  num_levels = 0: the reference's behaviour — one RNG stream per env, every level is new.
// num_levels > 0: the k-th level an env builds since it was (re)seeded is level number
//     start_level + mix32(mix32(chain_seed) + k) % num_levels,
// and "level number L" means exactly what a fresh `cenv_make(seed = L)` builds as its level 0 — fresh containers,
// fresh camera, rng.seed(L) — so the same number always gives the same level, whatever the env played before.
struct LevelPlan {
    int32_t num_levels;    // 0 = off
    int32_t start_level;
    uint32_t* chain_seed;  // [n]  the seed the env was made / last reseeded with
    uint32_t* drawn;       // [n]  k: levels built since then
    // Assigned levels (include/procgen2_vec.h pgv_assign_levels): the caller names the number of the level an env builds
    // NEXT, in either mode; such a level takes no place in the env's own sequence (k stays).  One pending assignment per
    // env, consumed by whoever builds the level — the step's reset, an explicit reset without seeds, or the side-stream
    // generator, which then notes in the slot's two words what the shadow slot holds (pg_prefetch.h).
    uint32_t* assigned;       // [n]  the pending assignment's level number
    uint32_t* number;         // [n]  the number of the level the env is IN (pgv_level_numbers); 0 where it has none
    uint32_t* slot_number;    // [n]  … of the level in the env's shadow slot, where slot_assigned says it has one
    uint8_t* assigned_on;     // [n]  1: an assignment is pending
    uint8_t* known;           // [n]  1: `number` holds (level-seed mode, or an assigned level) (pgv_level_known)
    uint8_t* slot_assigned;   // [n]  1: the shadow slot's level was built from an assignment
    // Free mode with prefetch: an assigned level that the side stream builds ahead starts the env's generator chain afresh
    // while the env still plays its old level.  A reset WITH seeds that comes first drops the assignment and must find
    // the chain's containers as the env's own history left them, so the generator keeps their bucket counts as they
    // stood when the env's current level was built (pg_prefetch.h chain_keep) until the next level is installed.
    uint32_t* kept0;          // [n]  the chain's container counts as of the level the env is in (G::chain_counts) …
    uint32_t* kept1;          // [n]
    uint8_t* kept_on;         // [n]  … bit 0: they are held, bit 1: an assignment built ahead has replaced the chain since
};
// The arrays lie packed behind the game's state in the state blob (engine.hip state_blob_bytes), the words first: 32 bytes
// an env.  This order is the snapshot's format (kSnapshotMagic) and the order of the plan's regions in a record (pg_records.h).
inline void list_plan(Carve& c, LevelPlan& p, int n) {
    for (uint32_t** words : {&p.chain_seed, &p.drawn, &p.assigned, &p.number, &p.slot_number, &p.kept0, &p.kept1}) c.take_env(*words, n, 1, 4, 4);
    for (uint8_t** bytes : {&p.assigned_on, &p.known, &p.slot_assigned, &p.kept_on}) c.take_env(*bytes, n, 1, 1, 1);
}

}  // namespace pg
