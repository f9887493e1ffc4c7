// The engine's own device memory as its two listings lay it out (procgen2_amd/csrc/pg_carve.h list_plan, pg_episodes.h
// list_episodes), compiled for the CPU and held to offsets and sizes written out here as numbers: the level plan's eleven
// arrays behind a game's state are a snapshot's format, the episode block's seventeen buffers are what the kernels index.
// Prints "OK <section>" per section and "ALL OK"; exit status 1 on the first failure.
#include <cstdio>

#include "pg_episodes.h"

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            std::printf("FAILED %s:%d: %s (n = %d)\n", __FILE__, __LINE__, #cond, n);    \
            return 1;                                                                    \
        }                                                                                \
    } while (0)

static uint8_t* at(const void* p) { return static_cast<uint8_t*>(const_cast<void*>(p)); }

static int test_plan(int n) {
    const size_t N = size_t(n);
    uint8_t* const base = reinterpret_cast<uint8_t*>(uintptr_t(0x7000001000));  // (never dereferenced)
    pg::LevelPlan p{};
    p.num_levels = 5;
    p.start_level = 100;
    pg::EnvRegions table;
    pg::Carve::bind(pg::list_plan, base, p, n, &table);
    CHECK(p.num_levels == 5 && p.start_level == 100);  // binding leaves the scalars alone
    // seven word arrays, word array k at 4·k·n …
    CHECK(at(p.chain_seed) == base + 0 * N);
    CHECK(at(p.drawn) == base + 4 * N);
    CHECK(at(p.assigned) == base + 8 * N);
    CHECK(at(p.number) == base + 12 * N);
    CHECK(at(p.slot_number) == base + 16 * N);
    CHECK(at(p.kept0) == base + 20 * N);
    CHECK(at(p.kept1) == base + 24 * N);
    // … then four byte arrays, byte array j at 28·n + j·n
    CHECK(at(p.assigned_on) == base + 28 * N);
    CHECK(at(p.known) == base + 29 * N);
    CHECK(at(p.slot_assigned) == base + 30 * N);
    CHECK(at(p.kept_on) == base + 31 * N);
    CHECK(pg::Carve::size(pg::list_plan, n) == 32 * N);
    // described: eleven per-env regions of one piece each, in the order of memory, and nothing else
    static const uint32_t kPieceBytes[11] = {4, 4, 4, 4, 4, 4, 4, 1, 1, 1, 1};
    static const size_t kOffsetPerEnv[11] = {0, 4, 8, 12, 16, 20, 24, 28, 29, 30, 31};
    CHECK(table.v.size() == 11);
    for (int k = 0; k < 11; k++) {
        CHECK(table.v[k].pieces == 1);
        CHECK(table.v[k].piece_bytes == kPieceBytes[k]);
        CHECK(table.v[k].base == base + kOffsetPerEnv[k] * N);
    }
    CHECK(table.unlisted_bytes == 0 && table.shared_bytes == 0);
    // without a base: sizes only
    pg::LevelPlan q{};
    pg::Carve::bind(pg::list_plan, nullptr, q, n);
    CHECK(!q.chain_seed && !q.drawn && !q.assigned && !q.number && !q.slot_number && !q.kept0 && !q.kept1);
    CHECK(!q.assigned_on && !q.known && !q.slot_assigned && !q.kept_on);
    return 0;
}

static size_t r256(size_t bytes) { return (bytes + 255) / 256 * 256; }

static int test_episodes(int n, int capacity) {
    const size_t N = size_t(n);
    uint8_t* const base = reinterpret_cast<uint8_t*>(uintptr_t(0x7000000000));  // 256-byte aligned, as hipMalloc's
    pg::EpisodeBuffers b{};
    b.n = n;
    b.max_steps = 7;
    b.capacity = capacity;
    const size_t total = pg::Carve::size(pg::list_episodes, n, b);
    CHECK(b.capacity == capacity && !b.reward);  // sizing works on a copy
    pg::Carve::bind(pg::list_episodes, base, b, n);
    CHECK(b.n == n && b.max_steps == 7 && b.capacity == capacity);
    struct Buffer {
        const void* p;
        size_t bytes;
    };
    const Buffer order[17] = {{b.reward, 4 * N},         {b.terminated, N},
                              {b.truncated, N},          {b.ended, N},
                              {b.counts, 8},             {b.ended_env, 4 * N},
                              {b.ended_return, 4 * N},   {b.ended_length, 4 * N},
                              {b.ended_level, 4 * N},    {b.ended_level_known, N},
                              {b.running_return, 4 * N}, {b.running_length, 4 * N},
                              {b.prev_done, N},          {b.kept_return, 4 * N},
                              {b.kept_length, 4 * N},    {b.block_count, size_t((n + 255) / 256) * 4},
                              {b.final_obs, size_t(capacity) * 12288}};
    CHECK((b.final_obs == nullptr) == (capacity == 0));
    const int listed = capacity == 0 ? 16 : 17;  // (an empty ring has no address)
    CHECK(at(order[0].p) == base);
    for (int k = 0; k < listed; k++) {
        CHECK(order[k].p != nullptr);
        CHECK(reinterpret_cast<uintptr_t>(order[k].p) % 256 == 0);
        if (k > 0) CHECK(at(order[k].p) >= at(order[k - 1].p) + order[k - 1].bytes);
    }
    CHECK(at(order[listed - 1].p) + order[listed - 1].bytes <= base + total);
    CHECK(pg::episode_blocks(n) == (n + 255) / 256);
    // nine arrays of words, five of bytes, the two counts, a word per workgroup of 256 envs, the ring
    const size_t want = 9 * r256(4 * N) + 5 * r256(N) + r256(8) + r256(size_t(pg::episode_blocks(n)) * 4) + r256(size_t(capacity) * 12288);
    CHECK(total == want);
    return 0;
}

int main() {
    const int sizes[6] = {1, 63, 64, 65, 257, 65536};
    for (int n : sizes)
        if (test_plan(n)) return 1;
    std::printf("OK level plan\n");
    for (int n : sizes)
        for (int capacity : {0, 1, n})
            if (test_episodes(n, capacity)) return 1;
    std::printf("OK episode block\n");
    std::printf("ALL OK\n");
    return 0;
}
