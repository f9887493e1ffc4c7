// The per-env rule of the episode bookkeeping (procgen2_amd/csrc/pg_episodes.h episode_step) compiled for the CPU, and a
// host restatement of the ordered compaction its two kernels make — workgroup counts, bases, wave ballots, ranks — held
// to a plain ascending scan.  Prints "OK <section>" per section and "ALL OK"; exit status 1 on the first failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "pg_episodes.h"

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                   \
        }                                                               \
    } while (0)

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

static int test_truncation_boundary() {
    const int T = 23;
    for (int len : {T - 3, T - 2}) {  // the step makes it T-2 / T-1: below the limit
        const pg::EpisodeStep s = pg::episode_step(1.0f, len, 0.5f, 0, 0, T);
        CHECK(s.counted && !s.terminated && !s.truncated && !s.ended && s.len == len + 1 && s.ret == 1.5f);
    }
    {  // the T-th step
        const pg::EpisodeStep s = pg::episode_step(1.0f, T - 1, 0.5f, 0, 0, T);
        CHECK(s.counted && !s.terminated && s.truncated && s.ended && s.len == T);
    }
    {  // the T-th step terminates: terminated, not truncated
        const pg::EpisodeStep s = pg::episode_step(1.0f, T - 1, 10.0f, 1, 0, T);
        CHECK(s.terminated && !s.truncated && s.ended && s.len == T && s.ret == 11.0f);
    }
    {  // a running length written past the limit ends at its next step instead of running for ever
        const pg::EpisodeStep s = pg::episode_step(0.0f, T, 0.0f, 0, 0, T);
        CHECK(s.truncated && s.ended && s.len == T + 1);
    }
    {  // no limit: never truncated
        const pg::EpisodeStep s = pg::episode_step(0.0f, 1 << 30, 0.0f, 0, 0, 0);
        CHECK(!s.truncated && !s.ended && s.len == (1 << 30) + 1);
    }
    {  // T = 1: every counted step ends
        const pg::EpisodeStep s = pg::episode_step(0.0f, 0, 0.0f, 0, 0, 1);
        CHECK(s.truncated && s.len == 1);
    }
    std::printf("OK truncation boundary\n");
    return 0;
}

static int test_reset_step() {
    // the step that serves an auto-reset (the done row was set before it): nothing is counted, nothing ends, not even at
    // the limit
    const pg::EpisodeStep s = pg::episode_step(0.0f, 0, 0.0f, 0, 1, 1);
    CHECK(!s.counted && !s.terminated && !s.truncated && !s.ended && s.len == 0 && bits(s.ret) == bits(0.0f));
    const pg::EpisodeStep k = pg::episode_step(2.5f, 7, 0.0f, 0, 255, 8);
    CHECK(!k.counted && !k.ended && k.len == 7 && k.ret == 2.5f);
    // the episode after it counts from one
    const pg::EpisodeStep n = pg::episode_step(s.ret, s.len, 1.0f, 1, 0, 0);
    CHECK(n.counted && n.terminated && n.ended && n.len == 1 && n.ret == 1.0f);
    std::printf("OK reset step\n");
    return 0;
}

static int test_accumulation() {
    // 100 000 rewards of 0.1f: the float32 sum in step order, one rounding a step — not 10000, and not a double's sum
    volatile float want = 0.0f;
    float ret = 0.0f;
    int len = 0;
    for (int k = 0; k < 100000; k++) {
        want = want + 0.1f;
        const pg::EpisodeStep s = pg::episode_step(ret, len, 0.1f, 0, 0, 0);
        ret = s.ret, len = s.len;
        CHECK(bits(ret) == bits(want));
    }
    CHECK(len == 100000);
    double wide = 0.0;
    for (int k = 0; k < 100000; k++) wide += 0.1f;
    CHECK(bits(ret) != bits(static_cast<float>(wide)));  // (the test can tell the two apart)
    std::printf("OK accumulation %.3f\n", ret);
    return 0;
}

// What episode_rule_kernel and episode_list_kernel do, lane by lane, on the host.
static void compact(const std::vector<uint8_t>& ended, int capacity, std::vector<int>& list, int counts[2], std::vector<int>& rows) {
    const int n = static_cast<int>(ended.size()), B = pg::kEpisodeBlock, blocks = (n + B - 1) / B;
    std::vector<int> block_count(blocks, 0);
    for (int b = 0; b < blocks; b++)  // the rule kernel: ballots, popcounts, the sum of a workgroup's four waves
        for (int w = 0; w < pg::kEpisodeWaves; w++) {
            uint64_t ballot = 0;
            for (int l = 0; l < 64; l++) {
                const int i = b * B + w * 64 + l;
                if (i < n && ended[i]) ballot |= uint64_t(1) << l;
            }
            block_count[b] += __builtin_popcountll(ballot);
        }
    list.assign(n, -1);
    rows.assign(capacity, -1);
    int total = 0;
    for (int c : block_count) total += c;
    counts[0] = total;
    counts[1] = total < capacity ? total : capacity;
    for (int b = 0; b < blocks; b++) {  // the list kernel, any order of workgroups
        int base = 0;
        for (int k = 0; k < b; k++) base += block_count[k];
        int wave_count[pg::kEpisodeWaves] = {};
        uint64_t ballots[pg::kEpisodeWaves] = {};
        for (int w = 0; w < pg::kEpisodeWaves; w++) {
            for (int l = 0; l < 64; l++) {
                const int i = b * B + w * 64 + l;
                if (i < n && ended[i]) ballots[w] |= uint64_t(1) << l;
            }
            wave_count[w] = __builtin_popcountll(ballots[w]);
        }
        std::vector<int> frame_env(B, -1);
        for (int w = 0; w < pg::kEpisodeWaves; w++)
            for (int l = 0; l < 64; l++) {
                const int i = b * B + w * 64 + l;
                if (!(i < n && ended[i])) continue;
                int place = pg::episode_rank_in_wave(ballots[w], l);
                for (int v = 0; v < w; v++) place += wave_count[v];
                list[base + place] = i;
                frame_env[place] = i;
            }
        const int frames = pg::episode_frames_of_block(base, block_count[b], capacity);
        for (int f = 0; f < frames; f++) {
            if (base + f >= capacity) std::abort();  // (a ring row past its capacity)
            rows[base + f] = frame_env[f];
        }
    }
}

static int test_compaction() {
    std::mt19937 rng(12345);
    for (int n : {1, 63, 64, 65, 300, 1000})
        for (int density = 0; density < 3; density++)  // none, all, about 1 %
            for (int capacity : {0, 1, 4, n}) {
                if (capacity > n) continue;
                std::vector<uint8_t> ended(n);
                for (int i = 0; i < n; i++) ended[i] = density == 0 ? 0 : density == 1 ? 1 : (rng() % 100 == 0);
                if (density == 2 && n >= 300) ended[n - 1] = ended[255] = ended[256] = 1;  // the seams
                std::vector<int> want;
                for (int i = 0; i < n; i++)
                    if (ended[i]) want.push_back(i);
                std::vector<int> list, rows;
                int counts[2];
                compact(ended, capacity, list, counts, rows);
                CHECK(counts[0] == static_cast<int>(want.size()));
                CHECK(counts[1] == (counts[0] < capacity ? counts[0] : capacity));
                for (int k = 0; k < n; k++) CHECK(list[k] == (k < counts[0] ? want[k] : -1));
                for (int k = 0; k < capacity; k++) CHECK(rows[k] == (k < counts[1] ? want[k] : -1));
            }
    std::printf("OK compaction\n");
    return 0;
}

int main() {
    if (test_truncation_boundary() || test_reset_step() || test_accumulation() || test_compaction()) return 1;
    std::printf("ALL OK\n");
    return 0;
}
