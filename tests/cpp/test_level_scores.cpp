// The level score rule (procgen2_amd/csrc/pg_level_scores.h) compiled for the CPU: fix() at its edges, accept by mask and by
// wrapping range, the chain of level_score_step against a straight loop written out from include/procgen2_vec.h, and finish.
// Prints "OK <section>" per section and "ALL OK"; exit status 1 on the first failure.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "pg_level_scores.h"

#define CHECK(cond) \
    do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

using namespace pg;
static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

static int test_fix() {
    const float u = 1.0f / 65536.0f, nan = __builtin_nanf("");
    CHECK(level_score_fix(kScoreAbs, nan) == 0 && level_score_fix(kScorePositive, nan) == 0);
    CHECK(level_score_fix(kScoreAbs, -1.5f) == 98304u && level_score_fix(kScorePositive, -1.5f) == 0 && level_score_fix(kScorePositive, 1.5f) == 98304u);
    CHECK(level_score_fix(kScoreAbs, -0.0f) == 0 && level_score_fix(kScoreAbs, 1.0f) == 65536u);
    CHECK(level_score_fix(kScoreAbs, 32768.0f) == 2147483647u && level_score_fix(kScoreAbs, -__builtin_inff()) == 2147483647u);
    CHECK(level_score_fix(kScoreAbs, std::nextafterf(32768.0f, 0.0f)) == 2147483520u);  // the largest float below 2^31
    CHECK(level_score_fix(kScoreAbs, 0.5f * u) == 0 && level_score_fix(kScoreAbs, 1.5f * u) == 2 && level_score_fix(kScoreAbs, 2.5f * u) == 2);  // ties to even
    CHECK(level_score_fix(kScoreAbs, std::nextafterf(0.5f * u, 1.0f)) == 1 && level_score_fix(kScorePositive, std::nextafterf(2.5f * u, 0.0f)) == 2);
    std::printf("OK fix\n");
    return 0;
}

static int test_accept() {
    uint32_t k = 0;
    for (uint32_t mask : {2u, 4u, 6u})
        for (uint8_t known : {0, 1, 2, 3, 40}) CHECK(level_score_accept(mask, 5, 3, 6, known, k) == (known < 3 && ((mask >> known) & 1u)) && k == 1);
    CHECK(level_score_accept(2, 5, 3, 5, 1, k) && k == 0 && level_score_accept(2, 5, 3, 7, 1, k) && k == 2);
    CHECK(!level_score_accept(2, 5, 3, 8, 1, k) && !level_score_accept(2, 5, 3, 4, 1, k) && k == 0xFFFFFFFFu);
    CHECK(level_score_accept(2, 0xFFFFFFFEu, 4, 0xFFFFFFFEu, 1, k) && k == 0 && level_score_accept(2, 0xFFFFFFFEu, 4, 1, 1, k) && k == 3);  // over 2^32
    CHECK(!level_score_accept(2, 0xFFFFFFFEu, 4, 2, 1, k) && !level_score_accept(2, 0xFFFFFFFEu, 4, 0xFFFFFFFDu, 1, k));
    std::printf("OK accept\n");
    return 0;
}

// Hand-picked stretches of five rows, flags and the six began bytes round them, levels 7, 7, 9, 3, 7 (the second a caller's
// label) under first_level 7, K = 3, mask = seeded: what is filed, by the loop written out and by the rule's functions.
struct Filed { uint64_t sum[3]; uint32_t steps[3], segments[3]; float top[3]; };
static int test_walk() {
    const int L = 5;
    const uint8_t R = kTrRecorded, TE = R | kTrTerminated, TR = R | kTrTruncated, VO = R | kTrVoid;
    static const uint8_t cases[][2 * L + 1] = {
        {R, R, R, R, R, 0, 0, 0, 0, 0, 0},      // one segment, cut by the stretch on both sides
        {R, TE, R, R, TR, 1, 0, 1, 0, 0, 1},    // a whole complete episode, then one on level 9 that began inside and is truncated
        {R, TR, R, R, R, 0, 0, 1, 0, 0, 0},     // complete but not whole; the rest partial on level 9
        {R, R, VO, R, TE, 1, 0, 0, 1, 0, 0},    // a VOID row closes as partial; no CUT behind it; a new whole episode ends
        {0, R, R, 0, R, 1, 1, 0, 1, 1, 0},      // rows not recorded: nothing to close, then a close, then a last row alone
        {R, R, R, R, R, 1, 0, 0, 1, 0, 1},      // CUT behind row 2 and behind the last row
        {TE, TE, TR, TE, TE, 1, 1, 1, 1, 1, 1}, // TERMINATED with began behind it: complete, never CUT; levels 9 and 3 are dropped
        {VO, 0, VO, TE | kTrVoid, 0, 1, 1, 1, 1, 1, 1},  // nothing live at all
    };
    const float r[L] = {10.0f, 0.04f, -10.0f, 0.1f, 1.0f}, x[L] = {-0.3f, 1.0f / 3.0f, -2.5f, 0.7f, 1e-6f};
    const uint32_t level[L] = {7, 7, 9, 3, 7};
    const uint8_t known[L] = {1, 2, 1, 1, 1};
    for (const auto& c : cases)
        for (int partial = 0; partial < 2; partial++) {
            const uint8_t *fl = c, *bg = c + L;
            Filed want{}, got{};
            for (int k = 0; k < 3; k++) want.top[k] = got.top[k] = -__builtin_inff();
            bool open = false, whole = false;  // the loop, written out
            uint64_t sum = 0;
            uint32_t steps = 0, lv = 0, kn = 0;
            float ret = 0.0f;
            for (int t = 0; t < L; t++) {
                const bool live = (fl[t] & kTrRecorded) && !(fl[t] & kTrVoid), complete = live && (fl[t] & (kTrTerminated | kTrTruncated));
                if (live && !open) open = true, lv = level[t], kn = known[t], whole = bg[t] != 0, sum = 0, steps = 0, ret = 0.0f;
                if (live) sum += uint32_t(std::nearbyintf(std::fabs(x[t]) * 65536.0f)), steps += 1, ret = ret + r[t];
                if (!open || (live && !complete && !bg[t + 1] && t + 1 < L)) continue;
                open = false;
                const uint32_t k = lv - 7u;
                if ((!complete && !partial) || kn != 1 || k >= 3) continue;
                want.sum[k] += sum, want.steps[k] += steps, want.segments[k] += 1;
                if (complete && whole && ret > want.top[k]) want.top[k] = ret;
            }
            LevelSegment seg{};
            bool is_open = false;
            for (int t = 0; t <= L; t++) {  // (t = L: behind the last row)
                uint32_t k = 0;
                const bool ok = t < L && level_score_accept(2, 7, 3, level[t], known[t], k);
                const uint8_t closed = t == L ? (is_open ? kLsPartial : uint8_t(0))
                                              : level_score_step(seg, is_open, level_score_cell(fl[t], bg[t], bg[t + 1], ok), level_score_fix(kScoreAbs, x[t]), r[t], k);
                if (!closed || !level_score_files(seg.opened, closed == kLsComplete, partial != 0)) continue;
                got.sum[seg.k] += seg.sum, got.steps[seg.k] += seg.steps, got.segments[seg.k] += 1;
                if (level_score_raises(seg.opened, closed == kLsComplete, seg.ret) && seg.ret > got.top[seg.k]) got.top[seg.k] = seg.ret;
            }
            CHECK(std::memcmp(&want, &got, sizeof want) == 0 && (&c != &cases[1] || (want.segments[0] == 1 && want.segments[2] == 1 && want.top[0] == 10.04f)));
        }
    std::printf("OK walk\n");
    return 0;
}

static int test_finish() {
    const float m = (float(uint64_t(300001)) / float(7u)) * (1.0f / 65536.0f);
    CHECK(same_bits(level_score_finish(123.0f, 0, 300001, 7, 0.25f), m));  // first touch: alpha and the old score do not count
    const float keep = 1.0f - 0.3f, a = keep * 0.9f, b = 0.3f * m;
    CHECK(same_bits(level_score_finish(0.9f, 4, 300001, 7, 0.3f), a + b));
    CHECK(same_bits(level_score_finish(0.9f, 4, 300001, 7, 0.0f), 0.9f) && same_bits(level_score_finish(0.9f, 4, 300001, 7, 1.0f), m));
    CHECK(same_bits(level_score_finish(0.0f, 0, (uint64_t(1) << 40) + 1, 3, 1.0f), (float(uint64_t(1) << 40) / 3.0f) * (1.0f / 65536.0f)));  // a sum past 2^32
    std::printf("OK finish\n");
    return 0;
}

int main() {
    if (test_fix() || test_accept() || test_walk() || test_finish()) return 1;
    std::printf("ALL OK\n");
    return 0;
}
