// The host half of the transitions (procgen2_amd/csrc/pg_transitions.h) compiled for the CPU: the n-step walk, the GAE step,
// and the listing of the feature's memory.
// Prints "OK <section>" per section and "ALL OK"; exit status 1 on the first failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <vector>

#include "pg_transitions.h"

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                   \
        }                                                               \
    } while (0)

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// The walk against the deque a replay learner keeps per env, run FORWARDS over the rows: every row that may be taken opens a
// window and is folded into every open window; a window closes when it holds n rows, behind a row that ends something, or
// in front of a row that may not be taken — and at the end of what the ring holds.  Exhaustive over the rows of a ring of
// seven pushes: each of the six rows is one of {not recorded, recorded, + TERMINATED, + TRUNCATED, + VOID} times the began byte
// behind it, 10^6 patterns; n in {1, 3, 6}; three envs with the pattern in the middle one, so a wrong env stride shows; every
// 97th pattern also with the ring wrapped (head 17) and one slot short (head 6).  `stride` > 1 (the sanitizer build's run) takes
// every stride-th pattern.
struct Window {
    int64_t start;
    int m;
    float ret, disc;
};
static int check_pattern(const int* kind, const int* began_bit, int64_t head, int T, int n_steps, float gamma, long& entries) {
    using namespace pg;
    const int n = 3, env = 1;
    static const uint8_t kinds[5] = {0, kTrRecorded, kTrRecorded | kTrTerminated, kTrRecorded | kTrTruncated, kTrRecorded | kTrVoid};
    const int64_t oldest = head > T ? head - T : 0;
    const int rows = static_cast<int>(head - 1 - oldest);  // rows oldest .. head - 2 are held with their successors
    std::vector<uint8_t> flags(size_t(T) * n, uint8_t(kTrRecorded)), began(size_t(T) * n, uint8_t(1));
    std::vector<int32_t> action(size_t(T) * n, -1);
    std::vector<float> reward(size_t(T) * n, 100.0f);
    for (int r = 0; r < rows; r++) {
        const int64_t q = oldest + r;
        const size_t at = history_began_offset(history_slot(q, T), n, env);
        flags[at] = kinds[kind[r]];
        action[at] = static_cast<int32_t>(q) + 3;
        reward[at] = r == 2 ? -10.0f : 0.04f * float(r + 1);
        began[history_began_offset(history_slot(q + 1, T), n, env)] = uint8_t(began_bit[r]);
    }
    TransitionRing g{n, T, head, began.data(), TransitionBuffers{T, nullptr, flags.data(), action.data(), reward.data()}};
    // the deque, forwards
    std::vector<TransitionResult> want(size_t(rows > 0 ? rows : 0));
    std::deque<Window> open;
    auto close_all = [&](uint8_t ends) {
        for (const Window& w : open) want[size_t(w.start - oldest)] = transition_result(int32_t(w.start) + 3, w.m, w.ret, w.disc, ends);
        open.clear();
    };
    for (int r = 0; r < rows; r++) {
        const int64_t q = oldest + r;
        const uint8_t f = kinds[kind[r]];
        if (!(f & kTrRecorded) || (f & kTrVoid)) {
            close_all(0);
            want[size_t(r)] = transition_result(0, 0, 0.0f, 1.0f, 0);
            continue;
        }
        open.push_back(Window{q, 0, 0.0f, 1.0f});
        for (Window& w : open) {
            const float t = w.disc * (r == 2 ? -10.0f : 0.04f * float(r + 1));
            w.ret = w.ret + t;
            w.disc = w.disc * gamma;
            w.m++;
        }
        uint8_t ends = f & (kTrTerminated | kTrTruncated);
        if (!ends && began_bit[r]) ends = kTrCut;
        if (ends)
            close_all(ends);
        else if (open.front().m == n_steps) {
            const Window w = open.front();
            open.pop_front();
            want[size_t(w.start - oldest)] = transition_result(int32_t(w.start) + 3, w.m, w.ret, w.disc, 0);
        }
    }
    close_all(0);
    for (int r = 0; r < rows; r++) {
        const TransitionResult got = transition_walk(g, oldest + r, env, n_steps, gamma), &w = want[size_t(r)];
        CHECK(got.action == w.action && got.steps == w.steps && got.status == w.status);
        CHECK(same_bits(got.ret, w.ret) && same_bits(got.discount, w.discount));
        CHECK(got.steps <= n_steps && (got.steps > 0) == ((got.status & kTrValid) != 0));
        entries++;
    }
    // what is never valid: the newest push (no successor), head, the push in front of the oldest, negative pushes, other envs' bounds
    for (int64_t p : {head - 1, head, oldest - 1, int64_t(-1), int64_t(1) << 40, INT64_MIN, INT64_MAX})
        CHECK(transition_walk(g, p, env, n_steps, gamma).status == 0 && transition_walk(g, p, env, n_steps, gamma).steps == 0);
    for (int bad : {-1, n, INT32_MAX, INT32_MIN}) CHECK(transition_walk(g, oldest, bad, n_steps, gamma).status == 0);
    return 0;
}
static int test_walk(long stride) {
    long entries = 0, patterns = 0;
    int kind[6], began_bit[6];
    for (long code = 0; code < 1000000; code += stride, patterns++) {
        long c = code;
        for (int r = 0; r < 6; r++, c /= 10) kind[r] = int(c % 10) % 5, began_bit[r] = int(c % 10) / 5;
        for (int n_steps : {1, 3, 6}) {
            if (check_pattern(kind, began_bit, 7, 7, n_steps, 0.99f, entries)) return 1;
            if (patterns % 97 == 0) {
                if (check_pattern(kind, began_bit, 17, 7, n_steps, 0.99f, entries)) return 1;
                if (check_pattern(kind, began_bit, 6, 7, n_steps, 1.0f, entries)) return 1;
                if (check_pattern(kind, began_bit, 1, 7, n_steps, 0.99f, entries) || check_pattern(kind, began_bit, 0, 7, n_steps, 0.99f, entries)) return 1;
            }
        }
    }
    CHECK(entries > 18000000 / stride);
    // the longest walk: 64 rows of reward 1 at gamma 1 in a ring of 65
    {
        using namespace pg;
        const int T = 65, n = 1;
        std::vector<uint8_t> flags(T, uint8_t(kTrRecorded)), began(T, uint8_t(0));
        std::vector<int32_t> action(T, 5);
        std::vector<float> reward(T, 1.0f);
        TransitionRing g{n, T, 65, began.data(), TransitionBuffers{T, nullptr, flags.data(), action.data(), reward.data()}};
        const TransitionResult r = transition_walk(g, 0, 0, kTrMaxSteps, 1.0f);
        CHECK(r.steps == 64 && r.ret == 64.0f && r.discount == 1.0f && r.status == kTrValid && r.action == 5);
        CHECK(transition_walk(g, 1, 0, kTrMaxSteps, 1.0f).steps == 63);
        // 0.04 three times at 0.99: the roundings, one by one
        reward.assign(T, 0.04f);
        const float t1 = 0.99f * 0.04f, d2 = 0.99f * 0.99f, t2 = d2 * 0.04f, s1 = 0.04f + t1, s2 = s1 + t2;
        const TransitionResult w = transition_walk(g, 10, 0, 3, 0.99f);
        CHECK(same_bits(w.ret, s2) && same_bits(w.discount, d2 * 0.99f) && w.steps == 3);
    }
    std::printf("OK walk (%ld patterns, %ld entries)\n", patterns, entries);
    return 0;
}

// The GAE step against a straight loop over an episode table written down by hand, and known answers.
static int test_gae() {
    using namespace pg;
    // gamma = lambda = 1, V = 0: the advantage is the sum of the rewards up to the episode's end
    {
        const uint8_t fl[6] = {kTrRecorded, kTrRecorded, kTrRecorded | kTrTerminated, kTrRecorded, kTrRecorded | kTrVoid, kTrRecorded};
        const float r[6] = {1, 2, 4, 8, 16, 32};
        const float want[6] = {7, 6, 4, 8, 0, 32};
        float carry = 0.0f;
        for (int t = 5; t >= 0; t--) {
            const GaeStep s = gae_step(fl[t], 0, r[t], 0.0f, 0.0f, 0.0f, 1.0f, 1.0f, carry);
            CHECK(s.adv == want[t] && s.ret == want[t]);
            carry = s.adv;
        }
    }
    // a truncated row bootstraps from its own value, a cut row from nothing, an unrecorded row returns V
    CHECK(gae_step(kTrRecorded | kTrTruncated, 0, 1.0f, 0.5f, 9.0f, 2.0f, 0.5f, 0.25f, 100.0f).adv == 1.0f + 0.5f * 2.0f - 0.5f);
    CHECK(gae_step(kTrRecorded, 1, 1.0f, 0.5f, 9.0f, 2.0f, 0.5f, 0.25f, 100.0f).adv == 1.0f - 0.5f);
    CHECK(gae_step(kTrRecorded | kTrTerminated, 1, 1.0f, 0.5f, 9.0f, 2.0f, 0.5f, 0.25f, 100.0f).adv == 1.0f - 0.5f);
    CHECK(gae_step(kTrRecorded, 0, 1.0f, 0.5f, 9.0f, 2.0f, 0.5f, 0.25f, 100.0f).adv == (1.0f + 0.5f * 9.0f - 0.5f) + 0.25f * 100.0f);
    CHECK(gae_step(0, 1, 1.0f, 0.5f, 9.0f, 2.0f, 0.5f, 0.25f, 100.0f).adv == 0.0f && gae_step(0, 1, 1.0f, 0.5f, 9.0f, 2.0f, 0.5f, 0.25f, 100.0f).ret == 0.5f);
    CHECK(gae_step(kTrRecorded | kTrVoid | kTrTerminated, 0, 1.0f, 0.5f, 9.0f, 2.0f, 0.5f, 0.25f, 100.0f).ret == 0.5f);
    // the straight loop, on rows drawn by a small generator; floats that round (0.04, values in thirds)
    uint32_t x = 12345u;
    auto draw = [&]() { return x = x * 1664525u + 1013904223u, x >> 8; };
    long rows = 0;
    for (int round = 0; round < 2000; round++) {
        const int L = 16;
        uint8_t fl[L], bg[L];
        float r[L], v[L + 1], tv[L], adv[L], ret[L];
        for (int t = 0; t < L; t++) {
            const uint32_t k = draw() % 16;
            fl[t] = k == 0 ? 0 : uint8_t(kTrRecorded | (k == 1 ? kTrTerminated : 0) | (k == 2 ? kTrTruncated : 0) | (k == 3 ? kTrVoid : 0));
            bg[t] = draw() % 8 == 0;
            r[t] = draw() % 3 == 0 ? 0.04f : float(draw() % 21) - 10.0f;
            v[t] = float(draw() % 2001) / 3.0f - 333.0f;
            tv[t] = float(draw() % 2001) / 7.0f;
        }
        v[L] = float(draw() % 2001) / 3.0f;
        const float gamma = round % 2 ? 1.0f : 0.99f, lambda = round % 2 ? 1.0f : 0.95f, c = gamma * lambda;
        const bool with_tv = (round / 2) % 2 == 0;
        float carry = 0.0f;
        for (int t = L - 1; t >= 0; t--) {  // the loop, written out
            if (!(fl[t] & kTrRecorded) || (fl[t] & kTrVoid)) {
                adv[t] = 0.0f, ret[t] = v[t], carry = 0.0f;
                continue;
            }
            const bool term = fl[t] & kTrTerminated, trunc = !term && (fl[t] & kTrTruncated), cut = !term && !trunc && bg[t];
            const float nv = term || cut ? 0.0f : trunc ? (with_tv ? tv[t] : 0.0f) : v[t + 1];
            const float a = gamma * nv;
            const float b = r[t] + a;
            const float delta = b - v[t];
            float out = delta;
            if (!term && !trunc && !cut) {
                const float d = c * carry;
                out = delta + d;
            }
            adv[t] = out, carry = out;
            ret[t] = out + v[t];
        }
        carry = 0.0f;
        for (int t = L - 1; t >= 0; t--, rows++) {
            const GaeStep s = gae_step(fl[t], bg[t], r[t], v[t], v[t + 1], with_tv ? tv[t] : 0.0f, gamma, c, carry);
            CHECK(same_bits(s.adv, adv[t]) && same_bits(s.ret, ret[t]));
            carry = s.adv;
        }
    }
    std::printf("OK gae (%ld rows)\n", rows);
    return 0;
}

static int test_listing() {
    using namespace pg;
    TransitionBuffers b{};
    b.capacity = 5;
    CHECK(Carve::size(list_transitions, 3, b) == 256 + 256 + 256 + 256);
    CHECK(Carve::size(list_transitions, 131, b) == 256 + 768 + 2816 + 2816);  // 655 bytes, 2 620 bytes twice
    alignas(256) static uint8_t block[256 + 768 + 2816 + 2816];
    Carve::bind(list_transitions, block, b, 131);
    CHECK(b.pending == block && b.flags == block + 256 && reinterpret_cast<uint8_t*>(b.action) == block + 1024 &&
          reinterpret_cast<uint8_t*>(b.reward) == block + 1024 + 2816);
    CHECK(transition_held(3, 5, 5) && !transition_held(4, 5, 5) && !transition_held(-1, 5, 5) && transition_held(2, 7, 5) && !transition_held(1, 7, 5));
    CHECK(transition_held((int64_t(1) << 40), (int64_t(1) << 40) + 2, 5) && !transition_held(INT64_MAX, INT64_MAX, 5));
    CHECK(transition_ends(kTrRecorded, 1) == kTrCut && transition_ends(kTrRecorded, 0) == 0 && transition_ends(kTrRecorded | kTrVoid, 1) == 0);
    CHECK(transition_ends(kTrRecorded | kTrTerminated, 1) == kTrTerminated && transition_ends(kTrRecorded | kTrTruncated, 1) == kTrTruncated);
    std::printf("OK listing\n");
    return 0;
}

int main(int argc, char** argv) {
    const long stride = argc > 1 ? std::atol(argv[1]) : 1;
    if (stride < 1 || test_walk(stride) || test_gae() || test_listing()) return 1;
    std::printf("ALL OK\n");
    return 0;
}
