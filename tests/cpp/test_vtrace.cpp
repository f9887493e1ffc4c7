// The V-trace rule (procgen2_amd/csrc/pg_vtrace.h vtrace_step) compiled for the CPU, against a straight loop written out from
// include/procgen2_vec.h, the GAE law against gae_step, and the clips on both sides of their bounds.
// Prints "OK <section>" per section and "ALL OK"; exit status 1 on the first failure.  `stride` > 1 takes every stride-th pattern.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pg_vtrace.h"

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                   \
        }                                                               \
    } while (0)

using namespace pg;
static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }
static float lesser(float a, float b) { return a < b ? a : b; }

// Every pattern of five rows, each one of {not recorded, recorded, + TERMINATED, + TRUNCATED, + VOID} times the began byte
// behind it: the chain of vtrace_step against the loop, with and without the GAE law's parameters, beside gae_step.
static int test_patterns(long stride) {
    const int L = 5;
    static const uint8_t kinds[5] = {0, kTrRecorded, kTrRecorded | kTrTerminated, kTrRecorded | kTrTruncated, kTrRecorded | kTrVoid};
    const float r[L] = {10.0f, 0.04f, -10.0f, 0.0f, 1.0f}, v[L + 1] = {-0.0f, 1.0f / 3.0f, -2.5f, 0.7f, 0.0f, 1.25f};
    const float tv[L] = {0.5f, -1.0f / 7.0f, 2.0f, 0.3f, -0.9f}, rho[L] = {0.2f, 0.9f, 1.0f, 1.7f, 3.0f};
    const VtraceRule rules[2] = {{0.99f, 0.95f, 1.3f, 0.8f, 2.0f, 0.37f, 2.0f}, {0.99f, 0.95f, 1.0f, 1.0f, 1.0f, 1.0f, 0.0f}};
    long rows = 0;
    for (long code = 0; code < 100000; code += stride) {
        uint8_t fl[L], bg[L];
        long c = code;
        for (int t = 0; t < L; t++, c /= 10) fl[t] = kinds[(c % 10) % 5], bg[t] = uint8_t((c % 10) / 5);
        for (int law = 0; law < 2; law++) {
            const VtraceRule& p = rules[law];
            float vs[L], pg[L], carry = 0.0f, next = v[L];
            for (int t = L - 1; t >= 0; t--) {  // the loop, written out
                if (!(fl[t] & kTrRecorded) || (fl[t] & kTrVoid)) {
                    vs[t] = v[t], pg[t] = 0.0f, carry = 0.0f, next = v[t];
                    continue;
                }
                const bool term = fl[t] & kTrTerminated, trunc = !term && (fl[t] & kTrTruncated), cut = !term && !trunc && bg[t];
                const bool ends = term || trunc || cut;
                const float nv = term || cut ? 0.0f : trunc ? tv[t] : v[t + 1];
                const float s = r[t] * p.reward_scale;
                const float rr = p.reward_clip <= 0.0f ? s : s > p.reward_clip ? p.reward_clip : s < -p.reward_clip ? -p.reward_clip : s;
                const float w = law ? 1.0f : rho[t];
                const float a = p.gamma * nv, b = rr + a, d = b - v[t], delta = lesser(w, p.rho_bar) * d;
                float x = delta;
                if (!ends) {
                    const float cc = p.lambda * lesser(w, p.c_bar), k = p.gamma * cc, e = k * carry;
                    x = delta + e;
                }
                vs[t] = x + v[t];
                const float pa = p.gamma * (ends ? nv : next), pb = rr + pa, pd = pb - v[t];
                pg[t] = lesser(w, p.pg_rho_bar) * pd;
                carry = x, next = vs[t];
            }
            float gcarry = 0.0f;
            carry = 0.0f, next = v[L];
            for (int t = L - 1; t >= 0; t--, rows++) {
                const VtraceStep got = vtrace_step(p, fl[t], bg[t], r[t], v[t], v[t + 1], tv[t], law ? 1.0f : rho[t], carry, next);
                CHECK(same_bits(got.vs, vs[t]) && same_bits(got.pg, pg[t]));
                carry = got.x, next = got.vs;
                if (law) {  // vs is GAE's returns, bit for bit
                    const GaeStep g = gae_step(fl[t], bg[t], r[t], v[t], v[t + 1], tv[t], p.gamma, p.gamma * p.lambda, gcarry);
                    CHECK(same_bits(got.vs, g.ret));
                    gcarry = g.adv;
                }
            }
        }
    }
    std::printf("OK patterns (%ld rows)\n", rows);
    return 0;
}

// The reward clip and the three thresholds, on both sides of each bound; a carry of infinity behind an ending row.
static int test_clips() {
    const VtraceRule p{0.5f, 0.5f, 1.25f, 0.75f, 2.0f, 0.5f, 2.0f};
    auto cell = [&](float reward, float rho) { return vtrace_cell(p, kTrRecorded, 0, reward, 0.0f, 0.0f, 0.0f, rho); };
    CHECK(cell(10.0f, 1.0f).r == 2.0f && cell(-10.0f, 1.0f).r == -2.0f && cell(3.0f, 1.0f).r == 1.5f && cell(4.0f, 1.0f).r == 2.0f && cell(0.0f, 1.0f).r == 0.0f);
    CHECK(vtrace_cell(VtraceRule{0.5f, 0.5f, 1.0f, 1.0f, 1.0f, 0.5f, 0.0f}, kTrRecorded, 0, 10.0f, 0.0f, 0.0f, 0.0f, 1.0f).r == 5.0f);
    CHECK(cell(2.0f, 1.0f).delta == 1.0f && cell(2.0f, 1.5f).delta == 1.25f && cell(2.0f, 1.25f).delta == 1.25f);  // rho_bar
    CHECK(cell(2.0f, 0.5f).k == 0.5f * (0.5f * 0.5f) && cell(2.0f, 1.0f).k == 0.5f * (0.5f * 0.75f));             // c_bar
    CHECK(cell(2.0f, 1.5f).pr == 1.5f && cell(2.0f, 3.0f).pr == 2.0f);                                             // pg_rho_bar
    const float inf = __builtin_inff();
    const VtraceStep ended = vtrace_step(p, kTrRecorded | kTrTerminated, 0, 2.0f, 0.0f, 9.0f, 9.0f, 1.0f, inf, inf);
    CHECK(ended.x == 1.0f && ended.vs == 1.0f && ended.pg == 1.0f);
    const VtraceStep dead = vtrace_step(p, 0, 1, 2.0f, -0.0f, 9.0f, 9.0f, 1.0f, inf, inf);
    CHECK(dead.x == 0.0f && same_bits(dead.vs, -0.0f) && dead.pg == 0.0f);
    std::printf("OK clips\n");
    return 0;
}

int main(int argc, char** argv) {
    const long stride = argc > 1 ? std::atol(argv[1]) : 1;
    if (stride < 1 || test_patterns(stride) || test_clips()) return 1;
    std::printf("ALL OK\n");
    return 0;
}
