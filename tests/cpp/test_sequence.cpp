// The per-env fold of pgv_step_sequence's summary (procgen2_amd/csrc/pg_sequence.h sequence_fold) compiled for the CPU and
// held to hand-made rows.  Prints "OK <section>" per section and "ALL OK"; exit status 1 on the first failure.
#include <cstdio>
#include <cstring>
#include <vector>

#include "pg_sequence.h"

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

static pg::SequenceFold run(const std::vector<float>& rewards, const std::vector<uint8_t>& dones) {
    pg::SequenceFold acc{0.0f, 0, 0};
    for (size_t t = 0; t < rewards.size(); t++) acc = pg::sequence_fold(acc, rewards[t], dones[t]);
    return acc;
}

static int test_no_done() {
    const pg::SequenceFold s = run({1.0f, 0.0f, 2.5f, 0.0f}, {0, 0, 0, 0});
    CHECK(s.len == 4 && !s.done && bits(s.ret) == bits(3.5f));
    std::printf("OK no done\n");
    return 0;
}

static int test_done_places() {
    {  // at sub-step 0: what follows — the reset step, the next episode — is not the sequence's
        const pg::SequenceFold s = run({10.0f, 0.0f, 1.0f, 1.0f}, {1, 0, 0, 0});
        CHECK(s.len == 1 && s.done == 1 && bits(s.ret) == bits(10.0f));
    }
    {  // at sub-step T - 1
        const pg::SequenceFold s = run({0.0f, 1.0f, 0.0f, 10.0f}, {0, 0, 0, 1});
        CHECK(s.len == 4 && s.done == 1 && bits(s.ret) == bits(11.0f));
    }
    {  // twice: the first one cuts; any non-zero byte is a done
        const pg::SequenceFold s = run({1.0f, 2.0f, 0.0f, 4.0f, 8.0f}, {0, 7, 0, 0, 1});
        CHECK(s.len == 2 && s.done == 1 && bits(s.ret) == bits(3.0f));
    }
    {  // a sub-step that serves a reset (reward 0, done 0) counts like any other
        const pg::SequenceFold s = run({0.0f, 0.0f, 1.0f}, {0, 0, 0});
        CHECK(s.len == 3 && !s.done && bits(s.ret) == bits(1.0f));
    }
    std::printf("OK done places\n");
    return 0;
}

static int test_order() {
    // 2^24 + 1 + 1 in float32: from the left each 1 is rounded away, from the right they survive
    const float big = 16777216.0f;
    const pg::SequenceFold a = run({big, 1.0f, 1.0f}, {0, 0, 0});
    const pg::SequenceFold b = run({1.0f, 1.0f, big}, {0, 0, 0});
    CHECK(bits(a.ret) == bits(16777216.0f) && bits(b.ret) == bits(16777218.0f) && bits(a.ret) != bits(b.ret));
    // one rounding a step: 0.1f ten times is not 1.0f
    const pg::SequenceFold c = run(std::vector<float>(10, 0.1f), std::vector<uint8_t>(10, 0));
    float want = 0.0f;
    for (int k = 0; k < 10; k++) want = want + 0.1f;
    CHECK(bits(c.ret) == bits(want) && bits(c.ret) != bits(1.0f) && c.len == 10);
    // from 0.0f, not from -0.0f: a sequence of -0.0f rewards sums to +0.0f
    const pg::SequenceFold z = run({-0.0f, -0.0f}, {0, 0});
    CHECK(bits(z.ret) == bits(0.0f));
    std::printf("OK order\n");
    return 0;
}

static int test_single_step() {
    const pg::SequenceFold s = run({2.0f}, {0});
    CHECK(s.len == 1 && !s.done && bits(s.ret) == bits(2.0f));
    const pg::SequenceFold d = run({2.0f}, {1});
    CHECK(d.len == 1 && d.done == 1 && bits(d.ret) == bits(2.0f));
    std::printf("OK T = 1\n");
    return 0;
}

static int test_listing() {
    // the engine's block behind the running values (pg_carve.h): three regions rounded to 256 bytes, in order
    pg::SequenceBuffers b{};
    CHECK(pg::Carve::size(pg::list_sequence, 300) == 1280 + 1280 + 512);
    alignas(256) static uint8_t block[3072];
    pg::Carve::bind(pg::list_sequence, block, b, 300);
    CHECK(reinterpret_cast<uint8_t*>(b.ret) == block && reinterpret_cast<uint8_t*>(b.len) == block + 1280 && b.done == block + 2560);
    std::printf("OK listing\n");
    return 0;
}

int main() {
    if (test_no_done() || test_done_places() || test_order() || test_single_step() || test_listing()) return 1;
    std::printf("ALL OK\n");
    return 0;
}
