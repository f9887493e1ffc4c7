// The host half of the frame history (procgen2_amd/csrc/pg_history.h) compiled for the CPU: the walk of a gathered entry, the
// slot and offset arithmetic, and the listing of the engine's own memory.
// Prints "OK <section>" per section and "ALL OK"; exit status 1 on the first failure.
#include <cstdio>
#include <deque>
#include <vector>

#include "pg_history.h"

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                   \
        }                                                               \
    } while (0)

// The walk against a deque per env, run FORWARDS over the held pushes the way a frame stack is kept: a push that began an
// episode, or the oldest one held, fills the deque with itself; any other is appended.  After push p the deque, newest first,
// is the walk of entry (p, env).  Exhaustive: every began pattern of the T slots, T in 1 .. 5, K in 1 .. 8, head in 0 .. 3T;
// n = 3 envs with the pattern in the middle one and its complement beside it, so a wrong env stride shows.
static int test_walk() {
    using namespace pg;
    long entries = 0;
    for (int T = 1; T <= 5; T++)
        for (int K = 1; K <= kPolicyMaxStack; K++)
            for (int64_t head = 0; head <= 3 * T; head++)
                for (unsigned pattern = 0; pattern < (1u << T); pattern++) {
                    const int n = 3, env = 1;
                    std::vector<uint8_t> began(size_t(T) * n);
                    for (int s = 0; s < T; s++) {
                        const uint8_t bit = (pattern >> s) & 1u;
                        began[history_began_offset(s, n, 0)] = !bit;
                        began[history_began_offset(s, n, env)] = bit;
                        began[history_began_offset(s, n, 2)] = !bit;
                    }
                    const int64_t oldest = head > T ? head - T : 0;
                    CHECK(!history_held(head, head, T) && !history_held(oldest - 1, head, T) && !history_held(-1, head, T));
                    std::deque<int64_t> q;
                    for (int64_t p = oldest; p < head; p++) {
                        CHECK(history_held(p, head, T) && history_slot(p, T) == p % T);
                        if (p == oldest || began[size_t(p % T) * n + env])
                            q.assign(size_t(K), p);
                        else {
                            q.push_back(p);
                            q.pop_front();
                        }
                        int64_t f[kPolicyMaxStack];
                        history_walk(began.data(), n, T, head, p, env, K, f);
                        for (int j = 0; j < K; j++) {
                            CHECK(f[j] == q[size_t(K - 1 - j)]);  // row slot K-1-j shows f[j]: the deque, oldest first
                            CHECK(history_held(f[j], head, T));   // the walk never leaves the held pushes
                        }
                        entries++;
                    }
                }
    CHECK(entries > 10000);
    std::printf("OK walk (%ld entries)\n", entries);
    return 0;
}

static int test_offsets() {
    using namespace pg;
    CHECK(history_frame_offset(0, 7, 0, 3) == 0 && history_frame_offset(0, 7, 1, 3) == 3 * 4096 && history_frame_offset(1, 7, 0, 3) == size_t(7) * 3 * 4096);
    CHECK(history_frame_offset(2, 131, 130, 1) == (size_t(2) * 131 + 130) * 4096);
    CHECK(history_began_offset(4, 131, 130) == 4 * 131 + 130);
    // every (slot, env) has its own C*4096 bytes, in order, and the last ends where the ring does
    size_t expect = 0;
    for (int slot = 0; slot < 5; slot++)
        for (int env = 0; env < 131; env++, expect += 3 * 4096) CHECK(history_frame_offset(slot, 131, env, 3) == expect);
    CHECK(expect == history_frames_bytes(5, 131, 3));
    // above 2^32 bytes: 65 536 envs, T = 32, RGB
    const size_t last = history_frame_offset(31, 65536, 65535, 3);
    CHECK(last == size_t(32) * 65536 * 3 * 4096 - size_t(3) * 4096);
    CHECK(last > (size_t(1) << 34) && history_frames_bytes(32, 65536, 3) == 25769803776ull);
    CHECK(history_frame_offset(5, 65536, 21845, 3) < (size_t(1) << 32) && history_frame_offset(5, 65536, 21846, 3) > (size_t(1) << 32));  // (the sixth slot)
    CHECK(history_began_offset(31, 65536, 65535) == size_t(32) * 65536 - 1);
    // a push number past 2^31
    CHECK(history_slot((int64_t(1) << 40) + 3, 5) == ((int64_t(1) << 40) + 3) % 5);
    CHECK(history_held((int64_t(1) << 40), (int64_t(1) << 40) + 1, 5) && !history_held((int64_t(1) << 40) - 5, (int64_t(1) << 40) + 1, 5));
    std::printf("OK offsets\n");
    return 0;
}

static int test_listing() {
    // the engine's own block (pg_carve.h): the flags, the began bytes, the four tables and — the engine's own — the frames,
    // each rounded to 256 bytes
    pg::HistoryBuffers b{};
    b.capacity = 5, b.planes = 3, b.own_frames = 0;
    CHECK(pg::Carve::size(pg::list_history, 3, b) == 256 + 256 + 4096);
    CHECK(pg::Carve::size(pg::list_history, 131, b) == 256 + 768 + 4096);
    b.own_frames = 1;
    CHECK(pg::Carve::size(pg::list_history, 131, b) == 256 + 768 + 4096 + size_t(5) * 131 * 3 * 4096);
    b.planes = 1;
    CHECK(pg::Carve::size(pg::list_history, 3, b) == 256 + 256 + 4096 + size_t(5) * 3 * 4096);
    alignas(256) static uint8_t block[256 + 256 + 4096 + 5 * 3 * 4096];
    pg::Carve::bind(pg::list_history, block, b, 3);
    CHECK(b.pending == block && b.began == block + 256 && reinterpret_cast<uint8_t*>(b.table) == block + 512 && b.frames == block + 512 + 4096);
    CHECK((reinterpret_cast<uintptr_t>(b.frames) & 15u) == 0);
    b.own_frames = 0, b.frames = nullptr;
    pg::Carve::bind(pg::list_history, block, b, 3);
    CHECK(b.frames == nullptr && b.pending == block);
    std::printf("OK listing\n");
    return 0;
}

int main() {
    if (test_walk() || test_offsets() || test_listing()) return 1;
    std::printf("ALL OK\n");
    return 0;
}
