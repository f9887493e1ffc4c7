// procgen2_amd/csrc/pg_history_filter.h compiled for the CPU: the flip and rotation mapping against numpy's rot90 transcribed,
// every byte of the border image and every word a run reads, exhaustively; the turn draws printed for the Python test.
#include <cstdio>
#include <vector>

#include "pg_history_filter.h"

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                   \
        }                                                               \
    } while (0)

// (H', W', pad): the shapes of tests/test_history_filter_gpu.py, and the largest
static const int kShapes[6][3] = {{64, 64, 0}, {8, 8, 16}, {1, 8, 0}, {63, 24, 1}, {56, 56, 4}, {64, 64, 16}};

// G = rot90(A[..., ::-1] if f else A, r), one quarter turn at a time: rot90(m)[i][j] = m[j][n - 1 - i]
static std::vector<int> turned(const std::vector<int>& a, int H, int W, int turn) {
    std::vector<int> g(a);
    if (turn & 1)
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) g[y * W + x] = a[y * W + (W - 1 - x)];
    for (int r = 0; r < (turn >> 1); r++) {  // (H = W)
        const std::vector<int> m(g);
        for (int i = 0; i < H; i++)
            for (int j = 0; j < W; j++) g[i * W + j] = m[j * W + (W - 1 - i)];
    }
    return g;
}

static int test_turns() {
    using namespace pg;
    for (const auto& s : kShapes) {
        const int H = s[0], W = s[1];
        std::vector<int> a(size_t(H) * W);
        for (int k = 0; k < H * W; k++) a[k] = k;
        for (int turn = 0; turn < 8; turn++) {
            if (turn >> 1 && H != W) continue;
            const std::vector<int> g = turned(a, H, W, turn);
            std::vector<int> seen(size_t(H) * W, 0);
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++) {
                    int ay, ax;
                    filter_turned(turn, H, W, y, x, ay, ax);
                    CHECK(ay >= 0 && ay < H && ax >= 0 && ax < W && g[y * W + x] == ay * W + ax);
                    seen[ay * W + ax]++;
                }
            for (int k = 0; k < H * W; k++) CHECK(seen[k] == 1);
        }
    }
    std::printf("OK turns\n");
    return 0;
}

// Every byte of the image, for every window, both edges, a cutout and every turn: a byte of the plane or a sentinel, the
// border and the margin zero, the pixels what aug_source_byte_index gives the turned pixel; every word written and every
// word a run reads inside the plane's share of the array.
static int test_image() {
    using namespace pg;
    long bytes = 0;
    for (const auto& s : kShapes) {
        const int H = s[0], W = s[1], pad = s[2], stride = filter_image_stride(W), words = filter_image_words(H, W);
        CHECK(stride % 8 == 0 && stride >= W + 2 && words * 4 == (H + 2) * stride && words <= kFilterImageWords && kFilterImageWords % 2 == 0);
        for (int y = 0; y < H; y++)
            for (int x0 = 0; x0 < W; x0 += kFilterRun)
                for (int ky = 0; ky < 3; ky++) {
                    const int first = filter_run_word(W, y, ky, x0);
                    CHECK(first >= 0 && first % 2 == 0 && first + 2 < words && first * 4 == (y + ky) * stride + x0);
                }
        for (int oy = -pad; oy <= 64 + pad - H; oy++)
            for (int ox = -pad; ox <= 64 + pad - W; ox++)
                for (int cut = 0; cut < 2; cut++)
                    for (int edge = 0; edge < 2; edge++)
                        for (int turn = 0; turn < 8; turn++) {
                            if (turn >> 1 && H != W) continue;
                            const AugParams p{oy, ox, cut ? H / 3 : 0, cut ? W / 4 : 0, cut ? (H + 1) / 2 : 0, cut ? W / 2 : 0, 0u};
                            for (int gy = 0; gy < H + 2; gy++)
                                for (int gx = 0; gx < stride; gx++, bytes++) {
                                    const int got = filter_image_source(p, edge, turn, H, W, gy, gx);
                                    CHECK((got >= 0 && got < 4096) || got == kAugZero || got == kAugCutout);
                                    const int y = gy - 1, x = gx - 1;
                                    if (y < 0 || y >= H || x < 0 || x >= W) {
                                        CHECK(got == kAugZero);
                                        continue;
                                    }
                                    int ay, ax;
                                    filter_turned(turn, H, W, y, x, ay, ax);
                                    CHECK(got == aug_source_byte_index(p, edge, ay, ax));
                                }
                        }
    }
    CHECK(bytes > 100000000);
    std::printf("OK image (%ld bytes)\n", bytes);
    return 0;
}

// The turn of entries 0 .. 255 for seeds 0, 1 and 2^32 - 1 under the four settings: "turns <seed> <turns> t0 t1 …".
static int print_turns() {
    using namespace pg;
    for (uint32_t seed : {0u, 1u, 0xFFFFFFFFu})
        for (int turns = 0; turns < 4; turns++) {
            std::printf("turns %u %d", seed, turns);
            for (uint32_t e = 0; e < 256; e++) {
                const int t = filter_turn(seed, e, turns);
                CHECK(t >= 0 && t < 8 && ((turns & kFilterFlip) || !(t & 1)) && ((turns & kFilterRot90) || !(t >> 1)));
                std::printf(" %d", t);
            }
            std::printf("\n");
        }
    return 0;
}

int main() {
    if (test_turns() || test_image() || print_turns()) return 1;
    std::printf("ALL OK\n");
    return 0;
}
