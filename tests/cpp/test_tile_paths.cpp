// The row routine of the path distances (procgen2_amd/csrc/pg_paths.h path_row, path_probe, path_cell_of) compiled for the
// CPU with 64 emulated lanes, against a queue BFS written here: random boards of every (w, h) in 1 .. 64 x 1 .. 64 at a few
// densities, the open boards 1x1, 1x64, 64x1 and 64x64 from each corner (distance |dx| + |dy|, maximum 126), a source in a
// wall, an empty passable set, no source, tile ids of 32 and above, the step codes, the cell rule.
// The row is given with a guard int16 on either side, which must stay as it was.
// Prints "OK <section>" per section and "ALL OK"; exit status 1 on the first failure.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <limits>
#include <vector>

#include "pg_paths.h"

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                   \
        }                                                               \
    } while (0)

static uint32_t g_rng = 12345u;
static uint32_t rnd() {
    g_rng ^= g_rng << 13, g_rng ^= g_rng >> 17, g_rng ^= g_rng << 5;
    return g_rng;
}

// include/procgen2_vec.h, point 4 of the path distances, with a queue
static std::vector<int16_t> queue_bfs(const std::vector<uint8_t>& tiles, int w, int h, uint32_t mask, uint32_t passable, int source) {
    std::vector<int16_t> dist(size_t(w) * h, int16_t(-1));
    if (source < 0) return dist;
    auto ok = [&](int c) {
        const uint32_t t = tiles[c] & mask;
        return t < 32u && ((passable >> t) & 1u) && dist[c] < 0;
    };
    std::deque<int> q{source};
    dist[source] = 0;
    while (!q.empty()) {
        const int c = q.front(), x = c / h, y = c % h;
        q.pop_front();
        const int nb[4] = {x > 0 ? c - h : -1, x < w - 1 ? c + h : -1, y > 0 ? c - 1 : -1, y < h - 1 ? c + 1 : -1};
        for (int k : nb)
            if (k >= 0 && ok(k)) dist[k] = int16_t(dist[c] + 1), q.push_back(k);
    }
    return dist;
}

constexpr int16_t kGuard = 0x5A5A;

// path_row on a guarded row; 0 = equal to the queue BFS (and the guards whole), else the line that failed
static int compare(const std::vector<uint8_t>& tiles, int w, int h, uint32_t mask, uint32_t passable, int source, int probe) {
    std::vector<int16_t> row(size_t(w) * h + 2, kGuard);
    pg::path_row(pg::EmulatedLanes{}, source >= 0 ? tiles.data() : nullptr, w, h, mask, passable, source, row.data() + 1);
    CHECK(row.front() == kGuard && row.back() == kGuard);
    const std::vector<int16_t> want = queue_bfs(tiles, w, h, mask, passable, source);
    for (size_t c = 0; c < want.size(); c++) CHECK(row[c + 1] == want[c]);
    int32_t dist = 77;
    uint8_t step = 77;
    pg::path_probe(row.data() + 1, w, h, probe, dist, step);
    CHECK(dist == (probe >= 0 ? want[probe] : -1));
    if (dist <= 0) {
        CHECK(step == 0);
    } else {
        const int x = probe / h, y = probe % h;
        const int nb[4] = {x > 0 ? probe - h : -1, x < w - 1 ? probe + h : -1, y > 0 ? probe - 1 : -1, y < h - 1 ? probe + 1 : -1};
        int first = 0;
        for (int k = 0; k < 4 && !first; k++)
            if (nb[k] >= 0 && want[nb[k]] == dist - 1) first = k + 1;
        CHECK(first != 0 && step == first);
    }
    return 0;
}

static int test_random_boards() {
    const int wall_percent[3] = {15, 35, 55};
    long boards = 0;
    for (int w = 1; w <= 64; w++)
        for (int h = 1; h <= 64; h++)
            for (int density : wall_percent) {
                std::vector<uint8_t> tiles(size_t(w) * h);
                for (auto& t : tiles) t = (rnd() % 100u) < uint32_t(density) ? uint8_t(1 + rnd() % 3u) : uint8_t(0);
                const int cells = w * h, source = int(rnd() % uint32_t(cells)), probe = int(rnd() % uint32_t(cells));
                CHECK(compare(tiles, w, h, 0xff, 1u, source, probe) == 0);
                boards++;
            }
    // two passable ids, a mask that folds ids, ids of 32 and above (never passable, whatever the mask's low bits say)
    for (int round = 0; round < 200; round++) {
        const int w = 1 + int(rnd() % 64u), h = 1 + int(rnd() % 64u), cells = w * h;
        std::vector<uint8_t> tiles(static_cast<size_t>(cells), uint8_t(0));
        for (auto& t : tiles) t = uint8_t(rnd() % 5u == 0 ? 32u + rnd() % 224u : rnd() % 12u);
        CHECK(compare(tiles, w, h, 0xff, 0x5u | (1u << 11) | (1u << 31), int(rnd() % uint32_t(cells)), int(rnd() % uint32_t(cells))) == 0);
        CHECK(compare(tiles, w, h, 7, 0x3u, int(rnd() % uint32_t(cells)), int(rnd() % uint32_t(cells))) == 0);
        CHECK(compare(tiles, w, h, 0xff, 0xFFFFFFFFu, int(rnd() % uint32_t(cells)), -1) == 0);
        boards += 3;
    }
    std::printf("OK random boards (%ld)\n", boards);
    return 0;
}

static int test_open_boards() {
    const int sides[4][2] = {{1, 1}, {1, 64}, {64, 1}, {64, 64}};
    for (const auto& side : sides) {
        const int w = side[0], h = side[1];
        const std::vector<uint8_t> tiles(size_t(w) * h, uint8_t(0));
        const int corners[4] = {0, h - 1, (w - 1) * h, w * h - 1};
        for (int source : corners) {
            std::vector<int16_t> row(size_t(w) * h);
            pg::path_row(pg::EmulatedLanes{}, tiles.data(), w, h, 0xff, 1u, source, row.data());
            int longest = 0;
            for (int c = 0; c < w * h; c++) {
                const int d = std::abs(c / h - source / h) + std::abs(c % h - source % h);
                CHECK(row[c] == d);
                longest = d > longest ? d : longest;
            }
            CHECK(longest == (w - 1) + (h - 1));
            for (int probe : corners) CHECK(compare(tiles, w, h, 0xff, 1u, source, probe) == 0);
        }
    }
    std::printf("OK open boards\n");
    return 0;
}

static int test_special_cases() {
    // a source in a wall: distance 0 there, and the field grows from it as from any cell
    {
        const int w = 9, h = 7;
        std::vector<uint8_t> tiles(size_t(w) * h, uint8_t(0));
        const int source = 3 * h + 2;
        tiles[source] = 1;
        std::vector<int16_t> row(size_t(w) * h);
        pg::path_row(pg::EmulatedLanes{}, tiles.data(), w, h, 0xff, 1u, source, row.data());
        CHECK(row[source] == 0 && row[source + 1] == 1 && row[source - h] == 1 && row[0] == 3 + 2);
        CHECK(compare(tiles, w, h, 0xff, 1u, source, 0) == 0);
        // walled in: the source alone
        for (int c = 0; c < w * h; c++) tiles[c] = 1;
        CHECK(compare(tiles, w, h, 0xff, 1u, source, source + 1) == 0);
        pg::path_row(pg::EmulatedLanes{}, tiles.data(), w, h, 0xff, 1u, source, row.data());
        for (int c = 0; c < w * h; c++) CHECK(row[c] == (c == source ? 0 : -1));
    }
    // an empty passable set: the source alone, on every size's corners
    for (int w : {1, 2, 63, 64})
        for (int h : {1, 2, 63, 64}) {
            const std::vector<uint8_t> tiles(size_t(w) * h, uint8_t(0));
            for (int source : {0, w * h - 1}) {
                std::vector<int16_t> row(size_t(w) * h);
                pg::path_row(pg::EmulatedLanes{}, tiles.data(), w, h, 0xff, 0u, source, row.data());
                for (int c = 0; c < w * h; c++) CHECK(row[c] == (c == source ? 0 : -1));
                CHECK(compare(tiles, w, h, 0xff, 0u, source, source) == 0);
            }
            CHECK(compare(tiles, w, h, 0xff, 1u, -1, 0) == 0);  // no source: all -1, the tiles not read
        }
    // a ring around the edge of 64 x 64 must not leak across lane 63 → lane 0 or bit 63 → bit 0
    {
        const int w = 64, h = 64;
        std::vector<uint8_t> tiles(size_t(w) * h, uint8_t(1));
        for (int y = 0; y < h; y++) tiles[y] = 0, tiles[(w - 1) * h + y] = 0;  // columns 0 and 63 open, nothing between
        std::vector<int16_t> row(size_t(w) * h);
        pg::path_row(pg::EmulatedLanes{}, tiles.data(), w, h, 0xff, 1u, 0, row.data());
        for (int y = 0; y < h; y++) CHECK(row[y] == y && row[(w - 1) * h + y] == -1);
        for (int x = 0; x < w; x++) tiles[x * h] = 0, tiles[x * h + h - 1] = 0;  // now the whole ring
        pg::path_row(pg::EmulatedLanes{}, tiles.data(), w, h, 0xff, 1u, 0, row.data());
        CHECK(row[w * h - 1] == 126 && row[(w - 1) * h] == 63 && row[h - 1] == 63 && row[h + 1] == -1);
        CHECK(compare(tiles, w, h, 0xff, 1u, 0, w * h - 1) == 0);
    }
    std::printf("OK special cases\n");
    return 0;
}

static int test_cells() {
    using pg::path_cell_of;
    CHECK(path_cell_of(0.0f, 0.0f, 5, 7) == 6 && path_cell_of(4.99f, 6.99f, 5, 7) == 4 * 7 + 0);
    CHECK(path_cell_of(2.5f, 3.0f, 5, 7) == 2 * 7 + 3 && path_cell_of(2.5f, 2.99f, 5, 7) == 2 * 7 + 4);
    CHECK(path_cell_of(-0.0f, 0.5f, 5, 7) == 6);
    CHECK(path_cell_of(-0.01f, 0.5f, 5, 7) == -1 && path_cell_of(5.0f, 0.5f, 5, 7) == -1);
    CHECK(path_cell_of(0.5f, -0.01f, 5, 7) == -1 && path_cell_of(0.5f, 7.0f, 5, 7) == -1);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (float bad : {inf, -inf, nan, 3e38f, -3e38f, 4294967296.0f})
        CHECK(path_cell_of(bad, 0.5f, 64, 64) == -1 && path_cell_of(0.5f, bad, 64, 64) == -1);
    for (int x = 0; x < 64; x++)
        for (int y = 0; y < 64; y++) CHECK(path_cell_of(float(x) + 0.25f, float(63 - y) + 0.75f, 64, 64) == y + x * 64);
    CHECK(pg::path_given_cell(-1, 10) == -1 && pg::path_given_cell(10, 10) == -1 && pg::path_given_cell(0, 10) == 0 && pg::path_given_cell(9, 10) == 9);
    CHECK(pg::path_given_cell(std::numeric_limits<int32_t>::min(), 10) == -1 && pg::path_given_cell(std::numeric_limits<int32_t>::max(), 10) == -1);
    CHECK(!pg::path_passable(0xFFFFFFFFu, 32u) && !pg::path_passable(0xFFFFFFFFu, 255u) && pg::path_passable(0x80000000u, 31u) && !pg::path_passable(0u, 0u));
    std::printf("OK cells\n");
    return 0;
}

int main() {
    if (test_random_boards() || test_open_boards() || test_special_cases() || test_cells()) return 1;
    std::printf("ALL OK\n");
    return 0;
}
