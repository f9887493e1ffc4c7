// The host half of the augmented history gathers (procgen2_amd/csrc/pg_history_aug.h) compiled for the CPU: the draws against
// a transcription of the header's formulas, aug_source_byte_index against the three cases of the header written out, for
// every window an entry can draw, and the output offset arithmetic.
// Prints "OK <section>" per section and "ALL OK"; exit status 1 on the first failure.
#include <cstdio>
#include <vector>

#include "pg_history_aug.h"

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                   \
        }                                                               \
    } while (0)

// (H', W', pad, cutout_min, cutout_max): the configurations of tests/history_aug_util.py
static const int kConfigs[7][5] = {{64, 64, 4, 0, 0}, {56, 56, 0, 4, 24}, {8, 8, 16, 1, 1}, {1, 8, 0, 0, 0}, {63, 24, 1, 24, 40}, {64, 64, 0, 64, 64}, {33, 40, 16, 8, 8}};

static pg::AugConfig config_of(int k, int edge, int colour, uint32_t seed) {
    return pg::AugConfig{kConfigs[k][0], kConfigs[k][1], kConfigs[k][2], edge, kConfigs[k][3], kConfigs[k][4], colour, seed};
}

// include/procgen2_vec.h, point 2 of the augmented gathers, written down again
static uint32_t t_mix(uint32_t x) {
    x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
    return x;
}
static uint32_t t_word(uint32_t seed, uint32_t e, uint32_t j) { return t_mix(t_mix(seed + 0x9E3779B9u * (e + 1u)) ^ (j * 0x85EBCA6Bu + 0xC2B2AE35u)); }
static int t_draw(uint32_t seed, uint32_t e, int m, uint32_t j) { return int((uint64_t(t_word(seed, e, j)) * uint64_t(m)) >> 32); }

static int test_draws() {
    using namespace pg;
    CHECK(mix32(0u) == 0u && mix32(1u) == t_mix(1u) && mix32(0xFFFFFFFFu) == t_mix(0xFFFFFFFFu));
    const uint32_t seeds[3] = {0u, 1u, 0xFFFFFFFFu};
    long rows = 0;
    for (int k = 0; k < 7; k++)
        for (uint32_t seed : seeds)
            for (int colour = 0; colour < 2; colour++)
                for (uint32_t e = 0; e < 4096; e++) {
                    const AugConfig a = config_of(k, kAugEdgeReplicate, colour, seed);
                    CHECK(aug_config_error(a) == nullptr);
                    const AugParams p = aug_params(a, e);
                    const int H = a.out_h, W = a.out_w, pad = a.pad, lo = a.cutout_min, hi = a.cutout_max;
                    CHECK(p.oy == -pad + t_draw(seed, e, 64 + 2 * pad - H + 1, 0) && p.ox == -pad + t_draw(seed, e, 64 + 2 * pad - W + 1, 1));
                    CHECK(p.oy >= -pad && p.oy + H <= 64 + pad && p.ox >= -pad && p.ox + W <= 64 + pad);
                    if (hi > 0) {
                        int ch = lo + t_draw(seed, e, hi - lo + 1, 2), cw = lo + t_draw(seed, e, hi - lo + 1, 3);
                        ch = ch < H ? ch : H, cw = cw < W ? cw : W;
                        CHECK(p.ch == ch && p.cw == cw && p.cy == t_draw(seed, e, H - ch + 1, 4) && p.cx == t_draw(seed, e, W - cw + 1, 5));
                        CHECK(p.ch >= 1 && p.cw >= 1 && p.cy >= 0 && p.cx >= 0 && p.cy + p.ch <= H && p.cx + p.cw <= W);
                        CHECK(p.colour == (colour ? t_word(seed, e, 6) : 0u));
                    } else
                        CHECK(p.ch == 0 && p.cw == 0 && p.cy == 0 && p.cx == 0 && p.colour == 0u);
                    int32_t row[8], gray[8];
                    aug_params_row(p, 3, row), aug_params_row(p, 1, gray);
                    CHECK(row[0] == p.oy && row[1] == p.ox && row[2] == p.cy && row[3] == p.cx && row[4] == p.ch && row[5] == p.cw && row[7] == 0);
                    CHECK(uint32_t(row[6]) == (p.colour & 0xFFFFFFu) && uint32_t(gray[6]) == (p.colour & 0xFFu) && gray[7] == 0);
                    rows++;
                }
    // a draw reaches both ends of its range and never m
    int low = 0, high = 0;
    for (uint32_t e = 0; e < 4096; e++) {
        const int d = aug_draw(1u, e, 9u, 0u);
        CHECK(d >= 0 && d < 9);
        low += d == 0, high += d == 8;
    }
    CHECK(low > 0 && high > 0 && aug_draw(5u, 5u, 1u, 3u) == 0);
    // what the host refuses
    AugConfig a = config_of(1, 0, 0, 1u);
    CHECK(!aug_config_error(a));
    AugConfig b = a; b.out_h = 0; CHECK(aug_config_error(b)); b.out_h = 65; CHECK(aug_config_error(b));
    b = a; b.out_w = 0; CHECK(aug_config_error(b)); b.out_w = 12; CHECK(aug_config_error(b)); b.out_w = 72; CHECK(aug_config_error(b));
    b = a; b.pad = -1; CHECK(aug_config_error(b)); b.pad = 17; CHECK(aug_config_error(b));
    b = a; b.edge = 2; CHECK(aug_config_error(b)); b = a; b.cutout_color = 2; CHECK(aug_config_error(b));
    b = a; b.cutout_min = 25; CHECK(aug_config_error(b)); b.cutout_min = 0; CHECK(aug_config_error(b));
    b = a; b.cutout_max = 65; CHECK(aug_config_error(b)); b.cutout_min = -1, b.cutout_max = 0; CHECK(aug_config_error(b));
    std::printf("OK draws (%ld rows)\n", rows);
    return 0;
}

// Every output pixel of every window and a rectangle in each corner and the middle, both edges, against the header's three
// cases; every index a byte of the plane or a sentinel.
static int test_source_index() {
    using namespace pg;
    long pixels = 0;
    for (int k = 0; k < 7; k++) {
        const int H = kConfigs[k][0], W = kConfigs[k][1], pad = kConfigs[k][2], lo = kConfigs[k][3], hi = kConfigs[k][4];
        std::vector<AugParams> cuts;
        if (hi == 0)
            cuts.push_back(AugParams{0, 0, 0, 0, 0, 0, 0u});
        else
            for (int side : {lo, hi}) {
                const int ch = side < H ? side : H, cw = side < W ? side : W;
                cuts.push_back(AugParams{0, 0, 0, 0, ch, cw, 0u});
                cuts.push_back(AugParams{0, 0, H - ch, W - cw, ch, cw, 0u});
                cuts.push_back(AugParams{0, 0, (H - ch) / 2, (W - cw) / 2, ch, cw, 0u});
            }
        for (int oy = -pad; oy <= 64 + pad - H; oy++)
            for (int ox = -pad; ox <= 64 + pad - W; ox++)
                for (AugParams p : cuts) {
                    p.oy = oy, p.ox = ox;
                    for (int edge = 0; edge < 2; edge++)
                        for (int y = 0; y < H; y++)
                            for (int x = 0; x < W; x++) {
                                const int got = aug_source_byte_index(p, edge, y, x);
                                CHECK((got >= 0 && got < 4096) || got == kAugZero || got == kAugCutout);
                                int want;
                                if (p.cy <= y && y < p.cy + p.ch && p.cx <= x && x < p.cx + p.cw)
                                    want = -2;
                                else {
                                    const int sy = oy + y, sx = ox + x;
                                    if (0 <= sy && sy <= 63 && 0 <= sx && sx <= 63)
                                        want = sy * 64 + sx;
                                    else if (edge == kAugEdgeZero)
                                        want = -1;
                                    else
                                        want = (sy < 0 ? 0 : sy > 63 ? 63 : sy) * 64 + (sx < 0 ? 0 : sx > 63 ? 63 : sx);
                                }
                                CHECK(got == want);
                                pixels++;
                            }
                }
    }
    CHECK(kAugZero == -1 && kAugCutout == -2 && pixels > 1000000);
    std::printf("OK source index (%ld pixels)\n", pixels);
    return 0;
}

// Units tile a plane, planes a row, rows the buffer: in order, without a gap, and the last byte is the buffer's last.
static int test_offsets() {
    using namespace pg;
    for (int k = 0; k < 7; k++)
        for (int es : {1, 2, 4})
            for (int planes : {1, 3})
                for (int stack : {1, 3, 8}) {
                    const int H = kConfigs[k][0], W = kConfigs[k][1], U = aug_unit_bytes(H, W, es), count = 3;
                    const size_t plane = aug_plane_bytes(H, W, es);
                    CHECK(plane == size_t(H) * W * es && (U == 16 || U == 8) && plane % U == 0 && (U == 16) == (plane % 16 == 0));
                    CHECK(aug_row_bytes(stack, planes, H, W, es) == plane * stack * planes);
                    const int units = int(plane / U);
                    size_t expect = 0;
                    for (size_t entry = 0; entry < size_t(count); entry++)
                        for (int ch = 0; ch < stack * planes; ch++)
                            for (int u = 0; u < units; u++, expect += U) {
                                const size_t at = aug_unit_offset(entry, stack, planes, H, W, es, ch, u, U);
                                CHECK(at == expect && at % U == 0);
                            }
                    CHECK(expect - 1 == size_t(count) * stack * planes * H * W * es - 1);
                }
    // rows that are 8 mod 16 bytes: 63 x 24 at one byte an element, an odd number of planes
    CHECK(aug_unit_bytes(63, 24, 1) == 8 && aug_row_bytes(1, 3, 63, 24, 1) % 16 == 8 && aug_unit_bytes(63, 24, 2) == 16 && aug_unit_bytes(1, 8, 1) == 8);
    CHECK(aug_unit_bytes(64, 64, 1) == 16 && aug_unit_bytes(56, 56, 2) == 16 && aug_unit_bytes(33, 40, 1) == 8);
    // above 2^32 bytes: 65 536 rows of K = 8, RGB, f32 at 64 x 64
    const int U = aug_unit_bytes(64, 64, 4);
    const size_t last = aug_unit_offset(65535, 8, 3, 64, 64, 4, 23, 64 * 64 * 4 / U - 1, U) + U - 1;
    CHECK(last == size_t(65536) * 8 * 3 * 64 * 64 * 4 - 1 && last > (size_t(1) << 34));
    CHECK(aug_unit_offset(10923, 8, 3, 64, 64, 4, 0, 0, U) > (size_t(1) << 32) && aug_unit_offset(10922, 8, 3, 64, 64, 4, 0, 0, U) < (size_t(1) << 32));
    std::printf("OK offsets\n");
    return 0;
}

int main() {
    if (test_draws() || test_source_index() || test_offsets()) return 1;
    std::printf("ALL OK\n");
    return 0;
}
