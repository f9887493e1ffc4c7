// CPU check of the two frame painters' shared raster code (procgen2_amd/csrc/pg_raster.h compiled for the host):
//   (a) random integer draw lists painted whole onto a W×H array,
//   (b) the same lists painted tile by tile (64×64 tiles, 256 emulated threads) and assembled, both as words and through
//       the packed-RGB row stores at an awkward base address,
//   (c) the oracle's spec_blit / spec_blit_rotated (oracle/pgo_raster.cpp, compiled into this executable).
// (a) == (b) word for word, (a) == (c) on R, G, B.  Built and run by tests/test_frame_tiles.py; prints "OK <name>" per
// section, exits non-zero on failure.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "pg_raster.h"
#include "pgo_raster.h"

static int fails = 0;
#define CHECK(cond, ...)                    \
    do {                                    \
        if (!(cond)) {                      \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");              \
            if (++fails > 10) std::exit(1); \
        }                                   \
    } while (0)

static std::mt19937 rng(20240607u);
static int pick(int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); }

struct Tex {
    int w, h, off;
    pgo::Texture ref;
};
static std::vector<uint32_t> atlas;
static std::vector<Tex> textures;

static void make_textures() {
    const int sizes[][2] = {{1, 1}, {7, 5}, {16, 16}, {64, 53}, {128, 256}, {300, 200}, {30, 6}};
    for (const auto& s : sizes) {
        Tex t;
        t.w = s[0];
        t.h = s[1];
        t.off = static_cast<int>(atlas.size());
        t.ref.w = t.w;
        t.ref.h = t.h;
        for (int k = 0; k < t.w * t.h; k++) {
            const int kind = pick(0, 3);
            const uint32_t a = kind == 0 ? 0u : kind == 1 ? 255u : static_cast<uint32_t>(pick(1, 254));
            const uint32_t r = pick(0, 255), g = pick(0, 255), b = pick(0, 255);
            atlas.push_back(r | g << 8 | b << 16 | a << 24);
            t.ref.rgba.push_back(static_cast<uint8_t>(r));
            t.ref.rgba.push_back(static_cast<uint8_t>(g));
            t.ref.rgba.push_back(static_cast<uint8_t>(b));
            t.ref.rgba.push_back(static_cast<uint8_t>(a));
        }
        textures.push_back(t);
    }
}

struct Draw {
    pg::Blit b;
    int tex;
    double deg;  // rotated draws: the angle the oracle is given
};

// One draw somewhere around a w×h frame: overlapping its neighbours, hanging over any edge, sometimes larger than the
// frame, sometimes a single pixel; flipped, alpha-modulated or rotated.
static Draw random_draw(int w, int h) {
    Draw d;
    d.tex = pick(0, static_cast<int>(textures.size()) - 1);
    const Tex& t = textures[d.tex];
    pg::Blit& b = d.b;
    const int shape = pick(0, 9);
    if (shape == 0) {
        b.dw = b.dh = 1;
    } else if (shape == 1) {  // larger than the frame
        b.dw = w + pick(1, 2 * w + 40);
        b.dh = h + pick(1, 2 * h + 40);
    } else {
        b.dw = pick(1, w + 20);
        b.dh = pick(1, h + 20);
    }
    b.dx = pick(-b.dw - 3, w + 3);
    b.dy = pick(-b.dh - 3, h + 3);
    if (shape == 1) {
        b.dx = pick(-b.dw / 2 - 5, 5);
        b.dy = pick(-b.dh / 2 - 5, 5);
    }
    b.tex_off = t.off;
    b.tex_w = t.w;
    int mod = pick(0, 2) == 0 ? pick(0, 254) : 255;
    b.rot_sn = 0;
    b.rot_cs = 65536;
    d.deg = 0.0;
    if (pick(0, 3) == 0) {  // S6: whole texture, no flip
        if (b.dw > 1500) b.dw = 1500;  // (the oracle scans the whole reach square: keep that affordable)
        if (b.dh > 1500) b.dh = 1500;
        b.sx = b.sy = 0;
        b.sw = t.w;
        b.sh = t.h;
        d.deg = pick(0, 5) == 0 ? 90.0 * pick(1, 3) : pick(-7200, 7200) / 10.0 + 0.05;
        const float theta = static_cast<float>(d.deg * (3.14159265358979323846 / 180.0));
        b.rot_sn = static_cast<int>(std::floor(static_cast<double>(sinf(theta)) * 65536.0 + 0.5));
        b.rot_cs = static_cast<int>(std::floor(static_cast<double>(cosf(theta)) * 65536.0 + 0.5));
        b.flip_mod = mod | pg::kRotated;
    } else {
        b.sx = pick(0, t.w - 1);
        b.sy = pick(0, t.h - 1);
        b.sw = pick(1, t.w - b.sx);
        b.sh = pick(1, t.h - b.sy);
        const int flip = pick(0, 3);
        b.flip_mod = mod | (flip == 1 ? pg::kFlipH : flip == 2 ? pg::kFlipV : 0);
    }
    return d;
}

static void paint_by(const pg::Blit& b, const pg::PixRect& r, uint32_t* px, int pitch, int ox, int oy, int nt) {
    for (int tid = 0; tid < nt; tid++) pg::paint_rect(b, atlas.data(), r, px, pitch, ox, oy, tid, nt);
}

static void test_size(int w, int h, int n_draws) {
    std::vector<Draw> list;
    for (int k = 0; k < n_draws; k++) list.push_back(random_draw(w, h));

    // (a) whole, one thread — and once more with 256, which must not matter
    const pg::PixRect frame{0, 0, w - 1, h - 1};
    std::vector<uint32_t> whole(size_t(w) * h, 0u), whole256(size_t(w) * h, 0u);
    for (const Draw& d : list) {
        pg::PixRect r = pg::draw_reach(d.b);
        if (!pg::rect_clip(r, frame)) continue;
        paint_by(d.b, r, whole.data(), w, 0, 0, 1);
        paint_by(d.b, r, whole256.data(), w, 0, 0, 256);
    }
    CHECK(whole == whole256, "%dx%d: the whole frame depends on the thread count", w, h);

    // (b) tile by tile; each tile leaves as words and as packed RGB rows
    const int tiles = pg::tiles_across(w) * pg::tiles_across(h);
    std::vector<uint32_t> tiled(size_t(w) * h, 0xdeadbeefu);
    const int skew = pick(0, 15);  // the frame's first byte sits at any alignment
    std::vector<uint8_t> rgb(size_t(w) * h * 3 + 32, 0xa5);
    std::vector<int> written(rgb.size(), 0);
    for (int t = 0; t < tiles; t++) {
        const pg::PixRect at = pg::tile_rect(w, h, t);
        uint32_t lds[pg::kTilePx];
        for (auto& v : lds) v = 0u;
        for (const Draw& d : list) {
            pg::PixRect r = pg::draw_reach(d.b);
            if (!pg::rect_clip(r, at)) continue;
            paint_by(d.b, r, lds, pg::kTile, at.x0, at.y0, 256);
        }
        const int last = at.x1 - at.x0, nb = 3 * (last + 1);
        for (int row = 0; row <= at.y1 - at.y0; row++) {
            for (int x = 0; x <= last; x++) tiled[size_t(at.y0 + row) * w + at.x0 + x] = lds[row * pg::kTile + x];
            const size_t at_byte = skew + (size_t(at.y0 + row) * w + at.x0) * 3;
            const pg::RowPlan plan = pg::row_plan(static_cast<uint32_t>(at_byte), nb);
            for (int slot = 0; slot < pg::kRowSlots; slot++) {
                int off;
                const int width = pg::row_slot(plan, slot, off);
                if (!width) continue;
                CHECK((at_byte + off) % width == 0, "%dx%d tile %d row %d slot %d: a %d-byte store at a misaligned address", w, h, t, row, slot, width);
                CHECK(off >= 0 && off + width <= nb, "%dx%d tile %d row %d slot %d: store outside the row", w, h, t, row, slot);
                for (int k = 0; k < width; k += 4) {
                    const uint32_t word = pg::row_word(lds + row * pg::kTile, off + k, last);
                    for (int c = 0; c < (width == 1 ? 1 : 4); c++) {
                        rgb[at_byte + off + k + c] = static_cast<uint8_t>(word >> (8 * c));
                        written[at_byte + off + k + c]++;
                    }
                }
            }
        }
    }
    CHECK(tiled == whole, "%dx%d: tile by tile differs from the whole frame", w, h);
    for (size_t k = 0; k < size_t(w) * h; k++)
        if (tiled[k] != whole[k]) {
            CHECK(false, "%dx%d: first differing pixel (%d, %d): tiled %08x whole %08x", w, h, int(k % w), int(k / w), tiled[k], whole[k]);
            break;
        }
    bool rows_ok = true;
    for (size_t k = 0; k < rgb.size() && rows_ok; k++) {
        const bool inside = k >= size_t(skew) && k < skew + size_t(w) * h * 3;
        if (!inside) {
            rows_ok = written[k] == 0 && rgb[k] == 0xa5;
        } else {
            const size_t j = k - skew;
            rows_ok = written[k] == 1 && rgb[k] == static_cast<uint8_t>(whole[j / 3] >> (8 * (j % 3)));
        }
        CHECK(rows_ok, "%dx%d: packed RGB byte %zu (skew %d) written %d times or wrong", w, h, k, skew, written[k]);
    }

    // (c) the oracle's statement of the spec
    pgo::Surface ref(w, h);
    ref.clear_black();
    for (const Draw& d : list) {
        const pg::Blit& b = d.b;
        const int flip = (b.flip_mod & pg::kFlipH) ? pgo::kFlipH : (b.flip_mod & pg::kFlipV) ? pgo::kFlipV : pgo::kFlipNone;
        pgo::spec_blit(ref, textures[d.tex].ref, float(b.sx), float(b.sy), float(b.sw), float(b.sh), float(b.dx), float(b.dy),
                       float(b.dw), float(b.dh), d.deg, flip, b.flip_mod & 0xff);
    }
    for (size_t k = 0; k < size_t(w) * h; k++) {
        const uint32_t want = ref.px[4 * k] | ref.px[4 * k + 1] << 8 | ref.px[4 * k + 2] << 16;
        if (whole[k] != want) {
            CHECK(false, "%dx%d: pixel (%d, %d) is %06x, the oracle's spec_blit says %06x", w, h, int(k % w), int(k / w), whole[k], want);
            break;
        }
    }
    std::printf("OK frame %dx%d (%d draws, %d tiles)\n", w, h, n_draws, tiles);
}

// Every alignment and every row length: each byte stored exactly once, by an aligned store, with the right value.
static void test_row_plans() {
    uint32_t row[pg::kTile];
    for (auto& v : row) v = static_cast<uint32_t>(rng()) & 0x00ffffffu;
    for (uint32_t addr = 0; addr < 32; addr++)
        for (int pixels = 1; pixels <= pg::kTile; pixels++) {
            const int nb = 3 * pixels;
            int count[3 * pg::kTile] = {0};
            const pg::RowPlan p = pg::row_plan(addr, nb);
            CHECK(p.head + 4 * p.lead + 16 * p.body + 4 * p.trail + p.tail == nb, "row plan addr %u nb %d does not add up", addr, nb);
            CHECK(p.body <= 12 && p.lead <= 3 && p.trail <= 3 && p.head <= 3 && p.tail <= 3, "row plan addr %u nb %d: too many pieces", addr, nb);
            for (int slot = 0; slot < pg::kRowSlots; slot++) {
                int off;
                const int width = pg::row_slot(p, slot, off);
                if (!width) continue;
                CHECK((addr + off) % width == 0, "row plan addr %u nb %d slot %d misaligned", addr, nb, slot);
                for (int k = 0; k < width; k++) {
                    const int j = off + k;
                    CHECK(j >= 0 && j < nb, "row plan addr %u nb %d slot %d outside", addr, nb, slot);
                    count[j]++;
                    const uint32_t word = pg::row_word(row, off + (k & ~3), pixels - 1);
                    CHECK(static_cast<uint8_t>(word >> (8 * (k & 3))) == static_cast<uint8_t>(row[j / 3] >> (8 * (j % 3))),
                          "row word addr %u nb %d byte %d", addr, nb, j);
                }
            }
            for (int j = 0; j < nb; j++) CHECK(count[j] == 1, "row plan addr %u nb %d: byte %d stored %d times", addr, nb, j, count[j]);
        }
    std::printf("OK row plans\n");
}

// S3 in 32 bits where it fits equals S3 in 64 bits.
static void test_sample_at() {
    for (int k = 0; k < 2000000; k++) {
        const int n = pick(1, 32767), len = pick(1, (1 << 30) / n > 4096 ? 4096 : (1 << 30) / n), i = pick(0, n - 1);
        CHECK(pg::sample_at(i, len, n, true) == pg::sample_at(i, len, n, false), "sample_at(%d, %d, %d)", i, len, n);
    }
    std::printf("OK sample index\n");
}

// A batch cut into launches of at most `limit` blocks: every (frame, tile) is painted exactly once, whatever the limit.
static void test_launch_split() {
    const long long limits[] = {1, 7, 64, 4095, 4096, 1LL << 24, 1LL << 40};
    for (int count : {1, 3, 9, 1000})
        for (int tiles : {1, 2, 8, 64, 4096})
            for (long long limit : limits) {
                const long long total = static_cast<long long>(count) * tiles;
                std::vector<uint8_t> seen(static_cast<size_t>(total), 0);
                long long launches = 0;
                for (long long b0 = 0; b0 < total; b0 += limit, launches++) {
                    const long long blocks = pg::launch_blocks(total, b0, limit);
                    CHECK(blocks >= 1 && blocks <= limit, "launch of %lld blocks under a limit of %lld", blocks, limit);
                    for (long long k = 0; k < blocks; k++) {
                        int frame, tile;
                        pg::block_place(b0 + k, tiles, frame, tile);
                        CHECK(frame >= 0 && frame < count && tile >= 0 && tile < tiles, "block %lld lands outside the batch", b0 + k);
                        seen[static_cast<size_t>(frame) * tiles + tile]++;
                    }
                }
                CHECK(launches == (total + limit - 1) / limit, "%lld launches for %lld blocks under a limit of %lld", launches, total, limit);
                for (uint8_t v : seen) CHECK(v == 1, "count %d tiles %d limit %lld: a tile painted %d times", count, tiles, limit, v);
            }
    // the largest batch the ABI allows: 65 536 envs of 4096 × 4096, 2^28 blocks
    int frame, tile;
    pg::block_place((1LL << 28) - 1, 4096, frame, tile);
    CHECK(frame == 65535 && tile == 4095, "the last block of the largest batch");
    std::printf("OK launch split\n");
}

int main() {
    make_textures();
    test_launch_split();
    test_row_plans();
    test_sample_at();
    const int sizes[][2] = {{64, 64}, {65, 63}, {131, 77}, {200, 120}, {512, 512}, {1, 1}, {128, 128}, {63, 200}, {3, 2}};
    for (const auto& s : sizes)
        for (int round = 0; round < 3; round++) test_size(s[0], s[1], 40 + 20 * round);
    if (fails) {
        std::printf("%d FAILURES\n", fails);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
