// The raster spec at ONE pixel of a W×H frame, and the cutting of a frame into 64×64 tiles: what the two painters of
// pg_frame.h share.  Like pg_geom.h this is plain `PG_HD` arithmetic with no HIP runtime in it, so g++ compiles the very
// same statements for tests/cpp/test_frame_tiles.cpp, which checks them against oracle/pgo_raster.cpp.
//
//   draw_reach    the pixels a resolved draw may touch (S5 not yet applied); a rotated draw (S6): the conservative
//                 square the spec scans
//   rect_clip     intersection of two inclusive rectangles (the frame's, a tile's)
//   paint_rect    threads tid, tid + nt, … of a group rasterise a draw over a rectangle: rotation in 16.16 (S6), sample
//                 index (S3), blend (S4) — into a target of 0x00BBGGRR words with any origin and pitch
//   launch_blocks / block_place   a batch's (frame, tile) pairs dealt to the blocks of one or several launches
//   row_plan / row_slot / row_word   a tile row's packed RGB bytes on their way to an address of any alignment
#pragma once

#include "pg_geom.h"

namespace pg {

constexpr int kTile = 64;                // a tile is kTile × kTile pixels: 16 KiB of LDS, the observation path's size
constexpr int kTilePx = kTile * kTile;

struct PixRect {
    int x0, y0, x1, y1;  // inclusive; empty when x1 < x0 or y1 < y0
};

PG_HD PixRect draw_reach(const Blit& b) {
    PixRect r;
    if (b.flip_mod & kRotated) {
        long long reach = 1;
        const long long diag2 = (long long)b.dw * b.dw + (long long)b.dh * b.dh;
        while (reach * reach * 4 < diag2) reach++;
        reach += 1;
        const long long cx2 = 2LL * b.dx + b.dw, cy2 = 2LL * b.dy + b.dh;
        r.x0 = static_cast<int>((cx2 - 2 * reach) / 2 - 1);
        r.x1 = static_cast<int>((cx2 + 2 * reach) / 2 + 1);
        r.y0 = static_cast<int>((cy2 - 2 * reach) / 2 - 1);
        r.y1 = static_cast<int>((cy2 + 2 * reach) / 2 + 1);
    } else {
        r.x0 = b.dx;
        r.y0 = b.dy;
        r.x1 = b.dx + b.dw - 1;
        r.y1 = b.dy + b.dh - 1;
    }
    return r;
}

PG_HD bool rect_clip(PixRect& r, const PixRect& to) {
    if (r.x0 < to.x0) r.x0 = to.x0;
    if (r.y0 < to.y0) r.y0 = to.y0;
    if (r.x1 > to.x1) r.x1 = to.x1;
    if (r.y1 > to.y1) r.y1 = to.y1;
    return r.x1 >= r.x0 && r.y1 >= r.y0;
}

// Tile `t` of a w×h frame, tiles numbered row by row; the right and bottom ones are partial when w or h is no multiple of 64.
PG_HD int tiles_across(int len) { return (len + kTile - 1) / kTile; }
PG_HD PixRect tile_rect(int w, int h, int t) {
    const int tx = t % tiles_across(w), ty = t / tiles_across(w);
    PixRect r{tx * kTile, ty * kTile, tx * kTile + kTile - 1, ty * kTile + kTile - 1};
    if (r.x1 > w - 1) r.x1 = w - 1;
    if (r.y1 > h - 1) r.y1 = h - 1;
    return r;
}

// A batch of frames is count · tiles blocks, numbered frame by frame; a batch too big for one grid goes out in launches of
// at most `limit` blocks, each told its first block b0.  How many blocks the launch at b0 has, and where block b paints.
PG_HD long long launch_blocks(long long total, long long b0, long long limit) { return total - b0 < limit ? total - b0 : limit; }
PG_HD void block_place(long long b, int tiles, int& frame, int& tile) {
    frame = static_cast<int>(b / tiles);
    tile = static_cast<int>(b - static_cast<long long>(frame) * tiles);
}

// S3, floor(((2i + 1)·len) / (2n)): in 32 bits where the caller has seen that 2·n·len fits (`narrow`), which is every
// draw a game makes; the quotient is the same either way.
PG_HD int sample_at(int i, int len, int n, bool narrow) {
    if (narrow) return static_cast<int>((static_cast<uint32_t>(2 * i + 1) * static_cast<uint32_t>(len)) / static_cast<uint32_t>(2 * n));
    return static_cast<int>(((2LL * i + 1) * len) / (2LL * n));
}

// One resolved draw at frame pixel (X, Y), whose word is *d.
PG_HD void paint_pixel(const Blit& b, const uint32_t* texels, bool narrow, int X, int Y, uint32_t* d) {
    int i, j;
    if (b.flip_mod & kRotated) {
        const long long px = 2LL * (X - b.dx) + 1 - b.dw, py = 2LL * (Y - b.dy) + 1 - b.dh;
        const long long lx = px * b.rot_cs + py * b.rot_sn + (long long)b.dw * 65536;
        const long long ly = -px * b.rot_sn + py * b.rot_cs + (long long)b.dh * 65536;
        if (lx < 0 || ly < 0 || lx >= 2LL * b.dw * 65536 || ly >= 2LL * b.dh * 65536) return;
        i = static_cast<int>(lx >> 17);
        j = static_cast<int>(ly >> 17);
    } else {
        i = X - b.dx;
        j = Y - b.dy;
        if (b.flip_mod & kFlipH) i = b.dw - 1 - i;
        if (b.flip_mod & kFlipV) j = b.dh - 1 - j;
    }
    const int u = b.sx + sample_at(i, b.sw, b.dw, narrow);
    const int v = b.sy + sample_at(j, b.sh, b.dh, narrow);
    const uint32_t texel = texels[b.tex_off + v * b.tex_w + u];
    const int mod = b.flip_mod & 0xff;
    int a = static_cast<int>(texel >> 24);
    if (mod != 255) a = static_cast<int>(div255(static_cast<uint32_t>(a * mod)));
    if (a == 0) return;
    *d = blend_px(*d, texel, a);
}

// The draw over the rectangle r (already clipped: to the frame, or to a tile of it), by thread `tid` of `nt`.  Pixel (X, Y)
// of the frame is px[(Y − oy)·pitch + (X − ox)].  r has at most 4096 × 4096 pixels, so the counts fit an int; the walk
// steps row and column along instead of dividing once a pixel.
PG_HD void paint_rect(const Blit& b, const uint32_t* texels, const PixRect& r, uint32_t* px, int pitch, int ox, int oy,
                      int tid, int nt) {
    const int fw = r.x1 - r.x0 + 1, fh = r.y1 - r.y0 + 1;
    if (fw <= 0 || fh <= 0) return;
    const bool narrow = 2LL * b.dw * b.sw < (1LL << 31) && 2LL * b.dh * b.sh < (1LL << 31);
    const int step_y = nt / fw, step_x = nt - step_y * fw;
    int ry = tid / fw, rx = tid - ry * fw;
    while (ry < fh) {
        const int X = r.x0 + rx, Y = r.y0 + ry;
        paint_pixel(b, texels, narrow, X, Y, &px[(Y - oy) * pitch + (X - ox)]);
        rx += step_x;
        ry += step_y;
        if (rx >= fw) {
            rx -= fw;
            ry++;
        }
    }
}

// ---- a tile row leaves as packed RGB -------------------------------------------------------------------------------
// Bytes `off` … `off + 3` of a row of pixels (0x00BBGGRR words → R, G, B, R, …) as one little-endian word.  `last` is
// the row's last pixel index: a word that ends the row reads no pixel behind it.
PG_HD uint32_t row_word(const uint32_t* row_px, int off, int last) {
    const int q = off / 3, r = off - 3 * q;
    const uint64_t lo = row_px[q] & 0x00ffffffu, hi = row_px[q + 1 <= last ? q + 1 : last] & 0x00ffffffu;
    return static_cast<uint32_t>((lo | hi << 24) >> (8 * r));
}

// nb bytes for an address with low bits `addr`: byte stores up to a 4-byte boundary, words up to a 16-byte boundary,
// 16-byte stores, then words and bytes again for what is left (W·3 need not be a multiple of 4, so every row of a frame
// may start at a different alignment).
struct RowPlan {
    int head, lead, body, trail, tail;  // counts: bytes, words, 16-byte pieces, words, bytes
};
PG_HD RowPlan row_plan(uint32_t addr, int nb) {
    RowPlan p;
    p.head = static_cast<int>((4u - (addr & 3u)) & 3u);
    if (p.head > nb) p.head = nb;
    int pos = p.head;
    p.lead = static_cast<int>(((16u - ((addr + pos) & 15u)) & 15u) >> 2);
    if (p.lead > (nb - pos) / 4) p.lead = (nb - pos) / 4;
    pos += 4 * p.lead;
    p.body = (nb - pos) / 16;
    pos += 16 * p.body;
    p.trail = (nb - pos) / 4;
    pos += 4 * p.trail;
    p.tail = nb - pos;
    return p;
}
// A row has kRowSlots jobs, one per lane: 12 pieces of 16 bytes (a full row is 192 bytes), 3 + 3 words, 3 + 3 bytes.
// Slot → byte offset in the row and width of its store; width 0 = nothing to do.
constexpr int kRowSlots = 32;
PG_HD int row_slot(const RowPlan& p, int slot, int& off) {
    const int lead_at = p.head, body_at = lead_at + 4 * p.lead, trail_at = body_at + 16 * p.body,
              tail_at = trail_at + 4 * p.trail;
    if (slot < 12) {
        off = body_at + 16 * slot;
        return slot < p.body ? 16 : 0;
    }
    if (slot < 15) {
        off = lead_at + 4 * (slot - 12);
        return slot - 12 < p.lead ? 4 : 0;
    }
    if (slot < 18) {
        off = trail_at + 4 * (slot - 15);
        return slot - 15 < p.trail ? 4 : 0;
    }
    if (slot < 21) {
        off = slot - 18;
        return slot - 18 < p.head ? 1 : 0;
    }
    if (slot < 24) {
        off = tail_at + (slot - 21);
        return slot - 21 < p.tail ? 1 : 0;
    }
    off = 0;
    return 0;
}

}  // namespace pg
