// The human-size frame of cenv_render (games/*/<game>.cpp `render_game(false)`): the same draw list as
// the observation, rasterised at W×H with camera_scale = zoom · W / 64.
//
// A game walks its draw list here as `template <class Painter> frame_draws(State, AtlasView, env, Painter&)`, which its
// `Frames` struct hands to the two kernels at the end of this file (frame_kernel<F>, frames_kernel<F>) — the draws
// themselves are the game's own statements (pg_geom.h DrawCall), shared with its observation paths — and reaches the
// target only through the painter's methods (begin, clear, draw, draw_rotated, screen, window, desc, cam, width /
// height, lead).  Two painters take it, with one statement of the raster spec between them (pg_raster.h, which the
// host tests compile too):
//
//   FramePainter  ONE env, one workgroup, a W×H target of 0x00BBGGRR words in global memory: pgv_render_frame, the
//                 debugging / viewer path ("a frame per keystroke"), deliberately plain — every draw resolved by all
//                 threads (uniform arguments → uniform control flow) and rasterised by all of them, a barrier after it.
//   TilePainter   one 64×64 tile of one env's frame in LDS, one workgroup per (frame, tile): pgv_render_frames, many
//                 envs at any size into the caller's u8 [K][H][W][3] on the device.  The camera is the whole frame's, so
//                 a draw resolves to exactly the numbers FramePainter sees; only the rasterised region is cut.  A draw
//                 that does not reach the tile returns before any barrier (its arguments are uniform over the workgroup,
//                 so the decision is); the others stride over their intersection with the tile.  The tile leaves as packed
//                 RGB with the widest stores each row's alignment allows.  Every tile walks the whole draw list: the
//                 tile-layer window is NOT narrowed per tile (padding, D8 / S2, lets a cell a little outside the naive
//                 range reach in; the early return already makes a draw that misses cost its resolve and nothing else).
#pragma once

#include "pg_engine.h"
#include "pg_geom.h"
#include "pg_raster.h"
#include "pg_sincos.h"

namespace pg {

constexpr int kFrameThreads = 256;

struct FrameTarget {
    uint32_t* px;  // [h][w]
    int w, h;
};

// The calls of a draw list that do not depend on where the pixels go: Derived supplies blit(), clear(), width(), height(), lead().
template <class Derived>
struct PainterCalls {
    AtlasView atlas;
    Camera cam;

    PG_D Derived& self() { return *static_cast<Derived*>(this); }
    PG_D int4 desc(int tex) const { return atlas.desc[tex]; }
    // First call of a draw list: the game's camera for this frame (its size is the painter's width() × height()).
    PG_D void begin(const AtlasView& a, const Camera& c) {
        atlas = a;
        cam = c;
    }

    // Renderer::render_texture (renderer.cpp:5-82)
    PG_D void draw(int tex, float px, float py, float scale, float alpha = 1.0f, bool flip_h = false,
                   bool flip_v = false) {
        const int4 d = desc(tex);
        Blit b;
        if (resolve_draw(cam, d.y, d.z, d.x, px, py, scale, alpha, flip_h, flip_v, b)) self().blit(b);
    }
    // Renderer::render_texture_rotated (renderer.cpp:84-101)
    PG_D void draw_rotated(int tex, float px, float py, float rotation, float scale, float alpha = 1.0f) {
        const int4 d = desc(tex);
        const float dx = (px - cam.px) * cam.scale + cam.sw * 0.5f;
        const float dy = (py - cam.py) * cam.scale + cam.sh * 0.5f;
        const float dw = d.y * scale * cam.scale;
        const float dh = d.z * scale * cam.scale;
        int mod = 255;
        if (alpha != 1.0f) mod = static_cast<int>(255 * alpha) & 0xff;
        const double deg = rotation * 180.0f / 3.14159265358979323846;
        screen(tex, dx, dy, dw, dh, deg, mod);
    }
    // A raw SDL_RenderTextureRotated in screen space: whole texture, float destination, `deg` degrees about its centre.
    PG_D void screen(int tex, float dx, float dy, float dw, float dh, double deg, int mod = 255) {
        const int4 d = desc(tex);
        if (!(dw >= 1.0f && dh >= 1.0f && dw < 32768.0f && dh < 32768.0f)) return;
        if (!(dx > -32768.0f && dx < 32768.0f && dy > -32768.0f && dy < 32768.0f)) return;
        Blit b;
        b.dx = static_cast<int>(dx);
        b.dy = static_cast<int>(dy);
        b.dw = static_cast<int>(dw);
        b.dh = static_cast<int>(dh);
        b.sx = 0;
        b.sy = 0;
        b.sw = d.y;
        b.sh = d.z;
        b.tex_off = d.x;
        b.tex_w = d.y;
        b.flip_mod = mod;
        b.rot_sn = 0;
        b.rot_cs = 65536;
        if (deg != 0.0) {
            const float theta = static_cast<float>(deg * (3.14159265358979323846 / 180.0));
            b.rot_sn = static_cast<int>(floor(static_cast<double>(sc_sinf(theta)) * 65536.0 + 0.5));
            b.rot_cs = static_cast<int>(floor(static_cast<double>(sc_cosf(theta)) * 65536.0 + 0.5));
            b.flip_mod |= kRotated;
        }
        self().blit(b);
    }
    // One draw of a game's draw list as the game states it (pg_geom.h DrawCall).
    PG_D void draw(const DrawCall& c) {
        if (c.go) draw(c.tex, c.wx, c.wy, c.scale, c.alpha, c.flip_h, c.flip_v);
    }
    PG_D void draw_rotated(const DrawCall& c) {
        if (c.go) draw_rotated(c.tex, c.wx, c.wy, c.rotation, c.scale, c.alpha);
    }
    PG_D TileWindow window() const { return tile_window(cam); }
};

struct FramePainter : PainterCalls<FramePainter> {
    FrameTarget t;
    int tid;

    PG_D explicit FramePainter(const FrameTarget& target) : t(target), tid(static_cast<int>(threadIdx.x)) {}
    PG_D float width() const { return static_cast<float>(t.w); }
    PG_D float height() const { return static_cast<float>(t.h); }
    PG_D bool lead() const { return tid == 0; }  // one thread per rendered frame (bossfight, D15)

    PG_D void clear() {  // SDL_RenderClear with (0,0,0,255)
        for (int k = tid; k < t.w * t.h; k += kFrameThreads) t.px[k] = 0;
        __syncthreads();
    }
    // All threads rasterise one resolved draw (raster spec S3–S6), then meet: the next draw may touch these pixels.
    PG_D void blit(const Blit& b) {
        PixRect r = draw_reach(b);
        if (rect_clip(r, PixRect{0, 0, t.w - 1, t.h - 1})) paint_rect(b, atlas.texels, r, t.px, t.w, 0, 0, tid, kFrameThreads);
        __syncthreads();
    }
};

// One pgv_render_frames launch: block b0 + blockIdx.x paints tile (b % tiles) of frame (b / tiles).
struct FrameBatch {
    const int32_t* indices;  // [count] env of frame k, or nullptr: env k
    uint8_t* rgb;            // [count][h][w][3]
    int w, h, tiles, n;      // tiles per frame; n envs in the batch (an index outside [0, n) gives a frame of zeros)
    long long b0;            // first block of this launch (a batch too big for one grid takes several)
};

struct TilePainter : PainterCalls<TilePainter> {
    uint32_t* tile;  // LDS, [kTile][kTile], pixel (X, Y) of the frame at [(Y − at.y0)·kTile + (X − at.x0)]
    PixRect at;      // the tile's pixels in the frame
    int w, h, tid, frame, index;

    PG_D TilePainter(uint32_t* lds, const FrameBatch& fb) : tile(lds), w(fb.w), h(fb.h), tid(static_cast<int>(threadIdx.x)) {
        block_place(fb.b0 + blockIdx.x, fb.tiles, frame, index);
        at = tile_rect(w, h, index);
    }
    PG_D float width() const { return static_cast<float>(w); }
    PG_D float height() const { return static_cast<float>(h); }
    PG_D bool lead() const { return tid == 0 && index == 0; }  // exactly one thread of one tile per rendered frame

    // The env this workgroup paints, or -1 (tile cleared) for an index outside the batch: never dereferenced.
    PG_D int env(const FrameBatch& fb) {
        const int e = fb.indices ? fb.indices[frame] : frame;
        if (e >= 0 && e < fb.n) return e;
        clear();
        return -1;
    }
    PG_D void clear() {
        for (int k = tid; k < kTilePx; k += kFrameThreads) tile[k] = 0;
        __syncthreads();
    }
    PG_D void blit(const Blit& b) {
        PixRect r = draw_reach(b);
        if (!rect_clip(r, at)) return;  // uniform over the workgroup: nothing written, no barrier needed
        paint_rect(b, atlas.texels, r, tile, kTile, at.x0, at.y0, tid, kFrameThreads);
        __syncthreads();
    }
    // The finished tile into the caller's frame (every clear and blit ended with a barrier): kRowSlots lanes a row, each
    // with one store of the width pg_raster.h row_plan found for its piece of the row.
    PG_D void store(const FrameBatch& fb) const {
        const int rows = at.y1 - at.y0 + 1, last = at.x1 - at.x0, nb = 3 * (last + 1);
        uint8_t* out = fb.rgb + static_cast<size_t>(frame) * h * w * 3;
        for (int k = tid; k < rows * kRowSlots; k += kFrameThreads) {
            const int row = k / kRowSlots, slot = k % kRowSlots;
            uint8_t* dst = out + (static_cast<size_t>(at.y0 + row) * w + at.x0) * 3;
            const uint32_t* src = tile + row * kTile;
            const RowPlan plan = row_plan(static_cast<uint32_t>(reinterpret_cast<uintptr_t>(dst)), nb);
            int off;
            const int width = row_slot(plan, slot, off);
            if (width == 16)
                *reinterpret_cast<uint4*>(dst + off) = make_uint4(row_word(src, off, last), row_word(src, off + 4, last),
                                                                  row_word(src, off + 8, last), row_word(src, off + 12, last));
            else if (width == 4)
                *reinterpret_cast<uint32_t*>(dst + off) = row_word(src, off, last);
            else if (width == 1)
                dst[off] = static_cast<uint8_t>(row_word(src, off, last));
        }
    }
};

// The blocks one launch may have: the device's limit on a grid's first dimension, and the 2^32 threads a grid may hold.
inline long long frame_grid_limit() {
    int dev = 0, most = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&most, hipDeviceAttributeMaxGridDimX, dev) != hipSuccess || most < 1)
        most = 65535;
    long long limit = most;
    if (limit > 0xffffffffLL / kFrameThreads) limit = 0xffffffffLL / kFrameThreads;
    return limit;
}

// The two kernels, once for every game.  F is the game's `Frames`: `using State`, and `draws(s, atlas, env, P)` — its
// frame_draws — as a static member template over the painter.
// One env, one workgroup, a W×H target in global memory: pgv_render_frame.
template <class F>
__global__ void __launch_bounds__(kFrameThreads) frame_kernel(typename F::State s, AtlasView atlas, int env, FrameTarget t) {
    FramePainter P(t);
    F::draws(s, atlas, env, P);
}

// The same draw list for one 64×64 tile of one env's frame, a workgroup per (frame, tile): pgv_render_frames.
template <class F>
__global__ void __launch_bounds__(kFrameThreads) frames_kernel(typename F::State s, AtlasView atlas, FrameBatch fb) {
    __shared__ uint32_t tile[kTilePx];
    TilePainter P(tile, fb);
    const int env = P.env(fb);
    if (env >= 0) F::draws(s, atlas, env, P);
    P.store(fb);
}

// Their launches (pg_state_obs.h ViewedGame: a game's launch_frame / launch_frames); frames_kernel over count · tiles
// blocks, in as many launches as the grid limit asks for.
template <class F>
void launch_frame_of(hipStream_t st, const typename F::State& s, const AtlasView& atlas, int env, uint32_t* d_px, int w, int h) {
    hipLaunchKernelGGL(frame_kernel<F>, dim3(1), dim3(kFrameThreads), 0, st, s, atlas, env, FrameTarget{d_px, w, h});
}
template <class F>
void launch_frames_of(hipStream_t st, const typename F::State& s, const AtlasView& atlas, const int32_t* d_indices, int count,
                      uint8_t* d_rgb, int w, int h) {
    FrameBatch fb{d_indices, d_rgb, w, h, tiles_across(w) * tiles_across(h), s.n, 0};
    const long long total = static_cast<long long>(count) * fb.tiles, limit = frame_grid_limit();
    for (; fb.b0 < total; fb.b0 += limit)
        hipLaunchKernelGGL(frames_kernel<F>, dim3(static_cast<unsigned>(launch_blocks(total, fb.b0, limit))), dim3(kFrameThreads), 0,
                           st, s, atlas, fb);
}

}  // namespace pg
