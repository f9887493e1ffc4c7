// Augmented gathers of the frame history (include/procgen2_vec.h pgv_history_gather_aug): pg_history.h's gather with a random
// shift or crop and a cutout worked into it — the augmentations of RAD, DrAC and DrQ — on the stored u8 bytes, in front of the
// value table:
//     a gathered row [K*C][H'][W'] elements; one window (oy, ox) and one rectangle (cy, cx, ch, cw) per entry, shared by its
//     K frames and C planes; the draws a function of (config, entry number) alone (aug_params, host and device alike);
//     element (slot, plane, y, x) = table[byte], byte by aug_source_byte_index: the plane's colour byte inside the rectangle,
//     else the stored byte at (oy + y, ox + x), outside the frame the nearest pixel's (REPLICATE) or 0 (ZERO).
//
// The kernel: one workgroup of 256 lanes per entry, begun as the plain gather's is (pg_history.h gather_entry); lane 0 writes
// the params row behind it.  Every lane works the entry's draws out for itself (they are workgroup-uniform).  Per DISTINCT
// frame of the walk a lane fetches its stored bytes of each plane (history_fetch) and the workgroup stages the C planes in LDS
// (C·4096 bytes) between two barriers under a workgroup-uniform condition; a frame the walk repeats is neither fetched nor
// staged again.  The lanes then write the output plane in dense order: unit u (U bytes, U/ES elements) of a plane is written
// by lane u % 256 in its store number u / 256, so the lanes of one store instruction lie U bytes apart.  A lane reads its
// source bytes from the staged planes one byte at a time (neighbouring lanes read neighbouring bytes: the same or the next LDS
// word), through aug_source_byte_index, then through the table, and packs them.
// U is 16 where a plane's H'·W'·ES bytes are a multiple of 16 — then every row and plane starts 16-byte aligned — and 8
// otherwise: W' is a multiple of 8, so a plane is always a whole number of 8-byte units, starts 8-byte aligned, and no store
// is ever narrower than a unit or reaches past its plane.  An entry that is not held, or whose env is outside the batch,
// gets a row of zero bytes by the same units (pg_planes.h zero_row).  Plain vector loads and stores, no atomics.
// Bounds.  The grid is `count` workgroups, entry = blockIdx.x < count; pushes[entry], envs[entry], params[entry·8 .. + 7];
// nothing of the ring is read unless 0 <= env < n and the push is held, and the walk only moves to held pushes (pg_history.h):
// a lane reads frames[frame offset + p·4096 + 16t .. + 15], p < C, t < 256.  The staged planes are indexed by
// p·4096 + aug_source_byte_index(...) with the index in 0 .. 4095 for every (oy, ox, y, x) (or a sentinel, which reads
// nothing of them: tests/cpp/test_history_aug.cpp, exhaustively); the table by a byte.  A lane writes unit u < H'·W'·ES / U of
// channel ch < K·C at  entry·K·C·H'·W'·ES + ch·H'·W'·ES + u·U .. + U-1  <  (entry + 1)·K·C·H'·W'·ES  (aug_unit_offset).
// Offsets are size_t: 65 536 rows of K = 8 RGB f32 are 25.8 GB.
#pragma once

#include "pg_history.h"

namespace pg {

// include/procgen2_vec.h PGV_AUG_*
constexpr int kAugEdgeReplicate = 0, kAugEdgeZero = 1;
constexpr int kAugCutoutBlack = 0, kAugCutoutRandom = 1;
constexpr int kAugMaxPad = 16;
constexpr int kAugParamWords = 8;

struct AugConfig {  // pgv_gather_aug without its pointer
    int out_h, out_w, pad, edge, cutout_min, cutout_max, cutout_color;
    uint32_t seed;
};
struct AugParams {
    int oy, ox, cy, cx, ch, cw;
    uint32_t colour;  // byte c: plane c's cutout byte
};

// nullptr, or why the config is refused.
PG_HD const char* aug_config_error(const AugConfig& a) {
    if (a.out_h < 1 || a.out_h > kObsH) return "out_height must be in 1 .. 64";
    if (a.out_w < 8 || a.out_w > kObsW || (a.out_w & 7)) return "out_width must be in 8 .. 64 and a multiple of 8";
    if (a.pad < 0 || a.pad > kAugMaxPad) return "pad must be in 0 .. 16";
    if (a.edge != kAugEdgeReplicate && a.edge != kAugEdgeZero) return "unknown edge rule";
    if (a.cutout_color != kAugCutoutBlack && a.cutout_color != kAugCutoutRandom) return "unknown cutout colour mode";
    if (a.cutout_min < 0 || a.cutout_max < 0 || a.cutout_max > 64) return "cutout sides must be in 0 .. 64";
    if (a.cutout_min > a.cutout_max) return "cutout_min is greater than cutout_max";
    if (a.cutout_min == 0 && a.cutout_max > 0) return "cutout_min must be >= 1 where cutout_max > 0";
    return nullptr;
}

// Word j of entry e, and a draw in 0 .. m-1 from it (synthetic_action's rule).
PG_HD uint32_t aug_word(uint32_t seed, uint32_t entry, uint32_t j) {
    return mix32(mix32(seed + 0x9E3779B9u * (entry + 1u)) ^ (j * 0x85EBCA6Bu + 0xC2B2AE35u));
}
PG_HD int aug_draw(uint32_t seed, uint32_t entry, uint32_t m, uint32_t j) {
    return static_cast<int>((static_cast<uint64_t>(aug_word(seed, entry, j)) * m) >> 32);
}
PG_HD AugParams aug_params(const AugConfig& a, uint32_t entry) {
    AugParams p{};
    p.oy = -a.pad + aug_draw(a.seed, entry, uint32_t(kObsH + 2 * a.pad - a.out_h + 1), 0);
    p.ox = -a.pad + aug_draw(a.seed, entry, uint32_t(kObsW + 2 * a.pad - a.out_w + 1), 1);
    if (a.cutout_max > 0) {
        const uint32_t sides = uint32_t(a.cutout_max - a.cutout_min + 1);
        const int h = a.cutout_min + aug_draw(a.seed, entry, sides, 2), w = a.cutout_min + aug_draw(a.seed, entry, sides, 3);
        p.ch = h < a.out_h ? h : a.out_h;
        p.cw = w < a.out_w ? w : a.out_w;
        p.cy = aug_draw(a.seed, entry, uint32_t(a.out_h - p.ch + 1), 4);
        p.cx = aug_draw(a.seed, entry, uint32_t(a.out_w - p.cw + 1), 5);
        p.colour = a.cutout_color == kAugCutoutRandom ? aug_word(a.seed, entry, 6) : 0u;
    }
    return p;
}
// The params row of an entry; `planes` = 3: the colour's three bytes, 1: byte 0 alone.
PG_HD void aug_params_row(const AugParams& p, int planes, int32_t* row) {
    row[0] = p.oy, row[1] = p.ox, row[2] = p.cy, row[3] = p.cx, row[4] = p.ch, row[5] = p.cw;
    row[6] = static_cast<int32_t>(p.colour & (planes == 1 ? 0xFFu : 0xFFFFFFu));
    row[7] = 0;
}

constexpr int kAugZero = -1, kAugCutout = -2;
// Where output pixel (y, x) reads a stored plane: a byte index 0 .. 4095, kAugZero (the byte is 0) or kAugCutout (the byte
// is the plane's colour byte).
PG_HD int aug_source_byte_index(const AugParams& p, int edge, int y, int x) {
    if (y >= p.cy && y < p.cy + p.ch && x >= p.cx && x < p.cx + p.cw) return kAugCutout;
    int sy = p.oy + y, sx = p.ox + x;
    if (sy < 0 || sy >= kObsH || sx < 0 || sx >= kObsW) {
        if (edge != kAugEdgeReplicate) return kAugZero;
        sy = sy < 0 ? 0 : sy >= kObsH ? kObsH - 1 : sy;
        sx = sx < 0 ? 0 : sx >= kObsW ? kObsW - 1 : sx;
    }
    return sy * kObsW + sx;
}

// Bytes a store unit: 16 where every plane is a whole number of them, else 8 (W' is a multiple of 8).
PG_HD int aug_unit_bytes(int out_h, int out_w, int es) { return (size_t(out_h) * size_t(out_w) * size_t(es)) % 16 == 0 ? 16 : 8; }
PG_HD size_t aug_plane_bytes(int out_h, int out_w, int es) { return size_t(out_h) * size_t(out_w) * size_t(es); }
PG_HD size_t aug_row_bytes(int stack, int planes, int out_h, int out_w, int es) { return size_t(stack) * size_t(planes) * aug_plane_bytes(out_h, out_w, es); }
// Byte offset in the output of unit u (unit_bytes each) of channel ch of an entry.
PG_HD size_t aug_unit_offset(size_t entry, int stack, int planes, int out_h, int out_w, int es, int ch, int unit, int unit_bytes) {
    return entry * aug_row_bytes(stack, planes, out_h, out_w, es) + size_t(ch) * aug_plane_bytes(out_h, out_w, es) + size_t(unit) * size_t(unit_bytes);
}

struct HistoryGatherAug {
    HistoryGather g;  // (out: [count][K*C][H'][W'] elements, 16-byte aligned)
    AugConfig cfg;
    int32_t* params;  // [count][8] or nullptr
};

#if defined(__HIPCC__)
typedef uint32_t AugVec8 __attribute__((ext_vector_type(2)));  // 8 bytes a lane

template <int ES, int C, int U>  // element bytes; planes; bytes a store unit
__global__ void __launch_bounds__(kHistoryBlock) history_gather_aug_kernel(HistoryGatherAug q) {
    typedef std::conditional_t<U == 16, PolicyVec16, AugVec8> Unit;
    constexpr int kPerWord = 4 / ES, kPerUnit = U / ES;  // pixels a word; pixels a unit
    constexpr int kRun = kPerUnit < 8 ? kPerUnit : 8;                    // pixels in a row of the output for certain: W' % 8 == 0
    __shared__ uint32_t table[256];
    __shared__ int64_t frame[kPolicyMaxStack];
    __shared__ int valid;
    __shared__ PolicyVec16 staged[C * kPolicyPlane / 16];  // the C planes of one frame, as stored
    const int tid = static_cast<int>(threadIdx.x);
    const size_t entry = blockIdx.x;
    const int K = q.g.stack;
    const AugParams ap = aug_params(q.cfg, static_cast<uint32_t>(entry));
    int env = 0;
    const bool ok = gather_entry(q.g, entry, tid, table, frame, &valid, env);
    if (tid == 0 && q.params) {
        int32_t row[kAugParamWords];
        aug_params_row(ap, C, row);
#pragma unroll
        for (int k = 0; k < kAugParamWords; k++) q.params[entry * kAugParamWords + k] = row[k];
    }
    const int W = q.cfg.out_w, edge = q.cfg.edge;
    const int units = q.cfg.out_h * W / kPerUnit;  // (exact: aug_unit_bytes)
    const size_t channel = aug_plane_bytes(q.cfg.out_h, W, ES);
    uint8_t* const out = q.g.out + entry * (size_t(K) * C * channel);
    if (!ok) {  // (workgroup-uniform)
        zero_row<Unit>(out, K * C, channel, units, tid);
        return;
    }
    const uint8_t* const bytes = reinterpret_cast<const uint8_t*>(staged);
    for (int j = 0; j < K; j++) {
        const int64_t f = frame[j];
        if (j == 0 || f != frame[j - 1]) {  // (workgroup-uniform)
            PolicyVec16 in[C];
            history_fetch<C>(q.g, f, env, tid, in);
            __syncthreads();  // every lane has done with the frame staged before
#pragma unroll
            for (int p = 0; p < C; p++) staged[p * (kPolicyPlane / 16) + tid] = in[p];
            __syncthreads();
        }
        uint8_t* const to = out + size_t(K - 1 - j) * C * channel;
#pragma unroll
        for (int p = 0; p < C; p++) {
            const uint8_t* const plane = bytes + p * kPolicyPlane;
            const uint32_t colour = (ap.colour >> (8 * p)) & 0xFFu;
            for (int u = tid; u < units; u += kHistoryBlock) {
                Unit w{};
#pragma unroll
                for (int r = 0; r < kPerUnit / kRun; r++) {
                    const int first = u * kPerUnit + r * kRun, y = first / W, x0 = first - y * W;
#pragma unroll
                    for (int i = 0; i < kRun; i++) {
                        const int at = aug_source_byte_index(ap, edge, y, x0 + i);
                        const uint32_t byte = at == kAugCutout ? colour : at == kAugZero ? 0u : plane[at];
                        const int px = r * kRun + i;
                        w[px / kPerWord] |= table[byte] << (8 * ES * (px % kPerWord));
                    }
                }
                *reinterpret_cast<Unit*>(to + p * channel + size_t(u) * U) = w;
            }
        }
    }
}

inline void launch_history_gather_aug(hipStream_t st, const HistoryGatherAug& q, int es) {
    for_es_planes(es, q.g.b.planes, [&](auto es_c, auto planes_c) {
        constexpr int ES = decltype(es_c)::value, C = decltype(planes_c)::value;
        void (*kernel)(HistoryGatherAug) = history_gather_aug_kernel<ES, C, 8>;
        if (aug_unit_bytes(q.cfg.out_h, q.cfg.out_w, ES) == 16) kernel = history_gather_aug_kernel<ES, C, 16>;
        hipLaunchKernelGGL(kernel, dim3(q.g.count), dim3(kHistoryBlock), 0, st, q);
    });
}
#endif

}  // namespace pg
