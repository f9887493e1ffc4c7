// Filtered gathers of the frame history (include/procgen2_vec.h pgv_history_gather_filter): pg_history_aug.h's augmented row,
// flipped and turned by quarter turns, then through a C x C x k x k filter (k = 1: a colour matrix; k = 3: a random
// convolution) with a bias and a clamp, in float32 with every product and every sum rounded on its own — the value-changing
// augmentations (network randomisation, colour jitter's linear parts, grayscale, brightness, blur) in the gather's one pass:
//     A_c(y, x)   the byte pg_history_aug.h gives plane c at (y, x): window, edge rule, cutout (aug_source_byte_index);
//     G           A flipped (f) and turned (r quarter turns, np.rot90) — one draw per entry (filter_turn), index-only;
//     v_c(y, x)   float(G_c(y, x)) / 255.0f by the f32 value table; +0.0f outside the image (the zero padding of the layer);
//     out_o(y, x) = clamp(bias_o + sum over (i, ky, kx), in that order, of w[o][i][ky][kx] * v_i(y + ky - k/2, x + kx - k/2)),
//                   as float32, or rounded once to binary16 or bfloat16.
//
// The kernel: pg_history.h's head and fetch, the slot loop written out as there, here with the f32 table, so that the head's table maps a byte to
// its float's bits; lane 0 writes the params row, its eighth word the turn.  The entry's weights and bias
// (C·C·k·k + C floats) are workgroup-uniform: every lane reads them once, before anything is stored, by uniform loads into
// registers, never per pixel.  Per DISTINCT frame of the walk the C fetched planes are staged in LDS as the aug kernel's
// are (stage_planes, C·4096 bytes).
//   k = 3: the workgroup then builds G ONCE per frame into a second LDS image, so that the window, cutout, flip and turn
//   arithmetic is done once per pixel and plane-independently, not once per tap: C planes of H'+2 rows of W'+8 bytes each
//   (filter_image_stride), pixel (y, x) at byte (y + 1)·stride + x + 1; the row above, the row below, byte 0 of a row and
//   the bytes behind the pixels are zero bytes (the border, and the margin that keeps the stride a multiple of 8).  A lane
//   builds whole words: four positions' source indices (filter_image_source), C words stored.  With the left margin 1 and
//   the stride a multiple of 8 the ten bytes x0-1 .. x0+8 a run of 8 pixels needs of a row are bytes x0 .. x0+9 of the
//   image's row: three aligned words, of which the first two are one aligned 8-byte read.
//   k = 1: no border and no second image; a lane reads its 8 bytes of each plane from the staged planes through the same
//   index (one index per pixel, shared by the planes).
// A lane takes runs of 8 consecutive output pixels of a row (W' % 8 == 0), run number tid, tid + 256, …: for each input
// plane it reads the 3 x 10 (1 x 8) bytes, turns each into its float once through the table, and accumulates all C output
// planes of the 8 pixels from that one read, input plane outermost, so every output's sum keeps the order (i, ky, kx).  The
// accumulators are pairs of neighbouring pixels: gfx950's packed f32 multiply and add (v_pk_mul_f32, v_pk_add_f32) round
// each half on its own, exactly as two scalar instructions do, and halve the instruction count; nothing is fused (the build's
// -ffp-contract=off; no fmaf here).  Matrix instructions do not fit: per output pixel the contraction is C·k·k = 27 deep and
// only C = 3 outputs wide, its operands are a sliding window (an im2col copy per tile would cost more LDS traffic than the
// 27 multiplies it feeds), and an MFMA's internal sum order and fused products would break the float32 definition above.
// The 8 results of a plane are clamped by comparisons, converted, packed and stored as 16-byte units (ES = 2: one, ES = 4:
// two) at aug_unit_offset with U = 16: W' % 8 == 0 makes every run, row and plane of 2- or 4-byte elements start 16-byte
// aligned, so the unit is always 16 (aug_unit_bytes); the zero row is written by the same units, bias or not.  Plain vector
// loads and stores, no atomics.
// LDS: 1 KB table + 12 KB staged + 13.9 KB image (k = 3, RGB) + the walk = 27.0 KB a workgroup; gfx950's 160 KB a CU hold
// five such workgroups (20 waves), k = 1 (13.1 KB) twelve.  At k = 3, RGB, it is the register file that limits them
// first: the compiler keeps the 30 values, 24 accumulators and what it hoists of the 84 weights in 118 (f32) to 201 (f16)
// VGPRs, two to four workgroups a CU; the kernel is bound by its 1 296 multiplies and adds a run, not by LDS or memory
// (docs/OPTLOG.md has the times).
// Bounds.  The head, the ring and the zero row: pg_history.h; the staging: pg_history_aug.h.  params[entry·8 .. + 7],
// weights[entry·wstride .. + C·C·k·k - 1] and bias[entry·bstride .. + C - 1], entry < count, with the strides 0 or exactly
// the set's size (checked on the host: the caller's tensors hold one set or `count` sets).  The staged planes are indexed by
// p·4096 + s where s = filter_image_source(...) is in 0 .. 4095 or a sentinel, which reads nothing of them, for every (oy,
// ox, flip, r, y, x): filter_turn maps 0 .. H'-1 x 0 .. W'-1 onto itself (r > 0 only where H' = W', the host refuses it
// otherwise) and aug_source_byte_index takes it from there (tests/cpp/test_history_filter.cpp and test_history_aug.cpp,
// exhaustively).  The image is written by words wi < (H'+2)·stride/4 <= kFilterImageWords of each plane p < C at
// p·kFilterImageWords + wi, and read at p·kFilterImageWords + ((y + ky)·stride + x0)/4 + 0 .. 2 with y + ky <= H'+1, x0 <=
// W'-8: the last byte read is (H'+1)·stride + W' + 3 < (H'+2)·stride (filter_run_word, swept in the same test).  A lane
// writes runs run < H'·W'/8 of channel ch < K·C at aug_unit_offset(entry, K, C, H', W', ES, ch, run·ES/2 + 0 .. ES/2 - 1,
// 16): bytes run·8·ES .. + 8·ES - 1 of the channel's H'·W'·ES.  A refused call launches nothing; a zero row writes the same
// bytes and reads neither weights nor ring.  Offsets are size_t: 65 536 rows of K = 8 RGB f32 are 25.8 GB.
#pragma once

#include "pg_history_aug.h"

namespace pg {

constexpr int kFilterFlip = 1, kFilterRot90 = 2;  // FilterConfig::turns
constexpr int kFilterRun = 8;                     // pixels a run

struct FilterConfig {  // pgv_gather_filter without its pointers
    int kernel, turns, clamp;
    float lo, hi;
    int weights_stride, bias_stride;  // floats from one entry's set to the next, or 0: one set for the call
};

// nullptr, or why the filter is refused for a ring of `planes` planes and rows of out_h x out_w.
PG_HD const char* filter_config_error(const FilterConfig& f, int planes, int out_h, int out_w) {
    if (f.kernel != 1 && f.kernel != 3) return "kernel must be 1 or 3";
    const int set = planes * planes * f.kernel * f.kernel;
    if (f.weights_stride != 0 && f.weights_stride != set) return "weights_stride must be 0 or C*C*kernel*kernel";
    if (f.bias_stride != 0 && f.bias_stride != planes) return "bias_stride must be 0 or C";
    if ((f.turns & kFilterRot90) && out_h != out_w) return "rot90 needs out_height = out_width";
    if (f.clamp && !(f.lo <= f.hi)) return "clamp needs lo <= hi, neither a NaN";
    return nullptr;
}

// The turn of an entry: f | r << 1, the eighth word of its params row.
PG_HD int filter_turn(uint32_t seed, uint32_t entry, int turns) {
    const int f = (turns & kFilterFlip) ? int(aug_word(seed, entry, 7) >> 31) : 0;
    const int r = (turns & kFilterRot90) ? aug_draw(seed, entry, 4u, 8) : 0;
    return f | r << 1;
}
// Where pixel (y, x) of G reads A: G = np.rot90(A[..., ::-1] if f else A, r) over (rows, columns); r > 0 only with H = W.
PG_HD void filter_turned(int turn, int H, int W, int y, int x, int& ay, int& ax) {
    const int r = turn >> 1;
    ay = r == 0 ? y : r == 1 ? x : r == 2 ? H - 1 - y : W - 1 - x;
    ax = r == 0 ? x : r == 1 ? H - 1 - y : r == 2 ? W - 1 - x : y;
    if (turn & 1) ax = W - 1 - ax;
}

// The image of G with its border: H+2 rows of `stride` bytes, pixel (y, x) at (y + 1)*stride + x + 1.
PG_HD int filter_image_stride(int out_w) { return out_w + 8; }
constexpr int kFilterImageWords = (kObsH + 2) * (kObsW + 8) / 4;  // words a plane, at most
PG_HD int filter_image_words(int out_h, int out_w) { return (out_h + 2) * filter_image_stride(out_w) / 4; }
// What byte (gy, gx) of the image holds, gy < H+2, gx < stride: aug_source_byte_index's answer for the pixel, kAugZero for
// the border and the margin.
PG_HD int filter_image_source(const AugParams& p, int edge, int turn, int H, int W, int gy, int gx) {
    const int y = gy - 1, x = gx - 1;
    if (y < 0 || y >= H || x < 0 || x >= W) return kAugZero;
    int ay, ax;
    filter_turned(turn, H, W, y, x, ay, ax);
    return aug_source_byte_index(p, edge, ay, ax);
}
// The first of the three words that hold bytes x0-1 .. x0+8 of pixel row y + ky - 1 (ky = 0 .. 2; x0 % 8 == 0): even.
PG_HD int filter_run_word(int out_w, int y, int ky, int x0) { return ((y + ky) * filter_image_stride(out_w) + x0) / 4; }

struct HistoryGatherFilter {
    HistoryGather g;  // (table: the f32 table; out: [count][K*C][H'][W'] elements, 16-byte aligned)
    AugConfig cfg;
    FilterConfig f;
    int32_t* params;       // [count][8] or nullptr
    const float* weights;  // [C][C][k][k], a set per entry or one
    const float* bias;     // [C] likewise, or nullptr
    int bf16;              // ES = 2: bfloat16, else binary16
};

#if defined(__HIPCC__)
typedef float FilterPair __attribute__((ext_vector_type(2)));  // two neighbouring pixels: one packed instruction

PG_D float filter_value(const uint32_t* table, uint32_t byte) { return __uint_as_float(table[byte]); }
// float32 → the element's bits: round to nearest even, subnormals, overflow to infinity.
template <int ES>
PG_D uint32_t filter_element(float v, int bf16) {
    if (ES == 4) return __float_as_uint(v);
    if (bf16) {
        const uint32_t u = __float_as_uint(v);
        return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
    }
    const _Float16 h = static_cast<_Float16>(v);
    uint16_t bits;
    __builtin_memcpy(&bits, &h, 2);
    return bits;
}

template <int ES, int C, int KS>  // element bytes (2, 4); planes; kernel
__global__ void __launch_bounds__(kHistoryBlock) history_gather_filter_kernel(HistoryGatherFilter q) {
    constexpr int kTaps = KS * KS, kSpan = kFilterRun + KS - 1;  // bytes of a row a run needs
    __shared__ GatherHead head;
    __shared__ PolicyVec16 staged[C * kPolicyPlane / 16];          // the C planes of one frame, as stored
    __shared__ uint64_t image[KS == 3 ? C * kFilterImageWords / 2 : 1];  // G with its border (k = 3)
    const int tid = static_cast<int>(threadIdx.x);
    const size_t entry = blockIdx.x;
    const int K = q.g.stack, H = q.cfg.out_h, W = q.cfg.out_w, edge = q.cfg.edge;
    const AugParams ap = aug_params(q.cfg, static_cast<uint32_t>(entry));
    const int turn = filter_turn(q.cfg.seed, static_cast<uint32_t>(entry), q.f.turns);
    // the entry's set, before anything is stored: uniform addresses
    float w[C * C * kTaps], b[C];
    {
        const float* const ws = q.weights + entry * size_t(q.f.weights_stride);
#pragma unroll
        for (int k = 0; k < C * C * kTaps; k++) w[k] = ws[k];
#pragma unroll
        for (int o = 0; o < C; o++) b[o] = q.bias ? q.bias[entry * size_t(q.f.bias_stride) + o] : 0.0f;
    }
    int env = 0;
    const bool ok = gather_entry(q.g, entry, tid, head, env);
    gather_params_row(q.params, entry, ap, C, turn, tid);
    const size_t channel = aug_plane_bytes(H, W, ES);
    uint8_t* const out = q.g.out + entry * (size_t(K) * C * channel);
    if (!ok) {  // (workgroup-uniform)
        zero_row<PolicyVec16>(out, K * C, channel, static_cast<int>(channel / 16), tid);
        return;
    }
    const uint32_t* const table = head.table;
    const uint8_t* const bytes = reinterpret_cast<const uint8_t*>(staged);
    uint32_t* const image_words = reinterpret_cast<uint32_t*>(image);
    const int runs = H * W / kFilterRun, runs_a_row = W / kFilterRun;
    const float lo = q.f.lo, hi = q.f.hi;
    for (int j = 0; j < K; j++) {
        const int64_t f = head.frame[j];
        if (j == 0 || f != head.frame[j - 1]) {  // (workgroup-uniform)
            PolicyVec16 in[C];
            history_fetch<C>(q.g, f, env, tid, in);
            stage_planes<C>(staged, in, tid);
            if (KS == 3) {
                const int stride = filter_image_stride(W), words_a_row = stride / 4, words = filter_image_words(H, W);
                for (int wi = tid; wi < words; wi += kHistoryBlock) {
                    const int gy = wi / words_a_row, gx = (wi - gy * words_a_row) * 4;
                    uint32_t word[C] = {};
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int at = filter_image_source(ap, edge, turn, H, W, gy, gx + i);
#pragma unroll
                        for (int p = 0; p < C; p++) {
                            const uint32_t byte = at == kAugCutout ? (ap.colour >> (8 * p)) & 0xFFu : at == kAugZero ? 0u : bytes[p * kPolicyPlane + at];
                            word[p] |= byte << (8 * i);
                        }
                    }
#pragma unroll
                    for (int p = 0; p < C; p++) image_words[p * kFilterImageWords + wi] = word[p];
                }
                __syncthreads();
            }
        }
        uint8_t* const to = out + size_t(K - 1 - j) * C * channel;
        for (int run = tid; run < runs; run += kHistoryBlock) {
            const int y = run / runs_a_row, x0 = (run - y * runs_a_row) * kFilterRun;
            int at[KS == 1 ? kFilterRun : 1];
            if (KS == 1) {
#pragma unroll
                for (int i = 0; i < kFilterRun; i++) at[i] = filter_image_source(ap, edge, turn, H, W, y + 1, x0 + i + 1);
            }
            FilterPair acc[C][kFilterRun / 2];
#pragma unroll
            for (int o = 0; o < C; o++)
#pragma unroll
                for (int m = 0; m < kFilterRun / 2; m++) acc[o][m] = FilterPair{b[o], b[o]};
#pragma unroll
            for (int i = 0; i < C; i++) {
                float v[KS][kSpan];
                if (KS == 1) {
#pragma unroll
                    for (int x = 0; x < kFilterRun; x++) {
                        const uint32_t byte = at[x] == kAugCutout ? (ap.colour >> (8 * i)) & 0xFFu : at[x] == kAugZero ? 0u : bytes[i * kPolicyPlane + at[x]];
                        v[0][x] = filter_value(table, byte);
                    }
                } else {
#pragma unroll
                    for (int ky = 0; ky < KS; ky++) {
                        const int first = i * kFilterImageWords + filter_run_word(W, y, ky, x0);
                        const uint64_t two = image[first / 2];  // (first is even: the stride and x0 are multiples of 8)
                        const uint32_t three[3] = {uint32_t(two), uint32_t(two >> 32), image_words[first + 2]};
#pragma unroll
                        for (int x = 0; x < kSpan; x++) v[ky][x] = filter_value(table, (three[x >> 2] >> (8 * (x & 3))) & 0xFFu);
                    }
                }
#pragma unroll
                for (int o = 0; o < C; o++)
#pragma unroll
                    for (int ky = 0; ky < KS; ky++)
#pragma unroll
                        for (int kx = 0; kx < KS; kx++) {
                            const float wt = w[(o * C + i) * kTaps + ky * KS + kx];
                            const FilterPair ww{wt, wt};
#pragma unroll
                            for (int m = 0; m < kFilterRun / 2; m++) {
                                const FilterPair vv{v[ky][2 * m + kx], v[ky][2 * m + 1 + kx]};
                                const FilterPair product = ww * vv;  // (its own rounding: -ffp-contract=off)
                                acc[o][m] = acc[o][m] + product;
                            }
                        }
            }
#pragma unroll
            for (int o = 0; o < C; o++) {
                uint32_t e[kFilterRun];
#pragma unroll
                for (int x = 0; x < kFilterRun; x++) {
                    float a = acc[o][x >> 1][x & 1];
                    if (q.f.clamp) a = a < lo ? lo : a > hi ? hi : a;
                    e[x] = filter_element<ES>(a, q.bf16);
                }
                constexpr int kUnits = ES / 2;  // 16-byte units a run
                PolicyVec16* const at16 = reinterpret_cast<PolicyVec16*>(to + aug_unit_offset(0, K, C, H, W, ES, o, run * kUnits, 16));
                if (ES == 2) {
                    at16[0] = PolicyVec16{e[0] | e[1] << 16, e[2] | e[3] << 16, e[4] | e[5] << 16, e[6] | e[7] << 16};
                } else {
                    at16[0] = PolicyVec16{e[0], e[1], e[2], e[3]};
                    at16[1] = PolicyVec16{e[4], e[5], e[6], e[7]};
                }
            }
        }
    }
}

inline void launch_history_gather_filter(hipStream_t st, const HistoryGatherFilter& q, int es) {
    for_es_planes<2>(es, q.g.b.planes, [&](auto es_c, auto planes_c) {  // (u8 is refused)
        constexpr int ES = decltype(es_c)::value, C = decltype(planes_c)::value;
        hipLaunchKernelGGL((q.f.kernel == 1 ? history_gather_filter_kernel<ES, C, 1> : history_gather_filter_kernel<ES, C, 3>), dim3(q.g.count),
                           dim3(kHistoryBlock), 0, st, q);
    });
}
#endif

}  // namespace pg
