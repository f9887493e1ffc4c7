// The host half of the policy observations (procgen2_amd/csrc/pg_policy_obs.h) compiled for the CPU: the value table, the
// gray rule, who owns which bytes of an env's block, and the listing of the engine's own memory.
// argv[1], optional: a file of 4 x 256 little-endian uint32 — the tables of PGV_POLICY_U8, _F16, _BF16, _F32 in that order —
// made independently (tests/test_policy_obs.py: numpy); the header's table must equal it.
// Prints "OK <section>" per section and "ALL OK"; exit status 1 on the first failure.
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "pg_policy_obs.h"

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                   \
        }                                                               \
    } while (0)

static int test_table(const char* path) {
    using namespace pg;
    CHECK(policy_element_bytes(kPolicyU8) == 1 && policy_element_bytes(kPolicyF16) == 2 && policy_element_bytes(kPolicyBF16) == 2 &&
          policy_element_bytes(kPolicyF32) == 4);
    // the literal anchors
    CHECK(policy_table_entry(kPolicyF32, 1) == 0x3B808081u && policy_table_entry(kPolicyF16, 1) == 0x1C04u && policy_table_entry(kPolicyBF16, 1) == 0x3B81u);
    CHECK(policy_table_entry(kPolicyF16, 128) == 0x3804u && policy_table_entry(kPolicyBF16, 128) == 0x3F01u);
    CHECK(policy_table_entry(kPolicyF32, 255) == 0x3F800000u && policy_table_entry(kPolicyF16, 255) == 0x3C00u && policy_table_entry(kPolicyBF16, 255) == 0x3F80u);
    for (int dtype = 0; dtype < 4; dtype++) {
        std::set<uint32_t> seen;
        CHECK(policy_table_entry(dtype, 0) == 0u);
        for (uint32_t v = 0; v < 256; v++) {
            const uint32_t w = policy_table_entry(dtype, v);
            CHECK(dtype != kPolicyU8 || w == v);
            CHECK(policy_element_bytes(dtype) == 4 || (w >> (8 * policy_element_bytes(dtype))) == 0u);  // nothing above the element
            CHECK(v == 0 || w > policy_table_entry(dtype, v - 1));  // (non-negative floats order as their patterns): all distinct
            seen.insert(w);
        }
        CHECK(seen.size() == 256);
    }
    // f16 against the compiler's own conversion where it has one
#if defined(__FLT16_MANT_DIG__)
    for (uint32_t v = 0; v < 256; v++) {
        const _Float16 h = static_cast<_Float16>(static_cast<float>(v) / 255.0f);
        uint16_t bits;
        std::memcpy(&bits, &h, 2);
        CHECK(policy_table_entry(kPolicyF16, v) == bits);
    }
#endif
    if (path) {
        std::vector<uint32_t> want(4 * 256);
        FILE* f = std::fopen(path, "rb");
        CHECK(f != nullptr);
        const size_t got = std::fread(want.data(), 4, want.size(), f);
        std::fclose(f);
        CHECK(got == want.size());
        for (int dtype = 0; dtype < 4; dtype++)
            for (uint32_t v = 0; v < 256; v++) CHECK(policy_table_entry(dtype, v) == want[dtype * 256 + v]);
        std::printf("OK table file\n");
    }
    std::printf("OK table\n");
    return 0;
}

static int test_gray() {
    using namespace pg;
    CHECK(policy_gray(0, 0, 0) == 0 && policy_gray(255, 255, 255) == 255);
    CHECK(policy_gray(255, 0, 0) == 77 && policy_gray(0, 255, 0) == 149 && policy_gray(0, 0, 255) == 29);
    CHECK(policy_gray(255, 255, 0) == 226 && policy_gray(0, 255, 255) == 178 && policy_gray(255, 0, 255) == 106);
    for (uint32_t v = 0; v < 256; v++) CHECK(policy_gray(v, v, v) == v);  // the weights sum to 256
    for (uint32_t r = 0; r < 256; r += 5)
        for (uint32_t g = 0; g < 256; g += 3)
            for (uint32_t b = 0; b < 256; b += 7) {
                const uint32_t y = policy_gray(r, g, b);
                const double exact = (77.0 * r + 150.0 * g + 29.0 * b) / 256.0;
                CHECK(y <= 255 && y == static_cast<uint32_t>(exact + 0.5));  // round half up of the exact weighted mean
                CHECK(g == 255 || policy_gray(r, g + 1, b) >= y);
            }
    std::printf("OK gray\n");
    return 0;
}

// One env's push as the kernel makes it, on the host, with marks in place of values: element e of channel ch of the new
// frame carries the mark (ch % C) * 4096 + e, byte b of it the byte b of that mark + 1 — so a byte in the wrong place shows.
static uint8_t mark_byte(int plane, int element, int es, int b) {
    const uint32_t m = static_cast<uint32_t>(plane * pg::kPolicyPlane + element) * 2654435761u + 1u;
    return static_cast<uint8_t>((m >> (8 * (b % 4))) + b + es);
}
static int walk(int es, int C, int K, bool dense, bool restart) {
    using namespace pg;
    const size_t bytes = policy_bytes_per_env(K, C, es);
    CHECK(bytes == size_t(K) * C * 4096 * es);
    std::vector<uint8_t> out(bytes), before(bytes);
    for (size_t k = 0; k < bytes; k++) before[k] = out[k] = static_cast<uint8_t>(k * 31 + (k >> 8) * 7 + 3);
    std::vector<int> writes(bytes, 0);
    if (!restart)
        for (int s = 0; s + 1 < K; s++)
            for (int wave = 0; wave < 4; wave++)
                for (int lane = 0; lane < 64; lane++) {
                    std::vector<uint8_t> held(size_t(C) * es * 16);
                    for (int p = 0; p < C; p++)
                        for (int k = 0; k < es; k++)
                            std::memcpy(&held[(size_t(p) * es + k) * 16], &out[policy_unit_offset(es, (s + 1) * C + p, wave, policy_unit(dense, es, lane, k))], 16);
                    for (int p = 0; p < C; p++)
                        for (int k = 0; k < es; k++) {
                            const size_t at = policy_unit_offset(es, s * C + p, wave, policy_unit(dense, es, lane, k));
                            CHECK(at + 16 <= bytes);
                            std::memcpy(&out[at], &held[(size_t(p) * es + k) * 16], 16);
                            for (int b = 0; b < 16; b++) writes[at + b]++;
                        }
                }
    for (int p = 0; p < C; p++)
        for (int wave = 0; wave < 4; wave++) {
            // what the wave's lanes hold: lane l the 16·es bytes of its pixels 16·(64·wave + l) .. + 15, i.e. units l·es .. l·es + es - 1
            std::vector<uint8_t> share(size_t(64) * es * 16);
            for (int lane = 0; lane < 64; lane++)
                for (int j = 0; j < kPolicyLanePixels; j++)
                    for (int b = 0; b < es; b++)
                        share[(size_t(lane) * kPolicyLanePixels + j) * es + b] = mark_byte(p, (wave * 64 + lane) * kPolicyLanePixels + j, es, b);
            for (int lane = 0; lane < 64; lane++)
                for (int k = 0; k < es; k++) {
                    // dense: the exchange hands lane l unit 64k + l; strided: it keeps its own unit l·es + k
                    const int unit = policy_unit(dense, es, lane, k);
                    CHECK(unit >= 0 && unit < 64 * es);
                    for (int s = restart ? 0 : K - 1; s < K; s++) {
                        const size_t at = policy_unit_offset(es, s * C + p, wave, unit);
                        CHECK(at + 16 <= bytes);
                        std::memcpy(&out[at], &share[size_t(unit) * 16], 16);
                        for (int b = 0; b < 16; b++) writes[at + b]++;
                    }
                }
        }
    for (size_t k = 0; k < bytes; k++) CHECK(writes[k] == 1);  // every byte of the env's block, exactly once
    const size_t slot = size_t(C) * 4096 * es;
    for (int s = 0; s < K; s++)
        for (int p = 0; p < C; p++)
            for (int e = 0; e < 4096; e++)
                for (int b = 0; b < es; b++) {
                    const size_t at = s * slot + (size_t(p) * 4096 + e) * es + b;
                    if (restart || s == K - 1)
                        CHECK(out[at] == mark_byte(p, e, es, b));
                    else
                        CHECK(out[at] == before[at + slot]);
                }
    return 0;
}
static int test_walk() {
    for (int es : {1, 2, 4})
        for (int K : {1, 3, 4})
            for (int C : {1, 3})
                for (int dense = 0; dense < 2; dense++)
                    for (int restart = 0; restart < 2; restart++)
                        if (walk(es, C, K, dense != 0, restart != 0)) {
                            std::printf("  (es %d, K %d, C %d, dense %d, restart %d)\n", es, K, C, dense, restart);
                            return 1;
                        }
    // the largest offset of the largest configuration needs more than 32 bits
    CHECK(size_t(65535) * pg::policy_bytes_per_env(4, 3, 4) + pg::policy_unit_offset(4, 11, 3, 255) + 16 == size_t(65536) * 4 * 3 * 4096 * 4);
    CHECK(size_t(65536) * pg::policy_bytes_per_env(4, 3, 4) > (size_t(1) << 33));
    std::printf("OK walk\n");
    return 0;
}

static int test_listing() {
    // the engine's own block (pg_carve.h): the flags, then the table, each rounded to 256 bytes
    pg::PolicyObsBuffers b{};
    CHECK(pg::Carve::size(pg::list_policy_obs, 3) == 256 + 1024);
    CHECK(pg::Carve::size(pg::list_policy_obs, 300) == 512 + 1024);
    alignas(256) static uint8_t block[1280];
    pg::Carve::bind(pg::list_policy_obs, block, b, 3);
    CHECK(b.restart == block && reinterpret_cast<uint8_t*>(b.table) == block + 256);
    std::printf("OK listing\n");
    return 0;
}

int main(int argc, char** argv) {
    if (test_table(argc > 1 ? argv[1] : nullptr) || test_gray() || test_walk() || test_listing()) return 1;
    std::printf("ALL OK\n");
    return 0;
}
