// The host/device rules of procgen2_amd/csrc/pg_frame_codes.h against loops written out, on literal cases.
#include <climits>
#include <cstdio>

#include "pg_frame_codes.h"

static uint32_t mix(uint32_t x) {  // pg_defs.h mix32, restated
    x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
    return x;
}
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
    const uint32_t seeds[] = {0u, 1u, 0xFFFFFFFFu, 12345u};
    int plus = 0, all = 0;
    for (uint32_t seed : seeds)
        for (uint32_t j : {0u, 1u, 31u, 255u})
            for (uint32_t d : {0u, 1u, 4095u, 4096u, 12287u}) {
                const int want = (mix(mix(seed ^ (j * 0x9E3779B9u)) + d) & 1u) ? 1 : -1;
                CHECK(pg::frame_code_weight(seed, j, d) == want);
                plus += want > 0, all++;
            }
    CHECK(plus > all / 4 && plus < 3 * all / 4);
    std::printf("OK weight\n");

    int32_t proj[32];
    for (int i = 0; i < 32; i++) proj[i] = i % 3 == 0 ? -(i + 1) : i;  // 0 at i = 1? no: i = 1 -> 1; zero below
    proj[2] = 0, proj[5] = INT_MIN, proj[6] = INT_MAX, proj[31] = -1, proj[30] = 0;
    uint32_t want = 0;
    for (int i = 0; i < 32; i++)
        if (proj[i] >= 0) want |= 1u << i;
    CHECK(pg::frame_code_word(proj) == want && (want >> 2 & 1) == 1 && (want >> 5 & 1) == 0 && (want >> 30) == 1);
    std::printf("OK word\n");

    const uint32_t words[3] = {0xDEADBEEFu, 0u, 0x80000001u};
    for (uint32_t salt : {0u, 7u, 0xFFFFFFFFu})
        for (int count : {1, 3}) {
            uint32_t lo = mix(salt + 0x9E3779B9u), hi = mix(salt ^ 0x85EBCA6Bu);
            for (int i = 0; i < count; i++) lo = mix(lo ^ words[i]), hi = mix(hi + (words[i] ^ 0xC2B2AE35u));
            CHECK(pg::frame_code_key(words, count, salt) == (uint64_t(hi) << 32 | lo));
        }
    CHECK(pg::frame_code_key(words, 3, 0) != pg::frame_code_key(words, 3, 1));  // a salt counts apart
    CHECK(pg::frame_code_key_of(0, 0) == 1 && pg::frame_code_key_of(0, 5) == 5 && pg::frame_code_key_of(2, 0) == (uint64_t(2) << 32));
    std::printf("OK key\n");

    const uint64_t key = 0x123456789ABCDEFEull;  // low word ends in ..E: slots 6, 7, 0, 1, .. of 8
    for (int i = 0; i < 8; i++) CHECK(pg::frame_code_slot(key, i, 8) == uint32_t((6 + i) % 8));
    CHECK(pg::frame_code_slot(0xFFFFFFFFull, 1, 1 << 28) == 0 && pg::frame_code_slot(key, 0, 1 << 28) == 0x0ABCDEFEu);
    CHECK(pg::frame_code_probes(8) == 8 && pg::frame_code_probes(64) == 64 && pg::frame_code_probes(128) == 128 && pg::frame_code_probes(1 << 28) == 128);
    std::printf("OK probe\nALL OK\n");
    return 0;
}
