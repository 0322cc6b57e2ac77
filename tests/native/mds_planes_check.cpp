// Host check of the byte-planes form of the Tip5 MDS + ARK (tip5_mds_planes.hpp: signed bytes by
// offset, three coefficient digits, 24 integer dot products C_q, the biased start constants and
// mds_ark's fold) against twenty-first's step-by-step form (128-bit MDS sum, reduce, then the field
// add of the round constant), for every Tip5 round constant over edge, one-hot-byte and random
// states (run by tests/test_mds_planes_host.py).  Also asserts the ranges the device code relies
// on: the digits, |C_q| < 2^20, al without wrap, T in (2^60, 2^62).
#include "goldilocks.hpp"
#include "tip5_constants.h"
#include "tip5_mds_planes.hpp"
#include <cstdio>
#include <random>
#include <vector>
using namespace nhip;
typedef unsigned __int128 u128;

static uint64_t bad = 0, n = 0;
static int64_t cq_max = 0;
#define REQUIRE(c, ...)                                   \
    do {                                                  \
        if (!(c)) {                                       \
            if (bad < 10) { printf(__VA_ARGS__); printf("\n"); } \
            ++bad;                                        \
        }                                                 \
    } while (0)

// step-by-step: s = sum_j M[(i-j)&15] x_j (128 bits), reduce as twenty-first, then + rc in the field
static uint64_t ref_word(const uint64_t* x, int i, uint64_t rc) {
    u128 s = 0;
    for (int j = 0; j < 16; ++j) s += (u128)TIP5_MDS[(i - j) & 15] * x[j];
    uint64_t slo = (uint64_t)s, shi = (uint64_t)(s >> 64);
    uint64_t t = shi * GL_EPS;
    uint64_t res = slo + t; bool over = res < slo;
    uint64_t y = res + (over ? GL_EPS : 0);
    uint64_t q = GL_P - rc;
    uint64_t x1 = y - q;
    if (y < q) x1 += GL_P;
    return x1;
}

// the planes form of one round's 16 outputs; start[i] = planes_start(K_i)
static void planes_round(const uint64_t* x, const uint64_t* start, uint64_t* out) {
    // signed bytes: XOR 0x80 on every byte; plane d = byte d of words 0..15
    int8_t plane[8][16];
    for (int j = 0; j < 16; ++j) {
        const uint64_t w = x[j] ^ 0x8080808080808080ull;
        for (int d = 0; d < 8; ++d) plane[d][j] = (int8_t)(uint8_t)(w >> (8 * d));
    }
    for (int i = 0; i < 16; ++i) {
        int32_t C[10];
        int pairs = 0;
        for (int q = 0; q < 10; ++q) {
            C[q] = 0;
            for (int e = 0; e < 3; ++e) {
                const int d = q - e;
                if (d < 0 || d > 7) continue;
                ++pairs;
                for (int j = 0; j < 16; ++j) C[q] += (int32_t)mds_digit((i - j) & 15, e) * plane[d][j];
            }
            const int64_t a = C[q] < 0 ? -(int64_t)C[q] : C[q];
            if (a > cq_max) cq_max = a;
            REQUIRE(a < (1 << 20), "|C_%d| = %lld", q, (long long)a);
        }
        REQUIRE(pairs == 24, "%d (q, e) pairs", pairs);
        // al = start + C_0 + 2^8 C_1 + 2^16 C_2 + 2^24 C_3: four signed multiply-adds
        const __int128 alw = (__int128)start[i] + C[0] + (__int128)C[1] * 256 + (__int128)C[2] * 65536 +
                             (__int128)C[3] * 16777216;
        REQUIRE(alw >= 0 && alw < ((__int128)1 << 64), "al wraps at output %d", i);
        const uint64_t al = (uint64_t)alw;
        // T: start pair (al >> 32, C_8 + (C_9 << 8) + 2^29), then four signed multiply-adds
        const uint32_t hb = (uint32_t)C[8] + ((uint32_t)C[9] << 8) + (uint32_t)PLANES_HB_BIAS;
        REQUIRE((int32_t)hb > 0, "high dword not positive");
        const uint64_t t0 = ((uint64_t)hb << 32) | (uint32_t)(al >> 32);
        const uint64_t T = t0 + (uint64_t)((int64_t)C[4] + (int64_t)C[5] * 256 + (int64_t)C[6] * 65536 +
                                          (int64_t)C[7] * 16777216);
        REQUIRE(T > (1ull << 60) && T < (1ull << 62), "T = %llx out of range", (unsigned long long)T);
        // mds_fold4 on sh = T >> 32, slo = (T mod 2^32, al mod 2^32)
        const uint32_t sh = (uint32_t)(T >> 32);
        const uint64_t slo = ((uint64_t)(uint32_t)T << 32) | (uint32_t)al;
        const u128 W = (u128)sh * 0xFFFFFFFFull + slo;
        REQUIRE(W >= 0xFFFFFFFFull, "s'' below 2^32 - 1");
        const bool G = (W >> 64) != 0;
        REQUIRE(!G || (uint64_t)W < GL_P, "W - 2^64 not below p");
        out[i] = (uint64_t)W - (G ? 0u : 0xFFFFFFFFu);
    }
}

static void chk_state(const uint64_t* x) {
    uint64_t start[16], out[16];
    for (int r = 0; r < 5; ++r) {
        for (int i = 0; i < 16; ++i) start[i] = planes_start(TIP5_RC_RAW[r * 16 + i] + GL_EPS);
        planes_round(x, start, out);
        for (int i = 0; i < 16; ++i) {
            ++n;
            const uint64_t a = ref_word(x, i, TIP5_RC_RAW[r * 16 + i]);
            REQUIRE(a == out[i], "round %d output %d: ref=%llx planes=%llx", r, i, (unsigned long long)a,
                    (unsigned long long)out[i]);
        }
    }
}

int main() {
    // the constants
    for (int k = 0; k < 16; ++k) {
        const int e0 = mds_digit(k, 0), e1 = mds_digit(k, 1), e2 = mds_digit(k, 2);
        REQUIRE(e0 >= -128 && e0 <= 127 && e1 >= -128 && e1 <= 127 && (e2 == 0 || e2 == 1), "digits of MDS[%d]", k);
        REQUIRE(e0 + 256 * e1 + 65536 * e2 == (int)TIP5_MDS[k], "digits of MDS[%d] do not recombine", k);
    }
    for (int i = 0; i < 80; ++i) {
        const uint64_t s = planes_start(TIP5_RC_RAW[i] + GL_EPS);
        REQUIRE(s >= PLANES_START_MIN && s < PLANES_START_MAX, "start %d out of range", i);
        // start + 2^93 = K + offset mod p
        const u128 l = ((u128)s + PLANES_BIAS) % GL_P;
        const u128 rr = ((u128)(TIP5_RC_RAW[i] % GL_P) + GL_EPS + PLANES_OFFSET) % GL_P;
        REQUIRE(l == rr, "start %d is not K + offset - bias", i);
    }
    // the constant tiles: each row of the 32 x 32 tile is non-zero in exactly one lane half, and
    // register r of either half is output r
    for (int e = 0; e < 3; ++e)
        for (int l = 0; l < 64; ++l) {
            const int row = l & 31, own = (row >> 2) & 1, r = (row & 3) + 4 * (row >> 3);
            for (int t = 0; t < 16; ++t) {
                const int want = (l >> 5) == own ? mds_digit((r - t) & 15, e) : 0;
                REQUIRE(planes_tile_byte(e, l, t) == want, "tile %d lane %d byte %d", e, l, t);
            }
            REQUIRE((r & 3) + 8 * (r >> 2) + 4 * own == row, "row map of register %d", r);
        }
    // states
    std::mt19937_64 g(17);
    uint64_t x[16];
    const uint64_t fills[] = {0ull, ~0ull, 0x8080808080808080ull, 0x7F7F7F7F7F7F7F7Full, GL_P - 1,
                              0x00000000FFFFFFFFull, 0xFFFFFFFF00000000ull};
    for (uint64_t f : fills) {
        for (int j = 0; j < 16; ++j) x[j] = f;
        chk_state(x);
        for (int k = 0; k < 16; ++k) {  // one word of the fill, the others 0 and the reverse
            for (int j = 0; j < 16; ++j) x[j] = j == k ? f : 0;
            chk_state(x);
            for (int j = 0; j < 16; ++j) x[j] = j == k ? 0 : f;
            chk_state(x);
        }
    }
    for (int b = 0; b < 128; ++b)  // one-hot bytes
        for (uint64_t v : {0x01ull, 0xFFull, 0x80ull, 0x7Full}) {
            for (int j = 0; j < 16; ++j) x[j] = 0;
            x[b >> 3] = v << (8 * (b & 7));
            chk_state(x);
        }
    // the states that push C_q to either end: bytes 0x00 / 0xFF chosen by the sign of a digit
    for (int e = 0; e < 2; ++e)
        for (int i = 0; i < 16; ++i)
            for (int sgn = 0; sgn < 2; ++sgn) {
                for (int j = 0; j < 16; ++j) x[j] = ((mds_digit((i - j) & 15, e) < 0) == (sgn != 0)) ? ~0ull : 0ull;
                chk_state(x);
            }
    for (int it = 0; it < 200000; ++it) {
        for (int j = 0; j < 16; ++j) x[j] = g();
        if (it & 1)
            for (int j = 0; j < 16; ++j) x[j] %= GL_P;
        chk_state(x);
    }
    printf("checked %llu, bad %llu, max |C_q| %lld\n", (unsigned long long)n, (unsigned long long)bad, (long long)cq_max);
    return bad != 0;
}
