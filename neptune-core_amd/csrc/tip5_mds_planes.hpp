// Constants of the "byte planes" form of the Tip5 MDS + ARK: the 16 x 16 circulant applied with
// v_mfma_i32_32x32x32_i8 to the state's bytes as they lie in the registers, one state per lane.
// Shared by the device code, tools/mds_planes_microbench.hip and tests/native/mds_planes_check.cpp
// (which runs the whole form with host integers against the step-by-step form).
//
//   * bytes: word j = sum_d u[j][d] 2^(8d); v = u - 128 = (int8)(u ^ 0x80), so
//     s_i = sum_j M[(i-j)&15] x_j = sum_d 2^(8d) sum_j M[(i-j)&15] v[j][d] + PLANES_OFFSET, with
//     PLANES_OFFSET = 128 * 0x0101010101010101 * sum(M) the same for every output (circulant);
//   * digits: M[k] = e0 + 2^8 e1 + 2^16 e2, e0, e1 in [-128, 127], e2 in {0, 1} (mds_digit);
//   * C_q[i] = sum over e + d = q of sum_j digit_e[(i-j)&15] v[j][d], q = 0..9: 24 (q, e) pairs,
//     |C_q| < 2^20, and s_i = sum_q 2^(8q) C_q[i] + PLANES_OFFSET;
//   * the high dword Hb = C_8 + (C_9 << 8) + PLANES_HB_BIAS (2^29) is positive;
//   * al = start + C_0 + 2^8 C_1 + 2^16 C_2 + 2^24 C_3 (64-bit, never wraps: start is in
//     [2^45, 2^64 - 2^45) and the sum's magnitude is < 2^45);
//     T  = (al >> 32) + Hb 2^32 + C_4 + 2^8 C_5 + 2^16 C_6 + 2^24 C_7, in (2^60, 2^62);
//     s'' = (al mod 2^32) + 2^32 T is mds_ark's accumulator pair with m1 = T mod 2^32, sh = T >> 32
//     already summed (the fold's add-with-carry of al's high half into ah is the start of T);
//   * start = K + PLANES_OFFSET - 2^93 mod p with K = RC + 2^32 - 1 (2^93 = PLANES_HB_BIAS 2^64),
//     so s'' = s + K mod p, and the fold's preconditions hold: s'' >= 2^32 - 1 (T > 2^60),
//     sh < 2^30, W - 2^64 < p.  The result is the canonical word mds_ark_fold gives.
#pragma once
#include <stdint.h>

#include "tip5_constants.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NHIP_PLANES_HD __host__ __device__
#else
#define NHIP_PLANES_HD
#endif

namespace nhip {

static constexpr uint64_t PLANES_P = 0xFFFFFFFF00000001ull;
static constexpr int32_t PLANES_HB_BIAS = 1 << 29;
static constexpr uint64_t PLANES_START_MIN = 1ull << 45;
static constexpr uint64_t PLANES_START_MAX = 0ull - (1ull << 45);  // exclusive

// digit e (0, 1, 2) of coefficient MDS[k]
NHIP_PLANES_HD constexpr int mds_digit(int k, int e) {
    const int m = (int)TIP5_MDS[k];
    const int b0 = m & 0xFF;
    const int e0 = b0 < 128 ? b0 : b0 - 256;
    const int m1 = (m - e0) >> 8;  // 0 .. 256
    const int b1 = m1 & 0xFF;
    const int e1 = b1 < 128 ? b1 : b1 - 256;
    const int e2 = (m1 - e1) >> 8;
    return e == 0 ? e0 : e == 1 ? e1 : e2;
}
constexpr bool mds_digits_in_range() {
    for (int k = 0; k < 16; ++k) {
        const int e0 = mds_digit(k, 0), e1 = mds_digit(k, 1), e2 = mds_digit(k, 2);
        if (e0 < -128 || e0 > 127 || e1 < -128 || e1 > 127 || e2 < 0 || e2 > 1) return false;
        if (e0 + 256 * e1 + 65536 * e2 != (int)TIP5_MDS[k]) return false;
    }
    return true;
}
static_assert(mds_digits_in_range(), "every MDS coefficient is e0 + 2^8 e1 + 2^16 e2 in signed bytes");

// The largest |C_q| any state can give: per output, sum over the round's 16 coefficients of
// 128 * (|e0| + |e1| + |e2|) (q = 2..7 take one digit of each index; the others fewer).
constexpr int64_t planes_cq_bound() {
    int64_t b = 0;
    for (int k = 0; k < 16; ++k) {
        int64_t a = 0;
        for (int e = 0; e < 3; ++e) a += mds_digit(k, e) < 0 ? -mds_digit(k, e) : mds_digit(k, e);
        b += 128 * a;
    }
    return b;
}
static_assert(planes_cq_bound() < (1 << 20), "|C_q| < 2^20");

constexpr uint64_t planes_mod_p(unsigned __int128 x) { return (uint64_t)(x % PLANES_P); }
constexpr uint64_t planes_mds_sum() {
    uint64_t s = 0;
    for (int k = 0; k < 16; ++k) s += TIP5_MDS[k];
    return s;
}
// 128 * 0x0101010101010101 * sum(M) mod p
static constexpr uint64_t PLANES_OFFSET =
    planes_mod_p((unsigned __int128)0x8080808080808080ull * planes_mds_sum());
// 2^93 mod p: what PLANES_HB_BIAS adds to s''
static constexpr uint64_t PLANES_BIAS = planes_mod_p((unsigned __int128)1 << 93);

// The low accumulator's start for a folded constant k = K (mds_ark's start, RC + 2^32 - 1, or
// tip5_rck0_fixed): k + PLANES_OFFSET - PLANES_BIAS mod p.
NHIP_PLANES_HD constexpr uint64_t planes_start(uint64_t k) {
    return (uint64_t)(((unsigned __int128)(k % PLANES_P) + PLANES_OFFSET + (PLANES_P - PLANES_BIAS)) % PLANES_P);
}
constexpr bool planes_start_in_range(uint64_t k) {
    return planes_start(k) >= PLANES_START_MIN && planes_start(k) < PLANES_START_MAX;
}
constexpr bool planes_starts_in_range() {
    for (int i = 0; i < 80; ++i)
        if (!planes_start_in_range(TIP5_RC_RAW[i] + 0xFFFFFFFFull)) return false;
    return true;
}
static_assert(planes_starts_in_range(), "al = start + L neither under- nor overflows for any Tip5 round constant");

// Byte t (0..15) of lane l's A fragment of constant tile e.  v_mfma_i32_32x32x32_i8 gives lane
// n + 32 g, in result register r, row (r & 3) + 8 (r >> 2) + 4 g of column n, and takes column n
// of B from lanes n and n + 32 (one half of K each), as it takes row l & 31 of A from lanes
// l & 31 and (l & 31) + 32.  A row owned by lane half g is non-zero only in the fragment of lane
// half g, where it holds the circulant's row of output i = r against the words t = 0..15 of a
// plane: register r of a lane is output r of the lane's own state, whatever the order of K within
// a fragment is (A and B share it).
NHIP_PLANES_HD constexpr int planes_tile_byte(int e, int l, int t) {
    const int row = l & 31, half = l >> 5;
    if (((row >> 2) & 1) != half) return 0;
    const int i = (row & 3) + 4 * (row >> 3);
    return mds_digit((i - t) & 15, e);
}

}  // namespace nhip
