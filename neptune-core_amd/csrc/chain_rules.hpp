// Consensus integers of the header-chain rules (Block::validate 0.a, 0.d-0.g and has_proof_of_work's
// target), one definition for the host (nhip_difficulty_target, nhip_difficulty_control,
// tests/native/chain_rules_check.cpp) and the device (k_block_links).  Plain C++: no HIP header, no
// inline assembly; under HIP the functions are __host__ __device__.
//
// Restated (neptune-core/src/protocol/consensus/block/):
//   Difficulty::new       difficulty_control.rs:51-65   a value <= MINIMUM in every limb becomes MINIMUM
//   Difficulty::target    :69-76    (p^5 - 1) / difficulty, the quotient as a Digest (five base-p digits,
//                                   element 0 the lowest: the Digest <-> BigUint order is twenty-first's,
//                                   unpinned, and the one digest_le already assumes).  target() divides by
//                                   the limbs as they were deserialized: no clamp here.  A zero difficulty
//                                   panics in the reference (division by zero); here it is reported
//                                   (false) and the caller fails closed.
//   safe_mul_fixed_point_rational  :82-109   its result goes through Difficulty::new
//   ProofOfWork + Difficulty       :258-283  6 limbs plus 5, wrapping
//   difficulty_control    :441-486  genesis-parent shortcut, i128 relative error clamped to
//                                   [-2^32, 4 * 2^32], overflow -> MAXIMUM.  `as i64` and the i64
//                                   subtraction wrap as a release build does.  A zero interval panics in
//                                   the reference (division by zero); here it is reported (false).
//   should_reset_difficulty        mod.rs:903-913
//   Timestamp +, -, BlockHeight::next   timestamp.rs:77-91, block_height.rs:67-69: Goldilocks field
//                                   operations on canonical values; comparisons on canonical values
//                                   (timestamp.rs:61-65)
#pragma once
#include <stdint.h>

#ifdef __HIP__
#define NHIP_HD __host__ __device__ inline
#else
#define NHIP_HD inline
#endif

namespace nhip {
namespace chain {

static constexpr uint64_t P = 0xFFFFFFFF00000001ull;
static constexpr int DIFFICULTY_LIMBS = 5, POW_LIMBS = 6;
static constexpr uint32_t DIFFICULTY_MINIMUM_LIMB0 = 6000;  // difficulty_control.rs:47
static constexpr uint64_t FUTUREDATING_LIMIT_MS = 5 * 60 * 1000;  // block/mod.rs:106

// canonical a, b < p
NHIP_HD uint64_t gl_add(uint64_t a, uint64_t b) {
    const uint64_t s = a + b;  // < 2^65: a carry out means s + 2^64 >= p
    return (s < a || s >= P) ? s - P : s;
}
NHIP_HD uint64_t gl_sub(uint64_t a, uint64_t b) { return a >= b ? a - b : a + (P - b); }

NHIP_HD void difficulty_new(uint32_t d[DIFFICULTY_LIMBS]) {
    bool lte_minimum = d[0] <= DIFFICULTY_MINIMUM_LIMB0;
    for (int i = 1; i < DIFFICULTY_LIMBS; ++i) lte_minimum = lte_minimum && d[i] == 0;
    if (lte_minimum) {
        d[0] = DIFFICULTY_MINIMUM_LIMB0;
        for (int i = 1; i < DIFFICULTY_LIMBS; ++i) d[i] = 0;
    }
}

// r = 2 r + bit over N limbs; returns the bit shifted out
template <int N>
NHIP_HD uint32_t shl1(uint32_t r[N], uint32_t bit) {
    for (int i = 0; i < N; ++i) {
        const uint32_t out = r[i] >> 31;
        r[i] = (r[i] << 1) | bit;
        bit = out;
    }
    return bit;
}
template <int N>
NHIP_HD bool geq(const uint32_t a[N], const uint32_t b[N]) {
    for (int i = N - 1; i >= 0; --i)
        if (a[i] != b[i]) return a[i] > b[i];
    return true;
}
template <int N>
NHIP_HD void sub_in_place(uint32_t a[N], const uint32_t b[N]) {
    uint64_t borrow = 0;
    for (int i = 0; i < N; ++i) {
        const uint64_t d = (uint64_t)a[i] - b[i] - borrow;
        a[i] = (uint32_t)d;
        borrow = (d >> 32) & 1u;
    }
}

// p^5 - 1 as ten u32 limbs, low first
NHIP_HD void max_threshold(uint32_t m[10]) {
    for (int i = 0; i < 10; ++i) m[i] = 0;
    m[0] = 1;
    for (int k = 0; k < 5; ++k) {  // m *= p, with p = 2^64 - 2^32 + 1: m + (m << 64) - (m << 32)
        uint32_t t[10];
        for (int i = 0; i < 10; ++i) t[i] = m[i];
        uint64_t carry = 0;
        int64_t borrow = 0;
        for (int i = 0; i < 10; ++i) {
            const uint64_t add = (uint64_t)t[i] + (i >= 2 ? t[i - 2] : 0u) + carry;
            carry = add >> 32;
            int64_t v = (int64_t)(add & 0xFFFFFFFFull) - (int64_t)(i >= 1 ? t[i - 1] : 0u) - borrow;
            borrow = 0;
            if (v < 0) {
                v += (int64_t)1 << 32;
                borrow = 1;
            }
            m[i] = (uint32_t)v;
        }
        // a borrow out of limb 9 is paid by the carry out of it (the product fits 320 bits)
    }
    uint32_t one[10] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    sub_in_place<10>(m, one);
}

// Difficulty::target.  false: the difficulty is zero (out is then all zero).
NHIP_HD bool difficulty_target(const uint32_t difficulty[DIFFICULTY_LIMBS], uint64_t out[5]) {
    for (int i = 0; i < 5; ++i) out[i] = 0;
    uint32_t dv[6] = {difficulty[0], difficulty[1], difficulty[2], difficulty[3], difficulty[4], 0};
    if ((dv[0] | dv[1] | dv[2] | dv[3] | dv[4]) == 0) return false;
    uint32_t num[10], q[10], r[6] = {0, 0, 0, 0, 0, 0};
    max_threshold(num);
    // restoring division, one numerator bit at a time: r < divisor < 2^160 before the shift, so 2 r + 1
    // fits the sixth limb
    for (int i = 0; i < 10; ++i) q[i] = 0;
    for (int bit = 319; bit >= 0; --bit) {
        shl1<6>(r, (num[bit >> 5] >> (bit & 31)) & 1u);
        if (geq<6>(r, dv)) {
            sub_in_place<6>(r, dv);
            q[bit >> 5] |= 1u << (bit & 31);
        }
    }
    // the quotient's base-p digits, lowest first: divide by p five times (q < p^5)
    const uint32_t pl[3] = {1u, 0xFFFFFFFFu, 0u};
    for (int digit = 0; digit < 5; ++digit) {
        uint32_t rem[3] = {0, 0, 0};
        for (int bit = 319; bit >= 0; --bit) {
            shl1<3>(rem, (q[bit >> 5] >> (bit & 31)) & 1u);
            const bool ge = geq<3>(rem, pl);
            if (ge) sub_in_place<3>(rem, pl);
            q[bit >> 5] = (q[bit >> 5] & ~(1u << (bit & 31))) | ((ge ? 1u : 0u) << (bit & 31));
        }
        out[digit] = ((uint64_t)rem[1] << 32) | rem[0];
    }
    return true;
}

// ProofOfWork + Difficulty
NHIP_HD void pow_add(const uint32_t pow[POW_LIMBS], const uint32_t difficulty[DIFFICULTY_LIMBS], uint32_t out[POW_LIMBS]) {
    uint64_t carry = 0;
    for (int i = 0; i < POW_LIMBS; ++i) {
        const uint64_t sum = carry + pow[i] + (i < DIFFICULTY_LIMBS ? difficulty[i] : 0u);
        out[i] = (uint32_t)sum;
        carry = sum >> 32;
    }
}

// Difficulty::safe_mul_fixed_point_rational; returns the out-of-bounds limb
NHIP_HD uint32_t safe_mul_fixed_point_rational(const uint32_t d[DIFFICULTY_LIMBS], uint32_t lo, uint32_t hi,
                                               uint32_t out[DIFFICULTY_LIMBS]) {
    uint32_t nd[DIFFICULTY_LIMBS + 1];
    uint32_t carry = 0;
    for (int i = 0; i < DIFFICULTY_LIMBS; ++i) {
        const uint64_t sum = (uint64_t)carry + (uint64_t)d[i] * lo;
        nd[i] = (uint32_t)sum;
        carry = (uint32_t)(sum >> 32);
    }
    nd[DIFFICULTY_LIMBS] = carry;
    carry = 0;
    for (int i = 0; i < DIFFICULTY_LIMBS; ++i) {
        const uint64_t sum = (uint64_t)carry + (uint64_t)d[i] * hi;
        const uint32_t digit = nd[i + 1] + (uint32_t)sum;
        const uint32_t carry_bit = digit < nd[i + 1] ? 1u : 0u;
        nd[i + 1] = digit;
        carry = (uint32_t)(sum >> 32) + carry_bit;
    }
    for (int i = 0; i < DIFFICULTY_LIMBS; ++i) out[i] = nd[i + 1];
    difficulty_new(out);
    return carry;
}

// a * b as (hi, lo)
NHIP_HD void mul64(uint64_t a, uint64_t b, uint64_t& hi, uint64_t& lo) {
    const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;
    lo = (mid << 32) | (uint32_t)p00;
    hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

// difficulty_control.  Timestamps and the interval canonical (< p).  false: target_block_interval is zero and
// the parent is not the genesis block, where the reference divides by it and panics (out is then all zero).
NHIP_HD bool difficulty_control(uint64_t new_timestamp, uint64_t old_timestamp, const uint32_t old_difficulty[DIFFICULTY_LIMBS],
                                uint64_t target_block_interval, uint64_t previous_block_height,
                                uint32_t out[DIFFICULTY_LIMBS]) {
    if (previous_block_height == 0) {  // BlockHeight::is_genesis
        for (int i = 0; i < DIFFICULTY_LIMBS; ++i) out[i] = old_difficulty[i];
        return true;
    }
    if (target_block_interval == 0) {
        for (int i = 0; i < DIFFICULTY_LIMBS; ++i) out[i] = 0;
        return false;
    }
    const uint64_t delta_t = gl_sub(new_timestamp, old_timestamp);
    const int64_t absolute_error = (int64_t)(delta_t - target_block_interval);  // (as i64) - (as i64), wrapping
    const uint64_t per = (1ull << 32) / target_block_interval;                  // (1 << 32) / i128::from(interval)
    // relative_error = absolute_error * per, clamped to [-2^32, 4 * 2^32]
    int64_t clamped;
    uint64_t hi, lo;
    if (absolute_error >= 0) {
        mul64((uint64_t)absolute_error, per, hi, lo);
        clamped = (hi != 0 || lo > (4ull << 32)) ? (int64_t)(4ull << 32) : (int64_t)lo;
    } else {
        mul64(0ull - (uint64_t)absolute_error, per, hi, lo);
        clamped = (hi != 0 || lo > (1ull << 32)) ? -(int64_t)(1ull << 32) : -(int64_t)lo;
    }
    // (1 << 32) + ((-clamped) >> 4), the shift arithmetic (rounding down)
    const int64_t neg = -clamped;
    const int64_t shifted = neg >= 0 ? (neg >> 4) : -((-neg + 15) >> 4);
    const int64_t one_plus_p_times_error = ((int64_t)1 << 32) + shifted;
    const uint32_t flo = (uint32_t)one_plus_p_times_error;
    const uint32_t fhi = (uint32_t)((uint64_t)one_plus_p_times_error >> 32);
    const uint32_t overflow = safe_mul_fixed_point_rational(old_difficulty, flo, fhi, out);
    if (overflow > 0)
        for (int i = 0; i < DIFFICULTY_LIMBS; ++i) out[i] = 0xFFFFFFFFu;  // Difficulty::MAXIMUM
    return true;
}

// Block::should_reset_difficulty; reset_interval 0: the network has none
NHIP_HD bool should_reset_difficulty(uint64_t reset_interval, uint64_t current_timestamp, uint64_t previous_timestamp) {
    if (reset_interval == 0) return false;
    return gl_sub(current_timestamp, previous_timestamp) >= reset_interval;
}

NHIP_HD uint64_t height_next(uint64_t h) { return gl_add(h, 1); }

// The header fields rules 0.a and 0.d-0.g read (canonical values)
struct LinkHeader {
    uint64_t height, timestamp;
    uint32_t cumulative_proof_of_work[POW_LIMBS];
    uint32_t difficulty[DIFFICULTY_LIMBS];
};
// Network parameters, every time already reduced mod p (Timestamp::millis is BFieldElement::new)
struct LinkParams {
    uint64_t minimum_block_time, target_block_interval, difficulty_reset_interval, now;
    uint32_t genesis_difficulty[DIFFICULTY_LIMBS];  // as Difficulty::new left it
};

NHIP_HD bool rule_0a(const LinkHeader& parent, const LinkHeader& child) { return height_next(parent.height) == child.height; }

// Rules 0.d-0.g in the reference's order (block/mod.rs:743-782): 0 when all hold, else 'd', 'e', 'f' or 'g'
NHIP_HD char rules_0d_0g(const LinkParams& np, const LinkHeader& parent, const LinkHeader& child) {
    if (gl_add(parent.timestamp, np.minimum_block_time) > child.timestamp) return 'd';
    uint32_t expected[DIFFICULTY_LIMBS];
    if (should_reset_difficulty(np.difficulty_reset_interval, child.timestamp, parent.timestamp)) {
        for (int i = 0; i < DIFFICULTY_LIMBS; ++i) expected[i] = np.genesis_difficulty[i];
    } else {
        // a zero interval (refused by chain_params_ok before any launch) fails the rule closed
        if (!difficulty_control(child.timestamp, parent.timestamp, parent.difficulty, np.target_block_interval,
                                parent.height, expected))
            return 'e';
    }
    for (int i = 0; i < DIFFICULTY_LIMBS; ++i)
        if (child.difficulty[i] != expected[i]) return 'e';
    uint32_t cumulative[POW_LIMBS];
    pow_add(parent.cumulative_proof_of_work, parent.difficulty, cumulative);
    for (int i = 0; i < POW_LIMBS; ++i)
        if (child.cumulative_proof_of_work[i] != cumulative[i]) return 'f';
    if (child.timestamp >= gl_add(np.now, FUTUREDATING_LIMIT_MS % P)) return 'g';
    return 0;
}

}  // namespace chain
}  // namespace nhip
