// The consensus integers of the header-chain rules (csrc/chain_rules.hpp) and the shape checks of their entry
// points (csrc/chain_shape.cpp) under ASan + UBSan (tests/test_chain_rules.py): Difficulty::target, the control
// law, the limb additions and the field arithmetic of timestamps against a naive recomputation on bit vectors
// (one bit per element: shift-and-add products, shift-and-subtract quotients) and, for the i128 steps of the
// control law, on __int128.  Inputs: the edge values the rules turn on and seeded random ones.  Host only: links
// no HIP.
#include <cstdio>
#include <cstdint>
#include <random>
#include <vector>

#include "../../neptune-core_amd/csrc/chain_rules.hpp"
#include "../../neptune-core_amd/csrc/chain_shape.hpp"

namespace {

namespace C = nhip::chain;
int checks = 0, failures = 0;

void expect(bool ok, const char* what) {
    ++checks;
    if (!ok) {
        std::fprintf(stderr, "FAIL %s\n", what);
        ++failures;
    }
}

// ---- naive unsigned integers: bits, lowest first
using Bits = std::vector<uint8_t>;
Bits trim(Bits a) {
    while (!a.empty() && a.back() == 0) a.pop_back();
    return a;
}
Bits from_u64(uint64_t v) {
    Bits b;
    for (int i = 0; i < 64; ++i) b.push_back((v >> i) & 1);
    return trim(b);
}
Bits from_limbs(const uint32_t* l, int n) {
    Bits b;
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 32; ++k) b.push_back((l[i] >> k) & 1);
    return trim(b);
}
int cmp(const Bits& a, const Bits& b) {
    if (a.size() != b.size()) return a.size() < b.size() ? -1 : 1;
    for (size_t i = a.size(); i-- > 0;)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return 0;
}
Bits add(const Bits& a, const Bits& b) {
    Bits r;
    uint8_t carry = 0;
    for (size_t i = 0; i < a.size() || i < b.size() || carry; ++i) {
        const uint8_t s = (i < a.size() ? a[i] : 0) + (i < b.size() ? b[i] : 0) + carry;
        r.push_back(s & 1);
        carry = s >> 1;
    }
    return trim(r);
}
Bits sub(const Bits& a, const Bits& b) {  // a >= b
    Bits r;
    int borrow = 0;
    for (size_t i = 0; i < a.size(); ++i) {
        int s = a[i] - (i < b.size() ? b[i] : 0) - borrow;
        borrow = s < 0;
        r.push_back((uint8_t)(s & 1));
    }
    return trim(r);
}
Bits shl(const Bits& a, size_t k) {
    if (a.empty()) return a;
    Bits r(k, 0);
    r.insert(r.end(), a.begin(), a.end());
    return r;
}
Bits shr(const Bits& a, size_t k) { return k >= a.size() ? Bits{} : Bits(a.begin() + k, a.end()); }
Bits low(const Bits& a, size_t k) { return trim(a.size() > k ? Bits(a.begin(), a.begin() + k) : a); }
Bits mul(const Bits& a, const Bits& b) {
    Bits r;
    for (size_t i = 0; i < b.size(); ++i)
        if (b[i]) r = add(r, shl(a, i));
    return r;
}
void divmod(const Bits& a, const Bits& b, Bits& q, Bits& r) {  // b != 0
    q.assign(a.size(), 0);
    r.clear();
    for (size_t i = a.size(); i-- > 0;) {
        r.insert(r.begin(), a[i]);
        r = trim(r);
        if (cmp(r, b) >= 0) {
            r = sub(r, b);
            q[i] = 1;
        }
    }
    q = trim(q);
}
uint64_t to_u64(const Bits& a) {
    uint64_t v = 0;
    for (size_t i = 0; i < a.size() && i < 64; ++i) v |= (uint64_t)a[i] << i;
    return v;
}
void to_limbs(const Bits& a, uint32_t* l, int n) {
    for (int i = 0; i < n; ++i) {
        l[i] = 0;
        for (int k = 0; k < 32; ++k)
            if ((size_t)(32 * i + k) < a.size()) l[i] |= (uint32_t)a[32 * i + k] << k;
    }
}

const Bits BP = from_u64(C::P);

// ---- the checks
void check_target(const uint32_t d[5]) {
    uint64_t got[5];
    const bool ok = C::difficulty_target(d, got);
    const Bits den = from_limbs(d, 5);
    if (den.empty()) {
        expect(!ok && !(got[0] | got[1] | got[2] | got[3] | got[4]), "target: zero difficulty reported");
        return;
    }
    Bits num = from_u64(1);
    for (int i = 0; i < 5; ++i) num = mul(num, BP);
    num = sub(num, from_u64(1));
    Bits q, r;
    divmod(num, den, q, r);
    // the identity: q * d <= p^5 - 1 < (q + 1) * d
    expect(cmp(mul(q, den), num) <= 0 && cmp(mul(add(q, from_u64(1)), den), num) > 0, "target: naive quotient identity");
    Bits back;
    bool same = ok;
    for (int i = 0; i < 5; ++i) {
        Bits digit, rest;
        divmod(q, BP, rest, digit);
        q = rest;
        same = same && to_u64(digit) == got[i] && got[i] < C::P;
        back = add(back, mul(from_u64(got[i]), [&] {
                       Bits pw = from_u64(1);
                       for (int k = 0; k < i; ++k) pw = mul(pw, BP);
                       return pw;
                   }()));
    }
    expect(same && q.empty(), "target: digits");
    expect(cmp(mul(back, den), num) <= 0 && cmp(mul(add(back, from_u64(1)), den), num) > 0, "target: identity on the digits");
}

void naive_new(uint32_t d[5]) {
    if (d[0] <= 6000 && !d[1] && !d[2] && !d[3] && !d[4]) {
        d[0] = 6000;
    }
}

void check_control(uint64_t new_ts, uint64_t old_ts, const uint32_t d[5], uint64_t interval, uint64_t height) {
    uint32_t got[5], want[5];
    const bool reported = C::difficulty_control(new_ts, old_ts, d, interval, height, got);
    expect(reported, "difficulty_control: a non-zero interval is never reported");
    if (height == 0) {
        for (int i = 0; i < 5; ++i) want[i] = d[i];
    } else {
        const unsigned __int128 p = C::P;
        const uint64_t delta = (uint64_t)(((unsigned __int128)new_ts + p - old_ts) % p);
        const int64_t abs_err = (int64_t)((uint64_t)(int64_t)delta - (uint64_t)(int64_t)interval);  // wrapping, as a release build
        __int128 rel = (__int128)abs_err * (((__int128)1 << 32) / (__int128)interval);
        const __int128 lo_c = -((__int128)1 << 32), hi_c = (__int128)4 << 32;
        rel = rel < lo_c ? lo_c : rel > hi_c ? hi_c : rel;
        const uint64_t factor = (uint64_t)(((__int128)1 << 32) + ((-rel) >> 4));  // i128 >> is arithmetic, as Rust's
        // old * factor on bit vectors: the result is bits 32..191, the overflow whatever lies above
        const Bits prod = mul(from_limbs(d, 5), from_u64(factor));
        to_limbs(low(shr(prod, 32), 160), want, 5);
        naive_new(want);
        if (!shr(prod, 192).empty())
            for (int i = 0; i < 5; ++i) want[i] = 0xFFFFFFFFu;
    }
    bool same = true;
    for (int i = 0; i < 5; ++i) same = same && got[i] == want[i];
    expect(same, "difficulty_control");
}

void check_pow_add(const uint32_t pow[6], const uint32_t d[5]) {
    uint32_t got[6], want[6];
    C::pow_add(pow, d, got);
    to_limbs(low(add(from_limbs(pow, 6), from_limbs(d, 5)), 192), want, 6);
    bool same = true;
    for (int i = 0; i < 6; ++i) same = same && got[i] == want[i];
    expect(same, "pow_add");
}

void check_field(uint64_t a, uint64_t b) {
    const unsigned __int128 p = C::P;
    expect(C::gl_add(a, b) == (uint64_t)(((unsigned __int128)a + b) % p), "gl_add");
    expect(C::gl_sub(a, b) == (uint64_t)(((unsigned __int128)a + p - b) % p), "gl_sub");
}

void check_shapes() {
    const int64_t good[4] = {-1, 0, 3, 2}, low_[2] = {-2, 0}, high[2] = {0, 2};
    expect(nhip::chain_parents_ok(good, 4) == NHIP_OK, "parents: -1 and 0..n-1");
    expect(nhip::chain_parents_ok(low_, 2) == NHIP_ERR_ARG, "parents: -2");
    expect(nhip::chain_parents_ok(high, 2) == NHIP_ERR_ARG, "parents: n");
    expect(nhip::chain_parents_ok(nullptr, 2) == NHIP_ERR_ARG, "parents: null");
    expect(nhip::chain_parents_ok(nullptr, 0) == NHIP_OK, "parents: none");
    const uint8_t bytes[64] = {};
    nhip_blk_block b[2] = {};
    b[0].offset = 0, b[0].size = 40, b[1].offset = 40, b[1].size = 24;
    expect(nhip::chain_blocks_ok(bytes, 64, b, 2) == NHIP_OK, "blocks: inside");
    expect(nhip::chain_blocks_ok(bytes, 63, b, 2) == NHIP_ERR_ARG, "blocks: past the end");
    expect(nhip::chain_blocks_ok(nullptr, 64, b, 2) == NHIP_ERR_ARG, "blocks: null bytes");
    expect(nhip::chain_blocks_ok(bytes, 64, nullptr, 2) == NHIP_ERR_ARG, "blocks: null blocks");
    expect(nhip::chain_blocks_ok(nullptr, 0, nullptr, 0) == NHIP_OK, "blocks: none");
    b[1].offset = ~0ull;
    expect(nhip::chain_blocks_ok(bytes, 64, b, 2) == NHIP_ERR_ARG, "blocks: offset wraps");
    nhip_chain_params p = {};
    C::LinkParams lp;
    p.minimum_block_time_ms = 60000, p.target_block_interval_ms = 588000, p.genesis_difficulty[0] = 17, p.pow_tree_height = 29;
    p.now_ms = C::P + 5;
    expect(nhip::chain_params_ok(&p, &lp) == NHIP_OK && lp.genesis_difficulty[0] == 6000 && lp.now == 5 &&
               lp.target_block_interval == 588000,
           "params: reduced, clamped");
    p.target_block_interval_ms = C::P;
    expect(nhip::chain_params_ok(&p, &lp) == NHIP_ERR_ARG, "params: zero interval mod p");
    p.target_block_interval_ms = 100, p.pow_tree_height = 0;
    expect(nhip::chain_params_ok(&p, &lp) == NHIP_ERR_ARG, "params: tree height 0");
    p.pow_tree_height = 33;
    expect(nhip::chain_params_ok(&p, &lp) == NHIP_ERR_ARG, "params: tree height 33");
    expect(nhip::chain_params_ok(nullptr, &lp) == NHIP_ERR_ARG, "params: null");
}

void check_rule_order() {
    C::LinkParams np = {};
    np.minimum_block_time = 60000, np.target_block_interval = 588000, np.now = 10000000;
    np.genesis_difficulty[0] = 6000;
    C::LinkHeader parent = {}, child = {};
    parent.height = 0, parent.timestamp = 1000000, parent.difficulty[0] = 70000;
    parent.cumulative_proof_of_work[0] = 0xFFFFFFFFu;
    child.height = 1, child.timestamp = 1060000, child.difficulty[0] = 70000;
    child.cumulative_proof_of_work[0] = 69999, child.cumulative_proof_of_work[1] = 1;
    expect(C::rule_0a(parent, child) && C::rules_0d_0g(np, parent, child) == 0, "rules: all hold");
    C::LinkHeader c2 = child;
    c2.timestamp = 1059999;
    expect(C::rules_0d_0g(np, parent, c2) == 'd', "rules: one millisecond under the minimum");
    c2 = child, c2.difficulty[0] ^= 1, c2.cumulative_proof_of_work[0] ^= 1;
    expect(C::rules_0d_0g(np, parent, c2) == 'e', "rules: 0.e before 0.f");
    c2 = child, c2.cumulative_proof_of_work[5] = 1;
    np.now = 0;
    expect(C::rules_0d_0g(np, parent, c2) == 'f', "rules: 0.f before 0.g");
    expect(C::rules_0d_0g(np, parent, child) == 'g', "rules: future dated");
    np.now = 1060000 - 300000;
    expect(C::rules_0d_0g(np, parent, child) == 'g', "rules: exactly at the limit");
    np.now += 1;
    expect(C::rules_0d_0g(np, parent, child) == 0, "rules: one millisecond inside the limit");
    parent.timestamp = C::P - 30000;  // prev.timestamp + minimum_block_time wraps mod p
    child.timestamp = 30000 - 1, np.now = C::P - 1;
    expect(C::rules_0d_0g(np, parent, child) == 'd', "rules: the wrapped sum is what is compared");
    child.timestamp = 30000, child.height = C::P - 1, parent.height = C::P - 2;
    expect(C::rule_0a(parent, child), "rules: height is a field element");
    parent.height = C::P - 1, child.height = 0;
    expect(C::rule_0a(parent, child), "rules: next() of p - 1 is 0");
    expect(C::should_reset_difficulty(1000, 5, 10) && !C::should_reset_difficulty(0, 5, 10) &&
               C::should_reset_difficulty(1000, 2000, 1000) && !C::should_reset_difficulty(1000, 1999, 1000),
           "should_reset_difficulty");
}

}  // namespace

int main() {
    std::mt19937_64 g(20250);
    const uint32_t edges[][5] = {{6000, 0, 0, 0, 0},   {5999, 0, 0, 0, 0}, {1, 0, 0, 0, 0},
                                 {0, 0, 0, 0, 0},      {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu},
                                 {0, 1, 0, 0, 0},      {0, 0, 0, 0, 0x80000000u}, {6001, 0, 0, 0, 0},
                                 {0xFFFFFFFFu, 0, 0, 0, 0}, {0, 0, 0, 0, 1}};
    const uint64_t target = 588000, minimum = 60000, t0 = 1754420400000ull;
    for (const auto& d : edges) {
        check_target(d);
        const uint64_t pairs[][4] = {{t0 + target, t0, target, 0},         {t0 + minimum, t0, target, 7},
                                     {t0 + target, t0, target, 7},         {t0 + 5 * target, t0, target, 7},
                                     {t0 + 1000 * target, t0, target, 7},  {t0, t0 + 1, target, 7},
                                     {3, C::P - 5, target, 7},             {t0 + 1, t0, 1, 7},
                                     {t0 + 99, t0, 100, 1},                {t0 + 7, t0, (1ull << 32) + 1, 2},
                                     {t0 + 7, t0, C::P - 1, 2},            {C::P - 1, 0, 1, 9}};
        for (const auto& c : pairs) check_control(c[0], c[1], d, c[2], c[3]);
        const uint32_t pmax[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        const uint32_t pzero[6] = {};
        check_pow_add(pmax, d);
        check_pow_add(pzero, d);
    }
    auto limb = [&]() -> uint32_t {
        const unsigned w = (unsigned)(g() % 3);
        return w == 0 ? (uint32_t)(g() & 1) : w == 1 ? (uint32_t)(g() & 0x1FFF) : (uint32_t)g();
    };
    for (int it = 0; it < 1200; ++it) {
        uint32_t d[5], pw[6];
        for (auto& x : d) x = limb();
        for (auto& x : pw) x = (uint32_t)g();
        check_target(d);  // a naive 320-bit division each
        const uint64_t choices[4] = {100, 588000, 1 + g() % (1ull << 33), 1 + g() % (C::P - 1)};
        const uint64_t interval = choices[g() % 4];
        const uint64_t old_ts = g() % C::P;
        const uint64_t new_ts = (g() & 1) ? (uint64_t)(((unsigned __int128)old_ts + g() % (10 * (interval % (1ull << 40)) + 1)) % C::P)
                                          : g() % C::P;
        check_control(new_ts, old_ts, d, interval, (g() % 3) ? g() % (1u << 20) : 0);
        check_pow_add(pw, d);
        check_field(g() % C::P, g() % C::P);
    }
    {  // a zero interval: reported unless the parent is the genesis block (whose shortcut comes first)
        const uint32_t d[5] = {70000, 0, 0, 0, 0};
        uint32_t out[5] = {1, 1, 1, 1, 1};
        expect(!C::difficulty_control(200, 100, d, 0, 3, out) && !(out[0] | out[1] | out[2] | out[3] | out[4]),
               "difficulty_control: zero interval reported");
        expect(C::difficulty_control(200, 100, d, 0, 0, out) && out[0] == 70000, "difficulty_control: genesis parent first");
        C::LinkParams np = {};
        C::LinkHeader parent = {}, child = {};
        parent.height = 3, child.height = 4, child.timestamp = 10;
        expect(C::rules_0d_0g(np, parent, child) == 'e', "rules: a zero interval fails 0.e closed");
    }
    check_field(C::P - 1, C::P - 1);
    check_field(0, C::P - 1);
    check_field(C::P - 1, 1);
    check_shapes();
    check_rule_order();
    std::printf("checks %d failures %d\n", checks, failures);
    return failures ? 1 : 0;
}
