// Host-side check of the pieces xfe.hpp gives the FRI, DEEP and OOD kernels beside the field
// arithmetic (run by tests/test_aux_chain_host.py, plain and under ASan + UBSan):
//  1. the two-adic root tables against b_pow / b_inv, root[k]^2 == root[k - 1], root[k] * inv[k] == 1;
//  2. 7^-1 * g^((N - i) mod N) == b_inv(7 * g^i) for log2_N = 5..32, with the tables filled as the
//     kernel fills them (sq[q] = the root of order 2^(log2_N - q)) and lds_pow's e < 2^32;
//  3. bary_slot's several-points-per-lane chain against the sum with one inversion per point, laid
//     over workgroups of 256 and 1,024 threads as the kernel lays it, for every points-per-lane
//     choice, and its zero flag for t on the domain (first lane, last lane, chain boundaries).
#include "xfe.hpp"
#include <cstdio>
#include <random>
#include <vector>
using namespace nhip;

static uint64_t bad = 0, n_checked = 0;
static void expect(bool ok, const char* what, uint64_t a = 0, uint64_t b = 0) {
    ++n_checked;
    if (!ok) {
        if (bad < 10) printf("FAIL %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
        ++bad;
    }
}

static void check_tables() {
    const uint64_t seven = to_mont(7);
    for (uint32_t k = 0; k <= 32; ++k) {
        const uint64_t r = b_pow(seven, (GL_P - 1) >> k);
        expect(root_of_unity(k) == r, "root table entry", k);
        expect(root_of_unity_inv(k) == b_inv(r), "inverse table entry", k);
        expect(mont_mul(root_of_unity(k), root_of_unity_inv(k)) == MONT_ONE_W, "root * inverse", k);
        if (k) expect(mont_mul(root_of_unity(k), root_of_unity(k)) == root_of_unity(k - 1), "root squared", k);
    }
    expect(root_of_unity(0) == MONT_ONE_W, "root of order 1");
    expect(SEVEN_INV == b_inv(seven), "SEVEN_INV");
    expect(mont_mul(SEVEN_INV, seven) == MONT_ONE_W, "7 * SEVEN_INV");
}

static void check_fri_inverse(std::mt19937_64& g) {
    const uint64_t seven = to_mont(7);
    for (uint32_t log2_N = 5; log2_N <= 32; ++log2_N) {
        uint64_t sq[33] = {};
        for (uint32_t q = 0; q < log2_N; ++q) sq[q] = root_of_unity(log2_N - q);
        const uint64_t N = 1ull << log2_N;
        std::vector<uint64_t> is = {0, 1, N / 2, N - 1};
        for (int r = 0; r < 40; ++r) is.push_back(g() & (N - 1));
        for (uint64_t i : is) {
            const uint64_t e = neg_mod_pow2((uint32_t)i, log2_N);
            expect(e < (1ull << 32) && e == ((N - i) & (N - 1)), "exponent of the inverse", log2_N, i);
            const uint64_t x = mont_mul(seven, lds_pow(sq, i));
            expect(mont_mul(SEVEN_INV, lds_pow(sq, e)) == b_inv(x), "7^-1 g^(N - i)", log2_N, i);
        }
    }
}

static Xfe rnd_xfe(std::mt19937_64& g) { return {g() % GL_P, g() % GL_P, g() % GL_P}; }

// the kernel's layout: thread tid of `width` takes slots width - 1 - tid, 2 width - 1 - tid, ...
static bool bary_block(Xfe t, const std::vector<Xfe>& cw, uint32_t L, uint32_t width, uint32_t ppl, Xfe& num, Xfe& den) {
    uint32_t log2L = 0;
    while ((1u << log2L) < L) ++log2L;
    uint64_t wsq[33] = {};
    for (uint32_t q = 0; q < log2L; ++q) wsq[q] = root_of_unity(log2L - q);
    const uint32_t S = (L + ppl - 1) / ppl;
    uint32_t log2p = 0;
    while ((1u << log2p) < ppl) ++log2p;
    const uint64_t wS = root_of_unity(log2p);
    bool zero = false;
    num = den = x_zero();
    for (uint32_t tid = 0; tid < width; ++tid)
        for (uint32_t s = width - 1 - tid; s < S; s += width)
            zero |= bary_slot(t, lds_pow(wsq, s), wS, s, S, L, ppl, [&](uint32_t i) { return cw.at(i); }, num, den);
    return zero;
}

static void check_barycentric(std::mt19937_64& g) {
    const uint32_t Ls[] = {1, 2, 64, 128, 256, 512, 1024};
    expect(bary_points_per_lane(1) == 1 && bary_points_per_lane(2) == 1 && bary_points_per_lane(64) == 1 &&
               bary_points_per_lane(128) == 2 && bary_points_per_lane(256) == 4 && bary_points_per_lane(512) == 8 &&
               bary_points_per_lane(1024) == 8 && bary_points_per_lane(1u << 31) == 8,
           "points per lane");
    for (uint32_t L : Ls) {
        uint32_t log2L = 0;
        while ((1u << log2L) < L) ++log2L;
        const uint64_t w = root_of_unity(log2L);
        std::vector<Xfe> cw(L);
        for (auto& v : cw) v = rnd_xfe(g);
        // every choice the helper takes (the kernel's own, bary_points_per_lane(L), is one of them)
        for (uint32_t ppl = 1; ppl <= BARY_PPL_MAX && ppl <= L; ppl *= 2) {
            const uint32_t S = L / ppl;
            for (uint32_t width : {256u, 1024u}) {
                const Xfe t = rnd_xfe(g);
                Xfe rnum = x_zero(), rden = x_zero();  // one inversion per point
                uint64_t wi = MONT_ONE_W;
                for (uint32_t i = 0; i < L; ++i, wi = mont_mul(wi, w)) {
                    const Xfe q = x_scale(x_inv(x_sub(t, x_lift(wi))), wi);
                    rnum = x_add(rnum, x_mul(q, cw[i]));
                    rden = x_add(rden, q);
                }
                Xfe num, den;
                const bool z = bary_block(t, cw, L, width, ppl, num, den);
                expect(!z, "no flag off the domain", L, ppl);
                expect(x_eq(num, rnum) && x_eq(den, rden), "barycentric sums", L, ppl);
                // t = w^i: first lane, last lane, the chain boundaries of both, the last point
                const uint32_t on[] = {0, S - 1, S % L, (2 * S - 1) % L, L - S, L - 1, (uint32_t)(g() % L)};
                for (uint32_t i : on) {
                    const Xfe ti = x_lift(b_pow(w, i));
                    expect(bary_block(ti, cw, L, width, ppl, num, den), "flag on the domain", L, i);
                }
            }
        }
    }
}

int main() {
    std::mt19937_64 g(11);
    check_tables();
    check_fri_inverse(g);
    check_barycentric(g);
    printf("checked %llu, bad %llu\n", (unsigned long long)n_checked, (unsigned long long)bad);
    return bad != 0;
}
