// Per-lane device code of the proof-of-work workloads (pow.rs citations in pow_kernels.hip), shared by
// pow_kernels.hip (k_pow_guess, k_pow_validate) and chain_kernels.hip (k_block_masts, k_block_links).
// Raw Montgomery digests throughout.
#pragma once
#include "pow.hpp"
#include "tip5_device.hpp"

namespace nhip {

__device__ __forceinline__ void hp_raw(const uint64_t* l, const uint64_t* r, uint64_t* out,
                                       const uint8_t* __restrict__ lut) {
    uint64_t s[16];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        s[q] = l[q];
        s[5 + q] = r[q];
    }
    tip5_hash_pair_digest(s, lut);  // capacity 1: FixedLength domain
#pragma unroll
    for (int q = 0; q < 5; ++q) out[q] = s[q];
}

__device__ __forceinline__ void ld5(const uint64_t* __restrict__ p, uint64_t* d) {
#pragma unroll
    for (int q = 0; q < 5; ++q) d[q] = p[q];
}
__device__ __forceinline__ void st5(uint64_t* __restrict__ p, const uint64_t* d) {
#pragma unroll
    for (int q = 0; q < 5; ++q) p[q] = d[q];
}

__device__ __forceinline__ void bud_raw(const uint64_t* prefix, uint64_t index, uint64_t* out,
                                        const uint8_t* __restrict__ lut) {
    const uint64_t idx[5] = {to_mont(index), 0, 0, 0, 0};
    hp_raw(prefix, idx, out, lut);
}

__device__ __forceinline__ uint32_t bitreverse(uint32_t k, uint32_t log2_n) {
    return log2_n ? (__brev(k) >> (32u - log2_n)) : 0u;
}

// ---------------------------------------------------------------- shared per-lane helpers
// Pow::indices (:333-343): indexer = hash_pair(hash, nonce), 62 x hash_pair(indexer, default)
__device__ inline void pow_indices(const uint64_t* picker, const uint64_t* nonce, uint32_t h, uint64_t& ia, uint64_t& ib,
                            const uint8_t* __restrict__ lut) {
    uint64_t x[5];
    hp_raw(picker, nonce, x, lut);
    const uint64_t zero[5] = {0, 0, 0, 0, 0};
    for (int r = 1; r < POW_NUM_INDEX_REPETITIONS; ++r) hp_raw(x, zero, x, lut);
    const uint64_t mask = (h >= 64) ? ~0ull : ((1ull << h) - 1);
    ia = from_mont(x[0]) & mask;
    ib = from_mont(x[1]) & mask;
}

// Tip5::hash_varlen of `len` raw words produced by `get(i)` (VariableLength sponge)
template <class F>
__device__ void varlen_raw(F get, uint32_t len, uint64_t* out, const uint8_t* __restrict__ lut) {
    uint64_t s[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) s[q] = 0;
    uint32_t pos = 0;
    for (; pos + TIP5_RATE <= len; pos += TIP5_RATE) {
        for (int q = 0; q < TIP5_RATE; ++q) s[q] = get(pos + q);
        tip5_permute_raw(s, lut);
    }
    const uint32_t rem = len - pos;
    for (uint32_t q = 0; q < TIP5_RATE; ++q) s[q] = q < rem ? get(pos + q) : (q == rem ? MONT_ONE : 0ull);
    tip5_permute_raw(s, lut);
#pragma unroll
    for (int q = 0; q < 5; ++q) out[q] = s[q];
}

// PowMastPaths::fast_mast_hash (:219-241).  pow.encode() = nonce ++ path_b ++ path_a ++ root
// (BFieldCodec: derived struct fields in reverse order, static-size fields without prefix).
template <class PathA, class PathB>
__device__ void fast_mast_hash(const PowMast& m, const uint64_t* root, PathA pa, PathB pb, const uint64_t* nonce,
                               uint32_t h, uint64_t* out, const uint8_t* __restrict__ lut) {
    const uint32_t len = 10 * h + 10;
    auto get = [&](uint32_t i) -> uint64_t {
        if (i < 5) return nonce[i];
        i -= 5;
        if (i < 5 * h) return pb(i / 5)[i % 5];
        i -= 5 * h;
        if (i < 5 * h) return pa(i / 5)[i % 5];
        return root[i - 5 * h];
    };
    uint64_t x[5], y[5];
    varlen_raw(get, len, x, lut);
    hp_raw(x, m.pow[0], y, lut);
    hp_raw(y, m.pow[1], x, lut);
    hp_raw(m.pow[2], x, y, lut);  // header mast hash
    varlen_raw([&](uint32_t i) { return y[i]; }, 5, x, lut);
    hp_raw(x, m.header[0], y, lut);
    hp_raw(y, m.header[1], x, lut);  // kernel mast hash
    varlen_raw([&](uint32_t i) { return x[i]; }, 5, y, lut);
    hp_raw(y, m.kernel[0], out, lut);
}

// twenty-first Digest ordering (unpinned): canonical values compared from the last
// element down.  Returns a <= b.
__device__ __forceinline__ bool digest_le(const uint64_t* a_raw, const uint64_t* b_raw) {
    for (int q = 4; q >= 0; --q) {
        const uint64_t a = from_mont(a_raw[q]), b = from_mont(b_raw[q]);
        if (a != b) return a < b;
    }
    return true;
}

// Pow::leaf (:325-331): MTree root of buds index..index+31 (mod 2^h)
__device__ inline void pow_leaf(const uint64_t* prefix, uint64_t index, uint32_t h, uint64_t* out,
                         const uint8_t* __restrict__ lut) {
    // iterative bottom-up merge with a stack of 5 subtree roots (binary counter)
    uint64_t stack[POW_NUM_BUD_LAYERS + 1][5];
    const uint64_t mask = (1ull << h) - 1;
    for (uint32_t j = 0; j < POW_BUDS_PER_LEAF; ++j) {
        uint64_t cur[5];
        bud_raw(prefix, (index + j) & mask, cur, lut);
        uint32_t lvl = 0;
        for (uint32_t t = j; t & 1u; t >>= 1, ++lvl) hp_raw(stack[lvl], cur, cur, lut);
        st5(stack[lvl], cur);
    }
    st5(out, stack[POW_NUM_BUD_LAYERS]);
}

// Pow::validate (:509-557) on one lane: the index picker, both leaves rebuilt from buds, both MTree::verify
// climbs (:162-180; index <= 2^h always holds here), fast_mast_hash, threshold.  pa(j) / pb(j): sibling j of
// path_a / path_b.
template <class PathA, class PathB>
__device__ bool pow_validate_lane(const uint64_t* root, const uint64_t* nonce, const uint64_t* commit,
                                  const uint64_t* parent, const uint64_t* target, const PowMast& mast, bool reboot,
                                  PathA pa, PathB pb, uint32_t h, const uint8_t* __restrict__ lut) {
    uint64_t picker[5];
    hp_raw(root, commit, picker, lut);  // index_picker_preimage = hash_pair(root, commit)
    uint64_t ia, ib;
    pow_indices(picker, nonce, h, ia, ib, lut);
    const uint64_t* prefix = reboot ? commit : parent;
    uint64_t leaf_a[5], leaf_b[5];
    pow_leaf(prefix, reboot ? ia : bitreverse((uint32_t)ia, h), h, leaf_a, lut);
    pow_leaf(prefix, reboot ? ib : bitreverse((uint32_t)ib, h), h, leaf_b, lut);
    uint8_t ok = 1;
    for (int w = 0; w < 2; ++w) {
        uint64_t run[5];
        st5(run, w == 0 ? leaf_a : leaf_b);
        uint64_t ri = w == 0 ? ia : ib;
        for (uint32_t j = 0; j < h; ++j) {
            const uint64_t* sib = w == 0 ? pa(j) : pb(j);
            if (ri & 1) hp_raw(sib, run, run, lut);
            else hp_raw(run, sib, run, lut);
            ri >>= 1;
        }
        for (int q = 0; q < 5; ++q) ok &= run[q] == root[q];
    }
    uint64_t d[5];
    fast_mast_hash(mast, root, pa, pb, nonce, h, d, lut);
    if (!digest_le(d, target)) ok = 0;
    return ok != 0;
}

}  // namespace nhip
