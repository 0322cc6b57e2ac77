// Block digests and the header-chain rules on the device (structs in chain.hpp).
//
//  k_block_proof_leaf  hash_varlen(proof.encode()), the second MAST leaf of Block (block/mod.rs:192-194):
//                      one variable-length sponge per block whose length is the whole block proof (config 4:
//                      ~81,400 words, ~8,140 dependent permutations), for tens to hundreds of blocks.  One
//                      16-lane DPP row per block (lane e holds state[e], tip5_permute_wide).
//  k_block_masts       the header's eight leaves and Merkle tree (block_header.rs:204-215), the kernel MAST
//                      over (header hash, body hash, appendix encoding) (block_kernel.rs:112-119), the block
//                      MAST over (kernel hash, proof leaf), and the PowMastPaths (block/mod.rs:946-962).  One
//                      lane per block, lane-per-state Tip5 as pow_kernels.hip.
//  k_block_links       Block::validate rules 0.a-0.g (block/mod.rs:726-782) in the reference's order, the
//                      first failure the status; then Block::has_proof_of_work (:920-942) into its own byte.
//                      One lane per (parent, child) pair; the integers are chain_rules.hpp's.
#include "chain.hpp"
#include "kernels.hpp"
#include "pow_device.hpp"

namespace nhip {

namespace {

constexpr uint32_t LEAF_WG = 64;  // one wave: four rows, four blocks

// LAT = true, the carry-light arithmetic, as the sponge replay and the row hashing choose for small
// batches: a file's tens to hundreds of blocks make a quarter as many waves, far fewer than the
// device has SIMDs, so every wave has its SIMD to itself and the time is one permutation's dependent chain
// times the number of absorbs.  The carry-light form shortens that chain at the price of more
// instructions, and the issue slots they take are free here.
//
// Four rows share a wave and end at different lengths.  The loop bound is the row's own: a row that is
// done (or has no block) leaves the loop with all its 16 lanes at once, and the row rotations of
// tip5_permute_wide read lanes of the same row only, so the rows still absorbing never read a lane that
// has left.
__global__ void __launch_bounds__(LEAF_WG) k_block_proof_leaf(ChainDev d) {
    __shared__ Tip5Lds t5;
    tip5_lds_init(t5);
    const uint32_t e = threadIdx.x & 15u;
    const uint32_t i = (blockIdx.x * LEAF_WG + threadIdx.x) >> 4;
    if (i >= d.n) return;  // the whole row
    uint64_t rcs[TIP5_ROUNDS];
#pragma unroll
    for (int r = 0; r < TIP5_ROUNDS; ++r) rcs[r] = c_tip5_rc_raw[r * 16 + e];
    const ChainBlockDev& b = d.blk[i];
    // the absorbed sequence: the encoding's prefix words (Genesis, Invalid: the discriminant alone), then
    // the proof's items as k_wire_words gathered them
    const uint64_t* __restrict__ pre = d.words + b.words_off + b.appendix_words;
    const uint64_t* __restrict__ items = d.proof_words + b.proof_off;
    const uint64_t n_pre = b.prefix_words, len = n_pre + b.proof_len;
    const uint64_t nchunks = len / TIP5_RATE + 1;
    auto chunk_word = [&](uint64_t c) -> uint64_t {  // words, then the padding's 1, then 0s
        const uint64_t pos = c * TIP5_RATE + e;
        if (e >= TIP5_RATE || pos > len) return 0ull;
        if (pos == len) return MONT_ONE;
        return to_mont(pos < n_pre ? pre[pos] : items[pos - n_pre]);
    };
    uint64_t s = 0, next = chunk_word(0);
    for (uint64_t c = 0; c < nchunks; ++c) {
        if (e < TIP5_RATE) s = next;  // absorb: the rate is overwritten, the capacity kept
        if (c + 1 < nchunks) next = chunk_word(c + 1);
        s = tip5_permute_wide<true>(s, e, rcs, t5.lut);
    }
    if (e < 5) d.leaf_raw[5ull * i + e] = s;
}

// hash_varlen of `len` canonical words
__device__ void hv_canonical(const uint64_t* w, uint32_t len, uint64_t* out, const uint8_t* __restrict__ lut) {
    varlen_raw([&](uint32_t k) { return to_mont(w[k]); }, len, out, lut);
}
__device__ void hv_u32(const uint32_t* w, uint32_t len, uint64_t* out, const uint8_t* __restrict__ lut) {
    varlen_raw([&](uint32_t k) { return to_mont((uint64_t)w[k]); }, len, out, lut);
}
// hash_varlen of a digest's encoding (its five words)
__device__ void hv_digest_raw(const uint64_t* d_raw, uint64_t* out, const uint8_t* __restrict__ lut) {
    varlen_raw([&](uint32_t k) { return d_raw[k]; }, 5, out, lut);
}

__global__ void __launch_bounds__(64) k_block_masts(ChainDev d) {
    __shared__ Tip5Lds t5;
    tip5_lds_init(t5);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    const uint8_t* lut = t5.lut;
    const ChainBlockDev& b = d.blk[i];
    const uint32_t h = d.tree_height;
    PowMast m;
    uint64_t x[5], y[5], z[5];
    // BlockHeader: leaves 0..7 = version, height, prev_block_digest, timestamp, pow, cumulative_proof_of_work,
    // difficulty, guesser_receiver_data; the pow leaf's path is [leaf 5, node(6,7), node(0..3)]
    hv_canonical(&b.version, 1, x, lut);
    hv_canonical(&b.height, 1, y, lut);
    hp_raw(x, y, z, lut);  // node(0,1)
    hv_canonical(b.prev, 5, x, lut);
    hv_canonical(&b.timestamp, 1, y, lut);
    hp_raw(x, y, x, lut);  // node(2,3)
    hp_raw(z, x, m.pow[2], lut);
    hv_u32(b.difficulty, 5, x, lut);
    varlen_raw([&](uint32_t k) { return to_mont(k < 5 ? b.lock_script[k] : b.receiver[k - 5]); }, 10, y, lut);
    hp_raw(x, y, m.pow[1], lut);
    hv_u32(b.cpow, 6, m.pow[0], lut);
    // pow.encode() = nonce ++ path_b ++ path_a ++ root; the paths also go out in Montgomery form
    const uint64_t* pa = d.paths + 10ull * h * i;
    uint64_t* pr = d.paths_raw + 10ull * h * i;
    for (uint32_t k = 0; k < 10 * h; ++k) pr[k] = to_mont(pa[k]);
    varlen_raw(
        [&](uint32_t k) -> uint64_t {
            if (k < 5) return to_mont(b.nonce[k]);
            k -= 5;
            if (k < 5 * h) return pr[5 * h + k];
            k -= 5 * h;
            if (k < 5 * h) return pr[k];
            return to_mont(b.root[k - 5 * h]);
        },
        10 * h + 10, x, lut);
    hp_raw(x, m.pow[0], y, lut);
    hp_raw(y, m.pow[1], x, lut);
    hp_raw(m.pow[2], x, y, lut);  // the header's MAST hash
    st5(d.header_raw + 5ull * i, y);
    // BlockKernel: leaves header hash, body hash, appendix encoding, padded to four with Digest::default()
    hv_digest_raw(y, x, lut);
    hv_canonical(b.body_hash, 5, m.header[0], lut);
    hv_canonical(d.words + b.words_off, b.appendix_words, y, lut);
    const uint64_t zero[5] = {0, 0, 0, 0, 0};
    hp_raw(y, zero, m.header[1], lut);
    hp_raw(x, m.header[0], y, lut);
    hp_raw(y, m.header[1], x, lut);  // the kernel's MAST hash
    // Block: leaves kernel hash, proof encoding
    hv_digest_raw(x, y, lut);
    ld5(d.leaf_raw + 5ull * i, m.kernel[0]);
    hp_raw(y, m.kernel[0], x, lut);
    st5(d.digest_raw + 5ull * i, x);
    d.mast[i] = m;
}

// Rule 0.c: the parent's block MMR with the parent's digest appended equals the child's.  A single-leaf
// append: while the leaf count has a trailing one bit, pop a peak and hash_pair(peak, acc).
__device__ bool mmr_append_matches(const ChainDev& d, const ChainBlockDev& pb, const ChainBlockDev& cb,
                                   const uint64_t* parent_digest_raw, const uint8_t* __restrict__ lut) {
    const uint64_t nl = pb.mmr_num_leafs;
    const uint32_t np = pb.mmr_n_peaks;
    // fail closed: an inconsistent parent accumulator, or a leaf count that cannot grow
    if (nl == ~0ull || np != (uint32_t)__builtin_popcountll(nl)) return false;
    const uint32_t merges = (uint32_t)__builtin_ctzll(~nl);  // trailing one bits, at most 63
    uint64_t acc[5];
    ld5(parent_digest_raw, acc);
    const uint64_t* pp = d.peaks + 5 * pb.peaks_off;
    for (uint32_t t = 0; t < merges; ++t) {
        uint64_t peak[5];
        for (int q = 0; q < 5; ++q) peak[q] = to_mont(pp[5 * (np - 1 - t) + q]);
        hp_raw(peak, acc, acc, lut);
    }
    const uint32_t kept = np - merges;
    if (cb.mmr_num_leafs != nl + 1 || cb.mmr_n_peaks != kept + 1) return false;
    const uint64_t* cp = d.peaks + 5 * cb.peaks_off;
    bool same = true;
    for (uint32_t k = 0; k < 5 * kept; ++k) same = same && cp[k] == pp[k];
    for (int q = 0; q < 5; ++q) same = same && cp[5 * kept + q] == from_mont(acc[q]);
    return same;
}

__device__ chain::LinkHeader link_header(const ChainBlockDev& b) {
    chain::LinkHeader h;
    h.height = b.height;
    h.timestamp = b.timestamp;
    for (int k = 0; k < 6; ++k) h.cumulative_proof_of_work[k] = b.cpow[k];
    for (int k = 0; k < 5; ++k) h.difficulty[k] = b.difficulty[k];
    return h;
}

__global__ void __launch_bounds__(64) k_block_links(ChainDev d, ChainLinkParams p, const int64_t* __restrict__ parent_of,
                                                    uint8_t* __restrict__ status, uint8_t* __restrict__ pow_ok) {
    __shared__ Tip5Lds t5;
    tip5_lds_init(t5);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    const uint8_t* lut = t5.lut;
    const int64_t par = parent_of[i];
    if (par < 0 || (uint64_t)par >= d.n) {  // the host refused anything but -1 and 0..n-1
        status[i] = NHIP_LINK_SKIPPED;
        pow_ok[i] = 0;
        return;
    }
    const ChainBlockDev& cb = d.blk[i];
    const ChainBlockDev& pb = d.blk[par];
    const chain::LinkHeader ch = link_header(cb), ph = link_header(pb);
    const uint64_t* parent_digest = d.digest_raw + 5ull * (uint64_t)par;
    uint8_t st = NHIP_LINK_OK;
    if (!chain::rule_0a(ph, ch)) {
        st = NHIP_LINK_BLOCK_HEIGHT;
    } else {
        bool prev_ok = true;
        for (int q = 0; q < 5; ++q) prev_ok = prev_ok && from_mont(parent_digest[q]) == cb.prev[q];
        if (!prev_ok) {
            st = NHIP_LINK_PREV_BLOCK_DIGEST;
        } else if (!mmr_append_matches(d, pb, cb, parent_digest, lut)) {
            st = NHIP_LINK_BLOCK_MMR_UPDATE;
        } else {
            const char c = chain::rules_0d_0g(p.np, ph, ch);
            st = c == 'd'   ? NHIP_LINK_MINIMUM_BLOCK_TIME
                 : c == 'e' ? NHIP_LINK_DIFFICULTY
                 : c == 'f' ? NHIP_LINK_CUMULATIVE_POW
                 : c == 'g' ? NHIP_LINK_FUTURE_DATING
                            : NHIP_LINK_OK;
        }
    }
    status[i] = st;

    // has_proof_of_work (block/mod.rs:920-942)
    bool reset = chain::should_reset_difficulty(p.np.difficulty_reset_interval, ch.timestamp, ph.timestamp);
    for (int k = 0; k < 5; ++k) reset = reset && ch.difficulty[k] == p.np.genesis_difficulty[k];
    if (reset) {
        pow_ok[i] = 1;
        return;
    }
    uint64_t target[5];
    if (!chain::difficulty_target(ph.difficulty, target)) {  // a zero difficulty: the reference panics
        pow_ok[i] = 0;
        return;
    }
    for (int q = 0; q < 5; ++q) target[q] = to_mont(target[q]);
    if (p.allows_mock_pow && digest_le(d.digest_raw + 5ull * i, target)) {  // is_valid_mock_pow
        pow_ok[i] = 1;
        return;
    }
    // pow_verify (:1013-1024): Pow::validate with the block's own MAST paths, the rule set of the height
    // after the parent's, and the child's prev_block_digest as the parent digest
    const bool reboot = chain::height_next(ph.height) < p.hardfork_alpha_height;
    const PowMast& m = d.mast[i];
    uint64_t commit[5], root[5], nonce[5], prev[5];
    varlen_raw(
        [&](uint32_t k) -> uint64_t {  // PowMastPaths::commit (pow.rs:209-217): pow, header, kernel
            return k < 15 ? m.pow[k / 5][k % 5] : k < 25 ? m.header[(k - 15) / 5][k % 5] : m.kernel[0][k - 25];
        },
        30, commit, lut);
    for (int q = 0; q < 5; ++q) {
        root[q] = to_mont(cb.root[q]);
        nonce[q] = to_mont(cb.nonce[q]);
        prev[q] = to_mont(cb.prev[q]);
    }
    const uint32_t h = d.tree_height;
    const uint64_t* pr = d.paths_raw + 10ull * h * i;
    pow_ok[i] = pow_validate_lane(root, nonce, commit, prev, target, m, reboot, [=](uint32_t j) { return pr + 5 * j; },
                                  [=](uint32_t j) { return pr + 5 * (h + j); }, h, lut)
                    ? 1
                    : 0;
}

unsigned blocks_for(uint64_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

}  // namespace

hipError_t launch_block_proof_leaf(const ChainDev& d, hipStream_t st) {
    if (d.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_block_proof_leaf, dim3(blocks_for(16ull * d.n, LEAF_WG)), dim3(LEAF_WG), 0, st, d);
    return hipGetLastError();
}

hipError_t launch_block_masts(const ChainDev& d, hipStream_t st) {
    if (d.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_block_masts, dim3(blocks_for(d.n, 64)), dim3(64), 0, st, d);
    return hipGetLastError();
}

hipError_t launch_block_links(const ChainDev& d, const ChainLinkParams& p, const int64_t* d_parent_of, uint8_t* d_status,
                              uint8_t* d_pow_ok, hipStream_t st) {
    if (d.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_block_links, dim3(blocks_for(d.n, 64)), dim3(64), 0, st, d, p, d_parent_of, d_status, d_pow_ok);
    return hipGetLastError();
}

}  // namespace nhip
