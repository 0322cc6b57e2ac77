// Proof-of-work Tip5 workloads, neptune-core/src/protocol/consensus/block/pow.rs:
//
//  guesser buffer  Pow::preprocess (:365-469) for MERKLE_TREE_HEIGHT h: 2^h buds
//                  bud(prefix, i) = hash_pair(prefix, [i, 0, 0, 0, 0]) (:321-323), NUM_BUD_LAYERS = 5
//                  sliding layers leaf[k] = hash_pair(bud[k], bud[(k + 2^i) mod 2^h]) (:427-435) so
//                  leaf k = the MTree root of buds k..k+31 (Pow::leaf, :325-331), the HardforkAlpha
//                  bit-reversal swap of the leaves (:451-458, bitreverse :349-356), then
//                  MTree::build_inplace (:66-119).  7 * 2^h permutations; h = 29 -> 3.8e9.
//  guess           Pow::guess (:471-507): indices (:333-343, NUM_INDEX_REPETITIONS = 63 chained
//                  hash_pairs), the two authentication paths (MTree::path, :151-160) read from the
//                  buffer, PowMastPaths::fast_mast_hash (:219-241) of the Pow, compared with the
//                  target.  One lane per nonce.
//  validate        Pow::validate (:509-557): index picker, both leaves rebuilt from buds (63
//                  permutations each), both MTree::verify climbs, fast_mast_hash, threshold.  One
//                  lane per block.
// Buffers hold raw Montgomery digests (5 u64); the C ABI converts at the boundary.
#include "kernels.hpp"
#include "pow_device.hpp"

namespace nhip {

__global__ void __launch_bounds__(256) k_pow_buds(PowPrefix prefix, uint64_t n, uint64_t* __restrict__ out) {
    __shared__ Tip5Lds t5;
    tip5_lds_init(t5);
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t d[5];
    bud_raw(prefix.d, i, d, t5.lut);
    st5(out + 5 * i, d);
}

__global__ void __launch_bounds__(256) k_pow_layer(const uint64_t* __restrict__ in, uint64_t* __restrict__ out,
                                                   uint64_t n, uint64_t shift) {
    __shared__ Tip5Lds t5;
    tip5_lds_init(t5);
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    uint64_t a[5], b[5], d[5];
    ld5(in + 5 * k, a);
    ld5(in + 5 * ((k + shift) & (n - 1)), b);
    hp_raw(a, b, d, t5.lut);
    st5(out + 5 * k, d);
}

// leafs.swap(k, rev_k) for k < rev_k (disjoint pairs: one lane per pair owner)
__global__ void k_pow_bitrev_swap(uint64_t* __restrict__ leafs, uint64_t n, uint32_t log2_n) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint64_t r = bitreverse((uint32_t)k, log2_n);
    if (k >= r) return;
    uint64_t a[5], b[5];
    ld5(leafs + 5 * k, a);
    ld5(leafs + 5 * r, b);
    st5(leafs + 5 * k, b);
    st5(leafs + 5 * r, a);
}

// parents [p0, 2 p0) of the MTree from children (leaves: node n + k lives at leafs[k])
__global__ void __launch_bounds__(256) k_pow_tree_level(const uint64_t* __restrict__ children, uint64_t* __restrict__ nodes,
                                                        uint64_t p0) {
    __shared__ Tip5Lds t5;
    tip5_lds_init(t5);
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p0) return;
    uint64_t a[5], b[5], d[5];
    ld5(children + 10 * i, a);
    ld5(children + 10 * i + 5, b);
    hp_raw(a, b, d, t5.lut);
    st5(nodes + 5 * (p0 + i), d);
}

__global__ void __launch_bounds__(256) k_pow_guess(const uint64_t* __restrict__ leafs, const uint64_t* __restrict__ nodes,
                                                   uint32_t h, PowMast mast, PowPrefix picker,
                                                   const uint64_t* __restrict__ nonces, uint64_t n, PowPrefix target,
                                                   uint64_t* __restrict__ out_digest, uint64_t* __restrict__ out_idx,
                                                   uint8_t* __restrict__ out_ok) {
    __shared__ Tip5Lds t5;
    tip5_lds_init(t5);
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t nonce[5];
    ld5(nonces + 5 * i, nonce);
    uint64_t ia, ib;
    pow_indices(picker.d, nonce, h, ia, ib, t5.lut);
    const uint64_t N = 1ull << h;
    // MTree::path(index)[j]: j == 0 -> leafs[index ^ 1]; else internal[((index + N) >> j) ^ 1]
    auto path_of = [&](uint64_t index) {
        return [=](uint32_t j) -> const uint64_t* {
            return j == 0 ? leafs + 5 * (index ^ 1) : nodes + 5 * (((index + N) >> j) ^ 1);
        };
    };
    uint64_t d[5];
    fast_mast_hash(mast, nodes + 5, path_of(ia), path_of(ib), nonce, h, d, t5.lut);
    st5(out_digest + 5 * i, d);
    out_idx[2 * i] = ia;
    out_idx[2 * i + 1] = ib;
    out_ok[i] = digest_le(d, target.d) ? 1 : 0;
}

__global__ void __launch_bounds__(64) k_pow_validate(const PowBlock* __restrict__ blocks, uint64_t n, uint32_t h,
                                                     uint8_t* __restrict__ verdicts) {
    __shared__ Tip5Lds t5;
    tip5_lds_init(t5);
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PowBlock& b = blocks[i];
    verdicts[i] = pow_validate_lane(b.root, b.nonce, b.commit, b.parent, b.target, b.mast, b.reboot != 0,
                                    [&](uint32_t j) { return b.path_a + 5 * j; },
                                    [&](uint32_t j) { return b.path_b + 5 * j; }, h, t5.lut)
                      ? 1
                      : 0;
}

// ---------------------------------------------------------------- launchers
static unsigned blocks_for(uint64_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

hipError_t launch_pow_preprocess(const PowPrefix& prefix, uint32_t h, bool bitrev_swap, uint64_t* d_a, uint64_t* d_b,
                                 uint64_t** leafs_out, uint64_t** nodes_out, hipStream_t st) {
    const uint64_t N = 1ull << h;
    hipLaunchKernelGGL(k_pow_buds, dim3(blocks_for(N, 256)), dim3(256), 0, st, prefix, N, d_a);
    uint64_t *in = d_a, *out = d_b;
    for (uint32_t i = 0; i < POW_NUM_BUD_LAYERS; ++i) {
        hipLaunchKernelGGL(k_pow_layer, dim3(blocks_for(N, 256)), dim3(256), 0, st, in, out, N, 1ull << i);
        uint64_t* t = in;
        in = out;
        out = t;
    }
    uint64_t* leafs = in;   // after the last layer
    uint64_t* nodes = out;  // the other buffer holds the internal nodes
    if (bitrev_swap)
        hipLaunchKernelGGL(k_pow_bitrev_swap, dim3(blocks_for(N, 256)), dim3(256), 0, st, leafs, N, h);
    for (uint64_t p0 = N >> 1; p0 >= 1; p0 >>= 1) {
        const uint64_t* children = p0 == (N >> 1) ? leafs : nodes + 5 * (2 * p0);
        hipLaunchKernelGGL(k_pow_tree_level, dim3(blocks_for(p0, 256)), dim3(256), 0, st, children, nodes, p0);
    }
    *leafs_out = leafs;
    *nodes_out = nodes;
    return hipGetLastError();
}

hipError_t launch_pow_guess(const uint64_t* leafs, const uint64_t* nodes, uint32_t h, const PowMast& mast,
                            const PowPrefix& picker, const uint64_t* d_nonces, uint64_t n, const PowPrefix& target,
                            uint64_t* d_digest, uint64_t* d_idx, uint8_t* d_ok, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pow_guess, dim3(blocks_for(n, 256)), dim3(256), 0, st, leafs, nodes, h, mast, picker, d_nonces,
                       n, target, d_digest, d_idx, d_ok);
    return hipGetLastError();
}

hipError_t launch_pow_validate(const PowBlock* d_blocks, uint64_t n, uint32_t h, uint8_t* d_verdicts, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pow_validate, dim3(blocks_for(n, 64)), dim3(64), 0, st, d_blocks, n, h, d_verdicts);
    return hipGetLastError();
}

}  // namespace nhip
