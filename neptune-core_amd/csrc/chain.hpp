// Block digests and the header-chain rules: what chain_capi.hip stages and
// chain_kernels.hip reads.  Canonical words unless a name says raw (Montgomery).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chain_rules.hpp"
#include "pow.hpp"

namespace nhip {

// One scanned block (nhip_blk_header's fields and where its variable parts lie in the call's pools)
struct ChainBlockDev {
    uint64_t version, height, timestamp;
    uint64_t prev[5], root[5], nonce[5], receiver[5], lock_script[5], body_hash[5];
    uint32_t cpow[6], difficulty[5], mmr_n_peaks;  // mmr_n_peaks as serialized, saturated at 65
    uint64_t mmr_num_leafs;
    uint64_t peaks_off;                     // digests: min(mmr_n_peaks, 64) peaks in the peaks pool
    uint64_t words_off;                     // words pool: the appendix encoding, then the proof encoding's prefix
    uint32_t appendix_words, prefix_words;
    uint64_t proof_off, proof_len;          // the proof's items in the gathered proof-word buffer
};

struct ChainLinkParams {
    chain::LinkParams np;
    uint64_t hardfork_alpha_height;
    uint32_t tree_height, allows_mock_pow;
};

// Everything the three kernels share; every pointer a device pointer
struct ChainDev {
    const ChainBlockDev* blk;
    const uint64_t* words;        // the words pool
    const uint64_t* proof_words;  // k_wire_words' output: every proof's items back to back
    const uint64_t* paths;        // per block: path_a then path_b, tree_height digests each
    const uint64_t* peaks;        // the peaks pool
    uint32_t n, tree_height;
    uint64_t* leaf_raw;           // per block: hash_varlen(proof.encode())
    uint64_t* digest_raw;         // per block: Block::hash
    uint64_t* header_raw;         // per block: the header's MAST hash
    uint64_t* paths_raw;          // `paths` in Montgomery form (k_block_masts writes, k_block_links reads)
    PowMast* mast;                // per block: PowMastPaths, raw
};

hipError_t launch_block_proof_leaf(const ChainDev& d, hipStream_t st);
hipError_t launch_block_masts(const ChainDev& d, hipStream_t st);
hipError_t launch_block_links(const ChainDev& d, const ChainLinkParams& p, const int64_t* d_parent_of, uint8_t* d_status,
                              uint8_t* d_pow_ok, hipStream_t st);

}  // namespace nhip
