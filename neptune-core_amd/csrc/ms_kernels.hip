// Mutator-set checks: thousands of independent short Tip5 chains, the shape of
// k_mtree_verify, plus a small hash-free decision kernel.
//
//  k_mmr_verify    : twenty-first MmrMembershipProof::verify(leaf_index, leaf, peaks, num_leafs),
//                    one lane per (leaf, path) item.  The crate is not in the reference tree; the
//                    restatement (mmr_climb below) rests on the path shape that
//                    neptune-core/src/util_types/archival_mmr.rs:250-281 (auth_path_node_indices)
//                    fixes: leaf sibling first, one digest per level of the leaf's peak.
//  k_ms_aocl_leaf  : MutatorSetAccumulator::verify's AOCL leg (mutator_set_accumulator.rs:257-278):
//                    leaf = hash_pair(hash_pair(item, sender_randomness), hash_pair(receiver_preimage,
//                    0^5)), member of the AOCL at aocl_leaf_index.  One lane per item.
//  k_ms_chunk_auth : one lane per chunk-dictionary entry (chunk_index, MMR path, Chunk) of an MsChunksDev:
//                    Tip5::hash(chunk) = hash_varlen of its BFieldCodec encoding, then the MMR climb
//                    against swbf_inactive at leaf index chunk_index (ms_chunk_auth_entry, ms_device.hpp,
//                    shared with k_ms_chunk_auth_jobs).  One byte per entry.
//  k_ms_records    : one wave per record (a lane per index), no Tip5: the 45 absolute indices, the entry bytes and the
//                    active window -> validate / can_remove (removal_record.rs:202-251,
//                    mutator_set_accumulator.rs:187-222) or verify (mutator_set_accumulator.rs:280-338).
//
// Chunk { relative_indices: Vec<u32> } is a derived BFieldCodec struct with one dynamically sized
// field: [n + 1, n, idx_0 .. idx_{n-1}] (the field's length prefix, then the Vec's own length), the
// rule that gives Claim its layout (neptune-core/src/tasm/claims/new_claim.rs).  The words are
// absorbed straight from the u32 list.
#include "ms_device.hpp"

namespace nhip {

__global__ void __launch_bounds__(256) k_mmr_verify(MmrDev mmr, const uint64_t* __restrict__ leaf_index,
                                                    const uint64_t* __restrict__ leaves,
                                                    const uint64_t* __restrict__ path_off,
                                                    const uint64_t* __restrict__ path, size_t n,
                                                    uint8_t* __restrict__ verdicts) {
    __shared__ Tip5Lds t5;
    tip5_lds_init(t5);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        uint64_t run[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) run[k] = to_mont(leaves[5 * i + k]);
        const uint64_t beg = path_off[i];
        verdicts[i] = mmr_climb(run, leaf_index[i], mmr, path + 5 * beg, path_off[i + 1] - beg, t5.lut) ? 1 : 0;
    }
}

// digests: n x 15 canonical words (item, sender_randomness, receiver_preimage), as k_absolute_index_sets takes them
__global__ void __launch_bounds__(256) k_ms_aocl_leaf(MmrDev aocl, const uint64_t* __restrict__ digests,
                                                      const uint64_t* __restrict__ leaf_index,
                                                      const uint64_t* __restrict__ path_off,
                                                      const uint64_t* __restrict__ path, size_t n,
                                                      uint8_t* __restrict__ member) {
    __shared__ Tip5Lds t5;
    tip5_lds_init(t5);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        uint64_t s[16], commitment[5], run[5];
#pragma unroll
        for (int k = 0; k < 10; ++k) s[k] = to_mont(digests[15 * i + k]);
        tip5_hash_pair_digest(s, t5.lut);  // hash_pair(item, sender_randomness)
#pragma unroll
        for (int k = 0; k < 5; ++k) commitment[k] = s[k];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            s[k] = to_mont(digests[15 * i + 10 + k]);
            s[5 + k] = 0;
        }
        tip5_hash_pair_digest(s, t5.lut);  // hash_pair(receiver_preimage, 0^5)
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            s[5 + k] = s[k];
            s[k] = commitment[k];
        }
        tip5_hash_pair_digest(s, t5.lut);
#pragma unroll
        for (int k = 0; k < 5; ++k) run[k] = s[k];
        const uint64_t beg = path_off[i];
        member[i] = mmr_climb(run, leaf_index[i], aocl, path + 5 * beg, path_off[i + 1] - beg, t5.lut) ? 1 : 0;
    }
}

__global__ void __launch_bounds__(256) k_ms_chunk_auth(MmrDev swbf, MsChunksDev ch, size_t entries,
                                                       uint8_t* __restrict__ auth) {
    __shared__ Tip5Lds t5;
    tip5_lds_init(t5);
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < entries; e += (size_t)gridDim.x * blockDim.x)
        auth[e] = ms_chunk_auth_entry(ch, e, swbf, t5.lut) ? 1 : 0;
}

// One 64-lane wave per record: lane t < 45 takes index t, and the lanes share the record's entries in the
// validate pass; the flags are ORed over the wave (ms_record_decide).  (One lane per record left 45 x entries
// dependent loads in a row on a grid of a few dozen waves: the launch then took as long at 512 records as at 4,096.)
__global__ void __launch_bounds__(256) k_ms_records(MsRecordsDev r, size_t n) {
    const uint32_t lane = threadIdx.x & 63u;
    const size_t wave = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6;
    const size_t n_waves = ((size_t)gridDim.x * blockDim.x) >> 6;
    for (size_t i = wave; i < n; i += n_waves)  // wave-uniform
        ms_record_decide(r, i, lane, r.active, r.n_active, r.aocl_num_leafs, nullptr);
}

hipError_t launch_mmr_verify(const MmrDev& mmr, const uint64_t* d_leaf_index, const uint64_t* d_leaves,
                             const uint64_t* d_path_off, const uint64_t* d_path, size_t n, uint8_t* d_verdicts,
                             hipStream_t st) {
    return ms_launch(k_mmr_verify, n, st, mmr, d_leaf_index, d_leaves, d_path_off, d_path, n, d_verdicts);
}

hipError_t launch_ms_aocl_leaf(const MmrDev& aocl, const uint64_t* d_digests, const uint64_t* d_leaf_index,
                               const uint64_t* d_path_off, const uint64_t* d_path, size_t n, uint8_t* d_member,
                               hipStream_t st) {
    return ms_launch(k_ms_aocl_leaf, n, st, aocl, d_digests, d_leaf_index, d_path_off, d_path, n, d_member);
}

hipError_t launch_ms_chunk_auth(const MmrDev& swbf, const MsChunksDev& ch, size_t entries, uint8_t* d_auth, hipStream_t st) {
    return ms_launch(k_ms_chunk_auth, entries, st, swbf, ch, entries, d_auth);
}

hipError_t launch_ms_records(const MsRecordsDev& r, size_t n, hipStream_t st) {
    return ms_launch(k_ms_records, 64 * n, st, r, n);  // a wave per record
}

}  // namespace nhip
