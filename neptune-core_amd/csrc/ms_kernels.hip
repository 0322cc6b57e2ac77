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
//  k_ms_chunk_auth : one lane per chunk-dictionary entry (chunk_index, MMR path, Chunk):
//                    Tip5::hash(chunk) = hash_varlen of its BFieldCodec encoding, then the MMR climb
//                    against swbf_inactive at leaf index chunk_index (removal_record.rs:237-243,
//                    mutator_set_accumulator.rs:309-316).  One byte per entry.
//  k_ms_records    : one wave per record (a lane per index), no Tip5: the 45 absolute indices, the entry bytes and the
//                    active window -> validate / can_remove (removal_record.rs:202-251,
//                    mutator_set_accumulator.rs:187-222) or verify (mutator_set_accumulator.rs:280-338).
//
// Chunk { relative_indices: Vec<u32> } is a derived BFieldCodec struct with one dynamically sized
// field: [n + 1, n, idx_0 .. idx_{n-1}] (the field's length prefix, then the Vec's own length), the
// rule that gives Claim its layout (neptune-core/src/tasm/claims/new_claim.rs).  The words are
// absorbed straight from the u32 list.
#include "../../include/neptune_hip.h"
#include "kernels.hpp"
#include "tip5_device.hpp"

namespace nhip {

static constexpr uint32_t MSK_CHUNK_BITS = 12;                     // CHUNK_SIZE = 2^12 (shared.rs:13)
static constexpr uint32_t MSK_BATCH_SIZE = 8;                      // BATCH_SIZE (shared.rs:14)
static constexpr uint32_t MSK_WINDOW_CHUNKS = 1u << (20 - 12);     // WINDOW_SIZE / CHUNK_SIZE
static constexpr uint32_t MSK_NUM_TRIALS = 45;                     // NUM_TRIALS (shared.rs:15)

// MmrMembershipProof::verify.  run: the leaf (raw Montgomery), replaced by the fold.  With
// d = leaf_index ^ num_leafs, the highest set bit h of d is the height of the leaf's peak: above
// it the two agree, at it num_leafs has the 1.  The leaf's Merkle-tree index inside that peak is
// (leaf_index mod 2^h) + 2^h, and the peak is the one after those of the set bits of num_leafs
// above h (peaks: tallest first).  h is in 0..63, so 1 << h and the mask are exact; with h = 0 the
// path is empty and the leaf is the peak.  Reads path[0 .. 5 h) and peaks[5 peak ..] only after
// path_len == h and peak < n_peaks.
__device__ __forceinline__ bool mmr_climb(uint64_t run[5], uint64_t leaf_index, const MmrDev& mmr,
                                          const uint64_t* __restrict__ path, uint64_t path_len,
                                          const uint8_t* __restrict__ lut) {
    if (leaf_index >= mmr.num_leafs) return false;
    const uint64_t d = leaf_index ^ mmr.num_leafs;  // != 0
    const uint32_t h = 63u - (uint32_t)__clzll((long long)d);
    const uint64_t top = 1ull << h, mask = top - 1;
    uint64_t mt_index = (leaf_index & mask) + top;
    const uint32_t peak = (uint32_t)__popcll(mmr.num_leafs) - (uint32_t)__popcll(mmr.num_leafs & mask) - 1u;
    if (path_len != h || peak >= mmr.n_peaks) return false;
    for (uint32_t lvl = 0; lvl < h; ++lvl) {
        uint64_t s[16];
        const bool odd = (mt_index & 1ull) != 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const uint64_t sib = to_mont(path[5 * (size_t)lvl + k]);
            s[k] = odd ? sib : run[k];  // odd: hash_pair(sibling, acc)
            s[5 + k] = odd ? run[k] : sib;
        }
        tip5_hash_pair_digest(s, lut);  // capacity 1: FixedLength domain
#pragma unroll
        for (int k = 0; k < 5; ++k) run[k] = s[k];
        mt_index >>= 1;
    }
    bool eq = true;
#pragma unroll
    for (int k = 0; k < 5; ++k) eq &= (run[k] == to_mont(mmr.peaks[5 * (size_t)peak + k]));
    return eq;
}

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

__global__ void __launch_bounds__(256) k_ms_chunk_auth(MmrDev swbf, const uint64_t* __restrict__ chunk_index,
                                                       const uint64_t* __restrict__ path_off,
                                                       const uint64_t* __restrict__ path,
                                                       const uint64_t* __restrict__ rel_off,
                                                       const uint32_t* __restrict__ rel, size_t entries,
                                                       uint8_t* __restrict__ auth) {
    __shared__ Tip5Lds t5;
    tip5_lds_init(t5);
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < entries;
         e += (size_t)gridDim.x * blockDim.x) {
        const uint64_t rbeg = rel_off[e];
        const uint64_t cnt = rel_off[e + 1] - rbeg;
        const uint32_t* __restrict__ idx = rel + rbeg;
        const uint64_t len = cnt + 2;  // [cnt + 1, cnt, idx...]
        uint64_t s[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) s[k] = 0;
        uint64_t pos = 0;
        for (; pos + TIP5_RATE <= len; pos += TIP5_RATE) {
#pragma unroll
            for (int k = 0; k < TIP5_RATE; ++k) {
                const uint64_t w = pos + k;
                s[k] = to_mont(w == 0 ? cnt + 1 : (w == 1 ? cnt : (uint64_t)idx[w - 2]));
            }
            tip5_permute_raw(s, t5.lut);
        }
        const uint64_t rem = len - pos;
#pragma unroll
        for (int k = 0; k < TIP5_RATE; ++k) {
            const uint64_t w = pos + k;
            uint64_t v = (uint64_t)k == rem ? 1ull : 0ull;
            if ((uint64_t)k < rem) v = w == 0 ? cnt + 1 : (w == 1 ? cnt : (uint64_t)idx[w - 2]);
            s[k] = to_mont(v);
        }
        tip5_permute_raw(s, t5.lut);
        uint64_t run[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) run[k] = s[k];
        const uint64_t beg = path_off[e];
        auth[e] = mmr_climb(run, chunk_index[e], swbf, path + 5 * beg, path_off[e + 1] - beg, t5.lut) ? 1 : 0;
    }
}

// active: sorted ascending
__device__ __forceinline__ bool active_contains(const uint32_t* __restrict__ active, uint64_t n_active, uint32_t x) {
    uint64_t lo = 0, hi = n_active;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        const uint32_t v = active[mid];
        if (v == x) return true;
        if (v < x) lo = mid + 1;
        else hi = mid;
    }
    return false;
}

// One 64-lane wave per record: lane t < 45 takes index t, and the lanes share the record's entries in the
// validate pass; the flags are ORed over the wave.  (One lane per record left 45 x entries dependent loads
// in a row on a grid of a few dozen waves: the launch then took as long at 512 records as at 4,096.)
static_assert(MSK_NUM_TRIALS <= 64, "one lane per index");
__global__ void __launch_bounds__(256) k_ms_records(MsRecordsDev r, size_t n) {
    using u128 = unsigned __int128;
    // get_batch_index (util_types/mutator_set.rs:74-76) and the active window's first index
    const uint64_t batch = (r.aocl_num_leafs ? r.aocl_num_leafs - 1 : 0) / MSK_BATCH_SIZE;
    const u128 start = (u128)batch << MSK_CHUNK_BITS;
    const u128 chunk_max = (u128)batch + (MSK_WINDOW_CHUNKS - 1);
    const uint32_t lane = threadIdx.x & 63u;
    const size_t wave = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6;
    const size_t n_waves = ((size_t)gridDim.x * blockDim.x) >> 6;
    for (size_t i = wave; i < n; i += n_waves) {  // wave-uniform
        const u128 mn = ((u128)r.minimum[2 * i + 1] << 64) | r.minimum[2 * i];
        const uint32_t* __restrict__ dist = r.distances + (size_t)MSK_NUM_TRIALS * i;
        const uint64_t ebeg = r.entry_off[i], eend = r.entry_off[i + 1];
        const bool not_in_aocl = r.aocl_member && r.aocl_member[i] != 1;
        const bool mine = lane < MSK_NUM_TRIALS;
        // AbsoluteIndexSet::to_array (absolute_index_set.rs:125-131); fail closed past the window
        const u128 index = mine ? mn + dist[lane] : mn;
        const bool out_of_range = __any(mine && (index < mn || (index >> MSK_CHUNK_BITS) > chunk_max)) != 0;
        bool absent_chunk = false, bad_path = false, has_absent = false;
        if (!out_of_range) {
            if (mine) {
                const uint64_t ci = (uint64_t)(index >> MSK_CHUNK_BITS);  // <= batch + 255: exact
                if (ci < batch) {
                    uint64_t e = ebeg;  // ChunkDictionary::get: the first entry with the key
                    while (e < eend && r.chunk_index[e] != ci) ++e;
                    if (e == eend) {
                        absent_chunk = true;
                    } else {
                        if (r.aocl_member && r.auth[e] != 1) bad_path = true;  // verify: the required entries only
                        const uint32_t want = (uint32_t)index & ((1u << MSK_CHUNK_BITS) - 1);
                        bool found = false;
                        for (uint64_t k = r.rel_off[e]; k < r.rel_off[e + 1]; ++k) found |= r.rel[k] == want;
                        has_absent = !found;
                    }
                } else {
                    has_absent = !active_contains(r.active, r.n_active, (uint32_t)(index - start));
                }
            }
            if (!r.aocl_member) {
                // validate: every entry authenticated, and no entry whose chunk index is not required
                for (uint64_t e = ebeg + lane; e < eend; e += 64) {
                    if (r.auth[e] != 1) bad_path = true;
                    const uint64_t ce = r.chunk_index[e];
                    bool required = false;
                    if (ce < batch)
                        for (uint32_t t = 0; t < MSK_NUM_TRIALS; ++t)
                            required |= (uint64_t)((mn + dist[t]) >> MSK_CHUNK_BITS) == ce;
                    if (!required) absent_chunk = true;
                }
            }
        }
        absent_chunk = __any(absent_chunk) != 0;
        bad_path = __any(bad_path) != 0;
        has_absent = __any(has_absent) != 0;
        const bool valid = !out_of_range && !absent_chunk && !bad_path;
        uint8_t status = NHIP_MS_OK;
        if (not_in_aocl) status = NHIP_MS_NOT_IN_AOCL;
        else if (out_of_range) status = NHIP_MS_OUT_OF_RANGE;
        else if (absent_chunk) status = NHIP_MS_ABSENT_CHUNK;
        else if (bad_path) status = NHIP_MS_BAD_MMR_PATH;
        else if (!has_absent) status = NHIP_MS_ALREADY_REMOVED;
        if (lane == 0) {
            if (r.valid) r.valid[i] = valid ? 1 : 0;
            r.verdict[i] = status == NHIP_MS_OK ? 1 : 0;
            r.status[i] = status;
        }
    }
}

static inline unsigned ms_grid(size_t n) {
    const size_t g = (n + 255) / 256;
    return (unsigned)(g > 16384 ? 16384 : g);  // grid-stride beyond 16k workgroups
}

hipError_t launch_mmr_verify(const MmrDev& mmr, const uint64_t* d_leaf_index, const uint64_t* d_leaves,
                             const uint64_t* d_path_off, const uint64_t* d_path, size_t n, uint8_t* d_verdicts,
                             hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_mmr_verify, dim3(ms_grid(n)), dim3(256), 0, st, mmr, d_leaf_index, d_leaves, d_path_off,
                       d_path, n, d_verdicts);
    return hipGetLastError();
}

hipError_t launch_ms_aocl_leaf(const MmrDev& aocl, const uint64_t* d_digests, const uint64_t* d_leaf_index,
                               const uint64_t* d_path_off, const uint64_t* d_path, size_t n, uint8_t* d_member,
                               hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ms_aocl_leaf, dim3(ms_grid(n)), dim3(256), 0, st, aocl, d_digests, d_leaf_index, d_path_off,
                       d_path, n, d_member);
    return hipGetLastError();
}

hipError_t launch_ms_chunk_auth(const MmrDev& swbf, const uint64_t* d_chunk_index, const uint64_t* d_path_off,
                                const uint64_t* d_path, const uint64_t* d_rel_off, const uint32_t* d_rel,
                                size_t entries, uint8_t* d_auth, hipStream_t st) {
    if (entries == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ms_chunk_auth, dim3(ms_grid(entries)), dim3(256), 0, st, swbf, d_chunk_index, d_path_off,
                       d_path, d_rel_off, d_rel, entries, d_auth);
    return hipGetLastError();
}

hipError_t launch_ms_records(const MsRecordsDev& r, size_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ms_records, dim3(ms_grid(64 * n)), dim3(256), 0, st, r, n);  // a wave per record
    return hipGetLastError();
}

}  // namespace nhip
