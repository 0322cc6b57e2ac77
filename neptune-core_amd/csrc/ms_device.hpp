// Device functions shared by the mutator-set kernels (ms_kernels.hip: one accumulator per launch;
// ms_apply_kernels.hip: one accumulator per job): the MMR climb, the chunk sponge, the authentication of one
// dictionary entry, the per-record validate / can_remove decision, the lane-per-item launch.  DESIGN.md §6c, §6d.
#pragma once
#include "../../include/neptune_hip.h"
#include "kernels.hpp"
#include "tip5_device.hpp"

namespace nhip {

static constexpr uint32_t MSK_CHUNK_BITS = 12;                     // CHUNK_SIZE = 2^12 (shared.rs:13)
static constexpr uint32_t MSK_BATCH_SIZE = MsJobScratch::BATCH_SIZE;  // BATCH_SIZE (shared.rs:14)
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

// Tip5::hash(chunk): hash_varlen of [cnt + 1, cnt, idx_0 .. idx_{cnt-1}], the words taken from
// word(i) (i < cnt) as the sponge reaches them.  run: the digest, raw Montgomery.
template <class Word>
__device__ __forceinline__ void ms_chunk_sponge(uint64_t cnt, Word&& word, uint64_t run[5],
                                                const uint8_t* __restrict__ lut) {
    const uint64_t len = cnt + 2;  // [cnt + 1, cnt, idx...]
    uint64_t s[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) s[k] = 0;
    uint64_t pos = 0;
    for (; pos + TIP5_RATE <= len; pos += TIP5_RATE) {
#pragma unroll
        for (int k = 0; k < TIP5_RATE; ++k) {
            const uint64_t w = pos + k;
            s[k] = to_mont(w == 0 ? cnt + 1 : (w == 1 ? cnt : (uint64_t)word(w - 2)));
        }
        tip5_permute_raw(s, lut);
    }
    const uint64_t rem = len - pos;
#pragma unroll
    for (int k = 0; k < TIP5_RATE; ++k) {
        const uint64_t w = pos + k;
        uint64_t v = (uint64_t)k == rem ? 1ull : 0ull;
        if ((uint64_t)k < rem) v = w == 0 ? cnt + 1 : (w == 1 ? cnt : (uint64_t)word(w - 2));
        s[k] = to_mont(v);
    }
    tip5_permute_raw(s, lut);
#pragma unroll
    for (int k = 0; k < 5; ++k) run[k] = s[k];
}

// Entry e of the dictionaries ch against swbf: Tip5::hash(chunk), then the MMR climb at leaf index chunk_index[e]
// (removal_record.rs:237-243, mutator_set_accumulator.rs:309-316).  k_ms_chunk_auth and k_ms_chunk_auth_jobs.
__device__ __forceinline__ bool ms_chunk_auth_entry(const MsChunksDev& ch, size_t e, const MmrDev& swbf,
                                                    const uint8_t* __restrict__ lut) {
    const uint64_t rbeg = ch.rel_off[e], cnt = ch.rel_off[e + 1] - rbeg;
    const uint32_t* __restrict__ idx = ch.rel + rbeg;
    uint64_t run[5];
    ms_chunk_sponge(cnt, [&](uint64_t w) { return idx[w]; }, run, lut);
    const uint64_t beg = ch.path_off[e];
    return mmr_climb(run, ch.chunk_index[e], swbf, ch.path + 5 * beg, ch.path_off[e + 1] - beg, lut);
}

// kernel(args...) in 256-thread workgroups over `lanes` lanes' worth of items; nothing to do is no launch
template <class Kernel, class... Args>
hipError_t ms_launch(Kernel kernel, size_t lanes, hipStream_t st, Args... args) {
    if (lanes == 0) return hipSuccess;
    const size_t g = (lanes + 255) / 256;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(g > 16384 ? 16384 : g)), dim3(256), 0, st, args...);  // then grid-stride
    return hipGetLastError();
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

// RemovalRecord::validate and can_remove / verify of record i by one 64-lane wave (lane t < 45 takes
// index t; the flags are ORed over the wave), against the accumulator given by (active, n_active,
// aocl_num_leafs).  Lane 0 writes r.valid / r.verdict / r.status.  index_set, when not null: 45 bytes
// per record, 1 where can_remove finds that index set (its chunk's entry or the active window holds
// it), written for records that validate.  Wave-uniform in i.
static_assert(MSK_NUM_TRIALS <= 64, "one lane per index");
__device__ __forceinline__ void ms_record_decide(const MsRecordsDev& r, size_t i, uint32_t lane,
                                                 const uint32_t* __restrict__ active, uint64_t n_active,
                                                 uint64_t aocl_num_leafs, uint8_t* __restrict__ index_set) {
    using u128 = unsigned __int128;
    // get_batch_index (util_types/mutator_set.rs:74-76) and the active window's first index
    const uint64_t batch = MsJobScratch::batch_index(aocl_num_leafs);
    const u128 start = (u128)batch << MSK_CHUNK_BITS;
    const u128 chunk_max = (u128)batch + (MSK_WINDOW_CHUNKS - 1);
    const u128 mn = ((u128)r.minimum[2 * i + 1] << 64) | r.minimum[2 * i];
    const uint32_t* __restrict__ dist = r.distances + (size_t)MSK_NUM_TRIALS * i;
    const uint64_t ebeg = r.ch.entry_off[i], eend = r.ch.entry_off[i + 1];
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
                while (e < eend && r.ch.chunk_index[e] != ci) ++e;
                if (e == eend) {
                    absent_chunk = true;
                } else {
                    if (r.aocl_member && r.auth[e] != 1) bad_path = true;  // verify: the required entries only
                    const uint32_t want = (uint32_t)index & ((1u << MSK_CHUNK_BITS) - 1);
                    bool found = false;
                    for (uint64_t k = r.ch.rel_off[e]; k < r.ch.rel_off[e + 1]; ++k) found |= r.ch.rel[k] == want;
                    has_absent = !found;
                }
            } else {
                has_absent = !active_contains(active, n_active, (uint32_t)(index - start));
            }
        }
        if (!r.aocl_member) {
            // validate: every entry authenticated, and no entry whose chunk index is not required
            for (uint64_t e = ebeg + lane; e < eend; e += 64) {
                if (r.auth[e] != 1) bad_path = true;
                const uint64_t ce = r.ch.chunk_index[e];
                bool required = false;
                if (ce < batch)
                    for (uint32_t t = 0; t < MSK_NUM_TRIALS; ++t)
                        required |= (uint64_t)((mn + dist[t]) >> MSK_CHUNK_BITS) == ce;
                if (!required) absent_chunk = true;
            }
        }
    }
    if (index_set && mine) index_set[(size_t)MSK_NUM_TRIALS * i + lane] = (!out_of_range && !absent_chunk && !has_absent) ? 1 : 0;
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

// ---- shared by k_ms_apply (ms_apply_kernels.hip) and the witness kernels (ms_update_kernels.hip)
using u128 = unsigned __int128;
static constexpr uint64_t MSA_NONE = ~0ull;


// hash_pair on canonical digests
__device__ __forceinline__ void dig_hp(const uint64_t* l, const uint64_t* r, uint64_t* out,
                                       const uint8_t* __restrict__ lut) {
    uint64_t s[16];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        s[k] = to_mont(l[k]);
        s[5 + k] = to_mont(r[k]);
    }
    tip5_hash_pair_digest(s, lut);
#pragma unroll
    for (int k = 0; k < 5; ++k) out[k] = from_mont(s[k]);
}

// the job's indices in the host's order: slot s -> (index, record in job)
struct JobIndices {
    const uint64_t* mn;    // the job's first record
    const uint32_t* dist;
    const uint32_t* perm;
    __device__ __forceinline__ u128 at(uint64_t s, uint32_t* rec = nullptr) const {
        const uint32_t p = perm[s];
        const uint32_t r = p / MSK_NUM_TRIALS;
        if (rec) *rec = r;
        return (((u128)mn[2 * (size_t)r + 1] << 64) | mn[2 * (size_t)r]) + dist[p];
    }
    // first slot in [lo, hi) whose index is >= v
    __device__ __forceinline__ uint64_t lower_bound(uint64_t lo, uint64_t hi, u128 v) const {
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (at(mid) < v) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    }
};

// first position in the sorted a[0 .. n) with a[pos] >= x
__device__ __forceinline__ uint64_t lb_u32(const uint32_t* a, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if ((uint64_t)a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// first group in [0, n) whose chunk index (aux[2 g + 1]) shifted right by sh is >= key
__device__ __forceinline__ uint64_t lb_group(const uint64_t* aux, uint64_t n, uint32_t sh, uint64_t key) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if ((aux[2 * mid + 1] >> sh) < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// index of the peak of height h in the peak list of an MMR of n leaves (bit h of n set)
__device__ __forceinline__ uint32_t peak_of_height(uint64_t n, uint32_t h) {
    return h >= 63 ? 0u : (uint32_t)__popcll(n >> (h + 1));
}

}  // namespace nhip
