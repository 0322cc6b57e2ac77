// Membership proofs and removal records back across a block: every witness of a job of
// nhip_ms_apply_batch, standing at the accumulator after it, taken to msa_before, as the end state.  The kernels run
// behind k_ms_chunk_auth_jobs and k_ms_records_jobs over the block's records and behind k_ms_apply, whose group
// table (a.aux: per group the record's dictionary entry and the chunk index, the touched chunks first) they read as
// it left it.  What the block changed in swbf_inactive is undone from the block's own records: a record's entry
// holds the chunk and its path before the block, so Tip5::hash(old chunk) climbed along that path is the old value
// of every ancestor of a touched chunk.  No cross-chunk lookup, no barrier, no workgroup per job.
//
//  k_ms_revert_nodes : a lane per group of every job; a touched group of an accepted job hashes the record's own
//                      chunk words and climbs the entry's path, keeping level L at node_off[job] + L n_grp + g.
//                      Groups that share an ancestor compute it twice.
//  k_ms_rev_admit    : a lane per witness: the admission rules in the header's order; integers and words only
//  k_ms_rev_paths    : eight lanes per output path (the AOCL paths, then the dictionaries' paths): a digest is the
//                      witness's own, or the old node (t, sibling) found with lb_group at that height
//  k_ms_rev_chunks   : eight lanes per output entry: the key, and the multiset difference of two sorted lists
//                      (the witness's chunk less the block's indices in it), every kept word placed by its rank
//  k_ms_rev_aocl_jobs: a lane per witness: its reverted AOCL part under its own job's msa_before.aocl (mmr_climb)
//  k_ms_rev_seal     : a lane per witness, behind k_ms_rev_aocl_jobs and k_ms_chunk_auth_jobs over the reverted witnesses:
//                      the first failure of admission, the error bytes and the verification; a failed witness's
//                      slots are zeroed
// Every lane writes inside the plan's ranges only: a length that disagrees with the plan is an error, not a write.
#include "ms_device.hpp"

namespace nhip {

namespace {

__device__ __forceinline__ uint32_t ilog2_dev(uint64_t x) { return 63u - (uint32_t)__clzll((long long)x); }

// the job of group i of the call: the last job whose groups begin at or before i
__device__ __forceinline__ size_t job_of_group(const MsApplyJob* jobs, size_t n_jobs, uint64_t i) {
    size_t lo = 0, hi = n_jobs;  // jobs[lo].grp_off <= i: jobs[0].grp_off == 0
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (jobs[mid].grp_off <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the in-chunk values of the job's slots [s0, s1) of one chunk are ascending: first slot with value >= v
__device__ __forceinline__ uint64_t lb_slot(const JobIndices& ix, uint64_t s0, uint64_t s1, uint64_t v) {
    const uint32_t in_chunk = (1u << MSK_CHUNK_BITS) - 1;
    uint64_t lo = s0, hi = s1;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if ((uint64_t)((uint32_t)ix.at(mid) & in_chunk) < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void zero_slots(const MsUpdateDev& u, size_t w) {
    for (uint64_t d = 5 * u.o_aocl_path_off[w]; d < 5 * u.o_aocl_path_off[w + 1]; ++d) u.o_aocl_path[d] = 0;
    const uint64_t ebeg = u.o_entry_off[w], eend = u.o_entry_off[w + 1];
    for (uint64_t e = ebeg; e < eend; ++e) u.o_chunk_index[e] = 0;
    for (uint64_t d = 5 * u.o_path_off[ebeg]; d < 5 * u.o_path_off[eend]; ++d) u.o_path[d] = 0;
    for (uint64_t d = u.o_rel_off[ebeg]; d < u.o_rel_off[eend]; ++d) u.o_rel[d] = 0;
}

}  // namespace

__global__ void __launch_bounds__(256) k_ms_revert_nodes(MsApplyDev a, MsRevertDev r, size_t n_jobs, size_t groups) {
    __shared__ Tip5Lds t5;
    tip5_lds_init(t5);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < groups; i += (size_t)gridDim.x * blockDim.x) {
        const size_t j = job_of_group(a.jobs, n_jobs, i);
        const MsApplyJob& jb = a.jobs[j];
        const uint64_t g = i - jb.grp_off;
        if (g >= jb.n_grp || a.status[j] != NHIP_MS_OK) continue;  // the group table is an accepted job's only
        const uint64_t* aux = a.aux + 2 * jb.grp_off;
        const uint64_t b0 = MsJobScratch::batch_index(jb.aocl_n);
        if (g >= lb_group(aux, jb.n_grp, 0, b0)) continue;  // a chunk still in the window
        const uint64_t e = aux[2 * g], ci = aux[2 * g + 1];
        if (e == MSA_NONE) continue;  // not reached: the record validated
        const uint32_t h = ilog2_dev(ci ^ b0);  // ci < b0; the entry's path has h digests: it authenticated
        const uint64_t plen = a.rec.ch.path_off[e + 1] - a.rec.ch.path_off[e];
        const uint64_t* __restrict__ path = a.rec.ch.path + 5 * a.rec.ch.path_off[e];
        const uint32_t* __restrict__ idx = a.rec.ch.rel + a.rec.ch.rel_off[e];
        uint64_t* out = r.nodes + 5 * (r.node_off[j] + g);  // level L: + 5 L n_grp
        uint64_t run[5];
        ms_chunk_sponge(a.rec.ch.rel_off[e + 1] - a.rec.ch.rel_off[e], [&](uint64_t w) { return idx[w]; }, run, t5.lut);
#pragma unroll
        for (int q = 0; q < 5; ++q) out[q] = from_mont(run[q]);
        // levels 1 .. h - 1: level h is the old peak, which is nobody's sibling
        for (uint32_t L = 0; L + 1 < h && L < plen; ++L) {
            uint64_t s[16];
            const bool odd = ((ci >> L) & 1ull) != 0;
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const uint64_t sib = to_mont(path[5 * (size_t)L + q]);
                s[q] = odd ? sib : run[q];
                s[5 + q] = odd ? run[q] : sib;
            }
            tip5_hash_pair_digest(s, t5.lut);
            out += 5 * jb.n_grp;
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                run[q] = s[q];
                out[q] = from_mont(s[q]);
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_ms_rev_admit(MsApplyDev a, MsUpdateDev u, MsRevertDev r, size_t witnesses) {
    for (size_t w = blockIdx.x * (size_t)blockDim.x + threadIdx.x; w < witnesses; w += (size_t)gridDim.x * blockDim.x) {
        const uint32_t j = u.wit_job[w];
        u.err[w] = 0;
        r.short_of[w] = 0;
        if (a.status[j] != NHIP_MS_OK) {
            u.status[w] = NHIP_MS_JOB_REJECTED;
            continue;
        }
        const MsApplyJob& jb = a.jobs[j];
        const MsJobScratch s(jb.aocl_n, jb.k);  // no wrap: the job is consistent
        const uint64_t l = u.aocl_leaf_index[w];
        bool in_aocl = true;
        if (l != MSA_NONE) {
            const uint64_t plen = u.aocl_path_off[w + 1] - u.aocl_path_off[w];
            in_aocl = l < s.n0 && plen == ilog2_dev(l ^ s.n1);  // l >= n0: born in this block or later
        }
        const u128 mn = ((u128)u.minimum[2 * w + 1] << 64) | u.minimum[2 * w];
        const uint32_t* __restrict__ dist = u.distances + (size_t)MSK_NUM_TRIALS * w;
        const uint64_t ebeg = u.ch.entry_off[w], eend = u.ch.entry_off[w + 1];
        const u128 chunk_max = (u128)s.b1 + (MSK_WINDOW_CHUNKS - 1);
        bool out_of_range = false, absent = false, bad_path = false;
        for (uint32_t t = 0; t < MSK_NUM_TRIALS; ++t) {
            const u128 v = mn + dist[t];
            if (v < mn || (v >> MSK_CHUNK_BITS) > chunk_max) out_of_range = true;
        }
        if (!out_of_range) {
            // the keys, strictly ascending, are exactly the chunk indices below b1
            uint64_t prev = 0;
            for (uint64_t e = ebeg; e < eend; ++e) {
                const uint64_t key = u.ch.chunk_index[e];
                if ((e > ebeg && key <= prev) || key >= s.b1) {
                    absent = true;
                } else if (u.ch.path_off[e + 1] - u.ch.path_off[e] != ilog2_dev(key ^ s.b1)) {
                    bad_path = true;
                }
                prev = key;
                bool required = false;
                for (uint32_t t = 0; t < MSK_NUM_TRIALS; ++t)
                    required |= (uint64_t)((mn + dist[t]) >> MSK_CHUNK_BITS) == key;
                if (!required) absent = true;
            }
            for (uint32_t t = 0; t < MSK_NUM_TRIALS; ++t) {
                const uint64_t ci = (uint64_t)((mn + dist[t]) >> MSK_CHUNK_BITS);  // <= b1 + 255: exact
                if (ci >= s.b1) continue;
                bool found = false;
                for (uint64_t e = ebeg; e < eend; ++e) found |= u.ch.chunk_index[e] == ci;
                if (!found) absent = true;
            }
        }
        uint8_t status = NHIP_MS_OK;
        if (!in_aocl) status = NHIP_MS_NOT_IN_AOCL;
        else if (out_of_range) status = NHIP_MS_OUT_OF_RANGE;
        else if (absent) status = NHIP_MS_ABSENT_CHUNK;
        else if (bad_path) status = NHIP_MS_BAD_MMR_PATH;
        u.status[w] = status;
    }
}

__global__ void __launch_bounds__(256) k_ms_rev_paths(MsApplyDev a, MsUpdateDev u, MsRevertDev r, size_t witnesses,
                                                      size_t entries) {
    constexpr uint32_t LANES = 8;  // per path; no lane waits for another
    const uint32_t lane = threadIdx.x & (LANES - 1);
    const size_t team = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) / LANES;
    const size_t n_teams = ((size_t)gridDim.x * blockDim.x) / LANES;
    for (size_t i = team; i < witnesses + entries; i += n_teams) {
        const bool is_aocl = i < witnesses;
        const uint64_t e = is_aocl ? 0 : i - witnesses;
        const uint64_t w = is_aocl ? i : u.o_ent_wit[e];
        const uint64_t* __restrict__ off = is_aocl ? u.o_aocl_path_off + w : u.o_path_off + e;
        const uint64_t d0 = off[0], len = off[1] - d0;  // the path's digests in its output array
        const bool accepted = u.status[w] == NHIP_MS_OK;
        // the witness's own path, of which the output is a prefix with some digests replaced
        const uint64_t* own = nullptr;
        uint64_t own_len = 0, T = 0, b0 = 0, n_grp = 0, c = 0;
        const uint64_t* aux = nullptr;
        const uint64_t* nodes = nullptr;
        if (accepted) {
            if (is_aocl) {
                own = u.aocl_path + 5 * u.aocl_path_off[w];
                own_len = u.aocl_path_off[w + 1] - u.aocl_path_off[w];
            } else {
                const uint32_t j = u.wit_job[w];
                const MsApplyJob& jb = a.jobs[j];
                const uint64_t se = u.o_ent_src[e];
                if (se != MSA_NONE) {
                    own = u.ch.path + 5 * u.ch.path_off[se];
                    own_len = u.ch.path_off[se + 1] - u.ch.path_off[se];
                }
                c = u.o_key[e];
                b0 = MsJobScratch::batch_index(jb.aocl_n);
                n_grp = jb.n_grp;
                aux = a.aux + 2 * jb.grp_off;
                T = lb_group(aux, n_grp, 0, b0);  // the job's touched chunks: groups [0, T)
                nodes = r.nodes + 5 * r.node_off[j];
            }
        }
        for (uint64_t tt = lane; tt < len; tt += LANES) {
            uint64_t* dst = (is_aocl ? u.o_aocl_path : u.o_path) + 5 * (d0 + tt);
            const uint64_t* src = nullptr;
            if (accepted) {
                if (tt < own_len) src = own + 5 * tt;
                if (!is_aocl && tt < 63) {
                    const uint32_t t = (uint32_t)tt;
                    const uint64_t q = (c >> t) ^ 1ull;
                    const uint64_t x = lb_group(aux, T, t, q);
                    if (x < T && (aux[2 * x + 1] >> t) == q) {  // a touched chunk, or an ancestor of one
                        const uint32_t hx = ilog2_dev(aux[2 * x + 1] ^ b0);  // k_ms_revert_nodes kept levels below hx
                        // (hx == 0, a chunk that is its own peak, is nobody's sibling: its level 0 is kept but a path
                        // that would read it has len 0 and does not come here)
                        src = t < (hx ? hx : 1u) ? nodes + 5 * ((uint64_t)t * n_grp + x) : nullptr;
                    }
                }
                if (!src) u.err[w] = 1;
            }
#pragma unroll
            for (int q = 0; q < 5; ++q) dst[q] = src ? src[q] : 0ull;
        }
    }
}

__global__ void __launch_bounds__(256) k_ms_rev_chunks(MsApplyDev a, MsUpdateDev u, MsRevertDev r, size_t entries) {
    constexpr uint32_t LANES = 8;  // per entry; no lane waits for another
    const uint32_t lane = threadIdx.x & (LANES - 1);
    const size_t team = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) / LANES;
    const size_t n_teams = ((size_t)gridDim.x * blockDim.x) / LANES;
    for (size_t e = team; e < entries; e += n_teams) {
        const uint64_t w = u.o_ent_wit[e];
        const uint64_t c = u.o_key[e];
        uint32_t* dst = u.o_rel + u.o_rel_off[e];
        const uint64_t len = u.o_rel_off[e + 1] - u.o_rel_off[e];
        bool ok = u.status[w] == NHIP_MS_OK;
        const uint32_t* cur = nullptr;
        uint64_t n_cur = 0, s0 = 0, s1 = 0;
        JobIndices ix{nullptr, nullptr, nullptr};
        if (ok) {
            const uint32_t j = u.wit_job[w];
            const MsApplyJob& jb = a.jobs[j];
            ix = JobIndices{a.rec.minimum + 2 * jb.rec_off, a.rec.distances + MSK_NUM_TRIALS * jb.rec_off,
                            a.idx_perm + MSK_NUM_TRIALS * jb.rec_off};
            const uint64_t* aux = a.aux + 2 * jb.grp_off;
            const uint32_t* grp = a.grp + jb.grp_off + j;
            const uint64_t T = lb_group(aux, jb.n_grp, 0, MsJobScratch::batch_index(jb.aocl_n));
            const uint64_t g = lb_group(aux, T, 0, c);
            if (g < T && aux[2 * g + 1] == c) {
                s0 = grp[g];
                s1 = grp[g + 1];
            }
            const uint64_t se = u.o_ent_src[e];
            if (se == MSA_NONE) {
                ok = false;  // not reached: the witness was admitted
                if (lane == 0) u.err[w] = 1;
            } else {
                cur = u.ch.rel + u.ch.rel_off[se];
                n_cur = u.ch.rel_off[se + 1] - u.ch.rel_off[se];
                if (n_cur < s1 - s0) {  // the planned length was floored
                    ok = false;
                    if (lane == 0) r.short_of[w] = 1;
                } else if (n_cur - (s1 - s0) != len) {  // the plan counted otherwise
                    ok = false;
                    if (lane == 0) u.err[w] = 1;
                }
            }
        }
        if (lane == 0) u.o_chunk_index[e] = ok ? c : 0ull;
        if (!ok) {
            for (uint64_t p = lane; p < len; p += LANES) dst[p] = 0;
            continue;
        }
        const uint32_t in_chunk = (1u << MSK_CHUNK_BITS) - 1;
        // the word at position p, the rank-th of its value, goes if the block inserted more copies than that; a word
        // that stays moves down by the block's indices below it and its own value's copies.  The witness's chunk is not
        // authenticated yet and may be unsorted: the ranks are then meaningless, `pos < len` keeps every write inside
        // the plan's range, words that no lane writes stay as they are until the verification behind this kernel
        // rejects the chunk and k_ms_rev_seal zeroes it.  An unsorted input is caught there, not here.
        for (uint64_t p = lane; p < n_cur; p += LANES) {
            const uint32_t v = cur[p];
            const uint64_t rank = p - lb_u32(cur, n_cur, v);
            const uint64_t lo = lb_slot(ix, s0, s1, v), hi = lb_slot(ix, lo, s1, (uint64_t)v + 1);
            if (rank < hi - lo) continue;
            const uint64_t pos = p - (lo - s0) - (hi - lo);
            if (pos < len) dst[pos] = v;
        }
        // every block index is there as often as the block inserted it
        for (uint64_t s = s0 + lane; s < s1; s += LANES) {
            const uint32_t vb = (uint32_t)ix.at(s) & in_chunk;
            const uint64_t have = lb_u32(cur, n_cur, (uint64_t)vb + 1) - lb_u32(cur, n_cur, vb);
            const uint64_t lo = lb_slot(ix, s0, s1, vb), hi = lb_slot(ix, lo, s1, (uint64_t)vb + 1);
            if (have < hi - lo) r.short_of[w] = 1;
        }
    }
}

// MmrMembershipProof::verify of every reverted AOCL part against its own job's msa_before.aocl (k_mmr_verify with the
// job looked up witness -> job, as k_ms_chunk_auth_jobs looks up entry -> owner -> job): one launch for any number of jobs
__global__ void __launch_bounds__(256) k_ms_rev_aocl_jobs(MsApplyDev a, MsUpdateDev u, uint8_t* __restrict__ member,
                                                          size_t witnesses) {
    __shared__ Tip5Lds t5;
    tip5_lds_init(t5);
    for (size_t w = blockIdx.x * (size_t)blockDim.x + threadIdx.x; w < witnesses; w += (size_t)gridDim.x * blockDim.x) {
        const MsApplyJob& jb = a.jobs[u.wit_job[w]];
        const MmrDev aocl{a.peaks + 5 * jb.aocl_peaks, jb.aocl_np, jb.aocl_n};
        uint64_t run[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) run[k] = to_mont(u.aocl_leaf[5 * w + k]);
        const uint64_t beg = u.o_aocl_path_off[w];
        member[w] = mmr_climb(run, u.aocl_leaf_index[w], aocl, u.o_aocl_path + 5 * beg, u.o_aocl_path_off[w + 1] - beg, t5.lut) ? 1 : 0;
    }
}

__global__ void __launch_bounds__(256) k_ms_rev_seal(MsUpdateDev u, MsRevertDev r, size_t witnesses) {
    for (size_t w = blockIdx.x * (size_t)blockDim.x + threadIdx.x; w < witnesses; w += (size_t)gridDim.x * blockDim.x) {
        if (u.status[w] != NHIP_MS_OK) continue;  // its slots are zero already
        uint8_t status = NHIP_MS_OK;
        if (u.err[w]) {
            status = NHIP_MS_UPDATE_INTERNAL;
        } else if (r.short_of[w]) {
            status = NHIP_MS_BAD_MMR_PATH;
        } else if (u.aocl_leaf_index[w] != MSA_NONE && r.member[w] != 1) {
            status = NHIP_MS_NOT_IN_AOCL;
        } else {
            for (uint64_t e = u.o_entry_off[w]; e < u.o_entry_off[w + 1]; ++e)
                if (r.auth[e] != 1) status = NHIP_MS_BAD_MMR_PATH;
        }
        if (status == NHIP_MS_OK) continue;
        u.status[w] = status;
        zero_slots(u, w);
    }
}

hipError_t launch_ms_revert_nodes(const MsApplyDev& a, const MsRevertDev& r, size_t n_jobs, size_t groups, hipStream_t st) {
    return ms_launch(k_ms_revert_nodes, groups, st, a, r, n_jobs, groups);
}

hipError_t launch_ms_rev_admit(const MsApplyDev& a, const MsUpdateDev& u, const MsRevertDev& r, size_t witnesses, hipStream_t st) {
    return ms_launch(k_ms_rev_admit, witnesses, st, a, u, r, witnesses);
}

hipError_t launch_ms_rev_paths(const MsApplyDev& a, const MsUpdateDev& u, const MsRevertDev& r, size_t witnesses,
                               size_t entries, hipStream_t st) {
    return ms_launch(k_ms_rev_paths, 8 * (witnesses + entries), st, a, u, r, witnesses, entries);  // 8 lanes per path
}

hipError_t launch_ms_rev_chunks(const MsApplyDev& a, const MsUpdateDev& u, const MsRevertDev& r, size_t entries, hipStream_t st) {
    return ms_launch(k_ms_rev_chunks, 8 * entries, st, a, u, r, entries);  // 8 lanes per entry
}

hipError_t launch_ms_rev_aocl_jobs(const MsApplyDev& a, const MsUpdateDev& u, uint8_t* d_member, size_t witnesses, hipStream_t st) {
    return ms_launch(k_ms_rev_aocl_jobs, witnesses, st, a, u, d_member, witnesses);
}

hipError_t launch_ms_rev_seal(const MsUpdateDev& u, const MsRevertDev& r, size_t witnesses, hipStream_t st) {
    return ms_launch(k_ms_rev_seal, witnesses, st, u, r, witnesses);
}

}  // namespace nhip
