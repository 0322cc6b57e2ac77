// Membership proofs and removal records across a block: every witness of a job of
// nhip_ms_apply_batch brought up to the accumulator after it, as the end state.  The kernels run behind
// k_ms_chunk_auth_jobs over the witnesses' dictionaries (the job looked up entry -> witness -> job) and behind
// k_ms_apply<true>, which keeps the nodes it computes in the job's digest scratch.  MsJobScratch (ms_shape.hpp) says
// where: k_ms_apply writes through it and these kernels read through it.  Both appends leave heights >= 1 of the nodes
// wholly among the appended leaves level after level (block_mmr_append's own layout; height 0 is the addition records
// or the new chunks' digests) and their left edge (the nodes that hold old and new leaves) in a.carry; the leaf
// mutation leaves level L of touched chunk g at mut_node, found as the kernel itself finds a sibling: lb_group over
// the group table at that height.
// A node is addressed by where it must lie, not searched in a table: a sibling block is wholly new (scratch),
// holds the old leaf count (carry) or is wholly old, and then it is a touched node, a digest of the witness's own
// path, or the old peak of exactly that height.  Anything else sets the witness's error byte: never a guess.
//
//  k_ms_wit_admit  : a lane per witness, the admission rules in the header's order (the AOCL climb is mmr_climb)
//  k_ms_wit_paths  : eight lanes per output path (the AOCL paths, then the dictionaries' paths), each digest found
//                    as above and copied.  (A lane per digest had to find its path by a binary search of 21
//                    dependent loads over the plan's offsets first: DESIGN.md §6g.)
//  k_ms_wit_chunks : eight lanes per output entry: the key, and the two-sorted-list merge of the old chunk (the
//                    witness's entry, or its part of the old window) with the block's indices in that chunk, every
//                    word placed by a binary search in the other list.  (A wave per entry left 56 lanes idle on
//                    chunks of 8 words and took 1.86 ms where this takes less: DESIGN.md §6g.)
//  k_ms_wit_seal   : a lane per witness: an error byte becomes NHIP_MS_UPDATE_INTERNAL and zeroes its slots
// Every lane writes inside the plan's ranges only: a length that disagrees with the plan is an error, not a write.
#include "ms_device.hpp"

namespace nhip {

namespace {

// One append of k_ms_apply<true>: the MMR had n leaves and has n1.
struct AppendNodes {
    uint64_t n, n1;
    const uint64_t* leaves;  // height 0: the n1 - n appended digests
    const uint64_t* levels;  // heights >= 1, as block_mmr_append leaves them
    const uint64_t* carry;   // 64 digests by height
    uint64_t mask;
};
enum { NODE_OLD = 0, NODE_HERE = 1, NODE_MISSING = 2 };

// Node q of height t < 64.  NODE_HERE: *out is its digest.  NODE_OLD: its block lies wholly below n.
__device__ __forceinline__ int append_node(const AppendNodes& m, uint32_t t, uint64_t q, const uint64_t** out) {
    const uint64_t low = t ? (m.n & ((1ull << t) - 1)) : 0;
    const uint64_t lo_t = (m.n >> t) + (low != 0), hi_t = m.n1 >> t;
    if (q >= lo_t) {
        if (q >= hi_t) return NODE_MISSING;
        if (t == 0) {
            *out = m.leaves + 5 * (q - m.n);
            return NODE_HERE;
        }
        uint64_t off = 0;  // the nodes of heights 1 .. t - 1
        for (uint32_t L = 1; L < t; ++L) {
            const uint64_t lo = (m.n >> L) + ((m.n & ((1ull << L) - 1)) != 0), hi = m.n1 >> L;
            off += hi > lo ? hi - lo : 0;
        }
        *out = m.levels + 5 * (off + (q - lo_t));
        return NODE_HERE;
    }
    if (low != 0 && q == (m.n >> t)) {
        if (!((m.mask >> t) & 1)) return NODE_MISSING;
        *out = m.carry + 5 * (size_t)t;
        return NODE_HERE;
    }
    return NODE_OLD;
}

__device__ __forceinline__ uint32_t ilog2_dev(uint64_t x) { return 63u - (uint32_t)__clzll((long long)x); }

}  // namespace

__global__ void __launch_bounds__(256) k_ms_wit_admit(MsApplyDev a, MsUpdateDev u, size_t witnesses) {
    __shared__ Tip5Lds t5;
    tip5_lds_init(t5);
    for (size_t w = blockIdx.x * (size_t)blockDim.x + threadIdx.x; w < witnesses; w += (size_t)gridDim.x * blockDim.x) {
        const uint32_t j = u.wit_job[w];
        u.err[w] = 0;
        if (a.status[j] != NHIP_MS_OK) {
            u.status[w] = NHIP_MS_JOB_REJECTED;
            continue;
        }
        const MsApplyJob& jb = a.jobs[j];
        const MsJobScratch s(jb.aocl_n, jb.k);  // no wrap: the job is consistent
        const uint64_t l = u.aocl_leaf_index[w];
        bool in_aocl = true;
        if (l != MSA_NONE) {
            const uint64_t pbeg = u.aocl_path_off[w], plen = u.aocl_path_off[w + 1] - pbeg;
            const uint64_t* leaf = u.aocl_leaf + 5 * w;
            if (l >= s.n1) {
                in_aocl = false;
            } else if (l < s.n0) {
                uint64_t run[5];
#pragma unroll
                for (int q = 0; q < 5; ++q) run[q] = to_mont(leaf[q]);
                const MmrDev aocl{a.peaks + 5 * jb.aocl_peaks, jb.aocl_np, s.n0};
                in_aocl = mmr_climb(run, l, aocl, u.aocl_path + 5 * pbeg, plen, t5.lut);
            } else {  // born in this block
                const uint64_t* add = a.additions + 5 * (jb.add_off + (l - s.n0));
                in_aocl = plen == 0;
#pragma unroll
                for (int q = 0; q < 5; ++q) in_aocl &= leaf[q] == add[q];
            }
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
            // the keys, strictly ascending, are exactly the chunk indices below b0
            uint64_t prev = 0;
            for (uint64_t e = ebeg; e < eend; ++e) {
                const uint64_t key = u.ch.chunk_index[e];
                if ((e > ebeg && key <= prev) || key >= s.b0) absent = true;
                prev = key;
                bool required = false;
                for (uint32_t t = 0; t < MSK_NUM_TRIALS; ++t)
                    required |= (uint64_t)((mn + dist[t]) >> MSK_CHUNK_BITS) == key;
                if (!required) absent = true;
                if (u.auth[e] != 1) bad_path = true;
            }
            for (uint32_t t = 0; t < MSK_NUM_TRIALS; ++t) {
                const uint64_t ci = (uint64_t)((mn + dist[t]) >> MSK_CHUNK_BITS);  // <= b1 + 255: exact
                if (ci >= s.b0) continue;
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

__global__ void __launch_bounds__(256) k_ms_wit_paths(MsApplyDev a, MsUpdateDev u, size_t witnesses, size_t entries) {
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
        uint64_t T = 0;  // the job's touched chunks: groups [0, T), the same for every digest of a dictionary path
        if (accepted && !is_aocl) {
            const MsApplyJob& jb = a.jobs[u.wit_job[w]];
            T = lb_group(a.aux + 2 * jb.grp_off, jb.n_grp, 0, MsJobScratch::batch_index(jb.aocl_n));
        }
        for (uint64_t tt = lane; tt < len; tt += LANES) {
            const uint32_t t = tt < 64 ? (uint32_t)tt : 64u;
            uint64_t* dst = (is_aocl ? u.o_aocl_path : u.o_path) + 5 * (d0 + tt);
            const uint64_t* src = nullptr;
            if (accepted) {
                const uint32_t j = u.wit_job[w];
                const MsApplyJob& jb = a.jobs[j];
                const MsJobScratch s(jb.aocl_n, jb.k);
                const uint64_t n0 = s.n0, n1 = s.n1, b0 = s.b0, b1 = s.b1;
                const uint64_t* dig = a.dig + 5 * jb.dig_off;  // the nodes k_ms_apply<true> kept, where s says
                int r = NODE_MISSING;
                if (t >= 63) {
                    // no path is that long: n1 < 2^64
                } else if (is_aocl) {
                    const uint64_t l = u.aocl_leaf_index[w];
                    const uint64_t q = (l >> t) ^ 1ull;
                    const AppendNodes m{n0, n1, a.additions + 5 * jb.add_off, dig + 5 * s.aocl(), a.carry + (size_t)j * 2 * 64 * 5,
                                        a.carry_mask[2 * (size_t)j]};
                    r = append_node(m, t, q, &src);
                    if (r == NODE_OLD) {
                        const uint64_t pbeg = u.aocl_path_off[w], plen = u.aocl_path_off[w + 1] - pbeg;
                        if (l < n0 && t < plen) {
                            src = u.aocl_path + 5 * (pbeg + t);
                            r = NODE_HERE;
                        } else if (((n0 >> t) & 1) && q == (n0 >> t) - 1) {  // the old peak of exactly that block
                            src = a.peaks + 5 * (jb.aocl_peaks + peak_of_height(n0, t));
                            r = NODE_HERE;
                        } else {
                            r = NODE_MISSING;
                        }
                    }
                } else {
                    const uint64_t c = u.o_key[e];
                    const uint64_t q = (c >> t) ^ 1ull;
                    const AppendNodes m{b0, b1, dig + 5 * s.fresh(), dig + 5 * s.fresh_levels(), a.carry + ((size_t)j * 2 + 1) * 64 * 5,
                                        a.carry_mask[2 * (size_t)j + 1]};
                    r = append_node(m, t, q, &src);
                    if (r == NODE_OLD) {
                        const uint64_t* aux = a.aux + 2 * jb.grp_off;
                        const uint64_t x = lb_group(aux, T, t, q);
                        const uint64_t se = u.o_ent_src[e];
                        if (x < T && (aux[2 * x + 1] >> t) == q) {  // a touched node
                            if (t <= ilog2_dev(aux[2 * x + 1] ^ b0)) {
                                src = dig + 5 * s.mut_node(jb.n_grp, t, x);
                                r = NODE_HERE;
                            } else {
                                r = NODE_MISSING;
                            }
                        } else if (c < b0 && se != MSA_NONE && t < u.ch.path_off[se + 1] - u.ch.path_off[se]) {
                            src = u.ch.path + 5 * (u.ch.path_off[se] + t);
                            r = NODE_HERE;
                        } else if (((b0 >> t) & 1) && q == (b0 >> t) - 1) {
                            src = a.peaks + 5 * (jb.swbf_peaks + peak_of_height(b0, t));
                            r = NODE_HERE;
                        } else {
                            r = NODE_MISSING;
                        }
                    }
                }
                if (r != NODE_HERE) {
                    src = nullptr;
                    u.err[w] = 1;
                }
            }
#pragma unroll
            for (int q = 0; q < 5; ++q) dst[q] = src ? src[q] : 0ull;
        }
    }
}

__global__ void __launch_bounds__(256) k_ms_wit_chunks(MsApplyDev a, MsUpdateDev u, size_t entries) {
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
        const uint32_t* old = nullptr;
        uint64_t n_old = 0, s0 = 0, s1 = 0;
        uint32_t bias = 0;
        JobIndices ix{nullptr, nullptr, nullptr};
        if (ok) {
            const uint32_t j = u.wit_job[w];
            const MsApplyJob& jb = a.jobs[j];
            const MsJobScratch s(jb.aocl_n, jb.k);
            ix = JobIndices{a.rec.minimum + 2 * jb.rec_off, a.rec.distances + MSK_NUM_TRIALS * jb.rec_off,
                            a.idx_perm + MSK_NUM_TRIALS * jb.rec_off};
            const uint64_t* aux = a.aux + 2 * jb.grp_off;
            const uint32_t* grp = a.grp + jb.grp_off + j;
            const uint64_t T1 = lb_group(aux, jb.n_grp, 0, s.b1);
            const uint64_t g = lb_group(aux, T1, 0, c);
            if (g < T1 && aux[2 * g + 1] == c) {
                s0 = grp[g];
                s1 = grp[g + 1];
            }
            if (c < s.b0) {
                const uint64_t se = u.o_ent_src[e];
                if (se == MSA_NONE) {
                    ok = false;  // not reached: the witness was admitted
                } else {
                    old = u.ch.rel + u.ch.rel_off[se];
                    n_old = u.ch.rel_off[se + 1] - u.ch.rel_off[se];
                }
            } else if (c - s.b0 < MSK_WINDOW_CHUNKS) {
                const uint32_t* act = a.active + jb.act_off;
                const uint64_t cc = c - s.b0;
                const uint64_t la = lb_u32(act, jb.n_active, cc << MSK_CHUNK_BITS);
                old = act + la;
                n_old = lb_u32(act, jb.n_active, (cc + 1) << MSK_CHUNK_BITS) - la;
                bias = (uint32_t)(cc << MSK_CHUNK_BITS);
            }
            if (ok && n_old + (s1 - s0) != len) ok = false;  // the plan counted otherwise
            if (!ok && lane == 0) u.err[w] = 1;
        }
        if (lane == 0) u.o_chunk_index[e] = ok ? c : 0ull;
        if (!ok) {
            for (uint64_t p = lane; p < len; p += LANES) dst[p] = 0;
            continue;
        }
        const uint32_t in_chunk = (1u << MSK_CHUNK_BITS) - 1;
        // an old word goes behind the inserted words below it, an inserted word behind the old words up to it
        for (uint64_t p = lane; p < n_old; p += LANES) {
            const uint32_t va = old[p] - bias;
            uint64_t lo = s0, hi = s1;
            while (lo < hi) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if (((uint32_t)ix.at(mid) & in_chunk) < va) lo = mid + 1;
                else hi = mid;
            }
            const uint64_t pos = p + (lo - s0);
            if (pos < len) dst[pos] = va;
        }
        for (uint64_t s = s0 + lane; s < s1; s += LANES) {
            const uint32_t vb = (uint32_t)ix.at(s) & in_chunk;
            const uint64_t pos = (s - s0) + lb_u32(old, n_old, (uint64_t)vb + 1 + bias);
            if (pos < len) dst[pos] = vb;
        }
    }
}

__global__ void __launch_bounds__(256) k_ms_wit_seal(MsUpdateDev u, size_t witnesses) {
    for (size_t w = blockIdx.x * (size_t)blockDim.x + threadIdx.x; w < witnesses; w += (size_t)gridDim.x * blockDim.x) {
        if (!u.err[w]) continue;
        u.status[w] = NHIP_MS_UPDATE_INTERNAL;
        for (uint64_t d = 5 * u.o_aocl_path_off[w]; d < 5 * u.o_aocl_path_off[w + 1]; ++d) u.o_aocl_path[d] = 0;
        const uint64_t ebeg = u.o_entry_off[w], eend = u.o_entry_off[w + 1];
        for (uint64_t e = ebeg; e < eend; ++e) u.o_chunk_index[e] = 0;
        for (uint64_t d = 5 * u.o_path_off[ebeg]; d < 5 * u.o_path_off[eend]; ++d) u.o_path[d] = 0;
        for (uint64_t d = u.o_rel_off[ebeg]; d < u.o_rel_off[eend]; ++d) u.o_rel[d] = 0;
    }
}

hipError_t launch_ms_wit_admit(const MsApplyDev& a, const MsUpdateDev& u, size_t witnesses, hipStream_t st) {
    return ms_launch(k_ms_wit_admit, witnesses, st, a, u, witnesses);
}

hipError_t launch_ms_wit_paths(const MsApplyDev& a, const MsUpdateDev& u, size_t witnesses, size_t entries, hipStream_t st) {
    return ms_launch(k_ms_wit_paths, 8 * (witnesses + entries), st, a, u, witnesses, entries);  // 8 lanes per path
}

hipError_t launch_ms_wit_chunks(const MsApplyDev& a, const MsUpdateDev& u, size_t entries, hipStream_t st) {
    return ms_launch(k_ms_wit_chunks, 8 * entries, st, a, u, entries);  // 8 lanes per entry
}

hipError_t launch_ms_wit_seal(const MsUpdateDev& u, size_t witnesses, hipStream_t st) {
    return ms_launch(k_ms_wit_seal, witnesses, st, u, witnesses);
}

}  // namespace nhip
