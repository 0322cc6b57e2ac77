// Batched mutator-set updates: Block::validate rules 2.b-2.e
// (protocol/consensus/block/mod.rs:816-849) and Block::mutator_set_accumulator_after (mod.rs:369-378)
// for many independent jobs, each (msa_before, addition records, removal records, optional expected
// accumulator).  The end state is computed directly, not record by record.
//
//  k_ms_chunk_auth_jobs : k_ms_chunk_auth with the entry's job looked up (MsChunkAuthJobsDev: entry -> owner -> job,
//                         the owners the block's records or nhip_ms_update_batch's witnesses): the same
//                         ms_chunk_auth_entry against that job's swbf_inactive.
//  k_ms_records_jobs    : k_ms_records with the record's job looked up (ms_record_decide), which also
//                         leaves one byte per index: set in msa_before or not.
//  k_ms_apply           : one 256-thread workgroup per job, every phase strided over the job's items with
//                         barriers between them; scratch in global memory (MsJobScratch), so a job of any size runs.
//                           1  consistency of msa_before
//                           2  the first record k_ms_records_jobs rejected (2.b)
//                           3  equal neighbours in the host's order of the records (2.c)
//                           4  per record: every index set before, or met in an earlier record (2.d)
//                           5  AOCL append; Tip5::hash of every touched and every new chunk, absorbed from
//                              the two sorted lists it merges; the level-synchronous leaf mutation; SWBF
//                              append; the window after; the comparison with the expected accumulator (2.e)
//
// The host stages order only (csrc/ms_shape.cpp): each job's active window sorted, its 45 m index slots
// sorted by (index, record) with the starts of the runs of one chunk index, and its records sorted by
// their index arrays.  The device recomputes every index from minimum + distance and takes every
// decision; a wrong order could only make it miss a duplicate or hash a wrong chunk.
//
// MMR append (block_mmr_append): the appended leaves sit at positions [n, n + cnt).  Level by level
// the aligned subtrees wholly inside that range are reduced in parallel (node q of level L covers
// [q 2^L, (q + 1) 2^L)); a level's first node with an odd index and last node with an even index have
// no partner in the range and are kept (64 x 2 digests in LDS).  One lane then merges along the left
// edge: a carry subtree that contains position n absorbs the old peak of its height when n has that
// bit, else the kept odd node of that level, until neither exists: at most 64 dependent hash_pairs.
// The peaks of n + cnt are old peaks (wholly below n), kept even nodes (wholly above) and that carry.
// Peak order (tallest first) and the merge of equal heights restate util_types/archival_mmr.rs.
#include "ms_device.hpp"

namespace nhip {

namespace {

// Appends cnt leaves (canonical digests, global) to the MMR (peaks_in, n); n + cnt does not wrap.
// scratch: room for cnt digests.  out: 64 digests; returns the number of peaks.  Called by the whole
// workgroup; orph: 2 x 64 x 5 words of LDS.  Ends behind a barrier.
// REC (nhip_ms_update_batch): the nodes along the left edge are kept as well, the one of height
// h (it holds position n and leaves on both sides of it) in carry[5 h ..] with bit h of *carry_mask set; the
// nodes wholly inside the range stay in scratch, level after level from height 1 on, as they always did.
template <bool REC>
__device__ uint32_t block_mmr_append(const uint64_t* peaks_in, uint64_t n, const uint64_t* leaves, uint64_t cnt,
                                     uint64_t* scratch, uint64_t* out, uint64_t (*orph)[64][5],
                                     const uint8_t* __restrict__ lut, uint64_t* carry = nullptr,
                                     uint64_t* carry_mask = nullptr) {
    const uint32_t tid = threadIdx.x;
    const uint64_t n1 = n + cnt;
    {
        const uint64_t* cur = leaves;
        uint64_t* nxt = scratch;
        uint64_t lo = n, hi = n1;
        for (uint32_t L = 0; L < 64 && hi > lo; ++L) {
            const uint64_t cnt_l = hi - lo;
            if (tid < 5) {
                if (lo & 1) orph[0][L][tid] = cur[tid];
                if (hi & 1) orph[1][L][tid] = cur[5 * (cnt_l - 1) + tid];
            }
            const uint64_t lo2 = (lo >> 1) + (lo & 1), hi2 = hi >> 1;
            const uint64_t cnt2 = hi2 > lo2 ? hi2 - lo2 : 0;
            const uint64_t first = 2 * lo2 - lo;  // 0 or 1
            for (uint64_t q = tid; q < cnt2; q += blockDim.x)
                dig_hp(cur + 5 * (first + 2 * q), cur + 5 * (first + 2 * q + 1), nxt + 5 * q, lut);
            __syncthreads();
            cur = nxt;
            nxt += 5 * cnt2;
            lo = lo2;
            hi = hi2;
        }
    }
    __syncthreads();
    uint32_t np = (uint32_t)__popcll(n1);
    if (tid == 0) {
        uint64_t c[5] = {0, 0, 0, 0, 0};
        bool have_c = false, done = false;
        uint64_t kept = 0;
        for (uint32_t L = 0; L < 64 && !done; ++L) {
            const bool a_bit = (n >> L) & 1;
            const uint64_t low = L ? (n & ((1ull << L) - 1)) : 0;
            const uint64_t lo_l = (n >> L) + (low != 0), hi_l = n1 >> L;
            const bool have_new = (lo_l & 1) && lo_l < hi_l;
            const uint64_t* left = nullptr;
            const uint64_t* right = nullptr;
            if (!have_c) {
                if (a_bit) {
                    if (have_new) {
                        left = peaks_in + 5 * (size_t)peak_of_height(n, L);
                        right = orph[0][L];
                    } else {
                        done = true;
                    }
                }
            } else if (a_bit) {
                left = peaks_in + 5 * (size_t)peak_of_height(n, L);
                right = c;
            } else if (have_new) {
                left = c;
                right = orph[0][L];
            } else {
                done = true;
            }
            if (left) {
                uint64_t t[5];
                dig_hp(left, right, t, lut);
#pragma unroll
                for (int k = 0; k < 5; ++k) c[k] = t[k];
                have_c = true;
                if (REC && L + 1 < 64) {
#pragma unroll
                    for (int k = 0; k < 5; ++k) carry[5 * (size_t)(L + 1) + k] = t[k];
                    kept |= 1ull << (L + 1);
                }
            }
        }
        if (REC) *carry_mask = kept;
        uint32_t w = 0;
        for (int h = 63; h >= 0; --h) {
            if (!((n1 >> h) & 1)) continue;
            const uint64_t start = h == 63 ? 0 : ((n1 >> (h + 1)) << (h + 1));
            const uint64_t end = start + (1ull << h);
            const uint64_t* src = c;
            if (end <= n) src = peaks_in + 5 * (size_t)peak_of_height(n, (uint32_t)h);
            else if (start >= n) src = orph[1][h];
#pragma unroll
            for (int k = 0; k < 5; ++k) out[5 * (size_t)w + k] = src[k];
            ++w;
        }
    }
    __syncthreads();
    return np;
}

}  // namespace

__global__ void __launch_bounds__(256) k_ms_chunk_auth_jobs(MsChunkAuthJobsDev c, size_t entries) {
    __shared__ Tip5Lds t5;
    tip5_lds_init(t5);
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < entries; e += (size_t)gridDim.x * blockDim.x) {
        const MsApplyJob& jb = c.jobs[c.owner_job[c.entry_owner[e]]];
        const MmrDev swbf{c.peaks + 5 * jb.swbf_peaks, jb.swbf_np, jb.swbf_n};
        c.auth[e] = ms_chunk_auth_entry(c.ch, e, swbf, t5.lut) ? 1 : 0;
    }
}

__global__ void __launch_bounds__(256) k_ms_records_jobs(MsApplyDev a, size_t n) {
    const uint32_t lane = threadIdx.x & 63u;
    const size_t wave = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6;
    const size_t n_waves = ((size_t)gridDim.x * blockDim.x) >> 6;
    for (size_t i = wave; i < n; i += n_waves) {  // wave-uniform
        const MsApplyJob& jb = a.jobs[a.rec_job[i]];
        ms_record_decide(a.rec, i, lane, a.active + jb.act_off, jb.n_active, jb.aocl_n, a.index_set);
    }
}

// REC: the nodes a witness of the job may need after the block are kept: both appends' left
// edges in a.carry, and every level of the leaf mutation (level L of group g at MsJobScratch::mut_node(n_grp, L, g)) where
// the plain form swaps two buffers.  Nothing else differs, and the plain form compiles to what it was.
template <bool REC>
__global__ void __launch_bounds__(256) k_ms_apply(MsApplyDev a, size_t n_jobs) {
    __shared__ Tip5Lds t5;
    __shared__ uint64_t sh_orph[2][64][5];
    __shared__ uint64_t sh_peaks[64][5];
    __shared__ unsigned long long sh_min;
    __shared__ uint32_t sh_flag;
    tip5_lds_init(t5);
    const uint32_t tid = threadIdx.x;
    for (size_t j = blockIdx.x; j < n_jobs; j += gridDim.x) {  // workgroup-uniform
        const MsApplyJob jb = a.jobs[j];
        const MsJobScratch s(jb.aocl_n, jb.k);
        const uint64_t n0 = s.n0, k = jb.k, n1 = s.n1, b0 = s.b0, b1 = s.b1, m = jb.m;
        const uint64_t n_idx = MSK_NUM_TRIALS * m;
        const JobIndices ix{a.rec.minimum + 2 * jb.rec_off, a.rec.distances + MSK_NUM_TRIALS * jb.rec_off,
                            a.idx_perm + MSK_NUM_TRIALS * jb.rec_off};
        const uint32_t* act = a.active + jb.act_off;
        uint8_t status = NHIP_MS_OK;
        uint64_t bad = MSA_NONE;

        // 1. consistency
        if ((uint32_t)__popcll(n0) != jb.aocl_np || (uint32_t)__popcll(jb.swbf_n) != jb.swbf_np || jb.swbf_n != b0 ||
            s.wrapped())
            status = NHIP_MS_INCONSISTENT;

        // 2. rule 2.b: the first record k_ms_records_jobs rejected
        if (status == NHIP_MS_OK && m) {
            if (tid == 0) sh_min = MSA_NONE;
            __syncthreads();
            for (uint64_t r = tid; r < m; r += blockDim.x)
                if (a.rec.status[jb.rec_off + r] != NHIP_MS_OK) atomicMin(&sh_min, (unsigned long long)r);
            __syncthreads();
            if (sh_min != MSA_NONE) {
                bad = sh_min;
                status = a.rec.status[jb.rec_off + bad];
            }
            __syncthreads();
        }

        // 3. rule 2.c: records with equal index arrays are neighbours in rec_perm (stable order)
        if (status == NHIP_MS_OK && m > 1) {
            if (tid == 0) sh_min = MSA_NONE;
            __syncthreads();
            const uint32_t* rp = a.rec_perm + jb.rec_off;
            for (uint64_t s = 1 + tid; s < m; s += blockDim.x) {
                const uint32_t ra = rp[s - 1], rb = rp[s];
                const u128 ma = ((u128)ix.mn[2 * (size_t)ra + 1] << 64) | ix.mn[2 * (size_t)ra];
                const u128 mb = ((u128)ix.mn[2 * (size_t)rb + 1] << 64) | ix.mn[2 * (size_t)rb];
                bool eq = true;
                for (uint32_t t = 0; t < MSK_NUM_TRIALS && eq; ++t)
                    eq = ma + ix.dist[(size_t)MSK_NUM_TRIALS * ra + t] == mb + ix.dist[(size_t)MSK_NUM_TRIALS * rb + t];
                if (eq) atomicMin(&sh_min, (unsigned long long)(ra > rb ? ra : rb));
            }
            __syncthreads();
            if (sh_min != MSA_NONE) {
                bad = sh_min;
                status = NHIP_MS_DUPLICATE_RECORD;
            }
            __syncthreads();
        }

        // 4. rule 2.d: a record fails when every index is set before or occurs in an earlier record
        if (status == NHIP_MS_OK && m) {
            if (tid == 0) sh_min = MSA_NONE;
            __syncthreads();
            const uint8_t* set = a.index_set + MSK_NUM_TRIALS * jb.rec_off;
            for (uint64_t r = tid; r < m; r += blockDim.x) {
                const u128 mr = ((u128)ix.mn[2 * r + 1] << 64) | ix.mn[2 * r];
                bool all = true;
                for (uint32_t t = 0; t < MSK_NUM_TRIALS && all; ++t) {
                    if (set[MSK_NUM_TRIALS * r + t]) continue;
                    uint32_t first_rec = 0;
                    // the first slot with this index belongs to the earliest record that has it
                    (void)ix.at(ix.lower_bound(0, n_idx, mr + ix.dist[MSK_NUM_TRIALS * r + t]), &first_rec);
                    all = first_rec < r;
                }
                if (all) atomicMin(&sh_min, (unsigned long long)r);
            }
            __syncthreads();
            if (sh_min != MSA_NONE) {
                bad = sh_min;
                status = NHIP_MS_UPDATE_IMPOSSIBLE;
            }
            __syncthreads();
        }

        uint64_t* o_aocl = a.out_peaks + j * 64 * 5;
        uint64_t* o_swbf = a.out_peaks + (n_jobs + j) * 64 * 5;
        uint32_t* o_act = a.out_active + jb.win_off;
        uint64_t n_out = 0;
        uint32_t np_aocl = 0, np_swbf = 0;
        if (status == NHIP_MS_OK) {
            // 5. the accumulator after
            uint64_t* dig = a.dig + 5 * jb.dig_off;  // the job's scratch: MsJobScratch (ms_shape.hpp)
            uint64_t* d_new = dig + 5 * s.fresh();  // the new chunks' digests, then their levels
            uint64_t* d_mut = dig + 5 * s.mut();    // the touched leaves, level by level
            uint64_t* aux = a.aux + 2 * jb.grp_off;
            const uint32_t* grp = a.grp + jb.grp_off + j;  // n_grp + 1 starts per job
            const uint64_t n_grp = jb.n_grp;

            np_aocl = block_mmr_append<REC>(a.peaks + 5 * jb.aocl_peaks, n0, a.additions + 5 * jb.add_off, k, dig + 5 * s.aocl(),
                                            o_aocl, sh_orph, t5.lut, REC ? a.carry + j * 2 * 64 * 5 : nullptr,
                                            REC ? a.carry_mask + 2 * j : nullptr);

            // the groups' chunk indices; touched: [0, T), new chunks: [T, T1), still active: [T1, n_grp)
            for (uint64_t g = tid; g < n_grp; g += blockDim.x) aux[2 * g + 1] = (uint64_t)(ix.at(grp[g]) >> MSK_CHUNK_BITS);
            __syncthreads();
            const uint64_t T = lb_group(aux, n_grp, 0, b0), T1 = lb_group(aux, n_grp, 0, b1);

            // Tip5::hash of every touched chunk (old content: its dictionary entry) and of every new chunk
            // (old content: its part of the window), merged with the inserted indices as they are absorbed
            for (uint64_t i = tid; i < T + s.slides; i += blockDim.x) {
                const uint32_t* old = nullptr;
                uint64_t n_old = 0, s0 = 0, s1 = 0;
                uint32_t bias = 0;
                uint64_t* dst;
                if (i < T) {
                    uint32_t rec = 0;
                    s0 = grp[i];
                    s1 = grp[i + 1];
                    (void)ix.at(s0, &rec);
                    const uint64_t ci = aux[2 * i + 1], grec = jb.rec_off + rec;
                    uint64_t e = a.rec.ch.entry_off[grec];
                    const uint64_t eend = a.rec.ch.entry_off[grec + 1];
                    while (e < eend && a.rec.ch.chunk_index[e] != ci) ++e;
                    if (e == eend) e = MSA_NONE;  // not reached: the record validated
                    aux[2 * i] = e;
                    if (e != MSA_NONE) {
                        old = a.rec.ch.rel + a.rec.ch.rel_off[e];
                        n_old = a.rec.ch.rel_off[e + 1] - a.rec.ch.rel_off[e];
                    }
                    dst = d_mut + 5 * i;
                } else {
                    const uint64_t c = i - T;
                    if (c < MSK_WINDOW_CHUNKS) {
                        const uint64_t la = lb_u32(act, jb.n_active, c << MSK_CHUNK_BITS);
                        old = act + la;
                        n_old = lb_u32(act, jb.n_active, (c + 1) << MSK_CHUNK_BITS) - la;
                        bias = (uint32_t)(c << MSK_CHUNK_BITS);
                    }
                    const uint64_t g = lb_group(aux, T1, 0, b0 + c);
                    if (g < T1 && aux[2 * g + 1] == b0 + c) {
                        s0 = grp[g];
                        s1 = grp[g + 1];
                    }
                    dst = d_new + 5 * c;
                }
                uint64_t ia = 0, ib = s0;
                uint32_t vb = ib < s1 ? (uint32_t)ix.at(ib) & ((1u << MSK_CHUNK_BITS) - 1) : ~0u;
                uint64_t run[5];
                ms_chunk_sponge(
                    n_old + (s1 - s0),
                    [&](uint64_t) {
                        const uint32_t va = ia < n_old ? old[ia] - bias : ~0u;
                        if (va <= vb) {
                            ++ia;
                            return va;
                        }
                        const uint32_t v = vb;
                        ++ib;
                        vb = ib < s1 ? (uint32_t)ix.at(ib) & ((1u << MSK_CHUNK_BITS) - 1) : ~0u;
                        return v;
                    },
                    run, t5.lut);
#pragma unroll
                for (int q = 0; q < 5; ++q) dst[q] = from_mont(run[q]);
            }
            __syncthreads();

            // leaf mutation, level-synchronous: a touched leaf's sibling at a level is another touched
            // leaf's node (the new value) or the digest of its own path
            uint64_t* cur = d_mut;
            uint64_t* nxt = dig + 5 * s.mut_node(n_grp, 1, 0);
            const uint32_t max_h = b0 ? 63u - (uint32_t)__clzll((long long)b0) : 0u;
            for (uint32_t L = 0; L < max_h && T; ++L) {
                for (uint64_t g = tid; g < T; g += blockDim.x) {
                    const uint64_t ci = aux[2 * g + 1];
                    const uint32_t h = 63u - (uint32_t)__clzll((long long)(ci ^ b0));
                    if (L < h) {
                        const uint64_t node = ci >> L, sib = node ^ 1ull;
                        const uint64_t x = lb_group(aux, T, L, sib);
                        const uint64_t e = aux[2 * g];
                        const uint64_t* sd = cur + 5 * g;  // e == MSA_NONE is not reached
                        if (x < T && (aux[2 * x + 1] >> L) == sib) sd = cur + 5 * x;
                        else if (e != MSA_NONE) sd = a.rec.ch.path + 5 * (a.rec.ch.path_off[e] + L);  // path_len == h: authenticated
                        if (node & 1) dig_hp(sd, cur + 5 * g, nxt + 5 * g, t5.lut);
                        else dig_hp(cur + 5 * g, sd, nxt + 5 * g, t5.lut);
                    } else {
#pragma unroll
                        for (int q = 0; q < 5; ++q) nxt[5 * g + q] = cur[5 * g + q];
                    }
                }
                __syncthreads();
                if (REC) {
                    cur = nxt;
                    nxt += 5 * s.mut_stride(n_grp);
                } else {
                    uint64_t* t = cur;
                    cur = nxt;
                    nxt = t;
                }
            }
            // the peaks of swbf_inactive after the mutation
            if (tid < jb.swbf_np) {
                uint32_t seen = 0, h = 0;
                for (int b = 63; b >= 0; --b)
                    if ((b0 >> b) & 1) {
                        if (seen == tid) {
                            h = (uint32_t)b;
                            break;
                        }
                        ++seen;
                    }
                const uint64_t start = h == 63 ? 0 : ((b0 >> (h + 1)) << (h + 1));
                const uint64_t x = lb_group(aux, T, 0, start);
                const uint64_t* src = x < T && aux[2 * x + 1] - start < (1ull << h)
                                          ? cur + 5 * x
                                          : a.peaks + 5 * (jb.swbf_peaks + tid);
#pragma unroll
                for (int q = 0; q < 5; ++q) sh_peaks[tid][q] = src[q];
            }
            __syncthreads();
            np_swbf = block_mmr_append<REC>(&sh_peaks[0][0], b0, d_new, s.slides, dig + 5 * s.fresh_levels(), o_swbf, sh_orph, t5.lut,
                                            REC ? a.carry + (j * 2 + 1) * 64 * 5 : nullptr,
                                            REC ? a.carry_mask + 2 * j + 1 : nullptr);

            // the window after: the old indices past the slid chunks, shifted down, merged with the inserted ones
            const bool all_slid = s.slides >= MSK_WINDOW_CHUNKS;
            const uint64_t shift = all_slid ? 0 : s.slides << MSK_CHUNK_BITS;
            const uint64_t la = all_slid ? jb.n_active : lb_u32(act, jb.n_active, shift);
            const uint64_t kept = jb.n_active - la;
            const uint64_t s_ins = n_grp ? grp[T1] : 0;  // grp[n_grp] = n_idx
            const u128 base = (u128)b1 << MSK_CHUNK_BITS;
            n_out = kept + (n_idx - s_ins);
            for (uint64_t p = tid; p < kept; p += blockDim.x) {
                const uint32_t v = act[la + p] - (uint32_t)shift;
                const uint64_t pos = p + (ix.lower_bound(s_ins, n_idx, base + v) - s_ins);
                if (pos < jb.win_cap) o_act[pos] = v;
            }
            for (uint64_t s = s_ins + tid; s < n_idx; s += blockDim.x) {
                const uint32_t v = (uint32_t)(ix.at(s) - base);  // < 2^20: at most chunk b0 + 255
                const uint64_t le = all_slid ? 0 : lb_u32(act, jb.n_active, (uint64_t)v + shift + 1) - la;
                const uint64_t pos = (s - s_ins) + le;
                if (pos < jb.win_cap) o_act[pos] = v;
            }
            __syncthreads();

            // rule 2.e
            if (a.has_expected) {
                if (tid == 0) sh_flag = 0;
                __syncthreads();
                bool diff = jb.exp_aocl_n != n1 || jb.exp_swbf_n != b1 || jb.exp_aocl_np != np_aocl ||
                            jb.exp_swbf_np != np_swbf || jb.exp_n_active != n_out;
                if (!diff) {
                    const uint64_t* ea = a.peaks + 5 * jb.exp_aocl_peaks;
                    const uint64_t* es = a.peaks + 5 * jb.exp_swbf_peaks;
                    for (uint32_t w = tid; w < 5 * np_aocl; w += blockDim.x) diff |= ea[w] != o_aocl[w];
                    for (uint32_t w = tid; w < 5 * np_swbf; w += blockDim.x) diff |= es[w] != o_swbf[w];
                    const uint32_t* ew = a.exp_active + jb.exp_act_off;
                    for (uint64_t w = tid; w < n_out && w < jb.win_cap; w += blockDim.x) diff |= ew[w] != o_act[w];
                }
                if (diff) sh_flag = 1;
                __syncthreads();
                if (sh_flag) status = NHIP_MS_UPDATE_MISMATCH;
                __syncthreads();
            }
        }
        if (tid == 0) {
            a.verdict[j] = status == NHIP_MS_OK ? 1 : 0;
            a.status[j] = status;
            a.bad[j] = bad;
            const bool have = status == NHIP_MS_OK || status == NHIP_MS_UPDATE_MISMATCH;
            a.out_np[j] = have ? np_aocl : 0;
            a.out_np[n_jobs + j] = have ? np_swbf : 0;
            a.out_n[j] = have ? n1 : 0;
            a.out_n[n_jobs + j] = have ? b1 : 0;
            a.out_n[2 * n_jobs + j] = have ? n_out : 0;
        }
        __syncthreads();
    }
}

hipError_t launch_ms_chunk_auth_jobs(const MsChunkAuthJobsDev& c, size_t entries, hipStream_t st) {
    return ms_launch(k_ms_chunk_auth_jobs, entries, st, c, entries);
}

hipError_t launch_ms_records_jobs(const MsApplyDev& a, size_t n_records, hipStream_t st) {
    return ms_launch(k_ms_records_jobs, 64 * n_records, st, a, n_records);  // a wave per record
}

hipError_t launch_ms_apply(const MsApplyDev& a, size_t n_jobs, hipStream_t st, bool keep_nodes) {
    if (n_jobs == 0) return hipSuccess;
    const dim3 grid((unsigned)(n_jobs > 65536 ? 65536 : n_jobs));
    if (keep_nodes) hipLaunchKernelGGL(k_ms_apply<true>, grid, dim3(256), 0, st, a, n_jobs);
    else hipLaunchKernelGGL(k_ms_apply<false>, grid, dim3(256), 0, st, a, n_jobs);
    return hipGetLastError();
}

}  // namespace nhip
