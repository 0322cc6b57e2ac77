// Host side of the mutator-set entry points (nhip_mmr_verify_batch, nhip_ms_can_remove_batch,
// nhip_ms_verify_batch, nhip_ms_apply_batch): shape checks, the only thing the host decides about their inputs,
// and the order it stages besides the caller's own arrays.  Every verdict is the
// device's; the host refuses (NHIP_ERR_ARG) what it could not stage without reading outside the
// caller's arrays: a null pointer with a non-zero count, an offset array that does not start at 0
// or decreases, and totals whose byte size leaves size_t.  Plain C++ (no HIP header; MsJobScratch alone is also the
// kernels'), so that tests/native/ms_shape_check.cpp and ms_apply_shape_check.cpp link it under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/neptune_hip.h"

#ifdef __HIP__
#define NHIP_MS_HD __host__ __device__ inline
#else
#define NHIP_MS_HD inline
#endif

namespace nhip {

// off[0..n]: off[0] == 0, non-decreasing, and off[n] * unit_bytes fits size_t.  *total = off[n].
int ms_csr_ok(const uint64_t* off, size_t n, size_t unit_bytes, uint64_t* total);

// peaks present when n_peaks != 0
int ms_mmr_ok(const nhip_mmr* mmr);
// both MMRs, and the active window's list present when n_active != 0
int ms_msa_ok(const nhip_msa* msa);

// n (leaf, path) items: path_off covers n paths, path present when it holds any digest
int ms_paths_ok(const uint64_t* path_off, const uint64_t* path, size_t n, uint64_t* path_digests);

struct MsChunkCounts {
    uint64_t entries = 0, path_digests = 0, rel_words = 0;
};
// the flattened chunk dictionaries of n records: entry_off covers the records, path_off and rel_off
// cover the entry_off[n] entries, and every array that has an element is present
int ms_chunks_ok(const nhip_ms_chunks* chunks, size_t n, MsChunkCounts* counts);

struct MsApplyCounts {
    uint64_t additions = 0, records = 0, window_cap = 0;
    MsChunkCounts chunks;
    bool accumulators = false;  // the accumulators after are asked for
};
// nhip_ms_apply_batch: both structs and every per-job array present, add_off / rec_off / active_off CSR over
// the jobs, every accumulator (before and expected) as ms_msa_ok, the records' arrays and dictionaries as
// ms_chunks_ok, at most (2^32 - 1) / 45 records in a job, the accumulator outputs all null or all present,
// and every job's window capacity >= n_active + 45 records.  Hashes nothing, decides nothing.
int ms_apply_ok(const nhip_ms_apply_in* in, const nhip_ms_apply_out* out, MsApplyCounts* counts);
// its input half alone (nhip_ms_update_plan has no nhip_ms_apply_out); counts->accumulators stays false
int ms_apply_in_ok(const nhip_ms_apply_in* in, MsApplyCounts* counts);

// ---- staged order: inputs that passed the checks above; hashes nothing, decides nothing;
// may throw std::bad_alloc

// Appends the accumulator's active window to pool and sorts what it appended (membership is order-free: the
// kernels search a sorted copy).
void ms_append_sorted_window(std::vector<uint32_t>& pool, const nhip_msa& msa);

// The 15 words (item, sender_randomness, receiver_preimage) of each of n records, record by record.
std::vector<uint64_t> ms_interleave15(const uint64_t* items, const uint64_t* sender_randomness,
                                      const uint64_t* receiver_preimages, size_t n);

// One job of nhip_ms_apply_batch as the host stages it and k_ms_apply reads it (ms_apply_kernels.hip): offsets
// into the pools of MsApplyDev (kernels.hpp; peaks and scratch in digests).
struct MsApplyJob {
    uint64_t aocl_n, swbf_n;          // msa_before: num_leafs
    uint64_t aocl_peaks, swbf_peaks;  // ... and its peak lists in the peaks pool
    uint64_t act_off, n_active;       // the sorted copy of its active window
    uint64_t add_off, k;              // addition records
    uint64_t rec_off, m;              // removal records (idx_perm: 45 rec_off; rec_perm: rec_off)
    uint64_t grp_off, n_grp;          // groups before this job; its n_grp + 1 starts are grp[grp_off + job ..]
    uint64_t dig_off;                 // its digest scratch (MsJobScratch below) in the dig pool
    uint64_t win_off, win_cap;        // the window after in out_active
    uint64_t exp_aocl_n, exp_swbf_n, exp_aocl_peaks, exp_swbf_peaks, exp_act_off, exp_n_active;
    uint32_t aocl_np, swbf_np, exp_aocl_np, exp_swbf_np;
};
// The bounds of a job and the layout of its digest scratch, in digests from dig_off: one definition for the host,
// which sizes the pool from it (ms_apply_order), and for k_ms_apply and the witness kernels, which address every
// node they keep or look up through it.  Three regions, back to back:
//   aocl  k + 1            block_mmr_append's levels over the addition records, height 1 first
//   fresh 2 slides + 1     the new chunks' digests, then (at fresh_levels) the levels of the SWBF append over them
//   mut   levels x n_grp   the leaf mutation, level L of touched chunk g at mut_node(n_grp, L, g): two levels that
//                          swap, or with keep_nodes one per height 0 .. ilog2(b0) + 1.  n_grp is an argument, not a
//                          member, so that a kernel loads it only on the path that needs it.
// n1 = aocl_n + k may wrap.  The host relies on slides = 0 then (no size follows a wrapped count).  The kernels rely
// on nothing for such a job: k_ms_apply tests wrapped() and answers NHIP_MS_INCONSISTENT before it touches the
// scratch, and the witness kernels skip a job that did not end NHIP_MS_OK.
struct MsJobScratch {
    static constexpr uint32_t BATCH_SIZE = 8;  // shared.rs:14
    uint64_t n0, n1, b0, b1;  // before and after: aocl.num_leafs, swbf_inactive.num_leafs (get_batch_index)
    uint64_t slides;          // b1 - b0 <= k / 8 + 1: the chunks that leave the window
    NHIP_MS_HD MsJobScratch(uint64_t aocl_n, uint64_t k)
        : n0(aocl_n), n1(aocl_n + k), b0(batch_index(n0)), b1(batch_index(n1)), slides(n1 < n0 ? 0 : b1 - b0) {}
    static NHIP_MS_HD uint64_t batch_index(uint64_t num_leafs) { return (num_leafs ? num_leafs - 1 : 0) / BATCH_SIZE; }
    NHIP_MS_HD bool wrapped() const { return n1 < n0; }
    NHIP_MS_HD uint64_t aocl() const { return 0; }
    NHIP_MS_HD uint64_t fresh() const { return (n1 - n0) + 1; }
    NHIP_MS_HD uint64_t fresh_levels() const { return fresh() + slides; }
    NHIP_MS_HD uint64_t mut() const { return fresh() + 2 * slides + 1; }
    static NHIP_MS_HD uint64_t mut_stride(uint64_t n_grp) { return n_grp; }  // one level
    NHIP_MS_HD uint64_t mut_node(uint64_t n_grp, uint64_t L, uint64_t g) const { return mut() + L * mut_stride(n_grp) + g; }
    NHIP_MS_HD uint64_t total(uint64_t n_grp, bool keep_nodes) const {
        uint64_t levels = keep_nodes ? 1 : 2;
        for (uint64_t b = keep_nodes ? b0 : 0; b; b >>= 1) ++levels;
        return mut() + levels * mut_stride(n_grp);
    }
};

// nhip_ms_apply_batch's staged arrays (MsApplyDev says what the kernels read in each): per job a sorted copy of
// its window, its index slots sorted by (index, slot) and grouped by chunk index, its records sorted by their
// index arrays (stable), and its offsets into every pool.
struct MsApplyOrder {
    std::vector<MsApplyJob> jobs;
    std::vector<uint64_t> peaks;
    std::vector<uint32_t> active, exp_active, rec_job, entry_rec, idx_perm, grp, rec_perm;
    uint64_t dig_total = 0, grp_total = 0, win_total = 0;
};
// keep_nodes: room for every level of the leaf mutation (k_ms_apply<true>, nhip_ms_update_batch)
void ms_apply_order(const nhip_ms_apply_in* in, const nhip_ms_apply_out* out, const MsApplyCounts& cnt,
                    MsApplyOrder* o, bool keep_nodes = false);

}  // namespace nhip
