// Shape checks of the mutator-set entry points (nhip_mmr_verify_batch, nhip_ms_can_remove_batch,
// nhip_ms_verify_batch, nhip_ms_apply_batch): the only thing the host decides about their inputs.  Every verdict is the
// device's; the host refuses (NHIP_ERR_ARG) what it could not stage without reading outside the
// caller's arrays: a null pointer with a non-zero count, an offset array that does not start at 0
// or decreases, and totals whose byte size leaves size_t.  Host only (no HIP), so that
// tests/native/ms_shape_check.cpp and ms_apply_shape_check.cpp link it under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/neptune_hip.h"

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

}  // namespace nhip
