// The integer decisions of a restore (nhip_ms_archive_restore_shape, nhip_ms_store_append_restored; DESIGN.md §6k,
// "The hand-over"), in a form that compiles for host and device: k_ms_rst_keys runs them per lane and
// tests/native/ms_restore_check.cpp runs them on the CPU against ms_archive_restore_plan, which stays the oracle.
// No __int128: an index is two u64 halves and an explicit carry.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ms_archive.hpp"

namespace nhip {

static constexpr uint32_t MS_RESTORE_TRIALS = 45;
static constexpr uint32_t MS_RESTORE_CHUNK_BITS = 12;
static constexpr uint64_t MS_RESTORE_WINDOW_CHUNKS = 1u << 8;
// the shape kernels' geometry (ms_restore_kernels.hip); include/neptune_hip.h names the same numbers for callers
static constexpr uint32_t MS_RESTORE_WAVES = NHIP_MS_RESTORE_WAVES;            // k_ms_rst_keys: witnesses per workgroup
static constexpr uint32_t MS_RESTORE_SCAN_WIDTH = NHIP_MS_RESTORE_SCAN_WIDTH;  // items per scan tile, one per lane
static constexpr uint32_t MS_RESTORE_CARRY_LANES = NHIP_MS_RESTORE_CARRY_LANES;  // lanes that carry across tiles

// minimum + distance as a chunk index.  False (*chunk untouched): the sum wraps u128, or its chunk index exceeds
// b + 255 (AbsoluteIndexSet::to_array saturates: fail closed).  b < 2^61, so b + 255 does not wrap.
NHIP_MS_HD bool ms_restore_chunk(uint64_t mn_lo, uint64_t mn_hi, uint32_t distance, uint64_t b, uint64_t* chunk) {
    const uint64_t lo = mn_lo + distance;
    const uint64_t carry = lo < mn_lo ? 1 : 0;
    const uint64_t hi = mn_hi + carry;
    if (hi < mn_hi) return false;  // the carry left the high word
    const uint64_t c_hi = hi >> MS_RESTORE_CHUNK_BITS;
    const uint64_t c_lo = (lo >> MS_RESTORE_CHUNK_BITS) | (hi << (64 - MS_RESTORE_CHUNK_BITS));
    if (c_hi != 0 || c_lo > b + (MS_RESTORE_WINDOW_CHUNKS - 1)) return false;
    *chunk = c_lo;
    return true;
}

// the first status: no such leaf (a leaf index other than MS_UPDATE_NONE at or past the leaf count, or no leaf at all)
NHIP_MS_HD bool ms_restore_not_in_aocl(uint64_t leaf_index, uint64_t aocl_leafs) {
    return aocl_leafs == 0 || (leaf_index != MS_UPDATE_NONE && leaf_index >= aocl_leafs);
}

// of a witness that passed ms_restore_not_in_aocl
NHIP_MS_HD uint32_t ms_restore_aocl_len(uint64_t leaf_index, uint64_t aocl_leafs) {
    return leaf_index == MS_UPDATE_NONE ? 0 : ms_arch_path_len(leaf_index, aocl_leafs);
}

// One witness, serially: its status and, when that is NHIP_MS_OK, its AOCL path length and its keys (the distinct
// chunk indices below b, ascending; at most 45).  What the 45 lanes of k_ms_rst_keys decide together.
NHIP_MS_HD uint8_t ms_restore_witness(uint64_t aocl_leafs, uint64_t mn_lo, uint64_t mn_hi, const uint32_t* distances,
                                      uint64_t leaf_index, uint32_t* aocl_len, uint64_t* keys, uint32_t* n_keys) {
    *aocl_len = 0;
    *n_keys = 0;
    if (ms_restore_not_in_aocl(leaf_index, aocl_leafs)) return NHIP_MS_NOT_IN_AOCL;
    const uint64_t b = MsJobScratch::batch_index(aocl_leafs);
    uint32_t nk = 0;
    for (uint32_t t = 0; t < MS_RESTORE_TRIALS; ++t) {
        uint64_t c;
        if (!ms_restore_chunk(mn_lo, mn_hi, distances[t], b, &c)) return NHIP_MS_OUT_OF_RANGE;
        if (c >= b) continue;
        uint32_t at = 0;  // insertion into the sorted distinct keys
        while (at < nk && keys[at] < c) ++at;
        if (at < nk && keys[at] == c) continue;
        for (uint32_t k = nk; k > at; --k) keys[k] = keys[k - 1];
        keys[at] = c;
        ++nk;
    }
    *n_keys = nk;
    *aocl_len = ms_restore_aocl_len(leaf_index, aocl_leafs);
    return NHIP_MS_OK;
}

}  // namespace nhip
