// Host plan of RemovalRecordList::try_unpack (block rule 2.a): everything of
// removal_record_list.rs:548-883 that needs no hash.  Per job (one packed Vec<RemovalRecord>) it scans the
// dictionaries, checks and bit-unpacks the chunks (chunk.rs:197-304), estimates the leaf count, runs the three
// consistency checks and the per-tree length assert, and, for a job that passes, lays out the unpacked records'
// shape and a device program (ms_unpack_kernels.hip) that fills in their path digests: a slot arena with one
// 5-word slot per known node, the distinct chunks with their leaf slots, the structure-digest copies, the parent
// ops grouped by height above the leaves, and the source slot of every output path digest.  Every status is
// decided here; the host hashes nothing.  Host only (no HIP), so that tests/native/ms_unpack_plan_check.cpp links
// it under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/neptune_hip.h"
#include "ms_shape.hpp"

namespace nhip {

// The packed input: jobs as CSR over records, the records' index sets, and their dictionaries with chunk_index
// holding the key, path the authentication structure and rel the packed words.
struct MsPackedIn {
    const uint64_t* rec_off;
    size_t n_jobs;
    const uint64_t* minimum;
    const uint32_t* distances;
    const nhip_ms_chunks* chunks;
};
struct MsUnpackCounts {
    uint64_t records = 0;
    MsChunkCounts chunks;
};
// rec_off CSR over the jobs, the index arrays present when there is a record, the dictionaries as ms_chunks_ok
int ms_packed_ok(const MsPackedIn& in, MsUnpackCounts* counts);

// Chunk::try_unpack's checks on the packed words of one chunk: NHIP_MS_OK and the number of indices, or the
// chunk error's status
uint8_t ms_packed_chunk_ok(const uint32_t* words, uint64_t n_words, uint32_t* n_indices);
// index i of a packed chunk: the 12-bit field i + 1 of the big-endian bit string
inline uint32_t ms_packed_field(const uint32_t* words, uint32_t i) {
    const uint32_t bit = 12 * (i + 1), w = bit >> 5, off = bit & 31;
    if (off <= 20) return (words[w] >> (20 - off)) & 0xFFFu;
    return ((words[w] << (off - 20)) | (words[w + 1] >> (52 - off))) & 0xFFFu;
}

// One job's ranges in the program arrays (slots are global: the job's arena is slot_off .. slot_off + n_slots)
struct MsUnpackJob {
    uint64_t slot_off, n_slots;
    uint64_t leaf_off, n_leaf;
    uint64_t copy_off, n_copy;
    uint64_t lvl_off, n_levels;  // lvl[lvl_off .. lvl_off + n_levels]: starts of the levels in op (in ops)
    uint64_t gath_off, n_gath;   // = the job's digests in the unpacked path array
};
struct MsUnpackPlan {
    // per job
    std::vector<uint8_t> status;
    std::vector<uint64_t> num_leafs_aocl;  // the estimate; 0 for a failed job
    // the unpacked shape over all records (a failed job's records own no entry)
    std::vector<uint64_t> entry_off, chunk_index, path_off, rel_off;
    std::vector<uint32_t> rel;
    // the device program
    std::vector<MsUnpackJob> jobs;
    std::vector<uint32_t> leaf_slot, leaf_cnt;  // per distinct chunk: its slot, its number of indices
    std::vector<uint64_t> leaf_words;           // ... and its first packed word in the input's rel
    std::vector<uint32_t> copy_slot;            // structure digest copy_src of the input's path -> slot
    std::vector<uint64_t> copy_src;
    std::vector<uint32_t> op;                   // 3 per op: dst, left, right
    std::vector<uint64_t> lvl;
    std::vector<uint32_t> gath_src;             // per unpacked path digest
    uint64_t n_slots = 0;
    uint32_t max_levels = 0;
};
// in: as ms_packed_ok accepts it.  NHIP_OK, or NHIP_ERR_OOM when the arena would pass 2^32 slots; may throw
// std::bad_alloc.
int ms_unpack_plan(const MsPackedIn& in, const MsUnpackCounts& counts, MsUnpackPlan* plan);

// The node indices of the authentication structure of `leaves` (sorted, distinct, < 2^height) in a Merkle tree
// of that height: the siblings on the leaves' paths that cannot be computed from them, by descending node index
// (the convention of oracle/stark_ref.py:292-302; twenty-first is not pinned: DESIGN.md §4).
void ms_auth_structure_nodes(uint32_t height, const std::vector<uint64_t>& leaves, std::vector<uint64_t>* nodes);

// nhip_ms_unpack_plan / nhip_ms_unpack_batch: the output struct's shape (count pass: every array but status and
// num_leafs_aocl null; fill: all present but, for the plan, path), then write totals and, when filling, the arrays
bool ms_unpacked_is_count_pass(const nhip_ms_unpacked* out);
int ms_unpacked_write(const MsUnpackPlan& plan, size_t n_jobs, bool need_path, nhip_ms_unpacked* out);

}  // namespace nhip
