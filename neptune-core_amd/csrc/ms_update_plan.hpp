// Host plan of nhip_ms_update_batch: the shape of every witness after the block, which is an
// integer function of the inputs.  With n0 / n1 the AOCL leaf counts before / after a job and b0 / b1 its batch
// indices: a witness's AOCL path after has ilog2(l ^ n1) digests, its dictionary's keys are its chunk indices
// below b1 in ascending order, an entry's path has ilog2(key ^ b1) digests and its chunk has the old chunk's
// words (the first input entry with that key for key < b0, the slid part of the old window otherwise) plus the
// job's record indices in that chunk.  The shape is laid out as if every job and every witness were accepted; no
// status is decided here and nothing is hashed.  Besides the output's offset arrays the plan holds what the
// witness kernels (ms_update_kernels.hip) read to find their way: each witness's job, each input entry's witness,
// each output entry's witness and the input entry it continues.  Host only (no HIP), so that
// tests/native/ms_update_plan_check.cpp links it under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/neptune_hip.h"
#include "ms_shape.hpp"

namespace nhip {

static constexpr uint64_t MS_UPDATE_NONE = ~0ull;  // aocl_leaf_index of a removal record; "no input entry"

struct MsUpdateCounts {
    uint64_t witnesses = 0, aocl_digests = 0;
    MsChunkCounts chunks;
};
// block: as ms_apply_in_ok accepts it.  wit_off CSR over the jobs, fewer than 2^32 witnesses, the per-witness
// arrays present when there is a witness, aocl_path_off / aocl_path as ms_paths_ok, the dictionaries as
// ms_chunks_ok.
int ms_update_ok(const nhip_ms_apply_in* block, const nhip_ms_update_in* wit, MsUpdateCounts* counts);

struct MsUpdatePlan {
    // the output's shape: per witness, then per output entry
    std::vector<uint64_t> aocl_path_off, entry_off;
    std::vector<uint64_t> chunk_index, path_off, rel_off;
    // what the kernels read besides
    std::vector<uint32_t> wit_job;     // per witness
    std::vector<uint32_t> in_ent_wit;  // per input entry: its witness
    std::vector<uint32_t> ent_wit;     // per output entry: its witness
    std::vector<uint64_t> ent_src;     // ... and the first input entry of that witness with its key, or MS_UPDATE_NONE
};
// inputs that passed the checks above; NHIP_OK, or NHIP_ERR_OOM when a total would leave size_t / 64; may throw
// std::bad_alloc
int ms_update_plan(const nhip_ms_apply_in* block, const nhip_ms_update_in* wit, const MsUpdateCounts& counts,
                   MsUpdatePlan* plan);

// nhip_ms_update_plan / nhip_ms_update_batch: the output struct's shape (count pass: every array pointer but status
// null; fill: the offset arrays and, where a total is not zero, the others present with their capacities; need_data:
// status, aocl_path, path and rel too), then the totals and, when filling, the plan's arrays.  Does not touch the
// output on an error.
bool ms_updated_is_count_pass(const nhip_ms_updated* out);
int ms_updated_check(const MsUpdatePlan& plan, bool need_data, const nhip_ms_updated* out);
// keys: chunk_index too (the plan's keys; nhip_ms_update_batch's come from the device)
void ms_updated_write(const MsUpdatePlan& plan, bool keys, nhip_ms_updated* out);

}  // namespace nhip
