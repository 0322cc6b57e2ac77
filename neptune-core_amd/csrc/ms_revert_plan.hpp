// Host plan of nhip_ms_revert_batch: the shape of every witness before the block, taken back from
// where it stands after it.  Like the update's (ms_update_plan.hpp) it is an integer function of the inputs, laid
// out as if every job and every witness were accepted; no status is decided here and nothing is hashed.  With
// n0 / n1 the AOCL leaf counts before / after a job and b0 its batch index before: a witness's AOCL path before has
// ilog2(l ^ n0) digests (none when l >= n0: such a witness is rejected), its dictionary's keys are its chunk
// indices below b0 in ascending order, an entry's path has ilog2(key ^ b0) digests and its chunk has the words of
// the first input entry with that key less the job's record indices in that chunk, floored at 0 (a chunk that holds
// fewer is the device's to reject).  The plan is an MsUpdatePlan: the same four offset arrays and keys, each
// witness's job, each output entry's witness and the input entry it continues; in_ent_wit stays empty, since no
// input entry is authenticated.  Host only (no HIP), so that tests/native/ms_revert_check.cpp links it under
// ASan + UBSan.
#pragma once
#include "ms_update_plan.hpp"

namespace nhip {

// block and wit as ms_apply_in_ok and ms_update_ok accept them; NHIP_OK, or NHIP_ERR_OOM when a total would leave
// size_t / 64; may throw std::bad_alloc
int ms_revert_plan(const nhip_ms_apply_in* block, const nhip_ms_update_in* wit, const MsUpdateCounts& counts,
                   MsUpdatePlan* plan);

// Per job, in digests: where the old levels of its touched chunks lie in the call's scratch (k_ms_revert_nodes,
// ms_revert_kernels.hip): level L of group g at off[j] + L * n_grp + g, L <= ilog2(b0).  off[n_jobs] is the total.
// n_grp (all of the job's groups, as ms_apply_order counts them) is an upper bound of its touched chunks.
std::vector<uint64_t> ms_revert_node_offsets(const std::vector<MsApplyJob>& jobs);

}  // namespace nhip
