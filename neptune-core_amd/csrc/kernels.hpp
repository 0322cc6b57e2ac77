// Internal launch wrappers (C++ linkage) shared between kernel TUs and the C-ABI layer.
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ab_env.hpp"
#include "ms_shape.hpp"
#include "ms_unpack_plan.hpp"
#include "proof_codec.hpp"
#include "stark.hpp"
#include "xfe.hpp"

namespace nhip {

hipError_t launch_permutation(uint64_t* d_states, size_t n, hipStream_t st);
hipError_t launch_hash_pair(const uint64_t* d_l, const uint64_t* d_r, uint64_t* d_out, size_t n, hipStream_t st);
hipError_t launch_hash_varlen(const uint64_t* d_data, const uint64_t* d_off, size_t n, uint64_t* d_out,
                              hipStream_t st);
hipError_t launch_mtree_level(const uint64_t* d_children, uint64_t* d_parents, size_t n_parents, hipStream_t st);
hipError_t launch_mtree_verify(const uint64_t* d_roots, int per_path_root, const uint64_t* d_indices,
                               const uint64_t* d_leaves, const uint64_t* d_paths, uint32_t depth, size_t n,
                               uint8_t* d_verdicts, hipStream_t st);

// ---- MAST / mutator-set hashing (mast_kernels.hip)
hipError_t launch_mast_roots(const uint64_t* d_leaves, uint32_t fields, uint32_t pow2, size_t n, uint64_t* d_roots,
                             hipStream_t st);
hipError_t launch_absolute_index_sets(const uint64_t* d_digests, const uint64_t* d_aocl, size_t n, uint64_t* d_min,
                                      uint32_t* d_dist, hipStream_t st);

// ---- mutator-set checks (ms_kernels.hip); every pointer a device pointer
struct MmrDev {
    const uint64_t* peaks;  // n_peaks canonical digests, tallest peak first
    uint32_t n_peaks;
    uint64_t num_leafs;
};
// The chunk dictionaries of n owners (records or witnesses), flattened, on the device (nhip_ms_chunks on the host):
// owner i has the entries entry_off[i] .. entry_off[i + 1], in dictionary order.
struct MsChunksDev {
    const uint64_t *entry_off, *chunk_index;  // n + 1; per entry
    const uint64_t *path_off, *path;          // entries + 1, in digests; MMR authentication paths, leaf sibling first
    const uint64_t* rel_off;                  // entries + 1, in u32
    const uint32_t* rel;                      // Chunk::relative_indices
};
struct MsRecordsDev {
    const uint64_t* minimum;    // n x 2 (u128, little-endian)
    const uint32_t* distances;  // n x 45
    MsChunksDev ch;
    const uint8_t* auth;         // per entry, from k_ms_chunk_auth / k_ms_chunk_auth_jobs
    const uint8_t* aocl_member;  // per record, from k_ms_aocl_leaf: verify; nullptr: validate / can_remove
    const uint32_t* active;      // the active window's indices, sorted ascending
    uint64_t n_active;
    uint64_t aocl_num_leafs;
    uint8_t* valid;  // validate (nullptr with aocl_member)
    uint8_t* verdict;
    uint8_t* status;
};
hipError_t launch_mmr_verify(const MmrDev& mmr, const uint64_t* d_leaf_index, const uint64_t* d_leaves,
                             const uint64_t* d_path_off, const uint64_t* d_path, size_t n, uint8_t* d_verdicts,
                             hipStream_t st);
hipError_t launch_ms_aocl_leaf(const MmrDev& aocl, const uint64_t* d_digests, const uint64_t* d_leaf_index,
                               const uint64_t* d_path_off, const uint64_t* d_path, size_t n, uint8_t* d_member,
                               hipStream_t st);
hipError_t launch_ms_chunk_auth(const MmrDev& swbf, const MsChunksDev& ch, size_t entries, uint8_t* d_auth, hipStream_t st);
hipError_t launch_ms_records(const MsRecordsDev& r, size_t n, hipStream_t st);

// ---- batched mutator-set updates (ms_apply_kernels.hip); every pointer a device pointer
// One job as the host stages it: MsApplyJob (ms_shape.hpp).
struct MsApplyDev {
    const MsApplyJob* jobs;
    const uint64_t* peaks;       // canonical digests: every job's four peak lists
    const uint32_t* active;      // every job's active window, sorted ascending
    const uint64_t* additions;   // canonical commitments
    MsRecordsDev rec;            // the records of all jobs, and k_ms_records_jobs' outputs
    const uint32_t* rec_job;     // per record
    uint8_t* index_set;          // 45 per record (ms_record_decide)
    const uint32_t* idx_perm;    // per job: its 45 m index slots (record-in-job x 45 + t) sorted by (index, record)
    const uint32_t* grp;         // per job: the starts of the runs of one chunk index in that order, then 45 m
    const uint32_t* rec_perm;    // per job: its records sorted by their index arrays (stable)
    const uint32_t* exp_active;  // the expected windows in the caller's order
    uint32_t has_expected;
    uint64_t* dig;               // digest scratch
    uint64_t* aux;               // 2 per group: dictionary entry, chunk index
    uint8_t* verdict;
    uint8_t* status;
    uint64_t* bad;               // first bad record in the job, ~0 = none
    uint64_t* out_peaks;         // 2 x n_jobs x 64 digests: AOCL, SWBF
    uint32_t* out_np;            // 2 x n_jobs
    uint64_t* out_n;             // 3 x n_jobs: aocl.num_leafs, swbf_inactive.num_leafs, n_active
    uint32_t* out_active;
    // k_ms_apply<true> only (nhip_ms_update_batch)
    uint64_t* carry;             // n_jobs x 2 x 64 digests: the left edge of the AOCL append, of the SWBF append
    uint64_t* carry_mask;        // n_jobs x 2: the heights kept there
};
// k_ms_chunk_auth_jobs: the job looked up entry -> owner -> job; the owners are the block's records or its witnesses
struct MsChunkAuthJobsDev {
    const MsApplyJob* jobs;
    const uint64_t* peaks;                    // MsApplyDev::peaks
    MsChunksDev ch;
    const uint32_t *entry_owner, *owner_job;  // per entry, per owner
    uint8_t* auth;                            // per entry: 1 = the chunk is in the job's swbf_inactive at chunk_index
};
hipError_t launch_ms_chunk_auth_jobs(const MsChunkAuthJobsDev& c, size_t entries, hipStream_t st);
hipError_t launch_ms_records_jobs(const MsApplyDev& a, size_t n_records, hipStream_t st);
hipError_t launch_ms_apply(const MsApplyDev& a, size_t n_jobs, hipStream_t st, bool keep_nodes = false);

// ---- witnesses across a block (ms_update_kernels.hip); every pointer a device pointer
// The witnesses of all jobs, the plan's shape (MsUpdatePlan, ms_update_plan.hpp) and the outputs.  The kernels run
// behind k_ms_apply<true> and read its MsApplyDev: the jobs, their statuses, the group table and the kept nodes.
struct MsUpdateDev {
    const uint64_t* minimum;          // witnesses x 2
    const uint32_t* distances;        // witnesses x 45
    const uint64_t* aocl_leaf_index;  // ~0: no AOCL part
    const uint64_t* aocl_leaf;        // witnesses x 5
    const uint64_t* aocl_path_off;
    const uint64_t* aocl_path;
    MsChunksDev ch;                   // the input dictionaries
    const uint8_t* auth;              // per input entry, from k_ms_chunk_auth_jobs
    const uint32_t* wit_job;          // per witness
    // the plan
    const uint64_t* o_aocl_path_off;  // witnesses + 1
    const uint64_t* o_entry_off;      // witnesses + 1
    const uint64_t* o_key;            // per output entry
    const uint64_t* o_path_off;
    const uint64_t* o_rel_off;
    const uint32_t* o_ent_wit;
    const uint64_t* o_ent_src;
    // outputs
    uint8_t* status;                  // per witness
    uint8_t* err;                     // per witness: a digest was found nowhere
    uint64_t* o_aocl_path;
    uint64_t* o_chunk_index;
    uint64_t* o_path;
    uint32_t* o_rel;
};
hipError_t launch_ms_wit_admit(const MsApplyDev& a, const MsUpdateDev& u, size_t witnesses, hipStream_t st);
hipError_t launch_ms_wit_paths(const MsApplyDev& a, const MsUpdateDev& u, size_t witnesses, size_t entries, hipStream_t st);
hipError_t launch_ms_wit_chunks(const MsApplyDev& a, const MsUpdateDev& u, size_t entries, hipStream_t st);
hipError_t launch_ms_wit_seal(const MsUpdateDev& u, size_t witnesses, hipStream_t st);

// ---- witnesses back across a block (ms_revert_kernels.hip); every pointer a device pointer
// The kernels read an MsUpdateDev whose inputs are the witnesses after the block and whose plan is
// ms_revert_plan's (auth stays null: no input entry is authenticated), the block's MsApplyDev behind k_ms_apply, and:
struct MsRevertDev {
    const uint64_t* node_off;  // per job, in digests: ms_revert_node_offsets
    uint64_t* nodes;           // the old levels of the touched chunks: level L of group g at node_off[j] + L n_grp + g
    uint8_t* short_of;         // per witness: a kept chunk holds fewer copies of a block index than the block inserted
    const uint8_t* member;     // per witness, from k_ms_rev_aocl_jobs over the reverted AOCL parts
    const uint8_t* auth;       // per output entry, from k_ms_chunk_auth_jobs over the reverted dictionaries
};
hipError_t launch_ms_revert_nodes(const MsApplyDev& a, const MsRevertDev& r, size_t n_jobs, size_t groups, hipStream_t st);
hipError_t launch_ms_rev_admit(const MsApplyDev& a, const MsUpdateDev& u, const MsRevertDev& r, size_t witnesses, hipStream_t st);
hipError_t launch_ms_rev_paths(const MsApplyDev& a, const MsUpdateDev& u, const MsRevertDev& r, size_t witnesses,
                               size_t entries, hipStream_t st);
hipError_t launch_ms_rev_chunks(const MsApplyDev& a, const MsUpdateDev& u, const MsRevertDev& r, size_t entries, hipStream_t st);
hipError_t launch_ms_rev_aocl_jobs(const MsApplyDev& a, const MsUpdateDev& u, uint8_t* d_member, size_t witnesses, hipStream_t st);
hipError_t launch_ms_rev_seal(const MsUpdateDev& u, const MsRevertDev& r, size_t witnesses, hipStream_t st);

// ---- the device-resident witness store (ms_store_kernels.hip); every pointer a device pointer
// A selection (MsStoreSelect, ms_store.hpp) and the pools it is gathered from and into.  Pools: 0 AOCL path digests,
// 1 keys, 2 dictionary path digests, 3 chunk words.  The d_* fixed arrays may be null together (read: none is copied).
struct MsStoreGatherDev {
    size_t n;                // selected witnesses
    const uint64_t* sel;     // n (read by the fixed part only)
    const uint64_t* src[4];  // n: the begin of each witness's range in the source pool
    const uint64_t* dst[4];  // n + 1: the exclusive scan of the selected lengths
    const uint32_t* unit_first;  // MsStoreSelect::unit_first
    const uint64_t *s_aocl, *s_key, *s_path;
    const uint32_t* s_rel;
    uint64_t *d_aocl, *d_key, *d_path;
    uint32_t* d_rel;
    const uint64_t *s_minimum, *s_leaf_index, *s_leaf;
    const uint32_t* s_distances;
    const uint8_t* s_sticky;
    uint64_t *d_minimum, *d_leaf_index, *d_leaf;
    uint32_t* d_distances;
    uint8_t* d_sticky;
};
// the work units of one gather: pool p has the units [end[p - 1], end[p]), the fixed part [end[3], end[4])
struct MsStoreGatherUnits {
    uint64_t end[5];
};
// unit_end: MsStoreSelect::unit_end
MsStoreGatherUnits ms_store_gather_units(const uint64_t unit_end[4], size_t n, bool fixed);
hipError_t launch_ms_store_gather(const MsStoreGatherDev& g, const MsStoreGatherUnits& units, hipStream_t st);
hipError_t launch_ms_store_seal(const MsUpdateDev& u, const uint8_t* sticky, uint8_t* sticky_next, size_t witnesses,
                                hipStream_t st);
hipError_t launch_ms_store_check_seal(const uint64_t* d_leaf_index, const uint8_t* d_sticky, size_t witnesses,
                                      uint8_t* d_member, uint8_t* d_valid, uint8_t* d_verdict, uint8_t* d_status,
                                      hipStream_t st);

// ---- packed removal records (ms_unpack_kernels.hip); every pointer a device pointer
// The program of MsUnpackPlan (ms_unpack_plan.hpp) and the buffers it runs over.
struct MsUnpackDev {
    const MsUnpackJob* jobs;
    const uint32_t *leaf_slot, *leaf_cnt, *copy_slot, *op, *gath_src;
    const uint64_t *leaf_words, *copy_src, *lvl;
    const uint64_t* path_in;  // the packed input's structures, canonical digests
    const uint32_t* rel_in;   // ... and its packed chunk words
    uint64_t* arena;          // n_slots canonical digests
    uint64_t* path_out;       // the unpacked paths
};
hipError_t launch_ms_unpack(const MsUnpackDev& u, size_t n_jobs, hipStream_t st);

// ---- batched STARK verifier (stark_kernels.hip)
static constexpr uint32_t AIR_LDS_HEADER = (16 + 4 + 4 + 4) * 24 + 16;  // red (per wave), zinv, derived, misc, flag
static constexpr uint32_t AIR_LDS_BUDGET = 160 * 1024 - 8192;              // k_ood_air dynamic LDS cap
static constexpr uint32_t AIR_LDS_SLOTS_MAX = (AIR_LDS_BUDGET - AIR_LDS_HEADER) / 24;

// Level-synchronous Merkle multiproof plan (see k_mp_plan in stark_kernels.hip).  Ops of level l
// live in MP_SHARDS shards (shard = proof index % MP_SHARDS) so the per-level slot reservations of
// the plan workgroups spread over MP_SHARDS counters instead of contending on one.
static constexpr uint32_t MP_SHARDS = 16;
// k_mp_hash_tail climbs at most this many levels (TailCaps); which kernel instance runs at which batch
// size and level, and every threshold of that choice: stark_launch_plan.hpp
static constexpr uint32_t MP_TAIL_LEVELS_MAX = 32;
// k_roots_verdicts_small's one workgroup: the root checks and the verdicts of n_records + n_proofs <= this
static constexpr uint32_t ROOTS_ONE_WG = 1024;
struct MpRoot {
    uint64_t code;  // source code of the tree's final node, ~0 = no check (skipped or already failed)
    uint64_t root_off;
    uint32_t fail_bit, pad;
};
struct MpPlan {
    uint64_t* ops;                // 2 source codes per op
    uint64_t* arena;              // parent digest of op g (Montgomery), 5 words
    const uint64_t* shard_base;   // [levels][MP_SHARDS] first op index of the shard
    const uint64_t* shard_cap;    // [levels][MP_SHARDS] op capacity of the shard
    uint32_t* counter;            // [levels][MP_SHARDS] ops appended (zeroed per run)
    MpRoot* roots;                // n_proofs x (4 + max_R)
    uint32_t* dups;               // [n_proofs][1 + max_R][k] (slot, earlier slot) pairs of equal leaf indices
    uint32_t* ndup;               // [n_proofs][1 + max_R]
    uint32_t levels;
    // per (proof, tree group) and level: the group's first op and its ops per tree (written by the
    // plan; k_mp_climb walks them), and the number of levels recorded
    uint64_t* lvl_g0;   // [n_proofs][1 + max_R][levels]
    uint32_t* lvl_cnt;  // [n_proofs][1 + max_R][levels]
    uint32_t* lvl_n;    // [n_proofs][1 + max_R]
};

// One proof of a batch as staged for k_decode: its raw words and its staged claim encoding in the
// batch word buffer, and the padded height the host sized the batch's scratch with (from the
// proof header; SHAPE_NONE = malformed header).
struct ProofIn {
    uint64_t off, len;
    uint64_t claim_off;
    uint32_t claim_in_n, claim_out_n;
    uint32_t sized_log2_ph, pad;
};

// ---- wire bytes -> aligned words (wire_kernels.hip): words[in[i].off + k] = the little-endian u64 at
// d_raw + d_boff[i] + 8k, reduced mod p, for k < in[i].len; the proofs' words lie back to back from
// word 0 in `in` order (total_words of them).  The kernel's aligned loads reach at most 15 bytes
// below a proof's first byte and 16 bytes past its last: d_raw sits in an allocation whose base is
// 16-byte aligned and which extends WIRE_TAIL_PAD bytes past the last proof byte.
static constexpr size_t WIRE_TAIL_PAD = 16;
hipError_t launch_wire_words(const uint8_t* d_raw, const uint64_t* d_boff, const ProofIn* d_in, uint32_t n,
                             uint64_t total_words, uint64_t* d_words, hipStream_t st);

// Merkle hash launches (k_mp_hash / k_mp_hash_wide) timed per launch (start / stop event pairs)
static constexpr uint32_t MAX_HASH_LAUNCHES = 64;

// device counters of a run (zeroed per run, read back with the verdicts)
enum : uint32_t { CNT_MP_SKIPPED = 0, CNT_PERMS_STATIC = 1, CNT_PERMS_LCW = 2, CNT_N = 4 };

struct StarkBatchDev {
    uint32_t n_proofs, max_R;
    StarkDims dims;
    Dims D;
    uint32_t fs_stride, xs_stride;  // per-proof Fiat-Shamir program slots / sample areas (k_decode)
    const ProofIn* in;
    const uint64_t* words;
    ProofDesc* desc;
    FsOp* ops;
    uint64_t* xs;
    uint32_t* idx;
    uint64_t* dig;
    uint64_t* ood;
    uint64_t* xdom;        // [n_proofs][k] round-0 FRI domain point of each check (raw), k_fri -> k_deep
    uint64_t* lcw;         // [n_proofs][max_lcw][5] last-codeword Merkle tree nodes (heap order)
    uint32_t max_lcw;      // max last-codeword length (power of two)
    uint32_t* fail;                    // set by k_decode (FAIL_DECODE or 0), then ORed by every check
    uint8_t* verdicts;
    unsigned long long* counters;      // CNT_*: multiproof ops skipped (trees whose authentication
                                       // structure failed), decoded permutation counts
    MpPlan mp;
    const uint64_t* mp_cap_host;  // host: op capacity per level (launch sizes)
    const OodIns* air_prog;        // compiled AIR (OodIns per level)
    const uint32_t* air_prog_off;  // [3 n_levels + 1]: the steps' per-kind segment bounds (seg_off)
    uint32_t air_n_levels;
    const Xfe* air_consts;         // constant table (raw Montgomery)
    uint4 air_cons_off;            // constraint-type boundaries
    size_t air_lds_bytes;
    uint32_t air_block;  // k_ood_air workgroup size (1,024 when the slot area keeps one workgroup per CU)
    uint32_t air_lds_slots;        // slots held in LDS
    uint32_t air_gslot_n;          // slots past the LDS budget, per proof, in air_gslots
    Xfe* air_gslots;               // [n_proofs][air_gslot_n]
};

// The events of a batch launch: the phase timestamps and the cross-stream fork / join points
// (stark_launch_plan.hpp has the cross-stream set and the pair that brackets each reported phase).
enum StarkEvent : int {
    EV_DECODED = 0,       // aux stream, after k_decode
    EV_FS_DONE = 1,       // aux, after the Fiat-Shamir replay
    EV_ROWS_DONE = 2,     // main, after the row hashing
    EV_PLAN_DONE = 3,     // aux, after the Merkle plan
    EV_HASH_DONE = 4,     // main, after the last Merkle hash launch
    EV_ROOTS_DONE = 5,    // main, after the root checks
    EV_OOD_DONE = 6,      // aux, after k_ood_air
    EV_FRI_DONE = 7,      // after k_fri: aux, or main for small batches
    EV_DEEP_DONE = 8,     // aux, after k_deep_rows8: the main stream joins here
    EV_VERDICTS = 9,      // main, after the verdicts
    EV_AUX_RELEASE = 10,  // main, at the point the OOD / FRI / DEEP chain is released
    EV_AUX_START = 11,    // aux, after waiting for that release
    EV_FORK = 12,         // main, before k_decode: the aux stream starts here
    EV_FRI_START = 13,    // before FRI of a small batch (main; aux when fused with the plan)
    STARK_EVENTS
};
// The pair of events that brackets each phase nhip_stats reports.  Phases overlap (two streams):
// each is timed from the event its inputs wait on.  These are the spans of a batch that runs FRI on
// the aux stream; plan_launch (stark_launch_plan.hpp) sets the others.
struct PhaseSpan {
    StarkEvent from, to;
};
struct PhaseBrackets {
    PhaseSpan decode{EV_FORK, EV_DECODED}, fs{EV_DECODED, EV_FS_DONE}, rows{EV_DECODED, EV_ROWS_DONE},
        plan{EV_FS_DONE, EV_PLAN_DONE};
    PhaseSpan hash[2] = {{EV_ROWS_DONE, EV_HASH_DONE}, {EV_PLAN_DONE, EV_HASH_DONE}};  // the shorter of the two
    PhaseSpan roots{EV_HASH_DONE, EV_ROOTS_DONE}, ood{EV_AUX_START, EV_OOD_DONE};
    PhaseSpan fri{EV_OOD_DONE, EV_FRI_DONE}, deep{EV_FRI_DONE, EV_DEEP_DONE};  // FRI after OOD, DEEP after FRI
    PhaseSpan total{EV_FORK, EV_VERDICTS};
};
struct StarkPhaseTimer {
    hipEvent_t ev[STARK_EVENTS];
    hipEvent_t lev[2 * MAX_HASH_LAUNCHES];  // per hash launch: dispatch begin / end (nullptr = untimed)
    hipEvent_t rev[2] = {nullptr, nullptr};  // the row-hashing launch: dispatch begin / end (nullptr = untimed)
    bool launch_events = false;  // use lev / rev on this launch (nhip_batch_set_launch_timing)
    bool phase_marks = true;     // record the phase events (off in a captured graph: no phase split)
    // written by each enqueue (launch_stark_phases)
    uint32_t mp_hash_launches;
    PhaseBrackets spans;  // the events that bracket each phase of this launch
};

// Phases on two streams: st_aux runs the latency-bound chain (Fiat-Shamir -> Merkle plan -> OOD ->
// FRI -> DEEP), st the VALU-bound hashing (rows -> per-level Merkle hashes -> roots -> verdicts).
hipError_t launch_stark_phases(const StarkBatchDev& b, hipStream_t st, hipStream_t st_aux, StarkPhaseTimer* tm);
hipError_t stark_set_kernel_attributes();
// nhip_set_fs_form: -1 = by batch size (default), 0 row, 1 pair, 2 quad; -1 return = bad form
int set_fs_form(int form);
// nhip_set_climb_from_ops: -1 = default, 0 = never, k = at k hash ops; -1 return = bad value
int set_climb_from_ops(int64_t ops);

// k_deep_rows8's carry-free accumulation (stark_kernels.hip): a row has M + 3A < DEEP_ROW_WORDS_MAX
// words (dims_from), a lane takes at most ceil(M / 8) + ceil(3A / 8) <= DEEP_LANE_TERMS_MAX of them,
// each partial product is < 2^54, and a 64-bit accumulator must not reach 2^63
static constexpr uint32_t DEEP_ROW_WORDS_MAX = 2048;
static constexpr uint64_t DEEP_LANE_TERMS_MAX = (DEEP_ROW_WORDS_MAX - 1 + 14) / 8;
static_assert(DEEP_LANE_TERMS_MAX * (1ull << 54) < (1ull << 63), "k_deep_rows8 accumulators stay below 2^63");
// k_deep_rows8: the weights (one uint4 of limbs per coefficient), then one XFE per revealed row
inline size_t deep_rows8_lds_bytes(const StarkDims& d) {
    return (size_t)(3 * d.num_main + 9 * d.num_aux) * 16 + (size_t)d.num_checks * 24;
}

}  // namespace nhip
