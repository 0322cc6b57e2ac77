// Host side of the device-resident archival mutator set (nhip_ms_archive_*): the geometry of the MMR
// level arrays, the mirror of the integers that describe the archive on the device (both leaf counts, the chunk table,
// the window, the capacities) and every shape decision of load, paths and restore.  The mirror holds no digest.  Every
// function checks before it changes anything.  Host only (no HIP), so that tests/native/ms_archive_check.cpp links it
// under ASan + UBSan; the geometry functions are shared with the kernels (ms_archive_kernels.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/neptune_hip.h"
#include "ms_update_plan.hpp"

namespace nhip {

static constexpr uint64_t MS_ARCHIVE_TAIL_NODES = NHIP_MS_ARCHIVE_TAIL_NODES;
static constexpr uint64_t MS_ARCHIVE_GATHER_UNIT = 1024;  // 8-byte destination words per work unit of k_ms_arch_gather
static constexpr uint64_t MS_ARCHIVE_LIMIT = (uint64_t)(SIZE_MAX / 64);  // of any total, as ms_update_plan's
static constexpr uint64_t MS_ARCHIVE_MAX_LEAFS = 1ull << 40;  // of one MMR: 2 cap digests must stay below the limit
static constexpr uint32_t MS_ARCHIVE_CHUNK_SIZE = 1u << 12, MS_ARCHIVE_WINDOW_SIZE = 1u << 20;

// ---- an MMR of n leaves as level arrays.  Level h holds n >> h digests: node (h, k) is the root of the leaves
// [k 2^h, (k + 1) 2^h) and exists iff (k + 1) 2^h <= n.  The levels lie in one array of 2 cap digests, cap a power of
// two >= n: level h has cap >> h slots from digest 2 cap - (2 cap >> h) on, so the address of a node is arithmetic on
// (h, k) alone.  Levels above ilog2(cap) hold nothing.
// A revert (ms_archive_revert_plan) takes n down to n0 and hashes no AOCL node: a node that exists at n0 has only old
// leaves below it, and no apply since wrote it.  The slots at or beyond n0 >> h of level h are stale from then on and
// nothing may read them (every reader addresses existing nodes only: paths, peaks, the copies of a growth); the next
// apply lists every node above a new leaf (MsArchApplyPlan::ids), so it overwrites a stale slot before the leaf count
// makes it visible.  The same holds for the SWBF MMR at b0, whose nodes above a rewritten chunk are hashed again.
NHIP_MS_HD uint64_t ms_arch_level_base(uint64_t cap, uint32_t h) { return 2 * cap - ((2 * cap) >> h); }  // h <= ilog2(cap) + 1
NHIP_MS_HD uint64_t ms_arch_node(uint64_t cap, uint32_t h, uint64_t k) { return ms_arch_level_base(cap, h) + k; }
NHIP_MS_HD uint32_t ms_arch_ilog2(uint64_t x) {  // x != 0
    uint32_t r = 0;
    while (x >>= 1) ++r;
    return r;
}
// MmrMembershipProof of leaf i < n: ilog2(i ^ n) digests, digest t the node (t, (i >> t) ^ 1)
NHIP_MS_HD uint32_t ms_arch_path_len(uint64_t i, uint64_t n) { return ms_arch_ilog2(i ^ n); }

// the smallest power of two >= max(need, floor, 1); 0 past MS_ARCHIVE_MAX_LEAFS
uint64_t ms_arch_level_cap(uint64_t need, uint64_t floor);

// How the levels above the leaves are built (load): k_ms_arch_level once per level while the level it reads has more
// than MS_ARCHIVE_TAIL_NODES nodes, then one k_ms_arch_tail workgroup for every level from tail_from on (fewer than
// MS_ARCHIVE_TAIL_NODES hashes together).
struct MsArchBuild {
    uint32_t wide_levels = 0;  // the levels 1 .. wide_levels get a launch each
    uint32_t tail_from = 1;    // the first level the tail writes
    uint32_t top = 0;          // the last level that holds a node (0: leaves alone, or nothing)
};
MsArchBuild ms_arch_build(uint64_t n);

struct MsArchiveMirror {
    uint64_t aocl_leafs = 0;
    std::vector<uint64_t> chunk_off, chunk_len;  // per chunk: where its words begin in the arena, how many
    std::vector<uint32_t> window;                // sorted ascending, repeats kept
    uint64_t rel_tail = 0, rel_live = 0;         // the arena: words used from its begin, and those a chunk owns
    uint64_t aocl_cap = 0, swbf_cap = 0;         // the level arrays' capacities in leaves (powers of two, 0: none yet)

    uint64_t chunks() const { return chunk_len.size(); }
    uint64_t rel_dead() const { return rel_tail - rel_live; }
    bool empty() const { return aocl_leafs == 0 && chunk_len.empty() && window.empty(); }
};

// nhip_ms_archive_load's shape checks: NHIP_ERR_ARG unless every pointer with a non-zero count is present, rel_off
// starts at 0 and does not decrease, every chunk is sorted ascending below 4,096, the window is sorted ascending below
// 2^20 and n_chunks == batch_index(n_leafs); NHIP_ERR_OOM past the limits.
int ms_archive_load_ok(const uint64_t* aocl_leaves, uint64_t n_leafs, const uint64_t* rel_off, const uint32_t* rel,
                       uint64_t n_chunks, const uint32_t* active, uint64_t n_active);
// the mirror after a load that passed the checks; may throw std::bad_alloc before it changes anything
void ms_archive_load_commit(MsArchiveMirror& m, uint64_t n_leafs, const uint64_t* rel_off, uint64_t n_chunks,
                            const uint32_t* active, uint64_t n_active, uint64_t aocl_cap, uint64_t swbf_cap);

// ---- paths: MmrMembershipProof of n leaves of an MMR of num_leafs leaves.  An index >= num_leafs: NHIP_ERR_ARG.
// path_off: n + 1, in digests.  May throw std::bad_alloc.
int ms_archive_paths_plan(uint64_t num_leafs, const uint64_t* leaf_index, size_t n, std::vector<uint64_t>* path_off);

// ---- restore: the shape of n witnesses' membership proofs (or dictionaries alone) against an archive of aocl_leafs
// leaves whose chunk c < batch_index(aocl_leafs) holds chunk_len[c] words.  The output's shape as an MsUpdatePlan
// (wit_job sized n, ent_wit the entry's witness; the rest of the kernel side unused) and one status per witness: the
// first of NHIP_MS_NOT_IN_AOCL (a leaf index >= aocl_leafs, or aocl_leafs == 0) and NHIP_MS_OUT_OF_RANGE (§6c's
// fail-closed rule against the batch index); such a witness owns no digest and no entry.
// NHIP_ERR_ARG: a null array with n != 0; NHIP_ERR_OOM past the limits.  May throw std::bad_alloc.
int ms_archive_restore_plan(uint64_t aocl_leafs, const uint64_t* chunk_len, uint64_t n_chunks, const uint64_t* minimum,
                            const uint32_t* distances, const uint64_t* aocl_leaf_index, size_t n, MsUpdatePlan* plan,
                            std::vector<uint8_t>* status);

// ---- apply: the archive across one block of k additions and the records' index sets (records x 45 indices, taken as
// valid against the accumulator before: the block part decides that, and a rejected block's plan is never used).
// With n0 / n1 the AOCL leaf counts and b0 / b1 the batch indices before / after: every chunk c in [b0, b1) is
// created from the part [4096 (c - b0), 4096 (c - b0 + 1)) of the old window made relative (empty from c - b0 = 256 on),
// every chunk below b1 that an index hits is merged with those indices (repeats kept), each written chunk goes to the
// arena's tail, and both MMRs get their new and changed leaves with all their ancestors.
struct MsArchWritten {  // one chunk written anew, ascending in c
    uint64_t c;
    uint64_t a_off, a_len;  // its words before: in the arena (c < b0), or in the old window (from_window), or none
    uint64_t a_sub;         // what a window word loses to become relative: 4096 (c - b0)
    uint64_t b_off, b_len;  // the block's relative indices in it, sorted, in MsArchApplyPlan::block_rel
    uint64_t out_off;       // where the merged words go in the arena; a_len + b_len of them
    uint64_t from_window;
};
struct MsArchApplyPlan {
    uint64_t n0 = 0, n1 = 0, b0 = 0, b1 = 0;
    std::vector<MsArchWritten> written;
    std::vector<uint32_t> block_rel;
    uint64_t rel_tail_after = 0, rel_live_after = 0;
    // per MMR (0 AOCL, 1 SWBF) the nodes to hash again, level after level from level 1 on: ids[lvl_off[h - 1] ..
    // lvl_off[h]) are the k of level h, ascending; a node is listed iff it exists after the block and a new or
    // written leaf lies below it
    std::vector<uint64_t> ids[2];
    std::vector<uint32_t> lvl_off[2];
    bool compact = false;  // dead words exceed live words after the block
};
// NHIP_ERR_OOM past the limits (n1 wraps or passes MS_ARCHIVE_MAX_LEAFS, an arena past MS_ARCHIVE_LIMIT).  May throw.
int ms_archive_apply_plan(const MsArchiveMirror& m, uint64_t additions, const uint64_t* minimum, const uint32_t* distances,
                          size_t records, MsArchApplyPlan* plan);
// the mirror after a block whose plan this is and whose window after is `active` (sorted); throws before it changes anything
void ms_archive_apply_commit(MsArchiveMirror& m, const MsArchApplyPlan& plan, const uint32_t* active, uint64_t n_active,
                             uint64_t aocl_cap, uint64_t swbf_cap);
// the arena after a compaction: chunk c's words at the exclusive scan of the lengths
void ms_archive_compact_commit(MsArchiveMirror& m);

// ---- revert: the archive back across the block it stands behind, as an end state (ArchivalState::update_mutator_set's
// walk over abandoned blocks: revert_remove per record, then add_is_reversible / revert_add per addition in reverse).
// With n1 / b1 the mirror's counts, n0 = n1 - additions and b0 = batch_index(n0): the AOCL keeps its first n0 leaves
// (no node is hashed); the chunks [b0, b1) are dropped; every chunk below b0 that a block index hits loses one copy of
// that index per occurrence the block inserted (Chunk::subtract, the inverse of the apply plan's "repeats kept") and is
// written anew at the arena's tail; the SWBF MMR gets those leaves and every node above them that exists at b0.
// `rewritten` reuses MsArchWritten, the one layout the kernels read: a_off / a_len the chunk's words now, b_off / b_len
// the block's sorted relative indices in it, out_off where its a_len - b_len words after go; a_sub and from_window 0.
struct MsArchRevertPlan {
    uint64_t n0 = 0, n1 = 0, b0 = 0, b1 = 0;
    std::vector<MsArchWritten> rewritten;  // ascending in c, all below b0
    std::vector<uint32_t> block_rel;
    uint64_t dropped_words = 0;  // of the chunks [b0, b1), which leave the table
    uint64_t rel_tail_after = 0, rel_live_after = 0;
    // the SWBF nodes to hash again, as MsArchApplyPlan::ids[1] / lvl_off[1]: a node is listed iff it exists at b0 and a
    // rewritten chunk lies below it
    std::vector<uint64_t> ids;
    std::vector<uint32_t> lvl_off;
    bool compact = false;  // dead words exceed live words after the revert
};
// beside the NHIP_* codes: no block of these additions and records can have led to the mirror (additions > aocl_leafs,
// batch_index(n0) > chunks, or a hit chunk with fewer words than block indices in it); *plan is left alone
static constexpr int MS_ARCHIVE_REVERT_IMPOSSIBLE = -1;
// The plan is total: any additions, any records (null arrays with records == 0), any mirror whose two chunk vectors
// have one length.  NHIP_ERR_ARG: records without their arrays; NHIP_ERR_OOM past the limits.  May throw std::bad_alloc.
int ms_archive_revert_plan(const MsArchiveMirror& m, uint64_t additions, const uint64_t* minimum, const uint32_t* distances,
                           size_t records, MsArchRevertPlan* plan);
// the mirror after a revert whose plan this is and whose window before the block is `active` (sorted); capacities stay;
// throws before it changes anything
void ms_archive_revert_commit(MsArchiveMirror& m, const MsArchRevertPlan& plan, const uint32_t* active, uint64_t n_active);
// capacities: at least need, at least double cap (ms_store_grown's rule); 0 past limit
size_t ms_archive_grown(size_t cap, size_t need, size_t limit);

// ---- the gather's work units (k_ms_arch_gather): a pool of `owners` consecutive destination ranges, off[owners + 1]
// in units of `scale` 8-byte words (5: digests) or, with pairs, of u32 words of which a unit holds
// 2 MS_ARCHIVE_GATHER_UNIT.  first[u]: the owner of unit u's first word; first[units] = owners - 1 (0 without owners).
struct MsArchUnits {
    uint64_t units = 0;
    std::vector<uint32_t> first;  // units + 1
};
MsArchUnits ms_arch_units(const uint64_t* off, size_t owners, uint64_t scale, bool pairs);

}  // namespace nhip
