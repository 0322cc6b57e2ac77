// Host side of the device-resident witness store (nhip_ms_store_*): the mirror of the integers that
// describe the witnesses on the device (index sets, leaf indices, the four offset arrays, the keys, the sticky status
// bytes) and the shape arithmetic of append, select (read / retain) and "the plan becomes the shape".  This is all
// ms_update_plan reads: it touches no digest and no chunk word, so neither is kept on the host.  Every function
// checks before it changes anything: an error leaves the mirror as it was.  Host only (no HIP), so that
// tests/native/ms_store_check.cpp links it under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/neptune_hip.h"
#include "ms_update_plan.hpp"

namespace nhip {

// the gather kernel's work unit: 8-byte destination words (k_ms_store_gather, ms_store_kernels.hip)
static constexpr size_t MS_STORE_GATHER_UNIT = NHIP_MS_STORE_GATHER_UNIT;
static constexpr uint64_t MS_STORE_LIMIT = (uint64_t)(SIZE_MAX / 64);  // of any total, as ms_update_plan's

struct MsStoreMirror {
    std::vector<uint64_t> minimum;         // W x 2
    std::vector<uint32_t> distances;       // W x 45
    std::vector<uint64_t> leaf_index;      // W; MS_UPDATE_NONE: a removal record
    std::vector<uint64_t> aocl_path_off{0};  // W + 1, in digests
    std::vector<uint64_t> entry_off{0};      // W + 1
    std::vector<uint64_t> key;               // per entry: the plan's (the device's are zero for a sticky witness)
    std::vector<uint64_t> path_off{0};       // entries + 1, in digests
    std::vector<uint64_t> rel_off{0};        // entries + 1, in u32
    std::vector<uint8_t> sticky;             // W: the first status that was not NHIP_MS_OK, else NHIP_MS_OK

    size_t witnesses() const { return leaf_index.size(); }
    size_t entries() const { return key.size(); }
    MsUpdateCounts counts() const {
        MsUpdateCounts c;
        c.witnesses = witnesses();
        c.aocl_digests = aocl_path_off.back();
        c.chunks = MsChunkCounts{entries(), path_off.back(), rel_off.back()};
        return c;
    }
    bool operator==(const MsStoreMirror& o) const {
        return minimum == o.minimum && distances == o.distances && leaf_index == o.leaf_index &&
               aocl_path_off == o.aocl_path_off && entry_off == o.entry_off && key == o.key && path_off == o.path_off &&
               rel_off == o.rel_off && sticky == o.sticky;
    }
};

// The mirror as the one job's witnesses of ms_update_plan (which reads no path and no chunk word: both null).
// wit_off: two words the caller keeps alive, as `chunks`.
void ms_store_as_update_in(const MsStoreMirror& m, uint64_t wit_off[2], nhip_ms_chunks* chunks, nhip_ms_update_in* in);

// ---- append: n witnesses behind the mirror's
struct MsStoreAppend {
    MsUpdateCounts add;  // what comes in
    // the new tails of the four offset arrays, rebased behind the mirror's totals: n, n, entries, entries
    std::vector<uint64_t> aocl_path_off, entry_off, path_off, rel_off;
};
// The shape checks of ms_update_ok (wit->wit_off ignored): NHIP_ERR_ARG; a total past MS_STORE_LIMIT or 2^32 - 1
// witnesses or entries: NHIP_ERR_OOM.  May throw std::bad_alloc.
int ms_store_append_plan(const MsStoreMirror& m, const nhip_ms_update_in* wit, size_t n, MsStoreAppend* a);
// after a plan that returned NHIP_OK; throws std::bad_alloc before it changes anything
void ms_store_append_commit(MsStoreMirror& m, const nhip_ms_update_in* wit, size_t n, const MsStoreAppend& a);

// ---- append, from a restore whose shape was decided on the device (nhip_ms_store_append_restored):
// the plan's integers as they came back, all four offset arrays beginning at 0.  No path and no chunk word exists on
// the host, so there is no nhip_ms_update_in to read.
struct MsStoreRestored {
    size_t n = 0;                                                    // witnesses, every one NHIP_MS_OK
    const uint64_t *minimum = nullptr, *leaf_index = nullptr;        // n x 2, n
    const uint32_t* distances = nullptr;                             // n x 45
    const uint64_t *aocl_path_off = nullptr, *entry_off = nullptr;   // n + 1
    const uint64_t* chunk_index = nullptr;                           // entry_off[n]
    const uint64_t *path_off = nullptr, *rel_off = nullptr;          // entry_off[n] + 1
};
// ms_store_append_plan's limits for totals (AOCL digests, entries, path digests, chunk words) that n witnesses add:
// NHIP_ERR_ARG for n >= 2^32 - 1, NHIP_ERR_OOM past MS_STORE_LIMIT or 2^32 - 1 witnesses or entries
int ms_store_restored_ok(const MsStoreMirror& m, size_t n, const uint64_t add[4]);
// what ms_store_append_commit leaves for the same integers; throws std::bad_alloc before it changes anything
void ms_store_append_restored_commit(MsStoreMirror& m, const MsStoreRestored& r);

// ---- select: the witnesses sel[0 .. n) in that order, repeats allowed (read), or the kept ones (retain)
// Pools: 0 AOCL path digests, 1 entries (keys), 2 dictionary path digests, 3 chunk words (u32).
struct MsStoreSelect {
    std::vector<uint64_t> sel;     // n
    std::vector<uint64_t> src[4];  // n: where the witness's range begins in the source pool
    std::vector<uint64_t> dst[4];  // n + 1: the exclusive scan of the selected lengths
    // per selected entry, rebased: entries + 1 each
    std::vector<uint64_t> path_off, rel_off;
    // The gather's work units (k_ms_store_gather): pool p has the units [unit_end[p - 1], unit_end[p]), each
    // MS_STORE_GATHER_UNIT 8-byte destination words (5 per digest, 1 per key, 2 chunk words).  unit_first tells the
    // kernel which selected witness owns a unit's first word: pool p's units + 1 entries begin at
    // unit_end[p - 1] + p, the last of them n - 1 (0 when nothing is selected).
    uint64_t unit_end[4] = {0, 0, 0, 0};
    std::vector<uint32_t> unit_first;
    size_t n() const { return sel.size(); }
    uint64_t total(int pool) const { return dst[pool].back(); }
};
// sel null: the identity over n == W witnesses (or nothing, n == 0).  An index >= W, or sel null with another n:
// NHIP_ERR_ARG; a total past MS_STORE_LIMIT: NHIP_ERR_OOM.  May throw std::bad_alloc.
int ms_store_select(const MsStoreMirror& m, const uint64_t* sel, size_t n, MsStoreSelect* s);
// keep: W bytes
std::vector<uint64_t> ms_store_kept(const uint8_t* keep, size_t W);
// the mirror of the selection alone (retain: the store's mirror afterwards)
MsStoreMirror ms_store_selected_mirror(const MsStoreMirror& m, const MsStoreSelect& s);

// ---- update and revert: the plan's shape (ms_update_plan's or ms_revert_plan's, one struct) becomes the mirror's
// (offsets and keys), `status` (W bytes) its sticky bytes
void ms_store_apply_plan(MsStoreMirror& m, MsUpdatePlan&& plan, const uint8_t* status);

// ---- capacities: at least `need`, at least double `cap`; 0 when that passes `limit` elements
size_t ms_store_grown(size_t cap, size_t need, size_t limit);

}  // namespace nhip
