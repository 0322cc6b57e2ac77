// What ms_restore_kernels.hip, ms_archive_capi.hip and ms_store_capi.hip share ("The hand-over"): the
// device form of the restore plan and the launches that hand restored witnesses to a store.  Every pointer is a
// device pointer.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ctx.hpp"
#include "ms_archive_device.hpp"
#include "ms_restore_shape.hpp"

namespace nhip {

// The shape scratch of n witnesses.  The four offset arrays hold lengths first and become exclusive scans in place.
//   aocl_path_off, entry_off : n + 1            keys : 45 n, witness w's sorted distinct keys from 45 w on
//   chunk_index              : 45 n             path_off, rel_off : 45 n + 1 (entry_off[n] entries are in use)
//   sums : 2 per scan tile of the larger scan   totals : aocl digests, entries, path digests, chunk words
struct MsRestoreShapeDev {
    const uint64_t *minimum, *leaf_index;
    const uint32_t* distances;
    const uint64_t* tab;  // the archive's chunk table: offset, length
    uint64_t aocl_leafs, n;
    uint8_t* status;
    uint64_t *aocl_path_off, *entry_off, *keys, *chunk_index, *path_off, *rel_off, *sums, *totals;
};
// The launches of the whole shape, in stream order: keys, the witness scan, the entries, the entry scan.
hipError_t launch_ms_restore_shape(const MsRestoreShapeDev& s, hipStream_t st);

// k_ms_arch_gather for pools whose owners the units find themselves (no MsArchUnits::first): the same three pools,
// `first` unused; rel.skew as MsArchRelPool says.
hipError_t launch_ms_arch_gather_own(const MsArchGatherDev& g, hipStream_t st);

// The hand-over's last kernel: the shape's offsets rebased behind a store's totals into its shape arrays, the keys
// into its key pool, and, with leaf, the archive's level-0 digest of every witness that has a leaf index (zeros for
// one that has none).
struct MsRestoreHandDev {
    MsRestoreShapeDev s;
    uint64_t entries;            // entry_off[n], known to the host by now
    uint64_t base[4];            // the store's totals: AOCL digests, entries, path digests, chunk words
    uint64_t w0;                 // ... and its witnesses
    uint64_t *aocl_path_off, *entry_off, *path_off, *rel_off, *key;  // the store's arrays, whole
    const uint64_t* aocl_nodes;  // level 0 of the AOCL begins the array
    uint64_t* leaf;              // the store's, whole; null: the caller's commitments were uploaded
};
hipError_t launch_ms_restore_hand(const MsRestoreHandDev& h, hipStream_t st);

// What a call that is not the archive's own may read of it: its context (fixed at creation), and under that context's
// lock the rest.
nhip_ctx* ms_archive_ctx(const nhip_ms_archive* a);
struct MsArchView {
    bool poisoned;
    MsArchLevels aocl, swbf;
    const uint64_t* tab;
    const uint32_t* arena;
};
MsArchView ms_archive_view(const nhip_ms_archive* a);

// The shape part of a call: declare() before commit(), enqueue() after, then read the totals and the statuses back.
struct RestoreShapePart {
    MsRestoreShapeDev d{};
    const size_t n;
    uint64_t totals[4] = {0, 0, 0, 0};
    RestoreShapePart(const MsArchView& v, size_t n_) : n(n_) {
        d.tab = v.tab;
        d.aocl_leafs = v.aocl.n;
        d.n = n_;
    }
    void declare(Stage& st, const uint64_t* minimum, const uint32_t* distances, const uint64_t* leaf_index) {
        const size_t tiles = (MS_RESTORE_TRIALS * n + MS_RESTORE_SCAN_WIDTH - 1) / MS_RESTORE_SCAN_WIDTH;
        st.in(d.minimum, minimum, n, 2);
        st.in(d.distances, distances, n, MS_RESTORE_TRIALS);
        st.in(d.leaf_index, leaf_index, n);
        st.tmp(d.status, n);
        st.tmp(d.aocl_path_off, n + 1);
        st.tmp(d.entry_off, n + 1);
        st.tmp(d.keys, n, MS_RESTORE_TRIALS);
        st.tmp(d.chunk_index, n, MS_RESTORE_TRIALS);
        st.tmp(d.path_off, MS_RESTORE_TRIALS * n + 1);
        st.tmp(d.rel_off, MS_RESTORE_TRIALS * n + 1);
        st.tmp(d.sums, tiles + 1, 2);
        st.tmp(d.totals, 4);
    }
    void enqueue(Stage& st, nhip_ctx* c, uint8_t* status_host) {
        st.launch([&] { return launch_ms_restore_shape(d, c->stream); });
        st.out(totals, d.totals, 4);
        st.out(status_host, d.status, n);
    }
    // the host plan's limits, from the totals that came back
    int limits() const {
        if (totals[1] > 0xFFFFFFFFull || totals[0] > MS_ARCHIVE_LIMIT || totals[2] > MS_ARCHIVE_LIMIT || totals[3] > MS_ARCHIVE_LIMIT)
            return NHIP_ERR_OOM;
        return NHIP_OK;
    }
};

}  // namespace nhip
