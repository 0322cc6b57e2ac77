// What ms_archive_kernels.hip and ms_archive_capi.hip share: the archive's device structs and the
// launch functions.  Every pointer is a device pointer.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ms_archive.hpp"

namespace nhip {

// One MMR as level arrays (ms_archive.hpp: ms_arch_node): 2 cap canonical digests, n leaves in level 0.
struct MsArchLevels {
    uint64_t* nodes;
    uint64_t cap, n;
};

// k_ms_arch_gather, a pool of authentication paths: owner s has leaf index leaf[s] in mmr and the destination digests
// dst_off[s] .. dst_off[s + 1], ilog2(leaf ^ n) of them or none; first: MsArchUnits::first.
struct MsArchPathPool {
    MsArchLevels mmr;
    const uint64_t *leaf, *dst_off;
    uint64_t owners, units;
    const uint32_t* first;
    uint64_t* dst;
};
// ... the pool of chunk words: owner e is chunk key[e], whose words lie in the arena where the table says
// (tab[2 c]: offset, tab[2 c + 1]: length; key null: owner e is chunk e), and has the destination words dst_off[e] .. dst_off[e + 1].
struct MsArchRelPool {
    const uint64_t* tab;
    const uint32_t* arena;
    const uint64_t *key, *dst_off;
    uint64_t owners, units;
    const uint32_t* first;
    uint32_t* dst;
    // 0 or 1: the pool's word w is element w + skew of dst, which is 8-byte aligned either way (a pool that begins at
    // an odd word of a larger array); units and `first` then count elements of dst, the first of which is nobody's
    uint64_t skew;
};
struct MsArchGatherDev {
    MsArchPathPool path[2];
    MsArchRelPool rel;
};

// level h (>= 1) of m, the parents [k0, k1), k1 <= m.n >> h
hipError_t launch_ms_arch_level(const MsArchLevels& m, uint32_t h, uint64_t k0, uint64_t k1, hipStream_t st);
// every level from[i] .. top[i] of m[i], i < 2, whole (MsArchBuild: few nodes each)
hipError_t launch_ms_arch_tail(const MsArchLevels m[2], const uint32_t from[2], const uint32_t top[2], hipStream_t st);
// Tip5::hash of the chunks [c0, c1) of the table into level 0 of swbf
// (d_written: of the chunks written[c0 .. c1) instead)
hipError_t launch_ms_arch_chunk_digests(const uint64_t* d_tab, const uint32_t* d_arena, uint64_t c0, uint64_t c1,
                                        const MsArchWritten* d_written, const MsArchLevels& swbf, hipStream_t st);
// apply: the n written chunks merged to the arena's tail and their table entries (MsArchWritten, ms_archive.hpp)
hipError_t launch_ms_arch_chunks(const MsArchWritten* d_written, uint64_t n, const uint32_t* d_block_rel,
                                 const uint32_t* d_window, uint32_t* d_arena, uint64_t* d_tab, hipStream_t st);
// revert: the n rewritten chunks minus the block's indices to the arena's tail and their table entries
// (MsArchRevertPlan::rewritten); *d_short_of, zero before, becomes 1 if a chunk holds fewer copies of a block index
// than the block inserted
hipError_t launch_ms_arch_unmerge(const MsArchWritten* d_rewritten, uint64_t n, const uint32_t* d_block_rel, uint32_t* d_arena,
                                  uint64_t* d_tab, uint32_t* d_short_of, hipStream_t st);
// apply, revert: per MMR the nodes ids[off[h - 1] .. off[h]) of level h = 1 .. levels hashed again (MsArchApplyPlan)
hipError_t launch_ms_arch_ancestors(const MsArchLevels m[2], const uint64_t* const d_ids[2], const uint32_t* const d_off[2],
                                    const uint32_t levels[2], hipStream_t st);
// d_out: 2 x 64 digests, the peaks of m[0] then of m[1], tallest first, zero behind the last
hipError_t launch_ms_arch_peaks(const MsArchLevels m[2], uint64_t* d_out, hipStream_t st);
hipError_t launch_ms_arch_gather(const MsArchGatherDev& g, hipStream_t st);

}  // namespace nhip
