// The device-resident archival mutator set (nhip_ms_archive_*): every node of the AOCL MMR and of the
// inactive-SWBF MMR as level arrays (ms_archive.hpp: node (h, k) at digest 2 cap - (2 cap >> h) + k), every chunk's
// words in a u32 arena behind an (offset, length) table, the window.
//
//  k_ms_arch_level         : load.  A lane per parent: node (h, k) = hash_pair((h - 1, 2 k), (h - 1, 2 k + 1)) for a
//                            contiguous range of k.  One launch per level while the level it reads has more than
//                            NHIP_MS_ARCHIVE_TAIL_NODES nodes.
//  k_ms_arch_tail          : load.  One workgroup per MMR finishes all remaining levels, a barrier between two levels:
//                            they hold fewer than NHIP_MS_ARCHIVE_TAIL_NODES hashes together, and a launch each would
//                            cost more than hashing them.
//  k_ms_arch_chunk_digests : load.  A lane per chunk: Tip5::hash(chunk) (ms_chunk_sponge) over the arena table into
//                            level 0 of the SWBF MMR.  A lane per chunk and not a 16-lane row: the sponge is a serial
//                            chain of permutations whatever the lane count, a load has thousands of chunks to fill the
//                            lanes with, and ms_chunk_sponge is the form every other mutator-set kernel already uses.
//  k_ms_arch_peaks         : the accumulator.  A lane per word of the (at most 64) peaks of both MMRs: the peak of
//                            height h is node (h, (n >> h) - 1).
//  k_ms_arch_chunks        : apply.  Eight lanes per chunk written: its words before merged with the block's indices in
//                            it, at the arena's tail, and its table entry.
//  k_ms_arch_unmerge       : revert.  Eight lanes per chunk rewritten: its words minus the block's indices in it (one copy
//                            per occurrence), at the arena's tail, and its table entry.
//  k_ms_arch_ancestors     : apply and revert.  One workgroup per MMR hashes every node above a new or changed leaf
//                            again, level after level from the host plan's lists, out of the archive's own level arrays.
//  k_ms_arch_gather        : paths, restore and the arena's compaction.  A lane per 8-byte destination word, consecutive lanes storing
//                            consecutive words, in units of MS_ARCHIVE_GATHER_UNIT words.  Two pools of authentication
//                            paths and one of chunk words.  Which output range a word belongs to is found as in
//                            k_ms_store_gather: the host names the owner of each unit's first word (MsArchUnits) and
//                            a lane searches the few owners between its unit's and the next unit's.  The source of
//                            digest t of leaf i's path is arithmetic: node (t, (i >> t) ^ 1).  Chunk words are u32 and
//                            a range may begin on a 4-byte boundary: a lane takes an aligned pair of destination
//                            words, finds each word's source on its own and stores 8 bytes; only the pool's last word
//                            can be a 4-byte store (or its first, where the pool begins on an odd word of a store's:
//                            MsArchRelPool::skew).
//  k_ms_arch_gather_own    : the hand-over of restored witnesses to a store.  The same gather for offsets made on the
//                            device (ms_restore_kernels.hip): no host map names a unit's owners, so each unit finds
//                            those of its first and last word by two searches of the whole offset array.
// Every lane writes inside the ranges the host planned only: a level's n >> h nodes, the destination totals.
#include "ms_archive.hpp"
#include "ms_archive_device.hpp"
#include "ms_device.hpp"
#include "ms_restore_device.hpp"

namespace nhip {

namespace {

constexpr uint32_t ARCH_THREADS = 256;
constexpr uint64_t UNIT = MS_ARCHIVE_GATHER_UNIT;
static_assert(UNIT == 4 * ARCH_THREADS, "four words per lane");

__device__ __forceinline__ const uint64_t* arch_node(const MsArchLevels& m, uint32_t h, uint64_t k) {
    return m.nodes + 5 * ms_arch_node(m.cap, h, k);
}

// parents [k0, k1) of level h, strided over `stride` lanes from lane `lane`; no __restrict__: one array
__device__ __forceinline__ void arch_level(const MsArchLevels& m, uint32_t h, uint64_t k0, uint64_t k1, uint64_t lane,
                                           uint64_t stride, const uint8_t* lut) {
    const uint64_t* child = m.nodes + 5 * ms_arch_level_base(m.cap, h - 1);
    uint64_t* parent = m.nodes + 5 * ms_arch_level_base(m.cap, h);
    for (uint64_t k = k0 + lane; k < k1; k += stride) {
        uint64_t out[5];
        dig_hp(child + 10 * k, child + 10 * k + 5, out, lut);
#pragma unroll
        for (int q = 0; q < 5; ++q) parent[5 * k + q] = out[q];
    }
}

// The owner of destination word g: the last i in [lo, hi) with off[i] * scale <= g.
// Requires off[lo] * scale <= g < off[hi] * scale.
__device__ __forceinline__ uint64_t owner(const uint64_t* __restrict__ off, uint64_t scale, uint64_t lo, uint64_t hi, uint64_t g) {
    uint64_t a = lo + 1, b = hi;
    while (a < b) {
        const uint64_t mid = a + (b - a) / 2;
        if (off[mid] * scale > g) b = mid;
        else a = mid + 1;
    }
    return a - 1;
}

// sa, hi: the unit's owners lie in [sa, hi)
__device__ __forceinline__ void gather_paths(const MsArchPathPool& p, uint64_t u, uint64_t sa, uint64_t hi) {
    const uint64_t total = 5 * p.dst_off[p.owners];
    const uint64_t g0 = u * UNIT, g1 = g0 + UNIT < total ? g0 + UNIT : total;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint64_t g = g0 + k * ARCH_THREADS + threadIdx.x;
        if (g < g1) {
            const uint64_t s = owner(p.dst_off, 5, sa, hi, g);
            const uint64_t d = g / 5;
            const uint32_t t = (uint32_t)(d - p.dst_off[s]);  // < ilog2(leaf ^ n): the sibling exists
            p.dst[g] = arch_node(p.mmr, t, (p.leaf[s] >> t) ^ 1)[g - 5 * d];
        }
    }
}

__device__ __forceinline__ uint32_t rel_word(const MsArchRelPool& p, uint64_t s, uint64_t w) {
    return p.arena[p.tab[2 * (p.key ? p.key[s] : s)] + (w - p.dst_off[s])];  // key null: chunk s (compaction)
}

// A unit's pairs are aligned in the destination array: word w of the pool is element w + skew of p.dst, which is
// 8-byte aligned, and a unit takes the elements [2 u UNIT, 2 (u + 1) UNIT); the elements below skew belong to nobody.
__device__ __forceinline__ void gather_rel(const MsArchRelPool& p, uint64_t u, uint64_t sa, uint64_t hi) {
    const uint64_t skew = p.skew, end = p.dst_off[p.owners] + skew;
    const uint64_t x0 = 2 * u * UNIT, x1 = x0 + 2 * UNIT < end ? x0 + 2 * UNIT : end;
    for (uint64_t x = x0 + 2 * (uint64_t)threadIdx.x; x < x1; x += 2 * ARCH_THREADS) {
        const bool low = x >= skew, high = x + 1 < x1;  // skew <= 1: the high element is a word whenever it is in range
        uint64_t s = 0;
        uint32_t v0 = 0, v1 = 0;
        if (low) {
            s = owner(p.dst_off, 1, sa, hi, x - skew);
            v0 = rel_word(p, s, x - skew);
        }
        if (high) {
            const uint64_t w = x + 1 - skew;
            const uint64_t s1 = low && w < p.dst_off[s + 1] ? s : owner(p.dst_off, 1, sa, hi, w);
            v1 = rel_word(p, s1, w);
        }
        if (low && high) *reinterpret_cast<uint2*>(p.dst + x) = make_uint2(v0, v1);  // x even, dst 8-byte aligned
        else if (low) p.dst[x] = v0;
        else if (high) p.dst[x + 1] = v1;
    }
}

// the unit's owners when no host map names them: those of its first and of its last word, by two searches of the
// whole offset array, the same in every lane
__device__ __forceinline__ void own_range(const uint64_t* __restrict__ off, uint64_t owners, uint64_t scale, uint64_t g0,
                                          uint64_t g_last, uint64_t* sa, uint64_t* hi) {
    *sa = owner(off, scale, 0, owners, g0);
    *hi = owner(off, scale, *sa, owners, g_last) + 1;
}

}  // namespace

__global__ void __launch_bounds__(ARCH_THREADS) k_ms_arch_level(MsArchLevels m, uint32_t h, uint64_t k0, uint64_t k1) {
    __shared__ Tip5Lds t5;
    tip5_lds_init(t5);
    arch_level(m, h, k0, k1, blockIdx.x * (uint64_t)blockDim.x + threadIdx.x, (uint64_t)gridDim.x * blockDim.x, t5.lut);
}

struct MsArchTail {
    MsArchLevels m[2];
    uint32_t from[2], top[2];
};
__global__ void __launch_bounds__(ARCH_THREADS) k_ms_arch_tail(MsArchTail a) {
    __shared__ Tip5Lds t5;
    tip5_lds_init(t5);
    const MsArchLevels m = a.m[blockIdx.x];
    const uint32_t from = a.from[blockIdx.x], top = a.top[blockIdx.x];  // workgroup-uniform: every lane meets every barrier
    for (uint32_t h = from; h <= top; ++h) {
        arch_level(m, h, 0, m.n >> h, threadIdx.x, blockDim.x, t5.lut);
        __syncthreads();  // level h is written (and visible to this workgroup) before level h + 1 reads it
    }
}

__global__ void __launch_bounds__(ARCH_THREADS) k_ms_arch_chunk_digests(const uint64_t* __restrict__ tab,
                                                                        const uint32_t* __restrict__ arena, uint64_t c0,
                                                                        uint64_t c1, const MsArchWritten* __restrict__ written,
                                                                        MsArchLevels swbf) {
    __shared__ Tip5Lds t5;
    tip5_lds_init(t5);
    // written: the chunks written[c0 .. c1) instead of the chunks c0 .. c1 - 1
    for (uint64_t i = c0 + blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < c1; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t c = written ? written[i].c : i;
        const uint32_t* __restrict__ idx = arena + tab[2 * c];
        uint64_t run[5];
        ms_chunk_sponge(tab[2 * c + 1], [&](uint64_t w) { return idx[w]; }, run, t5.lut);
        uint64_t* leaf = swbf.nodes + 5 * ms_arch_node(swbf.cap, 0, c);
#pragma unroll
        for (int q = 0; q < 5; ++q) leaf[q] = from_mont(run[q]);
    }
}

struct MsArchPair {
    MsArchLevels m[2];
};
__global__ void __launch_bounds__(320) k_ms_arch_peaks(MsArchPair a, uint64_t* __restrict__ out) {
    const MsArchLevels m = a.m[blockIdx.x];
    const uint32_t d = threadIdx.x / 5, q = threadIdx.x - 5 * d;  // peak d (tallest first), word q
    uint64_t v = 0;
    uint32_t seen = 0;
    for (int h = 63; h >= 0; --h) {
        if (!(m.n >> h & 1)) continue;
        if (seen++ == d) {
            v = arch_node(m, (uint32_t)h, (m.n >> h) - 1)[q];
            break;
        }
    }
    out[(size_t)blockIdx.x * 320 + threadIdx.x] = v;
}

// Eight lanes per chunk written: the merge of two sorted lists, the chunk's words before (in the arena, or the part of
// the old window that slides out, made relative) and the block's relative indices in it, each word placed by a binary
// search in the other list (a word before stands ahead of an equal block index; repeats kept), at the arena's tail
// where the host planned it.  Lane 0 of the eight writes the chunk's table entry.  Reads below the old tail and the
// old window only, writes [out_off, out_off + a_len + b_len) only.
__global__ void __launch_bounds__(ARCH_THREADS) k_ms_arch_chunks(const MsArchWritten* __restrict__ written, uint64_t n,
                                                                 const uint32_t* __restrict__ block_rel,
                                                                 const uint32_t* __restrict__ window, uint32_t* arena,
                                                                 uint64_t* __restrict__ tab) {
    const uint32_t sub = threadIdx.x & 7u;
    for (uint64_t i = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 3; i < n; i += ((uint64_t)gridDim.x * blockDim.x) >> 3) {
        const MsArchWritten w = written[i];
        const uint32_t* a = w.from_window ? window + w.a_off : arena + w.a_off;
        const uint32_t* b = block_rel + w.b_off;
        const uint32_t shift = (uint32_t)w.a_sub;
        uint32_t* out = arena + w.out_off;
        for (uint64_t k = sub; k < w.a_len; k += 8) {
            const uint32_t v = a[k] - shift;
            out[k + lb_u32(b, w.b_len, v)] = v;  // the block indices below it
        }
        for (uint64_t k = sub; k < w.b_len; k += 8) {
            const uint32_t v = b[k];
            uint64_t lo = 0, hi = w.a_len;  // the words before at or below it
            while (lo < hi) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if (a[mid] - shift <= v) lo = mid + 1;
                else hi = mid;
            }
            out[k + lo] = v;
        }
        if (sub == 0) {
            tab[2 * w.c] = w.out_off;
            tab[2 * w.c + 1] = w.a_len + w.b_len;
        }
    }
}

// Eight lanes per chunk rewritten: the multiset difference of two sorted lists, the chunk's words now and the block's
// relative indices in it (Chunk::subtract once per index; the inverse of k_ms_arch_chunks' "repeats kept").  The rule is
// k_ms_rev_chunks' (ms_revert_kernels.hip), restated: the word at position i, the rank-th of its value, goes if the
// block inserted more copies than that; a word that stays moves down by the block's indices below it and its own
// value's copies.  A block value with fewer copies in the chunk than the block inserted sets *short_of, and the host
// then trusts nothing the call wrote; `pos < out_len` keeps every write inside the planned range even then.  Lane 0 of
// the eight writes the chunk's table entry.  Reads below the old tail only (a_off + a_len <= old tail <= out_off),
// writes [out_off, out_off + a_len - b_len) only; the host plan has a_len >= b_len.
__global__ void __launch_bounds__(ARCH_THREADS) k_ms_arch_unmerge(const MsArchWritten* __restrict__ written, uint64_t n,
                                                                  const uint32_t* __restrict__ block_rel, uint32_t* arena,
                                                                  uint64_t* __restrict__ tab, uint32_t* __restrict__ short_of) {
    const uint32_t sub = threadIdx.x & 7u;
    for (uint64_t i = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 3; i < n; i += ((uint64_t)gridDim.x * blockDim.x) >> 3) {
        const MsArchWritten w = written[i];
        const uint32_t* a = arena + w.a_off;
        const uint32_t* b = block_rel + w.b_off;
        uint32_t* out = arena + w.out_off;
        const uint64_t out_len = w.a_len - w.b_len;
        for (uint64_t k = sub; k < w.a_len; k += 8) {
            const uint32_t v = a[k];
            const uint64_t rank = k - lb_u32(a, w.a_len, v);
            const uint64_t lt = lb_u32(b, w.b_len, v), cnt = lb_u32(b, w.b_len, (uint64_t)v + 1) - lt;
            if (rank < cnt) continue;
            const uint64_t pos = k - lt - cnt;
            if (pos < out_len) out[pos] = v;
        }
        for (uint64_t k = sub; k < w.b_len; k += 8) {  // every block index is there as often as the block inserted it
            const uint32_t v = b[k];
            if (k != 0 && b[k - 1] == v) continue;  // once per value
            const uint64_t cnt = lb_u32(b, w.b_len, (uint64_t)v + 1) - k;
            const uint64_t have = lb_u32(a, w.a_len, (uint64_t)v + 1) - lb_u32(a, w.a_len, v);
            if (have < cnt) *short_of = 1u;
        }
        if (sub == 0) {
            tab[2 * w.c] = w.out_off;
            tab[2 * w.c + 1] = out_len;
        }
    }
}

// apply: the nodes above the new and the written leaves, hashed again from the archive's own level arrays.  One
// workgroup per MMR; level h's nodes are ids[off[h - 1] .. off[h]), a barrier between two levels.
struct MsArchAncestors {
    MsArchLevels m[2];
    const uint64_t* ids[2];
    const uint32_t* off[2];
    uint32_t levels[2];
};
__global__ void __launch_bounds__(ARCH_THREADS) k_ms_arch_ancestors(MsArchAncestors a) {
    __shared__ Tip5Lds t5;
    tip5_lds_init(t5);
    const MsArchLevels m = a.m[blockIdx.x];
    const uint64_t* __restrict__ ids = a.ids[blockIdx.x];
    const uint32_t* __restrict__ off = a.off[blockIdx.x];
    const uint32_t levels = a.levels[blockIdx.x];  // workgroup-uniform
    for (uint32_t h = 1; h <= levels; ++h) {
        const uint64_t* child = m.nodes + 5 * ms_arch_level_base(m.cap, h - 1);
        uint64_t* parent = m.nodes + 5 * ms_arch_level_base(m.cap, h);
        for (uint32_t j = off[h - 1] + threadIdx.x; j < off[h]; j += blockDim.x) {
            const uint64_t k = ids[j];  // < m.n >> h: the plan lists existing nodes only
            uint64_t out[5];
            dig_hp(child + 10 * k, child + 10 * k + 5, out, t5.lut);
#pragma unroll
            for (int q = 0; q < 5; ++q) parent[5 * k + q] = out[q];
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(ARCH_THREADS) k_ms_arch_gather(MsArchGatherDev g) {
    const uint64_t e0 = g.path[0].units, e1 = e0 + g.path[1].units, e2 = e1 + g.rel.units;
    for (uint64_t u = blockIdx.x; u < e2; u += gridDim.x) {
        // the last word's owner is at most the next unit's first (owners - 1 behind the last unit)
        if (u < e0) gather_paths(g.path[0], u, g.path[0].first[u], (uint64_t)g.path[0].first[u + 1] + 1);
        else if (u < e1) gather_paths(g.path[1], u - e0, g.path[1].first[u - e0], (uint64_t)g.path[1].first[u - e0 + 1] + 1);
        else gather_rel(g.rel, u - e1, g.rel.first[u - e1], (uint64_t)g.rel.first[u - e1 + 1] + 1);
    }
}

// The same gather for pools whose offsets were made on the device (ms_restore_kernels.hip), where no host map can
// name a unit's owners: every unit finds them itself.
__global__ void __launch_bounds__(ARCH_THREADS) k_ms_arch_gather_own(MsArchGatherDev g) {
    const uint64_t e0 = g.path[0].units, e1 = e0 + g.path[1].units, e2 = e1 + g.rel.units;
    for (uint64_t u = blockIdx.x; u < e2; u += gridDim.x) {
        uint64_t sa, hi;
        if (u < e1) {
            const MsArchPathPool& p = u < e0 ? g.path[0] : g.path[1];
            const uint64_t v = u < e0 ? u : u - e0, total = 5 * p.dst_off[p.owners];
            const uint64_t g0 = v * UNIT, g1 = g0 + UNIT < total ? g0 + UNIT : total;  // g0 < total: the unit exists
            own_range(p.dst_off, p.owners, 5, g0, g1 - 1, &sa, &hi);
            gather_paths(p, v, sa, hi);
        } else {
            const MsArchRelPool& p = g.rel;
            const uint64_t v = u - e1, skew = p.skew, end = p.dst_off[p.owners] + skew;
            const uint64_t x0 = 2 * v * UNIT, x1 = x0 + 2 * UNIT < end ? x0 + 2 * UNIT : end;
            own_range(p.dst_off, p.owners, 1, (x0 > skew ? x0 : skew) - skew, x1 - 1 - skew, &sa, &hi);  // x1 > skew: units from the words
            gather_rel(p, v, sa, hi);
        }
    }
}

hipError_t launch_ms_arch_level(const MsArchLevels& m, uint32_t h, uint64_t k0, uint64_t k1, hipStream_t st) {
    return ms_launch(k_ms_arch_level, (size_t)(k1 - k0), st, m, h, k0, k1);
}

hipError_t launch_ms_arch_tail(const MsArchLevels m[2], const uint32_t from[2], const uint32_t top[2], hipStream_t st) {
    const MsArchTail a{{m[0], m[1]}, {from[0], from[1]}, {top[0], top[1]}};
    if (from[0] > top[0] && from[1] > top[1]) return hipSuccess;
    hipLaunchKernelGGL(k_ms_arch_tail, dim3(2), dim3(ARCH_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_ms_arch_chunk_digests(const uint64_t* d_tab, const uint32_t* d_arena, uint64_t c0, uint64_t c1,
                                        const MsArchWritten* d_written, const MsArchLevels& swbf, hipStream_t st) {
    return ms_launch(k_ms_arch_chunk_digests, (size_t)(c1 - c0), st, d_tab, d_arena, c0, c1, d_written, swbf);
}

hipError_t launch_ms_arch_chunks(const MsArchWritten* d_written, uint64_t n, const uint32_t* d_block_rel,
                                 const uint32_t* d_window, uint32_t* d_arena, uint64_t* d_tab, hipStream_t st) {
    return ms_launch(k_ms_arch_chunks, (size_t)(8 * n), st, d_written, n, d_block_rel, d_window, d_arena, d_tab);
}

hipError_t launch_ms_arch_unmerge(const MsArchWritten* d_rewritten, uint64_t n, const uint32_t* d_block_rel, uint32_t* d_arena,
                                  uint64_t* d_tab, uint32_t* d_short_of, hipStream_t st) {
    return ms_launch(k_ms_arch_unmerge, (size_t)(8 * n), st, d_rewritten, n, d_block_rel, d_arena, d_tab, d_short_of);
}

hipError_t launch_ms_arch_ancestors(const MsArchLevels m[2], const uint64_t* const d_ids[2], const uint32_t* const d_off[2],
                                    const uint32_t levels[2], hipStream_t st) {
    if (levels[0] == 0 && levels[1] == 0) return hipSuccess;
    const MsArchAncestors a{{m[0], m[1]}, {d_ids[0], d_ids[1]}, {d_off[0], d_off[1]}, {levels[0], levels[1]}};
    hipLaunchKernelGGL(k_ms_arch_ancestors, dim3(2), dim3(ARCH_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_ms_arch_peaks(const MsArchLevels m[2], uint64_t* d_out, hipStream_t st) {
    const MsArchPair a{{m[0], m[1]}};
    hipLaunchKernelGGL(k_ms_arch_peaks, dim3(2), dim3(320), 0, st, a, d_out);
    return hipGetLastError();
}

hipError_t launch_ms_arch_gather(const MsArchGatherDev& g, hipStream_t st) {
    const uint64_t units = g.path[0].units + g.path[1].units + g.rel.units;
    if (units == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ms_arch_gather, dim3((unsigned)(units > 8192 ? 8192 : units)), dim3(ARCH_THREADS), 0, st, g);
    return hipGetLastError();
}

hipError_t launch_ms_arch_gather_own(const MsArchGatherDev& g, hipStream_t st) {
    const uint64_t units = g.path[0].units + g.path[1].units + g.rel.units;
    if (units == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ms_arch_gather_own, dim3((unsigned)(units > 8192 ? 8192 : units)), dim3(ARCH_THREADS), 0, st, g);
    return hipGetLastError();
}

}  // namespace nhip
