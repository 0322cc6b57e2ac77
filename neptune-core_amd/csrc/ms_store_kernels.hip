// The device-resident witness store (nhip_ms_store_*).
//
//  k_ms_store_gather : read and retain.  Copies every selected witness's four variable-length ranges (AOCL path,
//                      keys, dictionary paths, chunk words) and, for retain, its fixed per-witness integers from the
//                      source pools to the destination pools.  The destination ranges of a selection are contiguous
//                      (the host's exclusive scan of the selected lengths, MsStoreSelect), so the copy is a lane per
//                      8-byte destination word: consecutive lanes store consecutive words, whole lines, whatever the
//                      witnesses' lengths.  A workgroup takes a unit of MS_STORE_GATHER_UNIT consecutive destination
//                      words of one pool.  Which witness a word belongs to is told for the unit and searched for
//                      the lane: the host's sweep (MsStoreSelect::unit_first) names the owner of each unit's first
//                      word, so a unit's words belong to the witnesses from its own entry to the next unit's, and
//                      each lane finds its word among those few by a binary search that is usually 0 to 2 steps.
//                      (Finding the unit's bounds on the device, two binary searches over all n + 1 offsets that
//                      every lane repeats, was 32 dependent loads ahead of 8 KiB of copying: DESIGN.md §6i.)  The
//                      chunk words are u32 and a witness's range may begin on a 4-byte boundary in both pools: a lane
//                      takes an aligned pair of destination words, finds each word's source on its own and stores 8
//                      bytes; only the pool's last word can be a 4-byte store.
//                      Every lane writes below the destination totals dst[pool][n] only.
//  k_ms_store_seal   : behind k_ms_wit_seal of a store update.  A witness whose sticky byte is set gets that status
//                      back and its slots zeroed whatever admission made of its zeroed data; the statuses after
//                      become the next set's sticky bytes.
//  k_ms_store_check_seal : behind k_mmr_verify and k_ms_records of nhip_ms_store_check: a removal record has no
//                      AOCL part (member = 1); a sticky witness reports its sticky status and zeros.
#include "ms_device.hpp"
#include "ms_store.hpp"

namespace nhip {

namespace {

constexpr uint32_t GATHER_THREADS = 256;
constexpr uint64_t UNIT = MS_STORE_GATHER_UNIT;
constexpr uint64_t FIXED_UNIT = 256;  // witnesses per unit of the fixed part

// The selected witness that owns destination word g: the last i in [lo, hi) with off[i] * scale <= g.
// Requires off[lo] * scale <= g < off[hi] * scale.
__device__ __forceinline__ size_t owner(const uint64_t* __restrict__ off, uint64_t scale, size_t lo, size_t hi, uint64_t g) {
    size_t a = lo + 1, b = hi;
    while (a < b) {
        const size_t mid = a + (b - a) / 2;
        if (off[mid] * scale > g) b = mid;
        else a = mid + 1;
    }
    return a - 1;
}

// unit `u` of a pool of 8-byte words; scale: words per offset unit (5 for digests)
__device__ __forceinline__ void gather_words(const uint64_t* __restrict__ src_off, const uint64_t* __restrict__ dst_off,
                                             size_t n, uint64_t scale, const uint64_t* __restrict__ sp,
                                             uint64_t* __restrict__ dp, const uint32_t* __restrict__ first, uint64_t u) {
    const uint64_t total = dst_off[n] * scale;
    const uint64_t g0 = u * UNIT, g1 = g0 + UNIT < total ? g0 + UNIT : total;
    if (g0 >= g1) return;
    // the last word's owner is at most the next unit's first (n - 1 behind the last unit)
    const size_t sa = first[u], hi = (size_t)first[u + 1] + 1;
    static_assert(UNIT == 4 * GATHER_THREADS, "four words per lane");
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint64_t g = g0 + k * GATHER_THREADS + threadIdx.x;
        if (g < g1) {
            const size_t s = owner(dst_off, scale, sa, hi, g);
            dp[g] = sp[src_off[s] * scale + (g - dst_off[s] * scale)];
        }
    }
}

// unit `u` of the u32 pool: UNIT aligned pairs
__device__ __forceinline__ void gather_pairs(const uint64_t* __restrict__ src_off, const uint64_t* __restrict__ dst_off,
                                             size_t n, const uint32_t* __restrict__ sp, uint32_t* __restrict__ dp,
                                             const uint32_t* __restrict__ first, uint64_t u) {
    const uint64_t total = dst_off[n];
    const uint64_t w0 = 2 * u * UNIT, w1 = w0 + 2 * UNIT < total ? w0 + 2 * UNIT : total;
    if (w0 >= w1) return;
    const size_t sa = first[u], hi = (size_t)first[u + 1] + 1;
    for (uint64_t w = w0 + 2 * (uint64_t)threadIdx.x; w < w1; w += 2 * GATHER_THREADS) {
        const size_t s = owner(dst_off, 1, sa, hi, w);
        const uint32_t v0 = sp[src_off[s] + (w - dst_off[s])];
        if (w + 1 < w1) {
            const size_t s1 = w + 1 < dst_off[s + 1] ? s : owner(dst_off, 1, sa, hi, w + 1);
            const uint32_t v1 = sp[src_off[s1] + (w + 1 - dst_off[s1])];
            *reinterpret_cast<uint2*>(dp + w) = make_uint2(v0, v1);  // w is even and dp is 256-byte aligned
        } else {
            dp[w] = v0;
        }
    }
}

}  // namespace

__global__ void __launch_bounds__(GATHER_THREADS) k_ms_store_gather(MsStoreGatherDev g, MsStoreGatherUnits units) {
    for (uint64_t u = blockIdx.x; u < units.end[4]; u += gridDim.x) {
        if (u < units.end[0]) {
            gather_words(g.src[0], g.dst[0], g.n, 5, g.s_aocl, g.d_aocl, g.unit_first, u);
        } else if (u < units.end[1]) {
            gather_words(g.src[1], g.dst[1], g.n, 1, g.s_key, g.d_key, g.unit_first + units.end[0] + 1, u - units.end[0]);
        } else if (u < units.end[2]) {
            gather_words(g.src[2], g.dst[2], g.n, 5, g.s_path, g.d_path, g.unit_first + units.end[1] + 2, u - units.end[1]);
        } else if (u < units.end[3]) {
            gather_pairs(g.src[3], g.dst[3], g.n, g.s_rel, g.d_rel, g.unit_first + units.end[2] + 3, u - units.end[2]);
        } else {  // the fixed part: FIXED_UNIT witnesses
            const uint64_t s0 = (u - units.end[3]) * FIXED_UNIT;
            const uint64_t s1 = s0 + FIXED_UNIT < g.n ? s0 + FIXED_UNIT : g.n;
            const uint64_t s = s0 + threadIdx.x;
            if (s < s1) {
                const uint64_t w = g.sel[s];
                g.d_minimum[2 * s] = g.s_minimum[2 * w];
                g.d_minimum[2 * s + 1] = g.s_minimum[2 * w + 1];
                g.d_leaf_index[s] = g.s_leaf_index[w];
#pragma unroll
                for (int q = 0; q < 5; ++q) g.d_leaf[5 * s + q] = g.s_leaf[5 * w + q];
                g.d_sticky[s] = g.s_sticky[w];
            }
            for (uint64_t i = MSK_NUM_TRIALS * s0 + threadIdx.x; i < MSK_NUM_TRIALS * s1; i += GATHER_THREADS) {
                const uint64_t si = i / MSK_NUM_TRIALS;
                g.d_distances[i] = g.s_distances[MSK_NUM_TRIALS * g.sel[si] + (i - MSK_NUM_TRIALS * si)];
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_ms_store_seal(MsUpdateDev u, const uint8_t* __restrict__ sticky,
                                                       uint8_t* __restrict__ sticky_next, size_t witnesses) {
    for (size_t w = blockIdx.x * (size_t)blockDim.x + threadIdx.x; w < witnesses; w += (size_t)gridDim.x * blockDim.x) {
        const uint8_t was = sticky[w];
        if (was == NHIP_MS_OK) {
            sticky_next[w] = u.status[w];
            continue;
        }
        u.status[w] = was;
        sticky_next[w] = was;
        for (uint64_t d = 5 * u.o_aocl_path_off[w]; d < 5 * u.o_aocl_path_off[w + 1]; ++d) u.o_aocl_path[d] = 0;
        const uint64_t ebeg = u.o_entry_off[w], eend = u.o_entry_off[w + 1];
        for (uint64_t e = ebeg; e < eend; ++e) u.o_chunk_index[e] = 0;
        for (uint64_t d = 5 * u.o_path_off[ebeg]; d < 5 * u.o_path_off[eend]; ++d) u.o_path[d] = 0;
        for (uint64_t d = u.o_rel_off[ebeg]; d < u.o_rel_off[eend]; ++d) u.o_rel[d] = 0;
    }
}

__global__ void __launch_bounds__(256) k_ms_store_check_seal(const uint64_t* __restrict__ leaf_index,
                                                             const uint8_t* __restrict__ sticky, size_t witnesses,
                                                             uint8_t* __restrict__ member, uint8_t* __restrict__ valid,
                                                             uint8_t* __restrict__ verdict, uint8_t* __restrict__ status) {
    for (size_t w = blockIdx.x * (size_t)blockDim.x + threadIdx.x; w < witnesses; w += (size_t)gridDim.x * blockDim.x) {
        const uint8_t was = sticky[w];
        if (was != NHIP_MS_OK) {
            member[w] = valid[w] = verdict[w] = 0;
            status[w] = was;
        } else if (leaf_index[w] == MSA_NONE) {
            member[w] = 1;
        }
    }
}

MsStoreGatherUnits ms_store_gather_units(const uint64_t unit_end[4], size_t n, bool fixed) {
    MsStoreGatherUnits u{};
    for (int p = 0; p < 4; ++p) u.end[p] = unit_end[p];
    u.end[4] = unit_end[3] + (fixed ? (n + FIXED_UNIT - 1) / FIXED_UNIT : 0);
    return u;
}

hipError_t launch_ms_store_gather(const MsStoreGatherDev& g, const MsStoreGatherUnits& units, hipStream_t st) {
    if (units.end[4] == 0) return hipSuccess;
    const uint64_t grid = units.end[4] > 8192 ? 8192 : units.end[4];  // then unit-stride
    hipLaunchKernelGGL(k_ms_store_gather, dim3((unsigned)grid), dim3(GATHER_THREADS), 0, st, g, units);
    return hipGetLastError();
}

hipError_t launch_ms_store_seal(const MsUpdateDev& u, const uint8_t* sticky, uint8_t* sticky_next, size_t witnesses,
                                hipStream_t st) {
    return ms_launch(k_ms_store_seal, witnesses, st, u, sticky, sticky_next, witnesses);
}

hipError_t launch_ms_store_check_seal(const uint64_t* d_leaf_index, const uint8_t* d_sticky, size_t witnesses,
                                      uint8_t* d_member, uint8_t* d_valid, uint8_t* d_verdict, uint8_t* d_status,
                                      hipStream_t st) {
    return ms_launch(k_ms_store_check_seal, witnesses, st, d_leaf_index, d_sticky, witnesses, d_member, d_valid, d_verdict,
                     d_status);
}

}  // namespace nhip
