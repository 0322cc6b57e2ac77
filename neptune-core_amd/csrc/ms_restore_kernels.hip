// The restore plan on the device and the hand-over of restored witnesses to a store (nhip_ms_archive_restore_shape,
// nhip_ms_store_append_restored; DESIGN.md §6k, "The hand-over").  Every integer equals ms_archive_restore_plan's.
//
//  k_ms_rst_keys       : one wave per witness.  Lane t < 45 forms minimum + distance[t] as two u64 halves with an
//                        explicit carry (ms_restore_chunk) and keeps its chunk index if that lies below the batch
//                        index; ballots decide the status in the plan's precedence.  The keys are made distinct and
//                        sorted by rank counting across the wave: a lane whose key a lower lane also holds drops it,
//                        every other lane counts the kept keys below its own and stores its key at that rank.  Lane 0
//                        writes the witness's AOCL path length, key count and status.
//  k_ms_rst_scan_tiles, k_ms_rst_scan_carry, k_ms_rst_scan_apply
//                      : the exclusive scan of two u64 arrays in place, with saturating adds (a total past the plan's
//                        limit stays past it).  Tiles of MS_RESTORE_SCAN_WIDTH items, one per lane: the tile sums, then
//                        one wave of MS_RESTORE_CARRY_LANES lanes that turns the sums into the tiles' carries (a
//                        segment of tiles per lane, scanned serially around a wave scan) and writes the totals, then
//                        each tile scanned again on top of its carry.  The item count may live on the device: the
//                        entries' count is the witness scan's total.
//  k_ms_rst_entries    : a lane per key slot (witness, j < 45): the key to its entry, the entry's path length
//                        ilog2(key ^ b) and its chunk's word count from the archive's table, as the lengths the second
//                        scan turns into path_off and rel_off.
//  k_ms_rst_hand       : the hand-over.  A lane per witness and per entry: the offsets rebased behind the store's totals
//                        into the store's shape arrays, the keys into its key pool, and the archive's level-0 digest
//                        as the witness's leaf where the caller gave none.
// Every lane writes inside what the host sized: n or n + 1 per witness array, 45 n or 45 n + 1 per entry array (a
// witness owns at most 45 entries), the store's arrays up to the totals the host grew them to.
#include "ms_device.hpp"
#include "ms_restore_device.hpp"

namespace nhip {

namespace {

constexpr uint32_t RST_THREADS = 64 * MS_RESTORE_WAVES;
constexpr uint32_t SCAN = MS_RESTORE_SCAN_WIDTH;
constexpr unsigned RST_MAX_GRID = 16384;
static_assert(MS_RESTORE_TRIALS <= 64, "a lane per trial");
static_assert(MS_RESTORE_CARRY_LANES == 64, "one wave carries");

__device__ __forceinline__ uint64_t sat_add(uint64_t a, uint64_t b) {
    const uint64_t s = a + b;
    return s < a ? ~0ull : s;
}

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int lane) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, lane), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}

struct Pair {
    uint64_t a, b;
};
__device__ __forceinline__ Pair pair_add(Pair x, Pair y) { return Pair{sat_add(x.a, y.a), sat_add(x.b, y.b)}; }

// the inclusive scan of one Pair per lane of a SCAN-wide workgroup; every lane meets every barrier
__device__ __forceinline__ Pair tile_scan(Pair v, Pair* lds) {
    const uint32_t t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < SCAN; d <<= 1) {
        Pair x = lds[t];
        if (t >= d) x = pair_add(lds[t - d], x);
        __syncthreads();
        lds[t] = x;
        __syncthreads();
    }
    return lds[t];
}

}  // namespace

__global__ void __launch_bounds__(RST_THREADS) k_ms_rst_keys(MsRestoreShapeDev s) {
    const uint32_t t = threadIdx.x & 63u;
    const uint64_t b = MsJobScratch::batch_index(s.aocl_leafs);
    // wave-uniform: every lane of a wave has the same w and meets every ballot and shuffle
    for (uint64_t w = (uint64_t)blockIdx.x * MS_RESTORE_WAVES + (threadIdx.x >> 6); w < s.n; w += (uint64_t)gridDim.x * MS_RESTORE_WAVES) {
        const uint64_t li = s.leaf_index[w], mn_lo = s.minimum[2 * w], mn_hi = s.minimum[2 * w + 1];
        const bool trial = t < MS_RESTORE_TRIALS;
        uint64_t key = 0;
        const bool in_range = trial ? ms_restore_chunk(mn_lo, mn_hi, s.distances[MS_RESTORE_TRIALS * w + t], b, &key) : true;
        const bool not_in = ms_restore_not_in_aocl(li, s.aocl_leafs);
        const bool out = __ballot(!in_range) != 0;
        const uint8_t status = not_in ? NHIP_MS_NOT_IN_AOCL : out ? NHIP_MS_OUT_OF_RANGE : NHIP_MS_OK;
        const bool has = trial && status == NHIP_MS_OK && key < b;
        const unsigned long long has_mask = __ballot(has);
        bool dup = false;
        for (uint32_t j = 0; j < MS_RESTORE_TRIALS; ++j) {
            const uint64_t kj = shfl_u64(key, (int)j);
            dup |= (has_mask >> j & 1) && j < t && kj == key;
        }
        const bool keep = has && !dup;
        const unsigned long long keep_mask = __ballot(keep);
        uint32_t rank = 0;
        for (uint32_t j = 0; j < MS_RESTORE_TRIALS; ++j) {
            const uint64_t kj = shfl_u64(key, (int)j);
            rank += (keep_mask >> j & 1) && kj < key ? 1u : 0u;
        }
        if (keep) s.keys[MS_RESTORE_TRIALS * w + rank] = key;  // rank < the kept keys <= 45
        if (t == 0) {
            s.status[w] = status;
            s.entry_off[w] = (uint64_t)__popcll(keep_mask);
            s.aocl_path_off[w] = status == NHIP_MS_OK ? ms_restore_aocl_len(li, s.aocl_leafs) : 0;
        }
    }
}

// sums[2 tile], sums[2 tile + 1]: the tile's sums of a0 and a1
__global__ void __launch_bounds__(SCAN) k_ms_rst_scan_tiles(const uint64_t* __restrict__ a0, const uint64_t* __restrict__ a1,
                                                            const uint64_t* __restrict__ n_ptr, uint64_t n_val,
                                                            uint64_t* __restrict__ sums) {
    __shared__ Pair lds[SCAN];
    const uint64_t n = n_ptr ? *n_ptr : n_val, tiles = (n + SCAN - 1) / SCAN;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // workgroup-uniform
        const uint64_t i = tile * SCAN + threadIdx.x;
        const Pair v = i < n ? Pair{a0[i], a1[i]} : Pair{0, 0};
        const Pair incl = tile_scan(v, lds);
        if (threadIdx.x == SCAN - 1) sums[2 * tile] = incl.a, sums[2 * tile + 1] = incl.b;
        __syncthreads();  // lds is reused by the next tile
    }
}

// one wave: sums becomes the tiles' carries; a0[n], a1[n] and totals[0], totals[1] the totals
__global__ void __launch_bounds__(MS_RESTORE_CARRY_LANES) k_ms_rst_scan_carry(uint64_t* __restrict__ a0, uint64_t* __restrict__ a1,
                                                                              const uint64_t* __restrict__ n_ptr, uint64_t n_val,
                                                                              uint64_t* __restrict__ sums, uint64_t* __restrict__ totals) {
    const uint64_t n = n_ptr ? *n_ptr : n_val, tiles = (n + SCAN - 1) / SCAN;
    const uint64_t seg = (tiles + MS_RESTORE_CARRY_LANES - 1) / MS_RESTORE_CARRY_LANES;
    const uint32_t t = threadIdx.x;
    const uint64_t lo = t * seg < tiles ? t * seg : tiles, hi = lo + seg < tiles ? lo + seg : tiles;
    Pair mine{0, 0};
    for (uint64_t k = lo; k < hi; ++k) mine = pair_add(mine, Pair{sums[2 * k], sums[2 * k + 1]});
    Pair incl = mine;  // the wave's inclusive scan of the segment sums
    for (uint32_t d = 1; d < MS_RESTORE_CARRY_LANES; d <<= 1) {
        const int from = (int)t - (int)d;
        const Pair o{shfl_u64(incl.a, from < 0 ? 0 : from), shfl_u64(incl.b, from < 0 ? 0 : from)};
        if (from >= 0) incl = pair_add(o, incl);
    }
    const int before = (int)t - 1;
    Pair run{shfl_u64(incl.a, before < 0 ? 0 : before), shfl_u64(incl.b, before < 0 ? 0 : before)};
    if (t == 0) run = Pair{0, 0};
    for (uint64_t k = lo; k < hi; ++k) {
        const Pair v{sums[2 * k], sums[2 * k + 1]};
        sums[2 * k] = run.a, sums[2 * k + 1] = run.b;
        run = pair_add(run, v);
    }
    if (t == MS_RESTORE_CARRY_LANES - 1) {
        a0[n] = incl.a, a1[n] = incl.b;
        totals[0] = incl.a, totals[1] = incl.b;
    }
}

__global__ void __launch_bounds__(SCAN) k_ms_rst_scan_apply(uint64_t* __restrict__ a0, uint64_t* __restrict__ a1,
                                                            const uint64_t* __restrict__ n_ptr, uint64_t n_val,
                                                            const uint64_t* __restrict__ sums) {
    __shared__ Pair lds[SCAN];
    const uint64_t n = n_ptr ? *n_ptr : n_val, tiles = (n + SCAN - 1) / SCAN;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t i = tile * SCAN + threadIdx.x;
        const Pair v = i < n ? Pair{a0[i], a1[i]} : Pair{0, 0};
        const Pair incl = tile_scan(v, lds);
        const Pair carry{sums[2 * tile], sums[2 * tile + 1]};
        // exclusive: what lies before the item.  incl >= v, and a saturated incl stays saturated
        if (i < n) {
            a0[i] = sat_add(carry.a, incl.a == ~0ull ? ~0ull : incl.a - v.a);
            a1[i] = sat_add(carry.b, incl.b == ~0ull ? ~0ull : incl.b - v.b);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k_ms_rst_entries(MsRestoreShapeDev s) {
    const uint64_t b = MsJobScratch::batch_index(s.aocl_leafs), slots = MS_RESTORE_TRIALS * s.n;
    for (uint64_t x = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; x < slots; x += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t w = x / MS_RESTORE_TRIALS, j = x - MS_RESTORE_TRIALS * w;
        const uint64_t e0 = s.entry_off[w], e1 = s.entry_off[w + 1];  // the scan ran: e1 - e0 <= 45, e1 <= 45 n
        if (j >= e1 - e0) continue;
        const uint64_t key = s.keys[x], e = e0 + j;  // key < b
        s.chunk_index[e] = key;
        s.path_off[e] = ms_arch_path_len(key, b);
        s.rel_off[e] = s.tab[2 * key + 1];
    }
}

__global__ void __launch_bounds__(256) k_ms_rst_hand(MsRestoreHandDev h) {
    const uint64_t n = h.s.n, E = h.entries;
    for (uint64_t x = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; x < n + E; x += (uint64_t)gridDim.x * blockDim.x) {
        if (x < n) {
            const uint64_t w = h.w0 + x;
            if (w == 0) h.aocl_path_off[0] = 0, h.entry_off[0] = 0;
            h.aocl_path_off[w + 1] = h.base[0] + h.s.aocl_path_off[x + 1];
            h.entry_off[w + 1] = h.base[1] + h.s.entry_off[x + 1];
            if (h.leaf) {
                const uint64_t li = h.s.leaf_index[x];  // < aocl_leafs or none: every status was OK
#pragma unroll
                for (int q = 0; q < 5; ++q) h.leaf[5 * w + q] = li == MS_UPDATE_NONE ? 0 : h.aocl_nodes[5 * li + q];
            }
        } else {
            const uint64_t k = x - n, e = h.base[1] + k;
            if (e == 0) h.path_off[0] = 0, h.rel_off[0] = 0;
            h.key[e] = h.s.chunk_index[k];
            h.path_off[e + 1] = h.base[2] + h.s.path_off[k + 1];
            h.rel_off[e + 1] = h.base[3] + h.s.rel_off[k + 1];
        }
    }
}

namespace {

unsigned grid_of(uint64_t groups) { return (unsigned)(groups > RST_MAX_GRID ? RST_MAX_GRID : groups); }

// the exclusive scan of a0 and a1 in place over n items (n_ptr: the count on the device, at most n_max), totals to t
hipError_t scan_pair(uint64_t* a0, uint64_t* a1, const uint64_t* n_ptr, uint64_t n_max, uint64_t* sums, uint64_t* t,
                     hipStream_t st) {
    const uint64_t tiles = (n_max + SCAN - 1) / SCAN;
    if (tiles) hipLaunchKernelGGL(k_ms_rst_scan_tiles, dim3(grid_of(tiles)), dim3(SCAN), 0, st, a0, a1, n_ptr, n_max, sums);
    hipLaunchKernelGGL(k_ms_rst_scan_carry, dim3(1), dim3(MS_RESTORE_CARRY_LANES), 0, st, a0, a1, n_ptr, n_max, sums, t);
    if (tiles) hipLaunchKernelGGL(k_ms_rst_scan_apply, dim3(grid_of(tiles)), dim3(SCAN), 0, st, a0, a1, n_ptr, n_max, sums);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_ms_restore_shape(const MsRestoreShapeDev& s, hipStream_t st) {
    if (s.n == 0) return hipSuccess;
    const uint64_t slots = MS_RESTORE_TRIALS * s.n;
    hipLaunchKernelGGL(k_ms_rst_keys, dim3(grid_of((s.n + MS_RESTORE_WAVES - 1) / MS_RESTORE_WAVES)), dim3(RST_THREADS), 0, st, s);
    hipError_t e = scan_pair(s.aocl_path_off, s.entry_off, nullptr, s.n, s.sums, s.totals, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ms_rst_entries, dim3(grid_of((slots + 255) / 256)), dim3(256), 0, st, s);
    // totals[1], the entry count, is on the device by now; the totals of this scan go behind it
    return scan_pair(s.path_off, s.rel_off, s.entry_off + s.n, slots, s.sums, s.totals + 2, st);
}

hipError_t launch_ms_restore_hand(const MsRestoreHandDev& h, hipStream_t st) {
    const uint64_t lanes = h.s.n + h.entries;
    if (lanes == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ms_rst_hand, dim3(grid_of((lanes + 255) / 256)), dim3(256), 0, st, h);
    return hipGetLastError();
}

}  // namespace nhip
