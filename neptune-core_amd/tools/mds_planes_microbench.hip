// The Tip5 MDS + ARK of a full round on the matrix cores as byte planes (mds_ark_planes,
// csrc/tip5_device.hpp) against the VALU form the kernels use (mds_ark_fold), one state per lane,
// 64 states per wave, both from the library's own header.  tools/mds_mfma_microbench.hip is the
// record of the earlier, rejected limb form.
//
//  1. Fragment map.  k_planes_cq writes the 10 x 16 sums C_q every lane holds after the 24
//     v_mfma_i32_32x32x32_i8; the host computes the same sums as integer dot products.  The states
//     are the 128 one-hot bytes (values 0x01 and 0xFF), states that encode their lane index, and
//     random ones, a distinct state on every lane; the A tiles are the circulant's digits
//     (asymmetric).  Any other lane-half, row or k <-> byte map than the one planes_tile_byte
//     assumes shows here.  The sums are also recombined as 128-bit integers
//     sum_q 2^(8q) C_q + 128 * 0x0101..01 * sum(M) and compared with the 128-bit MDS sum.
//  2. Both forms iterate ITERS dependent rounds (round constants of round it % 5) over the same
//     states; round 1's words and every final state must match.
//  3. Timing: each form 5 times, alternating; ns per state-MDS, VGPRs and waves per SIMD of both.
//     GO only if the slowest planes run beats the fastest VALU run.
//
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -Icsrc tools/mds_planes_microbench.hip -o build/mds_planes_mb
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "tip5_device.hpp"

using namespace nhip;
typedef unsigned __int128 u128;

#define CHECK(x)                                                             \
    do {                                                                     \
        hipError_t e_ = (x);                                                 \
        if (e_ != hipSuccess) {                                              \
            printf("%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

#ifndef MB_VALU_GROUP
#define MB_VALU_GROUP NHIP_SPONGE_MDS_GROUP
#endif

// n is a multiple of 256: every lane of every wave is active
template <int WAVES>
__global__ void __launch_bounds__(256, WAVES) k_valu(uint64_t* __restrict__ st, int iters, uint64_t* __restrict__ first) {
    const uint64_t gid = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    uint64_t x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = st[gid * 16 + i];
    int r = 0;
#pragma unroll 1
    for (int it = 0; it < iters; ++it) {
        mds_ark_fold<16, 0, 16, MB_VALU_GROUP>(x, c_tip5_rck_raw + r * 16);
        if (it == 0 && first)
#pragma unroll
            for (int i = 0; i < 16; ++i) first[gid * 16 + i] = x[i];
        r = r == 4 ? 0 : r + 1;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) st[gid * 16 + i] = x[i];
}

template <int WAVES>
__global__ void __launch_bounds__(256, WAVES) k_planes(uint64_t* __restrict__ st, int iters, uint64_t* __restrict__ first) {
    Tip5Planes pl;
    tip5_planes_init(pl);
    const uint64_t gid = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    uint64_t x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = st[gid * 16 + i];
    int r = 0;
#pragma unroll 1
    for (int it = 0; it < iters; ++it) {
        mds_ark_planes(x, c_tip5_rckp_raw + r * 16, pl);
        if (it == 0 && first)
#pragma unroll
            for (int i = 0; i < 16; ++i) first[gid * 16 + i] = x[i];
        r = r == 4 ? 0 : r + 1;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) st[gid * 16 + i] = x[i];
}

// the planes and the 24 MFMAs of mds_ark_planes alone: cq[(state * 10 + q) * 16 + i] = C_q[i]
template <int Q>
__device__ __forceinline__ void cq_store(const Tip5Planes& pl, const tip5_v4i* plane, int32_t* __restrict__ out) {
    const tip5_v16i c = planes_cq<Q>(pl, plane);
#pragma unroll
    for (int i = 0; i < 16; ++i) out[Q * 16 + i] = c[i];
    if constexpr (Q < 9) cq_store<Q + 1>(pl, plane, out);
}
__global__ void __launch_bounds__(256) k_planes_cq(const uint64_t* __restrict__ st, int32_t* __restrict__ cq) {
    Tip5Planes pl;
    tip5_planes_init(pl);
    const uint64_t gid = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    tip5_v4i plane[8];
#pragma unroll
    for (int d = 0; d < 8; ++d)
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            uint32_t w = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) w |= (uint32_t)(uint8_t)((st[gid * 16 + 4 * m + b] >> (8 * d)) ^ 0x80u) << (8 * b);
            plane[d][m] = (int)w;
        }
    cq_store<0>(pl, plane, cq + gid * 160);
}

static u128 mds_sum(const uint64_t* x, int i) {
    u128 s = 0;
    for (int j = 0; j < 16; ++j) s += (u128)TIP5_MDS[(i - j) & 15] * x[j];
    return s;
}

template <typename K>
static void report(const char* name, K kern) {
    hipFuncAttributes a;
    CHECK(hipFuncGetAttributes(&a, (const void*)kern));
    int blocks = 0;
    CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, (const void*)kern, 256, 0));
    printf("%-14s VGPRs %3d  scratch %zu B  waves per SIMD %d\n", name, a.numRegs, (size_t)a.localSizeBytes, blocks);
}

#ifndef MB_VALU_WAVES
#define MB_VALU_WAVES 1
#endif
#ifndef MB_PLANES_WAVES
#define MB_PLANES_WAVES 1
#endif

int main(int argc, char** argv) {
    const int iters = argc > 1 ? std::atoi(argv[1]) : 200;
    const int blocks = std::max(16, argc > 2 ? std::atoi(argv[2]) : 256 * 8 * 4);  // workgroups of 4 waves
    const size_t nstates = (size_t)blocks * 256;
    std::mt19937_64 g(5);
    std::vector<uint64_t> h(nstates * 16);
    for (auto& w : h) w = g() % GL_P;
    size_t s = 0;
    auto fill = [&](uint64_t f) {
        for (int i = 0; i < 16; ++i) h[s * 16 + i] = f;
        ++s;
    };
    fill(0), fill(~0ull), fill(0x8080808080808080ull), fill(0x7F7F7F7F7F7F7F7Full), fill(GL_P - 1);
    for (uint64_t v : {0x01ull, 0xFFull})  // one-hot bytes
        for (int b = 0; b < 128; ++b) {
            fill(0);
            h[(s - 1) * 16 + (b >> 3)] = v << (8 * (b & 7));
        }
    for (int l = 0; l < 256; ++l) {  // lane index in every word, then in one word
        for (int i = 0; i < 16; ++i) h[s * 16 + i] = ((uint64_t)((s & 63) + 1) << 56) | ((uint64_t)i << 8) | (s & 63);
        ++s;
    }
    for (int l = 0; l < 256; ++l) {
        fill(0);
        h[(s - 1) * 16 + ((s - 1) & 15)] = ((s - 1) & 63) * 0x0101010101010101ull + 1;
    }
    uint64_t *d0, *d1, *f0, *f1;
    int32_t* dcq;
    const size_t ncq = std::min<size_t>(nstates, 4096);
    CHECK(hipMalloc(&d0, nstates * 128));
    CHECK(hipMalloc(&d1, nstates * 128));
    CHECK(hipMalloc(&f0, nstates * 128));
    CHECK(hipMalloc(&f1, nstates * 128));
    CHECK(hipMalloc(&dcq, ncq * 160 * 4));
    auto reset = [&]() {
        CHECK(hipMemcpy(d0, h.data(), nstates * 128, hipMemcpyHostToDevice));
        CHECK(hipMemcpy(d1, h.data(), nstates * 128, hipMemcpyHostToDevice));
    };
    reset();
    // 1. fragment map and the 128-bit sums
    k_planes_cq<<<dim3(ncq / 256), dim3(256)>>>(d1, dcq);
    CHECK(hipDeviceSynchronize());
    std::vector<int32_t> cq(ncq * 160);
    CHECK(hipMemcpy(cq.data(), dcq, cq.size() * 4, hipMemcpyDeviceToHost));
    size_t bad_cq = 0, bad_128 = 0;
    const u128 off = (u128)0x8080808080808080ull * planes_mds_sum();
    for (size_t n = 0; n < ncq; ++n) {
        const uint64_t* x = &h[n * 16];
        for (int i = 0; i < 16; ++i) {
            __int128 sum = (__int128)off;
            for (int q = 0; q < 10; ++q) {
                int32_t want = 0;
                for (int e = 0; e < 3; ++e) {
                    const int d = q - e;
                    if (d < 0 || d > 7) continue;
                    for (int j = 0; j < 16; ++j)
                        want += mds_digit((i - j) & 15, e) * (int)(int8_t)(uint8_t)((x[j] >> (8 * d)) ^ 0x80u);
                }
                const int32_t got = cq[(n * 10 + q) * 16 + i];
                if (got != want && bad_cq++ < 8) printf("C_%d[%d] of state %zu (lane %zu): %d, want %d\n", q, i, n, n & 63, got, want);
                sum += (__int128)got << (8 * q);
            }
            bad_128 += (u128)sum != mds_sum(x, i);
        }
    }
    printf("fragment map: %zu states, C_q mismatches %zu, 128-bit sum mismatches %zu\n", ncq, bad_cq, bad_128);
    // 2. the two forms
    k_valu<MB_VALU_WAVES><<<dim3(blocks), dim3(256)>>>(d0, iters, f0);
    k_planes<MB_PLANES_WAVES><<<dim3(blocks), dim3(256)>>>(d1, iters, f1);
    CHECK(hipDeviceSynchronize());
    std::vector<uint64_t> a(nstates * 16), b(nstates * 16), sa(nstates * 16), sb(nstates * 16);
    CHECK(hipMemcpy(a.data(), f0, nstates * 128, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(b.data(), f1, nstates * 128, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(sa.data(), d0, nstates * 128, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(sb.data(), d1, nstates * 128, hipMemcpyDeviceToHost));
    size_t bad_first = 0, bad_final = 0, bad_host = 0;
    for (size_t i = 0; i < a.size(); ++i) bad_first += a[i] != b[i];
    for (size_t i = 0; i < sa.size(); ++i) bad_final += sa[i] != sb[i];
    for (size_t n = 0; n < ncq; ++n)  // round 1 against the host: (sum + rc) mod p, canonical
        for (int i = 0; i < 16; ++i)
            bad_host += b[n * 16 + i] != (uint64_t)((mds_sum(&h[n * 16], i) + TIP5_RC_RAW[i]) % GL_P);
    printf("round 1 mismatches %zu, final state mismatches %zu, round 1 against the host %zu\n", bad_first, bad_final, bad_host);
    report("valu", k_valu<MB_VALU_WAVES>);
    report("planes", k_planes<MB_PLANES_WAVES>);
    // 3. timing
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    const double mds = (double)nstates * iters;
    float vmin = 1e30f, vmax = 0, pmin = 1e30f, pmax = 0;
    for (int rep = 0; rep < 6; ++rep) {  // rep 0 warms up
        float ms;
        CHECK(hipEventRecord(e0));
        k_valu<MB_VALU_WAVES><<<dim3(blocks), dim3(256)>>>(d0, iters, nullptr);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (rep) vmin = std::min(vmin, ms), vmax = std::max(vmax, ms), printf("run %d valu   %.4f ms  %.5f ns per state-MDS\n", rep, ms, ms * 1e6 / mds);
        CHECK(hipEventRecord(e0));
        k_planes<MB_PLANES_WAVES><<<dim3(blocks), dim3(256)>>>(d1, iters, nullptr);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (rep) pmin = std::min(pmin, ms), pmax = std::max(pmax, ms), printf("run %d planes %.4f ms  %.5f ns per state-MDS\n", rep, ms, ms * 1e6 / mds);
    }
    const bool ok = !(bad_cq || bad_128 || bad_first || bad_final || bad_host);
    const bool go = ok && pmax < vmin;
    printf("{\"states\": %zu, \"iters\": %d, \"correct\": %s, \"valu_ns_min\": %.5f, \"valu_ns_max\": %.5f, "
           "\"planes_ns_min\": %.5f, \"planes_ns_max\": %.5f, \"planes_slowest_over_valu_fastest\": %.3f, \"gate\": \"%s\"}\n",
           nstates, iters, ok ? "true" : "false", vmin * 1e6 / mds, vmax * 1e6 / mds, pmin * 1e6 / mds, pmax * 1e6 / mds,
           pmax / vmin, go ? "GO" : "NO-GO");
    return ok ? 0 : 1;
}
