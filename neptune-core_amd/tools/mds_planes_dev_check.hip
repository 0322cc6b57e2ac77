// Device evaluator of the byte-planes MDS (mds_ark_planes, csrc/tip5_device.hpp) and of the round
// functions that take it as their template argument, beside tools/arith_dev_check.hip and with its
// conventions: it applies the functions to every record of a file, holds no reference arithmetic
// and compares nothing; tests/test_gpu_mds_planes.py chooses the states and checks the results
// against Python integers and the C oracle.  Stand-alone: it includes csrc/ and links no library.
//
//   mds_planes_dev_check <in.bin> <out.bin>      records of little-endian u64 words
//
// 256-thread workgroups, one lane per record, as k_hash_rows and k_mp_hash run the form: every lane
// takes its constant tiles, then the lanes without a record leave (so a wave's last records run
// with idle lanes in either lane half).
//
// Record layout (words):
//   in   raw state[16] (any 64-bit words), round (mod 5)                                    (17)
//   out  mds_ark_planes(state, round)[16]
//        tip5_permute_raw<Tip5Planes>(state mod p)[16]
//        tip5_rounds_0_3<Tip5Planes> + tip5_last_round<0, 16> (state mod p)[16]
//        tip5_hash_pair_digest<Tip5Planes>(state[0..10] mod p)[5], all raw Montgomery words    (53)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <vector>

#include "../csrc/goldilocks.hpp"
#include "../csrc/tip5_device.hpp"

using namespace nhip;

namespace {

constexpr uint32_t WG = 256, IN = 17, OUT = 53;

__device__ __forceinline__ uint64_t mod_p(uint64_t w) { return w >= GL_P ? w - GL_P : w; }

// 2 workgroups per CU at the least: at most 256 registers, the matrix results in VGPRs as in the kernels
__global__ void __launch_bounds__(WG, 2) k_planes(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, uint64_t n) {
    __shared__ Tip5Lds lds;
    tip5_lds_init(lds);
    Tip5Planes pl;
    tip5_planes_init(pl);
    const uint64_t g = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (g >= n) return;
    const uint64_t* src = in + g * IN;
    uint64_t* dst = out + g * OUT;
    uint64_t s[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) s[q] = src[q];
    mds_ark_planes(s, c_tip5_rckp_raw + (uint32_t)(src[16] % TIP5_ROUNDS) * 16, pl);
#pragma unroll
    for (int q = 0; q < 16; ++q) dst[q] = s[q];
#pragma unroll
    for (int q = 0; q < 16; ++q) s[q] = mod_p(src[q]);
    tip5_permute_raw(s, lds.lut, pl);
#pragma unroll
    for (int q = 0; q < 16; ++q) dst[16 + q] = s[q];
#pragma unroll
    for (int q = 0; q < 16; ++q) s[q] = mod_p(src[q]);
    tip5_rounds_0_3(s, lds.lut, pl);
    tip5_last_round<0, 16>(s, lds.lut);
#pragma unroll
    for (int q = 0; q < 16; ++q) dst[32 + q] = s[q];
#pragma unroll
    for (int q = 0; q < 10; ++q) s[q] = mod_p(src[q]);
#pragma unroll
    for (int q = 10; q < 16; ++q) s[q] = MONT_ONE;  // not read: the capacity is in the round-0 constants
    tip5_hash_pair_digest(s, lds.lut, pl);
#pragma unroll
    for (int q = 0; q < 5; ++q) dst[48 + q] = s[q];
}

bool hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    fprintf(stderr, "mds_planes_dev_check: %s: %s\n", what, hipGetErrorString(e));
    return false;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: mds_planes_dev_check <in.bin> <out.bin>\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 1;
    }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    const size_t rec = 8ull * IN;
    if (bytes <= 0 || (size_t)bytes % rec) {
        fprintf(stderr, "mds_planes_dev_check: %s holds no whole number of %zu-byte records\n", argv[1], rec);
        fclose(f);
        return 1;
    }
    const uint64_t n = (uint64_t)bytes / rec;
    std::vector<uint64_t> in(n * IN), out(n * OUT, 0);
    const size_t got = fread(in.data(), rec, n, f);
    fclose(f);
    if (got != n) {
        fprintf(stderr, "mds_planes_dev_check: short read of %s\n", argv[1]);
        return 1;
    }
    uint64_t *d_in = nullptr, *d_out = nullptr;
    const size_t in_bytes = in.size() * 8, out_bytes = out.size() * 8;
    if (!hip_ok(hipMalloc(&d_in, in_bytes), "hipMalloc") || !hip_ok(hipMalloc(&d_out, out_bytes), "hipMalloc") ||
        !hip_ok(hipMemcpy(d_in, in.data(), in_bytes, hipMemcpyHostToDevice), "copy in") ||
        !hip_ok(hipMemset(d_out, 0, out_bytes), "hipMemset"))
        return 1;
    hipLaunchKernelGGL(k_planes, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, 0, d_in, d_out, n);
    if (!hip_ok(hipGetLastError(), "launch") || !hip_ok(hipDeviceSynchronize(), "kernel") ||
        !hip_ok(hipMemcpy(out.data(), d_out, out_bytes, hipMemcpyDeviceToHost), "copy out"))
        return 1;
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    FILE* o = fopen(argv[2], "wb");
    if (!o) {
        perror(argv[2]);
        return 1;
    }
    const size_t put = fwrite(out.data(), 8ull * OUT, n, o);
    if (fclose(o) != 0 || put != n) {
        fprintf(stderr, "mds_planes_dev_check: short write of %s\n", argv[2]);
        return 1;
    }
    printf("%llu records\n", (unsigned long long)n);
    return 0;
}
