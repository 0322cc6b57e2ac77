// Device evaluator of the arithmetic headers (goldilocks.hpp, xfe.hpp, tip5_device.hpp, chain_rules.hpp):
// applies one op to every fixed-size record of a file and writes one output record per input record.
// It holds no reference arithmetic and compares nothing; tests/test_gpu_arith_edges.py and
// tests/test_arith_edges_host.py choose the operands and check the results against Python integers,
// the C oracle and tests/block_chain_ref.py.  Stand-alone: it includes csrc/ and links no library.
//
//   arith_dev_check list                               op names, record sizes in 64-bit words, "host" where
//                                                      --host is offered (no HIP call)
//   arith_dev_check [--host] <op> <in.bin> <out.bin>   records of little-endian u64 words; 32-bit limbs and
//                                                      flags take one word each
//
// Device path: 256-thread workgroups, one lane per record (tip5: also one 16-lane row, one row pair and
// one quad per record; a row, pair or quad without a record leaves as a whole).  --host runs the host
// instantiation of the ops whose functions are __host__ __device__.
//
// Record layouts (words):
//   bfe     in  a b                                             (2)
//           out mont_mul mont_mul_lat mont_mul_sel<true> mont_mul_sel<false> gl_add gl_sub to_mont(a)
//               to_mont_mul(a) from_mont(a) montyred(a, b) reduce96(a, (uint32_t)b)                     (11)
//   mul3    in  a0 b0 a1 b1 a2 b2 x[12]                         (18)
//           out mont_mul_n_dev<3>[3] pow7_12(x)[12] pow7(x[i])[12]                                      (27)
//   mdsred  in  al ah k (round-constant index, taken mod 80)    (3)
//           out mds_reduce_fold(al + rck[k], ah)  mds_reduce_ark_lat(al, ah, -(p - rc[k]))              (2)
//   mds16   in  s[16] round (mod 5)                             (17)
//           out mds_ark<NHIP_SPONGE_MDS_GROUP>[16] mds_ark<NHIP_PAIR_MDS_GROUP>[16]
//               mds_ark_fold<16,0,5>[5] mds_ark_fold<16,10,16>[6]                                       (43)
//   xfe     in  a[3] b[3] e                                     (7)
//           out x_mul[3] x_add[3] x_sub[3] x_scale(a, b.c0)[3] x_inv(a)[3] b_inv(a.c0) b_pow(a.c0, e)
//               x_pow(a, e)[3]                                                                          (20)
//   bary    in  t[3] L (1..512) codeword[512][3]                (1540)
//           out num[3] den[3] zero-flag: bary_slot over every slot, the root w of order 2^ceil(log2 L) (7)
//   tip5    in  canonical state[16]                             (16)
//           out tip5_permute_raw[16] tip5_permute_wide<false>[16] tip5_permute_wide<true>[16]
//               tip5_permute_pair[16] tip5_permute_quad[16] tip5_rounds_0_3 + tip5_last_round<0,16>[16]
//               tip5_hash_pair_digest(state[0..10])[5], all canonical                                   (101)
//   chain   in  difficulty[5] pow[6] new_ts old_ts interval previous_height reset_interval now
//               minimum_block_time child_difficulty[5] child_pow[6] child_height genesis_difficulty[5] (35)
//           out difficulty_target[5] flag  difficulty_control[5] flag  pow_add[6]  difficulty_new[5]
//               should_reset_difficulty  gl_add(new_ts, old_ts)  gl_sub(new_ts, old_ts)
//               height_next(previous_height)  rule_0a  rules_0d_0g (0, 'd', 'e', 'f', 'g')              (29)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../csrc/chain_rules.hpp"
#include "../csrc/goldilocks.hpp"
#include "../csrc/tip5_device.hpp"
#include "../csrc/xfe.hpp"

using namespace nhip;

namespace {

constexpr uint32_t WG = 256;
constexpr uint32_t BARY_LMAX = 512;

// ---------------------------------------------------------------- one lane per record
struct OpBfe {
    static constexpr uint32_t IN = 2, OUT = 11;
    __host__ __device__ static void apply(const uint64_t* in, uint64_t* out) {
        const uint64_t a = in[0], b = in[1];
        out[0] = mont_mul(a, b);
        out[1] = mont_mul_lat(a, b);
#if defined(__HIP_DEVICE_COMPILE__)
        out[2] = mont_mul_sel<true>(a, b);
        out[3] = mont_mul_sel<false>(a, b);
#else  // mont_mul_sel is device-only; the host path repeats the two forms it selects between
        out[2] = mont_mul_lat(a, b);
        out[3] = mont_mul(a, b);
#endif
        out[4] = gl_add(a, b);
        out[5] = gl_sub(a, b);
        out[6] = to_mont(a);
        out[7] = to_mont_mul(a);
        out[8] = from_mont(a);
        out[9] = montyred(a, b);
        out[10] = reduce96(a, (uint32_t)b);
    }
};

struct OpMul3 {
    static constexpr uint32_t IN = 18, OUT = 27;
    __device__ static void apply(const uint64_t* in, uint64_t* out) {
        uint64_t a[3], b[3], r[3], x[12];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            a[i] = in[2 * i];
            b[i] = in[2 * i + 1];
        }
        mont_mul_n_dev<3>(a, b, r);
#pragma unroll
        for (int i = 0; i < 3; ++i) out[i] = r[i];
#pragma unroll
        for (int i = 0; i < 12; ++i) x[i] = in[6 + i];
        pow7_12(x);
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            out[3 + i] = x[i];
            out[15 + i] = pow7(in[6 + i]);
        }
    }
};

struct OpMdsRed {
    static constexpr uint32_t IN = 3, OUT = 2;
    __device__ static void apply(const uint64_t* in, uint64_t* out) {
        const uint64_t al = in[0], ah = in[1];
        const uint32_t k = (uint32_t)(in[2] % 80u);
        out[0] = mds_reduce_fold(al + c_tip5_rck_raw[k], ah);
        out[1] = mds_reduce_ark_lat(al, ah, 0ull - (GL_P - c_tip5_rc_raw[k]));
    }
};

struct OpMds16 {
    static constexpr uint32_t IN = 17, OUT = 43;
    __device__ static void apply(const uint64_t* in, uint64_t* out) {
        const uint32_t r = (uint32_t)(in[16] % TIP5_ROUNDS);
        const uint64_t* rc = c_tip5_rc_raw + r * 16;
        const uint64_t* rck = c_tip5_rck_raw + r * 16;
        uint64_t s[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = in[i];
        mds_ark<NHIP_SPONGE_MDS_GROUP>(s, rc, rck);
#pragma unroll
        for (int i = 0; i < 16; ++i) out[i] = s[i];
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = in[i];
        mds_ark<NHIP_PAIR_MDS_GROUP>(s, rc, rck);
#pragma unroll
        for (int i = 0; i < 16; ++i) out[16 + i] = s[i];
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = in[i];
        mds_ark_fold<16, 0, 5>(s, rck);
#pragma unroll
        for (int i = 0; i < 5; ++i) out[32 + i] = s[i];
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = in[i];
        mds_ark_fold<16, 10, 16>(s, rck);
#pragma unroll
        for (int i = 0; i < 6; ++i) out[37 + i] = s[10 + i];
    }
};

__host__ __device__ inline void put_xfe(uint64_t* out, Xfe x) {
    out[0] = x.c0;
    out[1] = x.c1;
    out[2] = x.c2;
}

struct OpXfe {
    static constexpr uint32_t IN = 7, OUT = 20;
    __host__ __device__ static void apply(const uint64_t* in, uint64_t* out) {
        const Xfe a = {in[0], in[1], in[2]}, b = {in[3], in[4], in[5]};
        const uint64_t e = in[6];
        put_xfe(out, x_mul(a, b));
        put_xfe(out + 3, x_add(a, b));
        put_xfe(out + 6, x_sub(a, b));
        put_xfe(out + 9, x_scale(a, b.c0));
        put_xfe(out + 12, x_inv(a));
        out[15] = b_inv(a.c0);
        out[16] = b_pow(a.c0, e);
        put_xfe(out + 17, x_pow(a, e));
    }
};

struct OpBary {
    static constexpr uint32_t IN = 4 + 3 * BARY_LMAX, OUT = 7;
    __host__ __device__ static void apply(const uint64_t* in, uint64_t* out) {
        for (uint32_t i = 0; i < OUT; ++i) out[i] = 0;
        const Xfe t = {in[0], in[1], in[2]};
        if (in[3] == 0 || in[3] > BARY_LMAX) return;
        const uint32_t L = (uint32_t)in[3];
        uint32_t log2L = 0;
        while ((1u << log2L) < L) ++log2L;
        // w^(2^j) for the root w of order 2^log2L, as the FRI kernel stages it (the last entry is 1)
        uint64_t wsq[12];
        for (uint32_t j = 0; j <= log2L; ++j) wsq[j] = root_of_unity(log2L - j);
        const uint32_t ppl = bary_points_per_lane(L), S = (L + ppl - 1) / ppl;
        const uint64_t wS = lds_pow(wsq, S);  // L a power of two: the root of order ppl
        const uint64_t* cwp = in + 4;
        auto cw = [&](uint32_t i) { return Xfe{cwp[3 * i], cwp[3 * i + 1], cwp[3 * i + 2]}; };
        Xfe num = x_zero(), den = x_zero();
        bool zero = false;
        for (uint32_t s = 0; s < S; ++s)
            if (bary_slot(t, lds_pow(wsq, s), wS, s, S, L, ppl, cw, num, den)) zero = true;
        put_xfe(out, num);
        put_xfe(out + 3, den);
        out[6] = zero ? 1 : 0;
    }
};

struct OpChain {
    static constexpr uint32_t IN = 35, OUT = 29;
    __host__ __device__ static void apply(const uint64_t* in, uint64_t* out) {
        chain::LinkHeader parent, child;
        chain::LinkParams np;
        for (int i = 0; i < 5; ++i) parent.difficulty[i] = (uint32_t)in[i];
        for (int i = 0; i < 6; ++i) parent.cumulative_proof_of_work[i] = (uint32_t)in[5 + i];
        const uint64_t new_ts = in[11], old_ts = in[12], interval = in[13], prev_height = in[14];
        parent.height = prev_height;
        parent.timestamp = old_ts;
        np.target_block_interval = interval;
        np.difficulty_reset_interval = in[15];
        np.now = in[16];
        np.minimum_block_time = in[17];
        for (int i = 0; i < 5; ++i) child.difficulty[i] = (uint32_t)in[18 + i];
        for (int i = 0; i < 6; ++i) child.cumulative_proof_of_work[i] = (uint32_t)in[23 + i];
        child.height = in[29];
        child.timestamp = new_ts;
        for (int i = 0; i < 5; ++i) np.genesis_difficulty[i] = (uint32_t)in[30 + i];

        uint64_t target[5];
        out[5] = chain::difficulty_target(parent.difficulty, target) ? 1 : 0;
        for (int i = 0; i < 5; ++i) out[i] = target[i];
        uint32_t ctl[5];
        out[11] = chain::difficulty_control(new_ts, old_ts, parent.difficulty, interval, prev_height, ctl) ? 1 : 0;
        for (int i = 0; i < 5; ++i) out[6 + i] = ctl[i];
        uint32_t sum[6];
        chain::pow_add(parent.cumulative_proof_of_work, parent.difficulty, sum);
        for (int i = 0; i < 6; ++i) out[12 + i] = sum[i];
        uint32_t dn[5];
        for (int i = 0; i < 5; ++i) dn[i] = parent.difficulty[i];
        chain::difficulty_new(dn);
        for (int i = 0; i < 5; ++i) out[18 + i] = dn[i];
        out[23] = chain::should_reset_difficulty(np.difficulty_reset_interval, new_ts, old_ts) ? 1 : 0;
        out[24] = chain::gl_add(new_ts, old_ts);
        out[25] = chain::gl_sub(new_ts, old_ts);
        out[26] = chain::height_next(prev_height);
        out[27] = chain::rule_0a(parent, child) ? 1 : 0;
        out[28] = (uint64_t)(unsigned char)chain::rules_0d_0g(np, parent, child);
    }
};

template <class Op>
__global__ void __launch_bounds__(WG) k_records(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    Op::apply(in + i * Op::IN, out + i * Op::OUT);
}

template <class Op>
void host_records(const uint64_t* in, uint64_t* out, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) Op::apply(in + i * Op::IN, out + i * Op::OUT);
}

// ---------------------------------------------------------------- tip5: every form of the permutation
constexpr uint32_t T5_IN = 16, T5_OUT = 101;
constexpr uint32_t T5_RAW = 0, T5_WIDE = 16, T5_WIDE_LAT = 32, T5_PAIR = 48, T5_QUAD = 64, T5_SPLIT = 80, T5_DIGEST = 96;

__global__ void __launch_bounds__(WG) k_tip5_lane(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, uint64_t n) {
    __shared__ Tip5Lds lds;
    tip5_lds_init(lds);
    const uint64_t g = (uint64_t)blockIdx.x * WG + threadIdx.x;
    if (g >= n) return;
    const uint64_t* src = in + g * T5_IN;
    uint64_t* dst = out + g * T5_OUT;
    uint64_t s[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) s[q] = to_mont(src[q]);
    tip5_permute_raw(s, lds.lut);
#pragma unroll
    for (int q = 0; q < 16; ++q) dst[T5_RAW + q] = from_mont(s[q]);
#pragma unroll
    for (int q = 0; q < 16; ++q) s[q] = to_mont(src[q]);
    tip5_rounds_0_3(s, lds.lut);
    tip5_last_round<0, 16>(s, lds.lut);
#pragma unroll
    for (int q = 0; q < 16; ++q) dst[T5_SPLIT + q] = from_mont(s[q]);
#pragma unroll
    for (int q = 0; q < 10; ++q) s[q] = to_mont(src[q]);
#pragma unroll
    for (int q = 10; q < 16; ++q) s[q] = MONT_ONE;  // not read: the capacity is in the round-0 constants
    tip5_hash_pair_digest(s, lds.lut);
#pragma unroll
    for (int q = 0; q < 5; ++q) dst[T5_DIGEST + q] = from_mont(s[q]);
}

// one record per 16-lane row (PAIR: per two rows, both holding the state, row 0 writing)
template <bool PAIR, bool LAT>
__global__ void __launch_bounds__(WG) k_tip5_rows(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, uint64_t n,
                                                  uint32_t off) {
    __shared__ Tip5Lds lds;
    tip5_lds_init(lds);
    constexpr uint32_t LANES = PAIR ? 32u : 16u;
    const uint32_t e = threadIdx.x & 15u;
    const uint32_t h = PAIR ? (threadIdx.x >> 4) & 1u : 0u;
    const uint64_t g = ((uint64_t)blockIdx.x * WG + threadIdx.x) / LANES;
    if (g >= n) return;  // the whole row or pair
    uint64_t rc[TIP5_ROUNDS];
#pragma unroll
    for (int r = 0; r < TIP5_ROUNDS; ++r) rc[r] = c_tip5_rc_raw[r * 16 + e];
    uint32_t cm[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) cm[j] = h ? TIP5_MDS[j + 8] : TIP5_MDS[j];
    uint64_t s = to_mont(in[g * T5_IN + e]);
    if constexpr (PAIR) s = tip5_permute_pair(s, e, h, rc, cm, lds.lut);
    else s = tip5_permute_wide<LAT>(s, e, rc, lds.lut);
    if (h == 0) out[g * T5_OUT + off + e] = from_mont(s);
}

// one record per quad: lane e holds words e, e + 4, e + 8, e + 12
__global__ void __launch_bounds__(WG) k_tip5_quad(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, uint64_t n) {
    __shared__ Tip5Lds lds;
    __shared__ uint64_t rck[80];
    for (int i = threadIdx.x; i < 80; i += blockDim.x) rck[i] = c_tip5_rck_raw[i];
    tip5_lds_init(lds);  // (its barrier also orders the rck stores)
    const uint32_t e = threadIdx.x & 3u;
    const uint64_t g = ((uint64_t)blockIdx.x * WG + threadIdx.x) >> 2;
    if (g >= n) return;  // the whole quad
    uint32_t cq[3][4];
    tip5_quad_coefs(e, cq);
    uint64_t s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = to_mont(in[g * T5_IN + e + 4 * k]);
    tip5_permute_quad(s, cq, rck, e, lds.lut);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[g * T5_OUT + T5_QUAD + e + 4 * k] = from_mont(s[k]);
}

unsigned grid_for(uint64_t lanes) { return (unsigned)((lanes + WG - 1) / WG); }

void launch_tip5(const uint64_t* in, uint64_t* out, uint64_t n) {
    hipLaunchKernelGGL(k_tip5_lane, dim3(grid_for(n)), dim3(WG), 0, 0, in, out, n);
    hipLaunchKernelGGL((k_tip5_rows<false, false>), dim3(grid_for(16 * n)), dim3(WG), 0, 0, in, out, n, T5_WIDE);
    hipLaunchKernelGGL((k_tip5_rows<false, true>), dim3(grid_for(16 * n)), dim3(WG), 0, 0, in, out, n, T5_WIDE_LAT);
    hipLaunchKernelGGL((k_tip5_rows<true, true>), dim3(grid_for(32 * n)), dim3(WG), 0, 0, in, out, n, T5_PAIR);
    hipLaunchKernelGGL(k_tip5_quad, dim3(grid_for(4 * n)), dim3(WG), 0, 0, in, out, n);
}

template <class Op>
void launch_records(const uint64_t* in, uint64_t* out, uint64_t n) {
    hipLaunchKernelGGL(k_records<Op>, dim3(grid_for(n)), dim3(WG), 0, 0, in, out, n);
}

// ---------------------------------------------------------------- driver
struct OpEntry {
    const char* name;
    uint32_t in_words, out_words;
    void (*device)(const uint64_t*, uint64_t*, uint64_t);
    void (*host)(const uint64_t*, uint64_t*, uint64_t);  // null: device only
};

const OpEntry OPS[] = {
    {"bfe", OpBfe::IN, OpBfe::OUT, launch_records<OpBfe>, host_records<OpBfe>},
    {"mul3", OpMul3::IN, OpMul3::OUT, launch_records<OpMul3>, nullptr},
    {"mdsred", OpMdsRed::IN, OpMdsRed::OUT, launch_records<OpMdsRed>, nullptr},
    {"mds16", OpMds16::IN, OpMds16::OUT, launch_records<OpMds16>, nullptr},
    {"xfe", OpXfe::IN, OpXfe::OUT, launch_records<OpXfe>, host_records<OpXfe>},
    {"bary", OpBary::IN, OpBary::OUT, launch_records<OpBary>, host_records<OpBary>},
    {"tip5", T5_IN, T5_OUT, launch_tip5, nullptr},
    {"chain", OpChain::IN, OpChain::OUT, launch_records<OpChain>, host_records<OpChain>},
};

int usage() {
    fprintf(stderr, "usage: arith_dev_check list | arith_dev_check [--host] <op> <in.bin> <out.bin>\n");
    return 2;
}

bool hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    fprintf(stderr, "arith_dev_check: %s: %s\n", what, hipGetErrorString(e));
    return false;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "list")) {
        for (const OpEntry& op : OPS) printf("%s %u %u%s\n", op.name, op.in_words, op.out_words, op.host ? " host" : "");
        return 0;
    }
    const bool on_host = argc == 5 && !strcmp(argv[1], "--host");
    if (argc != (on_host ? 5 : 4)) return usage();
    char** arg = argv + (on_host ? 2 : 1);
    const OpEntry* op = nullptr;
    for (const OpEntry& o : OPS)
        if (!strcmp(o.name, arg[0])) op = &o;
    if (!op) return usage();
    if (on_host && !op->host) {
        fprintf(stderr, "arith_dev_check: %s is device only\n", op->name);
        return 2;
    }
    FILE* f = fopen(arg[1], "rb");
    if (!f) {
        perror(arg[1]);
        return 1;
    }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    const size_t rec = 8ull * op->in_words;
    if (bytes <= 0 || (size_t)bytes % rec) {
        fprintf(stderr, "arith_dev_check: %s holds no whole number of %zu-byte records\n", arg[1], rec);
        fclose(f);
        return 1;
    }
    const uint64_t n = (uint64_t)bytes / rec;
    std::vector<uint64_t> in(n * op->in_words), out(n * op->out_words, 0);
    const size_t got = fread(in.data(), rec, n, f);
    fclose(f);
    if (got != n) {
        fprintf(stderr, "arith_dev_check: short read of %s\n", arg[1]);
        return 1;
    }
    if (on_host) {
        op->host(in.data(), out.data(), n);
    } else {
        uint64_t *d_in = nullptr, *d_out = nullptr;
        const size_t in_bytes = in.size() * 8, out_bytes = out.size() * 8;
        if (!hip_ok(hipMalloc(&d_in, in_bytes), "hipMalloc") || !hip_ok(hipMalloc(&d_out, out_bytes), "hipMalloc") ||
            !hip_ok(hipMemcpy(d_in, in.data(), in_bytes, hipMemcpyHostToDevice), "copy in") ||
            !hip_ok(hipMemset(d_out, 0, out_bytes), "hipMemset"))
            return 1;
        op->device(d_in, d_out, n);
        if (!hip_ok(hipGetLastError(), "launch") || !hip_ok(hipDeviceSynchronize(), "kernel") ||
            !hip_ok(hipMemcpy(out.data(), d_out, out_bytes, hipMemcpyDeviceToHost), "copy out"))
            return 1;
        (void)hipFree(d_in);
        (void)hipFree(d_out);
    }
    FILE* o = fopen(arg[2], "wb");
    if (!o) {
        perror(arg[2]);
        return 1;
    }
    const size_t put = fwrite(out.data(), 8ull * op->out_words, n, o);
    if (fclose(o) != 0 || put != n) {
        fprintf(stderr, "arith_dev_check: short write of %s\n", arg[2]);
        return 1;
    }
    printf("%s %llu records%s\n", op->name, (unsigned long long)n, on_host ? " (host)" : "");
    return 0;
}
