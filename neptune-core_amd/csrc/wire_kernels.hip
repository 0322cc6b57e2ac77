// Wire bytes -> aligned field words on the device (the in-place feed path).
//
// bincode's Vec<BFieldElement> is 8-byte little-endian words at whatever byte offset the message puts
// them (transfer_transaction.rs:31-47, import_blocks_from_files.rs:100-115), while every STARK kernel
// indexes an 8-byte-aligned word buffer through ProofIn.off.  k_wire_words gathers each proof's words
// out of the raw bytes, at any byte shift, into the batch word buffer: output word k of proof i is the
// little-endian u64 at raw byte boff[i] + 8k, reduced once mod p (BFieldElement::new; the device
// counterpart of nhip_le_words / copy_le_words_nt, bit for bit).
//
// Loads: the 16-byte-aligned 16 bytes the wanted 8 start in and the 8 bytes after them (both naturally
// aligned), then a dword select and v_alignbyte_b32 per output dword (byte shift 0..3, so a shift of 0
// is a plain move and no 64-bit shift by 64 exists).  Neighbouring lanes read the same lines, so a wave
// fetches each raw line once.  The aligned loads reach at most 15 bytes before the first wanted byte
// and 16 bytes past the last: the caller keeps `raw` inside an allocation with that much room (a
// 16-byte-aligned base below, and WIRE_TAIL_PAD bytes above).  Stores: one 8-byte store per lane, consecutive lanes consecutive words;
// ProofIn.off may be odd, so nothing wider is aligned in general.
//
// Mixed lengths in one launch: a flat index over the batch's proof words (the proofs lie back to back
// from word 0 in ProofIn order); each workgroup takes WIRE_TILE consecutive words, binary-searches the
// proof of its first word in the `off` prefix sums (uniform over the workgroup), and its lanes walk on
// from there.  Zero-length proofs share their successor's `off` and are stepped over.
#include <hip/hip_runtime.h>

#include "goldilocks.hpp"
#include "kernels.hpp"

namespace nhip {

namespace {

constexpr uint32_t WIRE_BLOCK = 256;
constexpr uint32_t WIRE_PER_LANE = 4;
constexpr uint32_t WIRE_TILE = WIRE_BLOCK * WIRE_PER_LANE;

__global__ void __launch_bounds__(WIRE_BLOCK) k_wire_words(const uint8_t* __restrict__ raw,
                                                           const uint64_t* __restrict__ boff,
                                                           const ProofIn* __restrict__ in, uint32_t n, uint64_t total,
                                                           uint64_t* __restrict__ words) {
    const uint64_t tile = (uint64_t)blockIdx.x * WIRE_TILE;
    if (n == 0 || tile >= total) return;
    // the last proof whose first word is at or before the tile's (in[0].off == 0 <= tile)
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (in[mid].off <= tile) lo = mid;
        else hi = mid;
    }
    uint32_t i = lo;
    for (uint32_t j = 0; j < WIRE_PER_LANE; ++j) {
        const uint64_t w = tile + (uint64_t)j * WIRE_BLOCK + threadIdx.x;
        if (w >= total) return;
        while (i + 1 < n && in[i + 1].off <= w) ++i;
        const uint64_t k = w - in[i].off;
        if (k >= in[i].len) continue;  // a gap in the layout: nothing of this proof, nothing written
        const uintptr_t a = (uintptr_t)raw + boff[i] + 8 * k;
        const uintptr_t base = a & ~(uintptr_t)15;
        const uint4 q0 = *(const uint4*)base;         // 16 bytes at a 16-byte boundary
        const uint2 q1 = *(const uint2*)(base + 16);  // the next 8, at a 16-byte boundary too
        const uint32_t s = (uint32_t)a & 15u;
        const uint32_t t = s >> 2;  // the dword of the 24 bytes the wanted 8 start in
        const uint32_t d0 = t == 0 ? q0.x : t == 1 ? q0.y : t == 2 ? q0.z : q0.w;
        const uint32_t d1 = t == 0 ? q0.y : t == 1 ? q0.z : t == 2 ? q0.w : q1.x;
        const uint32_t d2 = t == 0 ? q0.z : t == 1 ? q0.w : t == 2 ? q1.x : q1.y;
        const uint32_t lo32 = __builtin_amdgcn_alignbyte(d1, d0, s & 3u);
        const uint32_t hi32 = __builtin_amdgcn_alignbyte(d2, d1, s & 3u);
        const uint64_t v = ((uint64_t)hi32 << 32) | lo32;
        words[w] = v >= GL_P ? v - GL_P : v;
    }
}

}  // namespace

hipError_t launch_wire_words(const uint8_t* d_raw, const uint64_t* d_boff, const ProofIn* d_in, uint32_t n,
                             uint64_t total_words, uint64_t* d_words, hipStream_t st) {
    if (n == 0 || total_words == 0) return hipSuccess;
    const uint64_t blocks = (total_words + WIRE_TILE - 1) / WIRE_TILE;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_wire_words, dim3((unsigned)blocks), dim3(WIRE_BLOCK), 0, st, d_raw, d_boff, d_in, n,
                       total_words, d_words);
    return hipGetLastError();
}

}  // namespace nhip
