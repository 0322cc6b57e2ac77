// A block file's mutator-set and transaction rules on the device (structs in blk_ms.hpp).
//
//  k_guesser_fee_records  BlockKernel::guesser_fee_addition_records (block_kernel.rs:47-93): one lane per (block,
//                         UTXO), lane 2 i the locked and lane 2 i + 1 the unlocked UTXO of block i.  Each lane encodes
//                         its UTXO (tx_rules.hpp), hashes it (hash_varlen, 19 or 28 words: two or three
//                         permutations) and commits: hash_pair(hash_pair(item, Block::hash), receiver_digest).
//                         Lane-per-state Tip5 as k_block_masts: a file's blocks make a few waves at the most.
//  k_blk_ms_rules         per (parent, child) pair: Block::validate rules 2.f-2.l (mod.rs:851-891; the integers are
//                         tx_rules.hpp's) and the pair's status, the first failure in the reference's order over the
//                         statuses of the guesser records and of the two apply passes.
#include "blk_ms.hpp"
#include "kernels.hpp"
#include "pow_device.hpp"

namespace nhip {

namespace {

__global__ void __launch_bounds__(64) k_guesser_fee_records(const BlkMsBlockDev* __restrict__ blk,
                                                            const uint64_t* __restrict__ digests, BlkMsParamsDev p,
                                                            uint32_t n, uint64_t* __restrict__ records,
                                                            uint8_t* __restrict__ n_records, uint8_t* __restrict__ status) {
    __shared__ Tip5Lds t5;
    tip5_lds_init(t5);
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = lane >> 1;
    const bool locked = (lane & 1u) == 0;
    if (i >= n) return;
    const uint8_t* lut = t5.lut;
    const BlkMsBlockDev& b = blk[i];
    uint64_t* out = records + 5ull * lane;
    const bool genesis = b.t.header_height == 0;  // BlockHeight::is_genesis
    const bool negative = txrules::is_negative(b.t.fee);
    if (genesis || negative) {
        for (int q = 0; q < 5; ++q) out[q] = 0;
        if (locked) {
            n_records[i] = 0;
            status[i] = genesis ? NHIP_GUESSER_OK : NHIP_GUESSER_NEGATIVE_FEE;
        }
        return;
    }
    txrules::I128 amount_locked, amount_unlocked;
    txrules::guesser_split(b.t.fee, amount_locked, amount_unlocked);
    uint64_t w[txrules::UTXO_LOCKED_WORDS];
    const int len = txrules::guesser_utxo_words(locked, locked ? amount_locked : amount_unlocked,
                                                txrules::release_date(b.t.header_timestamp), p.native_currency_hash,
                                                p.time_lock_hash, b.lock_script, w);
    uint64_t item[5], x[5], y[5];
    varlen_raw([&](uint32_t k) { return to_mont(w[k]); }, (uint32_t)len, item, lut);
    for (int q = 0; q < 5; ++q) x[q] = to_mont(digests[5ull * i + q]);
    hp_raw(item, x, y, lut);
    for (int q = 0; q < 5; ++q) x[q] = to_mont(b.receiver[q]);
    hp_raw(y, x, item, lut);
    for (int q = 0; q < 5; ++q) out[q] = from_mont(item[q]);
    if (locked) {
        n_records[i] = 2;
        status[i] = NHIP_GUESSER_OK;
    }
}

__global__ void __launch_bounds__(64) k_blk_ms_rules(BlkMsRulesDev d, BlkMsParamsDev p) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    const int64_t par = d.parent_of[i];
    uint8_t st = NHIP_BLKMS_OK, ms = NHIP_MS_OK;
    uint64_t bad = ~0ull;
    if (par < 0 || (uint64_t)par >= d.n) {  // the host refused anything but -1 and 0..n-1
        st = NHIP_BLKMS_SKIPPED;
    } else {
        const uint8_t a = d.a_status[i], b = d.b_status[i], fl = d.flags[i];
        if (b >= NHIP_MS_UNPACK_PAYLOAD_TOO_BIG && b <= NHIP_MS_UNPACK_PANIC) {
            st = NHIP_BLKMS_UNPACK;
            ms = b;
        } else if (d.guesser_status[par] != NHIP_GUESSER_OK) {
            st = NHIP_BLKMS_PARENT_NEGATIVE_FEE;
        } else if ((fl & BLKMS_FLAG_PARENT_OVERSIZE) || a != NHIP_MS_OK || b == NHIP_MS_INCONSISTENT) {
            st = NHIP_BLKMS_PARENT_MSA_INCONSISTENT;
            ms = NHIP_MS_INCONSISTENT;
        } else if (b == NHIP_MS_DUPLICATE_RECORD) {
            st = NHIP_BLKMS_REMOVAL_RECORDS_UNIQUENESS;
            ms = b;
            bad = d.b_bad[i];
        } else if (b == NHIP_MS_UPDATE_IMPOSSIBLE) {
            st = NHIP_BLKMS_UPDATE_IMPOSSIBLE;
            ms = b;
            bad = d.b_bad[i];
        } else if (b == NHIP_MS_UPDATE_MISMATCH || (b == NHIP_MS_OK && (fl & BLKMS_FLAG_EXPECTED_OVERSIZE))) {
            st = NHIP_BLKMS_UPDATE_INTEGRITY;
            ms = NHIP_MS_UPDATE_MISMATCH;
        } else if (b != NHIP_MS_OK) {  // a record's status: 2.b
            st = NHIP_BLKMS_REMOVAL_RECORDS_VALIDITY;
            ms = b;
            bad = d.b_bad[i];
        } else {
            const char c = txrules::rules_2f_2l(p.lim, d.blk[i].t);
            st = c == 'f'   ? NHIP_BLKMS_TRANSACTION_TIMESTAMP
                 : c == 'g' ? NHIP_BLKMS_COINBASE_TOO_BIG
                 : c == 'h' ? NHIP_BLKMS_NEGATIVE_COINBASE
                 : c == 'i' ? NHIP_BLKMS_NEGATIVE_FEE
                 : c == 'j' ? NHIP_BLKMS_TOO_MANY_INPUTS
                 : c == 'k' ? NHIP_BLKMS_TOO_MANY_OUTPUTS
                 : c == 'l' ? NHIP_BLKMS_TOO_MANY_ANNOUNCEMENTS
                            : NHIP_BLKMS_OK;
        }
    }
    d.status[i] = st;
    d.ms_status[i] = ms;
    d.bad_record[i] = bad;
}

unsigned blocks_for(uint64_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

}  // namespace

hipError_t launch_guesser_fee_records(const BlkMsBlockDev* d_blk, const uint64_t* d_digests, const BlkMsParamsDev& p,
                                      uint32_t n, uint64_t* d_records, uint8_t* d_n_records, uint8_t* d_status,
                                      hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_guesser_fee_records, dim3(blocks_for(2ull * n, 64)), dim3(64), 0, st, d_blk, d_digests, p, n,
                       d_records, d_n_records, d_status);
    return hipGetLastError();
}

hipError_t launch_blk_ms_rules(const BlkMsRulesDev& d, const BlkMsParamsDev& p, hipStream_t st) {
    if (d.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_blk_ms_rules, dim3(blocks_for(d.n, 64)), dim3(64), 0, st, d, p);
    return hipGetLastError();
}

}  // namespace nhip
