// A block file's mutator-set and transaction rules: what blk_ms_capi.hip stages and
// blk_ms_kernels.hip reads.  Canonical words throughout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tx_rules.hpp"

namespace nhip {

// What the guesser-fee records and rules 2.f-2.l read of one scanned block (the walk's integers)
struct BlkMsBlockDev {
    uint64_t receiver[5], lock_script[5];
    txrules::TxFacts t;
};

struct BlkMsParamsDev {
    uint64_t native_currency_hash[5], time_lock_hash[5];
    txrules::TxLimits lim;
};

// per pair, decided by nothing but the walk's counts: an accumulator with more than 64 serialized peaks
constexpr uint8_t BLKMS_FLAG_PARENT_OVERSIZE = 1, BLKMS_FLAG_EXPECTED_OVERSIZE = 2;

// every pointer a device pointer
struct BlkMsRulesDev {
    const BlkMsBlockDev* blk;
    const int64_t* parent_of;
    const uint8_t* guesser_status;  // per block: NHIP_GUESSER_*
    const uint8_t* a_status;        // per pair: pass A's NHIP_MS_* status
    const uint8_t* b_status;        // per pair: pass B's
    const uint64_t* b_bad;          // per pair: pass B's bad_record
    const uint8_t* flags;           // per pair: BLKMS_FLAG_*
    uint8_t* status;                // per pair: NHIP_BLKMS_*
    uint8_t* ms_status;
    uint64_t* bad_record;
    uint32_t n;
};

// records: n x 2 digests [locked, unlocked]; digests: n Block::hash
hipError_t launch_guesser_fee_records(const BlkMsBlockDev* d_blk, const uint64_t* d_digests, const BlkMsParamsDev& p,
                                      uint32_t n, uint64_t* d_records, uint8_t* d_n_records, uint8_t* d_status,
                                      hipStream_t st);
hipError_t launch_blk_ms_rules(const BlkMsRulesDev& d, const BlkMsParamsDev& p, hipStream_t st);

}  // namespace nhip
