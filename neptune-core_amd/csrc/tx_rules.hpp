// Consensus integers of a block's transaction rules (Block::validate 2.f-2.l, Block::block_subsidy) and of the
// guesser-fee UTXOs, one definition for the host (tests/native/tx_rules_check.cpp) and the device
// (k_guesser_fee_records, k_blk_ms_rules).  Plain C++: no HIP header, no inline assembly, no __int128 (an i128 is
// two u64 with an explicit signed compare); under HIP the functions are __host__ __device__.
//
// Restated (neptune-core/src/protocol/consensus/):
//   NativeCurrencyAmount           type_scripts/native_currency_amount.rs:50 (i128), :88-99 (one coin = 4 * 10^30 nau),
//                                  div_two :125-127 (i128 / 2, truncating toward zero)
//   Block::block_subsidy           block/mod.rs:393-408; INITIAL_BLOCK_SUBSIDY = 128 coins (:102)
//   BlockHeight::get_generation    block/block_height.rs:46-47,60-65
//   rules 2.f-2.l                  block/mod.rs:851-891, the limits consensus_rule_set.rs:71-91
//   guesser_fee_utxos              block/block_kernel.rs:47-67; total_guesser_reward block_body.rs:160-169;
//                                  Timestamp::years timestamp.rs:126-128; TimeLock::until type_scripts/time_lock.rs:39-44
//   Coin, Utxo                     transaction/utxo.rs:29-32,71-74; their BFieldCodec encodings follow the derive rules
//                                  bincode.cpp states (fields last-first, dynamic fields length-prefixed) [EXT, unpinned]
#pragma once
#include <stdint.h>

#ifdef __HIP__
#define NHIP_TX_HD __host__ __device__ inline
#else
#define NHIP_TX_HD inline
#endif

namespace nhip {
namespace txrules {

static constexpr uint64_t P = 0xFFFFFFFF00000001ull;
static constexpr uint64_t BLOCKS_PER_GENERATION = 160815, NUM_BLOCKS_SKIPPED_BECAUSE_REBOOT = 21310;
static constexpr uint64_t MINER_REWARD_TIME_LOCK_PERIOD_MS = 94670208000ull;  // Timestamp::years(3)
static constexpr int UTXO_UNLOCKED_WORDS = 19, UTXO_LOCKED_WORDS = 28;

// i128 in two's complement
struct I128 {
    uint64_t lo, hi;
};

NHIP_TX_HD bool is_negative(I128 a) { return (a.hi >> 63) != 0; }
NHIP_TX_HD bool is_zero(I128 a) { return (a.lo | a.hi) == 0; }
// a > b, signed
NHIP_TX_HD bool greater(I128 a, I128 b) {
    const bool an = is_negative(a), bn = is_negative(b);
    if (an != bn) return bn;
    if (a.hi != b.hi) return a.hi > b.hi;  // equal signs: the unsigned order of the bits is the signed one
    return a.lo > b.lo;
}
NHIP_TX_HD I128 sub(I128 a, I128 b) {  // wrapping
    I128 r;
    r.lo = a.lo - b.lo;
    r.hi = a.hi - b.hi - (a.lo < b.lo ? 1u : 0u);
    return r;
}
// a / 2, truncating toward zero
NHIP_TX_HD I128 half(I128 a) {
    if (is_negative(a)) {  // (a + 1) >> 1, arithmetic
        a.lo += 1;
        if (a.lo == 0) a.hi += 1;
    }
    I128 r;
    r.lo = (a.lo >> 1) | (a.hi << 63);
    r.hi = (uint64_t)((int64_t)a.hi >> 1);
    return r;
}

// 128 coins = 128 * 4 * 10^30 nau
NHIP_TX_HD I128 initial_block_subsidy() { return I128{0xe9dbd48000000000ull, 0x0000193e5939a08cull}; }

NHIP_TX_HD uint64_t generation(uint64_t height) {
    const uint64_t s = height + NUM_BLOCKS_SKIPPED_BECAUSE_REBOOT;
    return (s < height ? ~0ull : s) / BLOCKS_PER_GENERATION;  // saturating_add
}

// Block::block_subsidy: halved once per generation, zero once nothing is left
NHIP_TX_HD I128 block_subsidy(uint64_t height) {
    I128 reward = initial_block_subsidy();
    const uint64_t g = generation(height);
    for (uint64_t k = 0; k < g; ++k) {
        reward = half(reward);
        if (is_zero(reward)) return I128{0, 0};
    }
    return reward;
}

// What rules 2.f-2.l read of a block (timestamps and the height canonical)
struct TxFacts {
    uint64_t header_height, header_timestamp, kernel_timestamp;
    I128 fee, coinbase;
    uint32_t has_coinbase;
    uint64_t n_inputs, n_outputs, n_announcements;
};
struct TxLimits {
    uint64_t max_num_inputs, max_num_outputs, max_num_announcements;
};

// Rules 2.f-2.l in the reference's order: 0 when all hold, else 'f' .. 'l'
NHIP_TX_HD char rules_2f_2l(const TxLimits& lim, const TxFacts& t) {
    if (t.kernel_timestamp > t.header_timestamp) return 'f';
    if (t.has_coinbase) {
        if (greater(t.coinbase, block_subsidy(t.header_height))) return 'g';
        if (is_negative(t.coinbase)) return 'h';
    }
    if (is_negative(t.fee)) return 'i';
    if (t.n_inputs > lim.max_num_inputs) return 'j';
    if (t.n_outputs > lim.max_num_outputs) return 'k';
    if (t.n_announcements > lim.max_num_announcements) return 'l';
    return 0;
}

// guesser_fee_utxos' amounts for a non-negative fee: [locked, unlocked]
NHIP_TX_HD void guesser_split(I128 fee, I128& locked, I128& unlocked) {
    locked = half(fee);
    unlocked = sub(fee, locked);
}

// Timestamp + Timestamp: a Goldilocks addition of canonical values
NHIP_TX_HD uint64_t release_date(uint64_t parent_timestamp) {
    const uint64_t b = MINER_REWARD_TIME_LOCK_PERIOD_MS;
    const uint64_t s = parent_timestamp + b;
    return (s < parent_timestamp || s >= P) ? s - P : s;
}

// Utxo::encode of a guesser-fee UTXO, canonical words; returns the length.  Utxo = [len(coins_enc)] ++ coins_enc ++
// lock_script_hash with coins_enc = [n_coins] ++ ([len(coin)] ++ coin)*, Coin = [len(state_enc)] ++ [len(state)] ++
// state ++ type_script_hash; NativeCurrencyAmount = its i128 as four u32 limbs, low first.
NHIP_TX_HD int guesser_utxo_words(bool locked, I128 amount, uint64_t date, const uint64_t native_currency_hash[5],
                                  const uint64_t time_lock_hash[5], const uint64_t lock_script_hash[5],
                                  uint64_t out[UTXO_LOCKED_WORDS]) {
    int k = 0;
    out[k++] = locked ? 22 : 13;
    out[k++] = locked ? 2 : 1;
    out[k++] = 11;  // the native-currency coin
    out[k++] = 5;
    out[k++] = 4;
    out[k++] = amount.lo & 0xFFFFFFFFull;
    out[k++] = amount.lo >> 32;
    out[k++] = amount.hi & 0xFFFFFFFFull;
    out[k++] = amount.hi >> 32;
    for (int q = 0; q < 5; ++q) out[k++] = native_currency_hash[q];
    if (locked) {
        out[k++] = 8;  // TimeLock::until(date)
        out[k++] = 2;
        out[k++] = 1;
        out[k++] = date;
        for (int q = 0; q < 5; ++q) out[k++] = time_lock_hash[q];
    }
    for (int q = 0; q < 5; ++q) out[k++] = lock_script_hash[q];
    return k;
}

}  // namespace txrules
}  // namespace nhip
