// Host side of nhip_blk_digests / nhip_blk_chain_check (chain_capi.hip): shape checks
// only, as ms_shape.hpp's.  Every status byte is the device's; the host refuses (NHIP_ERR_ARG) what it
// could not stage without reading outside the caller's arrays.  Host only (no HIP), so that
// tests/native/chain_rules_check.cpp links it under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/neptune_hip.h"
#include "chain_rules.hpp"

namespace nhip {

static constexpr uint32_t CHAIN_MAX_TREE_HEIGHT = 32;  // POW_MAX_HEIGHT (pow.hpp)

// n scanned blocks of bytes[0, n_bytes): both arrays present, every block inside the buffer
int chain_blocks_ok(const uint8_t* bytes, size_t n_bytes, const nhip_blk_block* blocks, size_t n);
// parent_of[i] is -1 or names one of the n blocks
int chain_parents_ok(const int64_t* parent_of, size_t n);
// The parameters as k_block_links reads them: times reduced mod p (Timestamp::millis is
// BFieldElement::new), the genesis difficulty through Difficulty::new.  Refused: a tree height outside
// 1..32, and a target block interval that is zero mod p (the reference divides by it).
int chain_params_ok(const nhip_chain_params* p, chain::LinkParams* out);

}  // namespace nhip
