// Host side of nhip_blk_ms_walk, nhip_blk_guesser_fee_records and nhip_blk_ms_check: what the walk
// of csrc/bincode.cpp extracts of each scanned block (integers and byte copies only; nothing is hashed and nothing
// decided), and the jobs it lays out for the two passes of the existing apply path.  Plain C++ (no HIP header), so
// that tests/native/tx_rules_check.cpp links it under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/neptune_hip.h"

namespace nhip {

// The parts of n blocks, block by block; the pooled arrays are CSR over the blocks (or over the records / entries),
// in nhip_blk_ms_parts' layout
struct BlkMsParts {
    size_t n = 0;
    std::vector<uint64_t> height, timestamp, receiver_digest, lock_script_hash, fee, coinbase, kernel_timestamp,
        n_announcements, aocl_num_leafs, swbf_num_leafs, aocl_peaks, swbf_peaks;
    std::vector<uint8_t> coinbase_tag;
    std::vector<uint32_t> aocl_n_peaks, swbf_n_peaks;  // as serialized, saturated at 65; 64 slots stored per block
    std::vector<uint64_t> active_off{0}, out_off{0}, rec_off{0}, entry_off{0}, path_off{0}, rel_off{0};
    std::vector<uint32_t> active, distances, rel;
    std::vector<uint64_t> outputs, minimum, chunk_index, path;
};

// bincode.cpp: appends the block at `offset` to p (p is left as it was on a decode error).  May throw std::bad_alloc.
int blk_ms_walk_block(const uint8_t* bytes, size_t n_bytes, uint32_t pow_tree_height, uint64_t offset, BlkMsParts& p);

// The n blocks (blocks[i].offset <= n_bytes each); NHIP_ERR_DECODE at the first block that does not parse
int blk_ms_walk(const uint8_t* bytes, size_t n_bytes, uint32_t pow_tree_height, const nhip_blk_block* blocks, size_t n,
                BlkMsParts& p);

// Block i's body accumulator as an nhip_msa into p's pools, at most 64 peaks each
nhip_msa blk_ms_body_msa(const BlkMsParts& p, size_t i);
inline bool blk_ms_peaks_oversize(const BlkMsParts& p, size_t i) { return p.aocl_n_peaks[i] > 64 || p.swbf_n_peaks[i] > 64; }
// The packed dictionaries of all blocks' inputs
nhip_ms_chunks blk_ms_chunks(const BlkMsParts& p);

}  // namespace nhip
