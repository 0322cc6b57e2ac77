// Shape checks of the header-chain entry points (chain_shape.hpp).
#include "chain_shape.hpp"

namespace nhip {

int chain_blocks_ok(const uint8_t* bytes, size_t n_bytes, const nhip_blk_block* blocks, size_t n) {
    if (n == 0) return NHIP_OK;
    if (!bytes || !blocks || n > 0xFFFFFFFFull) return NHIP_ERR_ARG;
    for (size_t i = 0; i < n; ++i) {
        const nhip_blk_block& b = blocks[i];
        if (b.offset > n_bytes || b.size > n_bytes - b.offset) return NHIP_ERR_ARG;
    }
    return NHIP_OK;
}

int chain_parents_ok(const int64_t* parent_of, size_t n) {
    if (n == 0) return NHIP_OK;
    if (!parent_of) return NHIP_ERR_ARG;
    for (size_t i = 0; i < n; ++i)
        if (parent_of[i] < -1 || (parent_of[i] >= 0 && (uint64_t)parent_of[i] >= n)) return NHIP_ERR_ARG;
    return NHIP_OK;
}

int chain_params_ok(const nhip_chain_params* p, chain::LinkParams* out) {
    if (!p || !out || p->pow_tree_height < 1 || p->pow_tree_height > CHAIN_MAX_TREE_HEIGHT) return NHIP_ERR_ARG;
    out->minimum_block_time = p->minimum_block_time_ms % chain::P;
    out->target_block_interval = p->target_block_interval_ms % chain::P;
    out->difficulty_reset_interval = p->difficulty_reset_interval_ms % chain::P;
    out->now = p->now_ms % chain::P;
    if (out->target_block_interval == 0) return NHIP_ERR_ARG;
    for (int i = 0; i < chain::DIFFICULTY_LIMBS; ++i) out->genesis_difficulty[i] = p->genesis_difficulty[i];
    chain::difficulty_new(out->genesis_difficulty);
    return NHIP_OK;
}

}  // namespace nhip
