#include "blk_ms_parts.hpp"

#include <cstring>
#include <new>

namespace nhip {

int blk_ms_walk(const uint8_t* bytes, size_t n_bytes, uint32_t pow_tree_height, const nhip_blk_block* blocks, size_t n,
                BlkMsParts& p) {
    for (size_t i = 0; i < n; ++i) {
        if (blocks[i].offset > n_bytes) return NHIP_ERR_ARG;
        const int rc = blk_ms_walk_block(bytes, n_bytes, pow_tree_height, blocks[i].offset, p);
        if (rc) return rc;
    }
    return NHIP_OK;
}

nhip_msa blk_ms_body_msa(const BlkMsParts& p, size_t i) {
    nhip_msa m;
    const uint32_t na = p.aocl_n_peaks[i] < 64 ? p.aocl_n_peaks[i] : 64, ns = p.swbf_n_peaks[i] < 64 ? p.swbf_n_peaks[i] : 64;
    m.aocl = nhip_mmr{p.aocl_peaks.data() + 64 * 5 * i, na, p.aocl_num_leafs[i]};
    m.swbf_inactive = nhip_mmr{p.swbf_peaks.data() + 64 * 5 * i, ns, p.swbf_num_leafs[i]};
    m.n_active = p.active_off[i + 1] - p.active_off[i];
    m.active = m.n_active ? p.active.data() + p.active_off[i] : nullptr;
    return m;
}

nhip_ms_chunks blk_ms_chunks(const BlkMsParts& p) {
    return nhip_ms_chunks{p.entry_off.data(), p.chunk_index.data(), p.path_off.data(), p.path.data(),
                          p.rel_off.data(),   p.rel.data()};
}

}  // namespace nhip

namespace {
template <class T>
void put(T* dst, const std::vector<T>& src) {
    if (!src.empty()) std::memcpy(dst, src.data(), src.size() * sizeof(T));
}
}  // namespace

extern "C" {

void nhip_blk_ms_params_default(nhip_blk_ms_params* out) {
    if (!out) return;
    std::memset(out, 0, sizeof(*out));
    out->pow_tree_height = 29;  // pow.rs:33-37
    out->max_num_inputs = out->max_num_outputs = out->max_num_announcements = 1u << 14;
}

int nhip_blk_ms_walk(const uint8_t* bytes, size_t n_bytes, uint32_t pow_tree_height, const nhip_blk_block* blocks, size_t n,
                     nhip_blk_ms_parts* o) {
    if (!o || (n_bytes && !bytes) || (n && !blocks) || pow_tree_height > 64) return NHIP_ERR_ARG;
    const void* arrays[] = {o->height,         o->timestamp,   o->receiver_digest, o->lock_script_hash, o->fee,
                            o->coinbase,       o->coinbase_tag, o->kernel_timestamp, o->n_announcements, o->aocl_num_leafs,
                            o->swbf_num_leafs, o->aocl_n_peaks, o->swbf_n_peaks,    o->aocl_peaks,       o->swbf_peaks,
                            o->active_off,     o->active,      o->out_off,         o->outputs,          o->rec_off,
                            o->minimum,        o->distances,   o->entry_off,       o->chunk_index,      o->path_off,
                            o->path,           o->rel_off,     o->rel};
    size_t given = 0;
    for (const void* a : arrays) given += a != nullptr;
    if (given != 0 && given != sizeof(arrays) / sizeof(arrays[0])) return NHIP_ERR_ARG;
    try {
        nhip::BlkMsParts p;
        const int rc = nhip::blk_ms_walk(bytes, n_bytes, pow_tree_height, blocks, n, p);
        if (rc) return rc;
        const size_t A = p.active.size(), O = p.outputs.size() / 5, R = p.minimum.size() / 2, E = p.chunk_index.size(),
                     PD = p.path.size() / 5, W = p.rel.size();
        if (given && (o->active_cap < A || o->outputs_cap < O || o->records_cap < R || o->entries_cap < E ||
                      o->path_cap < PD || o->rel_cap < W))
            return NHIP_ERR_ARG;
        o->active_words = A;
        o->n_outputs = O;
        o->records = R;
        o->entries = E;
        o->path_digests = PD;
        o->rel_words = W;
        if (!given) return NHIP_OK;
        put(o->height, p.height);
        put(o->timestamp, p.timestamp);
        put(o->receiver_digest, p.receiver_digest);
        put(o->lock_script_hash, p.lock_script_hash);
        put(o->fee, p.fee);
        put(o->coinbase, p.coinbase);
        put(o->coinbase_tag, p.coinbase_tag);
        put(o->kernel_timestamp, p.kernel_timestamp);
        put(o->n_announcements, p.n_announcements);
        put(o->aocl_num_leafs, p.aocl_num_leafs);
        put(o->swbf_num_leafs, p.swbf_num_leafs);
        put(o->aocl_n_peaks, p.aocl_n_peaks);
        put(o->swbf_n_peaks, p.swbf_n_peaks);
        put(o->aocl_peaks, p.aocl_peaks);
        put(o->swbf_peaks, p.swbf_peaks);
        put(o->active_off, p.active_off);
        put(o->active, p.active);
        put(o->out_off, p.out_off);
        put(o->outputs, p.outputs);
        put(o->rec_off, p.rec_off);
        put(o->minimum, p.minimum);
        put(o->distances, p.distances);
        put(o->entry_off, p.entry_off);
        put(o->chunk_index, p.chunk_index);
        put(o->path_off, p.path_off);
        put(o->path, p.path);
        put(o->rel_off, p.rel_off);
        put(o->rel, p.rel);
        return NHIP_OK;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

}  // extern "C"
