#include "ms_shape.hpp"

namespace nhip {

int ms_csr_ok(const uint64_t* off, size_t n, size_t unit_bytes, uint64_t* total) {
    if (!off || n == SIZE_MAX) return NHIP_ERR_ARG;
    if (off[0] != 0) return NHIP_ERR_ARG;
    for (size_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return NHIP_ERR_ARG;
    if (unit_bytes && off[n] > (uint64_t)(SIZE_MAX / 2) / unit_bytes) return NHIP_ERR_ARG;
    if (total) *total = off[n];
    return NHIP_OK;
}

int ms_mmr_ok(const nhip_mmr* mmr) {
    if (!mmr || (mmr->n_peaks && !mmr->peaks)) return NHIP_ERR_ARG;
    return NHIP_OK;
}

int ms_msa_ok(const nhip_msa* msa) {
    if (!msa || ms_mmr_ok(&msa->aocl) || ms_mmr_ok(&msa->swbf_inactive)) return NHIP_ERR_ARG;
    if (msa->n_active && !msa->active) return NHIP_ERR_ARG;
    if (msa->n_active > (uint64_t)(SIZE_MAX / 2) / sizeof(uint32_t)) return NHIP_ERR_ARG;
    return NHIP_OK;
}

int ms_paths_ok(const uint64_t* path_off, const uint64_t* path, size_t n, uint64_t* path_digests) {
    uint64_t total = 0;
    if (ms_csr_ok(path_off, n, 5 * sizeof(uint64_t), &total)) return NHIP_ERR_ARG;
    if (total && !path) return NHIP_ERR_ARG;
    if (path_digests) *path_digests = total;
    return NHIP_OK;
}

int ms_chunks_ok(const nhip_ms_chunks* chunks, size_t n, MsChunkCounts* counts) {
    if (!chunks) return NHIP_ERR_ARG;
    MsChunkCounts c;
    if (ms_csr_ok(chunks->entry_off, n, sizeof(uint64_t), &c.entries)) return NHIP_ERR_ARG;
    if (c.entries >= (uint64_t)SIZE_MAX / sizeof(uint64_t)) return NHIP_ERR_ARG;
    if (c.entries && !chunks->chunk_index) return NHIP_ERR_ARG;
    if (ms_paths_ok(chunks->path_off, chunks->path, (size_t)c.entries, &c.path_digests)) return NHIP_ERR_ARG;
    if (ms_csr_ok(chunks->rel_off, (size_t)c.entries, sizeof(uint32_t), &c.rel_words)) return NHIP_ERR_ARG;
    if (c.rel_words && !chunks->rel) return NHIP_ERR_ARG;
    if (counts) *counts = c;
    return NHIP_OK;
}

}  // namespace nhip
