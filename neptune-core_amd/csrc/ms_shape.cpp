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

int ms_apply_ok(const nhip_ms_apply_in* in, const nhip_ms_apply_out* out, MsApplyCounts* counts) {
    if (!in || !out) return NHIP_ERR_ARG;
    MsApplyCounts c;
    const size_t n = in->n_jobs;
    if (n == 0) {
        if (counts) *counts = c;
        return NHIP_OK;
    }
    if (n > (size_t)UINT32_MAX || !in->msa_before || !out->verdict || !out->status || !out->bad_record)
        return NHIP_ERR_ARG;
    if (ms_csr_ok(in->add_off, n, 5 * sizeof(uint64_t), &c.additions)) return NHIP_ERR_ARG;
    if (c.additions && !in->additions) return NHIP_ERR_ARG;
    if (ms_csr_ok(in->rec_off, n, 45 * sizeof(uint32_t), &c.records)) return NHIP_ERR_ARG;
    if (c.records) {
        if (!in->minimum || !in->distances) return NHIP_ERR_ARG;
        if (ms_chunks_ok(in->chunks, (size_t)c.records, &c.chunks)) return NHIP_ERR_ARG;
    }
    const int given = (out->aocl_peaks != nullptr) + (out->aocl_n_peaks != nullptr) + (out->aocl_num_leafs != nullptr) +
                      (out->swbf_peaks != nullptr) + (out->swbf_n_peaks != nullptr) + (out->swbf_num_leafs != nullptr) +
                      (out->active_off != nullptr) + (out->n_active != nullptr);
    if (given != 0 && given != 8) return NHIP_ERR_ARG;
    c.accumulators = given == 8;
    if (c.accumulators) {
        if (ms_csr_ok(out->active_off, n, sizeof(uint32_t), &c.window_cap)) return NHIP_ERR_ARG;
        if (c.window_cap && !out->active) return NHIP_ERR_ARG;
    } else if (out->active) {
        return NHIP_ERR_ARG;
    }
    for (size_t j = 0; j < n; ++j) {
        if (ms_msa_ok(&in->msa_before[j])) return NHIP_ERR_ARG;
        if (in->msa_expected && ms_msa_ok(&in->msa_expected[j])) return NHIP_ERR_ARG;
        const uint64_t m = in->rec_off[j + 1] - in->rec_off[j];
        if (m > (uint64_t)UINT32_MAX / 45) return NHIP_ERR_ARG;
        const uint64_t need = in->msa_before[j].n_active + 45 * m;  // n_active <= SIZE_MAX / 8: no wrap
        if (c.accumulators && out->active_off[j + 1] - out->active_off[j] < need) return NHIP_ERR_ARG;
    }
    if (counts) *counts = c;
    return NHIP_OK;
}

}  // namespace nhip
