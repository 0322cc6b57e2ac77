#include "ms_shape.hpp"

#include <algorithm>

namespace nhip {

int ms_csr_ok(const uint64_t* off, size_t n, size_t unit_bytes, uint64_t* total) {
    if (!off || n == SIZE_MAX) return NHIP_ERR_ARG;
    if (off[0] != 0) return NHIP_ERR_ARG;
    // no early exit: one pass without a branch per element, whose speed does not depend on where the linker
    // puts the loop (ms_rate's 370,000 offsets: 76 or 112 us with the branch, by placement alone)
    uint64_t decreases = 0;
    for (size_t i = 0; i < n; ++i) decreases |= (uint64_t)(off[i + 1] < off[i]);
    if (decreases) return NHIP_ERR_ARG;
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

int ms_apply_in_ok(const nhip_ms_apply_in* in, MsApplyCounts* counts) {
    if (!in) return NHIP_ERR_ARG;
    MsApplyCounts c;
    const size_t n = in->n_jobs;
    if (n == 0) {
        if (counts) *counts = c;
        return NHIP_OK;
    }
    if (n > (size_t)UINT32_MAX || !in->msa_before) return NHIP_ERR_ARG;
    if (ms_csr_ok(in->add_off, n, 5 * sizeof(uint64_t), &c.additions)) return NHIP_ERR_ARG;
    if (c.additions && !in->additions) return NHIP_ERR_ARG;
    if (ms_csr_ok(in->rec_off, n, 45 * sizeof(uint32_t), &c.records)) return NHIP_ERR_ARG;
    if (c.records) {
        if (!in->minimum || !in->distances) return NHIP_ERR_ARG;
        if (ms_chunks_ok(in->chunks, (size_t)c.records, &c.chunks)) return NHIP_ERR_ARG;
    }
    for (size_t j = 0; j < n; ++j) {
        if (ms_msa_ok(&in->msa_before[j])) return NHIP_ERR_ARG;
        if (in->msa_expected && ms_msa_ok(&in->msa_expected[j])) return NHIP_ERR_ARG;
        if (in->rec_off[j + 1] - in->rec_off[j] > (uint64_t)UINT32_MAX / 45) return NHIP_ERR_ARG;
    }
    if (counts) *counts = c;
    return NHIP_OK;
}

int ms_apply_ok(const nhip_ms_apply_in* in, const nhip_ms_apply_out* out, MsApplyCounts* counts) {
    if (!in || !out) return NHIP_ERR_ARG;
    MsApplyCounts c;
    if (ms_apply_in_ok(in, &c)) return NHIP_ERR_ARG;
    const size_t n = in->n_jobs;
    if (n == 0) {
        if (counts) *counts = c;
        return NHIP_OK;
    }
    if (!out->verdict || !out->status || !out->bad_record) return NHIP_ERR_ARG;
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
        const uint64_t m = in->rec_off[j + 1] - in->rec_off[j];
        const uint64_t need = in->msa_before[j].n_active + 45 * m;  // n_active <= SIZE_MAX / 8: no wrap
        if (c.accumulators && out->active_off[j + 1] - out->active_off[j] < need) return NHIP_ERR_ARG;
    }
    if (counts) *counts = c;
    return NHIP_OK;
}

void ms_append_sorted_window(std::vector<uint32_t>& pool, const nhip_msa& msa) {
    const size_t at = pool.size();
    if (msa.n_active) pool.insert(pool.end(), msa.active, msa.active + msa.n_active);
    std::sort(pool.begin() + at, pool.end());
}

std::vector<uint64_t> ms_interleave15(const uint64_t* items, const uint64_t* sender_randomness,
                                      const uint64_t* receiver_preimages, size_t n) {
    std::vector<uint64_t> in(15 * n);
    for (size_t i = 0; i < n; ++i)
        for (int q = 0; q < 5; ++q) {
            in[15 * i + q] = items[5 * i + q];
            in[15 * i + 5 + q] = sender_randomness[5 * i + q];
            in[15 * i + 10 + q] = receiver_preimages[5 * i + q];
        }
    return in;
}

void ms_apply_order(const nhip_ms_apply_in* in, const nhip_ms_apply_out* out, const MsApplyCounts& cnt,
                    MsApplyOrder* o, bool keep_nodes) {
    using u128 = unsigned __int128;
    const size_t n = in->n_jobs, R = (size_t)cnt.records, E = (size_t)cnt.chunks.entries;
    *o = MsApplyOrder{};
    o->jobs.resize(n);
    o->rec_job.resize(R);
    o->entry_rec.resize(E);
    o->idx_perm.resize(45 * R);
    o->rec_perm.resize(R);
    std::vector<u128> vals;
    auto put_peaks = [&](const nhip_mmr& m) {
        const uint64_t off = o->peaks.size() / 5;
        if (m.n_peaks) o->peaks.insert(o->peaks.end(), m.peaks, m.peaks + 5 * (size_t)m.n_peaks);
        return off;
    };
    for (size_t j = 0; j < n; ++j) {
        const nhip_msa& b = in->msa_before[j];
        MsApplyJob& jb = o->jobs[j];
        jb = MsApplyJob{};
        jb.aocl_n = b.aocl.num_leafs;
        jb.swbf_n = b.swbf_inactive.num_leafs;
        jb.aocl_np = b.aocl.n_peaks;
        jb.swbf_np = b.swbf_inactive.n_peaks;
        jb.aocl_peaks = put_peaks(b.aocl);
        jb.swbf_peaks = put_peaks(b.swbf_inactive);
        jb.act_off = o->active.size();
        jb.n_active = b.n_active;
        ms_append_sorted_window(o->active, b);
        jb.add_off = in->add_off[j];
        jb.k = in->add_off[j + 1] - in->add_off[j];
        jb.rec_off = in->rec_off[j];
        jb.m = in->rec_off[j + 1] - in->rec_off[j];
        if (in->msa_expected) {
            const nhip_msa& x = in->msa_expected[j];
            jb.exp_aocl_n = x.aocl.num_leafs;
            jb.exp_swbf_n = x.swbf_inactive.num_leafs;
            jb.exp_aocl_np = x.aocl.n_peaks;
            jb.exp_swbf_np = x.swbf_inactive.n_peaks;
            jb.exp_aocl_peaks = put_peaks(x.aocl);
            jb.exp_swbf_peaks = put_peaks(x.swbf_inactive);
            jb.exp_act_off = o->exp_active.size();
            jb.exp_n_active = x.n_active;
            if (x.n_active) o->exp_active.insert(o->exp_active.end(), x.active, x.active + x.n_active);
        }
        // the job's index slots by (index, slot), the runs of one chunk index, the records by their index arrays
        const size_t m = (size_t)jb.m, r0 = (size_t)jb.rec_off;
        vals.resize(45 * m);
        for (size_t r = 0; r < m; ++r) {
            o->rec_job[r0 + r] = (uint32_t)j;
            const u128 mn = ((u128)in->minimum[2 * (r0 + r) + 1] << 64) | in->minimum[2 * (r0 + r)];
            for (size_t t = 0; t < 45; ++t) vals[45 * r + t] = mn + in->distances[45 * (r0 + r) + t];
            for (uint64_t e = in->chunks->entry_off[r0 + r]; e < in->chunks->entry_off[r0 + r + 1]; ++e)
                o->entry_rec[e] = (uint32_t)(r0 + r);
        }
        uint32_t* perm = o->idx_perm.data() + 45 * r0;
        for (size_t s = 0; s < 45 * m; ++s) perm[s] = (uint32_t)s;
        std::sort(perm, perm + 45 * m, [&](uint32_t x, uint32_t y) { return vals[x] != vals[y] ? vals[x] < vals[y] : x < y; });
        jb.grp_off = o->grp_total;
        for (size_t s = 0; s < 45 * m; ++s)
            if (s == 0 || (vals[perm[s]] >> 12) != (vals[perm[s - 1]] >> 12)) {
                o->grp.push_back((uint32_t)s);
                ++jb.n_grp;
            }
        o->grp.push_back((uint32_t)(45 * m));
        o->grp_total += jb.n_grp;
        uint32_t* rp = o->rec_perm.data() + r0;
        for (size_t r = 0; r < m; ++r) rp[r] = (uint32_t)r;
        std::stable_sort(rp, rp + m, [&](uint32_t x, uint32_t y) {
            return std::lexicographical_compare(vals.begin() + 45 * x, vals.begin() + 45 * x + 45,
                                                vals.begin() + 45 * y, vals.begin() + 45 * y + 45);
        });
        jb.dig_off = o->dig_total;
        o->dig_total += MsJobScratch(jb.aocl_n, jb.k).total(jb.n_grp, keep_nodes);
        jb.win_off = cnt.accumulators ? out->active_off[j] : o->win_total;
        jb.win_cap = cnt.accumulators ? out->active_off[j + 1] - out->active_off[j] : jb.n_active + 45 * jb.m;
        o->win_total += jb.win_cap;
    }
    if (cnt.accumulators) o->win_total = cnt.window_cap;
}

}  // namespace nhip
