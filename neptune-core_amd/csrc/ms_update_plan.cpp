#include "ms_update_plan.hpp"

#include <algorithm>
#include <new>

namespace nhip {

namespace {

using u128 = unsigned __int128;

inline uint64_t sat_dec(uint64_t x) { return x ? x - 1 : 0; }
// x != 0
inline uint64_t ilog2(uint64_t x) { return 63u - (uint64_t)__builtin_clzll(x); }

// number of elements of the sorted v in [lo, hi)
template <class T>
inline uint64_t count_in(const std::vector<T>& v, size_t from, size_t to, T lo, T hi) {
    const auto b = v.begin() + from, e = v.begin() + to;
    return (uint64_t)(std::lower_bound(b, e, hi) - std::lower_bound(b, e, lo));
}

}  // namespace

int ms_update_ok(const nhip_ms_apply_in* block, const nhip_ms_update_in* wit, MsUpdateCounts* counts) {
    if (!block || !wit) return NHIP_ERR_ARG;
    MsUpdateCounts c;
    const size_t n = block->n_jobs;
    if (n == 0) {
        if (counts) *counts = c;
        return NHIP_OK;
    }
    if (ms_csr_ok(wit->wit_off, n, 45 * sizeof(uint32_t), &c.witnesses)) return NHIP_ERR_ARG;
    if (c.witnesses >= (uint64_t)UINT32_MAX) return NHIP_ERR_ARG;
    if (c.witnesses) {
        if (!wit->minimum || !wit->distances || !wit->aocl_leaf_index || !wit->aocl_leaf) return NHIP_ERR_ARG;
        if (ms_paths_ok(wit->aocl_path_off, wit->aocl_path, (size_t)c.witnesses, &c.aocl_digests)) return NHIP_ERR_ARG;
        if (ms_chunks_ok(wit->chunks, (size_t)c.witnesses, &c.chunks)) return NHIP_ERR_ARG;
        if (c.chunks.entries >= (uint64_t)UINT32_MAX) return NHIP_ERR_ARG;
    }
    if (counts) *counts = c;
    return NHIP_OK;
}

int ms_update_plan(const nhip_ms_apply_in* block, const nhip_ms_update_in* wit, const MsUpdateCounts& counts,
                   MsUpdatePlan* plan) {
    const size_t n = block->n_jobs, W = (size_t)counts.witnesses;
    const uint64_t limit = (uint64_t)(SIZE_MAX / 64);
    *plan = MsUpdatePlan{};
    MsUpdatePlan& p = *plan;
    p.aocl_path_off.assign(W + 1, 0);
    p.entry_off.assign(W + 1, 0);
    p.path_off.push_back(0);
    p.rel_off.push_back(0);
    p.wit_job.resize(W);
    p.in_ent_wit.resize((size_t)counts.chunks.entries);
    std::vector<uint32_t> window;
    std::vector<uint64_t> job_chunks, keys;
    for (size_t j = 0; j < n; ++j) {
        const nhip_msa& b = block->msa_before[j];
        const uint64_t n0 = b.aocl.num_leafs, k = block->add_off[j + 1] - block->add_off[j], n1 = n0 + k;
        const bool wraps = n1 < n0;  // NHIP_MS_INCONSISTENT on the device: the witnesses get empty shapes
        const uint64_t b0 = sat_dec(n0) / 8, b1 = wraps ? 0 : sat_dec(n1) / 8;
        // the job's record indices by chunk (below b1: no other chunk gets a key), and its window, both sorted
        job_chunks.clear();
        for (uint64_t r = block->rec_off[j]; r < block->rec_off[j + 1]; ++r) {
            const u128 mn = ((u128)block->minimum[2 * r + 1] << 64) | block->minimum[2 * r];
            for (size_t t = 0; t < 45; ++t) {
                const u128 v = mn + block->distances[45 * r + t];
                if (v >= mn && (v >> 12) < (u128)b1) job_chunks.push_back((uint64_t)(v >> 12));
            }
        }
        std::sort(job_chunks.begin(), job_chunks.end());
        window.clear();
        ms_append_sorted_window(window, b);
        for (uint64_t w = wit->wit_off[j]; w < wit->wit_off[j + 1]; ++w) {
            p.wit_job[w] = (uint32_t)j;
            const uint64_t ebeg = wit->chunks->entry_off[w], eend = wit->chunks->entry_off[w + 1];
            for (uint64_t e = ebeg; e < eend; ++e) p.in_ent_wit[e] = (uint32_t)w;
            const uint64_t l = wit->aocl_leaf_index[w];
            const uint64_t alen = (l == MS_UPDATE_NONE || wraps || l >= n1) ? 0 : ilog2(l ^ n1);
            p.aocl_path_off[w + 1] = p.aocl_path_off[w] + alen;
            keys.clear();
            const u128 mn = ((u128)wit->minimum[2 * w + 1] << 64) | wit->minimum[2 * w];
            for (size_t t = 0; t < 45; ++t) {
                const u128 v = mn + wit->distances[45 * w + t];
                if (v >= mn && (v >> 12) < (u128)b1) keys.push_back((uint64_t)(v >> 12));
            }
            std::sort(keys.begin(), keys.end());
            keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
            for (const uint64_t key : keys) {
                uint64_t src = MS_UPDATE_NONE, n_old = 0;
                if (key < b0) {
                    for (uint64_t e = ebeg; e < eend && src == MS_UPDATE_NONE; ++e)
                        if (wit->chunks->chunk_index[e] == key) src = e;
                    if (src != MS_UPDATE_NONE) n_old = wit->chunks->rel_off[src + 1] - wit->chunks->rel_off[src];
                } else if (key - b0 < 256) {
                    const uint32_t lo = (uint32_t)((key - b0) << 12);
                    // the window's words are u32, the bound of the last chunk is 2^20
                    n_old = (uint64_t)(std::lower_bound(window.begin(), window.end(), lo + 4096u) -
                                       std::lower_bound(window.begin(), window.end(), lo));
                }
                const uint64_t ins = count_in<uint64_t>(job_chunks, 0, job_chunks.size(), key, key + 1);
                p.chunk_index.push_back(key);
                p.ent_wit.push_back((uint32_t)w);
                p.ent_src.push_back(src);
                p.path_off.push_back(p.path_off.back() + ilog2(key ^ b1));  // key < b1
                p.rel_off.push_back(p.rel_off.back() + n_old + ins);
                if (p.rel_off.back() > limit) return NHIP_ERR_OOM;
            }
            p.entry_off[w + 1] = p.chunk_index.size();
        }
    }
    if (p.chunk_index.size() >= (size_t)UINT32_MAX || p.aocl_path_off[W] > limit) return NHIP_ERR_OOM;
    return NHIP_OK;
}

bool ms_updated_is_count_pass(const nhip_ms_updated* out) {
    return !out->aocl_path_off && !out->aocl_path && !out->entry_off && !out->chunk_index && !out->path_off &&
           !out->path && !out->rel_off && !out->rel;
}

int ms_updated_check(const MsUpdatePlan& plan, bool need_data, const nhip_ms_updated* out) {
    if (ms_updated_is_count_pass(out)) return NHIP_OK;
    const size_t W = plan.wit_job.size(), A = (size_t)plan.aocl_path_off[W], E = plan.chunk_index.size();
    const size_t PD = (size_t)plan.path_off[E], RW = (size_t)plan.rel_off[E];
    if (!out->aocl_path_off || !out->entry_off || !out->path_off || !out->rel_off) return NHIP_ERR_ARG;
    if (out->aocl_cap < A || out->entries_cap < E || out->path_cap < PD || out->rel_cap < RW) return NHIP_ERR_ARG;
    if (E && !out->chunk_index) return NHIP_ERR_ARG;
    if (need_data && ((W && !out->status) || (A && !out->aocl_path) || (PD && !out->path) || (RW && !out->rel)))
        return NHIP_ERR_ARG;
    return NHIP_OK;
}

void ms_updated_write(const MsUpdatePlan& plan, bool keys, nhip_ms_updated* out) {
    const size_t W = plan.wit_job.size(), E = plan.chunk_index.size();
    if (!ms_updated_is_count_pass(out)) {
        std::copy(plan.aocl_path_off.begin(), plan.aocl_path_off.end(), out->aocl_path_off);
        std::copy(plan.entry_off.begin(), plan.entry_off.end(), out->entry_off);
        if (keys) std::copy(plan.chunk_index.begin(), plan.chunk_index.end(), out->chunk_index);
        std::copy(plan.path_off.begin(), plan.path_off.end(), out->path_off);
        std::copy(plan.rel_off.begin(), plan.rel_off.end(), out->rel_off);
    }
    out->aocl_digests = (size_t)plan.aocl_path_off[W];
    out->entries = E;
    out->path_digests = (size_t)plan.path_off[E];
    out->rel_words = (size_t)plan.rel_off[E];
}

}  // namespace nhip

extern "C" int nhip_ms_update_plan(const nhip_ms_apply_in* block, const nhip_ms_update_in* wit, nhip_ms_updated* out) {
    if (!out) return NHIP_ERR_ARG;
    nhip::MsApplyCounts bc;
    nhip::MsUpdateCounts wc;
    if (nhip::ms_apply_in_ok(block, &bc) || nhip::ms_update_ok(block, wit, &wc)) return NHIP_ERR_ARG;
    try {
        nhip::MsUpdatePlan plan;
        int rc = nhip::ms_update_plan(block, wit, wc, &plan);
        if (rc != NHIP_OK) return rc;
        if ((rc = nhip::ms_updated_check(plan, false, out)) != NHIP_OK) return rc;
        nhip::ms_updated_write(plan, true, out);
        return NHIP_OK;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}
