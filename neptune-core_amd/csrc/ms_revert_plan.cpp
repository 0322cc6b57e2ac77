#include "ms_revert_plan.hpp"

#include <algorithm>
#include <new>

namespace nhip {

namespace {

using u128 = unsigned __int128;

inline uint64_t sat_dec(uint64_t x) { return x ? x - 1 : 0; }
// x != 0
inline uint64_t ilog2(uint64_t x) { return 63u - (uint64_t)__builtin_clzll(x); }

}  // namespace

int ms_revert_plan(const nhip_ms_apply_in* block, const nhip_ms_update_in* wit, const MsUpdateCounts& counts,
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
    std::vector<uint64_t> job_chunks, keys;
    for (size_t j = 0; j < n; ++j) {
        const uint64_t n0 = block->msa_before[j].aocl.num_leafs, k = block->add_off[j + 1] - block->add_off[j];
        const bool wraps = n0 + k < n0;  // NHIP_MS_INCONSISTENT on the device: the witnesses get empty shapes
        const uint64_t b0 = wraps ? 0 : sat_dec(n0) / 8;
        // the job's record indices by chunk (below b0: no other chunk keeps its key), sorted
        job_chunks.clear();
        for (uint64_t r = block->rec_off[j]; r < block->rec_off[j + 1]; ++r) {
            const u128 mn = ((u128)block->minimum[2 * r + 1] << 64) | block->minimum[2 * r];
            for (size_t t = 0; t < 45; ++t) {
                const u128 v = mn + block->distances[45 * r + t];
                if (v >= mn && (v >> 12) < (u128)b0) job_chunks.push_back((uint64_t)(v >> 12));
            }
        }
        std::sort(job_chunks.begin(), job_chunks.end());
        for (uint64_t w = wit->wit_off[j]; w < wit->wit_off[j + 1]; ++w) {
            p.wit_job[w] = (uint32_t)j;
            const uint64_t ebeg = wit->chunks->entry_off[w], eend = wit->chunks->entry_off[w + 1];
            const uint64_t l = wit->aocl_leaf_index[w];
            const uint64_t alen = (l == MS_UPDATE_NONE || wraps || l >= n0) ? 0 : ilog2(l ^ n0);
            p.aocl_path_off[w + 1] = p.aocl_path_off[w] + alen;
            keys.clear();
            const u128 mn = ((u128)wit->minimum[2 * w + 1] << 64) | wit->minimum[2 * w];
            for (size_t t = 0; t < 45; ++t) {
                const u128 v = mn + wit->distances[45 * w + t];
                if (v >= mn && (v >> 12) < (u128)b0) keys.push_back((uint64_t)(v >> 12));
            }
            std::sort(keys.begin(), keys.end());
            keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
            for (const uint64_t key : keys) {
                uint64_t src = MS_UPDATE_NONE, n_now = 0;
                for (uint64_t e = ebeg; e < eend && src == MS_UPDATE_NONE; ++e)
                    if (wit->chunks->chunk_index[e] == key) src = e;
                if (src != MS_UPDATE_NONE) n_now = wit->chunks->rel_off[src + 1] - wit->chunks->rel_off[src];
                const auto range = std::equal_range(job_chunks.begin(), job_chunks.end(), key);
                const uint64_t gone = (uint64_t)(range.second - range.first);
                p.chunk_index.push_back(key);
                p.ent_wit.push_back((uint32_t)w);
                p.ent_src.push_back(src);
                p.path_off.push_back(p.path_off.back() + ilog2(key ^ b0));  // key < b0
                p.rel_off.push_back(p.rel_off.back() + (n_now > gone ? n_now - gone : 0));
                if (p.rel_off.back() > limit) return NHIP_ERR_OOM;
            }
            p.entry_off[w + 1] = p.chunk_index.size();
        }
    }
    if (p.chunk_index.size() >= (size_t)UINT32_MAX || p.aocl_path_off[W] > limit) return NHIP_ERR_OOM;
    return NHIP_OK;
}

std::vector<uint64_t> ms_revert_node_offsets(const std::vector<MsApplyJob>& jobs) {
    std::vector<uint64_t> off(jobs.size() + 1, 0);
    for (size_t j = 0; j < jobs.size(); ++j) {
        const uint64_t b0 = MsJobScratch::batch_index(jobs[j].aocl_n);
        const uint64_t levels = b0 ? ilog2(b0) + 1 : 0;  // no chunk is inactive before the first slide
        off[j + 1] = off[j] + levels * jobs[j].n_grp;  // n_grp < 2^32, levels <= 64
    }
    return off;
}

}  // namespace nhip

extern "C" int nhip_ms_revert_plan(const nhip_ms_apply_in* block, const nhip_ms_update_in* wit, nhip_ms_updated* out) {
    if (!out) return NHIP_ERR_ARG;
    nhip::MsApplyCounts bc;
    nhip::MsUpdateCounts wc;
    if (nhip::ms_apply_in_ok(block, &bc) || nhip::ms_update_ok(block, wit, &wc)) return NHIP_ERR_ARG;
    try {
        nhip::MsUpdatePlan plan;
        int rc = nhip::ms_revert_plan(block, wit, wc, &plan);
        if (rc != NHIP_OK) return rc;
        if ((rc = nhip::ms_updated_check(plan, false, out)) != NHIP_OK) return rc;
        nhip::ms_updated_write(plan, true, out);
        return NHIP_OK;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}
