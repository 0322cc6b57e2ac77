// Host side of the device-resident archival mutator set (ms_archive.hpp).  No HIP.
#include "ms_archive.hpp"

#include <algorithm>
#include <new>

namespace nhip {

namespace {

using u128 = unsigned __int128;
constexpr uint32_t NUM_TRIALS = 45, CHUNK_BITS = 12, WINDOW_CHUNKS = 1u << 8;

}  // namespace

uint64_t ms_arch_level_cap(uint64_t need, uint64_t floor) {
    const uint64_t want = std::max<uint64_t>({need, floor, 1});
    if (want > MS_ARCHIVE_MAX_LEAFS) return 0;
    uint64_t cap = 1;
    while (cap < want) cap <<= 1;
    return cap;
}

MsArchBuild ms_arch_build(uint64_t n) {
    MsArchBuild b;
    uint32_t h = 1;
    while ((n >> (h - 1)) > MS_ARCHIVE_TAIL_NODES) ++h;  // level h is wide while the level it reads has more nodes than that
    b.wide_levels = h - 1;
    b.tail_from = h;
    b.top = n ? ms_arch_ilog2(n) : 0;
    return b;
}

int ms_archive_load_ok(const uint64_t* aocl_leaves, uint64_t n_leafs, const uint64_t* rel_off, const uint32_t* rel,
                       uint64_t n_chunks, const uint32_t* active, uint64_t n_active) {
    if (n_leafs && !aocl_leaves) return NHIP_ERR_ARG;
    if (n_chunks != MsJobScratch::batch_index(n_leafs)) return NHIP_ERR_ARG;
    if (n_active && !active) return NHIP_ERR_ARG;
    if (n_leafs > MS_ARCHIVE_MAX_LEAFS || n_active > MS_ARCHIVE_LIMIT) return NHIP_ERR_OOM;
    if (n_chunks) {
        if (!rel_off || rel_off[0] != 0) return NHIP_ERR_ARG;
        for (uint64_t c = 0; c < n_chunks; ++c)
            if (rel_off[c + 1] < rel_off[c]) return NHIP_ERR_ARG;
        const uint64_t words = rel_off[n_chunks];
        if (words > MS_ARCHIVE_LIMIT) return NHIP_ERR_OOM;
        if (words && !rel) return NHIP_ERR_ARG;
        for (uint64_t c = 0; c < n_chunks; ++c)
            for (uint64_t k = rel_off[c]; k < rel_off[c + 1]; ++k)
                if (rel[k] >= MS_ARCHIVE_CHUNK_SIZE || (k > rel_off[c] && rel[k] < rel[k - 1])) return NHIP_ERR_ARG;
    }
    for (uint64_t k = 0; k < n_active; ++k)
        if (active[k] >= MS_ARCHIVE_WINDOW_SIZE || (k && active[k] < active[k - 1])) return NHIP_ERR_ARG;
    return NHIP_OK;
}

void ms_archive_load_commit(MsArchiveMirror& m, uint64_t n_leafs, const uint64_t* rel_off, uint64_t n_chunks,
                            const uint32_t* active, uint64_t n_active, uint64_t aocl_cap, uint64_t swbf_cap) {
    std::vector<uint64_t> off((size_t)n_chunks), len((size_t)n_chunks);
    for (uint64_t c = 0; c < n_chunks; ++c) {
        off[(size_t)c] = rel_off[c];
        len[(size_t)c] = rel_off[c + 1] - rel_off[c];
    }
    std::vector<uint32_t> window(active, active + (size_t)n_active);
    m.aocl_leafs = n_leafs;
    m.chunk_off = std::move(off);
    m.chunk_len = std::move(len);
    m.window = std::move(window);
    m.rel_tail = m.rel_live = n_chunks ? rel_off[n_chunks] : 0;
    m.aocl_cap = aocl_cap;
    m.swbf_cap = swbf_cap;
}

int ms_archive_paths_plan(uint64_t num_leafs, const uint64_t* leaf_index, size_t n, std::vector<uint64_t>* path_off) {
    if (n && !leaf_index) return NHIP_ERR_ARG;
    if (n > 0xFFFFFFFFull) return NHIP_ERR_OOM;
    for (size_t i = 0; i < n; ++i)
        if (leaf_index[i] >= num_leafs) return NHIP_ERR_ARG;
    path_off->assign(n + 1, 0);
    for (size_t i = 0; i < n; ++i) (*path_off)[i + 1] = (*path_off)[i] + ms_arch_path_len(leaf_index[i], num_leafs);
    return (*path_off)[n] > MS_ARCHIVE_LIMIT ? NHIP_ERR_OOM : NHIP_OK;  // 64 digests a path at most: no wrap
}

int ms_archive_restore_plan(uint64_t aocl_leafs, const uint64_t* chunk_len, uint64_t n_chunks, const uint64_t* minimum,
                            const uint32_t* distances, const uint64_t* aocl_leaf_index, size_t n, MsUpdatePlan* plan,
                            std::vector<uint8_t>* status) {
    const uint64_t b = MsJobScratch::batch_index(aocl_leafs);
    if (n_chunks != b || (n_chunks && !chunk_len)) return NHIP_ERR_ARG;
    if (n && (!minimum || !distances || !aocl_leaf_index)) return NHIP_ERR_ARG;
    if (n > 0xFFFFFFFFull) return NHIP_ERR_OOM;
    MsUpdatePlan p;
    p.wit_job.assign(n, 0);
    p.aocl_path_off.assign(n + 1, 0);
    p.entry_off.assign(n + 1, 0);
    p.path_off.assign(1, 0);
    p.rel_off.assign(1, 0);
    std::vector<uint8_t> st(n, NHIP_MS_OK);
    const u128 chunk_max = (u128)b + (WINDOW_CHUNKS - 1);
    for (size_t w = 0; w < n; ++w) {
        const uint64_t li = aocl_leaf_index[w];
        const u128 mn = ((u128)minimum[2 * w + 1] << 64) | minimum[2 * w];
        const uint32_t* dist = distances + (size_t)NUM_TRIALS * w;
        uint64_t keys[NUM_TRIALS];
        size_t nk = 0;
        if (aocl_leafs == 0 || (li != MS_UPDATE_NONE && li >= aocl_leafs)) {
            st[w] = NHIP_MS_NOT_IN_AOCL;
        } else {
            for (uint32_t t = 0; t < NUM_TRIALS; ++t) {
                const u128 index = mn + dist[t];  // AbsoluteIndexSet::to_array saturates: fail closed
                if (index < mn || (index >> CHUNK_BITS) > chunk_max) {
                    st[w] = NHIP_MS_OUT_OF_RANGE;
                    break;
                }
                const uint64_t ci = (uint64_t)(index >> CHUNK_BITS);
                if (ci < b) keys[nk++] = ci;
            }
        }
        uint64_t aocl_len = 0;
        if (st[w] == NHIP_MS_OK) {
            std::sort(keys, keys + nk);
            nk = (size_t)(std::unique(keys, keys + nk) - keys);
            if (li != MS_UPDATE_NONE) aocl_len = ms_arch_path_len(li, aocl_leafs);
        } else {
            nk = 0;
        }
        p.aocl_path_off[w + 1] = p.aocl_path_off[w] + aocl_len;
        for (size_t k = 0; k < nk; ++k) {
            const uint64_t c = keys[k];
            p.chunk_index.push_back(c);
            p.ent_wit.push_back((uint32_t)w);
            p.path_off.push_back(p.path_off.back() + ms_arch_path_len(c, b));
            const uint64_t words = p.rel_off.back() + chunk_len[c];
            if (words < p.rel_off.back() || words > MS_ARCHIVE_LIMIT) return NHIP_ERR_OOM;
            p.rel_off.push_back(words);
        }
        if (p.chunk_index.size() > 0xFFFFFFFFull) return NHIP_ERR_OOM;
        p.entry_off[w + 1] = p.chunk_index.size();
    }
    if (p.aocl_path_off[n] > MS_ARCHIVE_LIMIT || p.path_off.back() > MS_ARCHIVE_LIMIT) return NHIP_ERR_OOM;
    *plan = std::move(p);
    *status = std::move(st);
    return NHIP_OK;
}

namespace {

// the nodes above the leaves `leafs` (ascending, distinct) of an MMR of n leaves, level after level
void ancestors(const std::vector<uint64_t>& leafs, uint64_t n, std::vector<uint64_t>* ids, std::vector<uint32_t>* lvl_off) {
    ids->clear();
    lvl_off->assign(1, 0);
    std::vector<uint64_t> cur = leafs, next;
    for (uint32_t h = 1; h < 64 && (n >> h) != 0 && !cur.empty(); ++h) {
        next.clear();
        for (uint64_t k : cur) {
            const uint64_t p = k >> 1;
            if (p < (n >> h) && (next.empty() || next.back() != p)) next.push_back(p);  // exists: (p + 1) 2^h <= n
        }
        ids->insert(ids->end(), next.begin(), next.end());
        lvl_off->push_back((uint32_t)ids->size());
        cur.swap(next);
    }
}

}  // namespace

int ms_archive_apply_plan(const MsArchiveMirror& m, uint64_t additions, const uint64_t* minimum, const uint32_t* distances,
                          size_t records, MsArchApplyPlan* plan) {
    MsArchApplyPlan p;
    p.n0 = m.aocl_leafs;
    p.n1 = p.n0 + additions;
    if (p.n1 < p.n0 || p.n1 > MS_ARCHIVE_MAX_LEAFS || additions > 0xFFFFFFFFull || records > 0xFFFFFFFFull / NUM_TRIALS)
        return NHIP_ERR_OOM;
    p.b0 = MsJobScratch::batch_index(p.n0);
    p.b1 = MsJobScratch::batch_index(p.n1);
    // the block's indices below b1, as (chunk, relative) sorted; anything the block part rejects is skipped
    std::vector<std::pair<uint64_t, uint32_t>> hits;
    for (size_t r = 0; r < records; ++r) {
        const u128 mn = ((u128)minimum[2 * r + 1] << 64) | minimum[2 * r];
        for (uint32_t t = 0; t < NUM_TRIALS; ++t) {
            const u128 index = mn + distances[(size_t)NUM_TRIALS * r + t];
            if (index < mn || (index >> CHUNK_BITS) >= (u128)p.b1) continue;
            hits.emplace_back((uint64_t)(index >> CHUNK_BITS), (uint32_t)index & (MS_ARCHIVE_CHUNK_SIZE - 1));
        }
    }
    std::sort(hits.begin(), hits.end());
    p.block_rel.reserve(hits.size());
    for (const auto& h : hits) p.block_rel.push_back(h.second);
    uint64_t tail = m.rel_tail, live = m.rel_live;
    size_t i = 0;
    auto write = [&](uint64_t c, size_t h0, size_t h1) {
        MsArchWritten w{};
        w.c = c;
        if (c < p.b0) {
            w.a_off = m.chunk_off[(size_t)c];
            w.a_len = m.chunk_len[(size_t)c];
            live -= w.a_len;  // the old copy dies
        } else if (c - p.b0 < WINDOW_CHUNKS) {
            w.from_window = 1;
            w.a_sub = (c - p.b0) * MS_ARCHIVE_CHUNK_SIZE;
            const auto lo = std::lower_bound(m.window.begin(), m.window.end(), (uint32_t)w.a_sub);
            const auto hi = std::lower_bound(m.window.begin(), m.window.end(), (uint64_t)w.a_sub + MS_ARCHIVE_CHUNK_SIZE);
            w.a_off = (uint64_t)(lo - m.window.begin());
            w.a_len = (uint64_t)(hi - lo);
        }
        w.b_off = h0;
        w.b_len = h1 - h0;
        w.out_off = tail;
        tail += w.a_len + w.b_len;
        live += w.a_len + w.b_len;
        p.written.push_back(w);
    };
    // ascending in c: the touched chunks below b0, then every chunk of [b0, b1) with whatever hits it
    uint64_t next_new = p.b0;
    while (i < hits.size() || next_new < p.b1) {
        size_t j = i;
        const uint64_t hc = i < hits.size() ? hits[i].first : ~0ull;
        if (hc < p.b0 || (next_new < p.b1 && hc == next_new)) {
            while (j < hits.size() && hits[j].first == hc) ++j;
            write(hc, i, j);
            if (hc >= p.b0) ++next_new;
            i = j;
        } else {  // hc > next_new: a new chunk nothing hits
            write(next_new, i, i);
            ++next_new;
        }
        if (tail > MS_ARCHIVE_LIMIT || p.written.size() > 0xFFFFFFFFull) return NHIP_ERR_OOM;
    }
    p.rel_tail_after = tail;
    p.rel_live_after = live;
    p.compact = tail - live > live;
    std::vector<uint64_t> leafs;
    for (uint64_t l = p.n0; l < p.n1; ++l) leafs.push_back(l);
    ancestors(leafs, p.n1, &p.ids[0], &p.lvl_off[0]);
    leafs.clear();
    for (const MsArchWritten& w : p.written) leafs.push_back(w.c);
    ancestors(leafs, p.b1, &p.ids[1], &p.lvl_off[1]);
    *plan = std::move(p);
    return NHIP_OK;
}

void ms_archive_apply_commit(MsArchiveMirror& m, const MsArchApplyPlan& plan, const uint32_t* active, uint64_t n_active,
                             uint64_t aocl_cap, uint64_t swbf_cap) {
    std::vector<uint64_t> off = m.chunk_off, len = m.chunk_len;
    off.resize((size_t)plan.b1, 0);
    len.resize((size_t)plan.b1, 0);
    for (const MsArchWritten& w : plan.written) {
        off[(size_t)w.c] = w.out_off;
        len[(size_t)w.c] = w.a_len + w.b_len;
    }
    std::vector<uint32_t> window(active, active + (size_t)n_active);
    m.aocl_leafs = plan.n1;
    m.chunk_off = std::move(off);
    m.chunk_len = std::move(len);
    m.window = std::move(window);
    m.rel_tail = plan.rel_tail_after;
    m.rel_live = plan.rel_live_after;
    m.aocl_cap = aocl_cap;
    m.swbf_cap = swbf_cap;
}

void ms_archive_compact_commit(MsArchiveMirror& m) {
    uint64_t at = 0;
    for (size_t c = 0; c < m.chunk_len.size(); ++c) {
        m.chunk_off[c] = at;
        at += m.chunk_len[c];
    }
    m.rel_tail = m.rel_live = at;
}

int ms_archive_revert_plan(const MsArchiveMirror& m, uint64_t additions, const uint64_t* minimum, const uint32_t* distances,
                           size_t records, MsArchRevertPlan* plan) {
    if (records > 0xFFFFFFFFull / NUM_TRIALS) return NHIP_ERR_OOM;
    if (records && (!minimum || !distances)) return NHIP_ERR_ARG;
    if (additions > m.aocl_leafs) return MS_ARCHIVE_REVERT_IMPOSSIBLE;
    MsArchRevertPlan p;
    p.n1 = m.aocl_leafs;
    p.n0 = p.n1 - additions;
    p.b0 = MsJobScratch::batch_index(p.n0);
    p.b1 = m.chunks();
    if (p.b0 > p.b1) return MS_ARCHIVE_REVERT_IMPOSSIBLE;
    // the block's indices below b0, as (chunk, relative) sorted; those from b0 on lie in chunks that are dropped or in
    // the window, which is replaced whole
    std::vector<std::pair<uint64_t, uint32_t>> hits;
    for (size_t r = 0; r < records; ++r) {
        const u128 mn = ((u128)minimum[2 * r + 1] << 64) | minimum[2 * r];
        for (uint32_t t = 0; t < NUM_TRIALS; ++t) {
            const u128 index = mn + distances[(size_t)NUM_TRIALS * r + t];
            if (index < mn || (index >> CHUNK_BITS) >= (u128)p.b0) continue;
            hits.emplace_back((uint64_t)(index >> CHUNK_BITS), (uint32_t)index & (MS_ARCHIVE_CHUNK_SIZE - 1));
        }
    }
    std::sort(hits.begin(), hits.end());
    p.block_rel.reserve(hits.size());
    for (const auto& h : hits) p.block_rel.push_back(h.second);
    uint64_t tail = m.rel_tail, live = m.rel_live;
    for (size_t i = 0; i < hits.size();) {
        size_t j = i;
        while (j < hits.size() && hits[j].first == hits[i].first) ++j;
        MsArchWritten w{};
        w.c = hits[i].first;  // < b0 <= b1: inside the mirror's table
        w.a_off = m.chunk_off[(size_t)w.c];
        w.a_len = m.chunk_len[(size_t)w.c];
        w.b_off = i;
        w.b_len = j - i;
        if (w.a_len < w.b_len) return MS_ARCHIVE_REVERT_IMPOSSIBLE;
        w.out_off = tail;
        tail += w.a_len - w.b_len;
        if (tail < w.out_off || tail > MS_ARCHIVE_LIMIT || live < w.b_len) return NHIP_ERR_OOM;
        live -= w.b_len;  // the old copy dies, the new one is that much shorter
        p.rewritten.push_back(w);
        i = j;
    }
    for (uint64_t c = p.b0; c < p.b1; ++c) p.dropped_words += m.chunk_len[(size_t)c];
    if (live < p.dropped_words) return NHIP_ERR_OOM;  // a mirror whose live count is not the sum of its lengths
    live -= p.dropped_words;
    p.rel_tail_after = tail;
    p.rel_live_after = live;
    p.compact = tail - live > live;
    std::vector<uint64_t> leafs;
    for (const MsArchWritten& w : p.rewritten) leafs.push_back(w.c);
    ancestors(leafs, p.b0, &p.ids, &p.lvl_off);
    *plan = std::move(p);
    return NHIP_OK;
}

void ms_archive_revert_commit(MsArchiveMirror& m, const MsArchRevertPlan& plan, const uint32_t* active, uint64_t n_active) {
    std::vector<uint64_t> off(m.chunk_off.begin(), m.chunk_off.begin() + (size_t)plan.b0);
    std::vector<uint64_t> len(m.chunk_len.begin(), m.chunk_len.begin() + (size_t)plan.b0);
    for (const MsArchWritten& w : plan.rewritten) {
        off[(size_t)w.c] = w.out_off;
        len[(size_t)w.c] = w.a_len - w.b_len;
    }
    std::vector<uint32_t> window(active, active + (size_t)n_active);
    m.aocl_leafs = plan.n0;
    m.chunk_off = std::move(off);
    m.chunk_len = std::move(len);
    m.window = std::move(window);
    m.rel_tail = plan.rel_tail_after;
    m.rel_live = plan.rel_live_after;
}

size_t ms_archive_grown(size_t cap, size_t need, size_t limit) {
    if (need > limit) return 0;
    if (need <= cap) return cap;
    const size_t twice = cap > limit / 2 ? limit : 2 * cap;
    return std::max(need, twice);
}

MsArchUnits ms_arch_units(const uint64_t* off, size_t owners, uint64_t scale, bool pairs) {
    MsArchUnits u;
    const uint64_t per = pairs ? 2 * MS_ARCHIVE_GATHER_UNIT : MS_ARCHIVE_GATHER_UNIT;
    const uint64_t total = owners ? off[owners] * scale : 0;
    u.units = (total + per - 1) / per;
    u.first.assign((size_t)u.units + 1, owners ? (uint32_t)(owners - 1) : 0);
    size_t i = 0;
    for (uint64_t k = 0; k < u.units; ++k) {  // the last owner whose range begins at or before the unit's first word
        const uint64_t g = k * per;
        while (i + 1 < owners && off[i + 1] * scale <= g) ++i;
        u.first[(size_t)k] = (uint32_t)i;
    }
    return u;
}

}  // namespace nhip

extern "C" int nhip_ms_archive_restore_plan(uint64_t aocl_leafs, const uint64_t* chunk_len, uint64_t n_chunks,
                                            const uint64_t* minimum, const uint32_t* distances,
                                            const uint64_t* aocl_leaf_index, size_t n, nhip_ms_updated* out) {
    if (!out) return NHIP_ERR_ARG;
    try {
        nhip::MsUpdatePlan plan;
        std::vector<uint8_t> status;
        int rc = nhip::ms_archive_restore_plan(aocl_leafs, chunk_len, n_chunks, minimum, distances, aocl_leaf_index, n, &plan,
                                               &status);
        if (rc != NHIP_OK) return rc;
        if ((rc = nhip::ms_updated_check(plan, false, out)) != NHIP_OK) return rc;
        nhip::ms_updated_write(plan, true, out);
        if (out->status) std::copy(status.begin(), status.end(), out->status);
        return NHIP_OK;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}
