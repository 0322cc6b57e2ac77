#include "ms_store.hpp"

#include <algorithm>
#include <utility>

namespace nhip {

void ms_store_as_update_in(const MsStoreMirror& m, uint64_t wit_off[2], nhip_ms_chunks* chunks, nhip_ms_update_in* in) {
    wit_off[0] = 0;
    wit_off[1] = m.witnesses();
    *chunks = nhip_ms_chunks{m.entry_off.data(), m.key.data(), m.path_off.data(), nullptr, m.rel_off.data(), nullptr};
    *in = nhip_ms_update_in{wit_off, m.minimum.data(), m.distances.data(), m.leaf_index.data(), nullptr,
                            m.aocl_path_off.data(), nullptr, chunks};
}

int ms_store_append_plan(const MsStoreMirror& m, const nhip_ms_update_in* wit, size_t n, MsStoreAppend* a) {
    *a = MsStoreAppend{};
    if (n == 0) return NHIP_OK;
    if (!wit || n >= (size_t)UINT32_MAX) return NHIP_ERR_ARG;
    const uint64_t off[2] = {0, n};
    nhip_ms_update_in w = *wit;
    w.wit_off = off;
    nhip_ms_apply_in one{};
    one.n_jobs = 1;
    if (ms_update_ok(&one, &w, &a->add)) return NHIP_ERR_ARG;
    const MsUpdateCounts have = m.counts();
    const uint64_t W = have.witnesses + n, E = have.chunks.entries + a->add.chunks.entries;
    // every addend is below 2^63 (ms_csr_ok), so no sum wraps
    if (W >= (uint64_t)UINT32_MAX || E >= (uint64_t)UINT32_MAX || W > MS_STORE_LIMIT ||
        have.aocl_digests + a->add.aocl_digests > MS_STORE_LIMIT ||
        have.chunks.path_digests + a->add.chunks.path_digests > MS_STORE_LIMIT ||
        have.chunks.rel_words + a->add.chunks.rel_words > MS_STORE_LIMIT)
        return NHIP_ERR_OOM;
    const size_t ne = (size_t)a->add.chunks.entries;
    a->aocl_path_off.resize(n);
    a->entry_off.resize(n);
    a->path_off.resize(ne);
    a->rel_off.resize(ne);
    for (size_t i = 0; i < n; ++i) {
        a->aocl_path_off[i] = have.aocl_digests + wit->aocl_path_off[i + 1];
        a->entry_off[i] = have.chunks.entries + wit->chunks->entry_off[i + 1];
    }
    for (size_t e = 0; e < ne; ++e) {
        a->path_off[e] = have.chunks.path_digests + wit->chunks->path_off[e + 1];
        a->rel_off[e] = have.chunks.rel_words + wit->chunks->rel_off[e + 1];
    }
    return NHIP_OK;
}

void ms_store_append_commit(MsStoreMirror& m, const nhip_ms_update_in* wit, size_t n, const MsStoreAppend& a) {
    if (n == 0) return;
    const size_t W = m.witnesses(), E = m.entries(), ne = a.path_off.size();
    m.minimum.reserve(2 * (W + n));
    m.distances.reserve(45 * (W + n));
    m.leaf_index.reserve(W + n);
    m.aocl_path_off.reserve(W + n + 1);
    m.entry_off.reserve(W + n + 1);
    m.key.reserve(E + ne);
    m.path_off.reserve(E + ne + 1);
    m.rel_off.reserve(E + ne + 1);
    m.sticky.reserve(W + n);
    // nothing below allocates
    m.minimum.insert(m.minimum.end(), wit->minimum, wit->minimum + 2 * n);
    m.distances.insert(m.distances.end(), wit->distances, wit->distances + 45 * n);
    m.leaf_index.insert(m.leaf_index.end(), wit->aocl_leaf_index, wit->aocl_leaf_index + n);
    m.aocl_path_off.insert(m.aocl_path_off.end(), a.aocl_path_off.begin(), a.aocl_path_off.end());
    m.entry_off.insert(m.entry_off.end(), a.entry_off.begin(), a.entry_off.end());
    if (ne) m.key.insert(m.key.end(), wit->chunks->chunk_index, wit->chunks->chunk_index + ne);
    m.path_off.insert(m.path_off.end(), a.path_off.begin(), a.path_off.end());
    m.rel_off.insert(m.rel_off.end(), a.rel_off.begin(), a.rel_off.end());
    m.sticky.insert(m.sticky.end(), n, (uint8_t)NHIP_MS_OK);
}

int ms_store_restored_ok(const MsStoreMirror& m, size_t n, const uint64_t add[4]) {
    if (n >= (size_t)UINT32_MAX) return NHIP_ERR_ARG;
    const MsUpdateCounts have = m.counts();
    const uint64_t lim = MS_STORE_LIMIT;  // no sum wraps: each addend is compared alone first
    if (add[0] > lim || add[1] > lim || add[2] > lim || add[3] > lim) return NHIP_ERR_OOM;
    if (have.witnesses + n >= (uint64_t)UINT32_MAX || have.chunks.entries + add[1] >= (uint64_t)UINT32_MAX ||
        have.witnesses + n > lim || have.aocl_digests + add[0] > lim || have.chunks.path_digests + add[2] > lim ||
        have.chunks.rel_words + add[3] > lim)
        return NHIP_ERR_OOM;
    return NHIP_OK;
}

void ms_store_append_restored_commit(MsStoreMirror& m, const MsStoreRestored& r) {
    const size_t n = r.n;
    if (n == 0) return;
    const size_t W = m.witnesses(), E = m.entries(), ne = (size_t)r.entry_off[n];
    const MsUpdateCounts have = m.counts();
    m.minimum.reserve(2 * (W + n));
    m.distances.reserve(45 * (W + n));
    m.leaf_index.reserve(W + n);
    m.aocl_path_off.reserve(W + n + 1);
    m.entry_off.reserve(W + n + 1);
    m.key.reserve(E + ne);
    m.path_off.reserve(E + ne + 1);
    m.rel_off.reserve(E + ne + 1);
    m.sticky.reserve(W + n);
    // nothing below allocates
    m.minimum.insert(m.minimum.end(), r.minimum, r.minimum + 2 * n);
    m.distances.insert(m.distances.end(), r.distances, r.distances + 45 * n);
    m.leaf_index.insert(m.leaf_index.end(), r.leaf_index, r.leaf_index + n);
    for (size_t i = 0; i < n; ++i) {
        m.aocl_path_off.push_back(have.aocl_digests + r.aocl_path_off[i + 1]);
        m.entry_off.push_back(have.chunks.entries + r.entry_off[i + 1]);
    }
    for (size_t e = 0; e < ne; ++e) {
        m.key.push_back(r.chunk_index[e]);
        m.path_off.push_back(have.chunks.path_digests + r.path_off[e + 1]);
        m.rel_off.push_back(have.chunks.rel_words + r.rel_off[e + 1]);
    }
    m.sticky.insert(m.sticky.end(), n, (uint8_t)NHIP_MS_OK);
}

int ms_store_select(const MsStoreMirror& m, const uint64_t* sel, size_t n, MsStoreSelect* s) {
    *s = MsStoreSelect{};
    const size_t W = m.witnesses();
    if (!sel && n != W && n != 0) return NHIP_ERR_ARG;
    if (n > (size_t)MS_STORE_LIMIT) return NHIP_ERR_OOM;
    for (size_t i = 0; sel && i < n; ++i)
        if (sel[i] >= W) return NHIP_ERR_ARG;
    s->sel.resize(n);
    for (int p = 0; p < 4; ++p) {
        s->src[p].resize(n);
        s->dst[p].assign(n + 1, 0);
    }
    for (size_t i = 0; i < n; ++i) {
        const size_t w = sel ? (size_t)sel[i] : i;
        const size_t e0 = (size_t)m.entry_off[w], e1 = (size_t)m.entry_off[w + 1];
        const uint64_t beg[4] = {m.aocl_path_off[w], e0, m.path_off[e0], m.rel_off[e0]};
        const uint64_t end[4] = {m.aocl_path_off[w + 1], e1, m.path_off[e1], m.rel_off[e1]};
        s->sel[i] = w;
        for (int p = 0; p < 4; ++p) {
            s->src[p][i] = beg[p];
            s->dst[p][i + 1] = s->dst[p][i] + (end[p] - beg[p]);
            if (s->dst[p][i + 1] > MS_STORE_LIMIT) return NHIP_ERR_OOM;  // repeats can pass what the store holds
        }
    }
    if (s->total(1) >= (uint64_t)UINT32_MAX) return NHIP_ERR_OOM;
    const size_t E = (size_t)s->total(1);
    s->path_off.assign(E + 1, 0);
    s->rel_off.assign(E + 1, 0);
    for (size_t i = 0; i < n; ++i) {
        const size_t e0 = (size_t)s->src[1][i], d0 = (size_t)s->dst[1][i], len = (size_t)(s->dst[1][i + 1] - s->dst[1][i]);
        for (size_t k = 0; k < len; ++k) {
            s->path_off[d0 + k + 1] = s->dst[2][i] + (m.path_off[e0 + k + 1] - m.path_off[e0]);
            s->rel_off[d0 + k + 1] = s->dst[3][i] + (m.rel_off[e0 + k + 1] - m.rel_off[e0]);
        }
    }
    // the work units: elements of dst[p] per unit, and the owner of each unit's first element by one sweep
    const uint64_t per_unit[4] = {MS_STORE_GATHER_UNIT, MS_STORE_GATHER_UNIT, MS_STORE_GATHER_UNIT, 2 * MS_STORE_GATHER_UNIT};
    const uint64_t scale[4] = {5, 1, 5, 1};
    uint64_t at = 0;
    for (int p = 0; p < 4; ++p) {
        const uint64_t total = s->total(p) * scale[p], units = (total + per_unit[p] - 1) / per_unit[p];
        size_t i = 0;
        for (uint64_t u = 0; u < units; ++u) {
            while (s->dst[p][i + 1] * scale[p] <= u * per_unit[p]) ++i;  // u * per_unit < total: ends below n
            s->unit_first.push_back((uint32_t)i);
        }
        s->unit_first.push_back(n ? (uint32_t)(n - 1) : 0u);
        s->unit_end[p] = at += units;
    }
    return NHIP_OK;
}

std::vector<uint64_t> ms_store_kept(const uint8_t* keep, size_t W) {
    std::vector<uint64_t> sel;
    for (size_t w = 0; w < W; ++w)
        if (keep[w]) sel.push_back(w);
    return sel;
}

MsStoreMirror ms_store_selected_mirror(const MsStoreMirror& m, const MsStoreSelect& s) {
    MsStoreMirror o;
    const size_t n = s.n();
    o.minimum.reserve(2 * n);
    o.distances.reserve(45 * n);
    for (size_t i = 0; i < n; ++i) {
        const size_t w = (size_t)s.sel[i];
        o.minimum.insert(o.minimum.end(), m.minimum.begin() + 2 * w, m.minimum.begin() + 2 * w + 2);
        o.distances.insert(o.distances.end(), m.distances.begin() + 45 * w, m.distances.begin() + 45 * w + 45);
        o.leaf_index.push_back(m.leaf_index[w]);
        o.sticky.push_back(m.sticky[w]);
        const size_t e0 = (size_t)s.src[1][i], len = (size_t)(s.dst[1][i + 1] - s.dst[1][i]);
        o.key.insert(o.key.end(), m.key.begin() + e0, m.key.begin() + e0 + len);
    }
    o.aocl_path_off = s.dst[0];
    o.entry_off = s.dst[1];
    o.path_off = s.path_off;
    o.rel_off = s.rel_off;
    return o;
}

void ms_store_apply_plan(MsStoreMirror& m, MsUpdatePlan&& plan, const uint8_t* status) {
    m.aocl_path_off = std::move(plan.aocl_path_off);
    m.entry_off = std::move(plan.entry_off);
    m.key = std::move(plan.chunk_index);
    m.path_off = std::move(plan.path_off);
    m.rel_off = std::move(plan.rel_off);
    std::copy(status, status + m.witnesses(), m.sticky.begin());
}

size_t ms_store_grown(size_t cap, size_t need, size_t limit) {
    if (need > limit) return 0;
    if (need <= cap) return cap;
    const size_t twice = cap > limit / 2 ? limit : 2 * cap;
    return std::max(need, twice);
}

}  // namespace nhip
