// C-ABI layer of the device-resident archival mutator set (nhip_ms_archive_*; declarations: include/neptune_hip.h;
// DESIGN.md §6k).  The archive owns its device buffers (hipMalloc, not the context's workspace, which every other call
// recycles): the level arrays of the two MMRs, the chunk arena and its table, the window.  The host side is
// ms_archive.cpp (the mirror and every shape decision); the kernels are ms_archive_kernels.hip's.
#include <algorithm>
#include <new>
#include <vector>

#include "ms_parts.hpp"
#include "ms_archive.hpp"
#include "ms_archive_device.hpp"
#include "ms_restore_device.hpp"

namespace {

// One device array of the archive; never null once a load or an apply has sized it.
template <class T>
struct Arr {
    T* p = nullptr;
    size_t cap = 0;  // elements
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// New buffers for the arrays that have to grow, allocated first and swapped in together: until take() the archive's
// arrays are as they were, and drop() (or the destructor) frees what was allocated.
struct Fresh {
    struct One {
        void** slot;
        size_t* cap;
        void* fresh;
        size_t new_cap;
    };
    std::vector<One> all;
    ~Fresh() { drop(); }
    // use: the buffer the call works on, the fresh one when the array grows (geometrically, as ms_store_grown)
    template <class T>
    int want(Arr<T>& a, size_t need, T** use, bool* grown = nullptr) {
        need = std::max<size_t>(need, 1);
        if (grown) *grown = false;
        if (a.p && need <= a.cap) {
            *use = a.p;
            return NHIP_OK;
        }
        const size_t cap = nhip::ms_archive_grown(a.cap, need, SIZE_MAX / 64);
        if (!cap) return NHIP_ERR_OOM;
        T* q = nullptr;
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&q), cap * sizeof(T));
        if (e != hipSuccess) return nhip::hip_fail(e);
        all.push_back(One{reinterpret_cast<void**>(&a.p), &a.cap, q, cap});
        *use = q;
        if (grown) *grown = true;
        return NHIP_OK;
    }
    void take() {
        for (One& o : all) {
            if (*o.slot) (void)hipFree(*o.slot);
            *o.slot = o.fresh;
            *o.cap = o.new_cap;
        }
        all.clear();
    }
    void drop() {
        for (One& o : all) (void)hipFree(o.fresh);
        all.clear();
    }
};

}  // namespace

struct nhip_ms_archive {
    nhip_ctx* c = nullptr;
    nhip::MsArchiveMirror m;
    nhip_ms_archive_caps floor{};  // the initial capacities asked for
    Arr<uint64_t> nodes[2];        // 0 AOCL, 1 SWBF: 2 cap digests each
    Arr<uint64_t> tab;             // per chunk: offset, length
    Arr<uint32_t> arena, window;
    bool poisoned = false;         // a HIP error behind a launch that writes archive state: nothing is read any more

    nhip::MsArchLevels levels(int which) const {
        return which == 0 ? nhip::MsArchLevels{nodes[0].p, m.aocl_cap, m.aocl_leafs}
                          : nhip::MsArchLevels{nodes[1].p, m.swbf_cap, m.chunks()};
    }
};

namespace {

// every level above the leaves of both MMRs: k_ms_arch_level while a level is wide, one k_ms_arch_tail for the rest
void enqueue_build(Stage& st, nhip_ctx* c, const nhip::MsArchLevels lv[2]) {
    uint32_t from[2], top[2];
    for (int w = 0; w < 2; ++w) {
        const nhip::MsArchBuild b = nhip::ms_arch_build(lv[w].n);
        for (uint32_t h = 1; h <= b.wide_levels; ++h)
            st.launch([&] { return nhip::launch_ms_arch_level(lv[w], h, 0, lv[w].n >> h, c->stream); });
        from[w] = b.tail_from;
        top[w] = b.top;
    }
    st.launch([&] { return nhip::launch_ms_arch_tail(lv, from, top, c->stream); });
}

// the three pools of one gather: AOCL paths per witness, SWBF paths and chunk words per entry (either side may be
// absent: units 0)
struct GatherPlan {
    nhip::MsArchUnits units[3];
    nhip::MsArchGatherDev g{};
};

// The arena's compaction behind an apply or a revert that leaves more dead words than live ones: one gather of every
// chunk into a second arena (`spare`, rel_live words) and the table of that arena (d_tab2); the caller swaps both in.
struct Compaction {
    std::vector<uint64_t> scan, tab2;
    nhip::MsArchUnits units;
    // after: the mirror behind the call's writes, before ms_archive_compact_commit
    void plan(const nhip::MsArchiveMirror& after) {
        const size_t n = (size_t)after.chunks();
        scan.assign(n + 1, 0);
        for (size_t k = 0; k < n; ++k) scan[k + 1] = scan[k] + after.chunk_len[k];
        units = nhip::ms_arch_units(scan.data(), n, 1, true);
        tab2.resize(2 * n);
        for (size_t k = 0; k < n; ++k) tab2[2 * k] = scan[k], tab2[2 * k + 1] = after.chunk_len[k];
    }
    bool moves() const { return !scan.empty() && scan.back() != 0; }  // no live word: nothing to gather
    // behind a drained stream (the plan's device arrays are no longer needed): a small phase with buffers of its own
    int run(Stage& st, nhip_ctx* c, const uint64_t* d_tab, const uint32_t* d_arena, uint32_t* spare, uint64_t* d_tab2) {
        if (!moves()) return NHIP_OK;
        uint64_t* d_scan = nullptr;
        uint32_t* d_first = nullptr;
        int rc;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&d_scan), 8 * scan.size());
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_first), 4 * units.first.size());
        if (e == hipSuccess) {
            st.up(d_scan, scan.data(), scan.size());
            st.up(d_first, units.first.data(), units.first.size());
            nhip::MsArchGatherDev g{};
            g.rel.tab = d_tab, g.rel.arena = d_arena, g.rel.key = nullptr, g.rel.dst_off = d_scan;
            g.rel.owners = scan.size() - 1, g.rel.units = units.units, g.rel.first = d_first, g.rel.dst = spare;
            st.launch([&] { return nhip::launch_ms_arch_gather(g, c->stream); });
            st.up(d_tab2, tab2.data(), tab2.size());
            rc = st.finish();
        } else {
            rc = nhip::hip_fail(e);
        }
        if (d_scan) (void)hipFree(d_scan);
        if (d_first) (void)hipFree(d_first);
        return rc;
    }
};

}  // namespace

extern "C" {

int nhip_ms_archive_create(nhip_ctx* c, const nhip_ms_archive_caps* initial, nhip_ms_archive** out) {
    if (!c || !out) return NHIP_ERR_ARG;
    if (initial && (initial->aocl_leafs > nhip::MS_ARCHIVE_MAX_LEAFS || initial->chunks > nhip::MS_ARCHIVE_MAX_LEAFS ||
                    initial->rel_words > SIZE_MAX / 4096))
        return NHIP_ERR_ARG;
    nhip_ms_archive* a = new (std::nothrow) nhip_ms_archive;
    if (!a) return NHIP_ERR_OOM;
    a->c = c;
    if (initial) a->floor = *initial;
    *out = a;
    return NHIP_OK;
}

void nhip_ms_archive_destroy(nhip_ms_archive* a) {
    if (!a) return;
    {
        Stage st(a->c);  // the context's lock and device
        (void)hipStreamSynchronize(a->c->stream);
        a->nodes[0].release(), a->nodes[1].release(), a->tab.release(), a->arena.release(), a->window.release();
    }
    delete a;
}

int nhip_ms_archive_count(const nhip_ms_archive* a, uint64_t* aocl_leafs, uint64_t* chunks, uint64_t* n_active,
                          uint64_t* rel_live, uint64_t* rel_dead) {
    if (!a) return NHIP_ERR_ARG;
    const std::lock_guard<std::mutex> lock(a->c->mu);
    if (a->poisoned) return NHIP_ERR_HIP;
    if (aocl_leafs) *aocl_leafs = a->m.aocl_leafs;
    if (chunks) *chunks = a->m.chunks();
    if (n_active) *n_active = a->m.window.size();
    if (rel_live) *rel_live = a->m.rel_live;
    if (rel_dead) *rel_dead = a->m.rel_dead();
    return NHIP_OK;
}

int nhip_ms_archive_load(nhip_ms_archive* a, const uint64_t* aocl_leaves, uint64_t n_leafs, const uint64_t* rel_off,
                         const uint32_t* rel, uint64_t n_chunks, const uint32_t* active, uint64_t n_active) {
    if (!a) return NHIP_ERR_ARG;
    nhip_ctx* c = a->c;
    try {
        Stage st(c);
        if (a->poisoned) return NHIP_ERR_HIP;
        if (!a->m.empty()) return NHIP_ERR_ARG;
        int rc = nhip::ms_archive_load_ok(aocl_leaves, n_leafs, rel_off, rel, n_chunks, active, n_active);
        if (rc != NHIP_OK) return rc;
        const uint64_t aocl_cap = nhip::ms_arch_level_cap(n_leafs, a->floor.aocl_leafs);
        const uint64_t swbf_cap = nhip::ms_arch_level_cap(n_chunks, a->floor.chunks);
        if (!aocl_cap || !swbf_cap) return NHIP_ERR_OOM;
        nhip::MsArchiveMirror after;
        nhip::ms_archive_load_commit(after, n_leafs, rel_off, n_chunks, active, n_active, aocl_cap, swbf_cap);
        std::vector<uint64_t> tab(2 * (size_t)n_chunks);
        for (size_t k = 0; k < (size_t)n_chunks; ++k) {
            tab[2 * k] = after.chunk_off[k];
            tab[2 * k + 1] = after.chunk_len[k];
        }
        // all allocation before the first write, and every new buffer before any is swapped in
        Fresh fresh;
        uint64_t *aocl_nodes, *swbf_nodes, *d_tab;
        uint32_t *d_arena, *d_window;
        if ((rc = fresh.want(a->nodes[0], 10 * (size_t)aocl_cap, &aocl_nodes)) != NHIP_OK) return rc;
        if ((rc = fresh.want(a->nodes[1], 10 * (size_t)swbf_cap, &swbf_nodes)) != NHIP_OK) return rc;
        if ((rc = fresh.want(a->tab, 2 * (size_t)std::max<uint64_t>(n_chunks, a->floor.chunks), &d_tab)) != NHIP_OK) return rc;
        if ((rc = fresh.want(a->arena, (size_t)std::max<uint64_t>(after.rel_tail, a->floor.rel_words), &d_arena)) != NHIP_OK)
            return rc;
        if ((rc = fresh.want(a->window, (size_t)n_active, &d_window)) != NHIP_OK) return rc;
        fresh.take();  // an empty archive: nothing to keep
        const nhip::MsArchLevels lv[2] = {{a->nodes[0].p, aocl_cap, n_leafs}, {a->nodes[1].p, swbf_cap, n_chunks}};
        // the only time a leaf, a chunk word or the window crosses to the device
        st.up(a->nodes[0].p, aocl_leaves, 5 * (size_t)n_leafs);
        st.up(a->arena.p, rel, (size_t)after.rel_tail);
        st.up(a->tab.p, tab.data(), tab.size());
        st.up(a->window.p, active, (size_t)n_active);
        st.launch([&] { return nhip::launch_ms_arch_chunk_digests(a->tab.p, a->arena.p, 0, n_chunks, nullptr, lv[1], c->stream); });
        enqueue_build(st, c, lv);
        if ((rc = st.finish()) != NHIP_OK) {
            a->poisoned = true;  // the mirror still says "empty", the buffers may hold anything
            return rc;
        }
        a->m = std::move(after);
        return NHIP_OK;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

int nhip_ms_archive_accumulator(nhip_ms_archive* a, nhip_ms_apply_out* out) {
    if (!a || !out) return NHIP_ERR_ARG;
    if (!out->aocl_peaks || !out->aocl_n_peaks || !out->aocl_num_leafs || !out->swbf_peaks || !out->swbf_n_peaks ||
        !out->swbf_num_leafs || !out->active_off || !out->n_active || out->active_off[1] < out->active_off[0])
        return NHIP_ERR_ARG;
    nhip_ctx* c = a->c;
    try {
        Stage st(c);
        if (a->poisoned) return NHIP_ERR_HIP;
        const size_t n_active = a->m.window.size();
        if (out->active_off[1] - out->active_off[0] < n_active || (n_active && !out->active)) return NHIP_ERR_ARG;
        // read back into temporaries first: the outputs stay untouched unless the whole call succeeds
        std::vector<uint64_t> peaks(2 * 64 * 5, 0);
        std::vector<uint32_t> window(n_active);
        if (!a->m.empty()) {
            const nhip::MsArchLevels lv[2] = {a->levels(0), a->levels(1)};
            uint64_t* d_peaks;
            st.tmp(d_peaks, 2 * 64, 5);
            if (st.commit()) return st.finish();
            st.launch([&] { return nhip::launch_ms_arch_peaks(lv, d_peaks, c->stream); });
            st.out(peaks.data(), d_peaks, peaks.size());
            st.out(window.data(), a->window.p, n_active);
            if (const int rc = st.finish()) return rc;
        }
        const uint64_t n[2] = {a->m.aocl_leafs, a->m.chunks()};
        const uint32_t np[2] = {(uint32_t)__builtin_popcountll(n[0]), (uint32_t)__builtin_popcountll(n[1])};
        std::copy(peaks.begin(), peaks.begin() + 5 * np[0], out->aocl_peaks);
        std::copy(peaks.begin() + 320, peaks.begin() + 320 + 5 * np[1], out->swbf_peaks);
        out->aocl_n_peaks[0] = np[0], out->swbf_n_peaks[0] = np[1];
        out->aocl_num_leafs[0] = n[0], out->swbf_num_leafs[0] = n[1];
        if (n_active) std::copy(window.begin(), window.end(), out->active + out->active_off[0]);
        out->n_active[0] = n_active;
        if (out->verdict) out->verdict[0] = 1;
        if (out->status) out->status[0] = NHIP_MS_OK;
        if (out->bad_record) out->bad_record[0] = UINT64_MAX;
        return NHIP_OK;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

int nhip_ms_archive_paths(nhip_ms_archive* a, int which, const uint64_t* leaf_index, size_t n, uint64_t* path_off,
                          uint64_t* path, size_t path_cap, size_t* path_digests) {
    if (!a || (which != 0 && which != 1) || !path_digests) return NHIP_ERR_ARG;
    nhip_ctx* c = a->c;
    try {
        Stage st(c);
        if (a->poisoned) return NHIP_ERR_HIP;
        const nhip::MsArchLevels lv = a->levels(which);
        std::vector<uint64_t> off;
        int rc = nhip::ms_archive_paths_plan(lv.n, leaf_index, n, &off);
        if (rc != NHIP_OK) return rc;
        const size_t total = (size_t)off[n];
        if (!path_off && !path) {  // the count pass: from the mirror alone
            *path_digests = total;
            return NHIP_OK;
        }
        if (!path_off || path_cap < total || (total && !path)) return NHIP_ERR_ARG;
        if (total) {
            GatherPlan gp;
            gp.units[0] = nhip::ms_arch_units(off.data(), n, 5, false);
            nhip::MsArchPathPool& p = gp.g.path[0];
            p.mmr = lv;
            p.owners = n;
            p.units = gp.units[0].units;
            st.in(p.leaf, leaf_index, n);
            st.in(p.dst_off, off.data(), n + 1);
            st.in(p.first, gp.units[0].first.data(), gp.units[0].first.size());
            st.tmp(p.dst, total, 5);
            if (st.commit()) return st.finish();
            st.launch([&] { return nhip::launch_ms_arch_gather(gp.g, c->stream); });
            st.out(path, p.dst, 5 * total);
            if ((rc = st.finish()) != NHIP_OK) return rc;
        }
        std::copy(off.begin(), off.end(), path_off);
        *path_digests = total;
        return NHIP_OK;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

int nhip_ms_archive_leaves(nhip_ms_archive* a, int which, uint64_t first, uint64_t n, uint64_t* out) {
    if (!a || (which != 0 && which != 1)) return NHIP_ERR_ARG;
    nhip_ctx* c = a->c;
    try {
        Stage st(c);
        if (a->poisoned) return NHIP_ERR_HIP;
        const nhip::MsArchLevels lv = a->levels(which);
        if (first > lv.n || n > lv.n - first || (n && !out)) return NHIP_ERR_ARG;
        if (n) st.out(out, lv.nodes, 5 * (size_t)n, 5 * (size_t)first);  // level 0 begins the array
        return st.finish();
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

// ArchivalState::update_mutator_set's forward step as an end state.  The block runs through the block part (steps 1-5
// of nhip_ms_apply_batch) with msa_before checked against the archive's own accumulator first; on NHIP_MS_OK the
// chunks the block creates or hits are merged to the arena's tail, hashed, and both MMRs get their new leaves and every
// node above a new or changed leaf hashed again from the archive's own level arrays.
int nhip_ms_archive_apply(nhip_ms_archive* a, const nhip_ms_apply_in* block, nhip_ms_apply_out* block_out) {
    nhip::MsApplyCounts cnt;
    if (!a || !block || block->n_jobs != 1 || nhip::ms_apply_ok(block, block_out, &cnt) || !cnt.accumulators) return NHIP_ERR_ARG;
    nhip_ctx* c = a->c;
    try {
        Stage st(c);
        if (a->poisoned) return NHIP_ERR_HIP;
        nhip::MsArchiveMirror& m = a->m;
        const nhip_msa& before = block->msa_before[0];
        nhip::MsArchApplyPlan plan;
        int rc = nhip::ms_archive_apply_plan(m, cnt.additions, block->minimum, block->distances, (size_t)cnt.records, &plan);
        if (rc != NHIP_OK) return rc;
        const size_t NW = plan.written.size();
        // msa_before against the archive: the counts and the window against the mirror, the peaks against the device's
        std::vector<uint32_t> given;
        nhip::ms_append_sorted_window(given, before);
        bool same = before.aocl.num_leafs == m.aocl_leafs && before.swbf_inactive.num_leafs == m.chunks() &&
                    before.aocl.n_peaks == (uint32_t)__builtin_popcountll(m.aocl_leafs) &&
                    before.swbf_inactive.n_peaks == (uint32_t)__builtin_popcountll(m.chunks()) && given == m.window;
        BlockPart blk(*block, *block_out, cnt, false);
        const nhip::MsArchWritten* d_written;
        const uint32_t *d_block_rel, *d_off[2];
        const uint64_t* d_ids[2];
        uint64_t* d_peaks;
        std::vector<uint64_t> peaks(2 * 64 * 5, 0);
        blk.declare(st);
        st.in(d_written, plan.written.data(), NW);
        st.in(d_block_rel, plan.block_rel.data(), plan.block_rel.size());
        for (int w = 0; w < 2; ++w) {
            st.in(d_ids[w], plan.ids[w].data(), plan.ids[w].size());
            st.in(d_off[w], plan.lvl_off[w].data(), plan.lvl_off[w].size());
        }
        st.tmp(d_peaks, 2 * 64, 5);
        if (st.commit()) return st.finish();
        blk.enqueue(st, c);
        blk.read_back(st);
        if (!m.empty() && a->nodes[0].p) {
            const nhip::MsArchLevels lv[2] = {a->levels(0), a->levels(1)};
            st.launch([&] { return nhip::launch_ms_arch_peaks(lv, d_peaks, c->stream); });
            st.out(peaks.data(), d_peaks, peaks.size());
        }
        if ((rc = st.finish()) != NHIP_OK) return rc;  // nothing of the archive was written
        blk.write_outputs();
        if (same) {
            same = std::equal(before.aocl.peaks, before.aocl.peaks + 5 * (size_t)before.aocl.n_peaks, peaks.begin()) &&
                   std::equal(before.swbf_inactive.peaks, before.swbf_inactive.peaks + 5 * (size_t)before.swbf_inactive.n_peaks,
                              peaks.begin() + 320);
        }
        if (!same) {  // as nhip_ms_apply_batch reports an inconsistent msa_before
            block_out->verdict[0] = 0;
            block_out->status[0] = NHIP_MS_INCONSISTENT;
            block_out->bad_record[0] = UINT64_MAX;
            block_out->aocl_n_peaks[0] = block_out->swbf_n_peaks[0] = 0;
            block_out->aocl_num_leafs[0] = block_out->swbf_num_leafs[0] = block_out->n_active[0] = 0;
            return NHIP_OK;
        }
        if (block_out->status[0] != NHIP_MS_OK) return NHIP_OK;  // the archive stays as it was
        if (block_out->aocl_num_leafs[0] != plan.n1 || block_out->swbf_num_leafs[0] != plan.b1) return NHIP_ERR_HIP;
        const uint32_t* active_after = block_out->active + block_out->active_off[0];
        const uint64_t n_after = block_out->n_active[0];
        // ---- all allocation and growth before the first launch that writes archive state; the old arrays are read only
        const uint64_t aocl_cap = nhip::ms_arch_level_cap(plan.n1, std::max<uint64_t>(m.aocl_cap, a->floor.aocl_leafs));
        const uint64_t swbf_cap = nhip::ms_arch_level_cap(plan.b1, std::max<uint64_t>(m.swbf_cap, a->floor.chunks));
        if (!aocl_cap || !swbf_cap) return NHIP_ERR_OOM;
        Fresh fresh;
        uint64_t *nodes[2], *d_tab;
        uint32_t *d_arena, *d_window;
        bool grown[2], tab_grown, arena_grown;
        // a level array that changes its capacity changes its layout: always a fresh one then
        for (int w = 0; w < 2; ++w) {
            const uint64_t cap = w ? swbf_cap : aocl_cap, old = w ? m.swbf_cap : m.aocl_cap;
            if (cap != old || !a->nodes[w].p) {
                uint64_t* q = nullptr;  // a new buffer of exactly 2 cap digests
                const hipError_t e = hipMalloc(reinterpret_cast<void**>(&q), 10 * (size_t)cap * sizeof(uint64_t));
                if (e != hipSuccess) return nhip::hip_fail(e);
                fresh.all.push_back(Fresh::One{reinterpret_cast<void**>(&a->nodes[w].p), &a->nodes[w].cap, q, 10 * (size_t)cap});
                nodes[w] = q;
                grown[w] = true;
            } else {
                nodes[w] = a->nodes[w].p;
                grown[w] = false;
            }
        }
        if ((rc = fresh.want(a->tab, 2 * (size_t)plan.b1, &d_tab, &tab_grown)) != NHIP_OK) return rc;
        if ((rc = fresh.want(a->arena, (size_t)plan.rel_tail_after, &d_arena, &arena_grown)) != NHIP_OK) return rc;
        if ((rc = fresh.want(a->window, (size_t)n_after, &d_window)) != NHIP_OK) return rc;
        Arr<uint32_t> spare;  // the second arena of a compaction
        uint64_t* d_tab2 = nullptr;
        if (plan.compact) {
            hipError_t e = hipMalloc(reinterpret_cast<void**>(&spare.p), std::max<size_t>((size_t)plan.rel_live_after, 1) * 4);
            if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_tab2), std::max<size_t>(2 * (size_t)plan.b1, 1) * 8);
            if (e != hipSuccess) {
                spare.release();
                return nhip::hip_fail(e);
            }
        }
        auto bail = [&](int code) {
            spare.release();
            if (d_tab2) (void)hipFree(d_tab2);
            return code;
        };
        // device-to-device copies of what stays, into the fresh buffers
        auto d2d = [&](void* dst, const void* src, size_t bytes) {
            if (bytes) st.step([&] { return nhip::hip_fail(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream)); });
        };
        for (int w = 0; w < 2; ++w) {
            const uint64_t old_cap = w ? m.swbf_cap : m.aocl_cap, cap = w ? swbf_cap : aocl_cap;
            if (!grown[w] || !a->nodes[w].p || (w ? m.chunks() : m.aocl_leafs) == 0) continue;
            const uint64_t have = w ? m.chunks() : m.aocl_leafs;
            for (uint32_t h = 0; (have >> h) != 0; ++h)
                d2d(nodes[w] + 5 * nhip::ms_arch_level_base(cap, h), a->nodes[w].p + 5 * nhip::ms_arch_level_base(old_cap, h),
                    40 * (size_t)(have >> h));
        }
        if (tab_grown && a->tab.p) d2d(d_tab, a->tab.p, 16 * (size_t)m.chunks());
        if (arena_grown && a->arena.p) d2d(d_arena, a->arena.p, 4 * (size_t)m.rel_tail);
        if ((rc = st.finish()) != NHIP_OK) return bail(rc);  // the fresh buffers are dropped, the archive is as it was
        // the old window is read by the chunk merge and the new one is written behind it: keep the old buffer alive
        const uint32_t* old_window = a->window.p;
        const bool window_fresh = d_window != a->window.p;
        uint32_t* d_old_window = nullptr;
        if (!window_fresh && !m.window.empty()) {  // the merge reads the old words while the upload overwrites them: a copy
            const hipError_t e = hipMalloc(reinterpret_cast<void**>(&d_old_window), 4 * m.window.size());
            if (e != hipSuccess) return bail(nhip::hip_fail(e));
            d2d(d_old_window, a->window.p, 4 * m.window.size());
            if ((rc = st.finish()) != NHIP_OK) {
                (void)hipFree(d_old_window);
                return bail(rc);
            }
            old_window = d_old_window;
        }
        // ---- from here on the archive is written: a HIP error poisons it
        nhip::MsArchiveMirror after = m;
        nhip::ms_archive_apply_commit(after, plan, active_after, n_after, aocl_cap, swbf_cap);
        const nhip::MsArchLevels lv[2] = {{nodes[0], aocl_cap, plan.n1}, {nodes[1], swbf_cap, plan.b1}};
        st.up(nodes[0] + 5 * (size_t)plan.n0, block->additions, 5 * (size_t)cnt.additions);  // level 0 begins the array
        st.launch([&] { return nhip::launch_ms_arch_chunks(d_written, NW, d_block_rel, old_window, d_arena, d_tab, c->stream); });
        st.launch([&] { return nhip::launch_ms_arch_chunk_digests(d_tab, d_arena, 0, NW, d_written, lv[1], c->stream); });
        const uint32_t levels[2] = {(uint32_t)plan.lvl_off[0].size() - 1, (uint32_t)plan.lvl_off[1].size() - 1};
        st.launch([&] { return nhip::launch_ms_arch_ancestors(lv, d_ids, d_off, levels, c->stream); });
        st.up(d_window, active_after, (size_t)n_after);
        Compaction compaction;
        if (plan.compact) compaction.plan(after);
        rc = st.finish();
        if (rc == NHIP_OK && plan.compact) rc = compaction.run(st, c, d_tab, d_arena, spare.p, d_tab2);
        if (d_old_window) (void)hipFree(d_old_window);
        if (rc != NHIP_OK) {
            fresh.take();  // what the launches wrote into; nothing is read from it again
            a->poisoned = true;
            return bail(rc);
        }
        fresh.take();
        if (plan.compact) {
            if (compaction.moves()) {
                a->arena.release();
                a->arena.p = spare.p, a->arena.cap = std::max<size_t>((size_t)plan.rel_live_after, 1);
                spare.p = nullptr;
                a->tab.release();
                a->tab.p = d_tab2, a->tab.cap = std::max<size_t>(2 * (size_t)plan.b1, 1);
                d_tab2 = nullptr;
            }
            nhip::ms_archive_compact_commit(after);
        }
        bail(NHIP_OK);
        m = std::move(after);
        return NHIP_OK;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

// ArchivalState::update_mutator_set's walk back over an abandoned block as an end state (MsArchRevertPlan).  The block
// runs through the block part on (msa_before, block); the accumulator it computes has to be the archive's own (the tip
// check) before anything is written.  Then the rewritten chunks lose the block's indices at the arena's tail, are
// hashed, the SWBF nodes above them that exist at b0 are hashed again, the window before is uploaded, and the peaks at
// (n0, b0) are read back against msa_before's together with the kernel's short-of flag.
int nhip_ms_archive_revert(nhip_ms_archive* a, const nhip_ms_apply_in* block, nhip_ms_apply_out* block_out) {
    nhip::MsApplyCounts cnt;
    if (!a || !block || block->n_jobs != 1 || nhip::ms_apply_ok(block, block_out, &cnt) || !cnt.accumulators) return NHIP_ERR_ARG;
    nhip_ctx* c = a->c;
    try {
        Stage st(c);
        if (a->poisoned) return NHIP_ERR_HIP;
        nhip::MsArchiveMirror& m = a->m;
        const nhip_msa& before = block->msa_before[0];
        nhip::MsArchRevertPlan plan;
        int rc = nhip::ms_archive_revert_plan(m, cnt.additions, block->minimum, block->distances, (size_t)cnt.records, &plan);
        const bool impossible = rc == nhip::MS_ARCHIVE_REVERT_IMPOSSIBLE;  // reported behind the block part's own status
        if (rc != NHIP_OK && !impossible) return rc;
        const size_t NR = plan.rewritten.size();
        std::vector<uint32_t> window_before;
        nhip::ms_append_sorted_window(window_before, before);
        const bool have_nodes = !m.empty() && a->nodes[0].p && a->nodes[1].p;
        BlockPart blk(*block, *block_out, cnt, false);
        const nhip::MsArchWritten* d_rewritten;
        const uint32_t *d_block_rel, *d_off;
        const uint64_t* d_ids;
        uint64_t* d_peaks;  // the tip's, then those after the writes
        uint32_t* d_short_of;
        const uint32_t zero = 0;
        uint32_t short_of = 0;
        std::vector<uint64_t> peaks(2 * 64 * 5, 0), peaks_after(2 * 64 * 5, 0);
        blk.declare(st);
        st.in(d_rewritten, plan.rewritten.data(), NR);
        st.in(d_block_rel, plan.block_rel.data(), plan.block_rel.size());
        st.in(d_ids, plan.ids.data(), plan.ids.size());
        st.in(d_off, plan.lvl_off.data(), plan.lvl_off.size());
        st.in(d_short_of, &zero, 1);
        st.tmp(d_peaks, 4 * 64, 5);
        if (st.commit()) return st.finish();
        blk.enqueue(st, c);
        blk.read_back(st);
        if (have_nodes) {
            const nhip::MsArchLevels lv[2] = {a->levels(0), a->levels(1)};
            st.launch([&] { return nhip::launch_ms_arch_peaks(lv, d_peaks, c->stream); });
            st.out(peaks.data(), d_peaks, peaks.size());
        }
        if ((rc = st.finish()) != NHIP_OK) return rc;  // nothing of the archive was written
        blk.write_outputs();
        if (block_out->status[0] != NHIP_MS_OK) return NHIP_OK;  // a rule of the block: the archive stays as it was
        // ---- the tip check: the accumulator after the block against the archive's own, the counts and the window
        // against the mirror, the peaks against the device's; and msa_before against the plan's counts
        const uint32_t np1[2] = {(uint32_t)__builtin_popcountll(m.aocl_leafs), (uint32_t)__builtin_popcountll(m.chunks())};
        const uint32_t* tip_active = block_out->active + block_out->active_off[0];
        bool tip = !impossible && block_out->aocl_num_leafs[0] == m.aocl_leafs && block_out->swbf_num_leafs[0] == m.chunks() &&
                   block_out->aocl_n_peaks[0] == np1[0] && block_out->swbf_n_peaks[0] == np1[1] &&
                   block_out->n_active[0] == m.window.size() && std::equal(m.window.begin(), m.window.end(), tip_active);
        if (tip)
            tip = std::equal(block_out->aocl_peaks, block_out->aocl_peaks + 5 * (size_t)np1[0], peaks.begin()) &&
                  std::equal(block_out->swbf_peaks, block_out->swbf_peaks + 5 * (size_t)np1[1], peaks.begin() + 320);
        const uint32_t np0[2] = {(uint32_t)__builtin_popcountll(plan.n0), (uint32_t)__builtin_popcountll(plan.b0)};
        if (tip)
            tip = before.aocl.num_leafs == plan.n0 && before.swbf_inactive.num_leafs == plan.b0 && before.aocl.n_peaks == np0[0] &&
                  before.swbf_inactive.n_peaks == np0[1];
        if (!tip) {  // this block did not lead to this tip: as nhip_ms_apply_batch reports a 2.e failure
            block_out->verdict[0] = 0;
            block_out->status[0] = NHIP_MS_UPDATE_MISMATCH;
            block_out->bad_record[0] = UINT64_MAX;
            return NHIP_OK;
        }
        // ---- all allocation and growth before the first launch that writes archive state: host memory, then device
        nhip::MsArchiveMirror after = m;
        nhip::ms_archive_revert_commit(after, plan, window_before.data(), window_before.size());
        Compaction compaction;
        if (plan.compact) compaction.plan(after);
        Fresh fresh;
        uint32_t *d_arena, *d_window;
        bool arena_grown;
        if ((rc = fresh.want(a->arena, (size_t)plan.rel_tail_after, &d_arena, &arena_grown)) != NHIP_OK) return rc;
        if ((rc = fresh.want(a->window, window_before.size(), &d_window)) != NHIP_OK) return rc;
        Arr<uint32_t> spare;  // the second arena of a compaction, and its table (of the table's capacity: none shrinks)
        uint64_t* d_tab2 = nullptr;
        const size_t tab_cap = std::max<size_t>(a->tab.cap, 1);
        if (plan.compact) {
            hipError_t e = hipMalloc(reinterpret_cast<void**>(&spare.p), std::max<size_t>((size_t)plan.rel_live_after, 1) * 4);
            if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_tab2), tab_cap * 8);
            if (e != hipSuccess) {
                spare.release();
                return nhip::hip_fail(e);
            }
        }
        auto bail = [&](int code) {
            spare.release();
            if (d_tab2) (void)hipFree(d_tab2);
            return code;
        };
        if (arena_grown && a->arena.p && m.rel_tail) {
            st.step([&] {
                return nhip::hip_fail(hipMemcpyAsync(d_arena, a->arena.p, 4 * (size_t)m.rel_tail, hipMemcpyDeviceToDevice, c->stream));
            });
            if ((rc = st.finish()) != NHIP_OK) return bail(rc);  // the fresh buffers are dropped, the archive is as it was
        }
        // ---- from here on the archive is written: a HIP error poisons it
        const nhip::MsArchLevels lv[2] = {{a->nodes[0].p, m.aocl_cap, plan.n0}, {a->nodes[1].p, m.swbf_cap, plan.b0}};
        st.launch([&] { return nhip::launch_ms_arch_unmerge(d_rewritten, NR, d_block_rel, d_arena, a->tab.p, d_short_of, c->stream); });
        st.launch([&] { return nhip::launch_ms_arch_chunk_digests(a->tab.p, d_arena, 0, NR, d_rewritten, lv[1], c->stream); });
        const uint64_t* const ids2[2] = {nullptr, d_ids};
        const uint32_t* const off2[2] = {nullptr, d_off};
        const uint32_t levels[2] = {0, plan.lvl_off.empty() ? 0u : (uint32_t)plan.lvl_off.size() - 1};  // no AOCL node is hashed
        st.launch([&] { return nhip::launch_ms_arch_ancestors(lv, ids2, off2, levels, c->stream); });
        st.up(d_window, window_before.data(), window_before.size());
        // never a guess: the peaks at (n0, b0) against msa_before's and the short-of flag, on the drain that is due anyway
        if (have_nodes) {
            st.launch([&] { return nhip::launch_ms_arch_peaks(lv, d_peaks + 2 * 64 * 5, c->stream); });
            st.out(peaks_after.data(), d_peaks, peaks_after.size(), 2 * 64 * 5);
        }
        st.out(&short_of, d_short_of, 1);
        rc = st.finish();
        if (rc == NHIP_OK &&
            (short_of || !std::equal(before.aocl.peaks, before.aocl.peaks + 5 * (size_t)np0[0], peaks_after.begin()) ||
             !std::equal(before.swbf_inactive.peaks, before.swbf_inactive.peaks + 5 * (size_t)np0[1], peaks_after.begin() + 320)))
            rc = NHIP_ERR_HIP;  // the reference's closing sanity assert: nothing is reported as reverted
        if (rc == NHIP_OK && plan.compact) rc = compaction.run(st, c, a->tab.p, d_arena, spare.p, d_tab2);
        fresh.take();  // on an error: what the launches wrote into; nothing is read from it again
        if (rc != NHIP_OK) {
            a->poisoned = true;
            return bail(rc);
        }
        if (plan.compact) {
            if (compaction.moves()) {
                a->arena.release();
                a->arena.p = spare.p, a->arena.cap = std::max<size_t>((size_t)plan.rel_live_after, 1);
                spare.p = nullptr;
                a->tab.release();
                a->tab.p = d_tab2, a->tab.cap = tab_cap;
                d_tab2 = nullptr;
            }
            nhip::ms_archive_compact_commit(after);
        }
        bail(NHIP_OK);
        m = std::move(after);
        return NHIP_OK;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

int nhip_ms_archive_restore(nhip_ms_archive* a, const uint64_t* minimum, const uint32_t* distances,
                            const uint64_t* aocl_leaf_index, size_t n, nhip_ms_updated* out) {
    if (!a || !out) return NHIP_ERR_ARG;
    nhip_ctx* c = a->c;
    try {
        Stage st(c);
        if (a->poisoned) return NHIP_ERR_HIP;
        nhip::MsUpdatePlan plan;
        std::vector<uint8_t> status;
        int rc = nhip::ms_archive_restore_plan(a->m.aocl_leafs, a->m.chunk_len.data(), a->m.chunks(), minimum, distances,
                                               aocl_leaf_index, n, &plan, &status);
        if (rc != NHIP_OK) return rc;
        if ((rc = nhip::ms_updated_check(plan, true, out)) != NHIP_OK) return rc;
        const size_t E = plan.chunk_index.size();
        const size_t A = (size_t)plan.aocl_path_off[n], PD = (size_t)plan.path_off[E], RW = (size_t)plan.rel_off[E];
        if (!nhip::ms_updated_is_count_pass(out) && A + PD + RW) {
            GatherPlan gp;
            gp.units[0] = nhip::ms_arch_units(plan.aocl_path_off.data(), n, 5, false);
            gp.units[1] = nhip::ms_arch_units(plan.path_off.data(), E, 5, false);
            gp.units[2] = nhip::ms_arch_units(plan.rel_off.data(), E, 1, true);
            nhip::MsArchPathPool& pa = gp.g.path[0];
            nhip::MsArchPathPool& ps = gp.g.path[1];
            nhip::MsArchRelPool& pr = gp.g.rel;
            pa.mmr = a->levels(0), pa.owners = n, pa.units = gp.units[0].units;
            ps.mmr = a->levels(1), ps.owners = E, ps.units = gp.units[1].units;
            pr.tab = a->tab.p, pr.arena = a->arena.p, pr.owners = E, pr.units = gp.units[2].units;
            st.in(pa.leaf, aocl_leaf_index, n);
            st.in(pa.dst_off, plan.aocl_path_off.data(), n + 1);
            st.in(pa.first, gp.units[0].first.data(), gp.units[0].first.size());
            st.in(ps.leaf, plan.chunk_index.data(), E);
            st.in(ps.dst_off, plan.path_off.data(), E + 1);
            st.in(ps.first, gp.units[1].first.data(), gp.units[1].first.size());
            st.in(pr.dst_off, plan.rel_off.data(), E + 1);
            st.in(pr.first, gp.units[2].first.data(), gp.units[2].first.size());
            st.tmp(pa.dst, A, 5);
            st.tmp(ps.dst, PD, 5);
            st.tmp(pr.dst, RW);
            if (st.commit()) return st.finish();
            pr.key = ps.leaf;
            st.launch([&] { return nhip::launch_ms_arch_gather(gp.g, c->stream); });
            st.out(out->aocl_path, pa.dst, 5 * A);
            st.out(out->path, ps.dst, 5 * PD);
            st.out(out->rel, pr.dst, RW);
            if ((rc = st.finish()) != NHIP_OK) return rc;
        }
        nhip::ms_updated_write(plan, true, out);
        if (out->status) std::copy(status.begin(), status.end(), out->status);
        return NHIP_OK;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

// nhip_ms_archive_restore_plan on the device (ms_restore_kernels.hip): the inputs go up, the shape kernels run into
// stage scratch, the totals, the statuses and the per-witness offsets come back with one drain, the limits are decided
// from the totals, and a second, smaller read fetches the per-entry arrays, whose length is only known then.
int nhip_ms_archive_restore_shape(nhip_ms_archive* a, const uint64_t* minimum, const uint32_t* distances,
                                  const uint64_t* aocl_leaf_index, size_t n, nhip_ms_updated* out) {
    if (!a || !out) return NHIP_ERR_ARG;
    if (n && (!minimum || !distances || !aocl_leaf_index)) return NHIP_ERR_ARG;
    if (n > 0xFFFFFFFFull) return NHIP_ERR_OOM;
    nhip_ctx* c = a->c;
    try {
        Stage st(c);
        if (a->poisoned) return NHIP_ERR_HIP;
        nhip::MsUpdatePlan plan;  // the shape as ms_updated_check and ms_updated_write read it
        plan.wit_job.assign(n, 0);
        plan.aocl_path_off.assign(n + 1, 0);
        plan.entry_off.assign(n + 1, 0);
        plan.path_off.assign(1, 0);
        plan.rel_off.assign(1, 0);
        std::vector<uint8_t> status(n);
        nhip::RestoreShapePart shape(nhip::ms_archive_view(a), n);
        if (n) {
            shape.declare(st, minimum, distances, aocl_leaf_index);
            if (st.commit()) return st.finish();
            shape.enqueue(st, c, status.data());
            st.out(plan.aocl_path_off.data(), shape.d.aocl_path_off, n + 1);
            st.out(plan.entry_off.data(), shape.d.entry_off, n + 1);
            int rc = st.finish();
            if (rc == NHIP_OK) rc = shape.limits();
            if (rc != NHIP_OK) return rc;
            const size_t E = (size_t)shape.totals[1];
            plan.chunk_index.resize(E);
            plan.path_off.resize(E + 1);
            plan.rel_off.resize(E + 1);
            st.out(plan.chunk_index.data(), shape.d.chunk_index, E);
            st.out(plan.path_off.data(), shape.d.path_off, E + 1);
            st.out(plan.rel_off.data(), shape.d.rel_off, E + 1);
            if ((rc = st.finish()) != NHIP_OK) return rc;
        }
        if (const int rc = nhip::ms_updated_check(plan, false, out)) return rc;
        nhip::ms_updated_write(plan, true, out);
        if (out->status) std::copy(status.begin(), status.end(), out->status);
        return NHIP_OK;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

}  // extern "C"

nhip::MsArchView nhip::ms_archive_view(const nhip_ms_archive* a) {
    return MsArchView{a->poisoned, a->levels(0), a->levels(1), a->tab.p, a->arena.p};
}

nhip_ctx* nhip::ms_archive_ctx(const nhip_ms_archive* a) { return a->c; }
