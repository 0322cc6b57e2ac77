// C-ABI layer of the device-resident witness store (nhip_ms_store_*; declarations: include/neptune_hip.h; DESIGN.md
// §6i).  The store owns its device buffers (hipMalloc, not the context's workspace, which every other call recycles):
//   pools : AOCL path digests, keys (the device's: zero for a sticky witness), dictionary path digests, chunk words
//   shape : the four offset arrays and the sticky status bytes
//   fixed : minimum, distances, aocl_leaf_index, aocl_leaf
// each in two sets, current and next.  An update writes the next pools and shape and swaps them once the stream has
// drained clean and the block ended NHIP_MS_OK, and so does a revert (§6j), the same step in the other direction; a
// retain gathers all three into the next sets and swaps all three.
// The fixed set is double too because a gather cannot compact in place.  The host side is ms_store.cpp (the mirror
// and every shape decision); the block and witness parts are ms_parts.hpp's, shared with nhip_ms_update_batch and
// nhip_ms_revert_batch.
#include "ms_parts.hpp"
#include "ms_restore_device.hpp"
#include "ms_store.hpp"

namespace {

using nhip::MsStoreMirror;
using nhip::MsStoreSelect;

// One device array that grows geometrically and keeps its first `keep` elements; never null once ensured.
template <class T>
struct Buf {
    T* p = nullptr;
    size_t cap = 0, floor = 0;  // elements; floor: the initial capacity asked for
    int ensure(size_t need, size_t keep, hipStream_t stream) {
        if (p && need <= cap) return NHIP_OK;
        size_t want = nhip::ms_store_grown(cap, need, SIZE_MAX / 64);
        if (need && !want) return NHIP_ERR_OOM;
        want = std::max<size_t>({want, floor, 1});
        if (want > SIZE_MAX / 64) return NHIP_ERR_OOM;
        T* q = nullptr;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&q), want * sizeof(T));
        if (e != hipSuccess) return nhip::hip_fail(e);
        if (p && keep) {
            e = hipMemcpyAsync(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
            if (e != hipSuccess) {
                (void)hipFree(q);
                return nhip::hip_fail(e);
            }
        }
        if (p) (void)hipFree(p);
        p = q;
        cap = want;
        return NHIP_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

struct Pools {
    Buf<uint64_t> aocl, key, path;  // 5 words per digest; per entry; 5 words per digest
    Buf<uint32_t> rel;
    // totals in digests / entries / digests / words
    int ensure(const uint64_t t[4], const uint64_t keep[4], hipStream_t st) {
        int rc = aocl.ensure(5 * (size_t)t[0], 5 * (size_t)keep[0], st);
        if (!rc) rc = key.ensure((size_t)t[1], (size_t)keep[1], st);
        if (!rc) rc = path.ensure(5 * (size_t)t[2], 5 * (size_t)keep[2], st);
        if (!rc) rc = rel.ensure((size_t)t[3], (size_t)keep[3], st);
        return rc;
    }
};
struct Shape {
    Buf<uint64_t> aocl_path_off, entry_off, path_off, rel_off;
    Buf<uint8_t> sticky;
    int ensure(size_t W, size_t E, size_t keep_w, size_t keep_e, bool keep, hipStream_t st) {
        int rc = aocl_path_off.ensure(W + 1, keep ? keep_w + 1 : 0, st);
        if (!rc) rc = entry_off.ensure(W + 1, keep ? keep_w + 1 : 0, st);
        if (!rc) rc = path_off.ensure(E + 1, keep ? keep_e + 1 : 0, st);
        if (!rc) rc = rel_off.ensure(E + 1, keep ? keep_e + 1 : 0, st);
        if (!rc) rc = sticky.ensure(W, keep ? keep_w : 0, st);
        return rc;
    }
};
struct Fixed {
    Buf<uint64_t> minimum, leaf_index, leaf;
    Buf<uint32_t> distances;
    int ensure(size_t W, size_t keep_w, hipStream_t st) {
        int rc = minimum.ensure(2 * W, 2 * keep_w, st);
        if (!rc) rc = leaf_index.ensure(W, keep_w, st);
        if (!rc) rc = leaf.ensure(5 * W, 5 * keep_w, st);
        if (!rc) rc = distances.ensure(45 * W, 45 * keep_w, st);
        return rc;
    }
};

}  // namespace

struct nhip_ms_store {
    nhip_ctx* c = nullptr;
    MsStoreMirror m;
    Pools pools[2];
    Shape shape[2];
    Fixed fixed[2];
    int pc = 0, sc = 0, fc = 0;  // the current set of each

    nhip::MsChunksDev chunks() const {
        const Pools& p = pools[pc];
        const Shape& s = shape[sc];
        return nhip::MsChunksDev{s.entry_off.p, p.key.p, s.path_off.p, p.path.p, s.rel_off.p, p.rel.p};
    }
};

namespace {

void totals_of(const nhip::MsUpdateCounts& c, uint64_t t[4]) {
    t[0] = c.aocl_digests;
    t[1] = c.chunks.entries;
    t[2] = c.chunks.path_digests;
    t[3] = c.chunks.rel_words;
}

// the selection's nine arrays on the stage, and the source side of the gather
void declare_select(Stage& st, const nhip_ms_store& s, const MsStoreSelect& sel, nhip::MsStoreGatherDev& g) {
    const size_t n = sel.n();
    g.n = n;
    for (int p = 0; p < 4; ++p) {
        st.in(g.src[p], sel.src[p].data(), n);
        st.in(g.dst[p], sel.dst[p].data(), n + 1);
    }
    st.in(g.unit_first, sel.unit_first.data(), sel.unit_first.size());
    const Pools& cur = s.pools[s.pc];
    g.s_aocl = cur.aocl.p;
    g.s_key = cur.key.p;
    g.s_path = cur.path.p;
    g.s_rel = cur.rel.p;
}

// One job across the store, the witness side bound to it: forward (§6g) or, with `back`, from the accumulator after
// the block to msa_before (§6j).  The plan from the mirror, the witness kernels from the current set into the next,
// k_ms_store_seal, the swap.
int store_cross(nhip_ms_store* s, const nhip_ms_apply_in* block, nhip_ms_apply_out* block_out, uint8_t* status, bool back) {
    nhip::MsApplyCounts cnt;
    if (!s || !block || block->n_jobs != 1 || nhip::ms_apply_ok(block, block_out, &cnt)) return NHIP_ERR_ARG;
    nhip_ctx* c = s->c;
    try {
        Stage st(c);
        const size_t W = s->m.witnesses();
        if (W == 0) {  // the block part alone
            BlockPart blk(*block, *block_out, cnt, false);
            return run_parts(st, c, blk);
        }
        uint64_t wit_off[2];
        nhip_ms_chunks mirror_chunks;
        nhip_ms_update_in win;
        nhip::ms_store_as_update_in(s->m, wit_off, &mirror_chunks, &win);
        const nhip::MsUpdateCounts wc = s->m.counts();
        nhip::MsUpdatePlan plan;
        int rc = back ? nhip::ms_revert_plan(block, &win, wc, &plan) : nhip::ms_update_plan(block, &win, wc, &plan);
        if (rc != NHIP_OK) return rc;
        const size_t OE = plan.chunk_index.size();
        const uint64_t need[4] = {plan.aocl_path_off[W], OE, plan.path_off[OE], plan.rel_off[OE]}, none[4] = {0, 0, 0, 0};
        Pools& cur = s->pools[s->pc];
        Pools& nxt = s->pools[1 - s->pc];
        Shape& hcur = s->shape[s->sc];
        Shape& hnxt = s->shape[1 - s->sc];
        const Fixed& F = s->fixed[s->fc];
        if ((rc = nxt.ensure(need, none, c->stream)) != NHIP_OK) return rc;
        if ((rc = hnxt.ensure(W, OE, 0, 0, false, c->stream)) != NHIP_OK) return rc;
        WitnessResident res{};
        res.in.minimum = F.minimum.p;
        res.in.distances = F.distances.p;
        res.in.aocl_leaf_index = F.leaf_index.p;
        res.in.aocl_leaf = F.leaf.p;
        res.in.aocl_path_off = hcur.aocl_path_off.p;
        res.in.aocl_path = cur.aocl.p;
        res.in.ch = s->chunks();
        res.out.o_aocl_path = nxt.aocl.p;
        res.out.o_chunk_index = nxt.key.p;
        res.out.o_path = nxt.path.p;
        res.out.o_rel = nxt.rel.p;
        res.o_aocl_path_off = hnxt.aocl_path_off.p;
        res.o_entry_off = hnxt.entry_off.p;
        res.o_path_off = hnxt.path_off.p;
        res.o_rel_off = hnxt.rel_off.p;
        res.sticky = hcur.sticky.p;
        res.sticky_next = hnxt.sticky.p;
        nhip_ms_updated unused{};
        BlockPart blk(*block, *block_out, cnt, !back);  // forward: k_ms_apply keeps its nodes
        auto cross = [&](auto& part) -> int {
            if (const int e = run_parts(st, c, blk, &part)) return e;
            if (block_out->status[0] != NHIP_MS_OK) {  // the store stays as it was
                if (status) std::fill(status, status + W, (uint8_t)NHIP_MS_JOB_REJECTED);
                return NHIP_OK;
            }
            if (status) std::copy(part.wstatus.begin(), part.wstatus.end(), status);
            s->pc = 1 - s->pc;
            s->sc = 1 - s->sc;
            nhip::ms_store_apply_plan(s->m, std::move(plan), part.wstatus.data());
            return NHIP_OK;
        };
        if (back) {
            RevertPart rp(win, wc, plan, unused, blk, &res);
            return cross(rp);
        }
        WitnessPart wp(win, wc, plan, unused, &res);
        return cross(wp);
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

}  // namespace

extern "C" {

int nhip_ms_store_create(nhip_ctx* c, const nhip_ms_store_caps* initial, nhip_ms_store** out) {
    if (!c || !out) return NHIP_ERR_ARG;
    if (initial && (initial->witnesses > SIZE_MAX / 4096 || initial->aocl_digests > SIZE_MAX / 4096 ||
                    initial->entries > SIZE_MAX / 4096 || initial->path_digests > SIZE_MAX / 4096 ||
                    initial->rel_words > SIZE_MAX / 4096))
        return NHIP_ERR_ARG;
    nhip_ms_store* s = new (std::nothrow) nhip_ms_store;
    if (!s) return NHIP_ERR_OOM;
    s->c = c;
    if (initial) {
        for (int k = 0; k < 2; ++k) {
            Pools& p = s->pools[k];
            p.aocl.floor = 5 * initial->aocl_digests;
            p.key.floor = initial->entries;
            p.path.floor = 5 * initial->path_digests;
            p.rel.floor = initial->rel_words;
            Shape& h = s->shape[k];
            h.aocl_path_off.floor = h.entry_off.floor = initial->witnesses + 1;
            h.path_off.floor = h.rel_off.floor = initial->entries + 1;
            h.sticky.floor = initial->witnesses;
            Fixed& f = s->fixed[k];
            f.minimum.floor = 2 * initial->witnesses;
            f.leaf_index.floor = initial->witnesses;
            f.leaf.floor = 5 * initial->witnesses;
            f.distances.floor = 45 * initial->witnesses;
        }
    }
    *out = s;
    return NHIP_OK;
}

void nhip_ms_store_destroy(nhip_ms_store* s) {
    if (!s) return;
    {
        Stage st(s->c);  // the context's lock and device
        (void)hipStreamSynchronize(s->c->stream);
        for (int k = 0; k < 2; ++k) {
            Pools& p = s->pools[k];
            p.aocl.release(), p.key.release(), p.path.release(), p.rel.release();
            Shape& h = s->shape[k];
            h.aocl_path_off.release(), h.entry_off.release(), h.path_off.release(), h.rel_off.release(), h.sticky.release();
            Fixed& f = s->fixed[k];
            f.minimum.release(), f.leaf_index.release(), f.leaf.release(), f.distances.release();
        }
    }
    delete s;
}

int nhip_ms_store_count(const nhip_ms_store* s, uint64_t* witnesses, uint64_t* aocl_digests, uint64_t* entries,
                        uint64_t* path_digests, uint64_t* rel_words) {
    if (!s) return NHIP_ERR_ARG;
    const std::lock_guard<std::mutex> lock(s->c->mu);
    const nhip::MsUpdateCounts c = s->m.counts();
    if (witnesses) *witnesses = c.witnesses;
    if (aocl_digests) *aocl_digests = c.aocl_digests;
    if (entries) *entries = c.chunks.entries;
    if (path_digests) *path_digests = c.chunks.path_digests;
    if (rel_words) *rel_words = c.chunks.rel_words;
    return NHIP_OK;
}

int nhip_ms_store_append(nhip_ms_store* s, const nhip_ms_update_in* wit, size_t n) {
    if (!s) return NHIP_ERR_ARG;
    nhip_ctx* c = s->c;
    try {
        Stage st(c);
        nhip::MsStoreAppend a;
        if (const int rc = nhip::ms_store_append_plan(s->m, wit, n, &a)) return rc;
        if (n == 0) return NHIP_OK;
        uint64_t have[4], add[4], need[4];
        const nhip::MsUpdateCounts hc = s->m.counts();
        totals_of(hc, have);
        totals_of(a.add, add);
        for (int p = 0; p < 4; ++p) need[p] = have[p] + add[p];
        const size_t W0 = (size_t)hc.witnesses, E0 = (size_t)have[1], ne = (size_t)add[1];
        Pools& P = s->pools[s->pc];
        Shape& H = s->shape[s->sc];
        Fixed& F = s->fixed[s->fc];
        int rc = P.ensure(need, have, c->stream);
        if (!rc) rc = H.ensure(W0 + n, E0 + ne, W0, E0, true, c->stream);
        if (!rc) rc = F.ensure(W0 + n, W0, c->stream);
        if (rc) return rc;
        // the only time a witness's paths and chunk words cross to the device
        st.up(P.aocl.p + 5 * (size_t)have[0], wit->aocl_path, 5 * (size_t)add[0]);
        if (ne) {
            st.up(P.key.p + E0, wit->chunks->chunk_index, ne);
            st.up(P.path.p + 5 * (size_t)have[2], wit->chunks->path, 5 * (size_t)add[2]);
            st.up(P.rel.p + (size_t)have[3], wit->chunks->rel, (size_t)add[3]);
        }
        static const uint64_t zero = 0;
        if (W0 == 0) {
            st.up(H.aocl_path_off.p, &zero, 1);
            st.up(H.entry_off.p, &zero, 1);
        }
        if (E0 == 0) {
            st.up(H.path_off.p, &zero, 1);
            st.up(H.rel_off.p, &zero, 1);
        }
        st.up(H.aocl_path_off.p + W0 + 1, a.aocl_path_off.data(), n);
        st.up(H.entry_off.p + W0 + 1, a.entry_off.data(), n);
        st.up(H.path_off.p + E0 + 1, a.path_off.data(), ne);
        st.up(H.rel_off.p + E0 + 1, a.rel_off.data(), ne);
        st.step([&] { return nhip::hip_fail(hipMemsetAsync(H.sticky.p + W0, NHIP_MS_OK, n, c->stream)); });
        st.up(F.minimum.p + 2 * W0, wit->minimum, 2 * n);
        st.up(F.distances.p + 45 * W0, wit->distances, 45 * n);
        st.up(F.leaf_index.p + W0, wit->aocl_leaf_index, n);
        st.up(F.leaf.p + 5 * W0, wit->aocl_leaf, 5 * n);
        if ((rc = st.finish()) != NHIP_OK) return rc;
        nhip::ms_store_append_commit(s->m, wit, n, a);
        return NHIP_OK;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

// nhip_ms_archive_restore and nhip_ms_store_append in one, device to device ("The hand-over"): the
// shape kernels into stage scratch, one drain for the totals and the statuses, all or nothing and the limits, every
// growth, then the gather out of the archive straight behind the store's totals, the offsets rebased into the shape
// arrays, the fixed arrays, and the integers the mirror needs back to the host.
int nhip_ms_store_append_restored(nhip_ms_store* s, nhip_ms_archive* archive, const uint64_t* minimum, const uint32_t* distances,
                                  const uint64_t* aocl_leaf_index, const uint64_t* aocl_leaf, size_t n, uint8_t* status) {
    if (!s || !archive || nhip::ms_archive_ctx(archive) != s->c) return NHIP_ERR_ARG;
    nhip_ctx* c = s->c;
    if (n && (!minimum || !distances || !aocl_leaf_index)) return NHIP_ERR_ARG;
    if (n >= (size_t)UINT32_MAX) return NHIP_ERR_ARG;  // as nhip_ms_store_append
    try {
        Stage st(c);  // one context: its lock covers the archive too
        const nhip::MsArchView av = nhip::ms_archive_view(archive);
        if (av.poisoned) return NHIP_ERR_HIP;
        if (n == 0) return NHIP_OK;
        std::vector<uint8_t> wstatus(n);
        nhip::RestoreShapePart shape(av, n);
        shape.declare(st, minimum, distances, aocl_leaf_index);
        if (st.commit()) return st.finish();
        shape.enqueue(st, c, wstatus.data());
        int rc = st.finish();
        if (rc != NHIP_OK) return rc;
        if (status) std::copy(wstatus.begin(), wstatus.end(), status);
        if (std::any_of(wstatus.begin(), wstatus.end(), [](uint8_t x) { return x != NHIP_MS_OK; })) return NHIP_OK;
        if ((rc = shape.limits()) != NHIP_OK) return rc;
        const uint64_t* add = shape.totals;
        if ((rc = nhip::ms_store_restored_ok(s->m, n, add)) != NHIP_OK) return rc;
        uint64_t have[4], need[4];
        const nhip::MsUpdateCounts hc = s->m.counts();
        totals_of(hc, have);
        for (int p = 0; p < 4; ++p) need[p] = have[p] + add[p];
        const size_t W0 = (size_t)hc.witnesses, E0 = (size_t)have[1], ne = (size_t)add[1];
        // host memory first: what the mirror's commit reads
        std::vector<uint64_t> aocl_path_off(n + 1), entry_off(n + 1), key(ne), path_off(ne + 1), rel_off(ne + 1);
        Pools& P = s->pools[s->pc];
        Shape& H = s->shape[s->sc];
        Fixed& F = s->fixed[s->fc];
        rc = P.ensure(need, have, c->stream);
        if (!rc) rc = H.ensure(W0 + n, E0 + ne, W0, E0, true, c->stream);
        if (!rc) rc = F.ensure(W0 + n, W0, c->stream);
        if (rc) return rc;
        // ---- from here on only bytes behind the mirror's totals are written
        const uint64_t skew = have[3] & 1;  // the chunk words' pool may begin on an odd word: the gather stores aligned pairs
        nhip::MsArchGatherDev g{};
        nhip::MsArchPathPool& pa = g.path[0];
        nhip::MsArchPathPool& ps = g.path[1];
        nhip::MsArchRelPool& pr = g.rel;
        const uint64_t unit = nhip::MS_ARCHIVE_GATHER_UNIT;
        pa.mmr = av.aocl, pa.leaf = shape.d.leaf_index, pa.dst_off = shape.d.aocl_path_off, pa.owners = n;
        pa.units = (5 * add[0] + unit - 1) / unit, pa.dst = P.aocl.p + 5 * (size_t)have[0];
        ps.mmr = av.swbf, ps.leaf = shape.d.chunk_index, ps.dst_off = shape.d.path_off, ps.owners = ne;
        ps.units = (5 * add[2] + unit - 1) / unit, ps.dst = P.path.p + 5 * (size_t)have[2];
        pr.tab = av.tab, pr.arena = av.arena, pr.key = shape.d.chunk_index, pr.dst_off = shape.d.rel_off, pr.owners = ne;
        pr.units = add[3] ? (add[3] + skew + 2 * unit - 1) / (2 * unit) : 0;
        pr.dst = P.rel.p + (size_t)(have[3] - skew), pr.skew = skew;
        st.launch([&] { return nhip::launch_ms_arch_gather_own(g, c->stream); });
        nhip::MsRestoreHandDev hd{};
        hd.s = shape.d;
        hd.entries = ne;
        for (int p = 0; p < 4; ++p) hd.base[p] = have[p];
        hd.w0 = W0;
        hd.aocl_path_off = H.aocl_path_off.p, hd.entry_off = H.entry_off.p, hd.path_off = H.path_off.p, hd.rel_off = H.rel_off.p;
        hd.key = P.key.p;
        hd.aocl_nodes = av.aocl.nodes;
        hd.leaf = aocl_leaf ? nullptr : F.leaf.p;
        static const uint64_t zero = 0;
        if (E0 == 0 && ne == 0) {  // no entry lane writes the first offsets
            st.up(H.path_off.p, &zero, 1);
            st.up(H.rel_off.p, &zero, 1);
        }
        st.launch([&] { return nhip::launch_ms_restore_hand(hd, c->stream); });
        st.step([&] { return nhip::hip_fail(hipMemsetAsync(H.sticky.p + W0, NHIP_MS_OK, n, c->stream)); });
        auto d2d = [&](void* dst, const void* src, size_t bytes) {
            st.step([&] { return nhip::hip_fail(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream)); });
        };
        d2d(F.minimum.p + 2 * W0, shape.d.minimum, 16 * n);
        d2d(F.distances.p + 45 * W0, shape.d.distances, 4 * 45 * n);
        d2d(F.leaf_index.p + W0, shape.d.leaf_index, 8 * n);
        if (aocl_leaf) st.up(F.leaf.p + 5 * W0, aocl_leaf, 5 * n);
        // the integers the mirror needs: the offsets (from 0, the commit rebases them) and the keys
        st.out(aocl_path_off.data(), shape.d.aocl_path_off, n + 1);
        st.out(entry_off.data(), shape.d.entry_off, n + 1);
        st.out(key.data(), shape.d.chunk_index, ne);
        st.out(path_off.data(), shape.d.path_off, ne + 1);
        st.out(rel_off.data(), shape.d.rel_off, ne + 1);
        if ((rc = st.finish()) != NHIP_OK) return rc;
        nhip::MsStoreRestored r;
        r.n = n;
        r.minimum = minimum, r.leaf_index = aocl_leaf_index, r.distances = distances;
        r.aocl_path_off = aocl_path_off.data(), r.entry_off = entry_off.data(), r.chunk_index = key.data();
        r.path_off = path_off.data(), r.rel_off = rel_off.data();
        nhip::ms_store_append_restored_commit(s->m, r);
        return NHIP_OK;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

int nhip_ms_store_update(nhip_ms_store* s, const nhip_ms_apply_in* block, nhip_ms_apply_out* block_out, uint8_t* status) {
    return store_cross(s, block, block_out, status, false);
}

int nhip_ms_store_revert(nhip_ms_store* s, const nhip_ms_apply_in* block, nhip_ms_apply_out* block_out, uint8_t* status) {
    return store_cross(s, block, block_out, status, true);
}

int nhip_ms_store_read(nhip_ms_store* s, const uint64_t* sel_in, size_t n_sel, nhip_ms_updated* out) {
    if (!s || !out) return NHIP_ERR_ARG;
    nhip_ctx* c = s->c;
    try {
        Stage st(c);
        MsStoreSelect sel;
        int rc = nhip::ms_store_select(s->m, sel_in, n_sel, &sel);
        if (rc != NHIP_OK) return rc;
        // the selection's shape as a plan's, for the checks and the writes nhip_ms_update_batch uses
        nhip::MsUpdatePlan shape;
        shape.wit_job.resize(n_sel);
        shape.aocl_path_off = sel.dst[0];
        shape.entry_off = sel.dst[1];
        shape.chunk_index.resize((size_t)sel.total(1));
        shape.path_off = sel.path_off;
        shape.rel_off = sel.rel_off;
        if ((rc = nhip::ms_updated_check(shape, true, out)) != NHIP_OK) return rc;
        if (nhip::ms_updated_is_count_pass(out) || n_sel == 0) {  // from the mirror alone
            nhip::ms_updated_write(shape, false, out);
            return NHIP_OK;
        }
        const uint64_t t[4] = {sel.total(0), sel.total(1), sel.total(2), sel.total(3)};
        nhip::MsStoreGatherDev g{};
        declare_select(st, *s, sel, g);
        st.tmp(g.d_aocl, (size_t)t[0], 5);
        st.tmp(g.d_key, (size_t)t[1]);
        st.tmp(g.d_path, (size_t)t[2], 5);
        st.tmp(g.d_rel, (size_t)t[3]);
        if (st.commit()) return st.finish();
        const nhip::MsStoreGatherUnits units = nhip::ms_store_gather_units(sel.unit_end, n_sel, false);
        st.launch([&] { return nhip::launch_ms_store_gather(g, units, c->stream); });
        st.out(out->aocl_path, g.d_aocl, 5 * (size_t)t[0]);
        st.out(out->chunk_index, g.d_key, (size_t)t[1]);
        st.out(out->path, g.d_path, 5 * (size_t)t[2]);
        st.out(out->rel, g.d_rel, (size_t)t[3]);
        if ((rc = st.finish()) != NHIP_OK) return rc;
        nhip::ms_updated_write(shape, false, out);
        for (size_t i = 0; i < n_sel; ++i) out->status[i] = s->m.sticky[(size_t)sel.sel[i]];
        return NHIP_OK;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

int nhip_ms_store_retain(nhip_ms_store* s, const uint8_t* keep) {
    if (!s) return NHIP_ERR_ARG;
    nhip_ctx* c = s->c;
    try {
        Stage st(c);
        const size_t W = s->m.witnesses();
        if (W == 0) return NHIP_OK;
        if (!keep) return NHIP_ERR_ARG;
        const std::vector<uint64_t> kept = nhip::ms_store_kept(keep, W);
        const size_t n = kept.size();
        if (n == W) return NHIP_OK;
        MsStoreSelect sel;
        int rc = nhip::ms_store_select(s->m, kept.data(), n, &sel);
        if (rc != NHIP_OK) return rc;
        MsStoreMirror after = nhip::ms_store_selected_mirror(s->m, sel);
        const uint64_t t[4] = {sel.total(0), sel.total(1), sel.total(2), sel.total(3)}, none[4] = {0, 0, 0, 0};
        Pools& P = s->pools[1 - s->pc];
        Shape& H = s->shape[1 - s->sc];
        Fixed& F = s->fixed[1 - s->fc];
        if ((rc = P.ensure(t, none, c->stream)) != NHIP_OK) return rc;
        if ((rc = H.ensure(n, (size_t)t[1], 0, 0, false, c->stream)) != NHIP_OK) return rc;
        if ((rc = F.ensure(n, 0, c->stream)) != NHIP_OK) return rc;
        nhip::MsStoreGatherDev g{};
        declare_select(st, *s, sel, g);
        st.in(g.sel, sel.sel.data(), n);
        if (st.commit()) return st.finish();
        const Fixed& Fc = s->fixed[s->fc];
        g.d_aocl = P.aocl.p, g.d_key = P.key.p, g.d_path = P.path.p, g.d_rel = P.rel.p;
        g.s_minimum = Fc.minimum.p, g.s_leaf_index = Fc.leaf_index.p, g.s_leaf = Fc.leaf.p, g.s_distances = Fc.distances.p;
        g.s_sticky = s->shape[s->sc].sticky.p;
        g.d_minimum = F.minimum.p, g.d_leaf_index = F.leaf_index.p, g.d_leaf = F.leaf.p, g.d_distances = F.distances.p;
        g.d_sticky = H.sticky.p;
        st.up(H.aocl_path_off.p, after.aocl_path_off.data(), n + 1);
        st.up(H.entry_off.p, after.entry_off.data(), n + 1);
        st.up(H.path_off.p, after.path_off.data(), (size_t)t[1] + 1);
        st.up(H.rel_off.p, after.rel_off.data(), (size_t)t[1] + 1);
        const nhip::MsStoreGatherUnits units = nhip::ms_store_gather_units(sel.unit_end, n, true);
        st.launch([&] { return nhip::launch_ms_store_gather(g, units, c->stream); });
        if ((rc = st.finish()) != NHIP_OK) return rc;
        s->pc = 1 - s->pc;
        s->sc = 1 - s->sc;
        s->fc = 1 - s->fc;
        s->m = std::move(after);
        return NHIP_OK;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

// launch_mmr_verify over the AOCL parts, launch_ms_chunk_auth and launch_ms_records over the index sets and the
// dictionaries, all where the store keeps them; the accumulator staged as nhip_ms_can_remove_batch stages it.
int nhip_ms_store_check(nhip_ms_store* s, const nhip_msa* msa, uint8_t* aocl_member, uint8_t* valid, uint8_t* can_remove,
                        uint8_t* status) {
    if (!s || nhip::ms_msa_ok(msa)) return NHIP_ERR_ARG;
    nhip_ctx* c = s->c;
    try {
        Stage st(c);
        const size_t W = s->m.witnesses(), E = s->m.entries();
        if (W == 0) return NHIP_OK;
        if (!aocl_member || !valid || !can_remove || !status) return NHIP_ERR_ARG;
        std::vector<uint32_t> active;
        nhip::ms_append_sorted_window(active, *msa);
        const Fixed& F = s->fixed[s->fc];
        const Shape& H = s->shape[s->sc];
        nhip::MmrDev aocl{nullptr, msa->aocl.n_peaks, msa->aocl.num_leafs};
        nhip::MmrDev swbf{nullptr, msa->swbf_inactive.n_peaks, msa->swbf_inactive.num_leafs};
        nhip::MsRecordsDev r{};  // aocl_member null: validate / can_remove
        uint8_t *d_auth, *d_member;
        st.in(aocl.peaks, msa->aocl.peaks, msa->aocl.n_peaks, 5);
        st.in(swbf.peaks, msa->swbf_inactive.peaks, msa->swbf_inactive.n_peaks, 5);
        st.in(r.active, active.data(), active.size());
        st.tmp(d_auth, E);
        st.tmp(d_member, W);
        st.tmp(r.valid, W, 3);  // valid, verdict, status
        if (st.commit()) return st.finish();
        r.minimum = F.minimum.p;
        r.distances = F.distances.p;
        r.ch = s->chunks();
        r.auth = d_auth;
        r.n_active = active.size();
        r.aocl_num_leafs = msa->aocl.num_leafs;
        r.verdict = r.valid + W;
        r.status = r.valid + 2 * W;
        st.launch([&] {
            return nhip::launch_mmr_verify(aocl, F.leaf_index.p, F.leaf.p, H.aocl_path_off.p, s->pools[s->pc].aocl.p, W, d_member,
                                           c->stream);
        });
        st.launch([&] { return nhip::launch_ms_chunk_auth(swbf, r.ch, E, d_auth, c->stream); });
        st.launch([&] { return nhip::launch_ms_records(r, W, c->stream); });
        st.launch([&] {
            return nhip::launch_ms_store_check_seal(F.leaf_index.p, H.sticky.p, W, d_member, r.valid, r.verdict, r.status, c->stream);
        });
        st.out(aocl_member, d_member, W);
        st.out(valid, r.valid, W);
        st.out(can_remove, r.verdict, W);
        st.out(status, r.status, W);
        return st.finish();
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

}  // extern "C"
