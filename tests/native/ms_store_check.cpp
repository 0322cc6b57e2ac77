// Stand-alone check of the witness store's host side (csrc/ms_store.cpp; tests/test_ms_store_host.py): the mirror
// arithmetic of append, select / retain and "the plan becomes the shape" against brute-force restatements over random
// small stores.  Links ms_store.cpp, ms_update_plan.cpp and ms_shape.cpp (no HIP); built once plainly and once under
// ASan + UBSan.  Prints "checks N failures M".
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

#include "../../neptune-core_amd/csrc/ms_store.hpp"

using namespace nhip;

static long checks = 0, failures = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        ++checks;                                                    \
        if (!(x)) {                                                  \
            ++failures;                                              \
            std::printf("line %d: %s\n", __LINE__, #x);              \
        }                                                            \
    } while (0)

// a witness as plain lists: the brute-force side keeps these, never offsets
struct Wit {
    uint64_t mn[2];
    uint32_t dist[45];
    uint64_t leaf_index;
    uint64_t aocl_len;
    std::vector<uint64_t> key, path_len, rel_len;
};

static Wit random_wit(std::mt19937_64& g) {
    Wit w{};
    w.mn[0] = g();
    w.mn[1] = g() & 0xffff;
    if (g() % 2) {  // an index set around chunk 125, where the plans below give it keys
        w.mn[0] = g() % (130 * 4096);
        w.mn[1] = 0;
    }
    for (uint32_t& d : w.dist) d = (uint32_t)(g() & 0xfffff);
    w.leaf_index = g() % 4 ? g() % 1000 : MS_UPDATE_NONE;
    w.aocl_len = w.leaf_index == MS_UPDATE_NONE ? 0 : g() % 12;
    const size_t ne = g() % 5;
    for (size_t e = 0; e < ne; ++e) {
        w.key.push_back(g() % 100000);
        w.path_len.push_back(g() % 9);
        w.rel_len.push_back(g() % 3 ? g() % 20 : 0);
    }
    return w;
}

// the flat arrays of nhip_ms_update_in for a list of witnesses
struct Flat {
    std::vector<uint64_t> minimum, leaf_index, leaf, aocl_path_off{0}, aocl_path, entry_off{0}, key, path_off{0}, path, rel_off{0};
    std::vector<uint32_t> distances, rel;
    nhip_ms_chunks ch{};
    nhip_ms_update_in in{};
    explicit Flat(const std::vector<Wit>& ws) {
        for (const Wit& w : ws) {
            minimum.insert(minimum.end(), w.mn, w.mn + 2);
            distances.insert(distances.end(), w.dist, w.dist + 45);
            leaf_index.push_back(w.leaf_index);
            leaf.insert(leaf.end(), 5, 7);
            aocl_path_off.push_back(aocl_path_off.back() + w.aocl_len);
            for (size_t e = 0; e < w.key.size(); ++e) {
                key.push_back(w.key[e]);
                path_off.push_back(path_off.back() + w.path_len[e]);
                rel_off.push_back(rel_off.back() + w.rel_len[e]);
            }
            entry_off.push_back(key.size());
        }
        aocl_path.assign(5 * aocl_path_off.back() + 1, 1);
        path.assign(5 * path_off.back() + 1, 2);
        rel.assign(rel_off.back() + 1, 3);
        // distinct non-null addresses even for empty arrays, as a caller's would be
        minimum.reserve(1), distances.reserve(1), leaf_index.reserve(1), leaf.reserve(1), key.reserve(1);
        ch = nhip_ms_chunks{entry_off.data(), key.data(), path_off.data(), path.data(), rel_off.data(), rel.data()};
        in = nhip_ms_update_in{nullptr, minimum.data(), distances.data(), leaf_index.data(), leaf.data(),
                               aocl_path_off.data(), aocl_path.data(), &ch};
    }
};

// the mirror a list of witnesses must give, from scratch
static MsStoreMirror brute(const std::vector<Wit>& ws, const std::vector<uint8_t>& sticky) {
    MsStoreMirror m;
    for (size_t i = 0; i < ws.size(); ++i) {
        const Wit& w = ws[i];
        m.minimum.insert(m.minimum.end(), w.mn, w.mn + 2);
        m.distances.insert(m.distances.end(), w.dist, w.dist + 45);
        m.leaf_index.push_back(w.leaf_index);
        m.aocl_path_off.push_back(m.aocl_path_off.back() + w.aocl_len);
        for (size_t e = 0; e < w.key.size(); ++e) {
            m.key.push_back(w.key[e]);
            m.path_off.push_back(m.path_off.back() + w.path_len[e]);
            m.rel_off.push_back(m.rel_off.back() + w.rel_len[e]);
        }
        m.entry_off.push_back(m.key.size());
        m.sticky.push_back(sticky[i]);
    }
    return m;
}

static int append(MsStoreMirror& m, const std::vector<Wit>& ws) {
    Flat f(ws);
    MsStoreAppend a;
    const int rc = ms_store_append_plan(m, &f.in, ws.size(), &a);
    if (rc == NHIP_OK) ms_store_append_commit(m, &f.in, ws.size(), a);
    return rc;
}

static void random_stores(std::mt19937_64& g) {
    for (int round = 0; round < 200; ++round) {
        std::vector<Wit> all;
        MsStoreMirror m;
        const int batches = 1 + (int)(g() % 4);
        for (int b = 0; b < batches; ++b) {  // append, then the offsets
            std::vector<Wit> ws;
            for (size_t i = g() % 6; i > 0; --i) ws.push_back(random_wit(g));
            CHECK(append(m, ws) == NHIP_OK);
            all.insert(all.end(), ws.begin(), ws.end());
            CHECK(m == brute(all, std::vector<uint8_t>(all.size(), 0)));
        }
        const size_t W = all.size();
        const MsUpdateCounts c = m.counts();
        CHECK(c.witnesses == W && c.chunks.entries == m.key.size());
        std::vector<uint8_t> sticky(W);
        for (uint8_t& s : sticky) s = g() % 5 ? 0 : (uint8_t)(1 + g() % 5);
        m.sticky = sticky;

        // select: any order, repeats; every range where the lists say
        std::vector<uint64_t> sel;
        for (size_t i = W ? g() % (2 * W + 1) : 0; i > 0; --i) sel.push_back(g() % W);
        MsStoreSelect s;
        CHECK(ms_store_select(m, sel.data(), sel.size(), &s) == NHIP_OK);
        std::vector<Wit> chosen;
        std::vector<uint8_t> chosen_sticky;
        for (uint64_t w : sel) chosen.push_back(all[w]), chosen_sticky.push_back(sticky[w]);
        const MsStoreMirror want = brute(chosen, chosen_sticky);
        CHECK(ms_store_selected_mirror(m, s) == want);
        CHECK(s.dst[0] == want.aocl_path_off && s.dst[1] == want.entry_off && s.path_off == want.path_off && s.rel_off == want.rel_off);
        for (size_t i = 0; i < sel.size(); ++i) {
            const size_t w = sel[i], e0 = m.entry_off[w];
            CHECK(s.src[0][i] == m.aocl_path_off[w] && s.src[1][i] == e0 && s.src[2][i] == m.path_off[e0] && s.src[3][i] == m.rel_off[e0]);
            CHECK(s.dst[2][i] == want.path_off[want.entry_off[i]] && s.dst[3][i] == want.rel_off[want.entry_off[i]]);
        }
        {  // the gather's units: every unit's first element lies in the range of the witness it names
            const uint64_t per_unit[4] = {MS_STORE_GATHER_UNIT, MS_STORE_GATHER_UNIT, MS_STORE_GATHER_UNIT, 2 * MS_STORE_GATHER_UNIT};
            const uint64_t scale[4] = {5, 1, 5, 1};
            size_t at = 0;
            for (int p = 0; p < 4; ++p) {
                const uint64_t total = s.total(p) * scale[p], units = (total + per_unit[p] - 1) / per_unit[p];
                CHECK(s.unit_end[p] == (p ? s.unit_end[p - 1] : 0) + units && s.unit_first.size() >= at + units + 1);
                for (uint64_t u = 0; u < units; ++u) {
                    const size_t i = s.unit_first[at + u];
                    CHECK(i < sel.size() && s.dst[p][i] * scale[p] <= u * per_unit[p] && u * per_unit[p] < s.dst[p][i + 1] * scale[p]);
                }
                CHECK(s.unit_first[at + units] == (sel.empty() ? 0 : sel.size() - 1));
                at += units + 1;
            }
            CHECK(s.unit_first.size() == at);
        }
        if (W) {
            const MsStoreMirror before = m;
            sel.push_back(W);  // an index equal to W
            CHECK(ms_store_select(m, sel.data(), sel.size(), &s) == NHIP_ERR_ARG && m == before);
            CHECK(ms_store_select(m, nullptr, W + 1, &s) == NHIP_ERR_ARG);  // "all" is W
        }
        // "all", retain(all) the identity, retain(none) empty, retain(mask) in order
        CHECK(ms_store_select(m, nullptr, W, &s) == NHIP_OK && ms_store_selected_mirror(m, s) == m);
        std::vector<uint8_t> keep(W, 1);
        std::vector<uint64_t> kept = ms_store_kept(keep.data(), W);
        CHECK(kept.size() == W && ms_store_select(m, kept.data(), W, &s) == NHIP_OK && ms_store_selected_mirror(m, s) == m);
        std::fill(keep.begin(), keep.end(), 0);
        kept = ms_store_kept(keep.data(), W);
        CHECK(kept.empty() && ms_store_select(m, kept.data(), 0, &s) == NHIP_OK && ms_store_selected_mirror(m, s) == MsStoreMirror{});
        chosen.clear(), chosen_sticky.clear();
        for (size_t w = 0; w < W; ++w)
            if ((keep[w] = (uint8_t)(g() % 3 ? 7 : 0))) chosen.push_back(all[w]), chosen_sticky.push_back(sticky[w]);
        kept = ms_store_kept(keep.data(), W);
        CHECK(ms_store_select(m, kept.data(), kept.size(), &s) == NHIP_OK && ms_store_selected_mirror(m, s) == brute(chosen, chosen_sticky));

        // the mirror as the one job of ms_update_plan, and the plan as the mirror afterwards
        nhip_msa msa{};
        msa.aocl.num_leafs = 1000 + g() % 50;
        msa.swbf_inactive.num_leafs = (msa.aocl.num_leafs - 1) / 8;
        const uint64_t add_off[2] = {0, g() % 40}, rec_off[2] = {0, 0};
        nhip_ms_apply_in block{};
        block.n_jobs = 1;
        block.msa_before = &msa;
        block.add_off = add_off;
        block.rec_off = rec_off;
        uint64_t wit_off[2];
        nhip_ms_chunks ch;
        nhip_ms_update_in in;
        ms_store_as_update_in(m, wit_off, &ch, &in);
        CHECK(wit_off[0] == 0 && wit_off[1] == W && in.chunks == &ch && !in.aocl_path && !ch.path && !ch.rel);
        MsUpdatePlan plan;
        CHECK(ms_update_plan(&block, &in, m.counts(), &plan) == NHIP_OK);
        const MsUpdatePlan copy = plan;
        std::vector<uint8_t> status(W);
        for (uint8_t& x : status) x = (uint8_t)(g() % 3 ? 0 : 5);
        const MsStoreMirror old = m;
        ms_store_apply_plan(m, std::move(plan), status.data());
        CHECK(m.aocl_path_off == copy.aocl_path_off && m.entry_off == copy.entry_off && m.key == copy.chunk_index &&
              m.path_off == copy.path_off && m.rel_off == copy.rel_off && m.sticky == status);
        CHECK(m.minimum == old.minimum && m.distances == old.distances && m.leaf_index == old.leaf_index);
        CHECK(m.witnesses() == W && m.entry_off.size() == W + 1 && m.path_off.size() == m.key.size() + 1);
    }
}

static void shape_errors_and_overflow(std::mt19937_64& g) {
    std::vector<Wit> ws;
    for (int i = 0; i < 5; ++i) ws.push_back(random_wit(g));
    ws[2].key = {5, 9};
    ws[2].path_len = {3, 4};
    ws[2].rel_len = {6, 1};
    MsStoreMirror m;
    CHECK(append(m, ws) == NHIP_OK);
    const MsStoreMirror before = m;
    MsStoreAppend a;
    {  // shape errors, as ms_update_ok's
        Flat f(ws);
        CHECK(ms_store_append_plan(m, nullptr, 5, &a) == NHIP_ERR_ARG);
        nhip_ms_update_in in = f.in;
        in.minimum = nullptr;
        CHECK(ms_store_append_plan(m, &in, 5, &a) == NHIP_ERR_ARG);
        in = f.in;
        in.chunks = nullptr;
        CHECK(ms_store_append_plan(m, &in, 5, &a) == NHIP_ERR_ARG);
        f.aocl_path_off[0] = 1;
        CHECK(ms_store_append_plan(m, &f.in, 5, &a) == NHIP_ERR_ARG);
        f.aocl_path_off[0] = 0;
        std::swap(f.rel_off[1], f.rel_off[2]);
        const bool decreasing = f.rel_off[2] < f.rel_off[1];
        CHECK(!decreasing || ms_store_append_plan(m, &f.in, 5, &a) == NHIP_ERR_ARG);
        CHECK(ms_store_append_plan(m, &f.in, 0, &a) == NHIP_OK);  // nothing to append: nothing is read
        CHECK(m == before);
    }
    {  // totals that would leave size_t / 64: NHIP_ERR_OOM, the mirror as it was
        const std::vector<Wit> one(ws.begin() + 2, ws.begin() + 3);  // one witness, two entries
        {
            Flat f(one);
            f.rel_off[2] = MS_STORE_LIMIT - 2;  // with the words the mirror holds: past the limit
            CHECK(ms_store_append_plan(m, &f.in, 1, &a) == NHIP_ERR_OOM);
            CHECK(m == before);
        }
        // digests: one append of more than the limit is a shape error already (ms_csr_ok); two that pass it together
        for (int which = 0; which < 2; ++which) {
            Flat f(one);
            const uint64_t half = 200000000000000000ull;  // 2e17 < (SIZE_MAX / 2) / 40, and twice it > SIZE_MAX / 64
            (which ? f.path_off[2] : f.aocl_path_off[1]) = half;
            MsStoreMirror big = m;
            CHECK(ms_store_append_plan(big, &f.in, 1, &a) == NHIP_OK);
            ms_store_append_commit(big, &f.in, 1, a);
            const MsStoreMirror held = big;
            CHECK(ms_store_append_plan(big, &f.in, 1, &a) == NHIP_ERR_OOM && big == held);
            (which ? f.path_off[2] : f.aocl_path_off[1]) = MS_STORE_LIMIT;
            CHECK(ms_store_append_plan(m, &f.in, 1, &a) == NHIP_ERR_ARG && m == before);
        }
        Flat f(std::vector<Wit>(ws.begin() + 2, ws.begin() + 3));
        f.rel_off[2] = MS_STORE_LIMIT - m.rel_off.back();  // exactly the limit: accepted
        CHECK(ms_store_append_plan(m, &f.in, 1, &a) == NHIP_OK);
        MsStoreMirror huge = m;
        ms_store_append_commit(huge, &f.in, 1, a);
        CHECK(huge.rel_off.back() == MS_STORE_LIMIT && m == before);
        // a selection with repeats can pass what the store holds
        const std::vector<uint64_t> twice = {5, 5};
        MsStoreSelect s;
        CHECK(ms_store_select(huge, twice.data(), 2, &s) == NHIP_ERR_OOM);
    }
    // capacities
    CHECK(ms_store_grown(0, 0, 100) == 0 && ms_store_grown(8, 3, 100) == 8 && ms_store_grown(8, 9, 100) == 16);
    CHECK(ms_store_grown(8, 40, 100) == 40 && ms_store_grown(60, 61, 100) == 100 && ms_store_grown(60, 101, 100) == 0);
    CHECK(ms_store_grown(0, 5, 100) == 5 && ms_store_grown(SIZE_MAX / 2 + 1, SIZE_MAX / 2 + 2, SIZE_MAX) == SIZE_MAX);
}

int main() {
    std::mt19937_64 g(3000);
    random_stores(g);
    shape_errors_and_overflow(g);
    std::printf("checks %ld failures %ld\n", checks, failures);
    return failures ? 1 : 0;
}
