// Stand-alone check of the hand-over's host side (tests/test_ms_restore_store_host.py):
//  1. the shared integer header (csrc/ms_restore_shape.hpp: the u128 add as two halves, the b + 255 bound, the path
//     lengths, the keys), which the shape kernels run per lane, against ms_archive_restore_plan, the oracle, over edge
//     index sets and random ones;
//  2. ms_store_append_restored_commit against ms_store_append_plan + ms_store_append_commit on the same integers,
//     from an empty and from a non-empty mirror.
// Links ms_archive.cpp, ms_store.cpp, ms_update_plan.cpp and ms_shape.cpp (no HIP); built once plainly and once under
// ASan + UBSan.  Prints "checks N failures M".
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

#include "../../neptune-core_amd/csrc/ms_restore_shape.hpp"
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

struct Sets {
    std::vector<uint64_t> mn, li;
    std::vector<uint32_t> dist;
    size_t n() const { return li.size(); }
    void add(uint64_t lo, uint64_t hi, const std::vector<uint32_t>& d, uint64_t leaf) {
        mn.push_back(lo), mn.push_back(hi);
        dist.insert(dist.end(), d.begin(), d.end());
        li.push_back(leaf);
    }
};

static std::vector<uint32_t> steps(uint32_t first, uint32_t step) {
    std::vector<uint32_t> d(45);
    for (uint32_t t = 0; t < 45; ++t) d[t] = first + t * step;
    return d;
}

// the edges an archive of n_leafs leaves (batch index b) has to decide, bad witnesses between good ones
static void edge_sets(uint64_t n_leafs, Sets* s) {
    const uint64_t b = MsJobScratch::batch_index(n_leafs), C = 4096;
    const uint64_t last = n_leafs ? n_leafs - 1 : 0;
    s->add(0, 0, steps(0, 1), 0);                                   // one chunk: key 0
    if (b) s->add((b - 1) * C, 0, steps(0, 3), last);               // key b - 1 alone
    s->add(0, 0, steps(0, 4096), MS_UPDATE_NONE);                   // 45 distinct chunks from 0 on
    s->add(b * C, 0, steps(0, 4096), 0);                            // all at or above b
    if (b >= 2) s->add((b - 2) * C + 5, 0, steps(0, 1000), 1);      // straddles b
    {
        std::vector<uint32_t> d(45);                                // a, c, a, c, ... and descending
        for (uint32_t t = 0; t < 45; ++t) d[t] = t % 2 ? 3 * 4096 + t : t;
        s->add(0, 0, d, last);
        for (uint32_t t = 0; t < 45; ++t) d[t] = (44 - t) * 4096;
        s->add(0, 0, d, MS_UPDATE_NONE);
    }
    s->add((b + 255) * C, 0, steps(0, 90), 0);                      // chunk b + 255 exactly: in range, no entry
    s->add((b + 256) * C, 0, steps(0, 1), 0);                       // b + 256: out of range
    s->add((b + 255) * C, 0, steps(4095 - 44, 1), last);            // the last index of chunk b + 255
    s->add((b + 255) * C, 0, steps(4096 - 44, 1), last);            // ... and one past it
    s->add(0, 1, steps(0, 1), 0);                                   // a high word
    s->add(~0ull, 0, steps(1, 0), 0);                               // the carry into the high word
    s->add(~0ull - 4, ~0ull, steps(9, 0), 0);                       // the wrap of u128
    s->add(~0ull - 4, ~0ull, steps(0, 0), 0);                       // 2^128 - 5 itself: no wrap, far out of range
    s->add(5, 0, steps(0, 7), n_leafs);                             // leaf indices at, past, and none
    s->add(5, 0, steps(0, 7), ~0ull - 1);
    s->add(5, 0, steps(0, 7), MS_UPDATE_NONE);
    s->add(~0ull - 4, ~0ull, steps(9, 0), n_leafs);                 // past the AOCL and saturating: NOT_IN_AOCL
    s->add(0, 0, steps(0, 1), last);
}

static void random_sets(uint64_t n_leafs, std::mt19937_64& g, size_t count, Sets* s) {
    const uint64_t b = MsJobScratch::batch_index(n_leafs), C = 4096;
    for (size_t k = 0; k < count; ++k) {
        std::vector<uint32_t> d(45);
        const uint32_t spread = g() % 3 == 0 ? 1u << 20 : g() % 2 ? 1u << 14 : 40;
        for (uint32_t& x : d) x = (uint32_t)(g() % spread);
        uint64_t lo = g() % ((b + 260) * C), hi = 0;
        if (g() % 16 == 0) lo = g(), hi = g() % 4 ? 0 : g();
        if (g() % 32 == 0) lo = ~0ull - g() % 100, hi = g() % 2 ? ~0ull : 0;
        const uint64_t leaf = g() % 5 == 0 ? MS_UPDATE_NONE : g() % 7 == 0 ? n_leafs + g() % 3 : g() % (n_leafs ? n_leafs : 1);
        s->add(lo, hi, d, leaf);
    }
}

// the header, witness by witness, into the plan's form
static void header_plan(uint64_t n_leafs, const std::vector<uint64_t>& len, const Sets& s, MsUpdatePlan* p, std::vector<uint8_t>* st) {
    const uint64_t b = MsJobScratch::batch_index(n_leafs);
    *p = MsUpdatePlan{};
    p->aocl_path_off.assign(1, 0), p->entry_off.assign(1, 0), p->path_off.assign(1, 0), p->rel_off.assign(1, 0);
    st->clear();
    for (size_t w = 0; w < s.n(); ++w) {
        uint64_t keys[MS_RESTORE_TRIALS];
        uint32_t alen, nk;
        st->push_back(ms_restore_witness(n_leafs, s.mn[2 * w], s.mn[2 * w + 1], &s.dist[45 * w], s.li[w], &alen, keys, &nk));
        p->aocl_path_off.push_back(p->aocl_path_off.back() + alen);
        for (uint32_t k = 0; k < nk; ++k) {
            p->chunk_index.push_back(keys[k]);
            p->path_off.push_back(p->path_off.back() + ms_arch_path_len(keys[k], b));
            p->rel_off.push_back(p->rel_off.back() + len[(size_t)keys[k]]);
        }
        p->entry_off.push_back(p->chunk_index.size());
    }
}

static void check_header(uint64_t n_leafs, std::mt19937_64& g, size_t randoms) {
    const uint64_t b = MsJobScratch::batch_index(n_leafs);
    std::vector<uint64_t> len((size_t)b);
    for (uint64_t& l : len) l = g() % 4 ? g() % 30 : 0;
    Sets s;
    edge_sets(n_leafs, &s);
    random_sets(n_leafs, g, randoms, &s);
    MsUpdatePlan want, got;
    std::vector<uint8_t> st_want, st_got;
    CHECK(ms_archive_restore_plan(n_leafs, len.data(), b, s.mn.data(), s.dist.data(), s.li.data(), s.n(), &want, &st_want) == NHIP_OK);
    header_plan(n_leafs, len, s, &got, &st_got);
    CHECK(st_got == st_want);
    CHECK(got.aocl_path_off == want.aocl_path_off);
    CHECK(got.entry_off == want.entry_off);
    CHECK(got.chunk_index == want.chunk_index);
    CHECK(got.path_off == want.path_off);
    CHECK(got.rel_off == want.rel_off);
    for (size_t w = 0; w < s.n(); ++w) {  // one at a time too, so that a failure names its witness
        ++checks;
        if (st_got[w] != st_want[w] || got.entry_off[w + 1] - got.entry_off[w] != want.entry_off[w + 1] - want.entry_off[w]) {
            ++failures;
            std::printf("n_leafs %llu witness %zu: status %u / %u\n", (unsigned long long)n_leafs, w, st_got[w], st_want[w]);
        }
    }
    if (n_leafs >= 600) {  // the edge list reaches what it is there for
        size_t ok = 0, out = 0, not_in = 0, full = 0;
        for (size_t w = 0; w < 20; ++w) {
            ok += st_want[w] == NHIP_MS_OK, out += st_want[w] == NHIP_MS_OUT_OF_RANGE, not_in += st_want[w] == NHIP_MS_NOT_IN_AOCL;
            full += want.entry_off[w + 1] - want.entry_off[w] == 45;
        }
        CHECK(ok >= 10 && out >= 4 && not_in >= 3 && full >= 2);
    }
}

// ---- the mirror commit
static void check_commit(std::mt19937_64& g, size_t rounds) {
    MsStoreMirror a, bm;  // fed through nhip_ms_update_in, and through the plan's integers
    for (size_t r = 0; r < rounds; ++r) {
        const size_t n = 1 + g() % 6;
        std::vector<uint64_t> mn(2 * n), li(n), leaf(5 * n, 7), aoff(1, 0), eoff(1, 0), key, poff(1, 0), roff(1, 0);
        std::vector<uint32_t> dist(45 * n);
        for (uint64_t& x : mn) x = g();
        for (uint32_t& x : dist) x = (uint32_t)(g() & 0xfffff);
        for (size_t i = 0; i < n; ++i) {
            li[i] = g() % 4 ? g() % 1000 : MS_UPDATE_NONE;
            aoff.push_back(aoff.back() + (li[i] == MS_UPDATE_NONE ? 0 : g() % 12));
            const size_t ne = g() % 5;
            for (size_t e = 0; e < ne; ++e) {
                key.push_back(g() % 100000);
                poff.push_back(poff.back() + g() % 9);
                roff.push_back(roff.back() + (g() % 3 ? g() % 20 : 0));
            }
            eoff.push_back(key.size());
        }
        std::vector<uint64_t> apath(5 * aoff.back() + 1, 1), path(5 * poff.back() + 1, 2);
        std::vector<uint32_t> rel(roff.back() + 1, 3);
        key.reserve(1);
        const nhip_ms_chunks ch{eoff.data(), key.data(), poff.data(), path.data(), roff.data(), rel.data()};
        const nhip_ms_update_in in{nullptr, mn.data(), dist.data(), li.data(), leaf.data(), aoff.data(), apath.data(), &ch};
        MsStoreAppend plan;
        CHECK(ms_store_append_plan(a, &in, n, &plan) == NHIP_OK);
        ms_store_append_commit(a, &in, n, plan);
        const uint64_t add[4] = {aoff.back(), key.size(), poff.back(), roff.back()};
        CHECK(ms_store_restored_ok(bm, n, add) == NHIP_OK);
        MsStoreRestored rs;
        rs.n = n, rs.minimum = mn.data(), rs.leaf_index = li.data(), rs.distances = dist.data();
        rs.aocl_path_off = aoff.data(), rs.entry_off = eoff.data(), rs.chunk_index = key.data();
        rs.path_off = poff.data(), rs.rel_off = roff.data();
        ms_store_append_restored_commit(bm, rs);
        CHECK(a == bm);
        CHECK(bm.witnesses() == a.witnesses() && bm.counts().chunks.rel_words == a.counts().chunks.rel_words);
    }
    // the limits, as ms_store_append_plan has them
    const uint64_t big[4] = {MS_STORE_LIMIT, 0, 0, 0}, over[4] = {0, 0, 0, MS_STORE_LIMIT + 1}, many[4] = {0, 0xFFFFFFFFull, 0, 0};
    CHECK(ms_store_restored_ok(bm, 1, big) == (bm.counts().aocl_digests ? NHIP_ERR_OOM : NHIP_OK));
    CHECK(ms_store_restored_ok(bm, 1, over) == NHIP_ERR_OOM);
    CHECK(ms_store_restored_ok(bm, 1, many) == NHIP_ERR_OOM);
    CHECK(ms_store_restored_ok(bm, (size_t)UINT32_MAX, over) == NHIP_ERR_ARG);
    MsStoreMirror before = bm;
    ms_store_append_restored_commit(bm, MsStoreRestored{});  // n == 0
    CHECK(before == bm);
}

int main() {
    std::mt19937_64 g(20260101);
    for (uint64_t n_leafs : {0ull, 1ull, 8ull, 9ull, 600ull, 1027ull, 3000ull, 65536ull}) check_header(n_leafs, g, 700);
    check_commit(g, 400);
    std::printf("checks %ld failures %ld\n", checks, failures);
    return failures ? 1 : 0;
}
