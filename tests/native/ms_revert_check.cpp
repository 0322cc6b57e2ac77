// Stand-alone check of the host plan of nhip_ms_revert_batch (csrc/ms_revert_plan.cpp) and of the
// store's mirror step behind it, plainly and under ASan + UBSan (tests/test_ms_revert_plan.py builds and runs it;
// ms_revert.mk).  A fixed batch and 200 seeded random batches, each planned through the C entry point with the
// two-call sizing into exactly sized heap arrays (so that a write past a total is a sanitizer report) and compared
// with a naive recomputation that shares no code with the plan: sets, maps and linear scans where the plan sorts and
// bisects.  Then the same witnesses as one job through the store's mirror: the plan from the mirror equals the plan
// from the arrays, and "the plan becomes the shape" leaves the mirror with the plan's offsets and keys, the given
// statuses and its fixed part untouched.  Nothing here touches a GPU.
#include <cstdio>
#include <cstdint>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "../../include/neptune_hip.h"
#include "../../neptune-core_amd/csrc/ms_revert_plan.hpp"
#include "../../neptune-core_amd/csrc/ms_store.hpp"

static long checks = 0, failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        ++checks;                                                         \
        if (!(c)) {                                                       \
            ++failures;                                                   \
            if (failures < 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                                 \
    } while (0)

using u128 = unsigned __int128;

struct Dict {
    std::vector<uint64_t> key;
    std::vector<uint64_t> path_len;
    std::vector<std::vector<uint32_t>> rel;
};
struct Witness {
    u128 minimum;
    uint32_t dist[45];
    uint64_t leaf;  // UINT64_MAX: a removal record
    uint64_t path_len;
    Dict dict;
};
struct Job {
    uint64_t n0;
    uint64_t k;
    std::vector<Witness> records;  // the block's removal records (leaf unused)
    std::vector<Witness> wits;     // as they stand after the block
};

static uint64_t ilog2(uint64_t x) {
    uint64_t r = 0;
    while (x >>= 1) ++r;
    return r;
}

// The arrays of one call; the vectors own what the C structs point into.
struct Flat {
    std::vector<nhip_msa> msa;
    std::vector<uint64_t> add_off, additions, rec_off, rmin, wit_off, wmin, leaf_index, leaf, apath_off, apath;
    std::vector<uint32_t> rdist, wdist;
    struct Chunks {
        std::vector<uint64_t> entry_off{0}, key, path_off{0}, path, rel_off{0};
        std::vector<uint32_t> rel;
        nhip_ms_chunks c;
        void add(const Dict& d) {
            for (size_t e = 0; e < d.key.size(); ++e) {
                key.push_back(d.key[e]);
                path_off.push_back(path_off.back() + d.path_len[e]);
                path.resize(5 * path_off.back(), 7);
                rel.insert(rel.end(), d.rel[e].begin(), d.rel[e].end());
                rel_off.push_back(rel.size());
            }
            entry_off.push_back(key.size());
        }
        void seal() { c = nhip_ms_chunks{entry_off.data(), key.data(), path_off.data(), path.data(), rel_off.data(), rel.data()}; }
    } rch, wch;
    nhip_ms_apply_in block;
    nhip_ms_update_in wit;
};

static void flatten(const std::vector<Job>& jobs, Flat* f) {
    f->add_off = {0};
    f->rec_off = {0};
    f->wit_off = {0};
    f->apath_off = {0};
    f->msa.resize(jobs.size());
    auto put = [](const Witness& w, std::vector<uint64_t>& mn, std::vector<uint32_t>& dist) {
        mn.push_back((uint64_t)w.minimum);
        mn.push_back((uint64_t)(w.minimum >> 64));
        dist.insert(dist.end(), w.dist, w.dist + 45);
    };
    for (size_t j = 0; j < jobs.size(); ++j) {
        const Job& jb = jobs[j];
        f->msa[j] = nhip_msa{{nullptr, 0, jb.n0}, {nullptr, 0, (jb.n0 ? jb.n0 - 1 : 0) / 8}, nullptr, 0};
        f->add_off.push_back(f->add_off.back() + jb.k);
        for (const Witness& r : jb.records) {
            put(r, f->rmin, f->rdist);
            f->rch.add(r.dict);
        }
        f->rec_off.push_back(f->rec_off.back() + jb.records.size());
        for (const Witness& w : jb.wits) {
            put(w, f->wmin, f->wdist);
            f->leaf_index.push_back(w.leaf);
            f->apath_off.push_back(f->apath_off.back() + w.path_len);
            f->wch.add(w.dict);
        }
        f->wit_off.push_back(f->wit_off.back() + jb.wits.size());
    }
    f->additions.assign(5 * f->add_off.back() + 5, 3);
    f->leaf.assign(5 * f->leaf_index.size() + 5, 4);
    f->apath.assign(5 * f->apath_off.back() + 5, 5);
    f->rch.seal();
    f->wch.seal();
    f->block = nhip_ms_apply_in{jobs.size(), f->msa.data(), f->add_off.data(), f->additions.data(), f->rec_off.data(),
                                f->rmin.data(), f->rdist.data(), &f->rch.c, nullptr};
    f->wit = nhip_ms_update_in{f->wit_off.data(), f->wmin.data(), f->wdist.data(), f->leaf_index.data(), f->leaf.data(),
                               f->apath_off.data(), f->apath.data(), &f->wch.c};
}

// naive: per witness (aocl path length, [(key, path length, chunk length)]) before the block
struct Shape {
    uint64_t aocl;
    std::vector<uint64_t> key, path, rel;
};
static std::vector<Shape> naive(const std::vector<Job>& jobs) {
    std::vector<Shape> out;
    for (const Job& jb : jobs) {
        const bool wraps = jb.n0 + jb.k < jb.n0;
        const uint64_t b0 = wraps ? 0 : (jb.n0 ? jb.n0 - 1 : 0) / 8;
        std::map<uint64_t, uint64_t> hits;  // chunk -> the block's indices in it
        for (const Witness& r : jb.records)
            for (int t = 0; t < 45; ++t) {
                const u128 v = r.minimum + r.dist[t];
                if (v < r.minimum || (v >> 12) >= (u128)b0) continue;
                ++hits[(uint64_t)(v >> 12)];
            }
        for (const Witness& w : jb.wits) {
            Shape s;
            s.aocl = (w.leaf == UINT64_MAX || wraps || w.leaf >= jb.n0) ? 0 : ilog2(w.leaf ^ jb.n0);
            std::set<uint64_t> keys;
            for (int t = 0; t < 45; ++t) {
                const u128 v = w.minimum + w.dist[t];
                if (v >= w.minimum && (v >> 12) < (u128)b0) keys.insert((uint64_t)(v >> 12));
            }
            for (const uint64_t key : keys) {
                uint64_t now = 0;
                for (size_t e = 0; e < w.dict.key.size(); ++e)
                    if (w.dict.key[e] == key) {
                        now = w.dict.rel[e].size();
                        break;
                    }
                const uint64_t gone = hits.count(key) ? hits[key] : 0;
                s.key.push_back(key);
                s.path.push_back(ilog2(key ^ b0));
                s.rel.push_back(now > gone ? now - gone : 0);
            }
            out.push_back(s);
        }
    }
    return out;
}

// the same witnesses through the store's mirror, one job
static void mirror_step(const Job& jb) {
    Flat f;
    flatten({jb}, &f);
    const size_t W = jb.wits.size();
    nhip::MsStoreMirror m;
    nhip::MsStoreAppend a;
    CHECK(nhip::ms_store_append_plan(m, &f.wit, W, &a) == NHIP_OK);
    nhip::ms_store_append_commit(m, &f.wit, W, a);
    const nhip::MsStoreMirror before = m;
    uint64_t wit_off[2];
    nhip_ms_chunks mc;
    nhip_ms_update_in win;
    nhip::ms_store_as_update_in(m, wit_off, &mc, &win);
    nhip::MsUpdateCounts direct_counts;
    CHECK(nhip::ms_update_ok(&f.block, &f.wit, &direct_counts) == NHIP_OK);
    nhip::MsUpdatePlan direct, plan;
    CHECK(nhip::ms_revert_plan(&f.block, &f.wit, direct_counts, &direct) == NHIP_OK);
    CHECK(nhip::ms_revert_plan(&f.block, &win, m.counts(), &plan) == NHIP_OK);
    CHECK(plan.aocl_path_off == direct.aocl_path_off && plan.entry_off == direct.entry_off &&
          plan.chunk_index == direct.chunk_index && plan.path_off == direct.path_off && plan.rel_off == direct.rel_off &&
          plan.ent_wit == direct.ent_wit && plan.ent_src == direct.ent_src && plan.wit_job == direct.wit_job);
    CHECK(plan.in_ent_wit.empty());
    const nhip::MsUpdatePlan kept = plan;
    std::vector<uint8_t> status(W);
    for (size_t w = 0; w < W; ++w) status[w] = (uint8_t)(w % 3 == 1 ? NHIP_MS_NOT_IN_AOCL : NHIP_MS_OK);
    nhip::ms_store_apply_plan(m, std::move(plan), status.data());
    CHECK(m.witnesses() == W && m.entries() == kept.chunk_index.size());
    CHECK(m.aocl_path_off == kept.aocl_path_off && m.entry_off == kept.entry_off && m.key == kept.chunk_index &&
          m.path_off == kept.path_off && m.rel_off == kept.rel_off && m.sticky == status);
    CHECK(m.minimum == before.minimum && m.distances == before.distances && m.leaf_index == before.leaf_index);
    const nhip::MsUpdateCounts c = m.counts();
    CHECK(c.witnesses == W && c.aocl_digests == kept.aocl_path_off[W] && c.chunks.entries == kept.chunk_index.size() &&
          c.chunks.path_digests == kept.path_off.back() && c.chunks.rel_words == kept.rel_off.back());
    // the mirror after is a set of witnesses again: it plans a block forward
    nhip::ms_store_as_update_in(m, wit_off, &mc, &win);
    nhip::MsUpdatePlan fwd;
    CHECK(nhip::ms_update_plan(&f.block, &win, m.counts(), &fwd) == NHIP_OK);
    CHECK(fwd.wit_job.size() == W);
    // the scratch of the old levels: one level per height of b0 for every group
    std::vector<nhip::MsApplyJob> jobs(2);
    jobs[0].aocl_n = jb.n0, jobs[0].n_grp = 7;
    jobs[1].aocl_n = jb.n0, jobs[1].n_grp = 0;
    const std::vector<uint64_t> off = nhip::ms_revert_node_offsets(jobs);
    const uint64_t b0 = (jb.n0 ? jb.n0 - 1 : 0) / 8;
    CHECK(off.size() == 3 && off[0] == 0 && off[1] == 7 * (b0 ? ilog2(b0) + 1 : 0) && off[2] == off[1]);
}

static void run(const std::vector<Job>& jobs) {
    Flat f;
    flatten(jobs, &f);
    const std::vector<Shape> want = naive(jobs);
    nhip_ms_updated count{};
    CHECK(nhip_ms_revert_plan(&f.block, &f.wit, &count) == NHIP_OK);
    uint64_t A = 0, E = 0, PD = 0, RW = 0;
    for (const Shape& s : want) {
        A += s.aocl;
        E += s.key.size();
        for (const uint64_t x : s.path) PD += x;
        for (const uint64_t x : s.rel) RW += x;
    }
    CHECK(count.aocl_digests == A && count.entries == E && count.path_digests == PD && count.rel_words == RW);
    const size_t W = want.size();
    // exactly sized: one element past a total is a heap overflow
    std::vector<uint64_t> aoff(W + 1, 99), eoff(W + 1, 99), key(count.entries, 99), poff(count.entries + 1, 99),
        roff(count.entries + 1, 99);
    nhip_ms_updated fill{};
    fill.aocl_path_off = aoff.data();
    fill.entry_off = eoff.data();
    fill.chunk_index = key.data();
    fill.path_off = poff.data();
    fill.rel_off = roff.data();
    fill.aocl_cap = count.aocl_digests;
    fill.entries_cap = count.entries;
    fill.path_cap = count.path_digests;
    fill.rel_cap = count.rel_words;
    const int rc = nhip_ms_revert_plan(&f.block, &f.wit, &fill);
    CHECK(rc == NHIP_OK);
    if (rc != NHIP_OK) return;
    CHECK(aoff[0] == 0 && eoff[0] == 0 && poff[0] == 0 && roff[0] == 0);
    for (size_t w = 0; w < W; ++w) {
        const Shape& s = want[w];
        CHECK(aoff[w + 1] - aoff[w] == s.aocl);
        CHECK(eoff[w + 1] - eoff[w] == s.key.size());
        if (eoff[w + 1] - eoff[w] != s.key.size()) return;
        for (size_t q = 0; q < s.key.size(); ++q) {
            const size_t e = (size_t)eoff[w] + q;
            CHECK(key[e] == s.key[q]);
            CHECK(poff[e + 1] - poff[e] == s.path[q]);
            CHECK(roff[e + 1] - roff[e] == s.rel[q]);
        }
    }
    if (count.entries) {  // a capacity one short is refused and nothing is written
        std::vector<uint64_t> k2(count.entries, 99);
        nhip_ms_updated shortfall = fill;
        shortfall.chunk_index = k2.data();
        shortfall.entries_cap = count.entries - 1;
        CHECK(nhip_ms_revert_plan(&f.block, &f.wit, &shortfall) == NHIP_ERR_ARG);
        CHECK(k2[0] == 99);
    }
    // argument errors leave the outputs untouched
    nhip_ms_updated untouched = fill;
    std::vector<uint64_t> a2(W + 1, 99);
    untouched.aocl_path_off = a2.data();
    CHECK(nhip_ms_revert_plan(nullptr, &f.wit, &untouched) == NHIP_ERR_ARG);
    CHECK(nhip_ms_revert_plan(&f.block, nullptr, &untouched) == NHIP_ERR_ARG);
    CHECK(nhip_ms_revert_plan(&f.block, &f.wit, nullptr) == NHIP_ERR_ARG);
    CHECK(a2[0] == 99 && a2[W] == 99);
    for (const Job& jb : jobs) mirror_step(jb);
}

static Witness random_witness(std::mt19937_64& g, uint64_t n0, uint64_t k, bool record) {
    const uint64_t n1 = n0 + k, b1 = (n1 ? n1 - 1 : 0) / 8;
    Witness w{};
    uint64_t span = n1 + (g() % 8 == 0 ? 3 : 0);  // now and then a leaf index past the block
    if (span < n1 || span == 0) span = n1 ? n1 : 1;
    const uint64_t l = g() % span;
    w.leaf = record ? UINT64_MAX : l;
    w.path_len = g() % 12;
    const unsigned mode = (unsigned)(g() % 16);
    const uint64_t batch = l / 8;
    w.minimum = (u128)batch * 4096 + g() % 4096;
    if (mode == 0) w.minimum = ~(u128)0 - g() % 1000;                // saturates
    if (mode == 1) w.minimum = ((u128)(g() % 1000) << 76) | g();      // a chunk index past u64
    if (mode == 2 && b1 > 3) w.minimum = (u128)(g() % b1) * 4096;     // far below
    for (int t = 0; t < 45; ++t) w.dist[t] = (uint32_t)(g() % (1u << 20));
    if (mode == 3) w.dist[7] = UINT32_MAX;
    if (mode == 4) w.dist[3] = w.dist[4];  // the same index twice
    // a dictionary: some of its chunk indices below b1, now and then a stray or a repeated key
    std::set<uint64_t> cis;
    for (int t = 0; t < 45; ++t) {
        const u128 v = w.minimum + w.dist[t];
        if (v >= w.minimum && (v >> 12) < (u128)b1) cis.insert((uint64_t)(v >> 12));
    }
    for (const uint64_t ci : cis) {
        if (g() % 10 == 0) continue;
        std::vector<uint32_t> rel(g() % 9);
        for (uint32_t& x : rel) x = (uint32_t)(g() % 4096);
        const int copies = g() % 12 == 0 ? 2 : 1;
        for (int rep = 0; rep < copies; ++rep) {
            w.dict.key.push_back(ci);
            w.dict.path_len.push_back(g() % 7);
            w.dict.rel.push_back(rep ? std::vector<uint32_t>(3, 1) : rel);
        }
    }
    if (g() % 8 == 0) {
        w.dict.key.push_back(g());
        w.dict.path_len.push_back(2);
        w.dict.rel.push_back({1, 2, 3});
    }
    return w;
}

static Job random_job(std::mt19937_64& g) {
    Job jb;
    const unsigned pick = (unsigned)(g() % 10);
    jb.n0 = pick == 0 ? 0 : pick == 1 ? g() % 10 : pick == 2 ? (1ull << 40) + g() % 100 : pick == 3 ? UINT64_MAX - g() % 4 : g() % 5000;
    jb.k = pick == 3 ? g() % 8 : g() % 10 == 0 ? 0 : g() % 400;
    const size_t m = g() % 4, n = g() % 7;
    for (size_t r = 0; r < m; ++r) jb.records.push_back(random_witness(g, jb.n0, 0, true));
    for (size_t w = 0; w < n; ++w) {
        // now and then a witness with a record's own index set: its chunks are the touched ones
        if (m && g() % 3 == 0) {
            Witness x = jb.records[g() % m];
            x.leaf = g() % 2 ? UINT64_MAX : (jb.n0 ? g() % jb.n0 : 0);
            for (std::vector<uint32_t>& rel : x.dict.rel) rel.resize(rel.size() + g() % 4, 5);
            jb.wits.push_back(x);
        } else {
            jb.wits.push_back(random_witness(g, jb.n0, jb.k, g() % 3 == 0));
        }
    }
    return jb;
}

int main() {
    std::mt19937_64 g(3100);
    {  // a fixed batch: 600 leaves before, 20 additions; one record and four witnesses with chosen indices
        Job jb;
        jb.n0 = 600;
        jb.k = 20;  // b0 = 74, b1 = 77
        Witness rec{};
        rec.minimum = (u128)70 * 4096;
        for (int t = 0; t < 45; ++t) rec.dist[t] = (uint32_t)(t * 700);  // chunks 70 .. 77: six indices a chunk at most
        rec.leaf = UINT64_MAX;
        rec.dict.key = {70, 71, 72, 73};
        rec.dict.path_len = {3, 3, 1, 1};
        rec.dict.rel = {{1, 2}, {}, {9}, {4000}};
        jb.records.push_back(rec);
        Witness a = rec;  // the same index set as a membership proof of leaf 599, after the block
        a.leaf = 599;
        a.path_len = 5;  // ilog2(599 ^ 620)
        a.dict.key = {70, 71, 72, 73, 74, 75, 76};
        a.dict.path_len = {3, 3, 2, 2, 1, 1, 0};
        a.dict.rel = {std::vector<uint32_t>(9, 1), std::vector<uint32_t>(6, 2), {9, 10, 11}, std::vector<uint32_t>(20, 3), {1}, {}, {2}};
        jb.wits.push_back(a);  // chunk 72 holds fewer words than the block put there: floored at 0
        Witness born = rec;
        born.minimum = (u128)75 * 4096 + 17;
        born.leaf = 619;  // born in the block: no AOCL path, no entry below b0
        born.dict = Dict{};
        jb.wits.push_back(born);
        Witness first = rec;
        first.leaf = 0;
        first.path_len = 9;
        jb.wits.push_back(first);
        Witness none = rec;  // no dictionary at all: the kept chunks are empty
        none.dict = Dict{};
        jb.wits.push_back(none);
        run({jb});
        run({jb, jb});
        run({});
        Job empty;
        empty.n0 = 9;
        empty.k = 0;
        run({empty, jb, empty});
        Flat f;
        flatten({jb}, &f);
        nhip_ms_updated count{};
        CHECK(nhip_ms_revert_plan(&f.block, &f.wit, &count) == NHIP_OK);
        // a: 599 ^ 600 = 1111 (binary, four bits) -> 3 digests; first: 0 ^ 600 -> 9; four kept entries each for a, first
        // and none (chunks 70 .. 73)
        CHECK(count.aocl_digests == 3 + 9 && count.entries == 12);
    }
    for (int round = 0; round < 200; ++round) {
        std::vector<Job> jobs(g() % 5);
        for (Job& jb : jobs) jb = random_job(g);
        run(jobs);
    }
    std::printf("checks %ld failures %ld\n", checks, failures);
    return failures ? 1 : 0;
}
