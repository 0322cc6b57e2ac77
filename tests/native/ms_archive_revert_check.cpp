// Stand-alone check of the archival mutator set's revert plan (csrc/ms_archive.cpp: ms_archive_revert_plan,
// ms_archive_revert_commit; tests/test_ms_archive_revert_host.py) against brute force over plain maps: the chunks
// rewritten, their lengths, the tail offsets, the live and dead words, the compaction trigger, the SWBF nodes hashed
// again (each exists at b0, none is missing); a revert behind an apply returns the mirror's counts, lengths and window;
// every input that no block can have led to is reported and touches nothing.  Links ms_archive.cpp, ms_update_plan.cpp
// and ms_shape.cpp (no HIP); built once plainly and once under ASan + UBSan.  Prints "checks N failures M".
#include <algorithm>
#include <cstdio>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "../../neptune-core_amd/csrc/ms_archive.hpp"

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

static uint64_t batch_of(uint64_t n) { return (n ? n - 1 : 0) / 8; }

struct Block {
    uint64_t k = 0;
    size_t R = 0;
    std::vector<uint64_t> mn;
    std::vector<uint32_t> dist;
};

// a mirror of n leaves with chunks of 0 to 13 words, a window, and perhaps dead words behind the arena
static MsArchiveMirror random_mirror(std::mt19937_64& g, uint64_t n) {
    MsArchiveMirror m;
    std::vector<uint64_t> rel_off{0};
    for (uint64_t c = 0; c < batch_of(n); ++c) rel_off.push_back(rel_off.back() + g() % 14);
    std::vector<uint32_t> active(g() % 30);
    for (uint32_t& x : active) x = (uint32_t)(g() % (1u << 20));
    std::sort(active.begin(), active.end());
    ms_archive_load_commit(m, n, rel_off.data(), rel_off.size() - 1, active.data(), active.size(), 1, 1);
    if (g() % 2) m.rel_tail += g() % 300;
    return m;
}

static Block random_block(std::mt19937_64& g, uint64_t n0) {
    Block b;
    b.k = g() % 5 == 0 ? 2050 + g() % 100 : g() % 4 == 0 ? 0 : g() % 40;
    b.R = g() % 3 == 0 ? 0 : g() % 6;
    const uint64_t b0 = batch_of(n0);
    b.mn.assign(2 * b.R + 2, 0);
    b.dist.assign(45 * b.R + 1, 0);
    for (size_t r = 0; r < b.R; ++r) {
        b.mn[2 * r] = (b0 ? g() % (b0 + 1) : 0) * 4096 + g() % 4096;
        for (int t = 0; t < 45; ++t) b.dist[45 * r + t] = (uint32_t)(g() % (1u << 20));
        if (g() % 3 == 0) b.dist[45 * r + 1] = b.dist[45 * r];  // one index twice
        if (g() % 4 == 0)                                         // many indices in one low chunk
            for (int t = 2; t < 12; ++t) b.dist[45 * r + t] = (uint32_t)(g() % 64);
    }
    return b;
}

static bool same_plan(const MsArchRevertPlan& a, const MsArchRevertPlan& b) {
    bool ok = a.n0 == b.n0 && a.n1 == b.n1 && a.b0 == b.b0 && a.b1 == b.b1 && a.rewritten.size() == b.rewritten.size() &&
              a.block_rel == b.block_rel && a.ids == b.ids && a.lvl_off == b.lvl_off && a.compact == b.compact &&
              a.rel_tail_after == b.rel_tail_after && a.rel_live_after == b.rel_live_after && a.dropped_words == b.dropped_words;
    for (size_t i = 0; ok && i < a.rewritten.size(); ++i) ok = a.rewritten[i].c == b.rewritten[i].c && a.rewritten[i].out_off == b.rewritten[i].out_off;
    return ok;
}

static bool same_mirror(const MsArchiveMirror& a, const MsArchiveMirror& b) {
    return a.aocl_leafs == b.aocl_leafs && a.chunk_off == b.chunk_off && a.chunk_len == b.chunk_len && a.window == b.window &&
           a.rel_tail == b.rel_tail && a.rel_live == b.rel_live && a.aocl_cap == b.aocl_cap && a.swbf_cap == b.swbf_cap;
}

// the revert plan of `blk` on m1 (the mirror behind the block) against brute force; m0: the mirror before the block
static void one_batch(const MsArchiveMirror& m0, const MsArchiveMirror& m1, const Block& blk) {
    const uint64_t n1 = m1.aocl_leafs, n0 = n1 - blk.k, b0 = batch_of(n0), b1 = m1.chunks();
    MsArchRevertPlan p;
    CHECK(ms_archive_revert_plan(m1, blk.k, blk.mn.data(), blk.dist.data(), blk.R, &p) == NHIP_OK);
    CHECK(p.n0 == n0 && p.n1 == n1 && p.b0 == b0 && p.b1 == b1 && b1 == batch_of(n1));
    std::map<uint64_t, std::vector<uint32_t>> loss;
    for (size_t r = 0; r < blk.R; ++r)
        for (int t = 0; t < 45; ++t) {
            const uint64_t index = blk.mn[2 * r] + blk.dist[45 * r + t];
            if (index / 4096 < b0) loss[index / 4096].push_back((uint32_t)(index % 4096));
        }
    bool ok = p.rewritten.size() == loss.size();
    uint64_t tail = m1.rel_tail, live = m1.rel_live, dropped = 0;
    size_t i = 0;
    for (auto& kv : loss) {
        if (!ok) break;
        const MsArchWritten& w = p.rewritten[i++];
        std::sort(kv.second.begin(), kv.second.end());
        ok &= w.c == kv.first && w.c < b0 && w.a_off == m1.chunk_off[kv.first] && w.a_len == m1.chunk_len[kv.first] &&
              w.b_len == kv.second.size() && w.a_len >= w.b_len && w.out_off == tail && !w.from_window && w.a_sub == 0;
        ok &= w.a_off + w.a_len <= m1.rel_tail;  // reads stay below the old tail
        ok &= w.b_off + w.b_len <= p.block_rel.size() &&
              std::equal(kv.second.begin(), kv.second.end(), p.block_rel.begin() + (long)w.b_off);
        ok &= w.a_len - w.b_len == m0.chunk_len[kv.first];  // the length before the block
        tail += w.a_len - w.b_len;
        live -= w.b_len;
    }
    CHECK(ok);
    for (uint64_t c = b0; c < b1; ++c) dropped += m1.chunk_len[c];
    live -= dropped;
    CHECK(p.dropped_words == dropped && p.rel_tail_after == tail && p.rel_live_after == live && live == m0.rel_live);
    CHECK(p.compact == (tail - live > live));
    // the nodes hashed again: exactly the nodes that exist at b0 above a rewritten chunk
    std::set<uint64_t> cur;
    for (auto& kv : loss) cur.insert(kv.first);
    bool same = p.lvl_off.size() >= 1 && p.lvl_off[0] == 0;
    uint32_t h = 1;
    for (; (b0 >> h) != 0 && !cur.empty(); ++h) {
        std::set<uint64_t> next;
        for (uint64_t x : cur)
            if (((x >> 1) + 1) << h <= b0) next.insert(x >> 1);
        same &= p.lvl_off.size() > h;
        if (!same) break;
        same &= std::vector<uint64_t>(next.begin(), next.end()) ==
                std::vector<uint64_t>(p.ids.begin() + p.lvl_off[h - 1], p.ids.begin() + p.lvl_off[h]);
        for (uint32_t j = p.lvl_off[h - 1]; j < p.lvl_off[h]; ++j) same &= (p.ids[j] + 1) << h <= b0;  // exists at b0
        cur.swap(next);
    }
    same &= p.lvl_off.size() == h && p.lvl_off.back() == p.ids.size();
    CHECK(same);
    // the commit returns the mirror before the block: counts, lengths, window; offsets where the plan wrote; no
    // capacity shrinks
    MsArchiveMirror back = m1;
    ms_archive_revert_commit(back, p, m0.window.data(), m0.window.size());
    bool mo = back.aocl_leafs == m0.aocl_leafs && back.chunks() == m0.chunks() && back.chunk_len == m0.chunk_len &&
              back.window == m0.window && back.rel_live == m0.rel_live && back.rel_tail == tail &&
              back.aocl_cap == m1.aocl_cap && back.swbf_cap == m1.swbf_cap;
    uint64_t sum = 0;
    for (uint64_t c = 0; c < back.chunks(); ++c) {
        sum += back.chunk_len[c];
        mo &= back.chunk_off[c] == (loss.count(c) ? p.rewritten[(size_t)std::distance(loss.begin(), loss.find(c))].out_off : m1.chunk_off[c]);
        mo &= back.chunk_off[c] + back.chunk_len[c] <= tail;
    }
    mo &= sum == back.rel_live;
    CHECK(mo);
}

static void random_batches(std::mt19937_64& g) {
    for (int round = 0; round < 400; ++round) {
        const uint64_t n0 = round < 12 ? (uint64_t)round : g() % 2500;
        const MsArchiveMirror m0 = random_mirror(g, n0);
        const Block blk = random_block(g, n0);
        MsArchApplyPlan ap;
        CHECK(ms_archive_apply_plan(m0, blk.k, blk.mn.data(), blk.dist.data(), blk.R, &ap) == NHIP_OK);
        MsArchiveMirror m1 = m0;
        std::vector<uint32_t> win(g() % 20, 5);
        ms_archive_apply_commit(m1, ap, win.data(), win.size(), 8, 4);
        if (round % 3 == 0) ms_archive_compact_commit(m1);  // other arena offsets, no dead words
        one_batch(m0, m1, blk);
    }
}

// a fixed batch, by hand: 20 leaves (chunks 0 and 1), a block of 12 additions (b 2 -> 3) whose one record puts 3 in
// chunk 0 twice, 7 in chunk 1 once, and everything else at or beyond chunk 3
static void fixed_batch() {
    MsArchiveMirror m0;
    const uint64_t rel_off[3] = {0, 2, 2};  // chunk 0: two words, chunk 1: none
    const uint32_t active[2] = {10, 5000};
    ms_archive_load_commit(m0, 20, rel_off, 2, active, 2, 32, 4);
    Block blk;
    blk.k = 12, blk.R = 1;
    blk.mn = {3, 0};
    blk.dist.assign(45, 0);
    blk.dist[1] = 0;
    blk.dist[2] = 4096 + 7 - 3;
    for (int t = 3; t < 45; ++t) blk.dist[t] = 3 * 4096 + (uint32_t)t;
    MsArchApplyPlan ap;
    CHECK(ms_archive_apply_plan(m0, blk.k, blk.mn.data(), blk.dist.data(), blk.R, &ap) == NHIP_OK);
    MsArchiveMirror m1 = m0;
    const uint32_t after[1] = {904};
    ms_archive_apply_commit(m1, ap, after, 1, 32, 4);
    CHECK(m1.chunks() == 3 && m1.chunk_len == (std::vector<uint64_t>{4, 1, 1}) && m1.rel_tail == 8 && m1.rel_live == 6);
    MsArchRevertPlan p;
    CHECK(ms_archive_revert_plan(m1, 12, blk.mn.data(), blk.dist.data(), 1, &p) == NHIP_OK);
    CHECK(p.n0 == 20 && p.n1 == 32 && p.b0 == 2 && p.b1 == 3 && p.rewritten.size() == 2 && p.dropped_words == 1);
    CHECK(p.block_rel == (std::vector<uint32_t>{3, 3, 7}));
    if (p.rewritten.size() == 2) {
        const MsArchWritten &w0 = p.rewritten[0], &w1 = p.rewritten[1];
        CHECK(w0.c == 0 && w0.a_off == 2 && w0.a_len == 4 && w0.b_off == 0 && w0.b_len == 2 && w0.out_off == 8);
        CHECK(w1.c == 1 && w1.a_off == 6 && w1.a_len == 1 && w1.b_off == 2 && w1.b_len == 1 && w1.out_off == 10);
    }
    CHECK(p.rel_tail_after == 10 && p.rel_live_after == 2 && p.compact);  // 8 dead, 2 live
    CHECK(p.lvl_off == (std::vector<uint32_t>{0, 1}) && p.ids == (std::vector<uint64_t>{0}));  // node (1, 0) exists at b0 = 2
    one_batch(m0, m1, blk);
    // a block of nothing: nothing rewritten, nothing dropped, nothing hashed
    CHECK(ms_archive_revert_plan(m1, 0, nullptr, nullptr, 0, &p) == NHIP_OK);
    CHECK(p.n0 == 32 && p.b0 == 3 && p.rewritten.empty() && p.ids.empty() && p.dropped_words == 0 && p.rel_tail_after == 8 &&
          p.rel_live_after == 6 && !p.compact);
    MsArchiveMirror same = m1;
    ms_archive_revert_commit(same, p, after, 1);
    CHECK(same_mirror(same, m1));
    // down to nothing: an empty mirror again
    MsArchiveMirror e;
    MsArchApplyPlan ap0;
    CHECK(ms_archive_apply_plan(e, 17, nullptr, nullptr, 0, &ap0) == NHIP_OK);
    MsArchiveMirror e1 = e;
    ms_archive_apply_commit(e1, ap0, after, 1, 32, 2);
    CHECK(ms_archive_revert_plan(e1, 17, nullptr, nullptr, 0, &p) == NHIP_OK && p.n0 == 0 && p.b0 == 0 && p.b1 == 2);
    ms_archive_revert_commit(e1, p, nullptr, 0);
    CHECK(e1.empty() && e1.rel_live == 0 && e1.aocl_cap == 32 && e1.swbf_cap == 2);
}

// inputs no block can have led to: reported, and neither the plan nor the mirror is touched; under ASan no read or
// write leaves a vector
static void impossible(std::mt19937_64& g) {
    MsArchRevertPlan sentinel;
    sentinel.n0 = 77, sentinel.block_rel = {1, 2, 3}, sentinel.ids = {9}, sentinel.lvl_off = {0, 1};
    for (int round = 0; round < 120; ++round) {
        const uint64_t n = 9 + g() % 900;
        MsArchiveMirror m = random_mirror(g, n);
        const MsArchiveMirror keep = m;
        MsArchRevertPlan p = sentinel;
        // more additions than leaves
        CHECK(ms_archive_revert_plan(m, n + 1 + g() % 5, nullptr, nullptr, 0, &p) == MS_ARCHIVE_REVERT_IMPOSSIBLE);
        CHECK(ms_archive_revert_plan(m, ~0ull, nullptr, nullptr, 0, &p) == MS_ARCHIVE_REVERT_IMPOSSIBLE);
        // a table shorter than the batch index before the block
        MsArchiveMirror cut = m;
        const size_t fewer = (size_t)(g() % cut.chunks());
        cut.chunk_off.resize(fewer), cut.chunk_len.resize(fewer);
        CHECK(ms_archive_revert_plan(cut, 0, nullptr, nullptr, 0, &p) == MS_ARCHIVE_REVERT_IMPOSSIBLE);
        // a hit chunk with fewer words than block indices in it: 45 indices into one chunk of at most 13 words
        const uint64_t c = g() % m.chunks();
        std::vector<uint64_t> mn{c * 4096 + 5, 0};
        std::vector<uint32_t> dist(45);
        for (int t = 0; t < 45; ++t) dist[t] = (uint32_t)(g() % 4000);
        CHECK(m.chunk_len[c] < 45 && ms_archive_revert_plan(m, 0, mn.data(), dist.data(), 1, &p) == MS_ARCHIVE_REVERT_IMPOSSIBLE);
        // indices that wrap u128, or lie at or beyond b0, are nobody's: possible, nothing rewritten
        std::vector<uint64_t> far{~0ull, ~0ull};
        MsArchRevertPlan q;
        CHECK(ms_archive_revert_plan(m, 0, far.data(), dist.data(), 1, &q) == NHIP_OK && q.rewritten.empty());
        far = {m.chunks() * 4096, 0};
        CHECK(ms_archive_revert_plan(m, 0, far.data(), dist.data(), 1, &q) == NHIP_OK && q.rewritten.empty());
        CHECK(same_plan(p, sentinel) && same_mirror(m, keep));
        // records without their arrays
        CHECK(ms_archive_revert_plan(m, 0, nullptr, dist.data(), 1, &p) == NHIP_ERR_ARG);
        CHECK(ms_archive_revert_plan(m, 0, mn.data(), nullptr, 1, &p) == NHIP_ERR_ARG);
        CHECK(same_plan(p, sentinel));
    }
    MsArchiveMirror none;
    MsArchRevertPlan p = sentinel;
    CHECK(ms_archive_revert_plan(none, 1, nullptr, nullptr, 0, &p) == MS_ARCHIVE_REVERT_IMPOSSIBLE && same_plan(p, sentinel));
    CHECK(ms_archive_revert_plan(none, 0, nullptr, nullptr, 0, &p) == NHIP_OK && p.n0 == 0 && p.rewritten.empty() && !p.compact);
    CHECK(MS_ARCHIVE_REVERT_IMPOSSIBLE != NHIP_OK && MS_ARCHIVE_REVERT_IMPOSSIBLE != NHIP_ERR_ARG &&
          MS_ARCHIVE_REVERT_IMPOSSIBLE != NHIP_ERR_OOM && MS_ARCHIVE_REVERT_IMPOSSIBLE != NHIP_ERR_HIP);
}

int main() {
    std::mt19937_64 g(20261022);
    fixed_batch();
    random_batches(g);
    impossible(g);
    std::printf("checks %ld failures %ld\n", checks, failures);
    return failures ? 1 : 0;
}
