// Stand-alone check of the archival mutator set's host side (csrc/ms_archive.cpp; tests/test_ms_archive_host.py): the
// level-array geometry, the build schedule of load, the shape checks of load, the restore and path plans, the
// gather's work units and the apply plan (level ranges of an append, touched chunks, lengths after, arena offsets, the
// compaction trigger), each against a brute-force restatement over random small archives.  Links ms_archive.cpp,
// ms_update_plan.cpp and ms_shape.cpp (no HIP); built once plainly and once under ASan + UBSan.  Prints
// "checks N failures M".
#include <algorithm>
#include <cstdio>
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

// ---- 1. every node of an MMR of n leaves has a slot of its own below 2 cap, level after level
static void geometry(std::mt19937_64& g) {
    for (int round = 0; round < 60; ++round) {
        const uint64_t n = round < 20 ? (uint64_t)round : g() % 3000;
        const uint64_t floor = g() % 3 ? 0 : g() % 5000;
        const uint64_t cap = ms_arch_level_cap(n, floor);
        CHECK(cap >= n && cap >= floor && cap >= 1 && (cap & (cap - 1)) == 0);
        CHECK(cap == 1 || cap / 2 < std::max<uint64_t>({n, floor, 1}));
        std::vector<uint8_t> used(2 * cap, 0);
        uint64_t prev_end = 0;
        bool ok = true;
        for (uint32_t h = 0; (n >> h) != 0; ++h) {
            const uint64_t base = ms_arch_level_base(cap, h);
            ok &= base >= prev_end && base + (cap >> h) <= 2 * cap && (n >> h) <= (cap >> h);
            prev_end = base + (cap >> h);
            for (uint64_t k = 0; k < (n >> h); ++k) {
                const uint64_t at = ms_arch_node(cap, h, k);
                ok &= at == base + k && at < 2 * cap && !used[at] && (k + 1) << h <= n;
                if (at < 2 * cap) used[at] = 1;
            }
        }
        CHECK(ok);
    }
    CHECK(ms_arch_level_cap(MS_ARCHIVE_MAX_LEAFS, 0) == MS_ARCHIVE_MAX_LEAFS);
    CHECK(ms_arch_level_cap(MS_ARCHIVE_MAX_LEAFS + 1, 0) == 0 && ms_arch_level_cap(0, MS_ARCHIVE_MAX_LEAFS + 1) == 0);
}

// ---- 2. the path of leaf i: the siblings inside the subtree of the peak that holds it, found by walking the peaks
static std::vector<std::pair<uint32_t, uint64_t>> brute_path(uint64_t i, uint64_t n) {
    uint64_t first = 0;
    for (int h = 63; h >= 0; --h) {
        if (!(n >> h & 1)) continue;
        if (i < first + (1ull << h)) {
            std::vector<std::pair<uint32_t, uint64_t>> p;
            for (uint32_t t = 0; t < (uint32_t)h; ++t) p.push_back({t, (first >> t) + ((((i - first) >> t)) ^ 1)});
            return p;
        }
        first += 1ull << h;
    }
    return {};
}

static void paths(std::mt19937_64& g) {
    for (uint64_t n = 1; n <= 300; n += (n < 40 ? 1 : 1 + g() % 23)) {
        std::vector<uint64_t> idx, off;
        for (uint64_t i = 0; i < n; ++i) idx.push_back(i);
        CHECK(ms_archive_paths_plan(n, idx.data(), idx.size(), &off) == NHIP_OK && off.size() == n + 1 && off[0] == 0);
        bool ok = true;
        for (uint64_t i = 0; i < n; ++i) {
            const auto want = brute_path(i, n);
            ok &= ms_arch_path_len(i, n) == want.size() && off[i + 1] - off[i] == want.size();
            for (uint32_t t = 0; t < want.size() && ok; ++t) {
                const uint64_t k = (i >> t) ^ 1;
                ok &= want[t] == std::make_pair(t, k) && (k + 1) << t <= n;  // the sibling exists
            }
        }
        CHECK(ok);
        const uint64_t bad[3] = {0, n, 1};
        std::vector<uint64_t> keep = off;
        CHECK(ms_archive_paths_plan(n, bad, 3, &off) == NHIP_ERR_ARG && off == keep);
        CHECK(ms_archive_paths_plan(n, nullptr, 2, &off) == NHIP_ERR_ARG);
        CHECK(ms_archive_paths_plan(n, nullptr, 0, &off) == NHIP_OK && off == std::vector<uint64_t>{0});
    }
}

// ---- 3. load's schedule writes every level above the leaves once, bottom up, the wide ones by a launch each
static void schedule(std::mt19937_64& g) {
    const uint64_t T = MS_ARCHIVE_TAIL_NODES;
    std::vector<uint64_t> ns = {0, 1, 2, 3, 7, 8, 9, T, T + 1, 2 * T, 2 * T + 1, 2 * T + 2, 4 * T + 3, 8 * T, 1ull << 20, 1ull << 40};
    for (int k = 0; k < 200; ++k) ns.push_back(g() % (1ull << (1 + g() % 30)));
    for (uint64_t n : ns) {
        const MsArchBuild b = ms_arch_build(n);
        uint32_t top = 0;
        while ((n >> (top + 1)) != 0) ++top;
        CHECK(b.top == top && b.tail_from == b.wide_levels + 1 && b.tail_from >= 1);
        bool ok = true;
        for (uint32_t h = 1; h <= b.wide_levels; ++h) ok &= (n >> (h - 1)) > T;
        for (uint32_t h = b.tail_from; h < 64; ++h) ok &= (n >> (h - 1)) <= T;
        CHECK(ok);
    }
    CHECK(ms_arch_build(4 * T + 3).wide_levels == 2);  // 4 T + 3 and 2 T + 1 nodes are read by a launch each, T by the tail
    CHECK(ms_arch_build(T).wide_levels == 0 && ms_arch_build(T + 1).wide_levels == 1 && ms_arch_build(2 * T + 1).wide_levels == 1);
}

// ---- 4. load's shape checks
struct LoadArgs {
    std::vector<uint64_t> leaves, rel_off;
    std::vector<uint32_t> rel, active;
    uint64_t n = 0;
    int ok() const {
        return ms_archive_load_ok(leaves.data(), n, rel_off.data(), rel.empty() ? nullptr : rel.data(), rel_off.size() - 1,
                                  active.empty() ? nullptr : active.data(), active.size());
    }
};

static LoadArgs random_load(std::mt19937_64& g, uint64_t n) {
    LoadArgs a;
    a.n = n;
    a.leaves.assign(5 * n + 1, 7);
    a.rel_off.push_back(0);
    for (uint64_t c = 0; c < batch_of(n); ++c) {
        std::vector<uint32_t> ch(g() % 14);
        for (uint32_t& x : ch) x = (uint32_t)(g() % 4096);
        if (ch.size() > 2 && g() % 2) ch[1] = ch[0];  // a repeat is kept
        std::sort(ch.begin(), ch.end());
        a.rel.insert(a.rel.end(), ch.begin(), ch.end());
        a.rel_off.push_back(a.rel.size());
    }
    a.active.resize(g() % 30);
    for (uint32_t& x : a.active) x = (uint32_t)(g() % (1u << 20));
    std::sort(a.active.begin(), a.active.end());
    return a;
}

static void load_checks(std::mt19937_64& g) {
    for (int round = 0; round < 300; ++round) {
        const uint64_t n = round < 30 ? (uint64_t)round : g() % 400;
        const LoadArgs a = random_load(g, n);
        CHECK(a.ok() == NHIP_OK);
        MsArchiveMirror m;
        CHECK(m.empty());
        ms_archive_load_commit(m, n, a.rel_off.data(), a.rel_off.size() - 1, a.active.data(), a.active.size(), 4, 2);
        bool ok = m.aocl_leafs == n && m.chunks() == batch_of(n) && m.window == a.active && m.rel_tail == a.rel.size() &&
                  m.rel_live == a.rel.size() && m.rel_dead() == 0 && m.aocl_cap == 4 && m.swbf_cap == 2;
        for (uint64_t c = 0; c < m.chunks(); ++c)
            ok &= m.chunk_off[c] == a.rel_off[c] && m.chunk_len[c] == a.rel_off[c + 1] - a.rel_off[c];
        CHECK(ok);
        CHECK(m.empty() == (n == 0 && a.active.empty()));
        {  // one chunk more or fewer than the batch index
            LoadArgs b = a;
            b.rel_off.push_back(b.rel_off.back());
            CHECK(b.ok() == NHIP_ERR_ARG);
            if (a.rel_off.size() > 1) {
                b = a;
                b.rel_off.pop_back();
                CHECK(b.ok() == NHIP_ERR_ARG);
            }
        }
        if (a.rel_off.size() > 1) {
            LoadArgs b = a;
            b.rel_off[0] = 1;
            CHECK(b.ok() == NHIP_ERR_ARG);
            if (a.rel_off.size() > 2 && a.rel_off[1] < a.rel_off.back()) {
                b = a;
                b.rel_off[1] = b.rel_off.back() + 1;  // decreases behind it
                b.rel.resize(b.rel_off[1], 0);
                CHECK(b.ok() == NHIP_ERR_ARG);
            }
        }
        for (uint64_t c = 0; c + 1 < a.rel_off.size(); ++c) {
            const uint64_t lo = a.rel_off[c], hi = a.rel_off[c + 1];
            if (hi - lo >= 2 && a.rel[lo] != a.rel[hi - 1]) {
                LoadArgs b = a;
                std::swap(b.rel[lo], b.rel[hi - 1]);  // unsorted
                CHECK(b.ok() == NHIP_ERR_ARG);
                b = a;
                b.rel[hi - 1] = 4096;
                CHECK(b.ok() == NHIP_ERR_ARG);
                b.rel[hi - 1] = 4095;
                CHECK(b.ok() == NHIP_OK);
                break;
            }
        }
        if (a.active.size() >= 2 && a.active.front() != a.active.back()) {
            LoadArgs b = a;
            std::swap(b.active.front(), b.active.back());
            CHECK(b.ok() == NHIP_ERR_ARG);
            b = a;
            b.active.back() = 1u << 20;
            CHECK(b.ok() == NHIP_ERR_ARG);
            b.active.back() = (1u << 20) - 1;
            CHECK(b.ok() == NHIP_OK);
        }
        if (n) CHECK(ms_archive_load_ok(nullptr, n, a.rel_off.data(), a.rel.data(), a.rel_off.size() - 1, a.active.data(),
                                        a.active.size()) == NHIP_ERR_ARG);
        if (!a.rel.empty())
            CHECK(ms_archive_load_ok(a.leaves.data(), n, a.rel_off.data(), nullptr, a.rel_off.size() - 1, a.active.data(),
                                     a.active.size()) == NHIP_ERR_ARG);
        if (!a.active.empty())
            CHECK(ms_archive_load_ok(a.leaves.data(), n, a.rel_off.data(), a.rel.data(), a.rel_off.size() - 1, nullptr,
                                     a.active.size()) == NHIP_ERR_ARG);
    }
}

// ---- 5. the restore plan against plain sets, and the work units of its three pools
using u128 = unsigned __int128;

static void units_check(const std::vector<uint64_t>& off, uint64_t scale, bool pairs) {
    const size_t owners = off.size() - 1;
    const MsArchUnits u = ms_arch_units(off.data(), owners, scale, pairs);
    const uint64_t per = (pairs ? 2 : 1) * MS_ARCHIVE_GATHER_UNIT, total = off[owners] * scale;
    CHECK(u.units == (total + per - 1) / per && u.first.size() == u.units + 1);
    CHECK(u.first[u.units] == (owners ? owners - 1 : 0));
    bool ok = true;
    for (uint64_t k = 0; k < u.units; ++k) {
        const uint64_t g0 = k * per;
        size_t want = 0;  // the one owner whose range holds the unit's first word
        while (!(off[want] * scale <= g0 && g0 < off[want + 1] * scale)) ++want;
        ok &= u.first[k] == want;
        // what the kernel relies on: every word of the unit has its owner in [first[k], first[k + 1]]
        const uint64_t g1 = std::min(g0 + per, total);
        for (uint64_t g = g0; g < g1; g += 1 + (g1 - g0) / 64) {
            size_t s = 0;
            while (!(off[s] * scale <= g && g < off[s + 1] * scale)) ++s;
            ok &= u.first[k] <= s && s <= u.first[k + 1];
        }
        size_t s = 0;
        while (!(off[s] * scale <= g1 - 1 && g1 - 1 < off[s + 1] * scale)) ++s;
        ok &= s <= u.first[k + 1];
    }
    CHECK(ok);
}

static void restore(std::mt19937_64& g) {
    for (int round = 0; round < 250; ++round) {
        const uint64_t n_leafs = round < 12 ? (uint64_t)round : g() % 3000;
        const uint64_t b = batch_of(n_leafs);
        std::vector<uint64_t> len(b);
        for (uint64_t& l : len) l = g() % 4 ? g() % 600 : 0;
        const size_t W = round % 7 == 0 ? 0 : 1 + g() % 40;
        std::vector<uint64_t> mn(2 * W + 2), li(W + 1);
        std::vector<uint32_t> dist(45 * W + 1);
        for (size_t w = 0; w < W; ++w) {
            const uint64_t home = b ? g() % (b + 1) : 0;  // a batch the set is drawn around
            mn[2 * w] = home * 4096 - std::min<uint64_t>(home * 4096, g() % (40 * 4096)) + g() % 4096;
            mn[2 * w + 1] = 0;
            for (int t = 0; t < 45; ++t) dist[45 * w + t] = (uint32_t)(g() % (1u << 20));
            switch (g() % 12) {
            case 0: mn[2 * w] = mn[2 * w + 1] = ~0ull; break;             // saturates
            case 1: mn[2 * w] = (b + 256) * 4096; break;                   // past the window
            case 2: mn[2 * w + 1] = 1; break;                              // far past it
            case 3: dist[45 * w + 44] = 0xFFFFFFFFu; break;
            default: break;
            }
            li[w] = g() % 3 == 0 ? MS_UPDATE_NONE : (g() % 8 == 0 ? n_leafs + g() % 2 : (n_leafs ? g() % n_leafs : 0));
        }
        MsUpdatePlan p;
        std::vector<uint8_t> st;
        CHECK(ms_archive_restore_plan(n_leafs, len.data(), b, mn.data(), dist.data(), li.data(), W, &p, &st) == NHIP_OK);
        CHECK(p.wit_job.size() == W && p.aocl_path_off.size() == W + 1 && p.entry_off.size() == W + 1 && st.size() == W);
        const size_t E = p.chunk_index.size();
        CHECK(p.path_off.size() == E + 1 && p.rel_off.size() == E + 1 && p.ent_wit.size() == E && p.entry_off[W] == E);
        bool ok = true;
        for (size_t w = 0; w < W && ok; ++w) {
            const u128 m = ((u128)mn[2 * w + 1] << 64) | mn[2 * w];
            uint8_t want = NHIP_MS_OK;
            std::set<uint64_t> keys;
            bool bad = false;
            for (int t = 0; t < 45; ++t) {
                const u128 index = m + dist[45 * w + t];
                if (index < m || (index >> 12) > (u128)b + 255) bad = true;
                else if ((uint64_t)(index >> 12) < b) keys.insert((uint64_t)(index >> 12));
            }
            if (n_leafs == 0 || (li[w] != MS_UPDATE_NONE && li[w] >= n_leafs)) want = NHIP_MS_NOT_IN_AOCL;
            else if (bad) want = NHIP_MS_OUT_OF_RANGE;
            ok &= st[w] == want;
            const uint64_t alen = p.aocl_path_off[w + 1] - p.aocl_path_off[w];
            const uint64_t e0 = p.entry_off[w], e1 = p.entry_off[w + 1];
            if (want != NHIP_MS_OK) {
                ok &= alen == 0 && e0 == e1;
                continue;
            }
            ok &= alen == (li[w] == MS_UPDATE_NONE ? 0 : brute_path(li[w], n_leafs).size());
            ok &= e1 - e0 == keys.size();
            uint64_t e = e0;
            for (uint64_t c : keys) {
                if (e >= e1) break;
                ok &= p.chunk_index[e] == c && p.ent_wit[e] == w && p.path_off[e + 1] - p.path_off[e] == brute_path(c, b).size() &&
                      p.rel_off[e + 1] - p.rel_off[e] == len[c];
                ++e;
            }
        }
        CHECK(ok);
        units_check(p.aocl_path_off, 5, false);
        units_check(p.path_off, 5, false);
        units_check(p.rel_off, 1, true);
        // the chunk table has to be the batch index long; null arrays with witnesses are shape errors
        MsUpdatePlan keep = p;
        CHECK(ms_archive_restore_plan(n_leafs, len.data(), b + 1, mn.data(), dist.data(), li.data(), W, &p, &st) == NHIP_ERR_ARG);
        if (W) CHECK(ms_archive_restore_plan(n_leafs, len.data(), b, nullptr, dist.data(), li.data(), W, &p, &st) == NHIP_ERR_ARG);
        if (W) CHECK(ms_archive_restore_plan(n_leafs, len.data(), b, mn.data(), dist.data(), nullptr, W, &p, &st) == NHIP_ERR_ARG);
        CHECK(p.chunk_index == keep.chunk_index && p.rel_off == keep.rel_off);  // an error leaves the outputs alone
    }
    // long ranges: units that lie inside one owner, owners that lie inside one unit, empty owners at both ends
    for (int round = 0; round < 40; ++round) {
        std::vector<uint64_t> off{0};
        const size_t owners = 1 + g() % 60;
        for (size_t i = 0; i < owners; ++i) off.push_back(off.back() + (g() % 3 == 0 ? 0 : g() % 4 == 0 ? g() % 9000 : g() % 30));
        if (off.back() == 0) off.back() = 1;
        units_check(off, 5, false);
        units_check(off, 1, false);
        units_check(off, 1, true);
    }
    CHECK(ms_arch_units(nullptr, 0, 5, false).units == 0 && ms_arch_units(nullptr, 0, 5, false).first == std::vector<uint32_t>{0});
}

// ---- 6. the apply plan against plain maps: the chunks written, their lengths after, the arena offsets, the live and
// dead words, the compaction trigger, and the nodes hashed again in both MMRs
#include <map>
static void apply_plan(std::mt19937_64& g) {
    for (int round = 0; round < 300; ++round) {
        const uint64_t n0 = round < 10 ? (uint64_t)round : g() % 2500;
        LoadArgs a = random_load(g, n0);
        MsArchiveMirror m;
        ms_archive_load_commit(m, n0, a.rel_off.data(), a.rel_off.size() - 1, a.active.data(), a.active.size(), 1, 1);
        if (g() % 2) {  // an arena with dead words behind it, as earlier blocks leave it
            const uint64_t dead = g() % 300;
            m.rel_tail += dead;
        }
        const uint64_t k = g() % 5 == 0 ? 2050 + g() % 100 : g() % 4 == 0 ? 0 : g() % 40;
        const size_t R = g() % 3 == 0 ? 0 : g() % 6;
        const uint64_t b0 = batch_of(n0), b1 = batch_of(n0 + k);
        std::vector<uint64_t> mn(2 * R + 2, 0);
        std::vector<uint32_t> dist(45 * R + 1, 0);
        for (size_t r = 0; r < R; ++r) {
            mn[2 * r] = (b0 ? g() % (b0 + 1) : 0) * 4096 + g() % 4096;
            for (int t = 0; t < 45; ++t) dist[45 * r + t] = (uint32_t)(g() % (1u << 20));
            if (g() % 3 == 0) dist[45 * r + 1] = dist[45 * r];  // one index twice
        }
        MsArchApplyPlan p;
        CHECK(ms_archive_apply_plan(m, k, mn.data(), dist.data(), R, &p) == NHIP_OK);
        CHECK(p.n0 == n0 && p.n1 == n0 + k && p.b0 == b0 && p.b1 == b1);
        // brute force: what every written chunk gains from the block, and what it had
        std::map<uint64_t, std::vector<uint32_t>> gain;
        for (uint64_t c = b0; c < b1; ++c) gain[c];
        for (size_t r = 0; r < R; ++r)
            for (int t = 0; t < 45; ++t) {
                const uint64_t index = mn[2 * r] + dist[45 * r + t];
                if (index / 4096 < b1) gain[index / 4096].push_back((uint32_t)(index % 4096));
            }
        bool ok = p.written.size() == gain.size();
        uint64_t tail = m.rel_tail, live = m.rel_live;
        size_t i = 0;
        for (auto& kv : gain) {
            if (!ok || i >= p.written.size()) break;
            const MsArchWritten& w = p.written[i++];
            std::sort(kv.second.begin(), kv.second.end());
            uint64_t had = 0;
            if (kv.first < b0) {
                had = m.chunk_len[kv.first];
                ok &= !w.from_window && w.a_off == m.chunk_off[kv.first];
                live -= had;
            } else {
                const uint64_t lo = (kv.first - b0) * 4096;
                for (uint32_t x : m.window) had += x >= lo && x < lo + 4096;
                ok &= (had == 0 || (w.from_window && w.a_sub == lo && m.window[w.a_off] >= lo &&
                                    (w.a_off == 0 || m.window[w.a_off - 1] < lo)));
                if (kv.first - b0 >= 256) ok &= had == 0 && w.a_len == 0;
            }
            ok &= w.c == kv.first && w.a_len == had && w.b_len == kv.second.size() && w.out_off == tail;
            ok &= std::equal(kv.second.begin(), kv.second.end(), p.block_rel.begin() + (long)w.b_off);
            tail += had + kv.second.size();
            live += had + kv.second.size();
        }
        CHECK(ok);
        CHECK(p.rel_tail_after == tail && p.rel_live_after == live && p.compact == (tail - live > live));
        // the nodes hashed again: exactly the existing nodes above a new or written leaf
        for (int w = 0; w < 2; ++w) {
            const uint64_t n = w ? b1 : n0 + k;
            std::set<uint64_t> cur;
            if (w) for (auto& kv : gain) cur.insert(kv.first);
            else for (uint64_t l = n0; l < n0 + k; ++l) cur.insert(l);
            bool same = p.lvl_off[w].size() >= 1 && p.lvl_off[w][0] == 0;
            uint32_t h = 1;
            for (; (n >> h) != 0 && !cur.empty(); ++h) {
                std::set<uint64_t> next;
                for (uint64_t x : cur) if (((x >> 1) + 1) << h <= n) next.insert(x >> 1);
                same &= p.lvl_off[w].size() > h;
                if (!same) break;
                same &= std::vector<uint64_t>(next.begin(), next.end()) ==
                        std::vector<uint64_t>(p.ids[w].begin() + p.lvl_off[w][h - 1], p.ids[w].begin() + p.lvl_off[w][h]);
                cur.swap(next);
            }
            same &= p.lvl_off[w].size() == h && p.lvl_off[w].back() == p.ids[w].size();
            CHECK(same);
        }
        // the level ranges of an append: level h of the AOCL gains exactly the nodes [n0 >> h, n1 >> h)
        bool ranges = true;
        for (uint32_t h = 1; h < p.lvl_off[0].size(); ++h) {
            const uint64_t lo = n0 >> h, hi = (n0 + k) >> h;
            ranges &= p.lvl_off[0][h] - p.lvl_off[0][h - 1] <= hi - lo + 1;  // plus the one node that was a peak's sibling
            for (uint32_t j = p.lvl_off[0][h - 1]; j < p.lvl_off[0][h]; ++j) ranges &= p.ids[0][j] >= lo && p.ids[0][j] < hi;
        }
        CHECK(ranges);
        // the mirror after, and after a compaction
        MsArchiveMirror after = m;
        std::vector<uint32_t> win(g() % 20, 5);
        ms_archive_apply_commit(after, p, win.data(), win.size(), 8, 4);
        bool mo = after.aocl_leafs == n0 + k && after.chunks() == b1 && after.rel_tail == tail && after.rel_live == live &&
                  after.window == win && after.aocl_cap == 8 && after.swbf_cap == 4;
        uint64_t sum = 0;
        for (uint64_t c = 0; c < b1; ++c) {
            sum += after.chunk_len[c];
            if (!gain.count(c)) mo &= after.chunk_off[c] == m.chunk_off[c] && after.chunk_len[c] == m.chunk_len[c];
        }
        mo &= sum == live;
        ms_archive_compact_commit(after);
        uint64_t at = 0;
        for (uint64_t c = 0; c < b1; ++c) {
            mo &= after.chunk_off[c] == at;
            at += after.chunk_len[c];
        }
        mo &= after.rel_tail == live && after.rel_dead() == 0;
        CHECK(mo);
    }
    MsArchiveMirror m;
    MsArchApplyPlan p;
    m.aocl_leafs = MS_ARCHIVE_MAX_LEAFS;
    m.chunk_off.assign(1, 0), m.chunk_len.assign(1, 0);
    CHECK(ms_archive_apply_plan(m, 1, nullptr, nullptr, 0, &p) == NHIP_ERR_OOM);
    CHECK(ms_archive_grown(0, 5, 100) == 5 && ms_archive_grown(8, 9, 100) == 16 && ms_archive_grown(8, 40, 100) == 40 &&
          ms_archive_grown(60, 61, 100) == 100 && ms_archive_grown(8, 101, 100) == 0 && ms_archive_grown(8, 3, 100) == 8);
}

int main() {
    std::mt19937_64 g(20261021);
    geometry(g);
    paths(g);
    schedule(g);
    load_checks(g);
    restore(g);
    apply_plan(g);
    std::printf("checks %ld failures %ld\n", checks, failures);
    return failures ? 1 : 0;
}
