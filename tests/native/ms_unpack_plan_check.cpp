// Stand-alone check of the host plan of block rule 2.a (csrc/ms_unpack_plan.cpp) under ASan + UBSan
// (tests/test_ms_unpack_plan.py builds it with ms_unpack_plan.mk and runs it directly): a fixed batch, then seeded
// random packed lists, valid and mutated.  A valid list must plan to NHIP_MS_OK with the node sets a naive
// recomputation gives (std::set per tree: leaves, needed-minus-computable structure nodes, the reference's
// repeat-until-nothing-changes family completion).  Every plan, whatever its status, must be a program that stays
// inside its buffers and whose parent ops have both children known before use.  Hashes nothing.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "../../neptune-core_amd/csrc/ms_unpack_plan.hpp"

static long checks = 0, failures = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        ++checks;                                                        \
        if (!(c)) {                                                      \
            ++failures;                                                  \
            if (failures < 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                                \
    } while (0)

struct List {  // one packed list and, when it was generated as valid, what the naive recomputation expects
    std::vector<uint64_t> minimum;
    std::vector<uint32_t> distances;
    std::vector<uint64_t> entry_off{0}, key, path_off{0}, rel_off{0};
    std::vector<uint32_t> rel;
    uint64_t swbfi = 0;
    size_t known = 0, leaves = 0, structure = 0;
    bool valid = false;
};

static std::vector<uint32_t> pack_chunk(const std::vector<uint32_t>& idx) {
    std::vector<uint32_t> out;
    if (idx.empty()) return out;
    uint64_t cur = 0;
    unsigned width = 0;
    auto put = [&](uint32_t f) {
        cur = (cur << 12) | f;
        width += 12;
        if (width >= 32) {
            out.push_back((uint32_t)(cur >> (width - 32)));
            width -= 32;
            cur &= (1ull << width) - 1;
        }
    };
    put((uint32_t)idx.size());
    for (uint32_t x : idx) put(x);
    if (width) out.push_back((uint32_t)(cur << (32 - width)));
    return out;
}

// the naive node sets of the trees of an MMR of s leaves with the leaves `cis`
static void naive(uint64_t s, const std::set<uint64_t>& cis, std::map<uint32_t, size_t>* structure_len, size_t* known,
                  size_t* n_structure) {
    *known = *n_structure = 0;
    for (uint32_t h = 0; h < 64; ++h) {
        if (!(s >> h & 1)) continue;
        const uint64_t first = h == 63 ? 0 : (s >> (h + 1)) << (h + 1);
        std::set<uint64_t> nodes, needed, computable;
        for (uint64_t ci : cis)
            if (ci >= first && ci - first < (1ull << h)) nodes.insert(ci - first + (1ull << h));
        for (uint64_t leaf : nodes)
            for (uint64_t x = leaf; x > 1; x >>= 1) {
                computable.insert(x);
                needed.insert(x ^ 1);
            }
        size_t len = 0;
        for (uint64_t x : needed)
            if (!computable.count(x)) {
                nodes.insert(x);
                ++len;
            }
        (*structure_len)[h] = len;
        *n_structure += len;
        for (bool grew = true; grew;) {
            grew = false;
            std::vector<uint64_t> add;
            for (uint64_t x : nodes)
                if (!(x & 1) && nodes.count(x ^ 1) && !nodes.count(x >> 1)) add.push_back(x >> 1);
            for (uint64_t x : add) grew |= nodes.insert(x).second;
        }
        *known += nodes.size();
    }
}

static List generate(std::mt19937_64& g, bool small) {
    List l;
    l.valid = true;
    const uint64_t s = small ? 1 + g() % 64 : (g() % 3 == 0 ? (1ull << (20 + g() % 30)) + g() % 4096 : 1 + g() % 5000);
    l.swbfi = s;
    const size_t m = 1 + g() % 5;
    std::set<uint64_t> cis;
    for (size_t r = 0; r < m; ++r) {
        // a record's indices: up to 256 chunks wide, the window's first chunk at most s
        const uint64_t lo = s > 200 && g() % 2 ? s - g() % 200 : g() % (s + 1);
        const uint64_t mn = lo * 4096 + g() % 4096;
        l.minimum.push_back(mn);
        l.minimum.push_back(0);
        for (int t = 0; t < 45; ++t) {
            const uint32_t d = t == 0 ? 0 : (uint32_t)(g() % (g() % 4 ? 5 * 4096 : 1u << 20));
            l.distances.push_back(d);
            const uint64_t ci = (mn + d) >> 12;
            if (ci < s) cis.insert(ci);
        }
    }
    std::map<uint32_t, size_t> len;
    naive(s, cis, &len, &l.known, &l.structure);
    l.leaves = cis.size();
    std::vector<uint32_t> heights;
    for (uint32_t h = 0; h < 64; ++h)
        if (s >> h & 1) heights.push_back(h);
    const size_t n_entries = std::max(heights.size(), cis.size());
    for (size_t e = 0; e < n_entries; ++e) {
        std::vector<uint32_t> words;
        if (e < cis.size()) {
            std::vector<uint32_t> idx(g() % 4 == 0 ? g() % 4096 : g() % 9);
            for (uint32_t& x : idx) x = (uint32_t)(g() % 4096);
            words = pack_chunk(idx);
        }
        l.key.push_back(e >= heights.size() ? UINT64_MAX : heights[e] + (e < cis.size() ? 0 : 64));
        l.path_off.push_back(l.path_off.back() + (e < heights.size() ? len[heights[e]] : 0));
        l.rel.insert(l.rel.end(), words.begin(), words.end());
        l.rel_off.push_back(l.rel.size());
    }
    l.entry_off.push_back(n_entries);
    for (size_t r = 1; r < m; ++r) l.entry_off.push_back(n_entries);
    return l;
}

static void mutate(std::mt19937_64& g, List* l) {
    l->valid = false;
    const size_t E = l->key.size();
    switch (g() % 7) {
        case 0: if (E) l->key[g() % E] = g() % 3 ? g() % 130 : g(); break;
        case 1: if (!l->rel.empty()) l->rel[g() % l->rel.size()] ^= 1u << (g() % 32); break;
        case 2: if (E) { const size_t e = g() % E; const uint64_t more = 1 + g() % 2; for (size_t k = e + 1; k <= E; ++k) l->path_off[k] += more; } break;
        case 3: l->minimum[2 * (g() % (l->minimum.size() / 2)) + (g() % 2)] = g() >> (g() % 64); break;
        case 4: if (E > 1) { l->key.pop_back(); l->path_off.pop_back(); l->rel_off.pop_back(); for (size_t r = 1; r < l->entry_off.size(); ++r) l->entry_off[r] = E - 1; } break;
        case 5: if (E > 1) std::swap(l->key[0], l->key[E - 1]); break;
        default: l->distances[g() % l->distances.size()] = (uint32_t)g(); break;
    }
}

// runs the plan over the lists as the jobs of one call and checks the program
static void run(const std::vector<List>& lists) {
    std::vector<uint64_t> rec_off{0}, minimum, entry_off{0}, key, path_off{0}, rel_off{0};
    std::vector<uint32_t> distances, rel;
    for (const List& l : lists) {
        const size_t m = l.minimum.size() / 2;
        minimum.insert(minimum.end(), l.minimum.begin(), l.minimum.end());
        distances.insert(distances.end(), l.distances.begin(), l.distances.end());
        for (size_t r = 0; r < m; ++r) entry_off.push_back(key.size() + l.entry_off[r + 1]);
        for (size_t e = 0; e < l.key.size(); ++e) {
            path_off.push_back(path_off.back() + (l.path_off[e + 1] - l.path_off[e]));
            rel_off.push_back(rel_off.back() + (l.rel_off[e + 1] - l.rel_off[e]));
        }
        key.insert(key.end(), l.key.begin(), l.key.end());
        rel.insert(rel.end(), l.rel.begin(), l.rel.begin() + (ptrdiff_t)l.rel_off[l.key.size()]);
        rec_off.push_back(rec_off.back() + m);
    }
    std::vector<uint64_t> path(5 * (size_t)path_off.back() + 1, 7);
    const nhip_ms_chunks ch{entry_off.data(), key.data(), path_off.data(), path.data(), rel_off.data(), rel.data()};
    const nhip::MsPackedIn in{rec_off.data(), lists.size(), minimum.data(), distances.data(), &ch};
    nhip::MsUnpackCounts cnt;
    const int shape = nhip::ms_packed_ok(in, &cnt);
    CHECK(shape == NHIP_OK);
    if (shape != NHIP_OK) return;
    nhip::MsUnpackPlan p;
    CHECK(nhip::ms_unpack_plan(in, cnt, &p) == NHIP_OK);
    CHECK(p.jobs.size() == lists.size() && p.entry_off.size() == rec_off.back() + 1);
    CHECK(p.path_off.size() == p.chunk_index.size() + 1 && p.rel_off.size() == p.chunk_index.size() + 1);
    CHECK(p.path_off.back() == p.gath_src.size() && p.rel_off.back() == p.rel.size());
    std::vector<char> known((size_t)p.n_slots, 0);
    uint64_t slots = 0, gath = 0;
    for (size_t j = 0; j < lists.size(); ++j) {
        const List& l = lists[j];
        const nhip::MsUnpackJob& jb = p.jobs[j];
        if (l.valid) CHECK(p.status[j] == NHIP_MS_OK && p.num_leafs_aocl[j] == 8 * l.swbfi + 1);
        if (p.status[j] != NHIP_MS_OK) {
            CHECK(jb.n_slots == 0 && jb.n_leaf == 0 && jb.n_copy == 0 && jb.n_levels == 0 && jb.n_gath == 0);
            CHECK(p.entry_off[rec_off[j]] == p.entry_off[rec_off[j + 1]]);
            continue;
        }
        CHECK(jb.slot_off == slots && jb.gath_off == gath);
        slots += jb.n_slots;
        gath += jb.n_gath;
        CHECK(slots <= p.n_slots && gath <= p.gath_src.size());
        auto mine = [&](uint32_t s) { return s >= jb.slot_off && s < jb.slot_off + jb.n_slots; };
        for (uint64_t q = jb.leaf_off; q < jb.leaf_off + jb.n_leaf; ++q) {
            CHECK(mine(p.leaf_slot[q]) && !known[p.leaf_slot[q]]);
            known[p.leaf_slot[q]] = 1;
            const uint64_t words = p.leaf_cnt[q] ? (12 * ((uint64_t)p.leaf_cnt[q] + 1) + 31) / 32 : 0;
            CHECK(p.leaf_words[q] + words <= rel.size());
        }
        for (uint64_t q = jb.copy_off; q < jb.copy_off + jb.n_copy; ++q) {
            CHECK(mine(p.copy_slot[q]) && !known[p.copy_slot[q]] && p.copy_src[q] < path_off.back());
            known[p.copy_slot[q]] = 1;
        }
        CHECK(jb.n_levels <= 63 && jb.lvl_off + jb.n_levels < p.lvl.size());
        uint64_t n_ops = 0;
        for (uint64_t k = 0; k < jb.n_levels; ++k) {
            const uint64_t beg = p.lvl[jb.lvl_off + k], end = p.lvl[jb.lvl_off + k + 1];
            CHECK(beg <= end && 3 * end <= p.op.size());
            for (uint64_t o = beg; o < end; ++o)  // both children known before the level starts
                CHECK(mine(p.op[3 * o]) && mine(p.op[3 * o + 1]) && mine(p.op[3 * o + 2]) && !known[p.op[3 * o]] &&
                      known[p.op[3 * o + 1]] && known[p.op[3 * o + 2]] && p.op[3 * o + 1] != p.op[3 * o + 2]);
            for (uint64_t o = beg; o < end; ++o) known[p.op[3 * o]] = 1;
            n_ops += end - beg;
        }
        CHECK(jb.n_leaf + jb.n_copy + n_ops == jb.n_slots);
        for (uint64_t q = jb.gath_off; q < jb.gath_off + jb.n_gath; ++q) CHECK(mine(p.gath_src[q]) && known[p.gath_src[q]]);
        if (l.valid) {
            CHECK(jb.n_slots == l.known && jb.n_leaf == l.leaves && jb.n_copy == l.structure);
            // every record's entries: its distinct inactive chunk indices, ascending, each path as tall as its tree
            for (uint64_t r = rec_off[j]; r < rec_off[j + 1]; ++r) {
                std::set<uint64_t> cis;
                for (int t = 0; t < 45; ++t) {
                    const uint64_t ci = (minimum[2 * r] + distances[45 * r + t]) >> 12;
                    if (ci < l.swbfi) cis.insert(ci);
                }
                CHECK(p.entry_off[r + 1] - p.entry_off[r] == cis.size());
                uint64_t e = p.entry_off[r];
                for (uint64_t ci : cis) {
                    const uint32_t h = 63u - (uint32_t)__builtin_clzll(ci ^ l.swbfi);
                    CHECK(p.chunk_index[e] == ci && p.path_off[e + 1] - p.path_off[e] == h);
                    ++e;
                }
            }
        }
    }
    CHECK(slots == p.n_slots && gath == p.gath_src.size());
}

int main() {
    std::mt19937_64 g(2800);
    {  // a fixed batch: small valid lists, and the same lists with a field changed
        std::vector<List> lists;
        for (int k = 0; k < 12; ++k) {
            lists.push_back(generate(g, true));
            if (k % 3 == 2) mutate(g, &lists.back());
        }
        lists.push_back(List{});  // a job without records
        lists.back().valid = true;
        lists.back().known = 0;
        run(lists);
    }
    for (int round = 0; round < 25; ++round) {  // 200 random lists, eight to a call
        std::vector<List> lists;
        for (int k = 0; k < 8; ++k) {
            lists.push_back(generate(g, round % 2 == 0));
            if (g() % 2) mutate(g, &lists.back());
        }
        run(lists);
    }
    std::printf("checks %ld failures %ld\n", checks, failures);
    return failures ? 1 : 0;
}
