#include "ms_unpack_plan.hpp"

#include <algorithm>
#include <new>
#include <thread>
#include <utility>

namespace nhip {

namespace {

using u128 = unsigned __int128;
constexpr uint32_t MAX_PACKED_LENGTH = 1536;        // chunk.rs:22
constexpr uint64_t TREE_HEIGHT_OFFSET = 64;         // removal_record_list.rs:102
constexpr uint64_t IGNORE_TREE_HEIGHT = UINT64_MAX; // :97
constexpr uint32_t NO_SLOT = UINT32_MAX;

// the known nodes of one tree on one level, sorted by node index
using Level = std::vector<std::pair<uint64_t, uint32_t>>;  // (node index, slot)

uint32_t find_slot(const Level& lv, uint64_t node) {
    auto it = std::lower_bound(lv.begin(), lv.end(), std::make_pair(node, (uint32_t)0));
    return it != lv.end() && it->first == node ? it->second : NO_SLOT;
}

struct Tree {
    uint32_t height = 0;
    std::vector<uint64_t> leaves;  // Merkle leaf indices inside the tree, ascending
    std::vector<uint32_t> leaf_slot;
    std::vector<uint64_t> structure;  // its authentication structure's node indices, in the structure's order
    std::vector<Level> known;      // [k]: nodes k levels above the leaves
    std::vector<uint32_t> path;    // height slots per leaf: its siblings, leaf level first
};

// The scratch of one job; cleared, not freed, between jobs
struct Scratch {
    std::vector<uint32_t> heights;
    std::vector<uint64_t> structs, chunks;  // entries, in dictionary order
    std::vector<uint32_t> chunk_n;
    std::vector<uint64_t> all_ci, distinct, inactive, rec_ci;
    std::vector<Tree> trees;                // ascending height; the first n_trees are the job's (never shrunk)
    size_t n_trees = 0;
    size_t j0 = 0;    // the range this scratch plans: its first job and that job's first record
    uint64_t rb = 0;
    std::vector<uint32_t> chunk_tree, chunk_leaf;  // per inactive chunk: its tree and its leaf there
    std::vector<uint32_t> unpacked;
    std::vector<uint64_t> unpacked_off;
    std::vector<size_t> want, got;
    std::vector<std::vector<uint32_t>> level_ops;
};

// leaf_index_to_mt_index_and_peak_index for ci < n: the height of the leaf's tree and its node index there
inline void locate(uint64_t ci, uint64_t n, uint32_t* height, uint64_t* node) {
    const uint32_t h = 63u - (uint32_t)__builtin_clzll(ci ^ n);
    *height = h;
    *node = (ci & ((1ull << h) - 1)) + (1ull << h);
}

}  // namespace

int ms_packed_ok(const MsPackedIn& in, MsUnpackCounts* counts) {
    MsUnpackCounts c;
    if (in.n_jobs == 0) {
        if (counts) *counts = c;
        return NHIP_OK;
    }
    if (in.n_jobs > (size_t)UINT32_MAX) return NHIP_ERR_ARG;
    if (ms_csr_ok(in.rec_off, in.n_jobs, 45 * sizeof(uint32_t), &c.records)) return NHIP_ERR_ARG;
    if (c.records) {
        if (!in.minimum || !in.distances) return NHIP_ERR_ARG;
        if (c.records > (uint64_t)UINT32_MAX / 45) return NHIP_ERR_ARG;
        if (ms_chunks_ok(in.chunks, (size_t)c.records, &c.chunks)) return NHIP_ERR_ARG;
    }
    if (counts) *counts = c;
    return NHIP_OK;
}

uint8_t ms_packed_chunk_ok(const uint32_t* words, uint64_t n_words, uint32_t* n_indices) {
    *n_indices = 0;
    if (n_words == 0) return NHIP_MS_OK;
    if (n_words > MAX_PACKED_LENGTH) return NHIP_MS_UNPACK_PAYLOAD_TOO_BIG;
    const uint32_t indicated = (words[0] >> 20) & 0xFFFu;
    if (((indicated + 1) * 12 + 31) / 32 != n_words) return NHIP_MS_UNPACK_INCONSISTENT_LENGTH;
    const uint32_t used = ((indicated + 1) * 12) % 32;
    const uint32_t mask = used ? (1u << (32 - used)) - 1u : 0u;
    if (words[n_words - 1] & mask) return NHIP_MS_UNPACK_NONZERO_TRAILING_PADDING;
    *n_indices = indicated;
    return NHIP_MS_OK;
}

void ms_auth_structure_nodes(uint32_t height, const std::vector<uint64_t>& leaves, std::vector<uint64_t>* nodes) {
    nodes->clear();
    std::vector<uint64_t> cur(leaves.size()), level;
    for (size_t i = 0; i < leaves.size(); ++i) cur[i] = leaves[i] + (1ull << height);
    for (uint32_t k = 0; k < height && !cur.empty(); ++k) {
        // deeper levels hold the larger node indices: level by level, each level descending
        level.clear();
        for (size_t i = 0; i < cur.size(); ++i) {
            const uint64_t sib = cur[i] ^ 1;
            const bool present = (i > 0 && cur[i - 1] == sib) || (i + 1 < cur.size() && cur[i + 1] == sib);
            if (!present) level.push_back(sib);
        }
        nodes->insert(nodes->end(), level.rbegin(), level.rend());
        size_t w = 0;
        for (size_t i = 0; i < cur.size(); ++i)
            if (w == 0 || cur[w - 1] != cur[i] >> 1) cur[w++] = cur[i] >> 1;
        cur.resize(w);
    }
}

namespace {

// decode_from_vec and validate_consistency: the job's status, the estimate, and the trees with their leaves
uint8_t decide(const MsPackedIn& in, size_t j, Scratch& s, uint64_t* swbfi_out) {
    const nhip_ms_chunks& ch = *in.chunks;
    const uint64_t r0 = in.rec_off[j], r1 = in.rec_off[j + 1];
    s.heights.clear();
    s.structs.clear();
    s.chunks.clear();
    s.chunk_n.clear();
    uint64_t seen = 0;
    // scan: every record's dictionary, in order
    for (uint64_t r = r0; r < r1; ++r)
        for (uint64_t e = ch.entry_off[r]; e < ch.entry_off[r + 1]; ++e) {
            const uint64_t key = ch.chunk_index[e];
            const bool has_tree = key < 2 * TREE_HEIGHT_OFFSET;
            const bool has_chunk = key < TREE_HEIGHT_OFFSET || key == IGNORE_TREE_HEIGHT;
            if (!has_tree && !has_chunk) return NHIP_MS_UNPACK_ILLEGAL_TREE_HEIGHT;
            if (has_chunk) {  // the chunk's error comes before this entry's duplicate check
                uint32_t cnt = 0;
                const uint64_t w0 = ch.rel_off[e];
                const uint8_t st = ms_packed_chunk_ok(ch.rel ? ch.rel + w0 : nullptr, ch.rel_off[e + 1] - w0, &cnt);
                if (st != NHIP_MS_OK) return st;
                s.chunks.push_back(e);
                s.chunk_n.push_back(cnt);
            }
            if (has_tree) {
                const uint32_t h = (uint32_t)(key & (TREE_HEIGHT_OFFSET - 1));
                if (seen >> h & 1) return NHIP_MS_UNPACK_DUPLICATE_TREE_HEIGHTS;
                seen |= 1ull << h;
                s.heights.push_back(h);
                s.structs.push_back(e);
            }
        }
    // observed_chunk_indices_from_index_sets: all 45 m indices, active ones included
    s.all_ci.clear();
    for (uint64_t r = r0; r < r1; ++r) {
        const u128 mn = ((u128)in.minimum[2 * r + 1] << 64) | in.minimum[2 * r];
        for (uint32_t t = 0; t < 45; ++t) {
            u128 v = mn + in.distances[45 * r + t];
            if (v < mn) v = ~(u128)0;  // AbsoluteIndexSet::to_array saturates
            if ((v >> 12) >> 64) return NHIP_MS_UNPACK_INDEX_TOO_BIG;
            s.all_ci.push_back((uint64_t)(v >> 12));
        }
    }
    s.distinct = s.all_ci;
    std::sort(s.distinct.begin(), s.distinct.end());
    s.distinct.erase(std::unique(s.distinct.begin(), s.distinct.end()), s.distinct.end());
    const size_t n_chunks = s.chunks.size();
    const size_t taken = std::min(n_chunks, s.distinct.size());
    // estimate_num_leafs_aocl
    uint64_t est = taken ? s.distinct[taken - 1] : 0;
    for (size_t k = 1; k < s.heights.size(); ++k)
        if (s.heights[k] < s.heights[k - 1]) return NHIP_MS_UNPACK_PANIC;  // the is_sorted assert
    for (size_t k = s.heights.size(); k-- > 0;) {
        const uint64_t w = 1ull << s.heights[k];
        if (!(est & w)) est = (est | w) & ~(w - 1);
    }
    if (est > (UINT64_MAX - 1) / 8) return NHIP_MS_UNPACK_PANIC;  // 8 s + 1 leaves u64
    *swbfi_out = est;  // aocl_to_swbfi_leaf_counts(8 s + 1) = s; the window starts at chunk s
    // validate_consistency 1: the distinct inactive chunk indices
    s.inactive.assign(s.distinct.begin(), std::lower_bound(s.distinct.begin(), s.distinct.end(), est));
    if (s.inactive.size() != n_chunks) return NHIP_MS_UNPACK_INCONSISTENT_CHUNKS;
    // 2: one structure per tree
    if (s.structs.size() != (size_t)__builtin_popcountll(est)) return NHIP_MS_UNPACK_STRUCTURE_COUNT;
    // the trees by ascending height, with their leaves (inactive is ascending, so each tree's leaves are)
    s.n_trees = 0;
    for (uint32_t h = 0; h < 64; ++h)
        if (est >> h & 1) {
            if (s.trees.size() == s.n_trees) s.trees.emplace_back();
            Tree& t = s.trees[s.n_trees++];
            t.height = h;
            t.leaves.clear();
        }
    s.chunk_tree.clear();
    s.chunk_leaf.clear();
    for (uint64_t ci : s.inactive) {
        uint32_t h;
        uint64_t node;
        locate(ci, est, &h, &node);
        const size_t t = (size_t)__builtin_popcountll(est & ((1ull << h) - 1));
        s.chunk_tree.push_back((uint32_t)t);
        s.chunk_leaf.push_back((uint32_t)s.trees[t].leaves.size());
        s.trees[t].leaves.push_back(node - (1ull << h));
    }
    // 3: the sorted lengths; then convert_to_vec's assert: structure k fits the k-th tree by ascending height
    s.want.clear();
    s.got.clear();
    for (size_t t = 0; t < s.n_trees; ++t) {
        ms_auth_structure_nodes(s.trees[t].height, s.trees[t].leaves, &s.trees[t].structure);
        s.want.push_back(s.trees[t].structure.size());
        s.got.push_back((size_t)(ch.path_off[s.structs[t] + 1] - ch.path_off[s.structs[t]]));
    }
    bool per_tree = s.want == s.got;
    if (!per_tree) {
        std::vector<size_t> a = s.want, b = s.got;
        std::sort(a.begin(), a.end());
        std::sort(b.begin(), b.end());
        if (a != b) return NHIP_MS_UNPACK_STRUCTURE_LENGTH;
        return NHIP_MS_UNPACK_PANIC;
    }
    return NHIP_MS_OK;
}

// convert_to_vec for a job that passed decide(): appends the job's program and its records' shape
int emit(const MsPackedIn& in, size_t j, Scratch& s, uint64_t swbfi, MsUnpackPlan* p, uint8_t* status) {
    const nhip_ms_chunks& ch = *in.chunks;
    MsUnpackJob& jb = p->jobs[j - s.j0];
    const uint64_t slot0 = p->n_slots;
    uint64_t next = slot0;
    jb.slot_off = slot0;
    jb.leaf_off = p->leaf_slot.size();
    jb.copy_off = p->copy_slot.size();
    jb.lvl_off = p->lvl.size();
    jb.gath_off = p->gath_src.size();
    // leaves: the k-th smallest inactive chunk index owns the k-th chunk of the dictionaries
    uint32_t levels = 0;
    for (size_t ti = 0; ti < s.n_trees; ++ti) {
        Tree& t = s.trees[ti];
        if (t.known.size() < (size_t)t.height + 1) t.known.resize((size_t)t.height + 1);
        for (uint32_t k = 0; k <= t.height; ++k) t.known[k].clear();
        levels = std::max(levels, t.height);
    }
    s.unpacked.clear();
    s.unpacked_off.assign(1, 0);
    for (size_t k = 0; k < s.inactive.size(); ++k) {
        Tree& t = s.trees[s.chunk_tree[k]];
        const uint64_t slot = next++;
        t.known[0].emplace_back(t.leaves[s.chunk_leaf[k]] + (1ull << t.height), (uint32_t)slot);
        p->leaf_slot.push_back((uint32_t)slot);
        p->leaf_cnt.push_back(s.chunk_n[k]);
        p->leaf_words.push_back(ch.rel_off[s.chunks[k]]);
        const uint32_t* words = ch.rel + ch.rel_off[s.chunks[k]];
        for (uint32_t i = 0; i < s.chunk_n[k]; ++i) s.unpacked.push_back(ms_packed_field(words, i));
        s.unpacked_off.push_back(s.unpacked.size());
    }
    // the structures: node indices from the tree's leaves (decide()), digests in the structure's order
    for (size_t ti = 0; ti < s.n_trees; ++ti) {
        Tree& t = s.trees[ti];
        const uint64_t src = ch.path_off[s.structs[ti]];
        for (size_t q = 0; q < t.structure.size(); ++q) {
            const uint64_t node = t.structure[q];
            const uint32_t depth = 63u - (uint32_t)__builtin_clzll(node);
            const uint64_t slot = next++;
            t.known[t.height - depth].emplace_back(node, (uint32_t)slot);
            p->copy_slot.push_back((uint32_t)slot);
            p->copy_src.push_back(src + q);
        }
        for (uint32_t k = 0; k <= t.height; ++k) std::sort(t.known[k].begin(), t.known[k].end());
    }
    // complete families to the fixpoint: a parent k levels up needs given nodes and parents of level k - 1 only,
    // and a parent that is present is never recomputed
    if (s.level_ops.size() < levels) s.level_ops.resize(levels);
    for (uint32_t k = 0; k < levels; ++k) s.level_ops[k].clear();
    for (size_t ti = 0; ti < s.n_trees; ++ti) {
        Tree& t = s.trees[ti];
        for (uint32_t k = 0; k < t.height; ++k) {
            const Level& lv = t.known[k];
            Level& up = t.known[k + 1];
            const size_t given = up.size();
            for (size_t i = 0; i + 1 < lv.size(); ++i) {
                if (lv[i].first != (lv[i + 1].first ^ 1) || (lv[i].first & 1)) continue;
                const uint64_t parent = lv[i].first >> 1;
                if (given) {
                    auto end = up.begin() + (ptrdiff_t)given;
                    auto it = std::lower_bound(up.begin(), end, std::make_pair(parent, (uint32_t)0));
                    if (it != end && it->first == parent) continue;
                }
                const uint64_t slot = next++;
                up.emplace_back(parent, (uint32_t)slot);
                std::vector<uint32_t>& ops = s.level_ops[k];
                ops.push_back((uint32_t)slot);
                ops.push_back(lv[i].second);
                ops.push_back(lv[i + 1].second);
            }
            if (up.size() != given && given) std::sort(up.begin(), up.end());  // the parents alone are ascending
        }
    }
    if (next > (uint64_t)NO_SLOT) return NHIP_ERR_OOM;
    while (levels && s.level_ops[levels - 1].empty()) --levels;
    for (uint32_t k = 0; k < levels; ++k) {
        p->lvl.push_back(p->op.size() / 3);
        p->op.insert(p->op.end(), s.level_ops[k].begin(), s.level_ops[k].end());
    }
    p->lvl.push_back(p->op.size() / 3);
    // every leaf's path, read by walking the siblings up to node 1: per level one merge over the tree's leaves
    // (ascending, so their ancestors and the places of their siblings in the level's nodes are too)
    bool panic = false;
    for (size_t ti = 0; ti < s.n_trees; ++ti) {
        Tree& t = s.trees[ti];
        const size_t L = t.leaves.size();
        t.path.assign(L * t.height, NO_SLOT);
        for (uint32_t lvl = 0; lvl < t.height; ++lvl) {
            const Level& lv = t.known[lvl];
            size_t at = 0;
            for (size_t i = 0; i < L; ++i) {
                const uint64_t sib = ((t.leaves[i] + (1ull << t.height)) >> lvl) ^ 1;
                while (at < lv.size() && lv[at].first < (sib & ~1ull)) ++at;
                size_t q = at;
                while (q < lv.size() && lv[q].first < sib) ++q;  // at most one step
                if (q < lv.size() && lv[q].first == sib) t.path[i * t.height + lvl] = lv[q].second;
                else panic = true;  // the reference's "must live in sparse mmr dictionary"
            }
        }
    }
    // the records: sorted distinct inactive chunk indices
    const size_t entries_before = p->chunk_index.size(), gath_before = p->gath_src.size(), rel_before = p->rel.size();
    const uint64_t r0 = in.rec_off[j], r1 = in.rec_off[j + 1];
    for (uint64_t r = r0; r < r1 && !panic; ++r) {
        s.rec_ci.assign(s.all_ci.begin() + (ptrdiff_t)(45 * (r - r0)), s.all_ci.begin() + (ptrdiff_t)(45 * (r - r0 + 1)));
        std::sort(s.rec_ci.begin(), s.rec_ci.end());
        s.rec_ci.erase(std::unique(s.rec_ci.begin(), s.rec_ci.end()), s.rec_ci.end());
        for (uint64_t ci : s.rec_ci) {
            if (ci >= swbfi) break;
            const size_t k = (size_t)(std::lower_bound(s.inactive.begin(), s.inactive.end(), ci) - s.inactive.begin());
            const Tree& t = s.trees[s.chunk_tree[k]];
            const uint32_t* path = t.path.data() + (size_t)s.chunk_leaf[k] * t.height;
            p->gath_src.insert(p->gath_src.end(), path, path + t.height);
            p->chunk_index.push_back(ci);
            p->path_off.push_back(p->gath_src.size());
            p->rel.insert(p->rel.end(), s.unpacked.begin() + (ptrdiff_t)s.unpacked_off[k],
                          s.unpacked.begin() + (ptrdiff_t)s.unpacked_off[k + 1]);
            p->rel_off.push_back(p->rel.size());
        }
        p->entry_off[r - s.rb + 1] = p->chunk_index.size();
    }
    if (panic) {  // fail closed: the job's records own no entry and it runs no program
        p->chunk_index.resize(entries_before);
        p->path_off.resize(entries_before + 1);
        p->rel_off.resize(entries_before + 1);
        p->gath_src.resize(gath_before);
        p->rel.resize(rel_before);
        p->leaf_slot.resize((size_t)jb.leaf_off);
        p->leaf_cnt.resize((size_t)jb.leaf_off);
        p->leaf_words.resize((size_t)jb.leaf_off);
        p->copy_slot.resize((size_t)jb.copy_off);
        p->copy_src.resize((size_t)jb.copy_off);
        p->op.resize((size_t)p->lvl[(size_t)jb.lvl_off] * 3);
        p->lvl.resize((size_t)jb.lvl_off + 1);
        for (uint64_t r = r0; r < r1; ++r) p->entry_off[r - s.rb + 1] = entries_before;
        *status = NHIP_MS_UNPACK_PANIC;
        jb.n_levels = 0;
        return NHIP_OK;
    }
    jb.n_slots = next - slot0;
    jb.n_leaf = p->leaf_slot.size() - jb.leaf_off;
    jb.n_copy = p->copy_slot.size() - jb.copy_off;
    jb.n_levels = levels;
    jb.n_gath = p->gath_src.size() - jb.gath_off;
    p->n_slots = next;
    p->max_levels = std::max(p->max_levels, levels);
    return NHIP_OK;
}

}  // namespace

namespace {

// the jobs j0 .. j1 into *p, every offset counted from the range's own start
int plan_range(const MsPackedIn& in, size_t j0, size_t j1, MsUnpackPlan* p) {
    *p = MsUnpackPlan{};
    Scratch s;
    s.j0 = j0;
    s.rb = j1 > j0 ? in.rec_off[j0] : 0;
    const size_t n = j1 - j0, R = j1 > j0 ? (size_t)(in.rec_off[j1] - s.rb) : 0;
    p->status.assign(n, NHIP_MS_OK);
    p->num_leafs_aocl.assign(n, 0);
    p->jobs.assign(n, MsUnpackJob{});
    p->entry_off.assign(R + 1, 0);
    p->path_off.assign(1, 0);
    p->rel_off.assign(1, 0);
    for (size_t j = j0; j < j1; ++j) {
        uint64_t swbfi = 0;
        const uint64_t r0 = in.rec_off[j], r1 = in.rec_off[j + 1];
        uint8_t st = r1 > r0 ? decide(in, j, s, &swbfi) : (uint8_t)NHIP_MS_OK;  // no record: N = 1, nothing to do
        MsUnpackJob& jb = p->jobs[j - j0];
        jb.slot_off = p->n_slots;
        jb.leaf_off = p->leaf_slot.size();
        jb.copy_off = p->copy_slot.size();
        jb.lvl_off = p->lvl.size();
        jb.gath_off = p->gath_src.size();
        if (st == NHIP_MS_OK && r1 > r0) {
            const int rc = emit(in, j, s, swbfi, p, &st);
            if (rc != NHIP_OK) return rc;
        } else {
            p->lvl.push_back(p->op.size() / 3);
            for (uint64_t r = r0; r < r1; ++r) p->entry_off[r - s.rb + 1] = p->chunk_index.size();
        }
        p->status[j - j0] = st;
        p->num_leafs_aocl[j - j0] = st == NHIP_MS_OK ? 8 * swbfi + 1 : 0;
    }
    return NHIP_OK;
}

template <class T>
void append_plus(std::vector<T>& dst, const std::vector<T>& src, size_t from, T base) {
    const size_t at = dst.size();
    dst.resize(at + (src.size() - from));
    for (size_t i = from; i < src.size(); ++i) dst[at + i - from] = src[i] + base;
}

// q, planned for the jobs after those of *p, onto the end of *p
void append_plan(MsUnpackPlan* p, const MsUnpackPlan& q) {
    const uint64_t slots = p->n_slots, leafs = p->leaf_slot.size(), copies = p->copy_slot.size(), ops = p->op.size() / 3,
                   lvls = p->lvl.size(), gath = p->gath_src.size(), entries = p->chunk_index.size(), rel = p->rel.size();
    p->status.insert(p->status.end(), q.status.begin(), q.status.end());
    p->num_leafs_aocl.insert(p->num_leafs_aocl.end(), q.num_leafs_aocl.begin(), q.num_leafs_aocl.end());
    for (MsUnpackJob jb : q.jobs) {
        jb.slot_off += slots;
        jb.leaf_off += leafs;
        jb.copy_off += copies;
        jb.lvl_off += lvls;
        jb.gath_off += gath;
        p->jobs.push_back(jb);
    }
    append_plus(p->entry_off, q.entry_off, 1, entries);
    append_plus(p->chunk_index, q.chunk_index, 0, (uint64_t)0);
    append_plus(p->path_off, q.path_off, 1, gath);
    append_plus(p->rel_off, q.rel_off, 1, rel);
    append_plus(p->rel, q.rel, 0, (uint32_t)0);
    append_plus(p->leaf_slot, q.leaf_slot, 0, (uint32_t)slots);
    append_plus(p->leaf_cnt, q.leaf_cnt, 0, (uint32_t)0);
    append_plus(p->leaf_words, q.leaf_words, 0, (uint64_t)0);
    append_plus(p->copy_slot, q.copy_slot, 0, (uint32_t)slots);
    append_plus(p->copy_src, q.copy_src, 0, (uint64_t)0);
    append_plus(p->op, q.op, 0, (uint32_t)slots);
    append_plus(p->lvl, q.lvl, 0, ops);
    append_plus(p->gath_src, q.gath_src, 0, (uint32_t)slots);
    p->n_slots += q.n_slots;
    p->max_levels = std::max(p->max_levels, q.max_levels);
}

}  // namespace

// The jobs are independent: ranges of them are planned on up to 8 host threads (at least 4 jobs each) and the
// ranges' plans joined in job order, which gives the plan one thread would write.
int ms_unpack_plan(const MsPackedIn& in, const MsUnpackCounts& counts, MsUnpackPlan* p) {
    const size_t n = in.n_jobs;
    const nhip_ms_chunks none{};
    MsPackedIn use = in;
    if (counts.records == 0) use.chunks = &none;
    const size_t T = std::min<size_t>(8, (n + 3) / 4);
    if (T <= 1) return plan_range(use, 0, n, p);
    std::vector<MsUnpackPlan> parts(T);
    std::vector<int> rc(T, NHIP_OK);
    std::vector<std::thread> threads;
    auto work = [&](size_t t) {
        try {
            rc[t] = plan_range(use, n * t / T, n * (t + 1) / T, &parts[t]);
        } catch (const std::bad_alloc&) {
            rc[t] = NHIP_ERR_OOM;
        }
    };
    try {
        for (size_t t = 1; t < T; ++t) threads.emplace_back(work, t);
    } catch (...) {  // no thread to be had: the rest on this one
        for (size_t t = threads.size() + 1; t < T; ++t) work(t);
    }
    work(0);
    for (std::thread& th : threads) th.join();
    for (size_t t = 0; t < T; ++t)
        if (rc[t] != NHIP_OK) return rc[t];
    *p = std::move(parts[0]);
    for (size_t t = 1; t < T; ++t) {
        if (p->n_slots + parts[t].n_slots > (uint64_t)NO_SLOT) return NHIP_ERR_OOM;
        append_plan(p, parts[t]);
        parts[t] = MsUnpackPlan{};
    }
    return NHIP_OK;
}

bool ms_unpacked_is_count_pass(const nhip_ms_unpacked* out) {
    return !out->entry_off && !out->chunk_index && !out->path_off && !out->path && !out->rel_off && !out->rel;
}

int ms_unpacked_write(const MsUnpackPlan& plan, size_t n_jobs, bool need_path, nhip_ms_unpacked* out) {
    const size_t E = plan.chunk_index.size(), PD = plan.gath_src.size(), W = plan.rel.size();
    const bool count = ms_unpacked_is_count_pass(out);
    if (!count) {
        if (!out->status && n_jobs) return NHIP_ERR_ARG;
        if (!out->entry_off || !out->path_off || !out->rel_off) return NHIP_ERR_ARG;
        if (out->entries_cap < E || out->path_cap < PD || out->rel_cap < W) return NHIP_ERR_ARG;
        if ((E && !out->chunk_index) || (W && !out->rel) || (need_path && PD && !out->path)) return NHIP_ERR_ARG;
        std::copy(plan.entry_off.begin(), plan.entry_off.end(), out->entry_off);
        std::copy(plan.chunk_index.begin(), plan.chunk_index.end(), out->chunk_index);
        std::copy(plan.path_off.begin(), plan.path_off.end(), out->path_off);
        std::copy(plan.rel_off.begin(), plan.rel_off.end(), out->rel_off);
        std::copy(plan.rel.begin(), plan.rel.end(), out->rel);
    }
    if (out->status) std::copy(plan.status.begin(), plan.status.end(), out->status);
    if (out->num_leafs_aocl) std::copy(plan.num_leafs_aocl.begin(), plan.num_leafs_aocl.end(), out->num_leafs_aocl);
    out->entries = E;
    out->path_digests = PD;
    out->rel_words = W;
    return NHIP_OK;
}

}  // namespace nhip

extern "C" int nhip_ms_unpack_plan(const uint64_t* rec_off, size_t n_jobs, const uint64_t* minimum,
                                   const uint32_t* distances, const nhip_ms_chunks* packed, nhip_ms_unpacked* out) {
    if (!out) return NHIP_ERR_ARG;
    const nhip::MsPackedIn in{rec_off, n_jobs, minimum, distances, packed};
    nhip::MsUnpackCounts cnt;
    if (nhip::ms_packed_ok(in, &cnt)) return NHIP_ERR_ARG;
    try {
        nhip::MsUnpackPlan plan;
        const int rc = nhip::ms_unpack_plan(in, cnt, &plan);
        if (rc != NHIP_OK) return rc;
        return nhip::ms_unpacked_write(plan, n_jobs, false, out);
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}
