// The workspace layout of the host-buffer C ABI calls (csrc/stage_layout.hpp) under ASan + UBSan
// (tests/test_stage_layout.py): alignment, order, empty buffers, overflow, and for every staged entry point
// the offsets of its declarations (count, per, element size, as csrc/capi.hip and csrc/ms_capi.hip make them)
// against the plain arithmetic over its byte sizes that the calls used before.  Host only: links no HIP.
#include <cstdio>
#include <vector>

#include "../../neptune-core_amd/csrc/ms_shape.hpp"
#include "../../neptune-core_amd/csrc/stage_layout.hpp"

namespace {

int checks = 0, failures = 0;

void expect(bool ok, const char* what, const char* detail = "") {
    ++checks;
    if (!ok) {
        std::fprintf(stderr, "FAIL %s %s\n", what, detail);
        ++failures;
    }
}

struct Decl {
    size_t count, per, elem;
};

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// the declarations laid out by StageLayout against sizes[] laid out the plain way
void same_layout(const char* what, const std::vector<Decl>& decls, const std::vector<size_t>& sizes) {
    nhip::StageLayout lay;
    std::vector<unsigned> slots;
    for (const Decl& d : decls) slots.push_back(lay.add(d.count, d.per, d.elem));
    expect(!lay.overflow && lay.n == sizes.size() && decls.size() == sizes.size(), what, "count");
    size_t off = 0;
    for (size_t i = 0; i < sizes.size() && i < lay.n; ++i) {
        expect(slots[i] == i, what, "slot order");
        expect(lay.off[i] == off && lay.bytes[i] == sizes[i], what, "offset / bytes");
        expect(lay.off[i] % 256 == 0 && (i == 0 || lay.off[i] > lay.off[i - 1]), what, "aligned, increasing");
        off += align_up(sizes[i] ? sizes[i] : 1);
    }
    expect(lay.total == off, what, "total");
}

struct MsShape {
    size_t n, E, pd, rel, aocl_np, swbf_np, active, apd;
};
struct ApplyShape {
    size_t n, peaks, active, additions, R, E, pd, rel, grp, exp_active, dig, grp_total, win;
};

}  // namespace

int main() {
    using nhip::StageLayout;
    {  // the rules, one by one
        StageLayout lay;
        expect(lay.add(1, 1, 1) == 0 && lay.add(0, 5, 8) == 1 && lay.add(257, 1, 1) == 2 && lay.add(32, 1, 8) == 3, "rules",
               "slots");
        expect(lay.off[0] == 0 && lay.off[1] == 256 && lay.off[2] == 512 && lay.off[3] == 1024, "rules", "offsets");
        expect(lay.bytes[1] == 0 && lay.off[2] - lay.off[1] == 256, "rules", "a zero-byte buffer has its own unit");
        expect(lay.total == 256 + 256 + 512 + 256 && !lay.overflow && lay.n == 4, "rules", "total");
    }
    {  // overflow is reported, not wrapped
        StageLayout a;
        a.add(SIZE_MAX / 8 + 1, 1, 8);
        expect(a.overflow, "overflow", "count * sizeof(T)");
        StageLayout b;
        b.add(SIZE_MAX / 2 + 1, 1, 1);
        expect(!b.overflow, "overflow", "one buffer of SIZE_MAX / 2 + 1 bytes fits");
        b.add(SIZE_MAX / 2 + 1, 1, 1);
        expect(b.overflow, "overflow", "the sum of two buffers of SIZE_MAX / 2 + 1 bytes");
        StageLayout c;
        c.add(SIZE_MAX / 4, 5, 1);
        expect(c.overflow, "overflow", "count * per");
        StageLayout d;
        d.add(SIZE_MAX - 100, 1, 1);
        expect(d.overflow, "overflow", "rounding up to the unit");
        StageLayout e;
        for (unsigned i = 0; i < nhip::STAGE_MAX_BUFS; ++i) e.add(1, 1, 1);
        expect(!e.overflow && e.n == nhip::STAGE_MAX_BUFS, "overflow", "STAGE_MAX_BUFS buffers fit");
        e.add(1, 1, 1);
        expect(e.overflow && e.n == nhip::STAGE_MAX_BUFS, "overflow", "one buffer too many");
        StageLayout f;
        f.add(3, 1, 4);
        f.add(SIZE_MAX, 2, 1);
        f.add(1, 1, 1);
        expect(f.overflow, "overflow", "sticks");
    }
    // every staged entry point at its smallest non-empty shape and at one with several empty buffers
    for (const size_t n : {(size_t)1, (size_t)70000}) {
        same_layout("nhip_tip5_permutation", {{n, 16, 8}}, {n * 16 * 8});
        same_layout("nhip_tip5_hash_pair", {{n, 5, 8}, {n, 5, 8}, {n, 5, 8}}, {n * 40, n * 40, n * 40});
    }
    for (const size_t n : {(size_t)2, (size_t)1024})
        same_layout("nhip_mtree_build", {{n, 5, 8}, {n, 5, 8}}, {n * 40, n * 40});
    for (const size_t total : {(size_t)1, (size_t)0}) {  // hash_varlen / mast: all sequences empty
        const size_t n = 3, fields = 5, nl = n * fields;
        same_layout("nhip_tip5_hash_varlen", {{total, 1, 8}, {n + 1, 1, 8}, {n, 5, 8}}, {total * 8, (n + 1) * 8, n * 40});
        same_layout("nhip_mast_hash_batch", {{total, 1, 8}, {nl + 1, 1, 8}, {nl, 5, 8}, {n, 5, 8}},
                    {total * 8, (nl + 1) * 8, nl * 40, n * 40});
    }
    for (const size_t depth : {(size_t)1, (size_t)0}) {  // mtree_verify: no path
        const size_t n = 3, n_roots = depth ? n : 1;
        same_layout("nhip_mtree_verify", {{n_roots, 5, 8}, {n, 1, 8}, {n, 5, 8}, {n, depth * 5, 8}, {n, 1, 1}},
                    {n_roots * 40, n * 8, n * 40, n * depth * 40, n});
    }
    for (const size_t raw : {(size_t)17, (size_t)0}) {
        const size_t n = 1, total = raw / 8, proof_in = 40;  // sizeof(nhip::ProofIn): 3 x u64, 4 x u32
        same_layout("nhip_le_words_gpu", {{raw, 1, 1}, {n, 1, 8}, {n, 1, proof_in}, {total, 1, 8}},
                    {raw, n * 8, n * proof_in, total * 8});
    }
    for (const size_t n : {(size_t)1, (size_t)7})
        same_layout("nhip_absolute_index_sets", {{n, 15, 8}, {n, 1, 8}, {n, 2, 8}, {n, 45, 4}},
                    {15 * n * 8, n * 8, 2 * n * 8, 45 * n * 4});
    for (const MsShape& s : {MsShape{1, 1, 1, 1, 1, 1, 1, 1}, MsShape{2, 0, 0, 0, 0, 0, 0, 0}}) {
        same_layout("nhip_mmr_verify_batch", {{s.aocl_np, 5, 8}, {s.n, 1, 8}, {s.n, 5, 8}, {s.n + 1, 1, 8}, {s.apd, 5, 8}, {s.n, 1, 1}},
                    {s.aocl_np * 40, s.n * 8, s.n * 40, (s.n + 1) * 8, s.apd * 40, s.n});
        same_layout("nhip_ms_can_remove_batch",
                    {{s.swbf_np, 5, 8}, {s.active, 1, 4}, {s.n, 2, 8}, {s.n, 45, 4}, {s.n + 1, 1, 8}, {s.E, 1, 8}, {s.E + 1, 1, 8},
                     {s.pd, 5, 8}, {s.E + 1, 1, 8}, {s.rel, 1, 4}, {s.E, 1, 1}, {s.n, 3, 1}},
                    {s.swbf_np * 40, s.active * 4, s.n * 16, s.n * 45 * 4, (s.n + 1) * 8, s.E * 8, (s.E + 1) * 8, s.pd * 40,
                     (s.E + 1) * 8, s.rel * 4, s.E, 3 * s.n});
        same_layout("nhip_ms_verify_batch",
                    {{s.aocl_np, 5, 8}, {s.swbf_np, 5, 8}, {s.active, 1, 4}, {s.n, 15, 8}, {s.n, 1, 8}, {s.n + 1, 1, 8}, {s.apd, 5, 8},
                     {s.n + 1, 1, 8}, {s.E, 1, 8}, {s.E + 1, 1, 8}, {s.pd, 5, 8}, {s.E + 1, 1, 8}, {s.rel, 1, 4}, {s.n, 2, 8},
                     {s.n, 45, 4}, {s.n, 1, 1}, {s.E, 1, 1}, {s.n, 2, 1}},
                    {s.aocl_np * 40, s.swbf_np * 40, s.active * 4, 15 * s.n * 8, s.n * 8, (s.n + 1) * 8, s.apd * 40, (s.n + 1) * 8,
                     s.E * 8, (s.E + 1) * 8, s.pd * 40, (s.E + 1) * 8, s.rel * 4, s.n * 16, s.n * 45 * 4, s.n, s.E, 2 * s.n});
    }
    // nhip_ms_apply_batch: one job with one record and one entry; three jobs without a record (R = 0)
    for (const ApplyShape& s : {ApplyShape{1, 10, 1, 1, 1, 1, 1, 1, 2, 1, 6, 1, 46}, ApplyShape{3, 0, 0, 2, 0, 0, 0, 0, 3, 0, 9, 0, 0}}) {
        const size_t n = s.n, R = s.R, E = s.E, job = sizeof(nhip::MsApplyJob);
        same_layout("nhip_ms_apply_batch",
                    {{n, 1, job}, {s.peaks, 1, 8}, {s.active, 1, 4}, {s.additions, 5, 8}, {R, 2, 8}, {R, 45, 4}, {R ? R + 1 : 0, 1, 8},
                     {E, 1, 8}, {R ? E + 1 : 0, 1, 8}, {s.pd, 5, 8}, {R ? E + 1 : 0, 1, 8}, {s.rel, 1, 4}, {R, 1, 4}, {E, 1, 4},
                     {R, 45, 4}, {s.grp, 1, 4}, {R, 1, 4}, {s.exp_active, 1, 4}, {E, 1, 1}, {R, 3, 1}, {R, 45, 1}, {s.dig, 5, 8},
                     {s.grp_total, 2, 8}, {n, 2, 1}, {n, 1, 8}, {2 * n, 64 * 5, 8}, {n, 2, 4}, {n, 3, 8}, {s.win, 1, 4}},
                    {n * job, s.peaks * 8, s.active * 4, s.additions * 40, R * 16, R * 45 * 4, R ? (R + 1) * 8 : 0, E * 8,
                     R ? (E + 1) * 8 : 0, s.pd * 40, R ? (E + 1) * 8 : 0, s.rel * 4, R * 4, E * 4, R * 45 * 4, s.grp * 4, R * 4,
                     s.exp_active * 4, E, 3 * R, 45 * R, s.dig * 40, s.grp_total * 16, 2 * n, n * 8, 2 * n * 64 * 40, 2 * n * 4,
                     3 * n * 8, s.win * 4});
    }
    expect(sizeof(nhip::MsApplyJob) == 21 * 8 + 4 * 4, "MsApplyJob", "size");
    std::printf("checks %d failures %d\n", checks, failures);
    return failures ? 1 : 0;
}
