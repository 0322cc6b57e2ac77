// Host-side shape validator of nhip_ms_apply_batch (csrc/ms_shape.cpp: ms_apply_ok) under ASan + UBSan
// (tests/test_ms_apply_ref.py): good and malformed job batches, every array an exactly sized heap block so
// that a read past the declared shapes is a sanitizer report.  Host only: links no HIP.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../neptune-core_amd/csrc/ms_shape.hpp"

namespace {

int good = 0, bad = 0, failures = 0;

void expect(int rc, int want, const char* what) {
    if (rc != want) {
        std::fprintf(stderr, "FAIL %s: got %d, want %d\n", what, rc, want);
        ++failures;
    }
    (want == NHIP_OK ? good : bad) += 1;
}

template <class T>
const T* ptr(const std::vector<T>& v) {
    return v.empty() ? nullptr : v.data();
}
template <class T>
T* ptr(std::vector<T>& v) {
    return v.empty() ? nullptr : v.data();
}

// 3 jobs: 2, 0, 1 additions; 1, 2, 0 records; windows of 3, 0, 2 indices
struct Batch {
    std::vector<uint64_t> aocl_peaks = std::vector<uint64_t>(10, 3), swbf_peaks = std::vector<uint64_t>(5, 4);
    std::vector<uint32_t> act0 = {9, 1, 4}, act2 = {7, 7};
    std::vector<nhip_msa> before, expected;
    std::vector<uint64_t> add_off = {0, 2, 2, 3}, additions = std::vector<uint64_t>(15, 1), rec_off = {0, 1, 3, 3};
    std::vector<uint64_t> minimum = std::vector<uint64_t>(6, 5);
    std::vector<uint32_t> distances = std::vector<uint32_t>(135, 2);
    std::vector<uint64_t> entry_off = {0, 2, 2, 3}, chunk_index = {5, 9, 1}, path_off = {0, 1, 1, 3},
                          path = std::vector<uint64_t>(15, 7), rel_off = {0, 3, 3, 4};
    std::vector<uint32_t> rel = {1, 2, 3, 4};
    nhip_ms_chunks chunks;
    std::vector<uint8_t> verdict = std::vector<uint8_t>(3), status = std::vector<uint8_t>(3);
    std::vector<uint64_t> bad_record = std::vector<uint64_t>(3);
    std::vector<uint64_t> o_aocl = std::vector<uint64_t>(3 * 320), o_swbf = std::vector<uint64_t>(3 * 320),
                          o_an = std::vector<uint64_t>(3), o_sn = std::vector<uint64_t>(3),
                          o_nact = std::vector<uint64_t>(3), active_off = {0, 48, 138, 140};
    std::vector<uint32_t> o_anp = std::vector<uint32_t>(3), o_snp = std::vector<uint32_t>(3),
                          o_active = std::vector<uint32_t>(140);
    bool with_expected = false, with_acc = true;

    nhip_ms_apply_in in() {
        const nhip_mmr a{ptr(aocl_peaks), 2, 3}, s{ptr(swbf_peaks), 1, 1}, none{nullptr, 0, 0};
        before = {nhip_msa{a, none, ptr(act0), act0.size()}, nhip_msa{a, s, nullptr, 0},
                  nhip_msa{none, s, ptr(act2), act2.size()}};
        expected = before;
        chunks = nhip_ms_chunks{ptr(entry_off), ptr(chunk_index), ptr(path_off), ptr(path), ptr(rel_off), ptr(rel)};
        return nhip_ms_apply_in{before.size(), ptr(before), ptr(add_off), ptr(additions), ptr(rec_off), ptr(minimum),
                                ptr(distances), &chunks, with_expected ? ptr(expected) : nullptr};
    }
    nhip_ms_apply_out out() {
        nhip_ms_apply_out o{};
        o.verdict = ptr(verdict);
        o.status = ptr(status);
        o.bad_record = ptr(bad_record);
        if (with_acc) {
            o.aocl_peaks = ptr(o_aocl);
            o.aocl_n_peaks = ptr(o_anp);
            o.aocl_num_leafs = ptr(o_an);
            o.swbf_peaks = ptr(o_swbf);
            o.swbf_n_peaks = ptr(o_snp);
            o.swbf_num_leafs = ptr(o_sn);
            o.active_off = ptr(active_off);
            o.active = ptr(o_active);
            o.n_active = ptr(o_nact);
        }
        return o;
    }
};

int check(Batch& b, nhip::MsApplyCounts* c = nullptr) {
    const nhip_ms_apply_in in = b.in();
    const nhip_ms_apply_out out = b.out();
    return nhip::ms_apply_ok(&in, &out, c);
}

}  // namespace

int main() {
    using namespace nhip;
    {
        Batch b;
        MsApplyCounts c;
        expect(check(b, &c), NHIP_OK, "good");
        if (c.additions != 3 || c.records != 3 || c.window_cap != 140 || !c.accumulators || c.chunks.entries != 3) ++failures;
        b.with_expected = true;
        expect(check(b), NHIP_OK, "good with expected");
        b.with_acc = false;
        expect(check(b, &c), NHIP_OK, "good without the accumulators after");
        if (c.accumulators) ++failures;
    }
    {
        Batch b;
        nhip_ms_apply_in in = b.in();
        nhip_ms_apply_out out = b.out();
        expect(ms_apply_ok(nullptr, &out, nullptr), NHIP_ERR_ARG, "in null");
        expect(ms_apply_ok(&in, nullptr, nullptr), NHIP_ERR_ARG, "out null");
        in.n_jobs = 0;
        in.msa_before = nullptr;
        in.add_off = in.rec_off = nullptr;
        nhip_ms_apply_out none{};
        expect(ms_apply_ok(&in, &none, nullptr), NHIP_OK, "no jobs");
    }
    {  // a job batch with no record at all: the record arrays and the dictionaries may be absent
        Batch b;
        b.rec_off = {0, 0, 0, 0};
        b.minimum.clear();
        b.distances.clear();
        b.active_off = {0, 3, 3, 5};
        b.o_active.resize(5);
        nhip_ms_apply_in in = b.in();
        in.chunks = nullptr;
        const nhip_ms_apply_out out = b.out();
        expect(ms_apply_ok(&in, &out, nullptr), NHIP_OK, "no records, chunks null");
    }
    struct Case {
        const char* what;
        void (*mutate)(Batch&);
    };
    const Case cases[] = {
        {"add_off decreasing", [](Batch& b) { b.add_off = {0, 2, 1, 3}; }},
        {"add_off does not start at 0", [](Batch& b) { b.add_off = {1, 2, 2, 3}; }},
        {"add_off null", [](Batch& b) { b.add_off.clear(); }},
        {"additions null", [](Batch& b) { b.additions.clear(); }},
        {"rec_off decreasing", [](Batch& b) { b.rec_off = {0, 3, 1, 3}; }},
        {"rec_off null", [](Batch& b) { b.rec_off.clear(); }},
        {"minimum null", [](Batch& b) { b.minimum.clear(); }},
        {"distances null", [](Batch& b) { b.distances.clear(); }},
        {"entry_off decreasing", [](Batch& b) { b.entry_off = {0, 2, 1, 3}; }},
        {"rel null", [](Batch& b) { b.rel.clear(); }},
        {"verdict null", [](Batch& b) { b.verdict.clear(); }},
        {"status null", [](Batch& b) { b.status.clear(); }},
        {"bad_record null", [](Batch& b) { b.bad_record.clear(); }},
        {"one accumulator output missing", [](Batch& b) { b.o_sn.clear(); }},
        {"active_off missing", [](Batch& b) { b.active_off.clear(); }},
        {"active_off decreasing", [](Batch& b) { b.active_off = {0, 138, 48, 140}; }},
        {"window capacity one short (first job)", [](Batch& b) { b.active_off = {0, 47, 138, 140}; }},
        {"window capacity one short (records only)", [](Batch& b) { b.active_off = {0, 48, 137, 140}; }},
        {"window capacity one short (window only)", [](Batch& b) { b.active_off = {0, 48, 138, 139}; b.o_active.resize(139); }},
        {"window storage null", [](Batch& b) { b.o_active.clear(); }},
    };
    for (const Case& cs : cases) {
        Batch b;
        cs.mutate(b);
        expect(check(b), NHIP_ERR_ARG, cs.what);
    }
    {
        Batch b;
        nhip_ms_apply_in in = b.in();
        const nhip_ms_apply_out out = b.out();
        in.msa_before = nullptr;
        expect(ms_apply_ok(&in, &out, nullptr), NHIP_ERR_ARG, "msa_before null");
        in = b.in();
        b.before[0].active = nullptr;
        expect(ms_apply_ok(&in, &out, nullptr), NHIP_ERR_ARG, "a window null with n_active 3");
        in = b.in();
        b.before[1].swbf_inactive.peaks = nullptr;
        expect(ms_apply_ok(&in, &out, nullptr), NHIP_ERR_ARG, "peaks null with n_peaks 1");
        b.with_expected = true;
        in = b.in();
        b.expected[2].active = nullptr;
        expect(ms_apply_ok(&in, &out, nullptr), NHIP_ERR_ARG, "an expected window null with n_active 2");
        in = b.in();
        in.chunks = nullptr;
        expect(ms_apply_ok(&in, &out, nullptr), NHIP_ERR_ARG, "chunks null with records");
    }
    std::printf("good %d bad %d\n", good, bad);
    return failures ? 1 : 0;
}
