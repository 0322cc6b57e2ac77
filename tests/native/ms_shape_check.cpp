// Host-side shape validator of the mutator-set entry points (csrc/ms_shape.cpp) under ASan + UBSan
// (tests/test_ms_ref.py): good and malformed CSR inputs, every array an exactly sized heap block so
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

struct Chunks {
    std::vector<uint64_t> entry_off, chunk_index, path_off, path, rel_off;
    std::vector<uint32_t> rel;
    nhip_ms_chunks view() const {
        nhip_ms_chunks c;
        c.entry_off = entry_off.empty() ? nullptr : entry_off.data();
        c.chunk_index = chunk_index.empty() ? nullptr : chunk_index.data();
        c.path_off = path_off.empty() ? nullptr : path_off.data();
        c.path = path.empty() ? nullptr : path.data();
        c.rel_off = rel_off.empty() ? nullptr : rel_off.data();
        c.rel = rel.empty() ? nullptr : rel.data();
        return c;
    }
};

// 3 records with 2, 0 and 1 entries; paths of 1, 0, 2 digests; chunks of 3, 0, 1 indices
Chunks sample() {
    Chunks c;
    c.entry_off = {0, 2, 2, 3};
    c.chunk_index = {5, 9, 1};
    c.path_off = {0, 1, 1, 3};
    c.path.assign(15, 7);
    c.rel_off = {0, 3, 3, 4};
    c.rel = {1, 2, 3, 4};
    return c;
}

}  // namespace

int main() {
    using namespace nhip;
    uint64_t total = 0;
    {
        const std::vector<uint64_t> off = {0, 0, 4, 4, 9};
        expect(ms_csr_ok(off.data(), 4, 8, &total), NHIP_OK, "csr good");
        if (total != 9) ++failures;
        const std::vector<uint64_t> one = {0};
        expect(ms_csr_ok(one.data(), 0, 8, &total), NHIP_OK, "csr n = 0");
        expect(ms_csr_ok(nullptr, 0, 8, &total), NHIP_ERR_ARG, "csr null");
        const std::vector<uint64_t> dec = {0, 5, 4, 9};
        expect(ms_csr_ok(dec.data(), 3, 8, &total), NHIP_ERR_ARG, "csr decreasing");
        const std::vector<uint64_t> base = {1, 2, 3};
        expect(ms_csr_ok(base.data(), 2, 8, &total), NHIP_ERR_ARG, "csr first offset not 0");
        const std::vector<uint64_t> huge = {0, ~0ull};
        expect(ms_csr_ok(huge.data(), 1, 40, &total), NHIP_ERR_ARG, "csr byte size overflows");
    }
    {
        const std::vector<uint64_t> peaks(10, 3);
        nhip_mmr m{peaks.data(), 2, 3};
        expect(ms_mmr_ok(&m), NHIP_OK, "mmr good");
        nhip_mmr empty{nullptr, 0, 0};
        expect(ms_mmr_ok(&empty), NHIP_OK, "mmr empty");
        nhip_mmr null_peaks{nullptr, 2, 3};
        expect(ms_mmr_ok(&null_peaks), NHIP_ERR_ARG, "mmr null peaks");
        expect(ms_mmr_ok(nullptr), NHIP_ERR_ARG, "mmr null");
        const std::vector<uint32_t> active = {4, 1, 9};
        nhip_msa a{m, empty, active.data(), 3};
        expect(ms_msa_ok(&a), NHIP_OK, "msa good");
        nhip_msa null_active{m, empty, nullptr, 3};
        expect(ms_msa_ok(&null_active), NHIP_ERR_ARG, "msa null active");
        nhip_msa bad_mmr{m, null_peaks, nullptr, 0};
        expect(ms_msa_ok(&bad_mmr), NHIP_ERR_ARG, "msa bad swbf");
        expect(ms_msa_ok(nullptr), NHIP_ERR_ARG, "msa null");
    }
    {
        const std::vector<uint64_t> off = {0, 2, 2, 3};
        const std::vector<uint64_t> path(15, 1);
        expect(ms_paths_ok(off.data(), path.data(), 3, &total), NHIP_OK, "paths good");
        if (total != 3) ++failures;
        expect(ms_paths_ok(off.data(), nullptr, 3, &total), NHIP_ERR_ARG, "paths null digests");
        const std::vector<uint64_t> none = {0, 0, 0};
        expect(ms_paths_ok(none.data(), nullptr, 2, &total), NHIP_OK, "paths all empty");
    }
    {
        MsChunkCounts cc;
        Chunks c = sample();
        nhip_ms_chunks v = c.view();
        expect(ms_chunks_ok(&v, 3, &cc), NHIP_OK, "chunks good");
        if (cc.entries != 3 || cc.path_digests != 3 || cc.rel_words != 4) ++failures;
        expect(ms_chunks_ok(nullptr, 3, &cc), NHIP_ERR_ARG, "chunks null");

        Chunks none;
        none.entry_off = {0, 0};
        none.path_off = {0};
        none.rel_off = {0};
        v = none.view();
        expect(ms_chunks_ok(&v, 1, &cc), NHIP_OK, "a record with zero entries");

        c = sample();
        c.entry_off = {0, 2, 1, 3};
        v = c.view();
        expect(ms_chunks_ok(&v, 3, &cc), NHIP_ERR_ARG, "entry_off decreasing");

        c = sample();
        c.path_off = {0, 2, 1, 3};
        v = c.view();
        expect(ms_chunks_ok(&v, 3, &cc), NHIP_ERR_ARG, "path_off decreasing");

        c = sample();
        c.rel_off = {0, 3, 2, 4};
        v = c.view();
        expect(ms_chunks_ok(&v, 3, &cc), NHIP_ERR_ARG, "rel_off decreasing");

        c = sample();
        c.path_off[0] = 1;
        v = c.view();
        expect(ms_chunks_ok(&v, 3, &cc), NHIP_ERR_ARG, "path_off does not start at 0");

        c = sample();
        c.chunk_index.clear();
        v = c.view();
        expect(ms_chunks_ok(&v, 3, &cc), NHIP_ERR_ARG, "chunk_index null");

        c = sample();
        c.path.clear();
        v = c.view();
        expect(ms_chunks_ok(&v, 3, &cc), NHIP_ERR_ARG, "path null");

        c = sample();
        c.rel.clear();
        v = c.view();
        expect(ms_chunks_ok(&v, 3, &cc), NHIP_ERR_ARG, "rel null");

        c = sample();
        c.path_off.clear();
        v = c.view();
        expect(ms_chunks_ok(&v, 3, &cc), NHIP_ERR_ARG, "path_off null");

        c = sample();
        c.rel_off.clear();
        v = c.view();
        expect(ms_chunks_ok(&v, 3, &cc), NHIP_ERR_ARG, "rel_off null");
    }
    std::printf("good %d bad %d\n", good, bad);
    return failures ? 1 : 0;
}
