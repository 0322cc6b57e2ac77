// ASan / UBSan harness for the in-place scanners (neptune-core_amd/csrc/bincode.cpp:
// nhip_wire_scan_txs, nhip_wire_scan_blocks) and the upload plan built from their spans
// (csrc/wire.hpp).  The scanners walk untrusted wire bytes (transfer_transaction.rs:31-47,
// import_blocks_from_files.rs:100-115) and hand out byte spans that are then DMA'd and read by a GPU
// kernel, so a span outside the buffer is a device fault waiting to happen.  Built by
// tests/native/wire.mk with -fsanitize=address,undefined (host only, nothing runs on a GPU) and driven
// by tests/test_wire_sanitizers.py: each input is scanned as given, at every truncation (spread for
// large inputs) and after seeded mutations, each time from the END of an exactly sized heap block, so a
// one-byte over-read is a sanitizer report.  Checked on every run: every returned span lies inside the
// buffer, counts are consistent, a resumed scan (small span_cap) finds the same spans as one pass, and
// the plan's runs cover every span inside a raw buffer of the stated size.
//
// usage: wire_scan_check <mutations per input> {txs|blk10}:<path> ...
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/neptune_hip.h"
#include "../../neptune-core_amd/csrc/wire.hpp"

namespace {

uint64_t g_state = 0x5EEDF00Dull;
uint64_t next_u64() {
    g_state += 0x9E3779B97F4A7C15ull;
    uint64_t z = g_state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

const uint64_t INTERESTING[] = {0, 1, 2, 3, 5, 7, 8, 11, 12, 80, 255, 256, 0xFFFF, 0x7FFFFFFF, 0xFFFFFFFF,
                                0x100000000ull, 0xFFFFFFFF00000000ull, 0xFFFFFFFF00000001ull, 0x7FFFFFFFFFFFFFFFull,
                                ~0ull};

uint64_t g_runs = 0, g_ok = 0, g_bad = 0;

void fail(const char* what) {
    std::fprintf(stderr, "wire_scan_check: %s\n", what);
    ++g_bad;
}

// the input at the end of a heap block of exactly its size
struct Tail {
    std::unique_ptr<uint8_t[]> mem;
    const uint8_t* p;
    size_t n;
    explicit Tail(const std::vector<uint8_t>& x) : mem(new uint8_t[x.size() ? x.size() : 1]), n(x.size()) {
        if (n) std::memcpy(mem.get(), x.data(), n);
        p = mem.get();
    }
};

bool inside(const nhip_span& s, size_t n) { return s.offset <= n && s.len <= (n - s.offset) / 8; }

void check_plan(const uint8_t* bytes, const std::vector<nhip_span>& spans, size_t n_bytes) {
    if (!nhip::wire_spans_ok(spans.data(), spans.size(), n_bytes)) return fail("scanner span fails wire_spans_ok");
    nhip::WirePlan plan;
    nhip::wire_plan(bytes, spans.data(), spans.size(), plan);
    uint64_t prev_end = 0;
    for (const nhip::WireRun& r : plan.runs) {
        if (r.start >= r.end || r.end > n_bytes) fail("run outside the buffer");
        if (r.pos < prev_end || r.pos + (r.end - r.start) + nhip::WIRE_TAIL_PAD > plan.raw_bytes) fail("run outside the raw buffer");
        if (((uintptr_t)(bytes + r.start) & 63u) != (r.pos & 63u)) fail("run not congruent mod 64");
        prev_end = r.pos + (r.end - r.start);
    }
    for (size_t i = 0; i < spans.size(); ++i) {
        if (!spans[i].len) continue;
        bool found = false;
        for (const nhip::WireRun& r : plan.runs)
            if (spans[i].offset >= r.start && spans[i].offset + 8 * spans[i].len <= r.end) {
                found = plan.boff[i] == r.pos + (spans[i].offset - r.start);
                break;
            }
        if (!found) fail("span not covered by a run at its offset");
    }
}

void run_txs(const std::vector<uint8_t>& x) {
    ++g_runs;
    const Tail t(x);
    const size_t cap = t.n / 8 + 1;
    std::vector<nhip_span> spans(cap);
    size_t ntx = 0, np = 0, used = 0;
    const int rc = nhip_wire_scan_txs(t.p, t.n, (size_t)-1, spans.data(), cap, &ntx, &np, &used);
    if (rc != NHIP_OK && rc != NHIP_ERR_DECODE) return fail("scan_txs: unexpected return code");
    if (np > cap || used > t.n || ntx > np) return fail("scan_txs: inconsistent counts");
    if (rc == NHIP_OK && used != t.n) return fail("scan_txs: ok without consuming the stream");
    spans.resize(np);
    for (const nhip_span& s : spans)
        if (!inside(s, used)) return fail("scan_txs: span outside the consumed bytes");
    check_plan(t.p, spans, t.n);
    // the same stream in pieces: span_cap 3 (a ProofCollection of more proofs: NHIP_ERR_ARG at its start)
    std::vector<nhip_span> again;
    size_t pos = 0;
    for (;;) {
        nhip_span few[3];
        size_t a = 0, b = 0, c = 0;
        const int r2 = nhip_wire_scan_txs(t.p + pos, t.n - pos, (size_t)-1, few, 3, &a, &b, &c);
        if (b > 3 || c > t.n - pos) return fail("scan_txs (resumed): inconsistent counts");
        for (size_t i = 0; i < b; ++i) again.push_back(nhip_span{few[i].offset + pos, few[i].len});
        pos += c;
        if (r2 == NHIP_ERR_ARG) {
            if (a != 0 || c != 0) return fail("scan_txs: NHIP_ERR_ARG after taking transactions");
            again.clear();  // a transaction of more than 3 proofs: this form cannot finish the stream
            break;
        }
        if (r2 == NHIP_OK && c == 0 && pos < t.n) return fail("scan_txs: ok, nothing consumed, bytes left");
        if (r2 != NHIP_OK || pos >= t.n) {
            if (r2 != rc) return fail("scan_txs (resumed): return code differs from one pass");
            if (again.size() != spans.size() || (np && std::memcmp(again.data(), spans.data(), np * sizeof(nhip_span))))
                return fail("scan_txs (resumed): spans differ from one pass");
            break;
        }
    }
    if (rc == NHIP_OK) ++g_ok;
}

void run_blk(const std::vector<uint8_t>& x, uint32_t height) {
    ++g_runs;
    const Tail t(x);
    const size_t cap = t.n / 8 + 1;
    std::vector<nhip_span> spans(cap);
    std::vector<uint64_t> block_of(cap);
    size_t np = 0, nb = 0;
    const int rc = nhip_wire_scan_blocks(t.p, t.n, height, spans.data(), block_of.data(), cap, &np, &nb);
    if (rc != NHIP_OK) {
        if (rc != NHIP_ERR_DECODE) fail("scan_blocks: unexpected return code");
        if (np != 0) fail("scan_blocks: spans returned from a failed file");
        return;
    }
    if (np > nb || np > cap) return fail("scan_blocks: inconsistent counts");
    spans.resize(np);
    for (size_t i = 0; i < np; ++i) {
        if (!inside(spans[i], t.n)) return fail("scan_blocks: span outside the buffer");
        if (block_of[i] >= nb || (i && block_of[i] <= block_of[i - 1])) return fail("scan_blocks: block_of out of order");
    }
    check_plan(t.p, spans, t.n);
    if (np) {
        size_t a = 0, b = 0;
        if (nhip_wire_scan_blocks(t.p, t.n, height, spans.data(), nullptr, np - 1, &a, &b) != NHIP_ERR_ARG)
            fail("scan_blocks: short span_cap accepted");
    }
    ++g_ok;
}

template <class F>
void fuzz(const std::vector<uint8_t>& in, size_t mutations, F&& run) {
    run(in);
    const size_t step = in.size() <= 4096 ? 1 : in.size() / 600;
    for (size_t len = 0; len < in.size(); len += step) run(std::vector<uint8_t>(in.begin(), in.begin() + len));
    for (size_t m = 0; m < mutations && !in.empty(); ++m) {
        std::vector<uint8_t> x(in);
        const uint64_t r = next_u64();
        const size_t k = 1 + (r & 3);  // 1..4 edits
        for (size_t e = 0; e < k; ++e) {
            const uint64_t q = next_u64();
            if ((q & 1) || x.size() < 8) {
                x[(q >> 8) % x.size()] ^= (uint8_t)(1u << ((q >> 4) & 7));
            } else {
                const size_t pos = ((q >> 8) % (x.size() / 4)) * 4;
                const uint64_t v = (q & 2) ? INTERESTING[(q >> 40) % (sizeof(INTERESTING) / 8)] : next_u64();
                std::memcpy(&x[pos], &v, (q & 4) && pos + 8 <= x.size() ? 8 : 4);
            }
        }
        if ((r >> 8) % 16 == 0) x.resize((r >> 16) % (x.size() + 1));  // also truncate some
        run(x);
    }
}

std::vector<uint8_t> read_file(const char* path) {
    std::vector<uint8_t> b;
    FILE* f = std::fopen(path, "rb");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", path);
        std::exit(2);
    }
    uint8_t buf[1 << 16];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + n);
    std::fclose(f);
    return b;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s <mutations> kind:path ...\n", argv[0]);
        return 2;
    }
    const size_t mutations = std::strtoull(argv[1], nullptr, 10);
    for (int a = 2; a < argc; ++a) {
        const std::string arg = argv[a];
        const size_t colon = arg.find(':');
        if (colon == std::string::npos) return 2;
        const std::string kind = arg.substr(0, colon);
        const std::vector<uint8_t> in = read_file(arg.c_str() + colon + 1);
        if (kind == "txs") fuzz(in, mutations, [&](const std::vector<uint8_t>& x) { run_txs(x); });
        else if (kind == "blk10") fuzz(in, mutations, [&](const std::vector<uint8_t>& x) { run_blk(x, 10); });
        else return 2;
    }
    std::printf("runs %llu ok %llu bad %llu\n", (unsigned long long)g_runs, (unsigned long long)g_ok,
                (unsigned long long)g_bad);
    return g_bad ? 1 : 0;
}
