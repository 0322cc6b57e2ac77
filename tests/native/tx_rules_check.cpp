// The consensus integers of a block's transaction rules and guesser-fee UTXOs (csrc/tx_rules.hpp) and the host walk
// behind nhip_blk_ms_walk (csrc/bincode.cpp, csrc/blk_ms_parts.cpp) under ASan + UBSan (tests/test_tx_rules.py).  The
// two-u64 i128 arithmetic against __int128, Block::block_subsidy against the reference's loop on __int128, rules
// 2.f-2.l against a naive restatement, the UTXO encodings against a generic length-prefix builder; the walk against
// the values a block was written from, and truncated at every byte of its kernel.  Host only: links no HIP.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <random>
#include <vector>

#include "../../neptune-core_amd/csrc/blk_ms_parts.hpp"
#include "../../neptune-core_amd/csrc/tx_rules.hpp"

namespace {

namespace T = nhip::txrules;
using i128 = __int128;
using u128 = unsigned __int128;
int checks = 0, failures = 0;

void expect(bool ok, const char* what) {
    ++checks;
    if (!ok) {
        std::fprintf(stderr, "FAIL %s\n", what);
        ++failures;
    }
}

T::I128 split(i128 v) { return T::I128{(uint64_t)(u128)v, (uint64_t)((u128)v >> 64)}; }
i128 join(T::I128 a) { return (i128)(((u128)a.hi << 64) | a.lo); }

i128 naive_subsidy(uint64_t height) {
    i128 reward = (i128)128 * 4;
    for (int k = 0; k < 30; ++k) reward *= 10;
    const u128 sum = (u128)height + 21310;
    const uint64_t generation = (uint64_t)((sum > (u128)UINT64_MAX ? (u128)UINT64_MAX : sum) / 160815);
    for (uint64_t g = 0; g < generation; ++g) {
        reward /= 2;
        if (reward == 0) return 0;
    }
    return reward;
}

char naive_rule(const T::TxLimits& lim, const T::TxFacts& t) {
    if (t.kernel_timestamp > t.header_timestamp) return 'f';
    if (t.has_coinbase) {
        if (join(t.coinbase) > naive_subsidy(t.header_height)) return 'g';
        if (join(t.coinbase) < 0) return 'h';
    }
    if (join(t.fee) < 0) return 'i';
    if (t.n_inputs > lim.max_num_inputs) return 'j';
    if (t.n_outputs > lim.max_num_outputs) return 'k';
    if (t.n_announcements > lim.max_num_announcements) return 'l';
    return 0;
}

// generic BFieldCodec pieces: [len] + words
std::vector<uint64_t> dyn(const std::vector<uint64_t>& w) {
    std::vector<uint64_t> r{(uint64_t)w.size()};
    r.insert(r.end(), w.begin(), w.end());
    return r;
}
void cat(std::vector<uint64_t>& a, const std::vector<uint64_t>& b) { a.insert(a.end(), b.begin(), b.end()); }
std::vector<uint64_t> coin(const uint64_t hash[5], const std::vector<uint64_t>& state) {
    std::vector<uint64_t> r = dyn(dyn(state));  // the field's prefix, then Vec = [len] + items
    r.insert(r.end(), hash, hash + 5);
    return r;
}
std::vector<uint64_t> utxo(const std::vector<std::vector<uint64_t>>& coins, const uint64_t lock[5]) {
    std::vector<uint64_t> vec{(uint64_t)coins.size()};
    for (const auto& c : coins) cat(vec, dyn(c));
    std::vector<uint64_t> r = dyn(vec);
    r.insert(r.end(), lock, lock + 5);
    return r;
}

void check_integers(std::mt19937_64& rng) {
    std::vector<i128> edge{0, 1, -1, 2, -2, 3, -3, (i128)1 << 64, -((i128)1 << 64), ((i128)1 << 64) - 1,
                           (i128)(((u128)1 << 127) - 1), (i128)((u128)1 << 127), naive_subsidy(0), naive_subsidy(0) + 1};
    for (int k = 0; k < 200; ++k) edge.push_back((i128)(((u128)rng() << 64) | rng()) >> (rng() % 128));
    for (i128 a : edge) {
        expect(join(split(a)) == a, "split/join");
        expect(join(T::half(split(a))) == a / 2, "half");
        expect(T::is_negative(split(a)) == (a < 0), "is_negative");
        expect(T::is_zero(split(a)) == (a == 0), "is_zero");
        for (i128 b : edge) {
            expect(T::greater(split(a), split(b)) == (a > b), "greater");
            expect(join(T::sub(split(a), split(b))) == (i128)((u128)a - (u128)b), "sub");
        }
        if (a >= 0) {
            T::I128 lo, un;
            T::guesser_split(split(a), lo, un);
            expect(join(lo) == a / 2 && join(un) == a - a / 2 && join(lo) + join(un) == a, "guesser_split");
        }
    }
    expect(join(T::initial_block_subsidy()) == naive_subsidy(0), "initial subsidy");
    const uint64_t first = 160815 - 21310;
    std::vector<uint64_t> heights{0, 1, first - 1, first, first + 1, first + 160815 - 1, first + 160815, T::P - 1, UINT64_MAX,
                                  UINT64_MAX - 21310, UINT64_MAX - 21309};
    for (uint64_t g = 100; g < 115; ++g) heights.push_back(first + g * 160815 - 1), heights.push_back(first + g * 160815);
    for (int k = 0; k < 200; ++k) heights.push_back(rng() >> (rng() % 64));
    for (uint64_t h : heights) expect(join(T::block_subsidy(h)) == naive_subsidy(h), "block_subsidy");
    expect(T::is_zero(T::block_subsidy(first + 110 * 160815)), "subsidy runs out");
    for (uint64_t ts : std::vector<uint64_t>{0, 1, T::P - 1, T::P - 94670208000ull, T::P - 94670208001ull, 1700000000000ull})
        expect(T::release_date(ts) == (uint64_t)(((u128)ts + 94670208000ull) % T::P), "release_date");
}

void check_rules(std::mt19937_64& rng) {
    const T::TxLimits lim{1 << 14, 1 << 14, 1 << 14};
    const i128 sub5 = naive_subsidy(5);
    const std::vector<i128> amounts{0, 1, -1, sub5, sub5 + 1, sub5 - 1, (i128)(((u128)1 << 127) - 1), (i128)((u128)1 << 127)};
    const std::vector<uint64_t> counts{0, (1 << 14) - 1, 1 << 14, (1 << 14) + 1, UINT64_MAX};
    for (uint64_t kt : std::vector<uint64_t>{999, 1000, 1001, T::P - 1})
        for (i128 fee : amounts)
            for (i128 cb : amounts)
                for (uint32_t has : {0u, 1u})
                    for (int which = 0; which < 3; ++which)
                        for (uint64_t cnt : counts) {
                            T::TxFacts t{5, 1000, kt, split(fee), split(cb), has, 0, 0, 0};
                            (which == 0 ? t.n_inputs : which == 1 ? t.n_outputs : t.n_announcements) = cnt;
                            expect(T::rules_2f_2l(lim, t) == naive_rule(lim, t), "rules_2f_2l");
                        }
    for (int k = 0; k < 2000; ++k) {
        T::TxFacts t{rng() >> (rng() % 64), rng() % T::P, rng() % T::P, split((i128)(((u128)rng() << 64) | rng()) >> (rng() % 128)),
                     split((i128)(((u128)rng() << 64) | rng()) >> (rng() % 128)), (uint32_t)(rng() & 1), rng() % 40000,
                     rng() % 40000, rng() % 40000};
        expect(T::rules_2f_2l(lim, t) == naive_rule(lim, t), "rules_2f_2l random");
    }
}

void check_encodings(std::mt19937_64& rng) {
    for (int k = 0; k < 50; ++k) {
        uint64_t nc[5], tl[5], lock[5];
        for (int q = 0; q < 5; ++q) nc[q] = rng() % T::P, tl[q] = rng() % T::P, lock[q] = rng() % T::P;
        const u128 amount = (((u128)rng() << 64) | rng()) >> (1 + rng() % 127);
        const uint64_t date = rng() % T::P;
        const std::vector<uint64_t> limbs{(uint64_t)(amount & 0xFFFFFFFFu), (uint64_t)((amount >> 32) & 0xFFFFFFFFu),
                                          (uint64_t)((amount >> 64) & 0xFFFFFFFFu), (uint64_t)(amount >> 96)};
        uint64_t w[T::UTXO_LOCKED_WORDS];
        int len = T::guesser_utxo_words(false, split((i128)amount), date, nc, tl, lock, w);
        std::vector<uint64_t> want = utxo({coin(nc, limbs)}, lock);
        expect(len == T::UTXO_UNLOCKED_WORDS && want.size() == 19 && std::vector<uint64_t>(w, w + len) == want, "unlocked utxo");
        len = T::guesser_utxo_words(true, split((i128)amount), date, nc, tl, lock, w);
        want = utxo({coin(nc, limbs), coin(tl, {date})}, lock);
        expect(len == T::UTXO_LOCKED_WORDS && want.size() == 28 && std::vector<uint64_t>(w, w + len) == want, "locked utxo");
    }
}

// ---- a block's bytes (bincode, as oracle/bincode_ref.py writes them)
struct Wr {
    std::vector<uint8_t> b;
    void le(uint64_t v, int k) {
        for (int i = 0; i < k; ++i) b.push_back((uint8_t)(v >> (8 * i)));
    }
    void digest(const uint64_t* d) {
        for (int q = 0; q < 5; ++q) le(d[q], 8);
    }
};

struct Sample {
    uint32_t h = 3;
    uint64_t height = 7, timestamp = 1234, receiver[5] = {1, 2, 3, 4, 5}, lock[5] = {6, 7, 8, 9, T::P - 1};
    std::vector<uint64_t> minimum;    // records x 2
    std::vector<uint32_t> distances;  // records x 45
    std::vector<std::vector<uint64_t>> keys;                    // per record: the entries' keys
    std::vector<std::vector<std::vector<uint64_t>>> paths;      // per entry: words of its digests
    std::vector<std::vector<std::vector<uint32_t>>> rels;
    std::vector<uint64_t> outputs;  // x 5
    std::vector<uint64_t> ann_lens;
    uint64_t fee[2] = {~0ull, ~0ull}, coinbase[2] = {77, 1};
    uint8_t tag = 1;
    uint64_t kernel_timestamp = 1200;
    uint64_t aocl_n = 11, swbf_n = 1;
    std::vector<uint64_t> aocl_peaks, swbf_peaks;
    std::vector<uint32_t> active;
    size_t kernel_begin = 0, kernel_end = 0;

    std::vector<uint8_t> bytes() {
        Wr w;
        const uint64_t zero[5] = {0, 0, 0, 0, 0};
        w.le(0, 8);
        w.le(height, 8);
        w.digest(zero);
        w.le(timestamp, 8);
        for (uint32_t k = 0; k < 2 * h + 2; ++k) w.digest(zero);
        for (int k = 0; k < 11; ++k) w.le(k, 4);
        w.digest(receiver);
        w.digest(lock);
        kernel_begin = w.b.size();
        w.le(minimum.size() / 2, 8);
        for (size_t r = 0; r < minimum.size() / 2; ++r) {
            w.le(minimum[2 * r], 8);
            w.le(minimum[2 * r + 1], 8);
            for (int k = 0; k < 45; ++k) w.le(distances[45 * r + k], 4);
            w.le(keys[r].size(), 8);
            for (size_t e = 0; e < keys[r].size(); ++e) {
                w.le(keys[r][e], 8);
                w.le(paths[r][e].size() / 5, 8);
                for (uint64_t x : paths[r][e]) w.le(x, 8);
                w.le(rels[r][e].size(), 8);
                for (uint32_t x : rels[r][e]) w.le(x, 4);
            }
        }
        w.le(outputs.size() / 5, 8);
        for (uint64_t x : outputs) w.le(x, 8);
        w.le(ann_lens.size(), 8);
        for (uint64_t n : ann_lens) {
            w.le(n, 8);
            for (uint64_t k = 0; k < n; ++k) w.le(k, 8);
        }
        w.le(fee[0], 8);
        w.le(fee[1], 8);
        w.le(tag, 1);
        if (tag) w.le(coinbase[0], 8), w.le(coinbase[1], 8);
        w.le(kernel_timestamp, 8);
        w.digest(zero);
        w.le(1, 1);
        kernel_end = w.b.size();
        w.le(aocl_n, 8);
        w.le(aocl_peaks.size() / 5, 8);
        for (uint64_t x : aocl_peaks) w.le(x, 8);
        w.le(swbf_n, 8);
        w.le(swbf_peaks.size() / 5, 8);
        for (uint64_t x : swbf_peaks) w.le(x, 8);
        w.le(active.size(), 8);
        for (uint32_t x : active) w.le(x, 4);
        for (int k = 0; k < 2; ++k) w.le(0, 8), w.le(0, 8);  // lock-free and block MMRs: empty
        w.le(0, 8);                                           // appendix
        w.le(0, 4);                                           // BlockProof::Genesis
        return w.b;
    }
};

Sample sample(std::mt19937_64& rng) {
    Sample s;
    for (int r = 0; r < 3; ++r) {
        s.minimum.push_back(rng());
        s.minimum.push_back(rng() >> 40);
        for (int k = 0; k < 45; ++k) s.distances.push_back((uint32_t)rng());
        s.keys.emplace_back();
        s.paths.emplace_back();
        s.rels.emplace_back();
        for (int e = 0; e < (r == 1 ? 0 : 2); ++e) {
            s.keys[r].push_back(e == 0 ? 2 : UINT64_MAX);
            std::vector<uint64_t> p;
            for (int k = 0; k < 5 * (e + 1); ++k) p.push_back(rng() % T::P);
            s.paths[r].push_back(p);
            s.rels[r].push_back(std::vector<uint32_t>{(uint32_t)rng(), 5u, 7u});
        }
    }
    for (int k = 0; k < 10; ++k) s.outputs.push_back(rng() % T::P);
    s.ann_lens = {0, 3, 1};
    for (int k = 0; k < 15; ++k) s.aocl_peaks.push_back(rng() % T::P);
    for (int k = 0; k < 5; ++k) s.swbf_peaks.push_back(rng() % T::P);
    s.active = {9, 8, 7, 4000};
    return s;
}

void check_walk(std::mt19937_64& rng) {
    Sample s = sample(rng);
    const std::vector<uint8_t> b = s.bytes();
    nhip::BlkMsParts p;
    expect(nhip::blk_ms_walk_block(b.data(), b.size(), s.h, 0, p) == NHIP_OK && p.n == 1, "walk");
    expect(p.height[0] == s.height && p.timestamp[0] == s.timestamp && p.kernel_timestamp[0] == s.kernel_timestamp, "header");
    expect(std::memcmp(p.receiver_digest.data(), s.receiver, 40) == 0 && std::memcmp(p.lock_script_hash.data(), s.lock, 40) == 0,
           "guesser_receiver_data");
    expect(p.fee[0] == s.fee[0] && p.fee[1] == s.fee[1] && p.coinbase_tag[0] == 1 && p.coinbase[0] == 77 && p.coinbase[1] == 1,
           "amounts");
    expect(p.n_announcements[0] == 3 && p.outputs == s.outputs && p.out_off == std::vector<uint64_t>({0, 2}), "outputs");
    expect(p.minimum == s.minimum && p.distances == s.distances && p.rec_off == std::vector<uint64_t>({0, 3}), "records");
    expect(p.entry_off == std::vector<uint64_t>({0, 2, 2, 4}) && p.chunk_index == std::vector<uint64_t>({2, UINT64_MAX, 2, UINT64_MAX}),
           "entries");
    expect(p.path_off == std::vector<uint64_t>({0, 1, 3, 4, 6}) && p.rel_off == std::vector<uint64_t>({0, 3, 6, 9, 12}), "offsets");
    expect(p.path.size() == 30 && std::equal(s.paths[2][1].begin(), s.paths[2][1].end(), p.path.begin() + 20), "paths");
    expect(p.rel.size() == 12 && p.rel[9] == s.rels[2][1][0], "chunks");
    expect(p.aocl_num_leafs[0] == 11 && p.aocl_n_peaks[0] == 3 && p.swbf_n_peaks[0] == 1 && p.aocl_peaks.size() == 320 &&
               std::equal(s.aocl_peaks.begin(), s.aocl_peaks.end(), p.aocl_peaks.begin()) && p.aocl_peaks[15] == 0,
           "accumulator");
    expect(p.active == s.active && p.active_off == std::vector<uint64_t>({0, 4}), "window");
    const nhip_msa m = nhip::blk_ms_body_msa(p, 0);
    expect(m.aocl.n_peaks == 3 && m.aocl.num_leafs == 11 && m.swbf_inactive.peaks == p.swbf_peaks.data() && m.n_active == 4,
           "body msa");
    // a second block appends behind the first
    expect(nhip::blk_ms_walk_block(b.data(), b.size(), s.h, 0, p) == NHIP_OK && p.n == 2, "walk twice");
    expect(p.rec_off == std::vector<uint64_t>({0, 3, 6}) && p.entry_off.back() == 8 && p.path_off.back() == 12 &&
               p.rel_off.back() == 24 && p.active_off.back() == 8 && p.out_off.back() == 4 && p.aocl_peaks.size() == 640,
           "second block");
    // truncated at every byte of its kernel (and a few past it): a decode error, and the parts stay as they were
    for (size_t cut = s.kernel_begin; cut <= s.kernel_end + 8; ++cut) {
        const std::vector<uint8_t> t(b.begin(), b.begin() + cut);  // its own allocation: a read past `cut` is caught
        nhip::BlkMsParts q;
        expect(nhip::blk_ms_walk_block(t.data(), t.size(), s.h, 0, q) == NHIP_ERR_DECODE, "truncated");
        expect(q.n == 0 && q.height.empty() && q.minimum.empty() && q.rec_off.size() == 1 && q.entry_off.size() == 1, "untouched");
    }
    // lengths that the rest of the input cannot hold, and more than 64 peaks
    for (size_t at : {s.kernel_begin, s.kernel_end + 8}) {
        std::vector<uint8_t> t = b;
        const uint64_t huge = ~0ull >> 1;
        std::memcpy(t.data() + at, &huge, 8);
        nhip::BlkMsParts q;
        expect(nhip::blk_ms_walk_block(t.data(), t.size(), s.h, 0, q) == NHIP_ERR_DECODE && q.n == 0, "length past the buffer");
    }
    Sample big = sample(rng);
    big.aocl_peaks.assign(5 * 70, 3);
    big.swbf_peaks.assign(5 * 64, 4);
    const std::vector<uint8_t> bb = big.bytes();
    nhip::BlkMsParts q;
    expect(nhip::blk_ms_walk_block(bb.data(), bb.size(), big.h, 0, q) == NHIP_OK && q.aocl_n_peaks[0] == 65 && q.swbf_n_peaks[0] == 64 &&
               q.aocl_peaks.size() == 320 && nhip::blk_ms_peaks_oversize(q, 0) && nhip::blk_ms_body_msa(q, 0).aocl.n_peaks == 64,
           "peak counts saturate");
    // the public two-call form
    nhip_blk_block blk{};
    nhip_blk_ms_parts o{};
    expect(nhip_blk_ms_walk(b.data(), b.size(), s.h, &blk, 1, &o) == NHIP_OK && o.records == 3 && o.entries == 4 &&
               o.path_digests == 6 && o.rel_words == 12 && o.n_outputs == 2 && o.active_words == 4,
           "count pass");
    uint64_t one = 0;
    o.height = &one;
    expect(nhip_blk_ms_walk(b.data(), b.size(), s.h, &blk, 1, &o) == NHIP_ERR_ARG, "some arrays only");
    blk.offset = b.size() + 1;
    o.height = nullptr;
    expect(nhip_blk_ms_walk(b.data(), b.size(), s.h, &blk, 1, &o) == NHIP_ERR_ARG, "offset past the buffer");
    nhip_blk_ms_params prm;
    nhip_blk_ms_params_default(&prm);
    expect(prm.pow_tree_height == 29 && prm.max_num_inputs == 1u << 14 && prm.max_num_outputs == 1u << 14 &&
               prm.max_num_announcements == 1u << 14 && prm.time_lock_hash[4] == 0,
           "params default");
}

}  // namespace

int main() {
    std::mt19937_64 rng(2900);
    check_integers(rng);
    check_rules(rng);
    check_encodings(rng);
    check_walk(rng);
    std::printf("checks %d failures %d\n", checks, failures);
    return failures ? 1 : 0;
}
