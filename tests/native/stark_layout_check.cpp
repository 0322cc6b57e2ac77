// Host-side check of stark_layout.hpp (run by tests/test_stark_layout_host.py, plain and under
// ASan + UBSan): the named scratch layout, the readback description and the multiproof capacities
// against a flat restatement of the size table and the capacity loop they replaced, the capacity
// bound min(k, 2^(h-1-l)) against the parent counts of every set of revealed leaves, and the batch
// sizing on malformed, short, mixed and two-form proofs.
#include "stark_layout.hpp"

#include <cstdio>
#include <cstring>
#include <vector>
using namespace nhip;

static uint64_t bad = 0, n_checked = 0;
static void expect(bool ok, const char* what, uint64_t a = 0, uint64_t b = 0) {
    ++n_checked;
    if (!ok) {
        if (bad < 10) printf("FAIL %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
        ++bad;
    }
}

static Dims dims_for(uint32_t k) {
    Dims D{};
    D.d.num_main = 24;
    D.d.num_aux = 9;
    D.d.num_quot_seg = 4;
    D.d.num_checks = k;
    D.d.num_deep = 3;
    D.d.log2_expansion = 2;
    D.d.num_trace_randomizers = k + 6;
    D.d.num_sampled = 63;
    D.d.num_constraints = 10;
    D.expansion = 4;
    return D;
}

static size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

// ---- 1. the scratch layout and the readback against the restated size table
struct Named {
    const char* name;
    ScratchLayout::Buf ScratchLayout::*member;
    size_t restated;
};

static void check_layout(uint32_t n, uint32_t levels, uint32_t max_R, bool wire, uint32_t slots, uint32_t lds_cap,
                         uint32_t k, uint64_t mp_total) {
    HostBatch H;
    H.D = dims_for(k);
    H.n = n;
    H.levels = levels;
    H.max_R = max_R;
    H.max_last_cw = max_R ? 64 : 1;
    H.fs_stride = fs_ops_for(max_R);
    H.xs_stride = SampleLayout::of(H.D.d, max_R).total;
    const Readback rb = Readback::of(levels, n);
    const ScratchLayout S = ScratchLayout::of(H, rb, wire, mp_total, slots - air_lds_slots(slots, lds_cap));
    expect(!S.overflow, "no overflow");

    // the size table as it was written before the buffers had names, without its two dead slots
    const size_t OUT_HDR = CNT_N * 8;
    const size_t N1 = n ? n : 1, tpp = 4 + max_R;
    const Named t[] = {
        {"desc", &ScratchLayout::desc, N1 * sizeof(ProofDesc)},
        {"fs_ops", &ScratchLayout::fs_ops, N1 * H.fs_stride * sizeof(FsOp)},
        {"xs", &ScratchLayout::xs, N1 * H.xs_stride * 24},
        {"idx", &ScratchLayout::idx, N1 * k * 4},
        {"dig", &ScratchLayout::dig, N1 * 3 * k * 40},
        {"ood", &ScratchLayout::ood, N1 * 9 * 8},
        {"fail", &ScratchLayout::fail, N1 * 4},
        {"proof_in", &ScratchLayout::proof_in, N1 * sizeof(ProofIn)},
        {"readback", &ScratchLayout::readback, OUT_HDR + (size_t)levels * MP_SHARDS * 4 + N1 + 8},
        {"wire_boff", &ScratchLayout::wire_boff, wire ? N1 * 8 : 0},
        {"mp_ops", &ScratchLayout::mp_ops, mp_total * 16 + 16},
        {"mp_arena", &ScratchLayout::mp_arena, mp_total * 40 + 40},
        {"mp_shard_base", &ScratchLayout::mp_shard_base, (size_t)levels * MP_SHARDS * 8 + 8},
        {"mp_shard_cap", &ScratchLayout::mp_shard_cap, (size_t)levels * MP_SHARDS * 8 + 8},
        {"mp_roots", &ScratchLayout::mp_roots, N1 * tpp * sizeof(MpRoot)},
        {"mp_dups", &ScratchLayout::mp_dups, N1 * (1 + max_R) * k * 8},
        {"mp_ndup", &ScratchLayout::mp_ndup, N1 * (1 + max_R) * 4},
        {"xdom", &ScratchLayout::xdom, N1 * k * 8},
        {"lcw", &ScratchLayout::lcw, N1 * H.max_last_cw * 40},
        {"air_gslots", &ScratchLayout::air_gslots, N1 * (size_t)(slots - (slots < lds_cap ? slots : lds_cap)) * 24 + 24},
        {"mp_lvl_g0", &ScratchLayout::mp_lvl_g0, N1 * (1 + max_R) * (size_t)(levels + 1) * 8},
        {"mp_lvl_cnt", &ScratchLayout::mp_lvl_cnt, N1 * (1 + max_R) * (size_t)(levels + 1) * 4},
        {"mp_lvl_n", &ScratchLayout::mp_lvl_n, N1 * (1 + max_R) * 4},
    };
    constexpr size_t NB = sizeof(t) / sizeof(t[0]);
    static_assert(NB == 23, "the 23 live buffers");
    // ScratchLayout is nothing but its buffers, the total and the flag: no member is missed here
    static_assert(sizeof(ScratchLayout) == NB * sizeof(ScratchLayout::Buf) + 2 * sizeof(size_t), "every buffer is listed");
    size_t end = 0, sum = 0;
    for (size_t i = 0; i < NB; ++i) {
        const ScratchLayout::Buf& f = S.*(t[i].member);
        expect(f.bytes == t[i].restated, t[i].name, f.bytes, t[i].restated);
        expect(f.off % 256 == 0, "256-aligned", i, f.off);
        expect(f.off >= end && (i == 0 || f.off > (S.*(t[i - 1].member)).off), "ascending and disjoint", i, f.off);
        end = f.off + f.bytes;
        // the old total, but an empty buffer takes one unit (a distinct address)
        sum += al(t[i].restated ? t[i].restated : 1);
    }
    expect(end <= S.total, "within total", end, S.total);
    expect(S.total == sum, "total", S.total, sum);

    expect(rb.plan_counters_off == OUT_HDR, "plan counters offset");
    expect(rb.verdicts_off == OUT_HDR + (size_t)levels * MP_SHARDS * 4, "verdicts offset");
    expect(rb.copy_bytes == OUT_HDR + (size_t)levels * MP_SHARDS * 4 + n, "copied bytes");
    expect(rb.device_bytes == S.readback.bytes && rb.device_bytes >= rb.copy_bytes, "device readback bytes");
    expect(rb.host_bytes == OUT_HDR + (size_t)levels * MP_SHARDS * 4 + n + 16, "host readback bytes");
}

static void check_layouts() {
    const uint32_t cap = AIR_LDS_SLOTS_MAX;
    for (uint32_t n : {0u, 1u, 3u, 17u})
        for (uint32_t levels : {0u, 1u, 12u})
            for (uint32_t max_R : {0u, 1u, 9u})
                for (int wire = 0; wire < 2; ++wire)
                    for (uint32_t slots : {cap - 5, cap, cap + 1000})
                        for (uint32_t k : {1u, 8u, 80u})
                            for (uint64_t mp_total : {(uint64_t)0, (uint64_t)n * 4 * levels * k})
                                check_layout(n, levels, max_R, wire != 0, slots, cap, k, mp_total);
    // a lowered cap (nhip_air_options.lds_slots)
    check_layout(3, 12, 1, false, 300, 64, 8, 1000);
    // sizes that leave size_t are an overflow, not a wrapped total
    HostBatch H;
    H.D = dims_for(80);
    H.n = 0xFFFFFFFFu;
    H.levels = 31;
    H.max_R = 26;
    H.fs_stride = 0xFFFFFFFFu;
    H.xs_stride = 0xFFFFFFFFu;
    expect(ScratchLayout::of(H, Readback::of(31, H.n), true, 1ull << 62, 1u << 25).overflow, "overflow reported");
}

// ---- 2. sizing and capacities on synthetic proofs
// A proof of `len` words whose header declares 2^log2_ph rows: [len - 1, n_items, 2, kind, log2_ph, 0..]
static std::vector<uint64_t> proof(uint64_t len, uint64_t log2_ph, bool mont) {
    std::vector<uint64_t> w(len, 0);
    const uint64_t h[5] = {len - 1, 19, 2, LOG2_PADDED_HEIGHT, log2_ph};
    for (uint64_t i = 0; i < len && i < 5; ++i) w[i] = mont ? to_mont(h[i]) : h[i];
    return w;
}

struct Sized {
    HostBatch H;
    std::vector<ProofIn> pin;
    std::vector<ProofShape> shp;
};
static Sized size_of(const Dims& D, const std::vector<std::vector<uint64_t>>& proofs) {
    Sized z;
    z.H.D = D;
    z.pin.assign(proofs.size(), ProofIn{});
    for (size_t i = 0; i < proofs.size(); ++i) {
        z.pin[i].len = proofs[i].size();
        z.pin[i].claim_in_n = (uint32_t)i;
        z.pin[i].claim_out_n = 1;
    }
    size_batch(z.H, z.pin, z.shp, [&](size_t i, uint64_t* h5) { std::memcpy(h5, proofs[i].data(), 40); });
    return z;
}

// the capacity loop as it stood inside the batch fill
static void check_capacities(const Sized& z) {
    const HostBatch& H = z.H;
    const uint32_t k = H.D.d.num_checks, levels = H.levels;
    const size_t n = z.pin.size();
    std::vector<uint64_t> mp_scap((size_t)levels * MP_SHARDS, 0), mp_sbase((size_t)levels * MP_SHARDS, 0), mp_cap(levels, 0);
    for (size_t i = 0; i < n; ++i) {
        if (z.pin[i].sized_log2_ph == SHAPE_NONE) continue;
        const ProofShape& s = z.shp[i];
        const uint32_t sh = (uint32_t)(i % MP_SHARDS);
        for (uint32_t t = 0; t < 4 + s.R; ++t) {
            const uint32_t h = t < 4 ? s.log2_N : s.log2_N - (t - 4);
            for (uint32_t l = 0; l < h; ++l)
                mp_scap[(size_t)l * MP_SHARDS + sh] += std::min<uint64_t>(k, 1ull << std::min(h - 1 - l, 40u));
        }
    }
    uint64_t mp_total = 0;
    for (uint32_t l = 0; l < levels; ++l)
        for (uint32_t q = 0; q < MP_SHARDS; ++q) {
            mp_sbase[(size_t)l * MP_SHARDS + q] = mp_total;
            mp_total += mp_scap[(size_t)l * MP_SHARDS + q];
            mp_cap[l] += mp_scap[(size_t)l * MP_SHARDS + q];
        }
    MpCaps c;
    mp_capacities(H, z.pin, z.shp, c);
    expect(c.total == mp_total, "mp_total", c.total, mp_total);
    expect(c.scap == mp_scap, "shard capacities");
    expect(c.sbase == mp_sbase, "shard bases");
    expect(c.cap == mp_cap, "level capacities");
}

static void check_sizing() {
    for (uint32_t k : {1u, 8u, 80u}) {
        const Dims D = dims_for(k);
        // a mix of heights over more proofs than shards, a malformed header and two short proofs among them
        std::vector<std::vector<uint64_t>> ps;
        for (uint32_t i = 0; i < 20; ++i) ps.push_back(proof(40 + i, 3 + i % 7, false));
        ps[4][3] = LOG2_PADDED_HEIGHT + 1;  // another item kind first
        ps[9][0] += 1;                      // a length word that disagrees with the proof's length
        ps[11] = proof(4, 5, false);        // below five words
        ps[12] = {};                        // no words at all
        ps[13] = proof(40, LOG2_PH_MAX + 1, false);  // well formed, but no shape for that height
        const Sized z = size_of(D, ps);
        uint64_t cur = 0;
        uint32_t max_R = 0, levels = 0, max_lcw = 1;
        for (size_t i = 0; i < ps.size(); ++i) {
            expect(z.pin[i].off == cur && z.pin[i].len == ps[i].size(), "proof words back to back", i);
            cur += ps[i].size();
            const bool none = i == 4 || i == 9 || i == 11 || i == 12 || i == 13;
            expect((z.pin[i].sized_log2_ph == SHAPE_NONE) == none, "SHAPE_NONE exactly for the malformed", i);
            if (none) continue;
            ProofShape s{};
            expect(shape_of(D, 3 + i % 7, s) && z.pin[i].sized_log2_ph == s.log2_ph, "declared height", i);
            expect(z.shp[i].log2_N == s.log2_N && z.shp[i].R == s.R, "shape", i);
            max_R = std::max(max_R, s.R);
            levels = std::max(levels, s.log2_N);
            max_lcw = std::max(max_lcw, 1u << (s.log2_N - s.R));
        }
        expect(z.H.proof_words == cur, "proof_words");
        for (size_t i = 0; i < ps.size(); ++i) {
            expect(z.pin[i].claim_off == cur, "claims after the proofs", i);
            cur += (uint64_t)i + 1 + 10;
        }
        expect(z.H.words_total == cur && z.H.n == ps.size(), "words_total");
        expect(z.H.max_R == max_R && z.H.levels == levels && z.H.max_last_cw == max_lcw, "maxima over the well-formed only");
        expect(z.H.fs_stride == fs_ops_for(max_R) && z.H.xs_stride == SampleLayout::of(D.d, max_R).total, "strides");
        check_capacities(z);

        // nothing but malformed proofs: sizes of an empty batch, no capacity anywhere
        const Sized m = size_of(D, {ps[4], ps[11], ps[12], ps[13]});
        expect(m.H.max_R == 0 && m.H.levels == 0 && m.H.max_last_cw == 1, "malformed proofs size nothing");
        MpCaps c;
        mp_capacities(m.H, m.pin, m.shp, c);
        expect(c.total == 0 && c.scap.empty() && c.cap.empty(), "malformed proofs reserve nothing");
        check_capacities(size_of(D, {}));

        // the two input forms of one proof
        Dims DM = D;
        DM.mont_words = 1;
        for (uint32_t lph = 0; lph <= LOG2_PH_MAX + 1; ++lph) {
            const Sized a = size_of(D, {proof(64, lph, false)}), b = size_of(DM, {proof(64, lph, true)});
            expect(a.pin[0].sized_log2_ph == b.pin[0].sized_log2_ph && a.H.levels == b.H.levels && a.H.max_R == b.H.max_R &&
                       a.H.max_last_cw == b.H.max_last_cw,
                   "Montgomery and canonical forms agree", lph);
            ProofShape s{};  // no shape past LOG2_PH_MAX, or with more FRI rounds than the descriptors hold (small k)
            expect((a.pin[0].sized_log2_ph == SHAPE_NONE) == !shape_of(D, lph, s), "a shape exactly where shape_of has one", lph);
            expect(lph <= LOG2_PH_MAX || a.pin[0].sized_log2_ph == SHAPE_NONE, "height in range", lph);
        }
        // a canonical header read as Montgomery words is malformed
        expect(size_of(DM, {proof(64, 5, false)}).pin[0].sized_log2_ph == SHAPE_NONE, "form mismatch");
    }
}

// ---- 3. min(k, 2^(h-1-l)) bounds the parents at level l of any k revealed leaves
// Pairs of adjacent bits ORed into one: the set of parents of a set of nodes.
static uint64_t parents(uint64_t m) {
    m = (m | (m >> 1)) & 0x5555555555555555ull;
    m = (m | (m >> 1)) & 0x3333333333333333ull;
    m = (m | (m >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    m = (m | (m >> 4)) & 0x00FF00FF00FF00FFull;
    m = (m | (m >> 8)) & 0x0000FFFF0000FFFFull;
    m = (m | (m >> 16)) & 0x00000000FFFFFFFFull;
    return m;
}
// Every set of `size` nodes out of 2^bits, each climbed to the root: worst[l] = the most nodes any
// of them has `l` levels up.
static void climb_all(uint32_t bits, uint32_t size, uint32_t worst[7]) {
    const uint64_t lim = bits == 6 ? 0 : 1ull << (1u << bits);  // first mask past the node range (0: 64 nodes)
    for (uint64_t m = (1ull << size) - 1;;) {
        uint64_t up = m;
        for (uint32_t l = 0; l <= bits; ++l, up = parents(up))
            worst[l] = std::max(worst[l], (uint32_t)__builtin_popcountll(up));
        const uint64_t c = m & -m, r = m + c;  // the next mask of as many bits
        if (r == 0 || (lim && r >= lim)) break;
        m = (((r ^ m) >> 2) / c) | r;
    }
}
static void check_capacity_bound() {
    for (uint32_t h = 1; h <= 6; ++h) {
        // most[s][l]: the most parents at level l (l = 0: the leaves' own parents) of s distinct leaves
        uint32_t most[9][7] = {};
        for (uint32_t s = 1; s <= 8 && s <= (1u << h); ++s) {
            if (h < 6 || s <= 5) {
                uint32_t w[7] = {};
                climb_all(h, s, w);  // every s-subset of the 2^h leaves
                for (uint32_t l = 0; l < h; ++l) most[s][l] = w[l + 1];
            } else {
                // 64 leaves, 6 to 8 of them: s leaves have between ceil(s / 2) and s distinct parents, and
                // every such set of the 32 parents is some s leaves' (one or two leaves under each), so
                // the sets of parents are enumerated in place of the 10^8 to 10^9.6 sets of leaves
                for (uint32_t j = (s + 1) / 2; j <= s; ++j) {
                    uint32_t w[7] = {};
                    climb_all(h - 1, j, w);
                    for (uint32_t l = 0; l < h; ++l) most[s][l] = std::max(most[s][l], w[l]);
                }
            }
        }
        // k sampled indices are at most min(k, 2^h) distinct leaves
        for (uint32_t k = 1; k <= 8; ++k)
            for (uint32_t l = 0; l < h; ++l) {
                uint32_t seen = 0;
                for (uint32_t s = 1; s <= k && s <= (1u << h); ++s) seen = std::max(seen, most[s][l]);
                const uint64_t cap = std::min<uint64_t>(k, 1ull << (h - 1 - l));
                expect(cap >= seen, "capacity bounds the parent count", h * 100 + k, l);
                expect(cap == seen, "and is reached", h * 100 + k, l);
            }
    }
}

int main() {
    check_layouts();
    check_sizing();
    check_capacity_bound();
    printf("checked %llu, bad %llu\n", (unsigned long long)n_checked, (unsigned long long)bad);
    return bad ? 1 : 0;
}
