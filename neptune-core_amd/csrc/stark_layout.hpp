// The host arithmetic of a STARK batch (stark_host.cpp): what the proof lengths and headers say of
// its size, the multiproof op capacities, and where each buffer lies in the batch's device scratch
// and in its readback region.  No HIP runtime calls, so tests/native/stark_layout_check.cpp runs it
// under ASan + UBSan against a flat restatement of the sizes.
#pragma once
#include <algorithm>
#include <vector>

#include "kernels.hpp"
#include "stage_layout.hpp"
#include "stark.hpp"

namespace nhip {

// What the host knows of a batch: its layout in the device word buffer and the scratch sizes,
// from the proof lengths and the padded height each proof header declares.  Everything else (the
// proof-stream walk, descriptors, Fiat-Shamir programs, decode failures) is k_decode's, every run.
struct HostBatch {
    Dims D{};
    uint32_t n = 0;
    uint64_t proof_words = 0;   // proof region [0, proof_words) of the word buffer
    uint64_t words_total = 0;   // + the staged claim encodings
    uint32_t max_R = 0, max_last_cw = 1, levels = 0;
    uint32_t fs_stride = 0, xs_stride = 0;
    uint64_t perms_static = 0, perms_lcw = 0;  // device-counted, per run
};

inline uint64_t claim_words(uint64_t input_len, uint64_t output_len) { return output_len + input_len + 10; }

// Batch sizing.  In: H.D, and of every pin[i] its len and claim_in_n / claim_out_n; header5(i, h5)
// fetches proof i's first five words (called only for proofs of at least five).  Out: the rest of
// pin (proof words back to back, then the claim encodings), the shape each well-formed header
// declares (shp[i]; a malformed one gives sized_log2_ph == SHAPE_NONE and sizes nothing), and H's
// word counts, maxima and strides.  k_decode re-reads the header and rejects a proof whose walk
// disagrees (never happens for one buffer; guards the scratch bounds).
template <class Header5>
inline void size_batch(HostBatch& H, std::vector<ProofIn>& pin, std::vector<ProofShape>& shp, Header5&& header5) {
    const size_t n = pin.size();
    H.n = (uint32_t)n;
    shp.assign(n, ProofShape{});
    uint64_t cur = 0;
    for (size_t i = 0; i < n; ++i) {
        pin[i].off = cur;
        cur += pin[i].len;
    }
    H.proof_words = cur;
    for (size_t i = 0; i < n; ++i) {
        pin[i].claim_off = cur;
        cur += claim_words(pin[i].claim_in_n, pin[i].claim_out_n);
    }
    H.words_total = cur;
    for (size_t i = 0; i < n; ++i) {
        uint64_t h5[5], lph = 0;
        ProofShape s{};
        bool hdr = pin[i].len >= 5;
        if (hdr) {
            header5(i, h5);
            hdr = H.D.mont_words ? header_log2_ph<true>(h5, pin[i].len, lph) : header_log2_ph<false>(h5, pin[i].len, lph);
        }
        if (hdr && shape_of(H.D, lph, s)) {
            pin[i].sized_log2_ph = s.log2_ph;
            shp[i] = s;
            H.max_R = std::max(H.max_R, s.R);
            H.levels = std::max(H.levels, s.log2_N);
            H.max_last_cw = std::max(H.max_last_cw, 1u << (s.log2_N - s.R));
        } else {
            pin[i].sized_log2_ph = SHAPE_NONE;
        }
    }
    H.fs_stride = fs_ops_for(H.max_R);
    H.xs_stride = SampleLayout::of(H.D.d, H.max_R).total;
}

// Multiproof op capacity per (level, shard): a tree of height h has at most min(k, 2^(h-1-l))
// parents at level l; shard = proof index % MP_SHARDS.  A proof has 4 trees of its FRI domain's
// height (main, aux, quotient, FRI round 0) and one per further round, each half the one before.
struct MpCaps {
    std::vector<uint64_t> scap, sbase;  // [levels][MP_SHARDS] op capacity / first op of the shard
    std::vector<uint64_t> cap;          // [levels] op capacity of the level
    uint64_t total = 0;
};
inline void mp_capacities(const HostBatch& H, const std::vector<ProofIn>& pin, const std::vector<ProofShape>& shp,
                          MpCaps& c) {
    const uint32_t k = H.D.d.num_checks;
    c.scap.assign((size_t)H.levels * MP_SHARDS, 0);
    c.sbase.assign((size_t)H.levels * MP_SHARDS, 0);
    c.cap.assign(H.levels, 0);
    for (size_t i = 0; i < pin.size(); ++i) {
        if (pin[i].sized_log2_ph == SHAPE_NONE) continue;
        const ProofShape& s = shp[i];
        const uint32_t sh = (uint32_t)(i % MP_SHARDS);
        for (uint32_t t = 0; t < 4 + s.R; ++t) {
            const uint32_t h = t < 4 ? s.log2_N : s.log2_N - (t - 4);
            for (uint32_t l = 0; l < h; ++l)
                c.scap[(size_t)l * MP_SHARDS + sh] += std::min<uint64_t>(k, 1ull << std::min(h - 1 - l, 40u));
        }
    }
    c.total = 0;
    for (uint32_t l = 0; l < H.levels; ++l)
        for (uint32_t q = 0; q < MP_SHARDS; ++q) {
            c.sbase[(size_t)l * MP_SHARDS + q] = c.total;
            c.total += c.scap[(size_t)l * MP_SHARDS + q];
            c.cap[l] += c.scap[(size_t)l * MP_SHARDS + q];
        }
}

// The readback region [device counters | plan counters | verdicts]: one device buffer laid out as
// the pinned host buffer, so one memset clears the counters and one copy brings everything back
// (three fewer dependent packets per batch).
struct Readback {
    size_t plan_counters_off = 0;  // [levels][MP_SHARDS] uint32, after the CNT_N device counters
    size_t verdicts_off = 0;       // n bytes; also the bytes cleared before a run
    size_t copy_bytes = 0;         // verdicts_off + n: what a run copies back
    size_t device_bytes = 0, host_bytes = 0;  // sizes of the two buffers (padded)
    static Readback of(uint32_t levels, uint32_t n) {
        Readback r;
        r.plan_counters_off = CNT_N * 8;
        r.verdicts_off = r.plan_counters_off + (size_t)levels * MP_SHARDS * 4;
        r.copy_bytes = r.verdicts_off + n;
        r.device_bytes = r.verdicts_off + std::max<size_t>(1, n) + 8;
        r.host_bytes = r.copy_bytes + 16;
        return r;
    }
};

// Slots of the compiled AIR program held in LDS; the rest live in the scratch (air_gslots).
inline uint32_t air_lds_slots(uint32_t slots, uint32_t lds_cap) { return std::min(slots, lds_cap); }

// The batch's device scratch: one named buffer each, in this order, 256-byte aligned (StageLayout:
// an empty buffer still takes one unit).  overflow: a size left size_t (NHIP_ERR_OOM).
struct ScratchLayout {
    struct Buf {
        size_t off = 0, bytes = 0;
    };
    Buf desc, fs_ops, xs, idx, dig, ood, fail, proof_in;
    Buf readback;   // Readback::device_bytes
    Buf wire_boff;  // wire source: the proofs' byte offsets in the raw buffer
    Buf mp_ops, mp_arena, mp_shard_base, mp_shard_cap, mp_roots, mp_dups, mp_ndup;
    Buf xdom, lcw;
    Buf air_gslots;  // OOD slots past the LDS budget (an AIR larger than ~6K live XFEs)
    Buf mp_lvl_g0, mp_lvl_cnt, mp_lvl_n;  // per (proof, tree group, level) op ranges of the plan (k_mp_climb)
    size_t total = 0;
    bool overflow = false;

    // air_gslot_n: the AIR program's slots past the LDS budget, per proof (below 2^26: an AIR has
    // at most 2^24 nodes and as many constraints, and n is below 2^32)
    static ScratchLayout of(const HostBatch& H, const Readback& rb, bool wire, uint64_t mp_total, uint32_t air_gslot_n) {
        StageLayout L;
        const auto buf = [&L](size_t count, size_t per, size_t elem) {
            const unsigned slot = L.add(count, per, elem);
            return L.overflow ? Buf{} : Buf{L.off[slot], L.bytes[slot]};
        };
        const size_t N1 = std::max<size_t>(1, H.n), k = H.D.d.num_checks;
        const size_t groups = N1 * (1 + H.max_R), shards = (size_t)H.levels * MP_SHARDS;
        ScratchLayout S;
        S.desc = buf(N1, 1, sizeof(ProofDesc));
        S.fs_ops = buf(N1, H.fs_stride, sizeof(FsOp));
        S.xs = buf(N1, H.xs_stride, 24);
        S.idx = buf(N1, k, 4);
        S.dig = buf(N1, 3 * k, 40);
        S.ood = buf(N1, 9, 8);
        S.fail = buf(N1, 1, 4);
        S.proof_in = buf(N1, 1, sizeof(ProofIn));
        S.readback = buf(rb.device_bytes, 1, 1);
        S.wire_boff = buf(wire ? N1 : 0, 1, 8);
        S.mp_ops = buf(mp_total + 1, 1, 16);
        S.mp_arena = buf(mp_total + 1, 1, 40);
        S.mp_shard_base = buf(shards + 1, 1, 8);
        S.mp_shard_cap = buf(shards + 1, 1, 8);
        S.mp_roots = buf(N1, 4 + H.max_R, sizeof(MpRoot));
        S.mp_dups = buf(groups, k, 8);
        S.mp_ndup = buf(groups, 1, 4);
        S.xdom = buf(N1, k, 8);
        S.lcw = buf(N1, H.max_last_cw, 40);
        S.air_gslots = buf(N1 * air_gslot_n + 1, 1, 24);
        S.mp_lvl_g0 = buf(groups, (size_t)H.levels + 1, 8);
        S.mp_lvl_cnt = buf(groups, (size_t)H.levels + 1, 4);
        S.mp_lvl_n = buf(groups, 1, 4);
        S.total = L.total;
        S.overflow = L.overflow;
        return S;
    }
};

}  // namespace nhip
