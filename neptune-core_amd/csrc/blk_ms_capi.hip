// C-ABI layer of libneptune_hip.so, a block file's mutator-set and transaction rules (declarations:
// include/neptune_hip.h).  nhip_blk_ms_check is: shape checks, the host walk (bincode.cpp,
// blk_ms_parts.cpp), the block digests unless given (nhip_blk_digests), k_guesser_fee_records, pass A
// (nhip_ms_apply_batch: parent body accumulator + guesser records), pass B (nhip_ms_apply_batch_packed: the child's
// packed inputs and outputs against pass A's accumulator), k_blk_ms_rules.  Job i of either pass is block i, so the
// walk's pools are staged as they lie; a pair that is skipped, or whose parent has no accumulator after, runs on an
// empty accumulator, and k_blk_ms_rules reads nothing of such a job but pass B's unpack status (rule 2.a comes first).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "blk_ms.hpp"
#include "blk_ms_parts.hpp"
#include "chain_shape.hpp"
#include "ctx.hpp"

using nhip::Stage;

namespace {

constexpr uint64_t P = nhip::txrules::P;

int params_ok(const nhip_blk_ms_params* p, nhip::BlkMsParamsDev* out) {
    if (!p || p->pow_tree_height > nhip::CHAIN_MAX_TREE_HEIGHT) return NHIP_ERR_ARG;
    for (int q = 0; q < 5; ++q) {  // BFieldElement::new
        out->native_currency_hash[q] = p->native_currency_hash[q] % P;
        out->time_lock_hash[q] = p->time_lock_hash[q] % P;
    }
    out->lim = nhip::txrules::TxLimits{p->max_num_inputs, p->max_num_outputs, p->max_num_announcements};
    return NHIP_OK;
}

std::vector<nhip::BlkMsBlockDev> device_blocks(const nhip::BlkMsParts& p) {
    std::vector<nhip::BlkMsBlockDev> blk(p.n);
    for (size_t i = 0; i < p.n; ++i) {
        nhip::BlkMsBlockDev& b = blk[i];
        for (int q = 0; q < 5; ++q) {
            b.receiver[q] = p.receiver_digest[5 * i + q];
            b.lock_script[q] = p.lock_script_hash[5 * i + q];
        }
        b.t.header_height = p.height[i];
        b.t.header_timestamp = p.timestamp[i];
        b.t.kernel_timestamp = p.kernel_timestamp[i];
        b.t.fee = nhip::txrules::I128{p.fee[2 * i], p.fee[2 * i + 1]};
        b.t.coinbase = nhip::txrules::I128{p.coinbase[2 * i], p.coinbase[2 * i + 1]};
        b.t.has_coinbase = p.coinbase_tag[i];
        b.t.n_inputs = p.rec_off[i + 1] - p.rec_off[i];  // a packed list has one record per unpacked input
        b.t.n_outputs = p.out_off[i + 1] - p.out_off[i];
        b.t.n_announcements = p.n_announcements[i];
    }
    return blk;
}

// The walk and the digests every entry point starts from.  dig: the caller's, or own's
struct Decoded {
    nhip::BlkMsParts parts;
    std::vector<nhip::BlkMsBlockDev> blk;
    std::vector<uint64_t> own;
    const uint64_t* dig = nullptr;
};
int decode(nhip_ctx* c, const uint8_t* bytes, size_t n_bytes, uint32_t h, const nhip_blk_block* blocks, size_t n,
           const uint64_t* digests, Decoded& d) {
    int rc = nhip::blk_ms_walk(bytes, n_bytes, h, blocks, n, d.parts);
    if (rc) return rc;
    d.blk = device_blocks(d.parts);
    d.dig = digests;
    if (!digests) {
        d.own.resize(5 * n);
        if ((rc = nhip_blk_digests(c, bytes, n_bytes, h, blocks, n, d.own.data(), nullptr)) != NHIP_OK) return rc;
        d.dig = d.own.data();
    }
    return NHIP_OK;
}

struct Guesser {
    std::vector<uint64_t> records;
    std::vector<uint8_t> n_records, status;
};
int guesser_records(nhip_ctx* c, const Decoded& d, const nhip::BlkMsParamsDev& pd, Guesser& g) {
    const size_t n = d.parts.n;
    g.records.resize(10 * n);
    g.n_records.resize(2 * n);  // n_records, then status
    Stage st(c);
    const nhip::BlkMsBlockDev* d_blk;
    const uint64_t* d_dig;
    uint64_t* d_rec;
    uint8_t* d_bytes;
    st.in(d_blk, d.blk.data(), n);
    st.in(d_dig, d.dig, n, 5);
    st.tmp(d_rec, n, 10);
    st.tmp(d_bytes, n, 2);
    if (st.commit()) return st.finish();
    st.launch([&] {
        return nhip::launch_guesser_fee_records(d_blk, d_dig, pd, (uint32_t)n, d_rec, d_bytes, d_bytes + n, c->stream);
    });
    st.out(g.records.data(), d_rec, 10 * n);
    st.out(g.n_records.data(), d_bytes, 2 * n);
    const int rc = st.finish();
    if (rc) return rc;
    g.status.assign(g.n_records.begin() + n, g.n_records.end());
    g.n_records.resize(n);
    return NHIP_OK;
}

}  // namespace

extern "C" {

int nhip_blk_guesser_fee_records(nhip_ctx* c, const uint8_t* bytes, size_t n_bytes, const nhip_blk_ms_params* params,
                                 const nhip_blk_block* blocks, size_t n, const uint64_t* digests, uint64_t* records,
                                 uint8_t* n_records, uint8_t* status) {
    nhip::BlkMsParamsDev pd{};
    if (!c || params_ok(params, &pd)) return NHIP_ERR_ARG;
    if (n == 0) return NHIP_OK;
    if (!records || !n_records || !status || n > UINT32_MAX / 2 || nhip::chain_blocks_ok(bytes, n_bytes, blocks, n))
        return NHIP_ERR_ARG;
    try {
        Decoded d;
        int rc = decode(c, bytes, n_bytes, params->pow_tree_height, blocks, n, digests, d);
        if (rc) return rc;
        Guesser g;
        if ((rc = guesser_records(c, d, pd, g)) != NHIP_OK) return rc;
        std::copy(g.records.begin(), g.records.end(), records);
        std::copy(g.n_records.begin(), g.n_records.end(), n_records);
        std::copy(g.status.begin(), g.status.end(), status);
        return NHIP_OK;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

int nhip_blk_ms_check(nhip_ctx* c, const uint8_t* bytes, size_t n_bytes, const nhip_blk_ms_params* params,
                      const nhip_blk_block* blocks, size_t n, const int64_t* parent_of, const uint64_t* digests,
                      uint8_t* status, uint8_t* ms_status, uint64_t* bad_record) {
    nhip::BlkMsParamsDev pd{};
    if (!c || params_ok(params, &pd)) return NHIP_ERR_ARG;
    if (n == 0) return NHIP_OK;
    if (!status || !ms_status || !bad_record || n > UINT32_MAX / 2 || nhip::chain_blocks_ok(bytes, n_bytes, blocks, n) ||
        nhip::chain_parents_ok(parent_of, n))
        return NHIP_ERR_ARG;
    try {
        Decoded d;
        int rc = decode(c, bytes, n_bytes, params->pow_tree_height, blocks, n, digests, d);
        if (rc) return rc;
        const nhip::BlkMsParts& p = d.parts;
        Guesser g;
        if ((rc = guesser_records(c, d, pd, g)) != NHIP_OK) return rc;

        const nhip_msa empty{};
        std::vector<uint8_t> flags(n, 0);
        // pass A: job i = (parent's body accumulator, parent's guesser records, no removals)
        std::vector<nhip_msa> before_a(n, empty);
        std::vector<uint64_t> add_off(n + 1, 0), additions, none(n + 1, 0), act_off(n + 1, 0);
        for (size_t i = 0; i < n; ++i) {
            const int64_t par = parent_of[i];
            if (par >= 0) {
                if (nhip::blk_ms_peaks_oversize(p, (size_t)par)) flags[i] |= nhip::BLKMS_FLAG_PARENT_OVERSIZE;
                if (nhip::blk_ms_peaks_oversize(p, i)) flags[i] |= nhip::BLKMS_FLAG_EXPECTED_OVERSIZE;
                if (g.status[par] == NHIP_GUESSER_OK && !(flags[i] & nhip::BLKMS_FLAG_PARENT_OVERSIZE)) {
                    before_a[i] = nhip::blk_ms_body_msa(p, (size_t)par);
                    const size_t k = g.n_records[par] == 2 ? 2 : 0;
                    additions.insert(additions.end(), g.records.begin() + 10 * par, g.records.begin() + 10 * par + 5 * k);
                }
            }
            add_off[i + 1] = additions.size() / 5;
            act_off[i + 1] = act_off[i] + before_a[i].n_active;
        }
        std::vector<uint8_t> va(n), sa(n), vb(n), sb(n);
        std::vector<uint64_t> bad_a(n), bad_b(n);
        std::vector<uint64_t> aocl_peaks(n * 64 * 5), swbf_peaks(n * 64 * 5), aocl_nl(n), swbf_nl(n), n_act(n);
        std::vector<uint32_t> aocl_np(n), swbf_np(n), act(act_off[n] ? act_off[n] : 1);
        nhip_ms_apply_in in_a{};
        in_a.n_jobs = n;
        in_a.msa_before = before_a.data();
        in_a.add_off = add_off.data();
        in_a.additions = additions.data();
        in_a.rec_off = none.data();
        nhip_ms_apply_out out_a{va.data(),      sa.data(),      bad_a.data(),   aocl_peaks.data(), aocl_np.data(), aocl_nl.data(),
                                swbf_peaks.data(), swbf_np.data(), swbf_nl.data(), act_off.data(),    act.data(),     n_act.data()};
        if ((rc = nhip_ms_apply_batch(c, &in_a, &out_a)) != NHIP_OK) return rc;

        // pass B: job i = (pass A's accumulator, the child's packed inputs and outputs, its body's accumulator)
        std::vector<nhip_msa> before_b(n, empty), expected(n, empty);
        for (size_t i = 0; i < n; ++i) {
            expected[i] = nhip::blk_ms_body_msa(p, i);
            if (parent_of[i] < 0 || sa[i] != NHIP_MS_OK) continue;
            nhip_msa& m = before_b[i];
            m.aocl = nhip_mmr{aocl_peaks.data() + 64 * 5 * i, aocl_np[i], aocl_nl[i]};
            m.swbf_inactive = nhip_mmr{swbf_peaks.data() + 64 * 5 * i, swbf_np[i], swbf_nl[i]};
            m.n_active = n_act[i];
            m.active = n_act[i] ? act.data() + act_off[i] : nullptr;
        }
        const nhip_ms_chunks chunks = nhip::blk_ms_chunks(p);
        nhip_ms_apply_in in_b{};
        in_b.n_jobs = n;
        in_b.msa_before = before_b.data();
        in_b.add_off = p.out_off.data();
        in_b.additions = p.outputs.data();
        in_b.rec_off = p.rec_off.data();
        in_b.minimum = p.minimum.data();
        in_b.distances = p.distances.data();
        in_b.chunks = &chunks;
        in_b.msa_expected = expected.data();
        nhip_ms_apply_out out_b{};
        out_b.verdict = vb.data();
        out_b.status = sb.data();
        out_b.bad_record = bad_b.data();
        if ((rc = nhip_ms_apply_batch_packed(c, &in_b, &out_b)) != NHIP_OK) return rc;

        // rules 2.f-2.l and the pair's status
        std::vector<uint8_t> st_out(2 * n);
        std::vector<uint64_t> bad_out(n);
        Stage st(c);
        nhip::BlkMsRulesDev r{};
        r.n = (uint32_t)n;
        uint8_t* d_status;
        st.in(r.blk, d.blk.data(), n);
        st.in(r.parent_of, parent_of, n);
        st.in(r.guesser_status, g.status.data(), n);
        st.in(r.a_status, sa.data(), n);
        st.in(r.b_status, sb.data(), n);
        st.in(r.b_bad, bad_b.data(), n);
        st.in(r.flags, flags.data(), n);
        st.tmp(d_status, n, 2);
        st.tmp(r.bad_record, n);
        if (st.commit()) return st.finish();
        r.status = d_status;
        r.ms_status = d_status + n;
        st.launch([&] { return nhip::launch_blk_ms_rules(r, pd, c->stream); });
        st.out(st_out.data(), d_status, 2 * n);
        st.out(bad_out.data(), r.bad_record, n);
        if ((rc = st.finish()) != NHIP_OK) return rc;
        std::copy(st_out.begin(), st_out.begin() + n, status);
        std::copy(st_out.begin() + n, st_out.end(), ms_status);
        std::copy(bad_out.begin(), bad_out.end(), bad_record);
        return NHIP_OK;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

}  // extern "C"
