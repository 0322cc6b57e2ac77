// C-ABI layer of libneptune_hip.so, block digests and the header-chain rules (declarations:
// include/neptune_hip.h).  Each call: shape checks (chain_shape.cpp), the host-only decode of
// every block (one walk each of nhip_blk_header's and nhip_blk_sequences' decoders), the body MAST hashes as blocks_to_validate computes them
// (nhip_mast_hash_batch, two calls), then one Stage: the proofs' raw bytes uploaded run by run (wire.hpp),
// k_wire_words, k_block_proof_leaf, k_block_masts and, for the chain check, k_block_links.
#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "chain.hpp"
#include "chain_shape.hpp"
#include "ctx.hpp"
#include "goldilocks.hpp"
#include "kernels.hpp"
#include "wire.hpp"

using nhip::hip_fail;
using nhip::Stage;

extern "C" int nhip_internal_is_pinned(const void* p, size_t bytes);  // host_pinned.cpp
extern "C" void* nhip_internal_staging(nhip_ctx* c, size_t bytes);    // capi.hip
namespace nhip {  // bincode.cpp: one walk of a block each
int blk_header_append(const uint8_t* bytes, size_t n_bytes, uint32_t pow_tree_height, uint64_t offset,
                      nhip_blk_header_out* out, std::vector<uint64_t>& w);
int blk_sequences_into(const uint8_t* bytes, size_t n_bytes, uint32_t pow_tree_height, uint64_t offset,
                       std::vector<uint64_t>& words, uint64_t offsets[12]);
}  // namespace nhip

namespace {

struct ChainHost {
    std::vector<nhip::ChainBlockDev> blk;
    std::vector<uint64_t> words, paths, peaks;
    std::vector<nhip_span> spans;
    std::vector<nhip::ProofIn> in;
    uint64_t proof_words = 0;
};

// Host-only decode of the n blocks, and their body MAST hashes (two GPU calls of their own)
int chain_decode(nhip_ctx* c, const uint8_t* bytes, size_t n_bytes, uint32_t h, const nhip_blk_block* blocks, size_t n,
                 ChainHost& H) {
    H.blk.resize(n);
    H.spans.resize(n);
    H.in.resize(n);
    H.paths.resize((size_t)10 * h * n);
    std::vector<uint64_t> kdata, koff(8 * n + 1, 0), bdata, boff(4 * n + 1, 0), seq, tail;
    std::vector<uint64_t> tail_off(4 * n, 0);  // per block: its three body tail sequences in `tail`
    nhip_blk_header_out header;
    nhip_blk_header_out* hd = &header;
    for (size_t i = 0; i < n; ++i) {
        const size_t w0 = H.words.size();
        int rc = nhip::blk_header_append(bytes, n_bytes, h, blocks[i].offset, hd, H.words);
        if (rc) return rc;
        if (hd->appendix_words > 0xFFFFFFFFull) return NHIP_ERR_ARG;
        nhip::ChainBlockDev& b = H.blk[i];
        b = nhip::ChainBlockDev{};
        b.version = hd->version;
        b.height = hd->height;
        b.timestamp = hd->timestamp;
        for (int q = 0; q < 5; ++q) {
            b.prev[q] = hd->prev_block_digest[q];
            b.root[q] = hd->pow_root[q];
            b.nonce[q] = hd->pow_nonce[q];
            b.receiver[q] = hd->receiver_digest[q];
            b.lock_script[q] = hd->lock_script_hash[q];
            b.difficulty[q] = hd->difficulty[q];
        }
        for (int q = 0; q < 6; ++q) b.cpow[q] = hd->cumulative_proof_of_work[q];
        b.mmr_n_peaks = hd->mmr_n_peaks;
        b.mmr_num_leafs = hd->mmr_num_leafs;
        b.peaks_off = H.peaks.size() / 5;
        const uint32_t stored = hd->mmr_n_peaks < 64 ? hd->mmr_n_peaks : 64;
        H.peaks.insert(H.peaks.end(), &hd->mmr_peaks[0][0], &hd->mmr_peaks[0][0] + 5 * stored);
        b.words_off = w0;
        b.appendix_words = (uint32_t)hd->appendix_words;
        b.prefix_words = (uint32_t)hd->prefix_words;
        b.proof_off = H.proof_words;
        b.proof_len = hd->proof_len;
        H.spans[i] = nhip_span{hd->proof_offset, hd->proof_len};
        H.in[i] = nhip::ProofIn{};
        H.in[i].off = H.proof_words;
        H.in[i].len = hd->proof_len;
        H.proof_words += hd->proof_len;
        if (h) {
            rc = nhip_le_words(bytes, n_bytes, hd->path_a_offset, (size_t)5 * h, H.paths.data() + (size_t)10 * h * i);
            if (!rc) rc = nhip_le_words(bytes, n_bytes, hd->path_b_offset, (size_t)5 * h, H.paths.data() + (size_t)10 * h * i + 5 * h);
            if (rc) return rc;
        }
        // the transaction kernel's 8 MAST sequences and the body's tail sequences 2-4
        uint64_t so[12];
        rc = nhip::blk_sequences_into(bytes, n_bytes, h, blocks[i].offset, seq, so);
        if (rc) return rc;
        kdata.insert(kdata.end(), seq.begin(), seq.begin() + so[8]);
        for (int f = 0; f < 8; ++f) koff[8 * i + f + 1] = koff[8 * i] + so[f + 1];
        for (int f = 0; f < 4; ++f) tail_off[4 * i + f] = tail.size() + (so[8 + f] - so[8]);
        tail.insert(tail.end(), seq.begin() + so[8], seq.begin() + so[11]);
    }
    // body MAST hash (block_body.rs:175-182): sequence 1 is the transaction kernel's MAST hash
    std::vector<uint64_t> txk(5 * n), body(5 * n);
    int rc = nhip_mast_hash_batch(c, kdata.data(), koff.data(), 8, n, txk.data());
    if (rc) return rc;
    for (size_t i = 0; i < n; ++i) {
        bdata.insert(bdata.end(), txk.begin() + 5 * i, txk.begin() + 5 * i + 5);
        boff[4 * i + 1] = bdata.size();
        for (int f = 0; f < 3; ++f) {
            bdata.insert(bdata.end(), tail.begin() + tail_off[4 * i + f], tail.begin() + tail_off[4 * i + f + 1]);
            boff[4 * i + f + 2] = bdata.size();
        }
    }
    rc = nhip_mast_hash_batch(c, bdata.data(), boff.data(), 4, n, body.data());
    if (rc) return rc;
    for (size_t i = 0; i < n; ++i)
        for (int q = 0; q < 5; ++q) H.blk[i].body_hash[q] = body[5 * i + q];
    return NHIP_OK;
}

// Digests (and, with params, the link checks) of n decoded blocks: one Stage
int chain_run(nhip_ctx* c, const uint8_t* bytes, uint32_t h, size_t n, ChainHost& H, const nhip::ChainLinkParams* lp,
              const int64_t* parent_of, uint8_t* link_status, uint8_t* pow_ok, uint64_t* digests_out,
              nhip_pow_mast_paths* mast_out) {
    nhip::WirePlan plan;
    nhip::wire_plan(bytes, H.spans.data(), n, plan);
    std::vector<uint64_t> dig(5 * n);
    std::vector<nhip::PowMast> mast(mast_out ? n : 0);
    std::vector<uint8_t> bytes_out(lp ? 2 * n : 0);
    Stage st(c);
    nhip::ChainDev d{};
    d.n = (uint32_t)n;
    d.tree_height = h;
    uint8_t* d_raw;
    uint64_t *d_boff, *d_proof_words;
    nhip::ProofIn* d_in;
    const int64_t* d_parent = nullptr;
    uint8_t* d_status = nullptr;
    st.tmp(d_raw, plan.raw_bytes);
    st.tmp(d_boff, n);
    st.tmp(d_in, n);
    st.tmp(d_proof_words, (size_t)H.proof_words);
    st.in(d.blk, H.blk.data(), n);
    st.in(d.words, H.words.data(), H.words.size());
    st.in(d.paths, H.paths.data(), H.paths.size());
    st.in(d.peaks, H.peaks.data(), H.peaks.size());
    st.tmp(d.leaf_raw, n, 5);
    st.tmp(d.digest_raw, n, 5);
    st.tmp(d.header_raw, n, 5);
    st.tmp(d.paths_raw, H.paths.size());
    st.tmp(d.mast, n);
    if (lp) {
        st.in(d_parent, parent_of, n);
        st.tmp(d_status, n, 2);  // link_status, pow_ok
    }
    if (st.commit()) return st.finish();
    d.proof_words = d_proof_words;
    bool any_pageable = false;
    for (const nhip::WireRun& r : plan.runs)
        any_pageable |= !nhip_internal_is_pinned(bytes + r.start, (size_t)(r.end - r.start));
    std::vector<uint8_t> pageable;
    uint8_t* stage = nullptr;
    if (any_pageable) {
        stage = (uint8_t*)nhip_internal_staging(c, plan.raw_bytes);
        if (!stage) {
            pageable.resize(plan.raw_bytes);
            stage = pageable.data();
        }
    }
    st.step([&] {
        return hip_fail(nhip::wire_upload(plan, bytes, d_raw, stage,
                                          [](const void* q, size_t b) { return nhip_internal_is_pinned(q, b) != 0; },
                                          c->stream));
    });
    st.up(d_boff, plan.boff.data(), n);
    st.up(d_in, H.in.data(), n);
    st.launch([&] {
        return nhip::launch_wire_words(d_raw, d_boff, d_in, (uint32_t)n, H.proof_words, d_proof_words, c->stream);
    });
    st.launch([&] { return nhip::launch_block_proof_leaf(d, c->stream); });
    st.launch([&] { return nhip::launch_block_masts(d, c->stream); });
    if (lp) {
        st.launch([&] { return nhip::launch_block_links(d, *lp, d_parent, d_status, d_status + n, c->stream); });
        st.out(bytes_out.data(), d_status, 2 * n);
    }
    // into temporaries first: the outputs stay untouched unless the whole call succeeds
    st.out(dig.data(), d.digest_raw, 5 * n);
    if (mast_out) st.out(mast.data(), d.mast, n);
    const int rc = st.finish();
    if (rc) return rc;
    if (digests_out)
        for (size_t k = 0; k < 5 * n; ++k) digests_out[k] = nhip::from_mont(dig[k]);
    if (mast_out)
        for (size_t i = 0; i < n; ++i)
            for (int q = 0; q < 5; ++q) {
                for (int k = 0; k < 3; ++k) mast_out[i].pow[k][q] = nhip::from_mont(mast[i].pow[k][q]);
                for (int k = 0; k < 2; ++k) mast_out[i].header[k][q] = nhip::from_mont(mast[i].header[k][q]);
                mast_out[i].kernel[0][q] = nhip::from_mont(mast[i].kernel[0][q]);
            }
    if (lp)
        for (size_t i = 0; i < n; ++i) {
            link_status[i] = bytes_out[i];
            pow_ok[i] = bytes_out[n + i];
        }
    return NHIP_OK;
}

}  // namespace

extern "C" {

int nhip_blk_digests(nhip_ctx* c, const uint8_t* bytes, size_t n_bytes, uint32_t pow_tree_height,
                     const nhip_blk_block* blocks, size_t n, uint64_t* digests_out, nhip_pow_mast_paths* mast_out) {
    if (!c || pow_tree_height > nhip::CHAIN_MAX_TREE_HEIGHT) return NHIP_ERR_ARG;
    if (n == 0) return NHIP_OK;
    if (!digests_out || nhip::chain_blocks_ok(bytes, n_bytes, blocks, n)) return NHIP_ERR_ARG;
    try {
        ChainHost H;
        const int rc = chain_decode(c, bytes, n_bytes, pow_tree_height, blocks, n, H);
        if (rc) return rc;
        return chain_run(c, bytes, pow_tree_height, n, H, nullptr, nullptr, nullptr, nullptr, digests_out, mast_out);
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

int nhip_blk_chain_check(nhip_ctx* c, const uint8_t* bytes, size_t n_bytes, const nhip_chain_params* params,
                         const nhip_blk_block* blocks, size_t n, const int64_t* parent_of, uint8_t* link_status,
                         uint8_t* pow_ok, uint64_t* digests_out) {
    if (!c) return NHIP_ERR_ARG;
    if (n == 0) return NHIP_OK;
    nhip::ChainLinkParams lp{};
    if (nhip::chain_params_ok(params, &lp.np)) return NHIP_ERR_ARG;
    if (!link_status || !pow_ok || nhip::chain_blocks_ok(bytes, n_bytes, blocks, n) ||
        nhip::chain_parents_ok(parent_of, n))
        return NHIP_ERR_ARG;
    lp.hardfork_alpha_height = params->hardfork_alpha_height;
    lp.tree_height = params->pow_tree_height;
    lp.allows_mock_pow = params->allows_mock_pow ? 1u : 0u;
    try {
        ChainHost H;
        const int rc = chain_decode(c, bytes, n_bytes, params->pow_tree_height, blocks, n, H);
        if (rc) return rc;
        return chain_run(c, bytes, params->pow_tree_height, n, H, &lp, parent_of, link_status, pow_ok, digests_out, nullptr);
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

}  // extern "C"
