// Block files and peer transactions: bincode decoding straight into the
// verifier's inputs.
//
//  * Block files: `blocks_from_file_without_record`
//    (neptune-core/src/state/archival_state/import_blocks_from_files.rs:100-115) deserializes
//    `Block`s back to back with bincode 1.x legacy options (fixed little-endian integers, u64
//    sequence lengths, u32 enum variants, u8 Option tags and bools, trailing bytes allowed) and
//    advances by each block's serialized size.  nhip_blk_scan walks a whole buffer (an mmap'd
//    blk file) once and reports, per block, what `Block::validate` rules 1.a-1.d and the
//    BlockProgram claim need: the proof's word span, the appendix claims and the BFieldCodec MAST
//    sequences of the transaction kernel and the body.
//  * Peer transactions: `TransferTransaction { kernel, proof }` (protocol/peer/
//    transfer_transaction.rs:31-47) with `TransferTransactionProof::{ProofCollection(Box<..>),
//    SingleProof(Proof)}`; nhip_tx_scan / nhip_tx_parts give the member proofs' word spans in
//    ProofCollection field order, its digests and the kernel's MAST sequences.
//
// Field lists (serde declaration order): block/mod.rs:114-119,175-187; block_kernel.rs:26-31;
// block_header.rs:39-57 with BlockPow = Pow<POW_MEMORY_TREE_HEIGHT> (pow.rs:33-37,187-199);
// block_body.rs:69-99; block_appendix.rs:31-33; transaction_kernel.rs:30-50;
// removal_record.rs:40-43; absolute_index_set.rs:32-39; chunk_dictionary.rs:27-33; chunk.rs:40-42;
// addition_record.rs:26-28; announcement.rs:34-36; mutator_set_accumulator.rs:32-36;
// active_window.rs:18-21; native_currency_amount.rs:50 (i128); difficulty_control.rs:43,238;
// guesser_receiver_data.rs:15-18; proof_collection.rs:36-49; neptune_proof.rs:42-44,193.
// crates.io types ([EXT], not vendored, unpinned): BFieldElement = its canonical u64 (reduced mod p
// on the way in, as BFieldElement::new), Digest = 5 of them, Claim = {program_digest, version: u32,
// input, output}, Proof = Vec<BFieldElement>, MmrAccumulator = {leaf_count: u64, peaks: Vec<Digest>},
// MmrMembershipProof = {authentication_path: Vec<Digest>}.
//
// BFieldCodec (the MAST sequences; transaction_kernel.rs:246-277, block_body.rs:175-182): struct
// fields last-first (pow.rs:196-197), dynamically sized fields length-prefixed, Vec = [len] + items
// (each prefixed when dynamic), tuples in order with the same rule, Option = [0] | [1] + value,
// u64 / u128 as u32 limbs low first [EXT, unpinned].  The test restatement is
// oracle/bincode_ref.py.
//
// The header chain (nhip_blk_header).  BlockHeader's MAST sequences (block_header.rs:204-215)
// are the BFieldCodec encodings of its eight fields: version, height, timestamp one word each, prev_block_digest
// five, pow.encode() = nonce ++ path_b ++ path_a ++ root (pow.rs:196-197; static sizes, no prefix),
// cumulative_proof_of_work six and difficulty five u32 limbs in array order, guesser_receiver_data =
// lock_script_hash ++ receiver_digest.  BlockKernel's (block_kernel.rs:112-119): header and body MAST hashes,
// then appendix.encode().  Block's (block/mod.rs:192-194): the kernel MAST hash, then proof.encode().  Pin
// status: the reversed field order and Claim's layout are pinned (pow.rs:196-197, new_claim.rs:38-100);
// BlockAppendix { claims } = [len] + Vec<Claim> with each claim length-prefixed, and the derived enum BlockProof
// = [variant index] + its fields (SingleProof's Proof length-prefixed, Proof = [n + 1, n, items]) follow
// bfieldcodec_derive's rules for structs and enums [EXT, unpinned].
//
// Everything is host code: parsing is byte-serial and a few hundred MB/s per thread is far above
// what a verifier batch consumes.
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/neptune_hip.h"
#include "blk_ms_parts.hpp"
#include "chain_rules.hpp"

namespace {
constexpr uint64_t P = 0xFFFFFFFF00000001ull;
constexpr uint32_t NUM_TRIALS = 45;  // util_types/mutator_set/shared.rs:15

struct Rd {
    const uint8_t* b;
    size_t n, o;
    bool ok = true;
    bool need(size_t k) {
        if (!ok || k > n - o) {
            ok = false;
            return false;
        }
        return true;
    }
    uint64_t le(int k) {
        if (!need((size_t)k)) return 0;
        uint64_t v = 0;
        for (int i = k - 1; i >= 0; --i) v = (v << 8) | b[o + i];
        o += (size_t)k;
        return v;
    }
    uint8_t u8() { return (uint8_t)le(1); }
    uint32_t u32() { return (uint32_t)le(4); }
    uint64_t u64() { return le(8); }
    uint64_t bfe() {
        const uint64_t v = u64();
        return v >= P ? v - P : v;
    }
    void u128(uint64_t& lo, uint64_t& hi) {
        lo = u64();
        hi = u64();
    }
    bool boolean() {
        const uint8_t v = u8();
        if (v > 1) ok = false;
        return v == 1;
    }
    // sequence length: every element takes at least `min_elem` bytes, so a length the rest of the
    // input cannot hold is rejected before anything is allocated or walked
    uint64_t len(size_t min_elem) {
        const uint64_t v = u64();
        if (ok && min_elem && v > (n - o) / min_elem) ok = false;
        return ok ? v : 0;
    }
    uint32_t variant(uint32_t count) {
        const uint32_t v = u32();
        if (v >= count) ok = false;
        return v;
    }
    void skip(size_t k) {
        if (need(k)) o += k;
    }
    void digest(uint64_t d[5]) {
        for (int i = 0; i < 5; ++i) d[i] = bfe();
    }
};

// BFieldCodec emitter; `mark` / `close` make a length prefix
struct Em {
    std::vector<uint64_t> w;
    size_t mark() {
        w.push_back(0);
        return w.size();
    }
    void close(size_t m) { w[m - 1] = w.size() - m; }
    void put(uint64_t v) { w.push_back(v); }
    void u64(uint64_t v) {
        w.push_back(v & 0xFFFFFFFFull);
        w.push_back(v >> 32);
    }
    void u128(uint64_t lo, uint64_t hi) {
        u64(lo);
        u64(hi);
    }
};

// ---- serde walkers; each also emits the field's BFieldCodec encoding when `e` is non-null
void vec_digests(Rd& r, Em* e) {  // Vec<Digest> (static items): [len] + digests
    const uint64_t n = r.len(40);
    if (e) e->put(n);
    for (uint64_t i = 0; i < n && r.ok; ++i)
        for (int q = 0; q < 5; ++q) {
            const uint64_t v = r.bfe();
            if (e) e->put(v);
        }
}

void vec_u32(Rd& r, Em* e) {
    const uint64_t n = r.len(4);
    if (e) e->put(n);
    for (uint64_t i = 0; i < n && r.ok; ++i) {
        const uint32_t v = r.u32();
        if (e) e->put(v);
    }
}

void vec_bfe(Rd& r, Em* e) {
    const uint64_t n = r.len(8);
    if (e) e->put(n);
    for (uint64_t i = 0; i < n && r.ok; ++i) {
        const uint64_t v = r.bfe();
        if (e) e->put(v);
    }
}

// MmrAccumulator {leaf_count, peaks}: BFieldCodec peaks (dynamic, prefixed) then leaf_count
void mmr_accumulator(Rd& r, Em* e) {
    const uint64_t leaf_count = r.u64();
    size_t m = e ? e->mark() : 0;
    vec_digests(r, e);
    if (e) {
        e->close(m);
        e->u64(leaf_count);
    }
}

// RemovalRecord {absolute_indices: {minimum: u128, distances: [u32; 45]}, target_chunks}
void removal_record(Rd& r, Em* e) {
    uint64_t lo, hi;
    r.u128(lo, hi);
    uint32_t dist[NUM_TRIALS];
    for (uint32_t i = 0; i < NUM_TRIALS; ++i) dist[i] = r.u32();
    // target_chunks (dynamic) first: [len(ChunkDictionary)] + [len(dictionary)] + Vec of tuples
    const size_t m_cd = e ? e->mark() : 0;
    const size_t m_dict = e ? e->mark() : 0;
    const uint64_t n = r.len(8 + 8 + 8);
    if (e) e->put(n);
    for (uint64_t i = 0; i < n && r.ok; ++i) {
        const size_t m_item = e ? e->mark() : 0;  // dynamic tuple item
        const uint64_t idx = r.u64();
        if (e) e->u64(idx);
        const size_t m_pair = e ? e->mark() : 0;   // (MmrMembershipProof, Chunk), dynamic
        const size_t m_mmp = e ? e->mark() : 0;    // MmrMembershipProof in the tuple
        const size_t m_path = e ? e->mark() : 0;   // its authentication_path field
        vec_digests(r, e);
        if (e) {
            e->close(m_path);
            e->close(m_mmp);
        }
        const size_t m_chunk = e ? e->mark() : 0;  // Chunk in the tuple
        const size_t m_rel = e ? e->mark() : 0;    // its relative_indices field
        vec_u32(r, e);
        if (e) {
            e->close(m_rel);
            e->close(m_chunk);
            e->close(m_pair);
            e->close(m_item);
        }
    }
    if (e) {
        e->close(m_dict);
        e->close(m_cd);
        for (uint32_t i = 0; i < NUM_TRIALS; ++i) e->put(dist[i]);  // absolute_indices, static
        e->u128(lo, hi);
    }
}

// TransactionKernel: emits its 8 MAST sequences, `ends[i]` = end of sequence i in e->w
void tx_kernel(Rd& r, Em* e, size_t ends[8]) {
    auto end = [&](int i) {
        if (e) ends[i] = e->w.size();
    };
    uint64_t n = r.len(16 + 4 * NUM_TRIALS + 8);  // inputs: Vec<RemovalRecord> (dynamic items)
    if (e) e->put(n);
    for (uint64_t i = 0; i < n && r.ok; ++i) {
        const size_t m = e ? e->mark() : 0;
        removal_record(r, e);
        if (e) e->close(m);
    }
    end(0);
    vec_digests(r, e);  // outputs: Vec<AdditionRecord{canonical_commitment}>
    end(1);
    n = r.len(8);  // announcements: Vec<Announcement{message}>
    if (e) e->put(n);
    for (uint64_t i = 0; i < n && r.ok; ++i) {
        const size_t m_item = e ? e->mark() : 0;
        const size_t m_msg = e ? e->mark() : 0;
        vec_bfe(r, e);
        if (e) {
            e->close(m_msg);
            e->close(m_item);
        }
    }
    end(2);
    uint64_t lo, hi;
    r.u128(lo, hi);  // fee: NativeCurrencyAmount(i128)
    if (e) e->u128(lo, hi);
    end(3);
    const uint8_t tag = r.u8();  // coinbase: Option<NativeCurrencyAmount>
    if (tag > 1) r.ok = false;
    if (e) e->put(tag);
    if (tag == 1) {
        r.u128(lo, hi);
        if (e) e->u128(lo, hi);
    }
    end(4);
    const uint64_t ts = r.bfe();  // timestamp
    if (e) e->put(ts);
    end(5);
    uint64_t d[5];
    r.digest(d);  // mutator_set_hash
    if (e)
        for (int q = 0; q < 5; ++q) e->put(d[q]);
    end(6);
    const bool mb = r.boolean();  // merge_bit
    if (e) e->put(mb ? 1 : 0);
    end(7);
}

void claim_skip(Rd& r) {
    r.skip(40 + 4);
    r.skip(8 * r.len(8));
    r.skip(8 * r.len(8));
}

// Walk one block at r.o.  With `e`, emit the kernel's 8 and the body's 3 tail sequences.
bool parse_block(Rd& r, uint32_t tree_height, nhip_blk_block& b, Em* e, size_t ends[11]) {
    std::memset(&b, 0, sizeof(b));
    b.offset = r.o;
    r.bfe();  // version
    b.height = r.bfe();
    r.digest(b.prev_block_digest);
    b.timestamp = r.bfe();
    // pow: root, path_a, path_b, nonce; cumulative_proof_of_work [u32; 6]; difficulty [u32; 5];
    // guesser_receiver_data: 2 digests
    r.skip(40ull * (2ull * tree_height + 2) + 4 * 6 + 4 * 5 + 80);
    b.kernel_offset = r.o;
    size_t k_ends[8] = {};
    tx_kernel(r, e, k_ends);
    if (e)
        for (int i = 0; i < 8; ++i) ends[i] = k_ends[i];
    // body: mutator_set_accumulator {aocl, swbf_inactive, swbf_active{sbf: Vec<u32>}} -- BFieldCodec
    // fields last-first, so the three parts are emitted into scratch and concatenated reversed
    {
        Em parts[3];
        mmr_accumulator(r, e ? &parts[0] : nullptr);
        mmr_accumulator(r, e ? &parts[1] : nullptr);
        {
            Em* pe = e ? &parts[2] : nullptr;
            const size_t m = pe ? pe->mark() : 0;
            vec_u32(r, pe);
            if (pe) pe->close(m);
        }
        if (e) {
            for (int i = 2; i >= 0; --i) {
                e->put(parts[i].w.size());
                e->w.insert(e->w.end(), parts[i].w.begin(), parts[i].w.end());
            }
            ends[8] = e->w.size();
        }
    }
    mmr_accumulator(r, e);  // lock_free_mmr_accumulator
    if (e) ends[9] = e->w.size();
    mmr_accumulator(r, e);  // block_mmr_accumulator
    if (e) ends[10] = e->w.size();
    // appendix
    b.appendix_offset = r.o;
    const uint64_t nc = r.len(40 + 4 + 16);
    uint64_t claim_words = 0;
    for (uint64_t i = 0; i < nc && r.ok; ++i) {
        const size_t o0 = r.o;
        claim_skip(r);
        claim_words += (r.o - o0 - 44 - 16) / 8;
    }
    b.n_claims = (uint32_t)nc;
    b.claim_words = claim_words;
    if (nc > 0xFFFFFFFFull) r.ok = false;
    // proof
    b.proof_kind = r.variant(3);
    if (r.ok && b.proof_kind == NHIP_BLOCK_PROOF_SINGLE) {
        b.proof_len = r.len(8);
        b.proof_offset = r.o;
        r.skip(8 * b.proof_len);
    }
    b.size = r.o - b.offset;
    return r.ok;
}

uint64_t rd_word(const uint8_t* p) {
    uint64_t v;
    std::memcpy(&v, p, 8);  // little-endian host (x86-64 / the MI355X hosts)
    return v >= P ? v - P : v;
}
}  // namespace

extern "C" {

int nhip_blk_scan(const uint8_t* bytes, size_t n_bytes, uint32_t pow_tree_height, nhip_blk_block* blocks,
                  size_t cap, size_t* n_blocks) {
    if (!n_blocks || (n_bytes && !bytes) || pow_tree_height > 64) return NHIP_ERR_ARG;
    *n_blocks = 0;
    try {
        Rd r{bytes, n_bytes, 0};
        Em e;
        size_t ends[11];
        size_t count = 0;
        while (r.o < n_bytes) {
            nhip_blk_block b;
            e.w.clear();
            if (!parse_block(r, pow_tree_height, b, blocks ? &e : nullptr, ends)) {
                *n_blocks = count;  // blocks before the malformed one
                return NHIP_ERR_DECODE;
            }
            b.seq_words = blocks ? e.w.size() : 0;
            if (blocks) {
                if (count >= cap) return NHIP_ERR_ARG;
                blocks[count] = b;
            }
            ++count;
        }
        *n_blocks = count;
        return NHIP_OK;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

int nhip_blk_sequences(const uint8_t* bytes, size_t n_bytes, uint32_t pow_tree_height, const nhip_blk_block* block,
                       uint64_t* words, size_t cap, uint64_t offsets[12]) {
    if (!bytes || !block || !offsets || block->offset > n_bytes || pow_tree_height > 64) return NHIP_ERR_ARG;
    try {
        Rd r{bytes, n_bytes, (size_t)block->offset};
        Em e;
        size_t ends[11];
        nhip_blk_block b;
        if (!parse_block(r, pow_tree_height, b, &e, ends)) return NHIP_ERR_DECODE;
        offsets[0] = 0;
        for (int i = 0; i < 11; ++i) offsets[i + 1] = ends[i];
        if (!words) return NHIP_OK;  // size query: offsets[11]
        if (cap < e.w.size()) return NHIP_ERR_ARG;
        std::memcpy(words, e.w.data(), e.w.size() * 8);
        return NHIP_OK;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

int nhip_blk_claims(const uint8_t* bytes, size_t n_bytes, const nhip_blk_block* block, uint64_t* words,
                    nhip_claim* claims) {
    if (!bytes || !block || block->appendix_offset > n_bytes || (block->claim_words && !words) ||
        (block->n_claims && !claims))
        return NHIP_ERR_ARG;
    Rd r{bytes, n_bytes, (size_t)block->appendix_offset};
    const uint64_t nc = r.len(40 + 4 + 16);
    if (!r.ok || nc != block->n_claims) return NHIP_ERR_DECODE;
    uint64_t used = 0;
    for (uint64_t i = 0; i < nc; ++i) {
        nhip_claim& c = claims[i];
        r.digest(c.program_digest);
        c.version = r.u32();
        for (int side = 0; side < 2; ++side) {
            const uint64_t n = r.len(8);
            if (!r.ok || used + n > block->claim_words) return NHIP_ERR_DECODE;
            uint64_t* dst = words + used;
            for (uint64_t k = 0; k < n; ++k) dst[k] = r.bfe();
            (side == 0 ? c.input : c.output) = dst;
            (side == 0 ? c.input_len : c.output_len) = (size_t)n;
            used += n;
        }
        if (!r.ok) return NHIP_ERR_DECODE;
    }
    return NHIP_OK;
}

// One walk of the block at `offset` for what the chain rules and Block::hash read (header comment: "header
// chain"): *out, and the appendix encoding followed by the proof encoding's prefix appended to w (w is left as it
// was on a decode error).  May throw std::bad_alloc.
static int blk_header_walk(const uint8_t* bytes, size_t n_bytes, uint32_t pow_tree_height, uint64_t offset,
                           nhip_blk_header_out* out, std::vector<uint64_t>& w) {
    Rd r{bytes, n_bytes, (size_t)offset};
    std::memset(out, 0, sizeof(*out));
    out->version = r.bfe();
    out->height = r.bfe();
    r.digest(out->prev_block_digest);
    out->timestamp = r.bfe();
    r.digest(out->pow_root);
    out->path_a_offset = r.o;
    r.skip(40ull * pow_tree_height);
    out->path_b_offset = r.o;
    r.skip(40ull * pow_tree_height);
    r.digest(out->pow_nonce);
    for (int i = 0; i < 6; ++i) out->cumulative_proof_of_work[i] = r.u32();
    for (int i = 0; i < 5; ++i) out->difficulty[i] = r.u32();
    r.digest(out->receiver_digest);
    r.digest(out->lock_script_hash);
    size_t k_ends[8];
    tx_kernel(r, nullptr, k_ends);
    mmr_accumulator(r, nullptr);  // aocl
    mmr_accumulator(r, nullptr);  // swbf_inactive
    vec_u32(r, nullptr);          // swbf_active
    mmr_accumulator(r, nullptr);  // lock_free_mmr_accumulator
    out->mmr_num_leafs = r.u64();  // block_mmr_accumulator
    const uint64_t np = r.len(40);
    out->mmr_n_peaks = (uint32_t)std::min<uint64_t>(np, 65);
    for (uint64_t i = 0; i < np && r.ok; ++i) {
        uint64_t d[5];
        r.digest(d);
        if (i < 64) std::memcpy(out->mmr_peaks[i], d, 40);
    }
    // BlockAppendix { claims: Vec<Claim> }: [len] + ([n] + per claim [len] + Claim), Claim last-first
    // (new_claim.rs:38-100): output, input (each [len + 1, len, items]), version, program_digest
    Em e;
    e.w.swap(w);  // append to the caller's words
    const size_t w0 = e.w.size();
    const size_t m_field = e.mark();
    const uint64_t nc = r.len(40 + 4 + 16);
    e.put(nc);
    for (uint64_t i = 0; i < nc && r.ok; ++i) {
        uint64_t pd[5];
        r.digest(pd);
        const uint32_t version = r.u32();
        Em in;
        vec_bfe(r, &in);
        const size_t m_claim = e.mark();
        const size_t m_out = e.mark();
        vec_bfe(r, &e);
        e.close(m_out);
        e.put(in.w.size());
        e.w.insert(e.w.end(), in.w.begin(), in.w.end());
        e.put(version);
        for (int q = 0; q < 5; ++q) e.put(pd[q]);
        e.close(m_claim);
    }
    e.close(m_field);
    out->appendix_words = e.w.size() - w0;
    // BlockProof (derived enum): [discriminant], then SingleProof's field Proof(Vec<BFieldElement>),
    // dynamic, so prefixed: [n + 2], Proof = [n + 1] + Vec = [n] + items
    const uint32_t kind = r.variant(3);
    e.put(kind);
    if (r.ok && kind == NHIP_BLOCK_PROOF_SINGLE) {
        const uint64_t n = r.len(8);
        e.put(n + 2);
        e.put(n + 1);
        e.put(n);
        out->proof_offset = r.o;
        out->proof_len = n;
        r.skip(8 * n);
    }
    e.w.swap(w);
    if (!r.ok) {
        w.resize(w0);
        return NHIP_ERR_DECODE;
    }
    out->prefix_words = w.size() - w0 - out->appendix_words;
    return NHIP_OK;
}

int nhip_blk_header(const uint8_t* bytes, size_t n_bytes, uint32_t pow_tree_height, const nhip_blk_block* block,
                    nhip_blk_header_out* out, uint64_t* words, size_t cap) {
    if (!bytes || !block || !out || block->offset > n_bytes || pow_tree_height > 64) return NHIP_ERR_ARG;
    try {
        std::vector<uint64_t> w;
        const int rc = blk_header_walk(bytes, n_bytes, pow_tree_height, block->offset, out, w);
        if (rc) return rc;
        if (!words) return NHIP_OK;  // size query
        if (cap < w.size()) return NHIP_ERR_ARG;
        std::memcpy(words, w.data(), w.size() * 8);
        return NHIP_OK;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

int nhip_difficulty_target(const uint32_t difficulty[5], uint64_t target_out[5]) {
    if (!difficulty || !target_out) return NHIP_ERR_ARG;
    return nhip::chain::difficulty_target(difficulty, target_out) ? NHIP_OK : NHIP_ERR_ARG;
}

int nhip_difficulty_control(uint64_t new_timestamp, uint64_t old_timestamp, const uint32_t old_difficulty[5],
                            uint64_t target_block_interval, uint64_t previous_block_height, uint32_t difficulty_out[5]) {
    if (!old_difficulty || !difficulty_out) return NHIP_ERR_ARG;
    return nhip::chain::difficulty_control(new_timestamp % P, old_timestamp % P, old_difficulty, target_block_interval % P,
                                           previous_block_height % P, difficulty_out)
               ? NHIP_OK
               : NHIP_ERR_ARG;
}

int nhip_le_words(const uint8_t* bytes, size_t n_bytes, uint64_t offset, size_t n, uint64_t* out) {
    if ((n && (!bytes || !out)) || offset > n_bytes || n > (n_bytes - offset) / 8) return NHIP_ERR_ARG;
    for (size_t i = 0; i < n; ++i) out[i] = rd_word(bytes + offset + 8 * i);
    return NHIP_OK;
}

// ---- TransferTransaction
static bool parse_tx(Rd& r, nhip_tx* t, Em* e, size_t ends[8], uint64_t* spans, uint64_t* digests) {
    std::memset(t, 0, sizeof(*t));
    tx_kernel(r, e, ends);
    t->kind = r.variant(2);
    if (!r.ok) return false;
    if (t->kind == NHIP_TX_SINGLE_PROOF) {
        const uint64_t n = r.len(8);
        if (spans) {
            spans[0] = r.o;
            spans[1] = n;
        }
        r.skip(8 * n);
        t->n_proofs = 1;
    } else {
        // removal_records_integrity, collect_lock_scripts, lock_scripts_halt, kernel_to_outputs,
        // collect_type_scripts, type_scripts_halt (proof_collection.rs:36-49 field order)
        uint32_t np = 0;
        auto proof = [&]() {
            const uint64_t n = r.len(8);
            if (spans) {
                spans[2 * np] = r.o;
                spans[2 * np + 1] = n;
            }
            r.skip(8 * n);
            ++np;
        };
        proof();
        proof();
        uint64_t nl = r.len(8);
        for (uint64_t i = 0; i < nl && r.ok; ++i) proof();
        proof();
        proof();
        uint64_t nt = r.len(8);
        for (uint64_t i = 0; i < nt && r.ok; ++i) proof();
        t->n_lock_scripts = (uint32_t)nl;
        t->n_type_scripts = (uint32_t)nt;
        t->n_proofs = np;
        uint64_t nd = 0;
        auto digs = [&](uint64_t cnt) {
            for (uint64_t i = 0; i < cnt && r.ok; ++i) {
                uint64_t d[5];
                r.digest(d);
                if (digests) std::memcpy(digests + 5 * nd, d, 40);
                ++nd;
            }
        };
        t->n_lock_hashes = (uint32_t)r.len(40);
        digs(t->n_lock_hashes);
        t->n_type_hashes = (uint32_t)r.len(40);
        digs(t->n_type_hashes);
        digs(3);  // kernel_mast_hash, salted_inputs_hash, salted_outputs_hash
        t->n_merge_path = (uint32_t)r.len(40);
        digs(t->n_merge_path);
        t->n_digests = nd;
    }
    t->size = r.o;
    if (e) t->seq_words = e->w.size();
    return r.ok;
}

int nhip_tx_scan(const uint8_t* bytes, size_t n_bytes, nhip_tx* tx) {
    if (!tx || (n_bytes && !bytes)) return NHIP_ERR_ARG;
    try {
        Rd r{bytes, n_bytes, 0};
        Em e;
        size_t ends[8];
        return parse_tx(r, tx, &e, ends, nullptr, nullptr) ? NHIP_OK : NHIP_ERR_DECODE;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

int nhip_tx_parts(const uint8_t* bytes, size_t n_bytes, const nhip_tx* tx, uint64_t* seq_words,
                  uint64_t seq_offsets[9], uint64_t* proof_spans, uint64_t* digests) {
    if (!tx || !bytes || !seq_words || !seq_offsets || !proof_spans || (tx->n_digests && !digests))
        return NHIP_ERR_ARG;
    try {
        Rd r{bytes, n_bytes, 0};
        Em e;
        size_t ends[8];
        nhip_tx t;
        // the caller's buffers are sized from tx (a scan of the same bytes); re-check before copying
        std::vector<uint64_t> spans(2ull * tx->n_proofs + 2), dig(5ull * tx->n_digests + 5);
        Rd probe{bytes, n_bytes, 0};
        if (!parse_tx(probe, &t, nullptr, ends, nullptr, nullptr)) return NHIP_ERR_DECODE;
        if (t.n_proofs != tx->n_proofs || t.n_digests != tx->n_digests) return NHIP_ERR_ARG;
        if (!parse_tx(r, &t, &e, ends, spans.data(), dig.data())) return NHIP_ERR_DECODE;
        if (t.seq_words != tx->seq_words) return NHIP_ERR_ARG;
        seq_offsets[0] = 0;
        for (int i = 0; i < 8; ++i) seq_offsets[i + 1] = ends[i];
        std::memcpy(seq_words, e.w.data(), e.w.size() * 8);
        std::memcpy(proof_spans, spans.data(), 16ull * t.n_proofs);
        if (t.n_digests) std::memcpy(digests, dig.data(), 40ull * t.n_digests);
        return NHIP_OK;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

}  // extern "C"

namespace nhip {
// The proof spans of the TransferTransaction at the start of bytes[0, n) (arena.cpp): (byte offset
// from `bytes`, words) per proof in ProofCollection field order, appended to `spans`, and its size.
bool tx_proof_spans(const uint8_t* bytes, size_t n, std::vector<uint64_t>& spans, uint64_t& size) {
    size_t ends[8];
    nhip_tx t;
    Rd probe{bytes, n, 0};
    if (!parse_tx(probe, &t, nullptr, ends, nullptr, nullptr)) return false;  // sizes first
    const size_t base = spans.size();
    spans.resize(base + 2ull * t.n_proofs);
    Rd r{bytes, n, 0};
    if (!parse_tx(r, &t, nullptr, ends, spans.data() + base, nullptr)) return false;
    size = t.size;
    return true;
}

// chain_capi.hip's host decode, one walk each per block: nhip_blk_header's fields with its words appended to w,
// and nhip_blk_sequences' words (replacing `words`, whose capacity is reused) and offsets.  May throw
// std::bad_alloc.
int blk_header_append(const uint8_t* bytes, size_t n_bytes, uint32_t pow_tree_height, uint64_t offset,
                      nhip_blk_header_out* out, std::vector<uint64_t>& w) {
    return blk_header_walk(bytes, n_bytes, pow_tree_height, offset, out, w);
}
int blk_sequences_into(const uint8_t* bytes, size_t n_bytes, uint32_t pow_tree_height, uint64_t offset,
                       std::vector<uint64_t>& words, uint64_t offsets[12]) {
    Rd r{bytes, n_bytes, (size_t)offset};
    Em e;
    e.w.swap(words);
    e.w.clear();
    size_t ends[11];
    nhip_blk_block b;
    const bool ok = parse_block(r, pow_tree_height, b, &e, ends);
    e.w.swap(words);
    if (!ok) return NHIP_ERR_DECODE;
    offsets[0] = 0;
    for (int i = 0; i < 11; ++i) offsets[i + 1] = ends[i];
    return NHIP_OK;
}
}  // namespace nhip

// ---- the mutator-set and transaction parts of a block: integers and byte copies only
namespace {
// MmrAccumulator into 64 peak slots; the count as serialized, saturated at 65 (as nhip_blk_header's mmr_n_peaks)
void mmr_parts(Rd& r, uint64_t& num_leafs, uint32_t& n_peaks, std::vector<uint64_t>& slots) {
    num_leafs = r.u64();
    const uint64_t np = r.len(40);
    n_peaks = (uint32_t)std::min<uint64_t>(np, 65);
    const size_t at = slots.size();
    slots.resize(at + 64 * 5, 0);
    for (uint64_t i = 0; i < np && r.ok; ++i) {
        uint64_t d[5];
        r.digest(d);
        if (i < 64) std::memcpy(slots.data() + at + 5 * i, d, 40);
    }
}
}  // namespace

namespace nhip {
int blk_ms_walk_block(const uint8_t* bytes, size_t n_bytes, uint32_t pow_tree_height, uint64_t offset, BlkMsParts& p) {
    Rd r{bytes, n_bytes, (size_t)offset};
    BlkMsParts b;  // this block alone: p is touched only once it has parsed
    r.bfe();       // version
    b.height.push_back(r.bfe());
    r.skip(40);  // prev_block_digest
    b.timestamp.push_back(r.bfe());
    // pow: root, path_a, path_b, nonce; cumulative_proof_of_work [u32; 6]; difficulty [u32; 5]
    r.skip(40ull * (2ull * pow_tree_height + 2) + 4 * 6 + 4 * 5);
    uint64_t d[5];
    r.digest(d);
    b.receiver_digest.assign(d, d + 5);
    r.digest(d);
    b.lock_script_hash.assign(d, d + 5);
    // transaction kernel: inputs as they lie (the packed reading of §6f), outputs, announcements, fee, coinbase, timestamp
    const uint64_t n_in = r.len(16 + 4 * NUM_TRIALS + 8);
    for (uint64_t i = 0; i < n_in && r.ok; ++i) {
        uint64_t lo, hi;
        r.u128(lo, hi);
        b.minimum.push_back(lo);
        b.minimum.push_back(hi);
        for (uint32_t k = 0; k < NUM_TRIALS; ++k) b.distances.push_back(r.u32());
        const uint64_t n_ent = r.len(8 + 8 + 8);
        for (uint64_t e = 0; e < n_ent && r.ok; ++e) {
            b.chunk_index.push_back(r.u64());
            const uint64_t np = r.len(40);
            for (uint64_t k = 0; k < np && r.ok; ++k) {
                r.digest(d);
                b.path.insert(b.path.end(), d, d + 5);
            }
            b.path_off.push_back(b.path.size() / 5);
            const uint64_t nr = r.len(4);
            for (uint64_t k = 0; k < nr && r.ok; ++k) b.rel.push_back(r.u32());
            b.rel_off.push_back(b.rel.size());
        }
        b.entry_off.push_back(b.chunk_index.size());
    }
    const uint64_t n_out = r.len(40);
    for (uint64_t i = 0; i < n_out && r.ok; ++i) {
        r.digest(d);
        b.outputs.insert(b.outputs.end(), d, d + 5);
    }
    const uint64_t n_ann = r.len(8);
    for (uint64_t i = 0; i < n_ann && r.ok; ++i) r.skip(8 * r.len(8));
    b.n_announcements.push_back(n_ann);
    uint64_t lo, hi;
    r.u128(lo, hi);
    b.fee = {lo, hi};
    const uint8_t tag = r.u8();
    if (tag > 1) r.ok = false;
    lo = hi = 0;
    if (tag == 1) r.u128(lo, hi);
    b.coinbase_tag.push_back(tag);
    b.coinbase = {lo, hi};
    b.kernel_timestamp.push_back(r.bfe());
    r.skip(40);    // mutator_set_hash
    r.boolean();   // merge_bit
    // body: mutator_set_accumulator {aocl, swbf_inactive, swbf_active {sbf}}
    uint64_t nl;
    uint32_t np;
    mmr_parts(r, nl, np, b.aocl_peaks);
    b.aocl_num_leafs.push_back(nl);
    b.aocl_n_peaks.push_back(np);
    mmr_parts(r, nl, np, b.swbf_peaks);
    b.swbf_num_leafs.push_back(nl);
    b.swbf_n_peaks.push_back(np);
    const uint64_t na = r.len(4);
    for (uint64_t i = 0; i < na && r.ok; ++i) b.active.push_back(r.u32());
    // the rest of the block must parse too: a block that nhip_blk_scan refuses is refused here
    mmr_accumulator(r, nullptr);  // lock_free_mmr_accumulator
    mmr_accumulator(r, nullptr);  // block_mmr_accumulator
    const uint64_t nc = r.len(40 + 4 + 16);
    for (uint64_t i = 0; i < nc && r.ok; ++i) claim_skip(r);
    const uint32_t kind = r.variant(3);
    if (r.ok && kind == NHIP_BLOCK_PROOF_SINGLE) r.skip(8 * r.len(8));
    if (!r.ok) return NHIP_ERR_DECODE;

    auto cat = [](auto& dst, const auto& src) { dst.insert(dst.end(), src.begin(), src.end()); };
    auto cat_off = [](std::vector<uint64_t>& dst, const std::vector<uint64_t>& src) {  // src[0] == 0 is dst's last
        const uint64_t base = dst.back();
        for (size_t k = 1; k < src.size(); ++k) dst.push_back(base + src[k]);
    };
    cat(p.height, b.height);
    cat(p.timestamp, b.timestamp);
    cat(p.receiver_digest, b.receiver_digest);
    cat(p.lock_script_hash, b.lock_script_hash);
    cat(p.fee, b.fee);
    cat(p.coinbase, b.coinbase);
    cat(p.coinbase_tag, b.coinbase_tag);
    cat(p.kernel_timestamp, b.kernel_timestamp);
    cat(p.n_announcements, b.n_announcements);
    cat(p.aocl_num_leafs, b.aocl_num_leafs);
    cat(p.swbf_num_leafs, b.swbf_num_leafs);
    cat(p.aocl_n_peaks, b.aocl_n_peaks);
    cat(p.swbf_n_peaks, b.swbf_n_peaks);
    cat(p.aocl_peaks, b.aocl_peaks);
    cat(p.swbf_peaks, b.swbf_peaks);
    cat(p.active, b.active);
    p.active_off.push_back(p.active.size());
    cat(p.outputs, b.outputs);
    p.out_off.push_back(p.outputs.size() / 5);
    cat(p.minimum, b.minimum);
    cat(p.distances, b.distances);
    p.rec_off.push_back(p.minimum.size() / 2);
    cat_off(p.entry_off, b.entry_off);
    cat_off(p.path_off, b.path_off);
    cat_off(p.rel_off, b.rel_off);
    cat(p.chunk_index, b.chunk_index);
    cat(p.path, b.path);
    cat(p.rel, b.rel);
    ++p.n;
    return NHIP_OK;
}
}  // namespace nhip

// ---- in-place scanners: where the proofs lie in the wire bytes, no word copied
extern "C" {

int nhip_wire_scan_txs(const uint8_t* bytes, size_t n_bytes, size_t max_txs, nhip_span* spans, size_t span_cap,
                       size_t* n_txs, size_t* n_proofs, size_t* consumed) {
    if (n_txs) *n_txs = 0;
    if (n_proofs) *n_proofs = 0;
    if (consumed) *consumed = 0;
    if ((n_bytes && !bytes) || (span_cap && !spans)) return NHIP_ERR_ARG;
    try {
        std::vector<uint64_t> sp;
        size_t pos = 0, txs = 0, placed = 0;
        int rc = NHIP_OK;
        while (pos < n_bytes && txs < max_txs) {
            sp.clear();
            uint64_t size = 0;
            if (!nhip::tx_proof_spans(bytes + pos, n_bytes - pos, sp, size)) {
                rc = NHIP_ERR_DECODE;  // the transactions before it stay counted
                break;
            }
            const size_t np = sp.size() / 2;
            if (placed + np > span_cap) {
                // the span array is full: stop before this tx; a first tx that can never fit is the
                // caller's error, not an empty success to loop on
                if (txs == 0) rc = NHIP_ERR_ARG;
                break;
            }
            for (size_t i = 0; i < np; ++i) spans[placed + i] = nhip_span{sp[2 * i] + pos, sp[2 * i + 1]};
            placed += np;
            pos += size;
            ++txs;
        }
        if (n_txs) *n_txs = txs;
        if (n_proofs) *n_proofs = placed;
        if (consumed) *consumed = pos;
        return rc;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

int nhip_wire_scan_blocks(const uint8_t* bytes, size_t n_bytes, uint32_t pow_tree_height, nhip_span* spans,
                          uint64_t* block_of, size_t span_cap, size_t* n_proofs, size_t* n_blocks) {
    if (n_proofs) *n_proofs = 0;
    if (n_blocks) *n_blocks = 0;
    if ((n_bytes && !bytes) || (span_cap && !spans)) return NHIP_ERR_ARG;
    try {
        size_t nb = 0;
        int rc = nhip_blk_scan(bytes, n_bytes, pow_tree_height, nullptr, 0, &nb);
        if (rc) {
            if (n_blocks) *n_blocks = nb;
            return rc;  // a malformed block fails the whole file (import_blocks_from_files.rs:100-115)
        }
        std::vector<nhip_blk_block> blocks(std::max<size_t>(nb, 1));
        rc = nhip_blk_scan(bytes, n_bytes, pow_tree_height, blocks.data(), nb, &nb);
        if (rc) return rc;
        size_t singles = 0;
        for (size_t b = 0; b < nb; ++b) singles += blocks[b].proof_kind == NHIP_BLOCK_PROOF_SINGLE ? 1 : 0;
        if (singles > span_cap) return NHIP_ERR_ARG;
        size_t placed = 0;
        for (size_t b = 0; b < nb; ++b)
            if (blocks[b].proof_kind == NHIP_BLOCK_PROOF_SINGLE) {
                spans[placed] = nhip_span{blocks[b].proof_offset, blocks[b].proof_len};
                if (block_of) block_of[placed] = b;
                ++placed;
            }
        if (n_proofs) *n_proofs = placed;
        if (n_blocks) *n_blocks = nb;
        return NHIP_OK;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

}  // extern "C"
