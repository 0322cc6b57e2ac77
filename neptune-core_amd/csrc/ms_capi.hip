// C-ABI layer of libneptune_hip.so, the mutator-set entry points (declarations: include/neptune_hip.h;
// DESIGN.md §6c-§6g).  Each is: validate shapes, stage order (both ms_shape.cpp), build its parts, one Stage
// (ctx.hpp: declare the device buffers, commit, launch, read back), write the outputs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "ctx.hpp"
#include "kernels.hpp"
#include "ms_shape.hpp"
#include "ms_update_plan.hpp"

using nhip::Stage;

namespace {

const nhip_ms_chunks NO_CHUNKS{};  // no owner: the caller's dictionaries may be absent

// The six buffers of n owners' flattened dictionaries (counts from ms_chunks_ok), in the order every call stages them.
// With filled_by the paths are not uploaded: their buffer is that program's output (UnpackProgram::enqueue binds d.path).
void stage_chunks(Stage& st, const nhip_ms_chunks& ch, size_t n, const nhip::MsChunkCounts& cc, nhip::MsChunksDev& d,
                  nhip::MsUnpackDev* filled_by = nullptr) {
    const size_t E = (size_t)cc.entries;
    st.in(d.entry_off, ch.entry_off, n ? n + 1 : 0);
    st.in(d.chunk_index, ch.chunk_index, E);
    st.in(d.path_off, ch.path_off, n ? E + 1 : 0);
    if (filled_by) st.tmp(filled_by->path_out, (size_t)cc.path_digests, 5);
    else st.in(d.path, ch.path, (size_t)cc.path_digests, 5);
    st.in(d.rel_off, ch.rel_off, n ? E + 1 : 0);
    st.in(d.rel, ch.rel, (size_t)cc.rel_words);
}

// The packed-list prologue of a call: the device program of a host plan (ms_unpack_plan.hpp), the u32
// and the u64 arrays in one pool each, so that a call spends six buffers on it (arena included).
struct UnpackProgram {
    const nhip::MsUnpackPlan& p;
    const nhip_ms_chunks& packed;   // the input's dictionaries, and their counts from ms_chunks_ok
    const nhip::MsChunkCounts& cc;
    std::vector<uint32_t> w32;
    std::vector<uint64_t> w64;
    const uint32_t* d32 = nullptr;
    const uint64_t* d64 = nullptr;
    nhip::MsUnpackDev u{};  // path_out: declared by whoever owns the unpacked paths (nhip_ms_unpack_batch, stage_chunks)
    UnpackProgram(const nhip::MsUnpackPlan& plan, const nhip_ms_chunks& packed_in, const nhip::MsChunkCounts& counts)
        : p(plan), packed(packed_in), cc(counts) {
        for (const std::vector<uint32_t>* v : {&p.leaf_slot, &p.leaf_cnt, &p.copy_slot, &p.op, &p.gath_src})
            w32.insert(w32.end(), v->begin(), v->end());
        for (const std::vector<uint64_t>* v : {&p.leaf_words, &p.copy_src, &p.lvl}) w64.insert(w64.end(), v->begin(), v->end());
    }
    void declare(Stage& st) {
        st.in(u.jobs, p.jobs.data(), p.jobs.size());
        st.in(d32, w32.data(), w32.size());
        st.in(d64, w64.data(), w64.size());
        st.in(u.path_in, packed.path, (size_t)cc.path_digests, 5);
        st.in(u.rel_in, packed.rel, (size_t)cc.rel_words);
        st.tmp(u.arena, (size_t)p.n_slots, 5);
    }
    // after commit(); reader: the dictionaries that read the unpacked paths
    void enqueue(Stage& st, nhip_ctx* c, size_t n_jobs, nhip::MsChunksDev* reader = nullptr) {
        u.leaf_slot = d32;
        u.leaf_cnt = u.leaf_slot + p.leaf_slot.size();
        u.copy_slot = u.leaf_cnt + p.leaf_cnt.size();
        u.op = u.copy_slot + p.copy_slot.size();
        u.gath_src = u.op + p.op.size();
        u.leaf_words = d64;
        u.copy_src = u.leaf_words + p.leaf_words.size();
        u.lvl = u.copy_src + p.copy_src.size();
        if (reader) reader->path = u.path_out;
        st.launch([&] { return nhip::launch_ms_unpack(u, n_jobs, c->stream); });
    }
};

// The block's part of a call: what nhip_ms_apply_batch stages, launches and reads back for jobs that
// passed ms_apply_ok (n_jobs != 0).  With `unpack`, in.chunks is the plan's unpacked shape without paths, and the
// prologue fills them on the device first.  With keep_nodes, k_ms_apply keeps its nodes for a WitnessPart behind it.
struct BlockPart {
    const nhip_ms_apply_in& in;
    nhip_ms_apply_out& out;
    const nhip::MsApplyCounts& cnt;
    const bool keep_nodes;
    UnpackProgram* const unpack;
    const size_t n, R, E;
    nhip::MsApplyOrder o;
    nhip::MsApplyDev a{};  // rec.aocl_member null: the records as can_remove decides them
    const uint32_t* d_entry_rec = nullptr;  // k_ms_chunk_auth_jobs alone reads it and writes d_auth
    uint8_t* d_auth = nullptr;
    // read back into temporaries first: the outputs stay untouched unless the whole call succeeds
    std::vector<uint8_t> vs;
    std::vector<uint64_t> bad;

    BlockPart(const nhip_ms_apply_in& in_, nhip_ms_apply_out& out_, const nhip::MsApplyCounts& counts, bool keep,
              UnpackProgram* prologue = nullptr)
        : in(in_), out(out_), cnt(counts), keep_nodes(keep), unpack(prologue), n(in_.n_jobs), R((size_t)counts.records),
          E((size_t)counts.chunks.entries), vs(2 * n), bad(n) {
        nhip::ms_apply_order(&in, &out, cnt, &o, keep_nodes);
        a.has_expected = in.msa_expected ? 1 : 0;
    }
    void declare(Stage& st) {
        st.in(a.jobs, o.jobs.data(), n);
        st.in(a.peaks, o.peaks.data(), o.peaks.size());
        st.in(a.active, o.active.data(), o.active.size());
        st.in(a.additions, in.additions, (size_t)cnt.additions, 5);
        st.in(a.rec.minimum, in.minimum, R, 2);
        st.in(a.rec.distances, in.distances, R, 45);
        stage_chunks(st, R ? *in.chunks : NO_CHUNKS, R, cnt.chunks, a.rec.ch, unpack ? &unpack->u : nullptr);
        if (unpack) unpack->declare(st);
        st.in(a.rec_job, o.rec_job.data(), R);
        st.in(d_entry_rec, o.entry_rec.data(), E);
        st.in(a.idx_perm, o.idx_perm.data(), R, 45);
        st.in(a.grp, o.grp.data(), o.grp.size());
        st.in(a.rec_perm, o.rec_perm.data(), R);
        st.in(a.exp_active, o.exp_active.data(), o.exp_active.size());
        st.tmp(d_auth, E);
        st.tmp(a.rec.valid, R, 3);  // per record: valid, verdict, status
        st.tmp(a.index_set, R, 45);
        st.tmp(a.dig, (size_t)o.dig_total, 5);
        st.tmp(a.aux, (size_t)o.grp_total, 2);
        st.tmp(a.verdict, n, 2);  // per job: verdict, status
        st.tmp(a.bad, n);
        st.tmp(a.out_peaks, 2 * n, 64 * 5);  // AOCL, SWBF
        st.tmp(a.out_np, n, 2);
        st.tmp(a.out_n, n, 3);  // aocl.num_leafs, swbf_inactive.num_leafs, n_active
        st.tmp(a.out_active, (size_t)o.win_total);
        if (keep_nodes) {
            st.tmp(a.carry, 2 * n, 64 * 5);
            st.tmp(a.carry_mask, 2 * n);
        }
    }
    void enqueue(Stage& st, nhip_ctx* c) {  // after commit()
        a.rec.auth = d_auth;
        a.rec.verdict = a.rec.valid + R;
        a.rec.status = a.rec.valid + 2 * R;
        a.status = a.verdict + n;
        if (unpack) unpack->enqueue(st, c, n, &a.rec.ch);
        const nhip::MsChunkAuthJobsDev auth{a.jobs, a.peaks, a.rec.ch, d_entry_rec, a.rec_job, d_auth};
        st.launch([&] { return nhip::launch_ms_chunk_auth_jobs(auth, E, c->stream); });
        st.launch([&] { return nhip::launch_ms_records_jobs(a, R, c->stream); });
        st.launch([&] { return nhip::launch_ms_apply(a, n, c->stream, keep_nodes); });
    }
    void read_back(Stage& st) {
        st.out(vs.data(), a.verdict, 2 * n);
        st.out(bad.data(), a.bad, n);
        if (!cnt.accumulators) return;
        st.out(out.aocl_peaks, a.out_peaks, n * 64 * 5);
        st.out(out.swbf_peaks, a.out_peaks, n * 64 * 5, n * 64 * 5);
        st.out(out.aocl_n_peaks, a.out_np, n);
        st.out(out.swbf_n_peaks, a.out_np, n, n);
        st.out(out.aocl_num_leafs, a.out_n, n);
        st.out(out.swbf_num_leafs, a.out_n, n, n);
        st.out(out.n_active, a.out_n, n, 2 * n);
        st.out(out.active, a.out_active, (size_t)o.win_total);
    }
    void write_outputs() {  // after finish() == NHIP_OK
        std::copy(vs.begin(), vs.begin() + n, out.verdict);
        std::copy(vs.begin() + n, vs.end(), out.status);
        std::copy(bad.begin(), bad.end(), out.bad_record);
    }
};

// The witnesses' part of nhip_ms_update_batch, behind a BlockPart that keeps its nodes: inputs that
// passed ms_update_ok, the host plan, and an output that passed ms_updated_check for a fill.
struct WitnessPart {
    const nhip_ms_update_in& wi;
    const nhip::MsUpdateCounts& counts;
    const nhip::MsUpdatePlan& up;
    nhip_ms_updated& out;
    const size_t W, WE, WA, OE, OPD, ORW;  // witnesses, their input entries, and the plan's output totals
    nhip::MsUpdateDev ud{};
    const uint32_t* d_in_ent_wit = nullptr;  // per input entry: its witness
    uint8_t* d_wauth = nullptr;
    std::vector<uint8_t> wstatus;  // a temporary, as BlockPart's

    WitnessPart(const nhip_ms_update_in& wit, const nhip::MsUpdateCounts& wc, const nhip::MsUpdatePlan& plan,
                nhip_ms_updated& out_)
        : wi(wit), counts(wc), up(plan), out(out_), W((size_t)wc.witnesses), WE((size_t)wc.chunks.entries),
          WA((size_t)plan.aocl_path_off[W]), OE(plan.chunk_index.size()), OPD((size_t)plan.path_off[OE]),
          ORW((size_t)plan.rel_off[OE]), wstatus(W) {}
    void declare(Stage& st) {
        st.in(ud.minimum, wi.minimum, W, 2);
        st.in(ud.distances, wi.distances, W, 45);
        st.in(ud.aocl_leaf_index, wi.aocl_leaf_index, W);
        st.in(ud.aocl_leaf, wi.aocl_leaf, W, 5);
        st.in(ud.aocl_path_off, wi.aocl_path_off, W ? W + 1 : 0);
        st.in(ud.aocl_path, wi.aocl_path, (size_t)counts.aocl_digests, 5);
        stage_chunks(st, W ? *wi.chunks : NO_CHUNKS, W, counts.chunks, ud.ch);
        st.in(ud.wit_job, up.wit_job.data(), W);
        st.in(d_in_ent_wit, up.in_ent_wit.data(), WE);
        st.in(ud.o_aocl_path_off, up.aocl_path_off.data(), W + 1);
        st.in(ud.o_entry_off, up.entry_off.data(), W + 1);
        st.in(ud.o_key, up.chunk_index.data(), OE);
        st.in(ud.o_path_off, up.path_off.data(), OE + 1);
        st.in(ud.o_rel_off, up.rel_off.data(), OE + 1);
        st.in(ud.o_ent_wit, up.ent_wit.data(), OE);
        st.in(ud.o_ent_src, up.ent_src.data(), OE);
        st.tmp(d_wauth, WE);
        st.tmp(ud.status, W, 2);  // per witness: status, error byte
        st.tmp(ud.o_aocl_path, WA, 5);
        st.tmp(ud.o_chunk_index, OE);
        st.tmp(ud.o_path, OPD, 5);
        st.tmp(ud.o_rel, ORW);
    }
    // after commit(); a: the block's, its launches enqueued
    void enqueue(Stage& st, nhip_ctx* c, const nhip::MsApplyDev& a) {
        ud.auth = d_wauth;
        ud.err = ud.status + W;
        const nhip::MsChunkAuthJobsDev auth{a.jobs, a.peaks, ud.ch, d_in_ent_wit, ud.wit_job, d_wauth};  // entry -> witness -> job
        st.launch([&] { return nhip::launch_ms_chunk_auth_jobs(auth, WE, c->stream); });
        st.launch([&] { return nhip::launch_ms_wit_admit(a, ud, W, c->stream); });
        st.launch([&] { return nhip::launch_ms_wit_paths(a, ud, W, OE, c->stream); });
        st.launch([&] { return nhip::launch_ms_wit_chunks(a, ud, OE, c->stream); });
        st.launch([&] { return nhip::launch_ms_wit_seal(ud, W, c->stream); });
    }
    void read_back(Stage& st) {
        st.out(wstatus.data(), ud.status, W);
        st.out(out.aocl_path, ud.o_aocl_path, 5 * WA);
        st.out(out.chunk_index, ud.o_chunk_index, OE);
        st.out(out.path, ud.o_path, 5 * OPD);
        st.out(out.rel, ud.o_rel, ORW);
    }
    void write_outputs() {  // after finish() == NHIP_OK
        // the offset arrays and totals from the plan; chunk_index is the device's (zero for a rejected witness)
        nhip::ms_updated_write(up, false, &out);
        std::copy(wstatus.begin(), wstatus.end(), out.status);
    }
};

// One Stage over a block part and, for nhip_ms_update_batch, the witness part behind it
int run_parts(nhip_ctx* c, BlockPart& blk, WitnessPart* wit = nullptr) {
    Stage st(c);
    blk.declare(st);
    if (wit) wit->declare(st);
    if (st.commit()) return st.finish();
    blk.enqueue(st, c);
    if (wit) {
        wit->enqueue(st, c, blk.a);
        wit->read_back(st);
    }
    blk.read_back(st);
    if (const int rc = st.finish()) return rc;
    blk.write_outputs();
    if (wit) wit->write_outputs();
    return NHIP_OK;
}

}  // namespace

extern "C" {

// twenty-first MmrMembershipProof::verify for n (leaf, path) items against one MMR
// (application/loops/peer_loop.rs:1235, protocol/peer.rs:824; path shape archival_mmr.rs:250-281).
int nhip_mmr_verify_batch(nhip_ctx* c, const nhip_mmr* mmr, const uint64_t* leaf_index, const uint64_t* leaves,
                          const uint64_t* path_off, const uint64_t* path, size_t n, uint8_t* verdicts) {
    if (!c || nhip::ms_mmr_ok(mmr)) return NHIP_ERR_ARG;
    if (n == 0) return NHIP_OK;
    if (!leaf_index || !leaves || !verdicts || n > SIZE_MAX / 64) return NHIP_ERR_ARG;
    uint64_t pd = 0;
    if (nhip::ms_paths_ok(path_off, path, n, &pd)) return NHIP_ERR_ARG;
    Stage st(c);
    nhip::MmrDev dm{nullptr, mmr->n_peaks, mmr->num_leafs};
    const uint64_t *d_leaf_index, *d_leaves, *d_path_off, *d_path;
    uint8_t* d_verdicts;
    st.in(dm.peaks, mmr->peaks, mmr->n_peaks, 5);
    st.in(d_leaf_index, leaf_index, n);
    st.in(d_leaves, leaves, n, 5);
    st.in(d_path_off, path_off, n + 1);
    st.in(d_path, path, (size_t)pd, 5);
    st.tmp(d_verdicts, n);
    if (st.commit()) return st.finish();
    st.launch([&] {
        return nhip::launch_mmr_verify(dm, d_leaf_index, d_leaves, d_path_off, d_path, n, d_verdicts, c->stream);
    });
    st.out(verdicts, d_verdicts, n);
    return st.finish();
}

// RemovalRecord::validate (removal_record.rs:202-251) and MutatorSetAccumulator::can_remove
// (mutator_set_accumulator.rs:187-222) for n records (block/mod.rs:816-822, transaction_kernel.rs:129,145):
// k_ms_chunk_auth over every dictionary entry, then k_ms_records.
int nhip_ms_can_remove_batch(nhip_ctx* c, const nhip_msa* msa, const uint64_t* minimum, const uint32_t* distances,
                             const nhip_ms_chunks* chunks, size_t n, uint8_t* valid, uint8_t* can_remove,
                             uint8_t* status) {
    if (!c || nhip::ms_msa_ok(msa)) return NHIP_ERR_ARG;
    if (n == 0) return NHIP_OK;
    if (!minimum || !distances || !valid || !can_remove || !status || n > SIZE_MAX / 256) return NHIP_ERR_ARG;
    nhip::MsChunkCounts cc;
    if (nhip::ms_chunks_ok(chunks, n, &cc)) return NHIP_ERR_ARG;
    try {
        std::vector<uint32_t> active;
        nhip::ms_append_sorted_window(active, *msa);
        const size_t E = (size_t)cc.entries;
        Stage st(c);
        nhip::MmrDev swbf{nullptr, msa->swbf_inactive.n_peaks, msa->swbf_inactive.num_leafs};
        nhip::MsRecordsDev r{};  // aocl_member null: validate / can_remove
        uint8_t* d_auth;
        st.in(swbf.peaks, msa->swbf_inactive.peaks, msa->swbf_inactive.n_peaks, 5);
        st.in(r.active, active.data(), active.size());
        st.in(r.minimum, minimum, n, 2);
        st.in(r.distances, distances, n, 45);
        stage_chunks(st, *chunks, n, cc, r.ch);
        st.tmp(d_auth, E);
        st.tmp(r.valid, n, 3);  // valid, verdict, status
        if (st.commit()) return st.finish();
        r.auth = d_auth;
        r.n_active = active.size();
        r.aocl_num_leafs = msa->aocl.num_leafs;
        r.verdict = r.valid + n;
        r.status = r.valid + 2 * n;
        st.launch([&] { return nhip::launch_ms_chunk_auth(swbf, r.ch, E, d_auth, c->stream); });
        st.launch([&] { return nhip::launch_ms_records(r, n, c->stream); });
        st.out(valid, r.valid, n);
        st.out(can_remove, r.verdict, n);
        st.out(status, r.status, n);
        return st.finish();
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

// MutatorSetAccumulator::verify (mutator_set_accumulator.rs:252-339) for n (item, membership proof) pairs
// (wallet_state.rs:1796,1958; state/mod.rs:1050,1206,1341): k_ms_aocl_leaf, AbsoluteIndexSet::compute into
// device buffers (no host round trip), k_ms_chunk_auth, k_ms_records.
int nhip_ms_verify_batch(nhip_ctx* c, const nhip_msa* msa, const uint64_t* items, const uint64_t* sender_randomness,
                         const uint64_t* receiver_preimages, const uint64_t* aocl_leaf_index,
                         const uint64_t* aocl_path_off, const uint64_t* aocl_path, const nhip_ms_chunks* chunks,
                         size_t n, uint8_t* verdicts, uint8_t* status) {
    if (!c || nhip::ms_msa_ok(msa)) return NHIP_ERR_ARG;
    if (n == 0) return NHIP_OK;
    if (!items || !sender_randomness || !receiver_preimages || !aocl_leaf_index || !verdicts || !status ||
        n > SIZE_MAX / 256)
        return NHIP_ERR_ARG;
    uint64_t apd = 0;
    if (nhip::ms_paths_ok(aocl_path_off, aocl_path, n, &apd)) return NHIP_ERR_ARG;
    nhip::MsChunkCounts cc;
    if (nhip::ms_chunks_ok(chunks, n, &cc)) return NHIP_ERR_ARG;
    try {
        std::vector<uint32_t> active;
        nhip::ms_append_sorted_window(active, *msa);
        const std::vector<uint64_t> in = nhip::ms_interleave15(items, sender_randomness, receiver_preimages, n);
        const size_t E = (size_t)cc.entries;
        Stage st(c);
        nhip::MmrDev aocl{nullptr, msa->aocl.n_peaks, msa->aocl.num_leafs};
        nhip::MmrDev swbf{nullptr, msa->swbf_inactive.n_peaks, msa->swbf_inactive.num_leafs};
        nhip::MsRecordsDev r{};  // valid null: verify
        const uint64_t *d_in, *d_leaf_index, *d_aocl_path_off, *d_aocl_path;
        uint64_t* d_minimum;
        uint32_t* d_distances;
        uint8_t *d_member, *d_auth;
        st.in(aocl.peaks, msa->aocl.peaks, msa->aocl.n_peaks, 5);
        st.in(swbf.peaks, msa->swbf_inactive.peaks, msa->swbf_inactive.n_peaks, 5);
        st.in(r.active, active.data(), active.size());
        st.in(d_in, in.data(), n, 15);
        st.in(d_leaf_index, aocl_leaf_index, n);
        st.in(d_aocl_path_off, aocl_path_off, n + 1);
        st.in(d_aocl_path, aocl_path, (size_t)apd, 5);
        stage_chunks(st, *chunks, n, cc, r.ch);
        st.tmp(d_minimum, n, 2);
        st.tmp(d_distances, n, 45);
        st.tmp(d_member, n);
        st.tmp(d_auth, E);
        st.tmp(r.verdict, n, 2);  // verdict, status
        if (st.commit()) return st.finish();
        r.minimum = d_minimum;
        r.distances = d_distances;
        r.aocl_member = d_member;
        r.auth = d_auth;
        r.n_active = active.size();
        r.aocl_num_leafs = msa->aocl.num_leafs;
        r.status = r.verdict + n;
        st.launch([&] {
            return nhip::launch_ms_aocl_leaf(aocl, d_in, d_leaf_index, d_aocl_path_off, d_aocl_path, n, d_member, c->stream);
        });
        st.launch([&] { return nhip::launch_absolute_index_sets(d_in, d_leaf_index, n, d_minimum, d_distances, c->stream); });
        st.launch([&] { return nhip::launch_ms_chunk_auth(swbf, r.ch, E, d_auth, c->stream); });
        st.launch([&] { return nhip::launch_ms_records(r, n, c->stream); });
        st.out(verdicts, r.verdict, n);
        st.out(status, r.status, n);
        return st.finish();
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

// Block::validate rules 2.b-2.e and Block::mutator_set_accumulator_after for independent jobs (DESIGN.md
// §6d): k_ms_chunk_auth_jobs, k_ms_records_jobs, k_ms_apply.  The host stages order only (ms_shape.cpp).
int nhip_ms_apply_batch(nhip_ctx* c, const nhip_ms_apply_in* in, nhip_ms_apply_out* out) {
    nhip::MsApplyCounts cnt;
    if (!c || nhip::ms_apply_ok(in, out, &cnt)) return NHIP_ERR_ARG;
    if (in->n_jobs == 0) return NHIP_OK;
    try {
        BlockPart blk(*in, *out, cnt, false);
        return run_parts(c, blk);
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

// MsMembershipProof / RemovalRecord batch_update_from_addition and batch_update_from_remove over whole blocks, as the
// end state: nhip_ms_apply_batch with its nodes kept, then k_ms_chunk_auth_jobs over the witnesses'
// dictionaries, k_ms_wit_admit, k_ms_wit_paths, k_ms_wit_chunks, k_ms_wit_seal.  The host lays out shapes only.
int nhip_ms_update_batch(nhip_ctx* c, const nhip_ms_apply_in* block, nhip_ms_apply_out* block_out,
                         const nhip_ms_update_in* wit, nhip_ms_updated* out) {
    nhip::MsApplyCounts cnt;
    nhip::MsUpdateCounts wc;
    if (!c || !out || nhip::ms_apply_ok(block, block_out, &cnt) || nhip::ms_update_ok(block, wit, &wc)) return NHIP_ERR_ARG;
    try {
        nhip::MsUpdatePlan plan;
        int rc = nhip::ms_update_plan(block, wit, wc, &plan);
        if (rc != NHIP_OK) return rc;
        if ((rc = nhip::ms_updated_check(plan, true, out)) != NHIP_OK) return rc;
        if (nhip::ms_updated_is_count_pass(out) || block->n_jobs == 0) {
            nhip::ms_updated_write(plan, true, out);
            return NHIP_OK;
        }
        BlockPart blk(*block, *block_out, cnt, true);  // k_ms_apply keeps its nodes
        WitnessPart wp(*wit, wc, plan, *out);
        return run_parts(c, blk, &wp);
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

// RemovalRecordList::try_unpack for n_jobs packed lists: the host plan decides every status and
// lays out the unpacked shape (ms_unpack_plan.cpp); k_ms_unpack computes the path digests.
int nhip_ms_unpack_batch(nhip_ctx* c, const uint64_t* rec_off, size_t n_jobs, const uint64_t* minimum,
                         const uint32_t* distances, const nhip_ms_chunks* packed, nhip_ms_unpacked* out) {
    if (!c || !out) return NHIP_ERR_ARG;
    const nhip::MsPackedIn in{rec_off, n_jobs, minimum, distances, packed};
    nhip::MsUnpackCounts cnt;
    if (nhip::ms_packed_ok(in, &cnt)) return NHIP_ERR_ARG;
    try {
        nhip::MsUnpackPlan plan;
        int rc = nhip::ms_unpack_plan(in, cnt, &plan);
        if (rc != NHIP_OK) return rc;
        const bool count_pass = nhip::ms_unpacked_is_count_pass(out);
        if ((rc = nhip::ms_unpacked_write(plan, n_jobs, true, out)) != NHIP_OK) return rc;
        const size_t PD = plan.gath_src.size();
        if (count_pass || PD == 0) return NHIP_OK;
        UnpackProgram prog(plan, *packed, cnt.chunks);
        Stage st(c);
        prog.declare(st);
        st.tmp(prog.u.path_out, PD, 5);
        if (st.commit()) return st.finish();
        prog.enqueue(st, c, n_jobs);
        st.out(out->path, prog.u.path_out, 5 * PD);
        return st.finish();
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

// Block::validate rules 2.a-2.e: nhip_ms_apply_batch over the plan's unpacked shape, its paths filled on the device
// by k_ms_unpack ahead of the three launches; the jobs that fail 2.a are overwritten with their unpack status.
int nhip_ms_apply_batch_packed(nhip_ctx* c, const nhip_ms_apply_in* in, nhip_ms_apply_out* out) {
    nhip::MsApplyCounts cnt;
    if (!c || nhip::ms_apply_ok(in, out, &cnt)) return NHIP_ERR_ARG;
    const size_t n = in->n_jobs;
    if (n == 0) return NHIP_OK;
    try {
        const nhip::MsPackedIn pin{in->rec_off, n, in->minimum, in->distances, in->chunks};
        nhip::MsUnpackCounts pc;
        if (nhip::ms_packed_ok(pin, &pc)) return NHIP_ERR_ARG;
        nhip::MsUnpackPlan plan;
        int rc = nhip::ms_unpack_plan(pin, pc, &plan);
        if (rc != NHIP_OK) return rc;
        const nhip_ms_chunks unpacked{plan.entry_off.data(), plan.chunk_index.data(), plan.path_off.data(), nullptr,
                                      plan.rel_off.data(),   plan.rel.data()};
        nhip_ms_apply_in in2 = *in;
        in2.chunks = &unpacked;
        nhip::MsApplyCounts cnt2 = cnt;
        cnt2.chunks = nhip::MsChunkCounts{plan.chunk_index.size(), plan.gath_src.size(), plan.rel.size()};
        UnpackProgram prog(plan, cnt.records ? *in->chunks : NO_CHUNKS, pc.chunks);
        BlockPart blk(in2, *out, cnt2, false, &prog);
        if ((rc = run_parts(c, blk)) != NHIP_OK) return rc;
        for (size_t j = 0; j < n; ++j) {
            if (plan.status[j] == NHIP_MS_OK) continue;
            out->verdict[j] = 0;
            out->status[j] = plan.status[j];
            out->bad_record[j] = UINT64_MAX;
            if (cnt.accumulators) {
                out->aocl_n_peaks[j] = out->swbf_n_peaks[j] = 0;
                out->aocl_num_leafs[j] = out->swbf_num_leafs[j] = out->n_active[j] = 0;
            }
        }
        return NHIP_OK;
    } catch (const std::bad_alloc&) {
        return NHIP_ERR_OOM;
    }
}

}  // extern "C"
