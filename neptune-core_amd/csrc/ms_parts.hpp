// The parts a mutator-set entry point is built from (ms_capi.hip, ms_store_capi.hip): each
// declares its device buffers on a Stage (ctx.hpp), enqueues its launches after commit(), reads back and writes the
// caller's outputs once the whole call has succeeded.  Included by the .hip files of the entry points only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "ctx.hpp"
#include "kernels.hpp"
#include "ms_shape.hpp"
#include "ms_revert_plan.hpp"
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

// Where a store keeps the witnesses (ms_store_capi.hip): `in` names the current set (the input
// fields of MsUpdateDev) and `out` the next one (the plan's four offset arrays, uploaded there, and the four output
// pools).  sticky: the current set's first non-OK status per witness; sticky_next: where the statuses after go.
struct WitnessResident {
    nhip::MsUpdateDev in, out;
    uint64_t *o_aocl_path_off, *o_entry_off, *o_path_off, *o_rel_off;  // out's shape arrays, writable
    const uint8_t* sticky;
    uint8_t* sticky_next;
};

// What the witness parts of an update and of a revert share: the witnesses as the caller or the store holds them, the
// host plan (an MsUpdatePlan either way), the outputs, and the resident mode.  With `resident` (nhip_ms_store_update,
// nhip_ms_store_revert) the witnesses and the outputs are the store's device buffers: only the plan's arrays are
// staged, only the statuses are read back, and k_ms_store_seal runs behind the part's own seal.
struct WitnessIO {
    const nhip_ms_update_in& wi;
    const nhip::MsUpdateCounts& counts;
    const nhip::MsUpdatePlan& up;
    nhip_ms_updated& out;
    const size_t W, WE, WA, OE, OPD, ORW;  // witnesses, their input entries, and the plan's output totals
    nhip::MsUpdateDev ud{};
    std::vector<uint8_t> wstatus;  // a temporary, as BlockPart's
    const WitnessResident* const resident;

    WitnessIO(const nhip_ms_update_in& wit, const nhip::MsUpdateCounts& wc, const nhip::MsUpdatePlan& plan,
              nhip_ms_updated& out_, const WitnessResident* res)
        : wi(wit), counts(wc), up(plan), out(out_), W((size_t)wc.witnesses), WE((size_t)wc.chunks.entries),
          WA((size_t)plan.aocl_path_off[W]), OE(plan.chunk_index.size()), OPD((size_t)plan.path_off[OE]),
          ORW((size_t)plan.rel_off[OE]), wstatus(W), resident(res) {}
    // the witnesses, the plan and the outputs; status_bytes: per witness, the status first
    void declare_io(Stage& st, size_t status_bytes) {
        if (resident) {  // the plan's call-only arrays and the scratch; everything else is where the store keeps it
            const WitnessResident& r = *resident;
            ud = r.in;
            ud.o_aocl_path_off = r.o_aocl_path_off;
            ud.o_entry_off = r.o_entry_off;
            ud.o_path_off = r.o_path_off;
            ud.o_rel_off = r.o_rel_off;
            ud.o_aocl_path = r.out.o_aocl_path;
            ud.o_chunk_index = r.out.o_chunk_index;
            ud.o_path = r.out.o_path;
            ud.o_rel = r.out.o_rel;
            st.in(ud.wit_job, up.wit_job.data(), W);
            st.in(ud.o_key, up.chunk_index.data(), OE);  // the plan's keys; the store's are the device's (o_chunk_index)
            st.in(ud.o_ent_wit, up.ent_wit.data(), OE);
            st.in(ud.o_ent_src, up.ent_src.data(), OE);
            st.tmp(ud.status, W, status_bytes);
            return;
        }
        st.in(ud.minimum, wi.minimum, W, 2);
        st.in(ud.distances, wi.distances, W, 45);
        st.in(ud.aocl_leaf_index, wi.aocl_leaf_index, W);
        st.in(ud.aocl_leaf, wi.aocl_leaf, W, 5);
        st.in(ud.aocl_path_off, wi.aocl_path_off, W ? W + 1 : 0);
        st.in(ud.aocl_path, wi.aocl_path, (size_t)counts.aocl_digests, 5);
        stage_chunks(st, W ? *wi.chunks : NO_CHUNKS, W, counts.chunks, ud.ch);
        st.in(ud.wit_job, up.wit_job.data(), W);
        st.in(ud.o_aocl_path_off, up.aocl_path_off.data(), W + 1);
        st.in(ud.o_entry_off, up.entry_off.data(), W + 1);
        st.in(ud.o_key, up.chunk_index.data(), OE);
        st.in(ud.o_path_off, up.path_off.data(), OE + 1);
        st.in(ud.o_rel_off, up.rel_off.data(), OE + 1);
        st.in(ud.o_ent_wit, up.ent_wit.data(), OE);
        st.in(ud.o_ent_src, up.ent_src.data(), OE);
        st.tmp(ud.status, W, status_bytes);
        st.tmp(ud.o_aocl_path, WA, 5);
        st.tmp(ud.o_chunk_index, OE);
        st.tmp(ud.o_path, OPD, 5);
        st.tmp(ud.o_rel, ORW);
    }
    // after commit(), resident: the plan's shape, into the next set
    void upload_shape(Stage& st) {
        if (!resident) return;
        const WitnessResident& r = *resident;
        st.up(r.o_aocl_path_off, up.aocl_path_off.data(), W + 1);
        st.up(r.o_entry_off, up.entry_off.data(), W + 1);
        st.up(r.o_path_off, up.path_off.data(), OE + 1);
        st.up(r.o_rel_off, up.rel_off.data(), OE + 1);
    }
    void store_seal(Stage& st, nhip_ctx* c) {
        if (resident)
            st.launch([&] { return nhip::launch_ms_store_seal(ud, resident->sticky, resident->sticky_next, W, c->stream); });
    }
    void read_back(Stage& st) {
        st.out(wstatus.data(), ud.status, W);
        if (resident) return;
        st.out(out.aocl_path, ud.o_aocl_path, 5 * WA);
        st.out(out.chunk_index, ud.o_chunk_index, OE);
        st.out(out.path, ud.o_path, 5 * OPD);
        st.out(out.rel, ud.o_rel, ORW);
    }
    void write_outputs() {  // after finish() == NHIP_OK
        if (resident) return;  // the store takes wstatus
        // the offset arrays and totals from the plan; chunk_index is the device's (zero for a rejected witness)
        nhip::ms_updated_write(up, false, &out);
        std::copy(wstatus.begin(), wstatus.end(), out.status);
    }
};

// The witnesses' part of nhip_ms_update_batch, behind a BlockPart that keeps its nodes: inputs that
// passed ms_update_ok, the host plan, and an output that passed ms_updated_check for a fill.
struct WitnessPart : WitnessIO {
    const uint32_t* d_in_ent_wit = nullptr;  // per input entry: its witness
    uint8_t* d_wauth = nullptr;

    WitnessPart(const nhip_ms_update_in& wit, const nhip::MsUpdateCounts& wc, const nhip::MsUpdatePlan& plan,
                nhip_ms_updated& out_, const WitnessResident* res = nullptr)
        : WitnessIO(wit, wc, plan, out_, res) {}
    void declare(Stage& st) {
        declare_io(st, 2);  // per witness: status, error byte
        st.in(d_in_ent_wit, up.in_ent_wit.data(), WE);
        st.tmp(d_wauth, WE);
    }
    // after commit(); blk: the block's, its launches enqueued
    void enqueue(Stage& st, nhip_ctx* c, const BlockPart& blk) {
        const nhip::MsApplyDev& a = blk.a;
        upload_shape(st);
        ud.auth = d_wauth;
        ud.err = ud.status + W;
        const nhip::MsChunkAuthJobsDev auth{a.jobs, a.peaks, ud.ch, d_in_ent_wit, ud.wit_job, d_wauth};  // entry -> witness -> job
        st.launch([&] { return nhip::launch_ms_chunk_auth_jobs(auth, WE, c->stream); });
        st.launch([&] { return nhip::launch_ms_wit_admit(a, ud, W, c->stream); });
        st.launch([&] { return nhip::launch_ms_wit_paths(a, ud, W, OE, c->stream); });
        st.launch([&] { return nhip::launch_ms_wit_chunks(a, ud, OE, c->stream); });
        st.launch([&] { return nhip::launch_ms_wit_seal(ud, W, c->stream); });
        store_seal(st, c);
    }
};

// The witnesses' part of nhip_ms_revert_batch, behind a BlockPart (whose kept nodes it does not
// read: they are the values after the block): the witnesses as they stand after the block, ms_revert_plan's plan.
// Every reverted witness is authenticated against msa_before where it was written: its AOCL part by
// k_ms_rev_aocl_jobs (mmr_climb under the job's AOCL peaks, which are in the block's peak pool), its dictionary by
// the block's own chunk authentication, before k_ms_rev_seal folds the results into the status.
struct RevertPart : WitnessIO {
    nhip::MsRevertDev rd{};
    std::vector<uint64_t> node_off;
    uint8_t *d_member = nullptr, *d_oauth = nullptr;

    RevertPart(const nhip_ms_update_in& wit, const nhip::MsUpdateCounts& wc, const nhip::MsUpdatePlan& plan,
               nhip_ms_updated& out_, const BlockPart& blk, const WitnessResident* res = nullptr)
        : WitnessIO(wit, wc, plan, out_, res), node_off(nhip::ms_revert_node_offsets(blk.o.jobs)) {}
    void declare(Stage& st) {
        declare_io(st, 3);  // per witness: status, error byte, short-of byte
        st.in(rd.node_off, node_off.data(), node_off.size());
        st.tmp(rd.nodes, (size_t)node_off.back(), 5);
        st.tmp(d_member, W);
        st.tmp(d_oauth, OE);
    }
    void enqueue(Stage& st, nhip_ctx* c, const BlockPart& blk) {
        const nhip::MsApplyDev& a = blk.a;
        upload_shape(st);
        ud.err = ud.status + W;
        rd.short_of = ud.status + 2 * W;
        rd.member = d_member;
        rd.auth = d_oauth;
        st.launch([&] { return nhip::launch_ms_revert_nodes(a, rd, blk.n, (size_t)blk.o.grp_total, c->stream); });
        st.launch([&] { return nhip::launch_ms_rev_admit(a, ud, rd, W, c->stream); });
        st.launch([&] { return nhip::launch_ms_rev_paths(a, ud, rd, W, OE, c->stream); });
        st.launch([&] { return nhip::launch_ms_rev_chunks(a, ud, rd, OE, c->stream); });
        // the verification: every reverted witness against its job's msa_before
        st.launch([&] { return nhip::launch_ms_rev_aocl_jobs(a, ud, d_member, W, c->stream); });
        const nhip::MsChunksDev after{ud.o_entry_off, ud.o_chunk_index, ud.o_path_off, ud.o_path, ud.o_rel_off, ud.o_rel};
        const nhip::MsChunkAuthJobsDev auth{a.jobs, a.peaks, after, ud.o_ent_wit, ud.wit_job, d_oauth};  // entry -> witness -> job
        st.launch([&] { return nhip::launch_ms_chunk_auth_jobs(auth, OE, c->stream); });
        st.launch([&] { return nhip::launch_ms_rev_seal(ud, rd, W, c->stream); });
        store_seal(st, c);
    }
};

// One Stage over a block part and, for the update and revert calls, the witness part behind it
template <class Wit = WitnessPart>
int run_parts(Stage& st, nhip_ctx* c, BlockPart& blk, Wit* wit = nullptr) {
    blk.declare(st);
    if (wit) wit->declare(st);
    if (st.commit()) return st.finish();
    blk.enqueue(st, c);
    if (wit) {
        wit->enqueue(st, c, blk);
        wit->read_back(st);
    }
    blk.read_back(st);
    if (const int rc = st.finish()) return rc;
    blk.write_outputs();
    if (wit) wit->write_outputs();
    return NHIP_OK;
}
template <class Wit = WitnessPart>
int run_parts(nhip_ctx* c, BlockPart& blk, Wit* wit = nullptr) {
    Stage st(c);
    return run_parts(st, c, blk, wit);
}

}  // namespace
