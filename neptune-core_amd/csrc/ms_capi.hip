// C-ABI layer of libneptune_hip.so, the mutator-set entry points (declarations: include/neptune_hip.h;
// DESIGN.md §6c-§6g, §6j).  Each is: validate shapes, stage order (both ms_shape.cpp), build its parts, one Stage
// (ctx.hpp: declare the device buffers, commit, launch, read back), write the outputs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "ms_parts.hpp"

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

// MsMembershipProof::revert_update_from_remove / revert_update_from_batch_addition over whole blocks, as the end
// state: nhip_ms_apply_batch, then k_ms_revert_nodes, k_ms_rev_admit, k_ms_rev_paths, k_ms_rev_chunks,
// the verification of every reverted witness against msa_before (k_ms_rev_aocl_jobs, k_ms_chunk_auth_jobs) and
// k_ms_rev_seal.  The host lays out shapes only.  The block part does not keep its nodes: they are the values after
// the block, and the revert reads the old ones, which k_ms_revert_nodes computes from the records.
int nhip_ms_revert_batch(nhip_ctx* c, const nhip_ms_apply_in* block, nhip_ms_apply_out* block_out,
                         const nhip_ms_update_in* wit, nhip_ms_updated* out) {
    nhip::MsApplyCounts cnt;
    nhip::MsUpdateCounts wc;
    if (!c || !out || nhip::ms_apply_ok(block, block_out, &cnt) || nhip::ms_update_ok(block, wit, &wc)) return NHIP_ERR_ARG;
    try {
        nhip::MsUpdatePlan plan;
        int rc = nhip::ms_revert_plan(block, wit, wc, &plan);
        if (rc != NHIP_OK) return rc;
        if ((rc = nhip::ms_updated_check(plan, true, out)) != NHIP_OK) return rc;
        if (nhip::ms_updated_is_count_pass(out) || block->n_jobs == 0) {
            nhip::ms_updated_write(plan, true, out);
            return NHIP_OK;
        }
        BlockPart blk(*block, *block_out, cnt, false);
        RevertPart rp(*wit, wc, plan, *out, blk);
        return run_parts(c, blk, &rp);
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
