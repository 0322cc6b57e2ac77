"""GPU: membership proofs and removal records brought across a block (nhip_ms_update_batch: k_ms_apply with its nodes
kept, k_ms_chunk_auth_jobs over the witnesses, k_ms_wit_admit, k_ms_wit_paths, k_ms_wit_chunks, k_ms_wit_seal) against
the CPU restatement tests/ms_update_ref.py over `ms_ref.Archival`, never against themselves: statuses, AOCL paths,
keys, paths, chunks and the accumulator after, field by field.  The jobs come from tests/ms_update_cases.py, built
once and left unchanged; each test asserts that its jobs exercise what it claims."""
import numpy as np
import pytest

import ms_apply_ref as A
import ms_ref as R
import ms_update_cases as C
import ms_update_ref as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return C.cases()


def compare(group, got):
    for cs, g in zip(group, got):
        job = cs.want[0]
        assert g[:3] == job[:3], (cs.label, g[:3], job[:3])
        if job[3] is None:
            assert g[3] is None, cs.label
        else:
            assert A.same(C.back_msa(g[3]), job[3]), cs.label
        assert len(g[4]) == len(cs.want[1])
        for k, ((st, w), (want_st, want_w)) in enumerate(zip(g[4], cs.want[1])):
            assert st == want_st, (cs.label, k, st, want_st)
            assert C.plain(w) == C.plain(want_w), (cs.label, k)


def run(ctx, group):
    """The jobs of `group` in one call; every output against the helper's.  Returns the device's results."""
    from neptune_hip.mutator_set import update_witnesses_batch
    got = update_witnesses_batch(ctx, [cs.gpu() for cs in group])
    compare(group, got)
    return got


def pairs(cs):
    """(witness before, witness after) of the accepted witnesses, as plain data, with the witness itself"""
    return [(C.plain(old), C.plain(new), old) for old, (st, new) in zip(cs.wits, cs.want[1]) if st == R.OK]


# ---------------------------------------------------------------- 1. additions only
def test_additions_only_from_the_sets_of_600_and_601(ctx, cases):
    group = cases.adds600 + [cases.adds601]
    assert [len(cs.adds) for cs in group] == [0, 1, 9, 300, 3]
    assert [cs.b1 - cs.msa.batch_index for cs in group] == [0, 1, 2, 38, 0] and cases.adds601.msa.batch_index == 75
    assert all(cs.want[0][:3] == (True, R.OK, None) for cs in group)
    assert all(st == R.OK for cs in group for st, _ in cs.want[1])
    assert all(len(cs.wits) >= 550 and sum(w.aocl_leaf_index is None for w in cs.wits) == 20 for cs in group)
    assert all(old == new for old, new, _ in pairs(group[0]))  # no addition: the outputs are the inputs
    big = group[3]
    n0, old_peaks = 600, [tuple(p) for p in cases.msa.aocl.peaks]
    assert len(old_peaks) == 4 and len(big.want[0][3].aocl.peaks) == 4  # 600 = 512 + 64 + 16 + 8, 900 = 512 + 256 + 128 + 4
    grows = takes_peak = takes_new = 0
    for old, new, w in pairs(big):
        if w.aocl_leaf_index is None:
            continue
        l, before, after = w.aocl_leaf_index, old[4], new[4]
        grows += len(after) - len(before) >= 2
        for t in range(len(before), len(after)):
            takes_peak += after[t] in old_peaks
            takes_new += ((((l >> t) ^ 1) + 1) << t) > n0  # the sibling's block holds appended leaves
    assert grows and takes_peak and takes_new
    run(ctx, group)


# ---------------------------------------------------------------- 2. small sets
def test_small_sets(ctx, cases):
    group = cases.small
    by = {cs.label: cs for cs in group}
    assert list(by) == [f"{n0} + {k}" for n0 in (1, 8, 9, 255, 256) for k in (1, 9)]
    assert by["1 + 1"].wits[0].auth_path_aocl == [] and len(by["1 + 1"].want[1][0][1].auth_path_aocl) == 1
    assert by["8 + 1"].msa.batch_index == 0 and by["8 + 1"].b1 == 1  # the first slide ever
    assert by["1 + 9"].b1 == 1 and by["255 + 9"].b1 == 32 and by["256 + 9"].msa.batch_index == 31
    # a witness gains its first dictionary entry with the first slide ever
    assert any(not w.target_chunks and [ci for ci, _, _ in new.target_chunks] == [0]
               for w, (_, new) in zip(by["8 + 1"].wits, by["8 + 1"].want[1]))
    assert all(st == R.OK for cs in group for st, _ in cs.want[1])
    run(ctx, group)


# ---------------------------------------------------------------- 3. removals only
def test_removals_only(ctx, cases):
    one, twelve = cases.one, cases.removals
    assert len(one.recs) == 1 and len(twelve.recs) == 12 and not one.adds and not twelve.adds
    per_record = [set(C.chunks_of(r.absolute_indices, 74)) for r in twelve.recs]
    assert any(sum(ci in s for s in per_record) >= 2 for ci in set().union(*per_record))  # two records, one chunk
    own = own_untouched = unchanged = 0
    for cs in (one, twelve):
        for old, new, _ in pairs(cs):
            assert [e[0] for e in old[5]] == [e[0] for e in new[5]] and old[4] == new[4]  # no addition: same keys
            chunk_changed = any(a[2] != b[2] for a, b in zip(old[5], new[5]))
            path_changed = any(a[1] != b[1] for a, b in zip(old[5], new[5]))
            own += chunk_changed
            own_untouched += path_changed and not chunk_changed
            unchanged += old == new and len(old[5]) > 0
    assert own and own_untouched and unchanged
    # the job's own records, passed as witnesses: their chunks hold their own indices afterwards
    for cs in (one, twelve):
        m = len(cs.recs)
        for rec, (st, new) in zip(cs.recs, cs.want[1][-m:]):
            assert st == R.OK and new.absolute_indices == rec.absolute_indices
            for ci, _, chunk in new.target_chunks:
                mine = [i % R.CHUNK_SIZE for i in rec.absolute_indices.to_array() if i // R.CHUNK_SIZE == ci]
                assert mine and all(x in chunk.relative_indices for x in mine)
    run(ctx, [one, twelve])


# ---------------------------------------------------------------- 4. both
def test_additions_and_removals(ctx, cases):
    cs = cases.both
    assert len(cs.adds) == 20 and len(cs.recs) == 12 and cs.msa.batch_index == 74 and cs.b1 == 77
    hit = {}  # slid chunk -> the block's relative indices in it
    for r in cs.recs:
        for i in r.absolute_indices.to_array():
            if 74 <= i // R.CHUNK_SIZE < 77:
                hit.setdefault(i // R.CHUNK_SIZE, []).append(i % R.CHUNK_SIZE)
    touched = set().union(*[set(C.chunks_of(r.absolute_indices, 74)) for r in cs.recs])
    gains = merged = 0
    for old, new, _ in pairs(cs):
        old_keys = [e[0] for e in old[5]]
        for ci, path, rel in new[5]:
            if ci in hit and ci not in old_keys and all(x in rel for x in hit[ci]):
                gains += 1  # a new entry for a slid chunk that a record of this block hits as well
        # under the old peak [72, 74), which a removal changes and the append merges into [72, 76)
        for (ci, path, _), before in zip(new[5], old[5]):
            if ci in (72, 73) and ci == before[0] and touched & {72, 73} and len(before[1]) == 1 and len(path) == 2:
                merged += 1
    assert hit and gains and merged
    run(ctx, [cs])


# ---------------------------------------------------------------- 5. born in the block
def test_witnesses_born_in_the_block(ctx, cases):
    cs = cases.born
    assert len(cs.adds) == 300 and cases.born_at == [600, 601, 750, 898, 899] and cs.n1 == 900
    born = [(w, new) for w, (st, new) in zip(cs.wits, cs.want[1]) if w.aocl_leaf_index is not None and w.aocl_leaf_index >= 600]
    assert [w.aocl_leaf_index for w, _ in born] == cases.born_at
    assert all(w.auth_path_aocl == [] and w.target_chunks == [] for w, _ in born)
    assert all(st == R.OK for st, _ in cs.want[1])
    assert any(new.target_chunks for _, new in born) and any(not new.target_chunks for _, new in born)
    assert [len(new.auth_path_aocl) for _, new in born] == [(l ^ 900).bit_length() - 1 for l in cases.born_at]
    run(ctx, [cs])


# ---------------------------------------------------------------- 6. rejections
def _raw(ctx, group):
    from neptune_hip import _lib as L
    from neptune_hip.mutator_set import PackedUpdate
    pu = PackedUpdate([cs.gpu() for cs in group])
    assert pu.run(ctx.lib, ctx.handle) == L.NHIP_OK
    return pu


def _slots_zero(pu, i):
    o = pu.out
    a0, a1 = int(o["aocl_path_off"][i]), int(o["aocl_path_off"][i + 1])
    e0, e1 = int(o["entry_off"][i]), int(o["entry_off"][i + 1])
    return (not o["aocl_path"][a0:a1].any() and not o["chunk_index"][e0:e1].any()
            and not o["path"][int(o["path_off"][e0]):int(o["path_off"][e1])].any()
            and not o["rel"][int(o["rel_off"][e0]):int(o["rel_off"][e1])].any())


def test_one_rejection_per_witness_status(ctx, cases):
    bad, good = cases.with_mutants, cases.without_mutants
    want = [st for st, _ in bad.want[1]]
    assert [(name, want[k]) for (name, _, _), k in zip(cases.mutants, cases.mutant_at)] == [
        ("saturating index set", R.OUT_OF_RANGE), ("entry dropped", R.ABSENT_CHUNK), ("entry extra", R.ABSENT_CHUNK),
        ("entries swapped", R.ABSENT_CHUNK), ("path digest flipped", R.BAD_MMR_PATH), ("chunk word changed", R.BAD_MMR_PATH),
        ("aocl digest flipped", R.NOT_IN_AOCL), ("leaf index past the block", R.NOT_IN_AOCL),
        ("born with a wrong leaf", R.NOT_IN_AOCL)]
    assert all(want[k] == R.OK for k in range(19) if k not in cases.mutant_at) and len(want) == 19
    assert bad.want[0][:2] == (True, R.OK) and len(bad.recs) == 2 and len(bad.adds) == 9
    got_bad, got_good = run(ctx, [bad])[0], run(ctx, [good])[0]
    # the good witnesses around them: what the same call gives without the rejected ones
    kept = [g for k, g in enumerate(got_bad[4]) if k not in cases.mutant_at]
    assert [(st, C.plain(w)) for st, w in kept] == [(st, C.plain(w)) for st, w in got_good[4]]
    pu = _raw(ctx, [bad])
    assert all(_slots_zero(pu, k) for k in cases.mutant_at)
    assert not any(_slots_zero(pu, k) for k in range(19) if k not in cases.mutant_at)
    spans = pu.out["entry_off"][np.array(cases.mutant_at) + 1] - pu.out["entry_off"][np.array(cases.mutant_at)]
    assert int(spans.sum()) > 0  # the rejected witnesses keep planned slots; those are zero, not absent


def test_one_job_rejected_at_each_rule(ctx, cases):
    nb, rej = cases.neighbours, cases.rejected_jobs
    assert [cs.want[0][:3] for cs in rej] == [(False, R.ALREADY_REMOVED, 1), (False, A.DUPLICATE_RECORD, 2),
                                              (False, A.UPDATE_IMPOSSIBLE, 1)]
    assert all(st == U.JOB_REJECTED for cs in rej for st, _ in cs.want[1])
    assert all(cs.want[0][1] == R.OK and all(st == R.OK for st, _ in cs.want[1]) for cs in nb)
    group = [nb[0], rej[0], rej[1], nb[1], rej[2]]
    got = run(ctx, group)
    alone = [run(ctx, [cs])[0] for cs in nb]
    for g, a in ((got[0], alone[0]), (got[3], alone[1])):
        assert g[:3] == a[:3] and [(st, C.plain(w)) for st, w in g[4]] == [(st, C.plain(w)) for st, w in a[4]]
    pu = _raw(ctx, group)
    at = np.cumsum([0] + [len(cs.wits) for cs in group])
    for j in (1, 2, 4):
        assert all(_slots_zero(pu, i) for i in range(at[j], at[j + 1]))
        assert int(pu.out["entry_off"][at[j + 1]] - pu.out["entry_off"][at[j]]) > 0


# ---------------------------------------------------------------- 7. large counts
def test_64_bit_leaf_counts(ctx, cases):
    cs = cases.wide
    assert cs.msa.aocl.num_leafs == (1 << 40) + 5 and len(cs.msa.aocl.peaks) == 3 and len(cs.adds) == 9
    assert cs.msa.swbf_inactive.num_leafs == 1 << 37 and cs.b1 == (1 << 37) + 1
    assert [w.aocl_leaf_index - (1 << 40) for w in cs.wits] == [0, 3, 4, 5, 13]
    n1 = (1 << 40) + 14
    assert [len(new.auth_path_aocl) for _, new in cs.want[1]] == [3, 3, 3, 3, 1]
    assert all(len(new.auth_path_aocl) == ((w.aocl_leaf_index ^ n1).bit_length() - 1) for w, (_, new) in zip(cs.wits, cs.want[1]))
    assert all(not w.target_chunks and not new.target_chunks for w, (_, new) in zip(cs.wits, cs.want[1]))
    for w in cs.wits:  # wholly inside the window before and after
        assert all(cs.b1 <= i // R.CHUNK_SIZE <= (1 << 37) + 255 for i in w.absolute_indices.to_array())
    run(ctx, [cs])


# ---------------------------------------------------------------- 8. thirty jobs in one call
def test_thirty_mixed_jobs_equal_the_jobs_alone(ctx, cases):
    from neptune_hip import _lib as L
    from neptune_hip.mutator_set import PackedUpdate
    group = (cases.small + cases.extra + cases.rejected_jobs + cases.neighbours +
             [cases.with_mutants, cases.without_mutants, cases.born, cases.wide, cases.one, cases.both, cases.adds600[1],
              cases.adds601])
    assert len(group) == 30
    assert {cs.want[0][1] for cs in group} >= {R.OK, R.ALREADY_REMOVED, A.DUPLICATE_RECORD, A.UPDATE_IMPOSSIBLE}
    assert len({cs.msa.aocl.num_leafs for cs in group}) >= 8
    got = run(ctx, group)
    for cs, g in zip(group, got):
        a = run(ctx, [cs])[0]
        assert g[:3] == a[:3] and (g[3] is None) == (a[3] is None), cs.label
        if g[3] is not None:
            assert A.same(C.back_msa(g[3]), C.back_msa(a[3])), cs.label
        assert [(st, C.plain(w)) for st, w in g[4]] == [(st, C.plain(w)) for st, w in a[4]], cs.label
    # the same call twice on one context: equal bytes
    blobs = []
    for _ in range(2):
        pu = PackedUpdate([cs.gpu() for cs in group])
        assert pu.run(ctx.lib, ctx.handle) == L.NHIP_OK
        a = pu.apply.arrays
        blob = [pu.out[f].tobytes() for f in sorted(pu.out)]
        blob += [a[f].tobytes() for f in ("verdict", "status", "bad_record", "aocl_n_peaks", "aocl_num_leafs",
                                          "swbf_n_peaks", "swbf_num_leafs", "n_active")]
        for j in range(30):
            blob.append(a["aocl_peaks"][j, :int(a["aocl_n_peaks"][j])].tobytes())
            blob.append(a["swbf_peaks"][j, :int(a["swbf_n_peaks"][j])].tobytes())
            lo = int(a["active_off"][j])
            blob.append(a["active"][lo:lo + int(a["n_active"][j])].tobytes())
        blobs.append(b"".join(blob))
    assert blobs[0] == blobs[1]


# ---------------------------------------------------------------- 9. the loop closed
def test_updated_witnesses_pass_the_existing_checks_and_stale_ones_do_not(ctx, cases):
    from neptune_hip import mutator_set as MS
    cs = cases.both
    msa, update, _ = cs.gpu()
    arch = cases.arch
    spent = set(cases.removed) | set(cases.low)
    unspent = [i for i in cases.live if i not in spent]
    assert len(unspent) > 500
    items = [arch.items[i][0] for i in unspent]
    stale = [MS.MsMembershipProof(arch.items[i][1], arch.items[i][2], w.auth_path_aocl, i, C._chunks(w.target_chunks))
             for i, w in ((i, U.proof_witness(arch, i)) for i in unspent)]
    status, after, fresh = MS.update_membership_proofs(ctx, msa, update, items, stale)
    assert status == MS.OK and A.same(C.back_msa(after), cs.want[0][3])
    assert all(st == MS.OK for st, _ in fresh)
    fresh = [p for _, p in fresh]
    assert MS.verify_batch(ctx, after, items, fresh) == [(True, MS.OK)] * len(unspent)

    def same(a, b):
        return (list(map(tuple, a.auth_path_aocl)) == list(map(tuple, b.auth_path_aocl)) and
                [(ci, list(map(tuple, p)), list(ch.relative_indices)) for ci, p, ch in a.target_chunks] ==
                [(ci, list(map(tuple, p)), list(ch.relative_indices)) for ci, p, ch in b.target_chunks])

    changed = [not same(a, b) for a, b in zip(stale, fresh)]
    verdicts = MS.verify_batch(ctx, after, items, stale)
    assert sum(changed) > 400 and changed.count(False) > 0
    assert [v for v, _ in verdicts] == [not ch for ch in changed]  # stale wherever the block changed what it holds
    # the mempool's records of unspent items
    recs = [C.to_record(arch.removal_record(i)) for i in unspent[::25]]
    status, after2, fresh_recs = MS.update_removal_records(ctx, msa, update, recs)
    assert status == MS.OK and all(st == MS.OK for st, _ in fresh_recs) and len(recs) >= 20
    fresh_recs = [r for _, r in fresh_recs]
    assert MS.can_remove_batch(ctx, after, fresh_recs) == [(True, True, MS.OK)] * len(recs)
    rec_changed = [[(ci, list(map(tuple, p)), list(ch.relative_indices)) for ci, p, ch in a.target_chunks] !=
                   [(ci, list(map(tuple, p)), list(ch.relative_indices)) for ci, p, ch in b.target_chunks]
                   for a, b in zip(recs, fresh_recs)]
    assert [v for v, _, _ in MS.can_remove_batch(ctx, after, recs)] == [not ch for ch in rec_changed] and any(rec_changed)
