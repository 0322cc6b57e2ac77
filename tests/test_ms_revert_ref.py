"""tests/ms_revert_ref.py held to `ms_ref.Archival` (no GPU): the end state of a revert, applied to the witnesses
tests/ms_update_ref.py gives for the state after a block, equals the witnesses derived from scratch before it, all of
them, field by field.  Each test asserts that its data reaches what it claims: AOCL paths that get shorter, entries
that drop, digests that are replaced, a chunk two records touch."""
import copy

import pytest

import ms_apply_ref as A
import ms_ref as R
import ms_revert_cases as D
import ms_revert_ref as V
import ms_update_cases as C


@pytest.fixture(scope="module")
def cases():
    return C.cases()


def _back(cs, job=None):
    """(the witnesses after, the helper's outcome of taking them back)"""
    assert cs.want[0][1] == R.OK
    after = [w for _, w in cs.want[1]]
    assert all(w is not None for w in after)
    return after, V.outcome(cs.arch, cs.msa, cs.adds, cs.recs, after, job=job)


def _equal_all(cs, got):
    assert len(got) == len(cs.wits)
    for k, ((st, w), before) in enumerate(zip(got, cs.wits)):
        assert st == R.OK, (cs.label, k, st)
        assert C.plain(w) == C.plain(before), (cs.label, k)


def _shorter_aocl(after, got):
    return sum(len(g.auth_path_aocl) < len(a.auth_path_aocl) for a, (_, g) in zip(after, got) if g is not None)


def _losing_entries(after, got):
    return sum(len(g.target_chunks) < len(a.target_chunks) for a, (_, g) in zip(after, got) if g is not None)


def test_additions_and_removals(cases):
    cs = cases.both
    after, (job, got) = _back(cs)
    assert job[1] == R.OK and len(got) == 592
    _equal_all(cs, got)
    assert _shorter_aocl(after, got) == 23 and _losing_entries(after, got) == 240
    blk = V.Block(cs.msa, len(cs.adds), cs.recs)
    # a chunk two records touch
    owners = {}
    for r, rec in enumerate(cs.recs):
        for i in rec.absolute_indices.to_array():
            if i // R.CHUNK_SIZE < blk.b0:
                owners.setdefault(i // R.CHUNK_SIZE, set()).add(r)
    assert any(len(s) > 1 for s in owners.values())
    # digests replaced by old node values, and digests kept, in the same run
    replaced = sum(len(blk.replaced(ci)) for w in after for ci, _, _ in w.target_chunks if ci < blk.b0)
    kept = sum(V.ilog2(ci ^ blk.b0) for w in after for ci, _, _ in w.target_chunks if ci < blk.b0) - replaced
    assert replaced > 100 and kept > 100
    assert V.shapes(blk, after) == tuple(C.U.shapes([(R.OK, w) for w in cs.wits]))


def test_removals_only(cases):
    for cs, n in ((cases.removals, 592), (cases.one, 581)):
        after, (job, got) = _back(cs)
        assert job[1] == R.OK and len(got) == n
        _equal_all(cs, got)
        assert _shorter_aocl(after, got) == 0 and _losing_entries(after, got) == 0
        changed = sum(C.plain(a)[5] != C.plain(g)[5] for a, (_, g) in zip(after, got))
        assert changed  # the removals did change dictionaries, and the revert took that back


def test_many_slides(cases):
    cs = cases.adds600[3]
    assert len(cs.adds) == 300 and not cs.recs
    after, (_, got) = _back(cs)
    assert len(got) == 580
    _equal_all(cs, got)
    assert _shorter_aocl(after, got) == 85 and _losing_entries(after, got) == 579
    assert max(len(a.auth_path_aocl) - len(g.auth_path_aocl) for a, (_, g) in zip(after, got)) >= 2


def test_born_in_the_block_is_not_in_the_aocl_before(cases):
    cs = cases.born
    after, (_, got) = _back(cs)
    n0 = cs.msa.aocl.num_leafs
    born = [k for k, w in enumerate(cs.wits) if w.aocl_leaf_index >= n0]
    assert len(born) == 5 and len(got) == 7
    for k, ((st, w), before) in enumerate(zip(got, cs.wits)):
        if k in born:
            assert st == R.NOT_IN_AOCL and w is None
        else:
            assert st == R.OK and C.plain(w) == C.plain(before)


def test_wide(cases):
    cs = cases.wide
    after, (_, got) = _back(cs, job=cs.want[0])
    n0 = cs.msa.aocl.num_leafs
    assert n0 == (1 << 40) + 5
    old = [k for k, w in enumerate(cs.wits) if w.aocl_leaf_index < n0]
    assert len(old) == 3 and len(got) == 5
    for k, ((st, w), before) in enumerate(zip(got, cs.wits)):
        if k in old:
            assert st == R.OK and C.plain(w) == C.plain(before)
        else:
            assert st == R.NOT_IN_AOCL
    assert any(len(after[k].auth_path_aocl) > len(got[k][1].auth_path_aocl) for k in old)


def test_statuses_and_their_order(cases):
    cs = cases.both
    after = [w for _, w in cs.want[1]]
    blk = V.Block(cs.msa, len(cs.adds), cs.recs)
    rich = next(w for w in after if w.aocl_leaf_index is not None and len(w.target_chunks) >= 3 and
                any(ci < blk.b0 and len(p) > 1 for ci, p, _ in w.target_chunks))
    assert V.admission(blk, rich) == R.OK
    w = copy.deepcopy(rich)
    ci, path, ch = w.target_chunks[0]
    w.target_chunks[0] = (ci, path[:-1], ch)
    assert V.admission(blk, w) == R.BAD_MMR_PATH
    w.target_chunks = w.target_chunks[:-1]
    assert V.admission(blk, w) == R.ABSENT_CHUNK
    w.absolute_indices = R.IndexSet((1 << 128) - 5, w.absolute_indices.distances)
    assert V.admission(blk, w) == R.OUT_OF_RANGE
    w.auth_path_aocl = w.auth_path_aocl[:-1]
    assert V.admission(blk, w) == R.NOT_IN_AOCL
    # a block index missing from a kept chunk: no end state
    touched = next(w for w in after if any(ci in blk.by_chunk for ci, _, _ in w.target_chunks))
    m = copy.deepcopy(touched)
    k = next(k for k, (ci, _, _) in enumerate(m.target_chunks) if ci in blk.by_chunk)
    ci, path, ch = m.target_chunks[k]
    rel = list(ch.relative_indices)
    rel.remove(blk.by_chunk[ci][0])
    m.target_chunks[k] = (ci, path, R.Chunk(rel))
    assert V.admission(blk, m) == R.OK and V.revert_witness(blk, m) is None
    # a rejected job rejects every witness
    job, got = V.outcome(cs.arch, cs.msa, cs.adds, [cs.recs[0], cs.recs[0]], after[:3])
    assert job[1] == A.DUPLICATE_RECORD and got == [(V.JOB_REJECTED, None)] * 3


def test_a_stale_witness_does_not_survive(cases):
    """A witness that never crossed the block passes admission when the block has no addition (the shapes are the
    same on both sides); what comes back is rejected or is valid against the accumulator before."""
    cs = cases.removals
    assert not cs.adds
    after = [w for _, w in cs.want[1]]
    blk = V.Block(cs.msa, 0, cs.recs)
    # its chunk lacks the block's indices
    k = next(k for k, w in enumerate(after) if w.aocl_leaf_index is not None and
             any(ci in blk.by_chunk for ci, _, _ in w.target_chunks))
    stale = cs.wits[k]
    assert C.plain(stale) != C.plain(after[k]) and V.admission(blk, stale) == R.OK
    assert V.revert_witness(blk, stale) is None
    assert V.outcome(cs.arch, cs.msa, [], cs.recs, [after[0], stale])[1][1] == (R.BAD_MMR_PATH, None)
    # its chunks are untouched and only digests of its paths changed with the block: those are the digests the revert
    # replaces by the old values, so what comes back is the witness itself, which is valid before the block
    k = next(k for k, w in enumerate(after) if w.target_chunks and C.plain(w) != C.plain(cs.wits[k]) and
             not any(ci in blk.by_chunk for ci, _, _ in w.target_chunks))
    stale = cs.wits[k]
    assert V.admission(blk, stale) == R.OK
    assert V.outcome(cs.arch, cs.msa, [], cs.recs, [stale])[1] == [(R.OK, V.revert_witness(blk, stale))]
    assert C.plain(V.revert_witness(blk, stale)) == C.plain(stale) and V.verification(cs.msa, stale) == R.OK


def test_paths_of_37_levels():
    """The helper against a sparse Bloom-filter MMR of 2^37 chunks built from scratch on both sides of the block."""
    d = D.deep()
    blk = V.Block(d.msa, len(d.adds), [d.rec])
    assert blk.b0 == blk.b1 == 1 << 37 and sorted(blk.by_chunk) == [d.ci2, d.ci]
    assert blk.by_chunk[d.ci2] == [17, 17] and V.ilog2(d.ci ^ d.ci2) == 1
    assert all(len(path) == 37 for _, path, _ in d.rec.target_chunks) and len(d.rec.target_chunks) == 2
    assert all(len(path) == 37 for w in d.after for _, path, _ in w.target_chunks)
    assert sum(len(w.target_chunks) for w in d.after) == 8
    # the record is valid before the block, and every witness verifies on its side of it, against the peaks
    assert R.can_remove(d.msa, d.rec) == (True, True, R.OK)
    assert all(V.verification(d.msa, w) == R.OK for w in d.before)
    assert all(V.verification(d.msa_after, w) == R.OK for w in d.after)
    assert d.msa.swbf_inactive.peaks != d.msa_after.swbf_inactive.peaks
    # the digests the block changed: level 0 beside the touched chunk, level 10, and level 36, the top of the path
    assert blk.replaced(d.sib) == [0, 1] and 10 in blk.replaced(d.c10) and blk.replaced(d.c36) == [36]
    assert blk.replaced(d.ci) == [1] and blk.replaced(d.ci2) == [1]  # each other's sibling subtree at level 1
    job, got = V.outcome(None, d.msa, d.adds, [d.rec], d.after, job=d.job)
    assert [st for st, _ in got] == [R.OK] * 6 + [R.NOT_IN_AOCL]
    assert [C.plain(w) for _, w in got[:6]] == [C.plain(w) for w in d.before]
    assert [len(ch.relative_indices) for _, _, ch in got[0][1].target_chunks] == [0, 3]  # a chunk left with 0 words
    # a stale witness of this job: reverted by shape it does not authenticate against the peak before
    stale = copy.deepcopy(d.before[1])
    assert V.admission(blk, stale) == R.OK and V.outcome(None, d.msa, d.adds, [d.rec], [stale], job=d.job)[1][0][0] == R.BAD_MMR_PATH
