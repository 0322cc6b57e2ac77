"""tests/ms_update_ref.py checked against tests/ms_ref.py's own verifier (no GPU): the witnesses the helper gives for the
state after a block are the ones `ms_verify` / `can_remove` accept against the accumulator after, their lengths are
the two xor formulas, the old AOCL path is a prefix of the new one, and the keys are the chunk indices below the new
batch index in ascending order.  The admission statuses come in the stated order."""
import copy

import pytest

import ms_ref as R
import ms_update_cases as C
import ms_update_ref as U


@pytest.fixture(scope="module")
def cases():
    return C.cases()


def _ilog2(x):
    return x.bit_length() - 1


def _accepted(cs):
    return [(old, new) for old, (st, new) in zip(cs.wits, cs.want[1]) if st == R.OK]


def test_fresh_proofs_verify_against_the_accumulator_after(cases):
    checked = 0
    for cs in (cases.adds600[2], cases.both, cases.born, cases.small[5]):
        after = cs.want[0][3]
        arch = cs.arch
        items = list(arch.items) + list(cs.adds)
        spent = set(cases.removed) if arch is cases.arch else set(cases.small_sets[arch.msa().aocl.num_leafs][1])
        spent |= set(cases.low) if cs.recs else set()
        for old, new in _accepted(cs):
            if new.aocl_leaf_index is None:
                rec = R.Record(new.absolute_indices, new.target_chunks)
                assert R.validate(after, rec) == (True, R.OK), cs.label
                continue
            l = new.aocl_leaf_index
            mp = R.MembershipProof(items[l][1], items[l][2], new.auth_path_aocl, l, new.target_chunks)
            want = (False, R.ALREADY_REMOVED) if l in spent else (True, R.OK)
            assert R.ms_verify(after, items[l][0], mp) == want, (cs.label, l)
            checked += l not in spent
    assert checked > 1000


def test_lengths_prefixes_and_keys(cases):
    for cs in C.everything(cases):
        n0, n1, b1 = cs.msa.aocl.num_leafs, cs.n1, cs.b1
        for old, new in _accepted(cs):
            l = new.aocl_leaf_index
            if l is not None:
                assert len(new.auth_path_aocl) == _ilog2(l ^ n1), cs.label
                if l < n0:
                    assert len(old.auth_path_aocl) == _ilog2(l ^ n0)
                assert list(new.auth_path_aocl[:len(old.auth_path_aocl)]) == list(old.auth_path_aocl), cs.label
            keys = [ci for ci, _, _ in new.target_chunks]
            assert keys == C.chunks_of(new.absolute_indices, b1), cs.label
            assert all(len(path) == _ilog2(ci ^ b1) for ci, path, _ in new.target_chunks), cs.label
            assert all(list(ch.relative_indices) == sorted(ch.relative_indices) for _, _, ch in new.target_chunks)


def test_admission_statuses_and_their_order(cases):
    cs = cases.with_mutants
    got = [st for st, _ in cs.want[1]]
    assert [got[k] for k in cases.mutant_at] == [want for _, want, _ in cases.mutants]
    assert all(got[k] == R.OK for k in range(len(got)) if k not in cases.mutant_at)
    # of several failures the first in the order NOT_IN_AOCL, OUT_OF_RANGE, ABSENT_CHUNK, BAD_MMR_PATH is reported
    w = copy.deepcopy(cases.mutants[4][2])                       # BAD_MMR_PATH
    assert U.admission(cs.msa, cs.commitments, w) == R.BAD_MMR_PATH
    w.target_chunks = w.target_chunks[:-1]                       # ... and ABSENT_CHUNK
    assert U.admission(cs.msa, cs.commitments, w) == R.ABSENT_CHUNK
    w.absolute_indices = R.IndexSet((1 << 128) - 5, w.absolute_indices.distances)
    assert U.admission(cs.msa, cs.commitments, w) == R.OUT_OF_RANGE
    w.auth_path_aocl = [C.flip(w.auth_path_aocl[0])] + list(w.auth_path_aocl[1:])
    assert U.admission(cs.msa, cs.commitments, w) == R.NOT_IN_AOCL
    # a rejected job rejects every witness
    for job in cases.rejected_jobs:
        assert job.want[0][1] != R.OK and all(st == U.JOB_REJECTED and w is None for st, w in job.want[1])
    assert [job.want[0][1] for job in cases.rejected_jobs] == [R.ALREADY_REMOVED, 7, 8]
