"""The CPU side of the batched mutator-set update (nhip_ms_apply_batch): the sequential accumulator-only
restatement of tests/ms_apply_ref.py against `ms_ref.Archival`, the helper's rule 2.c / 2.d restatements on
hand-made cases, the binding's declarations, and the host-side shape validator under ASan + UBSan
(tests/native/ms_apply_shape_check.cpp, a stand-alone program; nothing is preloaded and nothing runs on a GPU)."""
import copy
import os
import random
import shutil
import subprocess

import pytest

import ms_apply_ref as A
import ms_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
P = R.P


def _digest(rng):
    return tuple(rng.randrange(P) for _ in range(5))


def test_sequential_accumulator_equals_archival_for_every_prefix():
    rng = random.Random(77)
    arch = R.Archival()
    removed, slides = [], 0
    for k in range(300):
        before = arch.msa()
        item = (_digest(rng), _digest(rng), _digest(rng))
        arch.add(*item)
        after = arch.msa()
        assert A.same(A.msa_add(before, A.commitment(*item)), after), k
        slides += after.swbf_inactive.num_leafs - before.swbf_inactive.num_leafs
        if k % 15 == 14:  # 20 removals interleaved: the windows and the slid chunks are not empty
            victim = rng.randrange(k) if k % 30 == 14 else k - 2
            if victim not in removed:
                arch.remove(arch.removal_record(victim))
                removed.append(victim)
    assert len(removed) >= 18 and slides == 37 == arch.msa().batch_index
    assert sum(1 for ci in range(37) if arch.bloom.get(ci)) >= 10 and arch.msa().swbf_active


def test_apply_flags_the_record_whose_indices_are_all_set():
    rng = random.Random(78)
    arch = R.Archival()
    for _ in range(40):
        arch.add(_digest(rng), _digest(rng), _digest(rng))
    snap = A.clone(arch)
    recs = [arch.removal_record(i) for i in (3, 30)]
    forged = copy.deepcopy(recs[0])
    d = forged.absolute_indices.distances
    d[0], d[1] = d[1], d[0]
    assert d[0] != d[1] and A.distinct([recs[0], forged]) is None and A.distinct([recs[0], recs[1], recs[0]]) == 2
    assert A.apply(A.clone(arch), [], recs)[0] is None
    assert A.apply(A.clone(arch), [], [recs[0], forged])[0] == 1
    assert A.apply(A.clone(arch), [], [forged, recs[1], recs[0]])[0] == 2
    msa = arch.msa()
    assert A.outcome(arch, msa, [], [recs[0], forged])[:3] == (False, A.UPDATE_IMPOSSIBLE, 1)
    assert A.outcome(arch, msa, [], [recs[0], recs[0]])[:3] == (False, A.DUPLICATE_RECORD, 1)
    ok = A.outcome(arch, msa, [(_digest(rng),) * 3], recs)
    assert ok[:3] == (True, R.OK, None) and ok[3].aocl.num_leafs == 41 and len(ok[3].swbf_active) >= 45
    assert A.outcome(arch, msa, [], recs, expected=msa)[:2] == (False, A.UPDATE_MISMATCH)
    assert A.outcome(arch, msa, [], recs, expected=ok[3])[1] == A.UPDATE_MISMATCH  # ok[3] has the addition
    bad = R.Msa(msa.aocl, R.Mmr(msa.swbf_inactive.peaks, msa.swbf_inactive.num_leafs + 1), msa.swbf_active)
    assert A.outcome(arch, bad, [], recs)[:2] == (False, A.INCONSISTENT)
    assert arch.items == snap.items and arch.bloom == snap.bloom  # outcome leaves the set unchanged


def test_binding_declares_the_apply_entry_point():
    import neptune_hip._lib as L
    from neptune_hip import blocks, mutator_set as MS
    lib = L.load()
    assert len(L.SIGNATURES["nhip_ms_apply_batch"][0]) == 3 and hasattr(lib, "nhip_ms_apply_batch")
    assert lib.nhip_abi_version() >= 2600
    assert (MS.INCONSISTENT, MS.DUPLICATE_RECORD, MS.UPDATE_IMPOSSIBLE, MS.UPDATE_MISMATCH) == \
        (A.INCONSISTENT, A.DUPLICATE_RECORD, A.UPDATE_IMPOSSIBLE, A.UPDATE_MISMATCH) == (6, 7, 8, 9)
    assert len(MS.STATUS_NAMES) == 10 and MS.STATUS_NAMES[MS.UPDATE_MISMATCH] == "UPDATE_MISMATCH"
    assert callable(blocks.mutator_set_update_valid) and callable(blocks.accumulator_after)
    u = MS.MutatorSetUpdate()
    assert list(u.removals) == [] and list(u.additions) == []


def test_apply_shape_validator_clean_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ absent")
    subprocess.check_call(["make", "-s", "-f", "ms_apply_shape.mk", "-C", NATIVE, f"OUT={tmp_path}"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(tmp_path, "ms_apply_shape_check")], capture_output=True, text=True, timeout=120,
                       env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    good, bad = (int(x) for x in r.stdout.split()[1::2])
    assert good >= 5 and bad >= 25, r.stdout
