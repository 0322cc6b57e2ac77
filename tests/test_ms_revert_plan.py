"""nhip_ms_revert_plan, the host half of nhip_ms_revert_batch, through ctypes (no GPU): every shape array against
`shapes` of tests/ms_revert_ref.py for the jobs of tests/ms_update_cases.py (the witnesses standing after the block),
many jobs in one call against the jobs alone, the two-call sizing, argument errors that leave the outputs untouched,
the ABI version and the prototypes, and the plan and the store's mirror step in tests/native/ms_revert_check.cpp, a
stand-alone program built once plainly and once under ASan + UBSan (nothing is preloaded and nothing runs on a GPU)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import ms_ref as R
import ms_revert_ref as V
import ms_update_cases as C

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
ENTRY_POINTS = {"nhip_ms_revert_plan": 3, "nhip_ms_revert_batch": 5, "nhip_ms_store_revert": 4}


@pytest.fixture(scope="module")
def cases():
    return C.cases()


def after_job(cs):
    """The job of `cs` with the witnesses as they stand after it (the helper's), in the library's types."""
    assert cs.want[0][1] == R.OK and all(st == R.OK for st, _ in cs.want[1])
    msa, update, _ = cs.gpu()
    return msa, update, [C.to_witness(w) for _, w in cs.want[1]]


def _group(cases):
    return [cases.adds600[0], cases.adds600[1], cases.adds600[2], cases.adds600[3], cases.adds601, cases.one,
            cases.removals, cases.both, cases.wide] + cases.small + cases.extra


def _plan(group):
    import neptune_hip.mutator_set as MS
    return MS.revert_plan_batch([after_job(cs) for cs in group])


def _check(group):
    o = _plan(group)
    alen, ecnt, keys, plen, rlen = [], [], [], [], []
    for cs in group:
        blk = V.Block(cs.msa, len(cs.adds), cs.recs)
        for have, part in zip((alen, ecnt, keys, plen, rlen), V.shapes(blk, [w for _, w in cs.want[1]])):
            have += part
    assert [int(x) for x in np.diff(o["aocl_path_off"].astype(np.int64))] == alen
    assert [int(x) for x in np.diff(o["entry_off"].astype(np.int64))] == ecnt
    assert [int(x) for x in o["chunk_index"]] == keys
    assert [int(x) for x in np.diff(o["path_off"].astype(np.int64))] == plen
    assert [int(x) for x in np.diff(o["rel_off"].astype(np.int64))] == rlen
    assert all(int(o[name][0]) == 0 for name in ("aocl_path_off", "entry_off", "path_off", "rel_off"))
    assert not o["status"].any() and not o["aocl_path"].any() and not o["path"].any() and not o["rel"].any()
    return o, len(alen)


def test_abi_and_prototypes():
    import neptune_hip._lib as L
    import neptune_hip.mutator_set as MS
    lib = L.load()
    assert lib.nhip_abi_version() >= 3100
    for name, argc in ENTRY_POINTS.items():
        assert len(L.SIGNATURES[name][0]) == argc and L.SIGNATURES[name][1] is ctypes.c_int and hasattr(lib, name), name
    hdr = open(os.path.join(os.path.dirname(NATIVE), "..", "include", "neptune_hip.h")).read()
    for name in ENTRY_POINTS:
        assert f"int {name}(" in hdr, name
    for fn in ("revert_plan_batch", "revert_witnesses_batch", "revert_membership_proofs"):
        assert callable(getattr(MS, fn)), fn
    assert callable(MS.WitnessStore.revert)
    assert lib.nhip_ms_revert_plan(None, None, None) == L.NHIP_ERR_ARG
    assert lib.nhip_ms_revert_batch(None, None, None, None, None) == L.NHIP_ERR_ARG
    assert lib.nhip_ms_store_revert(None, None, None, None) == L.NHIP_ERR_ARG


def test_every_job_alone_equals_the_helper(cases):
    total = 0
    for cs in _group(cases):
        total += _check([cs])[1]
    assert total > 4000
    # the shapes the helper gives for the state before are the from-scratch witnesses' own
    cs = cases.both
    blk = V.Block(cs.msa, len(cs.adds), cs.recs)
    assert V.shapes(blk, [w for _, w in cs.want[1]]) == tuple(C.U.shapes([(R.OK, w) for w in cs.wits]))


def test_many_jobs_in_one_call_equal_the_jobs_alone(cases):
    jobs = cases.small + [cases.one, cases.adds600[2], cases.wide] + cases.extra
    alone = [_check([cs])[0] for cs in jobs]
    for group, parts in ((jobs, alone), (jobs[::-1], alone[::-1])):
        o, _ = _check(group)
        for name in ("aocl_path_off", "entry_off", "path_off", "rel_off"):
            want = np.concatenate([[0]] + [np.diff(p[name].astype(np.int64)) for p in parts]).cumsum()
            assert (o[name].astype(np.int64) == want).all(), name
        assert (o["chunk_index"] == np.concatenate([p["chunk_index"] for p in parts])).all()
    o, _ = _check([])
    assert all(int(o[name][0]) == 0 for name in ("aocl_path_off", "entry_off", "path_off", "rel_off"))


def test_born_and_floored_shapes(cases):
    """A witness born in the block gets no AOCL path; a kept chunk with fewer words than the block put into it gets
    length 0, not a wrapped one."""
    import neptune_hip.mutator_set as MS
    cs = cases.born
    msa, update, _ = cs.gpu()
    wits = [C.to_witness(w) for _, w in cs.want[1]]
    o = MS.revert_plan_batch([(msa, update, wits)])
    n0 = cs.msa.aocl.num_leafs
    for k, w in enumerate(wits):
        want = ((w.aocl_leaf_index ^ n0).bit_length() - 1) if w.aocl_leaf_index < n0 else 0
        assert int(o["aocl_path_off"][k + 1] - o["aocl_path_off"][k]) == want
    cs = cases.removals
    msa, update, _ = cs.gpu()
    blk = V.Block(cs.msa, 0, cs.recs)
    after = [w for _, w in cs.want[1]]
    k = next(k for k, w in enumerate(after) if any(ci in blk.by_chunk for ci, _, _ in w.target_chunks))
    w = C.to_witness(after[k])
    pos = next(p for p, (ci, _, _) in enumerate(w.target_chunks) if ci in blk.by_chunk)
    ci, path, _ = w.target_chunks[pos]
    w.target_chunks[pos] = (ci, path, MS.Chunk([]))
    o = MS.revert_plan_batch([(msa, update, [w])])
    assert int(o["rel_off"][pos + 1] - o["rel_off"][pos]) == 0 and int(o["entry_off"][1]) == len(w.target_chunks)


def test_two_call_sizing_and_argument_errors(cases):
    import neptune_hip._lib as L
    import neptune_hip.mutator_set as MS
    lib = L.load()
    pu = MS.PackedUpdate([after_job(cs) for cs in (cases.one, cases.small[3])], revert=True)
    assert pu.run(lib) == L.NHIP_OK
    fill = pu.cout
    A, E, PD, RW = int(fill.aocl_digests), int(fill.entries), int(fill.path_digests), int(fill.rel_words)
    assert (A, E, PD, RW) == (int(pu.out["aocl_path_off"][-1]), int(pu.out["entry_off"][-1]),
                              int(pu.out["path_off"][-1]), int(pu.out["rel_off"][-1])) and min(A, E, PD, RW) > 0
    status = np.full(pu.n_witnesses, 0xAB, dtype=np.uint8)
    count = L.MsUpdated(status=status.ctypes.data)
    call = lambda **kw: lib.nhip_ms_revert_plan(  # noqa: E731
        kw.get("block", ctypes.byref(pu.apply.cin)), kw.get("wit", ctypes.byref(pu.win)), kw.get("out", ctypes.byref(count)))
    assert call() == L.NHIP_OK and (status == 0xAB).all()
    assert (int(count.aocl_digests), int(count.entries), int(count.path_digests), int(count.rel_words)) == (A, E, PD, RW)
    assert call(out=None) == L.NHIP_ERR_ARG and call(block=None) == L.NHIP_ERR_ARG and call(wit=None) == L.NHIP_ERR_ARG

    def broken(**kw):
        w = L.MsUpdateIn(*(getattr(pu.win, f) for f, _ in L.MsUpdateIn._fields_))
        for f, v in kw.items():
            setattr(w, f, v)
        return ctypes.byref(w)

    for a in pu.out.values():
        a.reshape(-1).view(np.uint8)[:] = 0xCD
    untouched = lambda: all((a.reshape(-1).view(np.uint8) == 0xCD).all() for a in pu.out.values())  # noqa: E731
    for f in ("wit_off", "minimum", "distances", "aocl_leaf_index", "aocl_leaf", "aocl_path_off", "aocl_path", "chunks"):
        assert call(wit=broken(**{f: None}), out=ctypes.byref(fill)) == L.NHIP_ERR_ARG and untouched(), f
    off = pu.wit_off.copy()
    off[1] = off[2] + 1
    assert call(wit=broken(wit_off=off.ctypes.data), out=ctypes.byref(fill)) == L.NHIP_ERR_ARG and untouched()
    block = L.MsApplyIn(*(getattr(pu.apply.cin, f) for f, _ in L.MsApplyIn._fields_))
    block.rec_off = None
    assert call(block=ctypes.byref(block), out=ctypes.byref(fill)) == L.NHIP_ERR_ARG and untouched()
    for f in ("aocl_cap", "entries_cap", "path_cap", "rel_cap"):
        short = L.MsUpdated(*(getattr(fill, g) for g, _ in L.MsUpdated._fields_))
        setattr(short, f, getattr(short, f) - 1)
        assert call(out=ctypes.byref(short)) == L.NHIP_ERR_ARG and untouched(), f
    for f in ("aocl_path_off", "entry_off", "chunk_index", "path_off", "rel_off"):
        short = L.MsUpdated(*(getattr(fill, g) for g, _ in L.MsUpdated._fields_))
        setattr(short, f, None)
        assert call(out=ctypes.byref(short)) == L.NHIP_ERR_ARG and untouched(), f
    assert call(out=ctypes.byref(fill)) == L.NHIP_OK
    assert int(pu.out["entry_off"][-1]) == E and int(pu.out["rel_off"][-1]) == RW
    # the plan leaves status, aocl_path, path and rel alone
    assert all((pu.out[f].reshape(-1).view(np.uint8) == 0xCD).all() for f in ("status", "aocl_path", "path", "rel"))


def test_plan_and_mirror_step_plain_and_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ absent")
    subprocess.check_call(["make", "-s", "-f", "ms_revert.mk", "-C", NATIVE, f"OUT={tmp_path}"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    for exe in ("ms_revert_check", "ms_revert_check_san"):
        r = subprocess.run([os.path.join(tmp_path, exe)], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, (exe, r.stdout[-2000:], r.stderr[-4000:])
        checks, failures = (int(x) for x in r.stdout.split()[1::2])
        assert checks >= 5000 and failures == 0, (exe, r.stdout)
