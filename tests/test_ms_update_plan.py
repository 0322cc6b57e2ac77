"""nhip_ms_update_plan, the host half of nhip_ms_update_batch, through ctypes (no GPU): every shape array against the
shapes of the witnesses tests/ms_update_ref.py gives for the jobs of tests/ms_update_cases.py, many jobs in one call
against the jobs alone, the two-call sizing, the shape errors, and the plan under ASan + UBSan
(tests/native/ms_update_plan_check.cpp, a stand-alone program; nothing is preloaded and nothing runs on a GPU)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import ms_ref as R
import ms_update_cases as C

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")


@pytest.fixture(scope="module")
def cases():
    return C.cases()


def _plan(group):
    import neptune_hip.mutator_set as MS
    return MS.update_plan_batch([cs.gpu() for cs in group])


def _check(group):
    """The plan of `group` in one call against the helper's witnesses after, witness by witness; a witness the helper
    rejects has no shape of its own there and keeps whatever range the plan gives it."""
    o = _plan(group)
    n_wit = sum(len(cs.wits) for cs in group)
    for name in ("aocl_path_off", "entry_off"):
        assert len(o[name]) == n_wit + 1 and int(o[name][0]) == 0 and (np.diff(o[name].astype(np.int64)) >= 0).all()
    E = int(o["entry_off"][-1])
    assert len(o["chunk_index"]) == E and len(o["path_off"]) == len(o["rel_off"]) == E + 1
    assert int(o["path_off"][0]) == int(o["rel_off"][0]) == 0
    i, compared = 0, 0
    for cs in group:
        for st, w in cs.want[1]:
            lo, hi = int(o["entry_off"][i]), int(o["entry_off"][i + 1])
            if st == R.OK:
                assert int(o["aocl_path_off"][i + 1] - o["aocl_path_off"][i]) == len(w.auth_path_aocl), cs.label
                assert [int(x) for x in o["chunk_index"][lo:hi]] == [ci for ci, _, _ in w.target_chunks], cs.label
                assert [int(x) for x in np.diff(o["path_off"][lo:hi + 1])] == [len(p) for _, p, _ in w.target_chunks], cs.label
                assert [int(x) for x in np.diff(o["rel_off"][lo:hi + 1])] == \
                    [len(ch.relative_indices) for _, _, ch in w.target_chunks], cs.label
                compared += 1
            i += 1
    assert not o["status"].any() and not o["aocl_path"].any() and not o["path"].any() and not o["rel"].any()
    return o, compared


def test_abi_and_signatures():
    import neptune_hip._lib as L
    lib = L.load()
    assert lib.nhip_abi_version() >= 2900
    for name, argc in (("nhip_ms_update_plan", 3), ("nhip_ms_update_batch", 5)):
        assert len(L.SIGNATURES[name][0]) == argc and hasattr(lib, name)
    assert ctypes.sizeof(L.MsUpdateIn) == 64 and ctypes.sizeof(L.MsUpdated) == 9 * 8 + 8 * 8


def test_every_job_alone_equals_the_helper(cases):
    total = 0
    for cs in C.everything(cases):
        total += _check([cs])[1]
    assert total > 5000


def test_many_jobs_in_one_call_equal_the_jobs_alone(cases):
    jobs = cases.small + [cases.one, cases.born, cases.with_mutants] + cases.rejected_jobs + cases.neighbours + [cases.wide]
    alone = [_check([cs])[0] for cs in jobs]
    for group, parts in ((jobs, alone), (jobs[::-1], alone[::-1])):
        o, _ = _check(group)
        for name in ("aocl_path_off", "entry_off", "path_off", "rel_off"):
            want = np.concatenate([[0]] + [np.diff(p[name].astype(np.int64)) for p in parts]).cumsum()
            assert (o[name].astype(np.int64) == want).all(), name
        assert (o["chunk_index"] == np.concatenate([p["chunk_index"] for p in parts])).all()
    o, _ = _check([])
    assert all(int(o[name][0]) == 0 for name in ("aocl_path_off", "entry_off", "path_off", "rel_off"))


def test_two_call_sizing_and_shape_errors(cases):
    import neptune_hip._lib as L
    import neptune_hip.mutator_set as MS
    lib = L.load()
    pu = MS.PackedUpdate([cs.gpu() for cs in (cases.one, cases.small[3])])
    assert pu.run(lib) == L.NHIP_OK
    fill = pu.cout
    A, E, PD, RW = int(fill.aocl_digests), int(fill.entries), int(fill.path_digests), int(fill.rel_words)
    assert (A, E, PD, RW) == (int(pu.out["aocl_path_off"][-1]), int(pu.out["entry_off"][-1]),
                              int(pu.out["path_off"][-1]), int(pu.out["rel_off"][-1])) and min(A, E, PD, RW) > 0
    status = np.full(pu.n_witnesses, 0xAB, dtype=np.uint8)
    count = L.MsUpdated(status=status.ctypes.data)
    call = lambda **kw: lib.nhip_ms_update_plan(  # noqa: E731
        kw.get("block", ctypes.byref(pu.apply.cin)), kw.get("wit", ctypes.byref(pu.win)), kw.get("out", ctypes.byref(count)))
    assert call() == L.NHIP_OK and (status == 0xAB).all()
    assert (int(count.aocl_digests), int(count.entries), int(count.path_digests), int(count.rel_words)) == (A, E, PD, RW)
    assert call(out=None) == L.NHIP_ERR_ARG and call(block=None) == L.NHIP_ERR_ARG and call(wit=None) == L.NHIP_ERR_ARG

    def broken(**kw):
        w = L.MsUpdateIn(*(getattr(pu.win, f) for f, _ in L.MsUpdateIn._fields_))
        for f, v in kw.items():
            setattr(w, f, v)
        return ctypes.byref(w)

    for f in ("wit_off", "minimum", "distances", "aocl_leaf_index", "aocl_leaf", "aocl_path_off", "aocl_path", "chunks"):
        assert call(wit=broken(**{f: None})) == L.NHIP_ERR_ARG, f  # a null pointer with a non-zero count
    off = pu.wit_off.copy()
    off[0] = 1
    assert call(wit=broken(wit_off=off.ctypes.data)) == L.NHIP_ERR_ARG  # offsets that do not start at 0
    off = pu.wit_off.copy()
    off[1] = off[2] + 1
    assert call(wit=broken(wit_off=off.ctypes.data)) == L.NHIP_ERR_ARG  # ... or decrease
    off = pu.aocl_path_off.copy()
    off[3], off[4] = off[4] + 1, off[3]
    assert call(wit=broken(aocl_path_off=off.ctypes.data)) == L.NHIP_ERR_ARG
    eo = pu.packed.entry_off.copy()
    eo[1], eo[2] = eo[2] + 1, eo[1]
    bad_chunks = L.MsChunks(eo.ctypes.data, pu.chunks.chunk_index, pu.chunks.path_off, pu.chunks.path,
                            pu.chunks.rel_off, pu.chunks.rel)
    assert call(wit=broken(chunks=ctypes.pointer(bad_chunks))) == L.NHIP_ERR_ARG
    block = L.MsApplyIn(*(getattr(pu.apply.cin, f) for f, _ in L.MsApplyIn._fields_))
    block.add_off = None
    assert call(block=ctypes.byref(block)) == L.NHIP_ERR_ARG
    # the fill pass: a capacity too small or an offset array missing leaves the arrays untouched
    before = {f: a.copy() for f, a in pu.out.items()}
    for f in ("aocl_cap", "entries_cap", "path_cap", "rel_cap"):
        short = L.MsUpdated(*(getattr(fill, g) for g, _ in L.MsUpdated._fields_))
        setattr(short, f, getattr(short, f) - 1)
        for a in pu.out.values():
            a.reshape(-1).view(np.uint8)[:] = 0xCD
        assert call(out=ctypes.byref(short)) == L.NHIP_ERR_ARG, f
        assert all((a.reshape(-1).view(np.uint8) == 0xCD).all() for a in pu.out.values()), f
    for f in ("aocl_path_off", "entry_off", "chunk_index", "path_off", "rel_off"):
        short = L.MsUpdated(*(getattr(fill, g) for g, _ in L.MsUpdated._fields_))
        setattr(short, f, None)
        assert call(out=ctypes.byref(short)) == L.NHIP_ERR_ARG, f
    assert call(out=ctypes.byref(fill)) == L.NHIP_OK
    for f in ("aocl_path_off", "entry_off", "chunk_index", "path_off", "rel_off"):
        assert (pu.out[f] == before[f]).all(), f
    # the plan leaves status, aocl_path, path and rel alone
    assert all((pu.out[f].reshape(-1).view(np.uint8) == 0xCD).all() for f in ("status", "aocl_path", "path", "rel"))


def test_plan_clean_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ absent")
    subprocess.check_call(["make", "-s", "-f", "ms_update_plan.mk", "-C", NATIVE, f"OUT={tmp_path}"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(tmp_path, "ms_update_plan_check")], capture_output=True, text=True, timeout=120,
                       env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    checks, failures = (int(x) for x in r.stdout.split()[1::2])
    assert checks >= 1000 and failures == 0, r.stdout
