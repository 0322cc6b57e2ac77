"""nhip_ms_unpack_plan, the host half of block rule 2.a, through ctypes (no GPU): statuses and every shape array
against the restatement tests/ms_pack_ref.py for the good lists and the mutants of tests/ms_pack_cases.py, several
jobs in one call against the jobs alone, the shape errors, and the plan under ASan + UBSan (tests/native/
ms_unpack_plan_check.cpp, a stand-alone program; nothing is preloaded and nothing runs on a GPU)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import ms_pack_cases as C
import ms_pack_ref as K

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")


def _expected_shape(jobs):
    """(entry_off, chunk_index, path lengths, rel lengths, rel) of the restatement's answers, a failed job's records
    owning no entry."""
    entry_off, ci, plen, rlen, rel = [0], [], [], [], []
    for _, packed, status, records in jobs:
        for k in range(len(packed)):
            for c, path, chunk in (records[k].target_chunks if status == 0 else []):
                ci.append(c)
                plen.append(len(path))
                rlen.append(len(chunk.relative_indices))
                rel += chunk.relative_indices
            entry_off.append(len(ci))
    return entry_off, ci, plen, rlen, rel


def _check(jobs):
    import neptune_hip.mutator_set as MS
    status, leafs, u = MS.unpack_plan_batch([C.to_library(p) for _, p, _, _ in jobs])
    assert [int(s) for s in status] == [s for _, _, s, _ in jobs], [n for n, _, _, _ in jobs]
    entry_off, ci, plen, rlen, rel = _expected_shape(jobs)
    assert [int(x) for x in u.entry_off] == entry_off
    assert [int(x) for x in u.chunk_index] == ci
    assert [int(x) for x in np.diff(u.path_off)] == plen and int(u.path_off[0]) == 0
    assert [int(x) for x in np.diff(u.rel_off)] == rlen and int(u.rel_off[0]) == 0
    assert [int(x) for x in u.rel] == rel
    for (_, packed, st, _), n in zip(jobs, leafs):
        want = K.decode_from_vec(packed).num_leafs_aocl if st == 0 else 0
        assert int(n) == want
    return status, u


def test_abi_and_signatures():
    import neptune_hip._lib as L
    lib = L.load()
    assert lib.nhip_abi_version() >= 2800
    for name, argc in (("nhip_ms_unpack_plan", 6), ("nhip_ms_unpack_batch", 7), ("nhip_ms_apply_batch_packed", 3)):
        assert len(L.SIGNATURES[name][0]) == argc and hasattr(lib, name)


@pytest.mark.parametrize("k", range(len(C.batch())))
def test_one_job_equals_the_restatement(k):
    _check([C.batch()[k]])


def test_many_jobs_in_one_call_equal_the_jobs_alone():
    jobs = list(C.batch())
    assert {s for _, _, s, _ in jobs} >= set(range(K.PAYLOAD_TOO_BIG, K.UNPACK_PANIC + 1)) | {0}
    _check(jobs)
    _check(jobs[::-1])
    _check([])


def test_regression_inputs_and_empty_shapes(golden_dir):
    import json
    import ms_ref as R
    pins = json.load(open(os.path.join(golden_dir, "ms_pack_pins.json")))
    jobs = []
    for k, pin in enumerate(pins["regressions"]["inputs"]):
        rec = R.Record(R.IndexSet(int(pin["minimum"]), list(pin["distances"])),
                       [(key, [], R.Chunk(list(rel))) for key, _, rel in pin["dictionary"]])
        jobs.append(("regression%d" % k, [rec]) + K.try_unpack_status([rec]))
    assert [s for _, _, s, _ in jobs] == [p["returns"]["status"] for p in pins["regressions"]["inputs"]]
    _check(jobs)
    _check([("none", [], 0, [])] * 3)  # jobs without records


def test_shape_errors():
    import neptune_hip._lib as L
    import neptune_hip.mutator_set as MS
    lib = L.load()
    pl = MS.PackedLists([C.to_library(K.pack(C.two_trees()))])
    status = np.zeros(1, dtype=np.uint8)
    out = L.MsUnpacked(status=status.ctypes.data)
    call = lambda **kw: lib.nhip_ms_unpack_plan(  # noqa: E731
        kw.get("rec_off", pl.rec_off.ctypes.data), kw.get("n", 1), kw.get("minimum", pl.minimum.ctypes.data),
        pl.distances.ctypes.data, kw.get("chunks", ctypes.byref(pl.chunks)), kw.get("out", ctypes.byref(out)))
    assert call() == L.NHIP_OK and out.entries == 5 and out.path_digests == 6 and status[0] == 0
    assert call(out=None) == L.NHIP_ERR_ARG
    assert call(rec_off=None) == L.NHIP_ERR_ARG
    assert call(minimum=None) == L.NHIP_ERR_ARG  # a null pointer with a non-zero count
    assert call(chunks=None) == L.NHIP_ERR_ARG
    bad = pl.rec_off.copy()
    bad[0] = 1
    assert call(rec_off=bad.ctypes.data) == L.NHIP_ERR_ARG  # offsets that do not start at 0
    dec = np.array([0, 3, 2], dtype=np.uint64)
    assert call(rec_off=dec.ctypes.data, n=2) == L.NHIP_ERR_ARG  # ... or decrease
    eo = pl.packed.entry_off.copy()
    eo[1], eo[2] = eo[2] + 1, eo[1]
    broken = L.MsChunks(eo.ctypes.data, pl.chunks.chunk_index, pl.chunks.path_off, pl.chunks.path, pl.chunks.rel_off,
                        pl.chunks.rel)
    assert call(chunks=ctypes.byref(broken)) == L.NHIP_ERR_ARG
    # the fill pass: capacities too small, or an array missing
    E = int(out.entries)
    a = [np.zeros(max(k, 1), dtype=np.uint64) for k in (len(pl.rec_off) + 2, E, E + 1, E + 1)]
    rel = np.zeros(int(out.rel_words) + 1, dtype=np.uint32)
    fill = L.MsUnpacked(status=status.ctypes.data, entry_off=a[0].ctypes.data, chunk_index=a[1].ctypes.data,
                        path_off=a[2].ctypes.data, rel_off=a[3].ctypes.data, rel=rel.ctypes.data,
                        entries_cap=E - 1, path_cap=int(out.path_digests), rel_cap=int(out.rel_words))
    assert call(out=ctypes.byref(fill)) == L.NHIP_ERR_ARG
    fill.entries_cap, fill.rel_cap = E, int(out.rel_words) - 1
    assert call(out=ctypes.byref(fill)) == L.NHIP_ERR_ARG
    fill.rel_cap, fill.rel_off = int(out.rel_words), None
    assert call(out=ctypes.byref(fill)) == L.NHIP_ERR_ARG
    fill.rel_off = a[3].ctypes.data
    assert call(out=ctypes.byref(fill)) == L.NHIP_OK and int(a[0][3]) == E


def test_plan_clean_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ absent")
    subprocess.check_call(["make", "-s", "-f", "ms_unpack_plan.mk", "-C", NATIVE, f"OUT={tmp_path}"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(tmp_path, "ms_unpack_plan_check")], capture_output=True, text=True, timeout=120,
                       env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    checks, failures = (int(x) for x in r.stdout.split()[1::2])
    assert checks >= 1000 and failures == 0, r.stdout
