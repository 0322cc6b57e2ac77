"""The host side of the device-resident witness store (nhip_ms_store_*), no GPU: the binding's
prototypes, the ABI version, a fresh store's counts, and the mirror arithmetic (csrc/ms_store.cpp) against brute-force
restatements in tests/native/ms_store_check.cpp, a stand-alone program built once plainly and once under ASan + UBSan
(nothing is preloaded and nothing runs on a GPU)."""
import ctypes
import os
import shutil
import subprocess

import pytest

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
ENTRY_POINTS = {"nhip_ms_store_create": 3, "nhip_ms_store_destroy": 1, "nhip_ms_store_count": 6, "nhip_ms_store_append": 3,
                "nhip_ms_store_update": 4, "nhip_ms_store_read": 4, "nhip_ms_store_retain": 2, "nhip_ms_store_check": 6}


def test_abi_and_prototypes():
    import neptune_hip._lib as L
    import neptune_hip.mutator_set as MS
    lib = L.load()
    assert lib.nhip_abi_version() >= 3000
    for name, argc in ENTRY_POINTS.items():
        assert len(L.SIGNATURES[name][0]) == argc and hasattr(lib, name), name
    assert L.SIGNATURES["nhip_ms_store_destroy"][1] is None
    assert ctypes.sizeof(L.MsStoreCaps) == 5 * ctypes.sizeof(ctypes.c_size_t)
    hdr = open(os.path.join(os.path.dirname(NATIVE), "..", "include", "neptune_hip.h")).read()
    assert f"#define NHIP_MS_STORE_GATHER_UNIT {L.MS_STORE_GATHER_UNIT}\n" in hdr
    for method in ("append", "update", "read", "retain", "check", "counts", "close", "__len__"):
        assert callable(getattr(MS.WitnessStore, method)), method


def test_a_fresh_store_counts_nothing():
    import neptune_hip as nh
    import neptune_hip.mutator_set as MS
    try:
        ctx = nh.Context(0)
    except nh.NhipError:
        pytest.skip("creating a context needs a device")
    with ctx, MS.WitnessStore(ctx, dict(witnesses=1, aocl_digests=2, entries=1, path_digests=2, rel_words=3)) as store:
        assert store.counts() == (0, 0, 0, 0, 0) and len(store) == 0 and store.read() == []


def test_null_handles_are_argument_errors():
    import neptune_hip._lib as L
    lib = L.load()
    h = ctypes.c_void_p()
    assert lib.nhip_ms_store_create(None, None, ctypes.byref(h)) == L.NHIP_ERR_ARG and not h
    assert lib.nhip_ms_store_count(None, None, None, None, None, None) == L.NHIP_ERR_ARG
    assert lib.nhip_ms_store_append(None, None, 0) == L.NHIP_ERR_ARG
    assert lib.nhip_ms_store_update(None, None, None, None) == L.NHIP_ERR_ARG
    assert lib.nhip_ms_store_read(None, None, 0, None) == L.NHIP_ERR_ARG
    assert lib.nhip_ms_store_retain(None, None) == L.NHIP_ERR_ARG
    assert lib.nhip_ms_store_check(None, None, None, None, None, None) == L.NHIP_ERR_ARG
    lib.nhip_ms_store_destroy(None)


def test_mirror_arithmetic_plain_and_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ absent")
    subprocess.check_call(["make", "-s", "-f", "ms_store.mk", "-C", NATIVE, f"OUT={tmp_path}"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    for exe in ("ms_store_check", "ms_store_check_san"):
        r = subprocess.run([os.path.join(tmp_path, exe)], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, (exe, r.stdout[-2000:], r.stderr[-4000:])
        checks, failures = (int(x) for x in r.stdout.split()[1::2])
        assert checks >= 5000 and failures == 0, (exe, r.stdout)
