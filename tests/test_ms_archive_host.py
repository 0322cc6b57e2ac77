"""The host side of the device-resident archival mutator set (nhip_ms_archive_*), no GPU: the header's
constant against the binding's, null handles, and the host arithmetic (csrc/ms_archive.cpp: level-array geometry, the
build schedule of load, load's shape checks, the path and restore plans, the gather's work units) against brute-force
restatements in tests/native/ms_archive_check.cpp, a stand-alone program built once plainly and once under
ASan + UBSan (nothing is preloaded and nothing runs on a GPU)."""
import ctypes
import os
import shutil
import subprocess

import pytest

import ms_archive_cases as AC

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")


def test_the_tail_constant_is_one_number():
    import neptune_hip._lib as L
    hdr = open(os.path.join(os.path.dirname(NATIVE), "..", "include", "neptune_hip.h")).read()
    assert f"#define NHIP_MS_ARCHIVE_TAIL_NODES {L.MS_ARCHIVE_TAIL_NODES}\n" in hdr
    assert AC.TAIL_NODES == L.MS_ARCHIVE_TAIL_NODES


def test_null_handles_are_argument_errors():
    import neptune_hip._lib as L
    lib = L.load()
    h = ctypes.c_void_p()
    assert lib.nhip_ms_archive_create(None, None, ctypes.byref(h)) == L.NHIP_ERR_ARG and not h
    assert lib.nhip_ms_archive_count(None, None, None, None, None, None) == L.NHIP_ERR_ARG
    assert lib.nhip_ms_archive_load(None, None, 0, None, None, 0, None, 0) == L.NHIP_ERR_ARG
    assert lib.nhip_ms_archive_accumulator(None, None) == L.NHIP_ERR_ARG
    assert lib.nhip_ms_archive_apply(None, None, None) == L.NHIP_ERR_ARG
    assert lib.nhip_ms_archive_paths(None, 0, None, 0, None, None, 0, None) == L.NHIP_ERR_ARG
    assert lib.nhip_ms_archive_leaves(None, 0, 0, 0, None) == L.NHIP_ERR_ARG
    assert lib.nhip_ms_archive_restore(None, None, None, None, 0, None) == L.NHIP_ERR_ARG
    assert lib.nhip_ms_archive_restore_plan(0, None, 0, None, None, None, 0, None) == L.NHIP_ERR_ARG
    lib.nhip_ms_archive_destroy(None)


def test_host_arithmetic_plain_and_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ absent")
    subprocess.check_call(["make", "-s", "-f", "ms_archive.mk", "-C", NATIVE, f"OUT={tmp_path}"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    for exe in ("ms_archive_check", "ms_archive_check_san"):
        r = subprocess.run([os.path.join(tmp_path, exe)], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, (exe, r.stdout[-2000:], r.stderr[-4000:])
        checks, failures = (int(x) for x in r.stdout.split()[1::2])
        assert checks >= 4000 and failures == 0, (exe, r.stdout)
