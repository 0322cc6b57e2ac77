"""The host side of the archival mutator set's way back across a block (nhip_ms_archive_revert), no
GPU: the null-handle argument errors, the ABI number, and the revert plan (csrc/ms_archive.cpp:
ms_archive_revert_plan / ms_archive_revert_commit) against brute force in tests/native/ms_archive_revert_check.cpp, a
stand-alone program built once plainly and once under ASan + UBSan (nothing is preloaded and nothing runs on a GPU)."""
import os
import shutil
import subprocess

import pytest

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")


def test_null_handles_are_argument_errors():
    import neptune_hip._lib as L
    lib = L.load()
    assert lib.nhip_abi_version() >= 3300
    assert lib.nhip_ms_archive_revert(None, None, None) == L.NHIP_ERR_ARG


def test_the_header_states_the_contract():
    hdr = open(os.path.join(os.path.dirname(NATIVE), "..", "include", "neptune_hip.h")).read()
    decl = "int nhip_ms_archive_revert(nhip_ms_archive *archive, const nhip_ms_apply_in *block, nhip_ms_apply_out *block_out);"
    assert decl in hdr
    comment = hdr[:hdr.index(decl)].rsplit("/*", 1)[1]
    for word in ("NHIP_MS_UPDATE_MISMATCH", "n_jobs == 1", "poisons", "n0 == 0"):
        assert word in comment, word


def test_revert_plan_plain_and_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ absent")
    subprocess.check_call(["make", "-s", "-f", "ms_archive_revert.mk", "-C", NATIVE, f"OUT={tmp_path}"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    for exe in ("ms_archive_revert_check", "ms_archive_revert_check_san"):
        r = subprocess.run([os.path.join(tmp_path, exe)], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, (exe, r.stdout[-2000:], r.stderr[-4000:])
        checks, failures = (int(x) for x in r.stdout.split()[1::2])
        assert checks >= 3000 and failures == 0, (exe, r.stdout)
