"""The workspace layout of the host-buffer C ABI calls (csrc/stage_layout.hpp) under ASan + UBSan: a
stand-alone program (tests/native/stage_layout_check.cpp, built by tests/native/stage_layout.mk); nothing is
preloaded and nothing runs on a GPU."""
import os
import shutil
import subprocess

import pytest

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")


def test_stage_layout_clean_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ absent")
    subprocess.check_call(["make", "-s", "-f", "stage_layout.mk", "-C", NATIVE, f"OUT={tmp_path}"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(tmp_path, "stage_layout_check")], capture_output=True, text=True, timeout=120,
                       env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    checks, failures = (int(x) for x in r.stdout.split()[1::2])
    assert checks >= 300 and failures == 0, r.stdout
