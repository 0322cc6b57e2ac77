"""The consensus integers of the header-chain rules (csrc/chain_rules.hpp) and the shape checks of their entry
points (csrc/chain_shape.cpp) under ASan + UBSan: a stand-alone program (tests/native/chain_rules_check.cpp, built
by tests/native/chain_rules.mk) that compares them with a naive bit-by-bit recomputation; nothing is preloaded,
nothing is loaded into Python and nothing runs on a GPU."""
import os
import shutil
import subprocess

import pytest

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")


def test_chain_rules_clean_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ absent")
    subprocess.check_call(["make", "-s", "-f", "chain_rules.mk", "-C", NATIVE, f"OUT={tmp_path}"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(tmp_path, "chain_rules_check")], capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    checks, failures = (int(x) for x in r.stdout.split()[1::2])
    assert checks >= 9600 and failures == 0, r.stdout
