"""The consensus integers of a block's transaction rules and guesser-fee UTXOs (csrc/tx_rules.hpp) and the host walk
behind nhip_blk_ms_walk (csrc/bincode.cpp, csrc/blk_ms_parts.cpp) under ASan + UBSan: a stand-alone program
(tests/native/tx_rules_check.cpp, built by tests/native/tx_rules.mk) that compares them with a naive recomputation on
__int128 and walks a block truncated at every byte of its kernel; nothing is preloaded, nothing is loaded into Python
and nothing runs on a GPU."""
import os
import shutil
import subprocess

import pytest

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")


def test_tx_rules_and_host_walk_clean_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ absent")
    subprocess.check_call(["make", "-s", "-f", "tx_rules.mk", "-C", NATIVE, f"OUT={tmp_path}"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(tmp_path, "tx_rules_check")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    checks, failures = (int(x) for x in r.stdout.split()[1::2])
    assert checks >= 90000 and failures == 0, r.stdout
