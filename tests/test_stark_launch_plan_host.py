"""stark_launch_plan.hpp, the launch schedule of a STARK batch, compiled for the host (tests/native/
stark_launch_plan_check.cpp): the plan, walked by a recording enqueue, against a transcription of the
launch function it was split from (every kernel, stream, grid, block, decision argument, timed slot,
event record and wait, over ~1.7 million shapes and modes), the properties of a plan (waits follow
their records across streams, one release of the aux chain, ascending levels, timed slots in order,
no empty grid), and every launch kind and branch reached.  Plain and under ASan + UBSan (host code
only, run as a program of its own).  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SAN = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
       "-Xarch_host", "-fno-sanitize-recover=all"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fno-omit-frame-pointer"] + SAN], ids=["plain", "asan_ubsan"])
def test_plan_equals_the_restated_launch(tmp_path, flags):
    exe = tmp_path / "stark_launch_plan_check"
    subprocess.check_call([HIPCC, *flags, "-std=c++17", "-x", "hip", "--offload-arch=gfx950",
                           "-I", os.path.join(ROOT, "neptune-core_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "stark_launch_plan_check.cpp"), "-o", str(exe)],
                          stderr=subprocess.DEVNULL)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad 0" in out.stdout
