"""The byte-planes form of the Tip5 MDS + ARK (tip5_mds_planes.hpp) in host integers: digits, offset,
the 24 dot products, the biased start constants and the fold equal twenty-first's step-by-step form
for every round constant, with every range the device code relies on asserted.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_mds_planes_form_matches_stepwise(tmp_path):
    exe = tmp_path / "mds_planes_check"
    subprocess.check_call([HIPCC, "-O2", "-std=c++17", "-x", "hip", "--offload-arch=gfx950",
                           "-I", os.path.join(ROOT, "neptune-core_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "mds_planes_check.cpp"), "-o", str(exe)],
                          stderr=subprocess.DEVNULL)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad 0" in out.stdout
