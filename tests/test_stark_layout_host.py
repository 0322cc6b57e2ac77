"""stark_layout.hpp, the host arithmetic of a STARK batch, compiled for the host (tests/native/
stark_layout_check.cpp): every named scratch buffer against the flat size table it replaced, offsets
ascending, aligned and disjoint, the readback description, the multiproof capacities against the
restated loop and against the parent counts of every set of revealed leaves, and the batch sizing on
malformed, short, mixed-height and two-form proofs.  Plain and under ASan + UBSan (host code only, run
as a program of its own).  CPU only."""
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
def test_layout_readback_capacities_and_sizing(tmp_path, flags):
    exe = tmp_path / "stark_layout_check"
    subprocess.check_call([HIPCC, *flags, "-std=c++17", "-x", "hip", "--offload-arch=gfx950",
                           "-I", os.path.join(ROOT, "neptune-core_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "stark_layout_check.cpp"), "-o", str(exe)],
                          stderr=subprocess.DEVNULL)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad 0" in out.stdout
