"""The byte-planes MDS on the hardware: build/mds_planes_dev_check (neptune-core_amd/tools/mds_planes_dev_check.hip)
runs mds_ark_planes, tip5_permute_raw, the absorb form (tip5_rounds_0_3 + the last round) and tip5_hash_pair_digest
with the planes form as their template argument, one state per lane, and every word is compared bit for bit with
Python integers (one round's MDS + ARK) and the C oracle's permutation: states of all 0x00, 0xFF, 0x80, 0x7F bytes
and words p - 1, the 128 one-hot bytes with 0x01 and 0xFF, states that encode their own index, and 1,000 random
ones.  The kernels as launched are checked by the end-to-end tests.

The evaluator runs as a child process under a time limit of its own.  A child that ends on a signal or at its
limit fails its test, and every later test of this module then fails without starting another child."""
import os
import subprocess

import pytest

import mds_planes_cases as M

pytestmark = pytest.mark.gpu

_dead = []   # why no further child may start


def _run(count, tmp_path):
    assert os.path.exists(M.EXE), "build/mds_planes_dev_check missing: run make -C neptune-core_amd (build())"
    if _dead:
        pytest.fail(f"not started: {_dead[0]}")
    inp, want = M.case()
    inp, want = inp[:count], want[:count]
    try:
        got = M.run_evaluator(inp, tmp_path, tag=str(count))
    except subprocess.TimeoutExpired:
        _dead.append(f"the evaluator's child ran into its {M.CHILD_TIMEOUT_S} s limit")
        pytest.fail(_dead[0])
    except M.ChildFailed as e:
        if e.returncode < 0:
            _dead.append(f"the evaluator's child ended on signal {-e.returncode}")
        pytest.fail(str(e))
    M.check(inp, want, got)


def test_planes_forms_match_the_references_six_workgroups(tmp_path):
    """Every state: five whole workgroups and a partly filled sixth."""
    inp, _ = M.case()
    assert inp.shape[0] == 5 + 123 + 256 + 1000
    _run(inp.shape[0], tmp_path)


@pytest.mark.parametrize("count", M.COUNTS)
def test_planes_forms_with_idle_lanes(tmp_path, count):
    """1 to 67 states: the wave's other lanes took their constant tiles and left; lanes 32..63 idle (31, 32),
    one lane of the upper half busy (33), one idle (63), a second wave of 1 and 3 lanes (65, 67)."""
    _run(count, tmp_path)
