"""The arithmetic headers under the device compiler and on the hardware, operand by operand: the evaluator
build/arith_dev_check (neptune-core_amd/tools/arith_dev_check.hip) applies goldilocks.hpp, xfe.hpp, tip5_device.hpp
and chain_rules.hpp to the edge and random operands of tests/arith_edges_cases.py in kernels of its own, and every
result is compared bit for bit with Python integers, the C oracle's permutation and tests/block_chain_ref.py.  The
device-only forms are reached here and nowhere else outside the end-to-end tests: the inline-assembly carry-out
forms (mont_mul_n_dev, mds_fold4, mds_reduce_fold), the carry-light forms and the DPP / permlane16_swap
permutations.

The evaluator runs as a child process, one op at a time, under a time limit of its own.  A child that ends on a
signal or at its limit fails its test, and every later test of this module then fails without starting another
child.  The coverage predicates are asserted on the references before any child starts."""
import os
import subprocess

import pytest

import arith_edges_cases as A

pytestmark = pytest.mark.gpu

_dead = []   # why no further child may start


def _run(case, tmp_path, tag=""):
    assert os.path.exists(A.EXE), "build/arith_dev_check missing: run make -C neptune-core_amd (build())"
    if _dead:
        pytest.fail(f"not started: {_dead[0]}")
    try:
        got = A.run_evaluator(case.op, case.inp, tmp_path, host=False, tag=tag)
    except subprocess.TimeoutExpired:
        _dead.append(f"the evaluator's {case.op} child ran into its {A.CHILD_TIMEOUT_S} s limit")
        pytest.fail(_dead[0])
    except A.ChildFailed as e:
        if e.returncode < 0:
            _dead.append(f"the evaluator's {case.op} child ended on signal {-e.returncode}")
        pytest.fail(str(e))
    A.check(case, got)


@pytest.mark.parametrize("op", ["bfe", "mul3", "mdsred", "mds16", "xfe", "bary", "chain"])
def test_device_instantiation_matches_the_reference(tmp_path, op):
    case = A.CASES[op]()
    A.assert_coverage(case)
    _run(case, tmp_path)


def test_tip5_every_form_three_workgroups(tmp_path):
    """700 states: three lane-form workgroups, the last partly filled; 44 row-form, 88 pair-form and 11 quad-form
    workgroups.  Every form gives the oracle's permutation; tip5_hash_pair_digest gives its digest."""
    case = A.tip5_case()
    A.assert_coverage(case)
    _run(case, tmp_path)


@pytest.mark.parametrize("count", A.TIP5_COUNTS)
def test_tip5_idle_rows_pairs_and_quads(tmp_path, count):
    """1, 3, 5, 17 and 67 states: the last wave has idle rows, an idle row pair and idle quads, which leave whole."""
    _run(A.tip5_prefix(A.tip5_case(), count), tmp_path, tag=str(count))
