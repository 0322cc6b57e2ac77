"""The arithmetic evaluator without a GPU: neptune-core_amd/tools/arith_dev_check.hip is built, `list` names the
ops and record sizes, and every op offered with --host (the host instantiation of goldilocks.hpp, xfe.hpp and
chain_rules.hpp) runs over the operand sets of tests/arith_edges_cases.py against their references, bit for bit.
The coverage predicates of every op's operands, the device-only ones included, are asserted on the references
alone.  A fault in a reference or a record format shows here; tests/test_gpu_arith_edges.py runs the same sets
through the device instantiation.  Nothing is preloaded and nothing is loaded into Python."""
import subprocess

import pytest

import arith_edges_cases as A

HOST_OPS = [op for op, (_, _, host) in A.OPS.items() if host]


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", A.PKG, "build/arith_dev_check"])
    return A.EXE


def test_list_names_every_op_and_record_size(exe):
    out = subprocess.run([exe, "list"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    got = {}
    for line in out.stdout.strip().splitlines():
        w = line.split()
        got[w[0]] = (int(w[1]), int(w[2]), w[3:] == ["host"])
    assert got == A.OPS


def test_device_only_ops_refuse_the_host_path(exe, tmp_path):
    for op, (_, _, host) in A.OPS.items():
        if not host:
            out = subprocess.run([exe, "--host", op, str(tmp_path / "none"), str(tmp_path / "out")],
                                 capture_output=True, text=True, timeout=60)
            assert out.returncode == 2 and "device only" in out.stderr, op


@pytest.mark.parametrize("op", list(A.OPS))
def test_operands_reach_every_edge(op):
    A.assert_coverage(A.CASES[op]())


@pytest.mark.parametrize("op", HOST_OPS)
def test_host_instantiation_matches_the_reference(exe, tmp_path, op):
    case = A.CASES[op]()
    A.assert_coverage(case)
    A.check(case, A.run_evaluator(op, case.inp, tmp_path, host=True))
