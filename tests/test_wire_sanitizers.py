"""The in-place scanners (nhip_wire_scan_txs / nhip_wire_scan_blocks) under ASan + UBSan,
host only: a stand-alone program (tests/native/wire_scan_check.cpp, built by tests/native/wire.mk with the
sanitizer flags of tests/native/Makefile) scans valid streams, every truncation and seeded mutations,
each from the end of an exactly sized heap block, and checks that every span it is handed lies inside
the buffer and that the upload plan made from the spans covers them.  Nothing runs on a GPU and nothing
is loaded into Python; a sanitizer report or a failed check fails the run."""
import os
import random
import shutil
import subprocess

import pytest

import bincode_ref as B

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")


@pytest.fixture(scope="module")
def check_bin(tmp_path_factory):
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc absent")
    out = tmp_path_factory.mktemp("wire_san")
    subprocess.check_call(["make", "-s", "-f", "wire.mk", "-C", NATIVE, f"OUT={out}"])
    return os.path.join(out, "wire_scan_check")


def test_wire_scanners_clean_under_asan_ubsan(check_bin, tmp_path):
    from test_blocks_host import H, _blocks, _proof_collection
    assert H == 10
    rng = random.Random(91)
    single = lambda n: {"kernel": B.random_kernel(rng), "kind": B.TT_SINGLE_PROOF,  # noqa: E731
                        "proof": [rng.randrange(B.P) for _ in range(n)]}
    # spans of at most 3 proofs per transaction resume with span_cap 3; the 7-proof collection does not
    txs = [single(40), single(0), single(13)]
    small = b"".join(B.encode_transfer_transaction(t) for t in txs)
    mixed = b"".join(B.encode_transfer_transaction(t) for t in (
        single(21), {"kernel": B.random_kernel(rng), "kind": B.TT_PROOF_COLLECTION,
                     "proof": _proof_collection(rng, 2, 1, 3)}, single(9)))
    blk = b"".join(B.encode_block(b) for b in _blocks(3, 4))
    args = []
    for kind, name, data in (("txs", "small.bin", small), ("txs", "mixed.bin", mixed), ("blk10", "blk.dat", blk)):
        path = tmp_path / name
        path.write_bytes(data)
        args.append(f"{kind}:{path}")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([check_bin, "2000"] + args, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    runs, ok, bad = (int(x) for x in r.stdout.split()[1::2])
    assert runs > 8000 and ok > 0 and bad == 0, r.stdout
