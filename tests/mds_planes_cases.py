"""States, references and the child-process runner for the byte-planes MDS evaluator
(neptune-core_amd/tools/mds_planes_dev_check.hip) — TEST HELPER ONLY (not collected).

Every expected value is made here from Python integers (the MDS + ARK of one round) and the C oracle's
permutation (coracle); nothing is taken from the headers under test.  The case is built once per process and
left unchanged.  Records are raw Montgomery words r = x * 2^64 mod p, any 64-bit word for the MDS alone (the
permutations take the words mod p).

The states, in this order, so that every prefix the tests run holds some of each kind that fits:
    5    every byte 0x00, 0xFF, 0x80, 0x7F, and every word p - 1
    123  states that encode their own index in every word (a lane-half, row or lane mix-up moves one)
    256  the 128 one-hot bytes with values 0x01 and 0xFF
    1000 random canonical states
"""
from __future__ import annotations

import functools
import os
import random
import subprocess

import numpy as np

import tip5_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "neptune-core_amd", "build", "mds_planes_dev_check")

P = (1 << 64) - (1 << 32) + 1
RR = 1 << 64
RINV = pow(RR, -1, P)
IN_WORDS, OUT_WORDS = 17, 53
CHILD_TIMEOUT_S = 120
COUNTS = [1, 31, 32, 33, 63, 64, 65, 67]      # idle lanes in either lane half, a partly filled second wave
RC_RAW = [c * RR % P for c in T.ROUND_CONSTANTS]
MDS = list(T.MDS_FIRST_COLUMN)


class ChildFailed(Exception):
    """The evaluator ended with a non-zero exit code (negative: on a signal)."""

    def __init__(self, returncode, text):
        super().__init__(f"mds_planes_dev_check exit {returncode}: {text}")
        self.returncode = returncode


def states():
    g = random.Random(0x9A7E5)
    out = [[0] * 16, [(1 << 64) - 1] * 16, [0x8080808080808080] * 16, [0x7F7F7F7F7F7F7F7F] * 16, [P - 1] * 16]
    while len(out) < 128:
        n = len(out)
        out.append([((n + 1) << 48) | (j << 40) | ((n & 63) << 8) | (n >> 6 << 4) | j for j in range(16)])
    for v in (0x01, 0xFF):
        for b in range(128):
            s = [0] * 16
            s[b >> 3] = v << (8 * (b & 7))
            out.append(s)
    out += [[g.randrange(P) for _ in range(16)] for _ in range(1000)]
    return out


@functools.lru_cache(maxsize=None)
def case():
    """(inp [n, 17], want [n, 53]) as uint64."""
    import coracle as C
    st = states()
    n = len(st)
    assert n % 256 != 0 and n > 4 * 256
    want = np.zeros((n, OUT_WORDS), dtype=object)
    rounds = [i % 5 for i in range(n)]
    for i, (s, r) in enumerate(zip(st, rounds)):
        for o in range(16):
            want[i, o] = (sum(MDS[(o - j) & 15] * s[j] for j in range(16)) + RC_RAW[16 * r + o]) % P
    canon = np.array([[w % P * RINV % P for w in s] for s in st], dtype=object).astype(np.uint64)
    perm = C.permutation_batch(canon)
    fixed = canon.copy()
    fixed[:, 10:] = 1
    digest = C.permutation_batch(fixed)[:, :5]
    to_raw = np.vectorize(lambda v: int(v) * RR % P, otypes=[object])
    want[:, 16:32] = want[:, 32:48] = to_raw(perm)
    want[:, 48:53] = to_raw(digest)
    inp = np.array([s + [r] for s, r in zip(st, rounds)], dtype=object).astype(np.uint64)
    return inp, want.astype(np.uint64)


def run_evaluator(inp: np.ndarray, tmp_path, tag: str) -> np.ndarray:
    """One child process; raises subprocess.TimeoutExpired at the limit and ChildFailed on a non-zero exit."""
    src, dst = os.path.join(str(tmp_path), f"planes{tag}.in"), os.path.join(str(tmp_path), f"planes{tag}.out")
    np.ascontiguousarray(inp, dtype="<u8").tofile(src)
    out = subprocess.run([EXE, src, dst], capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    if out.returncode != 0:
        raise ChildFailed(out.returncode, out.stdout + out.stderr)
    return np.fromfile(dst, dtype="<u8").astype(np.uint64).reshape(inp.shape[0], OUT_WORDS)


FIELDS = [(0, 16, "mds_ark_planes"), (16, 32, "tip5_permute_raw"), (32, 48, "tip5_rounds_0_3 + last round"),
          (48, 53, "tip5_hash_pair_digest")]


def check(inp, want, got):
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.argwhere(got != want)
    if len(bad):
        name = lambda c: next(nm for a, b, nm in FIELDS if a <= c < b)            # noqa: E731
        lines = [f"record {r} (lane {r % 64}) {name(c)} word {c}: got {int(got[r, c]):#x} want {int(want[r, c]):#x} "
                 f"state {[hex(int(x)) for x in inp[r][:16]]}" for r, c in bad[:8]]
        raise AssertionError(f"{len(bad)} mismatching words\n" + "\n".join(lines))
