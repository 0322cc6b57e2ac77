#!/usr/bin/env python3
"""Rate of the block digests on one GPU: --blocks synthetic blocks (default 64 and 256) whose
SingleProof has the bench's config-4 size (81,400 words, 651 KB; random words, nothing is verified), through
nhip_blk_digests, against two yardsticks in the same run on the same proof encodings:

  * the existing nhip_tip5_hash_varlen, one lane per proof encoding (what the row-form kernel exists to beat);
  * the C oracle's hash_varlen on 16 host threads (what a caller does today).

Prints one JSON line per block count, times in milliseconds as [best, median] of --repeats runs:
  * digests_call      : the whole nhip_blk_digests call (host decode, body MAST hashes, staging, kernels, read-back);
  * digests_kernels   : its launches alone (HIP events of nhip_timing_* around every launch of the call);
  * varlen_call / varlen_kernels : the same for nhip_tip5_hash_varlen on the proof encodings;
  * oracle_16_threads : the C oracle on 16 host threads;
  * library           : the first 16 hex digits of libneptune_hip.so's SHA-256.
The proof leaf nhip_blk_digests used (PowMastPaths.kernel[0]) is checked against both yardsticks' digests.

    python tools/blk_chain_rate.py [--blocks 64 256] [--words 81400] [--repeats 7]
"""
import argparse
import ctypes
import hashlib
import json
import os
import random
import statistics
import struct
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("neptune-core_amd", "oracle"):
    p = os.path.join(ROOT, sub)
    if p not in sys.path:
        sys.path.insert(0, p)

P = (1 << 64) - (1 << 32) + 1
HEIGHT = 29  # production pow tree height
THREADS = 16


def best_median(xs):
    return [round(min(xs), 3), round(statistics.median(xs), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--words", type=int, default=81400)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()

    import bincode_ref as B   # oracle/: synthetic blocks
    import coracle as CO      # oracle/: the C Tip5

    import neptune_hip as nh
    from neptune_hip import _lib as L
    from neptune_hip._lib import check

    lib_hash = hashlib.sha256(open(L.LIB_PATH, "rb").read()).hexdigest()[:16]
    g = random.Random(8)
    rng = np.random.default_rng(8)
    n_max, W = max(args.blocks), args.words
    # a block with an empty SingleProof ends in the item count: rewrite it and append the items
    heads = [B.encode_block(B.random_block(g, [], B.SINGLE_PROOF, [], tree_height=HEIGHT))[:-8] + struct.pack("<Q", W)
             for _ in range(n_max)]
    words = rng.integers(0, P, size=(n_max, W), dtype=np.uint64)

    with nh.Context(0) as ctx:
        for n in args.blocks:
            data = np.frombuffer(b"".join(heads[i] + words[i].tobytes() for i in range(n)), dtype=np.uint8)
            count = ctypes.c_size_t(0)
            scanned = (L.BlkBlock * n)()
            check(ctx.lib.nhip_blk_scan(data.ctypes.data, data.size, HEIGHT, ctypes.cast(scanned, ctypes.c_void_p), n,
                                        ctypes.byref(count)), "nhip_blk_scan")
            assert count.value == n
            dig = np.zeros((n, 5), dtype=np.uint64)
            mast = (L.PowMastPaths * n)()

            def digests():
                check(ctx.lib.nhip_blk_digests(ctx.handle, data.ctypes.data, data.size, HEIGHT,
                                               ctypes.cast(scanned, ctypes.c_void_p), n, dig.ctypes.data,
                                               ctypes.cast(mast, ctypes.c_void_p)), "nhip_blk_digests")

            enc = np.empty((n, W + 4), dtype=np.uint64)
            enc[:, :4] = [B.SINGLE_PROOF, W + 2, W + 1, W]
            enc[:, 4:] = words[:n]
            flat = enc.reshape(-1)
            off = np.arange(n + 1, dtype=np.uint64) * np.uint64(W + 4)
            vout = np.zeros(5 * n, dtype=np.uint64)

            def varlen():
                check(ctx.lib.nhip_tip5_hash_varlen(ctx.handle, flat, off, n, vout), "nhip_tip5_hash_varlen")

            def timed(f):
                f()  # warm-up: workspace and staging growth, code load
                ctx.timing(True)
                wall, kern = [], []
                for _ in range(args.repeats):
                    ctx.timing_read(reset=True)
                    t0 = time.perf_counter()
                    f()
                    wall.append((time.perf_counter() - t0) * 1e3)
                    kern.append(ctx.timing_read(reset=True)[0])
                ctx.timing(False)
                return best_median(wall), best_median(kern)

            d_call, d_kern = timed(digests)
            v_call, v_kern = timed(varlen)
            leaf = np.array([[int(x) for x in m.kernel[0]] for m in mast], dtype=np.uint64)
            assert (leaf == vout.reshape(n, 5)).all(), "proof leaf != nhip_tip5_hash_varlen"

            parts = [(i * n // THREADS, (i + 1) * n // THREADS) for i in range(THREADS)]
            parts = [(a, b) for a, b in parts if b > a]

            def oracle():
                with ThreadPoolExecutor(THREADS) as ex:
                    outs = list(ex.map(lambda ab: CO.hash_varlen_batch(enc[ab[0]:ab[1]].reshape(-1),
                                                                      off[:ab[1] - ab[0] + 1]), parts))
                return np.concatenate(outs)

            ref = oracle()
            assert (ref == leaf).all(), "proof leaf != the C oracle"
            o_wall = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                oracle()
                o_wall.append((time.perf_counter() - t0) * 1e3)
            print(json.dumps({"blocks": n, "proof_words": W, "repeats": args.repeats, "digests_call": d_call,
                              "digests_kernels": d_kern, "varlen_call": v_call, "varlen_kernels": v_kern,
                              "oracle_16_threads": best_median(o_wall), "library": lib_hash,
                              "unit": "ms [best, median]"}), flush=True)


if __name__ == "__main__":
    main()
