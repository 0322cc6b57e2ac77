#!/usr/bin/env python3
"""Rate of the batched mutator-set update on one GPU: a synthetic batch of J independent block
updates through nhip_ms_apply_batch.  Every job starts from the same accumulator (swbf_inactive of 2^10 chunks
of 8 indices under one peak, built with the library's own nhip_mtree_build; a window of 2,000 indices) and
carries K addition records and M removal records of its own, each record with 24 indices in inactive chunks
(dictionary entries with authentic paths of height 10) and 21 in the window.  Every job is accepted (checked).

Prints one JSON line per shape (the whole update, additions only, removals only):
  * jobs_per_s             : end to end (packing excluded; staging, the three kernels and the read-back included);
  * apply_perms_per_s      : achieved Tip5 permutations/s of the call's kernels (HIP events of nhip_timing_*
                             around k_ms_chunk_auth_jobs, k_ms_records_jobs and k_ms_apply): one per pair hash
                             (entry climbs, both MMR appends, one climb per touched chunk) plus the sponge's per
                             chunk hashed (entries, touched chunks, new chunks);
  * mtree_perms_per_s      : the existing nhip_mtree_verify_dev in the same run on an equal number of pair
                             hashes (paths of depth 20);
  * ratio                  : apply_perms_per_s / mtree_perms_per_s, the yardstick.
Best of --repeats.

    python tools/ms_apply_rate.py [--jobs 1024] [--additions 64] [--records 8] [--repeats 5]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("neptune-core_amd",):
    p = os.path.join(ROOT, sub)
    if p not in sys.path:
        sys.path.insert(0, p)

P = (1 << 64) - (1 << 32) + 1
HEIGHT, CHUNK_LEN, INACTIVE, WINDOW = 10, 8, 24, 2000
B0 = 1 << HEIGHT
N0 = 8 * B0 + 1  # batch index B0; two AOCL peaks


def sponge(n):
    """Permutations of Tip5::hash of a chunk of n indices: n + 2 words, padded."""
    return (n + 2) // 10 + 1


def popcount(x):
    return bin(x).count("1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=1024)
    ap.add_argument("--additions", type=int, default=64)
    ap.add_argument("--records", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    import neptune_hip as nh
    from neptune_hip import _lib as L
    from neptune_hip import mutator_set as MS

    rng = np.random.default_rng(7)
    with nh.Context(0) as ctx:
        # the inactive part: chunk contents, their hashes, the Merkle tree over them (one peak)
        rel_all = np.sort(rng.integers(0, 4096, size=(B0, CHUNK_LEN), dtype=np.uint32), axis=1)
        words = np.concatenate([np.full((B0, 1), CHUNK_LEN + 1, dtype=np.uint64), np.full((B0, 1), CHUNK_LEN, dtype=np.uint64),
                                rel_all.astype(np.uint64)], axis=1)
        leaves = ctx.hash_varlen(data=words.reshape(-1), offsets=np.arange(B0 + 1, dtype=np.uint64) * np.uint64(CHUNK_LEN + 2))
        nodes = ctx.mtree_build(leaves)
        heap = np.concatenate([nodes, leaves])  # heap order: node i, leaf ci at B0 + ci
        path_all = np.stack([heap[((B0 + np.arange(B0)) >> lvl) ^ 1] for lvl in range(HEIGHT)], axis=1)  # (B0, HEIGHT, 5)
        window = np.sort(rng.integers(0, 1 << 20, size=WINDOW, dtype=np.uint32))
        before = MS.MutatorSetAccumulator(MS.MmrAccumulator(rng.integers(0, P, size=(2, 5), dtype=np.uint64), N0),
                                          MS.MmrAccumulator(nodes[1:2], B0), window)

        def shape(J, K, M):
            """The arrays of J jobs with K additions and M records each, and the permutations their kernels run."""
            R, E = J * M, J * M * INACTIVE
            ci_in, ci_act = np.zeros((0, INACTIVE), dtype=np.uint64), np.zeros((0, 45 - INACTIVE), dtype=np.uint64)
            if R:
                ci_in = np.stack([rng.permutation(B0)[:INACTIVE] for _ in range(R)]).astype(np.uint64)
                ci_act = np.stack([rng.permutation(256)[:45 - INACTIVE] for _ in range(R)]).astype(np.uint64) + np.uint64(B0)
            chunk = np.concatenate([ci_in, ci_act], axis=1)
            index = chunk * np.uint64(4096) + rng.integers(0, 4096, size=chunk.shape, dtype=np.uint64)
            mn = np.zeros((R, 2), dtype=np.uint64)
            if R:
                mn[:, 0] = index.min(axis=1)
            dist = (index - mn[:, :1]).astype(np.uint32)
            flat = ci_in.reshape(-1).astype(np.int64)
            packed = MS.PackedChunks(np.arange(R + 1, dtype=np.uint64) * np.uint64(INACTIVE), ci_in.reshape(-1).copy(),
                                     np.arange(E + 1, dtype=np.uint64) * np.uint64(HEIGHT),
                                     np.ascontiguousarray(path_all[flat]).reshape(-1, 5),
                                     np.arange(E + 1, dtype=np.uint64) * np.uint64(CHUNK_LEN),
                                     np.ascontiguousarray(rel_all[flat]).reshape(-1))
            n1 = N0 + K
            b1 = (n1 - 1) // 8
            pair = E * HEIGHT + J * (K + popcount(N0) - popcount(n1)) + J * ((b1 - B0) + popcount(B0) - popcount(b1))
            perms = pair + E * sponge(CHUNK_LEN)
            for j in range(J):
                cj = chunk[j * M:(j + 1) * M].reshape(-1)
                ci, cnt = np.unique(cj, return_counts=True)
                touched = ci < B0
                pair_j = int(touched.sum()) * HEIGHT
                pair += pair_j
                perms += pair_j + sum(sponge(CHUNK_LEN + int(c)) for c in cnt[touched])
                for c in range(b1 - B0):
                    old = int(np.searchsorted(window, (c + 1) * 4096) - np.searchsorted(window, c * 4096)) if c < 256 else 0
                    perms += sponge(old + int(cnt[ci == B0 + c].sum()))
            return dict(J=J, K=K, M=M, mn=mn, dist=dist, packed=packed, pair=pair, perms=perms,
                        additions=rng.integers(0, P, size=(J * K, 5), dtype=np.uint64))

        def measure(s):
            J, K, M = s["J"], s["K"], s["M"]
            msas = (L.Msa * J)()
            cm, _keep = before._c()
            for j in range(J):
                msas[j] = cm
            cc = s["packed"]._c()
            add_off = np.arange(J + 1, dtype=np.uint64) * np.uint64(K)
            rec_off = np.arange(J + 1, dtype=np.uint64) * np.uint64(M)
            ptr = lambda a: a.ctypes.data if a.size else None  # noqa: E731
            cin = L.MsApplyIn(J, msas, add_off.ctypes.data, ptr(s["additions"]), rec_off.ctypes.data, ptr(s["mn"]),
                              ptr(s["dist"]), ctypes.pointer(cc), None)
            verdict, status = np.zeros(J, dtype=np.uint8), np.zeros(J, dtype=np.uint8)
            bad = np.zeros(J, dtype=np.uint64)
            cout = L.MsApplyOut(verdict.ctypes.data, status.ctypes.data, bad.ctypes.data)

            def call():
                L.check(ctx.lib.nhip_ms_apply_batch(ctx.handle, ctypes.byref(cin), ctypes.byref(cout)), "nhip_ms_apply_batch")

            call()  # warm-up: workspace allocation, code load
            assert (status == MS.OK).all() and verdict.all(), status[:16]
            ctx.timing(True)
            wall, kernel = [], []
            for _ in range(args.repeats):
                ctx.timing_read(reset=True)
                t0 = time.perf_counter()
                call()
                wall.append(time.perf_counter() - t0)
                kernel.append(ctx.timing_read(reset=True)[0] * 1e-3)
            # the existing kernel on as many pair hashes: paths of depth 20 against one root
            depth = 20
            n = max(s["perms"] // depth, 1)
            d_root = ctx.upload(rng.integers(0, P, size=5, dtype=np.uint64))
            d_idx = ctx.upload(rng.integers(0, 1 << depth, size=n, dtype=np.uint64))
            d_leaf = ctx.upload(rng.integers(0, P, size=(n, 5), dtype=np.uint64))
            d_path = ctx.upload(rng.integers(0, P, size=(n * depth, 5), dtype=np.uint64))
            d_v = ctx.alloc(n)
            ctx.mtree_verify_dev(d_root, 1, d_idx, d_leaf, d_path, depth, n, d_v)
            ctx.synchronize()
            mt = []
            for _ in range(args.repeats):
                ctx.timing_read(reset=True)
                ctx.mtree_verify_dev(d_root, 1, d_idx, d_leaf, d_path, depth, n, d_v)
                mt.append(ctx.timing_read(reset=True)[0] * 1e-3)
            ctx.timing(False)
            rate, mt_rate = s["perms"] / min(kernel), n * depth / min(mt)
            return {"jobs": J, "additions": K, "records": M, "pair_hashes": s["pair"], "apply_perms": s["perms"],
                    "jobs_per_s": J / min(wall), "apply_kernel_ms": min(kernel) * 1e3, "apply_wall_ms": min(wall) * 1e3,
                    "apply_perms_per_s": rate, "mtree_kernel_ms": min(mt) * 1e3, "mtree_perms_per_s": mt_rate,
                    "ratio": rate / mt_rate}

        for label, K, M in (("update", args.additions, args.records), ("additions only", args.additions, 0),
                            ("removals only", 0, args.records)):
            print(json.dumps(dict(shape=label, **measure(shape(args.jobs, K, M)))), flush=True)


if __name__ == "__main__":
    main()
