#!/usr/bin/env python3
"""Rate of bringing witnesses across a block on one GPU: one job through nhip_ms_update_batch on
tools/ms_apply_rate.py's synthetic accumulator (swbf_inactive of 2^10 chunks of 8 indices under one peak, a window of
2,000 indices), here with a real AOCL of 2^13 + 1 leaves so that membership proofs authenticate.  The block carries K
addition records and M removal records (24 indices in inactive chunks, 21 in the window, as there); every witness is a
membership proof with 24 inactive entries (authentic paths of height 10, chunks of 8 indices), 21 indices in the
window and an AOCL path of 13 digests.  Every witness is accepted (checked).

The call's kernels are timed with HIP events (nhip_timing_*) in three calls on the same block, warm-up then best of
--repeats, and told apart by difference:
  * block_kernel_ms   : nhip_ms_apply_batch (k_ms_chunk_auth_jobs, k_ms_records_jobs, k_ms_apply);
  * nodes_kernel_ms   : nhip_ms_update_batch without witnesses (the same with k_ms_apply<true>, which keeps its nodes)
                        and nodes_ratio = nodes_kernel_ms / block_kernel_ms;
  * witness_kernel_ms : the whole call minus that: admission (k_ms_chunk_auth_jobs over the witnesses' entries,
                        k_ms_wit_admit: Tip5) and the copy kernels (k_ms_wit_paths, k_ms_wit_chunks, k_ms_wit_seal).
Per-kernel times inside the witness side come from a kernel trace of this tool, not from here.
  * stage_readback_ms : wall time of the whole call minus its kernels: the host plan, staging, read-back;
  * witnesses_per_s   : end to end (packing excluded);
  * gather_bytes      : what k_ms_wit_paths must move, from the shapes: 40 bytes read and 40 written per output digest
                        (AOCL paths and dictionary paths); chunk_bytes likewise for k_ms_wit_chunks (4 + 4 per word).
One JSON line per witness count.

    python tools/ms_update_rate.py [--witnesses 1024,16384,65536] [--additions 64] [--records 8] [--repeats 5]
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
HEIGHT, CHUNK_LEN, INACTIVE, WINDOW, AOCL_HEIGHT = 10, 8, 24, 2000, 13
B0 = 1 << HEIGHT
N0 = 8 * B0 + 1  # batch index B0; two AOCL peaks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--witnesses", default="1024,16384,65536")
    ap.add_argument("--additions", type=int, default=64)
    ap.add_argument("--records", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    import neptune_hip as nh
    from neptune_hip import _lib as L
    from neptune_hip import mutator_set as MS

    rng = np.random.default_rng(7)
    ptr = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    with nh.Context(0) as ctx:
        rel_all = np.sort(rng.integers(0, 4096, size=(B0, CHUNK_LEN), dtype=np.uint32), axis=1)
        words = np.concatenate([np.full((B0, 1), CHUNK_LEN + 1, dtype=np.uint64), np.full((B0, 1), CHUNK_LEN, dtype=np.uint64),
                                rel_all.astype(np.uint64)], axis=1)
        leaves = ctx.hash_varlen(data=words.reshape(-1), offsets=np.arange(B0 + 1, dtype=np.uint64) * np.uint64(CHUNK_LEN + 2))
        nodes = ctx.mtree_build(leaves)
        heap = np.concatenate([nodes, leaves])  # heap order: node i, leaf ci at B0 + ci
        path_all = np.stack([heap[((B0 + np.arange(B0)) >> lvl) ^ 1] for lvl in range(HEIGHT)], axis=1)  # (B0, HEIGHT, 5)
        window = np.sort(rng.integers(0, 1 << 20, size=WINDOW, dtype=np.uint32))
        # the AOCL: 2^13 random leaves under one peak, and one more leaf
        A0 = 1 << AOCL_HEIGHT
        aocl_leaves = rng.integers(0, P, size=(A0 + 1, 5), dtype=np.uint64)
        anodes = ctx.mtree_build(aocl_leaves[:A0])
        aheap = np.concatenate([anodes, aocl_leaves[:A0]])
        before = MS.MutatorSetAccumulator(MS.MmrAccumulator(np.stack([anodes[1], aocl_leaves[A0]]), N0),
                                          MS.MmrAccumulator(nodes[1:2], B0), window)

        def index_sets(n):
            """n index sets: 24 indices in distinct inactive chunks, 21 in the window; their inactive chunks, ascending"""
            if n == 0:
                return np.zeros((0, 2), dtype=np.uint64), np.zeros((0, 45), dtype=np.uint32), np.zeros((0, INACTIVE), dtype=np.uint64)
            ci_in = np.sort(np.stack([rng.permutation(B0)[:INACTIVE] for _ in range(n)]).astype(np.uint64), axis=1)
            ci_act = np.stack([rng.permutation(256)[:45 - INACTIVE] for _ in range(n)]).astype(np.uint64) + np.uint64(B0)
            chunk = np.concatenate([ci_in, ci_act], axis=1)
            index = chunk * np.uint64(4096) + rng.integers(0, 4096, size=chunk.shape, dtype=np.uint64)
            mn = np.zeros((n, 2), dtype=np.uint64)
            mn[:, 0] = index.min(axis=1)
            return mn, (index - mn[:, :1]).astype(np.uint32), ci_in

        def dictionaries(ci_in):
            n = ci_in.shape[0]
            E = n * INACTIVE
            flat = ci_in.reshape(-1).astype(np.int64)
            return MS.PackedChunks(np.arange(n + 1, dtype=np.uint64) * np.uint64(INACTIVE), ci_in.reshape(-1).copy(),
                                   np.arange(E + 1, dtype=np.uint64) * np.uint64(HEIGHT),
                                   np.ascontiguousarray(path_all[flat]).reshape(-1, 5),
                                   np.arange(E + 1, dtype=np.uint64) * np.uint64(CHUNK_LEN),
                                   np.ascontiguousarray(rel_all[flat]).reshape(-1))

        K, M = args.additions, args.records
        rmn, rdist, rci = index_sets(M)
        rpacked = dictionaries(rci)
        rcc = rpacked._c()
        additions = rng.integers(0, P, size=(K, 5), dtype=np.uint64)
        cm, _keep = before._c()
        msas = (L.Msa * 1)(cm)
        add_off, rec_off = np.array([0, K], dtype=np.uint64), np.array([0, M], dtype=np.uint64)
        cin = L.MsApplyIn(1, msas, add_off.ctypes.data, ptr(additions), rec_off.ctypes.data, ptr(rmn), ptr(rdist),
                          ctypes.pointer(rcc), None)
        verdict, status, bad = np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint64)
        cout = L.MsApplyOut(verdict.ctypes.data, status.ctypes.data, bad.ctypes.data)

        def timed(call):
            call()  # warm-up: workspace allocation, code load
            ctx.timing(True)
            wall, kernel = [], []
            for _ in range(args.repeats):
                ctx.timing_read(reset=True)
                t0 = time.perf_counter()
                call()
                wall.append(time.perf_counter() - t0)
                kernel.append(ctx.timing_read(reset=True)[0] * 1e-3)
            ctx.timing(False)
            return min(wall), min(kernel)

        def update_call(W):
            mn, dist, ci_in = index_sets(W)
            packed = dictionaries(ci_in)
            cc = packed._c()
            l = rng.integers(0, A0, size=W, dtype=np.uint64)
            leaf = np.ascontiguousarray(aocl_leaves[l.astype(np.int64)])
            apath = np.ascontiguousarray(np.stack([aheap[((A0 + l.astype(np.int64)) >> lvl) ^ 1] for lvl in range(AOCL_HEIGHT)],
                                                  axis=1)).reshape(-1, 5) if W else np.zeros((0, 5), dtype=np.uint64)
            apath_off = np.arange(W + 1, dtype=np.uint64) * np.uint64(AOCL_HEIGHT)
            wit_off = np.array([0, W], dtype=np.uint64)
            win = L.MsUpdateIn(wit_off.ctypes.data, ptr(mn), ptr(dist), ptr(l), ptr(leaf), apath_off.ctypes.data, ptr(apath),
                               ctypes.pointer(cc))
            count = L.MsUpdated()
            L.check(ctx.lib.nhip_ms_update_plan(ctypes.byref(cin), ctypes.byref(win), ctypes.byref(count)), "nhip_ms_update_plan")
            A, E, PD, RW = int(count.aocl_digests), int(count.entries), int(count.path_digests), int(count.rel_words)
            o = dict(status=np.zeros(max(W, 1), dtype=np.uint8), aocl_path_off=np.zeros(W + 1, dtype=np.uint64),
                     aocl_path=np.zeros((max(A, 1), 5), dtype=np.uint64), entry_off=np.zeros(W + 1, dtype=np.uint64),
                     chunk_index=np.zeros(max(E, 1), dtype=np.uint64), path_off=np.zeros(E + 1, dtype=np.uint64),
                     path=np.zeros((max(PD, 1), 5), dtype=np.uint64), rel_off=np.zeros(E + 1, dtype=np.uint64),
                     rel=np.zeros(max(RW, 1), dtype=np.uint32))
            fill = L.MsUpdated(*(o[f].ctypes.data for f, _ in L.MsUpdated._fields_[:9]), A, E, PD, RW)
            keep = (mn, dist, ci_in, packed, cc, l, leaf, apath, apath_off, wit_off, win, o)

            def call():
                L.check(ctx.lib.nhip_ms_update_batch(ctx.handle, ctypes.byref(cin), ctypes.byref(cout), ctypes.byref(win),
                                                     ctypes.byref(fill)), "nhip_ms_update_batch")
            return call, o, (A, E, PD, RW), keep

        def apply_call():
            L.check(ctx.lib.nhip_ms_apply_batch(ctx.handle, ctypes.byref(cin), ctypes.byref(cout)), "nhip_ms_apply_batch")

        _, block_kernel = timed(apply_call)
        assert status[0] == MS.OK and verdict[0] == 1, status
        call0, _, _, keep0 = update_call(0)
        _, nodes_kernel = timed(call0)
        for W in (int(x) for x in args.witnesses.split(",")):
            call, o, (A, E, PD, RW), keep = update_call(W)
            wall, kernel = timed(call)
            assert status[0] == MS.OK and (o["status"][:W] == MS.OK).all(), o["status"][:16]
            assert A == W * AOCL_HEIGHT and E >= W * INACTIVE
            gather_bytes, chunk_bytes = 80 * (A + PD), 8 * RW
            print(json.dumps({
                "witnesses": W, "additions": K, "records": M, "entries_after": E, "aocl_digests": A, "path_digests": PD,
                "rel_words": RW, "block_kernel_ms": block_kernel * 1e3, "nodes_kernel_ms": nodes_kernel * 1e3,
                "nodes_ratio": nodes_kernel / block_kernel, "witness_kernel_ms": (kernel - nodes_kernel) * 1e3,
                "call_kernel_ms": kernel * 1e3, "call_wall_ms": wall * 1e3, "stage_readback_ms": (wall - kernel) * 1e3,
                "witnesses_per_s": W / wall, "gather_bytes": gather_bytes, "chunk_bytes": chunk_bytes}), flush=True)
            del keep


if __name__ == "__main__":
    main()
