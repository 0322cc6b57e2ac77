#!/usr/bin/env python3
"""Rate of the mutator-set checks on one GPU: a synthetic block of R removal records x 45
chunk-dictionary entries, every entry with an MMR path of height 20 (swbf_inactive of 2^20 leaves, one
peak) and a chunk of 8 indices, through nhip_ms_can_remove_batch.

Prints one JSON line:
  * records_per_s          : end to end (packing excluded; staging, both kernels and the read-back included);
  * ms_perms_per_s         : achieved Tip5 permutations/s of the call's kernels (HIP events of nhip_timing_*
                             around k_ms_chunk_auth and k_ms_records): one permutation per pair hash (20 per
                             entry) plus the sponge's permutations per chunk (10 words: 2);
  * mtree_perms_per_s      : the existing nhip_mtree_verify_dev in the same run on an equal number of pair
                             hashes (R x 45 paths of depth 20);
  * ratio                  : ms_perms_per_s / mtree_perms_per_s, the yardstick.
The paths are random, so every entry fails authentication and every record reports BAD_MMR_PATH (checked);
the climb has no early exit, so the rate is that of valid records.  Best of --repeats.

    python tools/ms_rate.py [--records 4096] [--repeats 5]
"""
import argparse
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
ENTRIES, HEIGHT, CHUNK_LEN = 45, 20, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import ctypes

    import neptune_hip as nh
    from neptune_hip import mutator_set as MS
    from neptune_hip._lib import check

    rng = np.random.default_rng(6)
    R, E = args.records, args.records * ENTRIES
    batch = 1 << HEIGHT
    msa = MS.MutatorSetAccumulator(MS.MmrAccumulator(rng.integers(0, P, size=(2, 5), dtype=np.uint64), 8 * batch + 1),
                                   MS.MmrAccumulator(rng.integers(0, P, size=(1, 5), dtype=np.uint64), batch),
                                   rng.integers(0, 1 << 20, size=1000, dtype=np.uint32))
    # record r: 45 distinct inactive chunks inside one window, one index in each
    base = rng.integers(0, batch - 256, size=R, dtype=np.uint64)
    chunk = np.stack([np.sort(rng.permutation(256)[:ENTRIES]) for _ in range(R)]).astype(np.uint64) + base[:, None]
    index = chunk * np.uint64(4096) + rng.integers(0, 4096, size=(R, ENTRIES), dtype=np.uint64)
    mn = np.zeros((R, 2), dtype=np.uint64)
    mn[:, 0] = index.min(axis=1)
    dist = (index - mn[:, :1]).astype(np.uint32)
    packed = MS.PackedChunks(np.arange(R + 1, dtype=np.uint64) * np.uint64(ENTRIES), chunk.reshape(-1).copy(),
                             np.arange(E + 1, dtype=np.uint64) * np.uint64(HEIGHT),
                             rng.integers(0, P, size=(E * HEIGHT, 5), dtype=np.uint64),
                             np.arange(E + 1, dtype=np.uint64) * np.uint64(CHUNK_LEN),
                             rng.integers(0, 4096, size=E * CHUNK_LEN, dtype=np.uint32))
    pair_hashes = E * HEIGHT
    ms_perms = pair_hashes + E * ((CHUNK_LEN + 2) // 10 + 1)

    with nh.Context(0) as ctx:
        cm, _keep = msa._c()
        cc = packed._c()
        valid, can, status = (np.zeros(R, dtype=np.uint8) for _ in range(3))

        def ms_call():
            check(ctx.lib.nhip_ms_can_remove_batch(ctx.handle, ctypes.byref(cm), mn.ctypes.data, dist.ctypes.data,
                                                   ctypes.byref(cc), R, valid.ctypes.data, can.ctypes.data,
                                                   status.ctypes.data), "nhip_ms_can_remove_batch")

        ms_call()  # warm-up: workspace allocation, code load
        assert (status == MS.BAD_MMR_PATH).all() and not valid.any() and not can.any()
        ctx.timing(True)
        ms_wall, ms_kernel = [], []
        for _ in range(args.repeats):
            ctx.timing_read(reset=True)
            t0 = time.perf_counter()
            ms_call()
            ms_wall.append(time.perf_counter() - t0)
            ms_kernel.append(ctx.timing_read(reset=True)[0] * 1e-3)

        # the existing kernel on as many pair hashes: E paths of depth HEIGHT against one root
        d_root = ctx.upload(rng.integers(0, P, size=5, dtype=np.uint64))
        d_idx = ctx.upload(rng.integers(0, 1 << HEIGHT, size=E, dtype=np.uint64))
        d_leaf = ctx.upload(rng.integers(0, P, size=(E, 5), dtype=np.uint64))
        d_path = ctx.upload(packed.path)
        d_v = ctx.alloc(E)
        ctx.mtree_verify_dev(d_root, 1, d_idx, d_leaf, d_path, HEIGHT, E, d_v)
        ctx.synchronize()
        mt_kernel = []
        for _ in range(args.repeats):
            ctx.timing_read(reset=True)
            ctx.mtree_verify_dev(d_root, 1, d_idx, d_leaf, d_path, HEIGHT, E, d_v)
            mt_kernel.append(ctx.timing_read(reset=True)[0] * 1e-3)
        ctx.timing(False)

    ms_rate, mt_rate = ms_perms / min(ms_kernel), pair_hashes / min(mt_kernel)
    print(json.dumps({"records": R, "entries": E, "path_height": HEIGHT, "pair_hashes": pair_hashes,
                      "ms_perms": ms_perms, "records_per_s": R / min(ms_wall), "ms_kernel_ms": min(ms_kernel) * 1e3,
                      "ms_wall_ms": min(ms_wall) * 1e3, "ms_perms_per_s": ms_rate,
                      "mtree_kernel_ms": min(mt_kernel) * 1e3, "mtree_perms_per_s": mt_rate,
                      "ratio": ms_rate / mt_rate}))


if __name__ == "__main__":
    main()
