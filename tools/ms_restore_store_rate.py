#!/usr/bin/env python3
"""Restored witnesses into a store, through the host and device to device ("The hand-over"), on one GPU,
at tools/ms_archive_rate.py's shape: a synthetic archive of N AOCL leaves (random digests), batch_index(N) chunks of
--chunk-len random sorted words and a window of 2,000 words; --witnesses membership proofs whose 45 indices lie around
the leaf's batch.

Per leaf count the two ways alternate in one process, warm-up first, then best and median of --repeats, each into a
fresh store, with wall time around the calls and HIP events around their launches (nhip_timing_*):
  * host   : nhip_ms_archive_restore (count pass and fill) into numpy arrays, then nhip_ms_store_append from them;
  * device : nhip_ms_store_append_restored.
For the device way the bytes that cross each way are counted from its contract: up, the index sets and the leaf
indices; down, the statuses, the totals, the offsets and the keys.  Both stores are read back once and compared.
One JSON line per leaf count.

    python tools/ms_restore_store_rate.py [--leafs 65536,1048576] [--witnesses 16384] [--chunk-len 24] [--repeats 5]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("neptune-core_amd",):
    p = os.path.join(ROOT, sub)
    if p not in sys.path:
        sys.path.insert(0, p)

P = (1 << 64) - (1 << 32) + 1
WINDOW = 2000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leafs", default="65536,1048576")
    ap.add_argument("--witnesses", type=int, default=16384)
    ap.add_argument("--chunk-len", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    import neptune_hip as nh
    from neptune_hip import _lib as L
    from neptune_hip import mutator_set as MS

    rng = np.random.default_rng(11)
    z = lambda dtype, *shape: np.zeros(shape, dtype=dtype)  # noqa: E731
    with nh.Context(0) as ctx:
        lib = ctx.lib
        ctx.timing(True)
        for N in (int(x) for x in args.leafs.split(",")):
            B = max(N - 1, 0) // 8
            W = args.witnesses
            leaves = rng.integers(0, P, size=(N, 5), dtype=np.uint64)
            rel = np.sort(rng.integers(0, 4096, size=(B, args.chunk_len), dtype=np.uint32), axis=1).reshape(-1)
            rel_off = np.arange(B + 1, dtype=np.uint64) * np.uint64(args.chunk_len)
            window = np.sort(rng.integers(0, 1 << 20, size=WINDOW, dtype=np.uint32))
            leaf = rng.integers(0, N, size=W, dtype=np.uint64)
            base = (leaf // np.uint64(8)) * np.uint64(4096)
            index = base[:, None] + rng.integers(0, 1 << 20, size=(W, 45), dtype=np.uint64)
            mn = z(np.uint64, W, 2)
            mn[:, 0] = index.min(axis=1)
            dist = (index - mn[:, :1]).astype(np.uint32)
            commitments = np.ascontiguousarray(leaves[leaf.astype(np.int64)])
            wit_off = np.asarray([0, W], dtype=np.uint64)

            stats = {}

            def timed(name, call):
                ctx.timing_read(reset=True)
                t0 = time.perf_counter()
                call()
                wall = time.perf_counter() - t0
                stats.setdefault(name + "_wall_ms", []).append(wall * 1e3)
                stats.setdefault(name + "_kernel_ms", []).append(ctx.timing_read(reset=True)[0])

            totals = [None]

            def through_the_host(store):
                count = L.MsUpdated()
                L.check(lib.nhip_ms_archive_restore(archive._h, mn.ctypes.data, dist.ctypes.data, leaf.ctypes.data, W,
                                                    ctypes.byref(count)), "nhip_ms_archive_restore")
                A, E, PD, RW = (int(getattr(count, f)) for f in ("aocl_digests", "entries", "path_digests", "rel_words"))
                totals[0] = (A, E, PD, RW)
                o = dict(status=z(np.uint8, max(W, 1)), aocl_path_off=z(np.uint64, W + 1), aocl_path=z(np.uint64, max(A, 1), 5),
                         entry_off=z(np.uint64, W + 1), chunk_index=z(np.uint64, max(E, 1)), path_off=z(np.uint64, E + 1),
                         path=z(np.uint64, max(PD, 1), 5), rel_off=z(np.uint64, E + 1), rel=z(np.uint32, max(RW, 1)))
                cout = L.MsUpdated(*(o[f].ctypes.data for f, _ in L.MsUpdated._fields_[:9]), A, E, PD, RW)
                L.check(lib.nhip_ms_archive_restore(archive._h, mn.ctypes.data, dist.ctypes.data, leaf.ctypes.data, W,
                                                    ctypes.byref(cout)), "nhip_ms_archive_restore")
                assert not o["status"].any()
                chunks = L.MsChunks(o["entry_off"].ctypes.data, o["chunk_index"].ctypes.data, o["path_off"].ctypes.data,
                                    o["path"].ctypes.data, o["rel_off"].ctypes.data, o["rel"].ctypes.data)
                win = L.MsUpdateIn(wit_off.ctypes.data, mn.ctypes.data, dist.ctypes.data, leaf.ctypes.data,
                                   commitments.ctypes.data, o["aocl_path_off"].ctypes.data, o["aocl_path"].ctypes.data,
                                   ctypes.pointer(chunks))
                L.check(lib.nhip_ms_store_append(store._h, ctypes.byref(win), W), "nhip_ms_store_append")

            status = z(np.uint8, W)

            def device_to_device(store):
                L.check(lib.nhip_ms_store_append_restored(store._h, archive._h, mn.ctypes.data, dist.ctypes.data,
                                                          leaf.ctypes.data, None, W, status.ctypes.data),
                        "nhip_ms_store_append_restored")
                assert not status.any()

            archive = MS.Archive(ctx)
            L.check(archive.load_raw(leaves, rel_off, rel, window), "nhip_ms_archive_load")
            kept = {}
            for rep in range(args.repeats + 1):  # the first is the warm-up
                for name, way in (("host", through_the_host), ("device", device_to_device)):
                    store = MS.WitnessStore(ctx)
                    timed(name, lambda: way(store))
                    if rep == args.repeats:
                        kept[name] = store
                    else:
                        store.close()
                if rep == 0:
                    stats.clear()
            # the two stores hold the same: counts, and every array of a read of a sample
            assert kept["host"].counts() == kept["device"].counts() == (W,) + totals[0]
            sample = [0, 1, W // 2, W - 1]
            ra, rb = kept["host"].read_raw(sample)[2], kept["device"].read_raw(sample)[2]
            assert all((ra[f] == rb[f]).all() for f in ra), "the two ways disagree"
            acc = archive.accumulator()
            for s in kept.values():
                s.close()
            archive.close()

            A, E, PD, RW = totals[0]
            best = {k: min(v) for k, v in stats.items()}
            med = {k: statistics.median(v) for k, v in stats.items()}
            out = dict(leafs=N, chunks=B, witnesses=W, chunk_len=args.chunk_len, aocl_peaks=len(acc.aocl.peaks),
                       restore_totals=dict(aocl_digests=A, entries=E, path_digests=PD, rel_words=RW),
                       best_ms={k: round(v, 4) for k, v in best.items()}, median_ms={k: round(v, 4) for k, v in med.items()},
                       host_bytes_each_way=40 * (A + PD) + 4 * RW,
                       device_bytes_up=W * (16 + 180 + 8), device_bytes_down=W + 32 + 16 * (W + 1) + 8 * E + 16 * (E + 1),
                       device_median_below_host_best=med["device_wall_ms"] < best["host_wall_ms"],
                       speedup_median=round(med["host_wall_ms"] / med["device_wall_ms"], 2))
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
