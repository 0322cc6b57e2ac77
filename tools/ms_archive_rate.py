#!/usr/bin/env python3
"""Rate of the device-resident archival mutator set on one GPU: a synthetic archive of N AOCL leaves
(random digests), batch_index(N) chunks of --chunk-len random sorted words and a window of 2,000 words.

Per leaf count, with wall time around the call and HIP events around its launches (nhip_timing_*), warm-up first, then
best and median of --repeats:
  * load     : a fresh archive each repeat: upload, one chunk sponge per chunk, every level of both MMRs
               (hashes = N - popcount(N) + B - popcount(B) hash pairs plus B sponges);
  * acc      : nhip_ms_archive_accumulator;
  * paths    : nhip_ms_archive_paths of --witnesses random AOCL leaves (fill call);
  * plan     : nhip_ms_archive_restore_plan alone (host only), the part of restore that is neither kernel nor copy;
  * restore  : nhip_ms_archive_restore of --witnesses membership proofs whose 45 indices lie around the leaf's batch
               (fill call).  gather_GBps is the bytes k_ms_arch_gather reads plus writes over its event time;
  * apply    : nhip_ms_archive_apply of a block of 64 addition records (eight window slides) on the fresh archive,
               whose arrays all have to grow for it (the wall time includes packing the block in Python);
  * revert   : nhip_ms_archive_revert of that block, back to the loaded set (packing included, as apply's);
  * reload   : the only other way back: destroy, create and load of the whole set before.  It needs every leaf, chunk
               word and the window of the earlier set on the host; the revert needs the block alone.
A sample of the restored AOCL paths is checked with nhip_mmr_verify_batch against the archive's own accumulator.
One JSON line per leaf count.

    python tools/ms_archive_rate.py [--leafs 65536,1048576] [--witnesses 16384] [--chunk-len 24] [--repeats 5]
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
            # witnesses: a leaf, and 45 indices within the 256 chunks that end at its batch's window
            leaf = rng.integers(0, N, size=W, dtype=np.uint64)
            base = (leaf // np.uint64(8)) * np.uint64(4096)
            index = base[:, None] + rng.integers(0, 1 << 20, size=(W, 45), dtype=np.uint64)
            mn = z(np.uint64, W, 2)
            mn[:, 0] = index.min(axis=1)
            dist = (index - mn[:, :1]).astype(np.uint32)
            lens = np.full(B, args.chunk_len, dtype=np.uint64)
            block = MS.MutatorSetUpdate([], rng.integers(0, P, size=(64, 5), dtype=np.uint64))

            stats = {}

            def timed(name, call):
                ctx.timing_read(reset=True)
                t0 = time.perf_counter()
                rc = call()
                wall = time.perf_counter() - t0
                L.check(rc, name)
                stats.setdefault(name + "_wall_ms", []).append(wall * 1e3)
                stats.setdefault(name + "_kernel_ms", []).append(ctx.timing_read(reset=True)[0])

            def arrays(A, E, PD, RW):
                o = dict(status=z(np.uint8, max(W, 1)), aocl_path_off=z(np.uint64, W + 1), aocl_path=z(np.uint64, max(A, 1), 5),
                         entry_off=z(np.uint64, W + 1), chunk_index=z(np.uint64, max(E, 1)), path_off=z(np.uint64, E + 1),
                         path=z(np.uint64, max(PD, 1), 5), rel_off=z(np.uint64, E + 1), rel=z(np.uint32, max(RW, 1)))
                return o, L.MsUpdated(*(o[f].ctypes.data for f, _ in L.MsUpdated._fields_[:9]), A, E, PD, RW)

            archive = None
            for rep in range(args.repeats + 1):  # the first is the warm-up
                if archive is not None:
                    archive.close()
                archive = MS.Archive(ctx)
                timed("load", lambda: archive.load_raw(leaves, rel_off, rel, window))
                acc = [None]

                def accumulate():
                    acc[0] = archive.accumulator()
                    return L.NHIP_OK
                timed("acc", accumulate)
                total = ctypes.c_size_t()
                L.check(lib.nhip_ms_archive_paths(archive._h, 0, leaf.ctypes.data, W, None, None, 0, ctypes.byref(total)),
                        "nhip_ms_archive_paths")
                poff, ppath = z(np.uint64, W + 1), z(np.uint64, max(total.value, 1), 5)
                timed("paths", lambda: lib.nhip_ms_archive_paths(archive._h, 0, leaf.ctypes.data, W, poff.ctypes.data,
                                                                 ppath.ctypes.data, total.value, ctypes.byref(total)))
                count = L.MsUpdated()
                timed("plan", lambda: lib.nhip_ms_archive_restore_plan(N, lens.ctypes.data, B, mn.ctypes.data, dist.ctypes.data,
                                                                       leaf.ctypes.data, W, ctypes.byref(count)))
                A, E, PD, RW = (int(getattr(count, f)) for f in ("aocl_digests", "entries", "path_digests", "rel_words"))
                o, cout = arrays(A, E, PD, RW)
                timed("restore", lambda: lib.nhip_ms_archive_restore(archive._h, mn.ctypes.data, dist.ctypes.data,
                                                                     leaf.ctypes.data, W, ctypes.byref(cout)))
                timed("apply", lambda: (archive.apply(acc[0], block), L.NHIP_OK)[1])
                back = [None]

                def revert():
                    back[0] = archive.revert(acc[0], block)
                    return L.NHIP_OK
                timed("revert", revert)
                assert back[0][:2] == (True, MS.OK) and archive.counts()[:3] == (N, B, WINDOW), back[0][:3]

                def reload():
                    nonlocal archive
                    archive.close()
                    archive = MS.Archive(ctx)
                    return archive.load_raw(leaves, rel_off, rel, window)
                timed("reload", reload)
                if rep == 0:
                    stats.clear()
            assert not o["status"].any() and (o["aocl_path_off"] == poff).all() and (o["aocl_path"][:A] == ppath[:A]).all()
            k = min(W, 256)
            items = [(int(leaf[i]), leaves[int(leaf[i])], o["aocl_path"][int(poff[i]):int(poff[i + 1])]) for i in range(k)]
            assert all(MS.mmr_verify_batch(ctx, acc[0].aocl, items)), "a restored AOCL path does not verify"
            archive.close()

            hashes = (N - bin(N).count("1")) + (B - bin(B).count("1"))
            gather_bytes = 2 * (40 * (A + PD) + 4 * RW)
            best = {k: min(v) for k, v in stats.items()}
            med = {k: statistics.median(v) for k, v in stats.items()}
            out = dict(leafs=N, chunks=B, witnesses=W, chunk_len=args.chunk_len, hash_pairs=hashes, sponges=B,
                       restore_totals=dict(aocl_digests=A, entries=E, path_digests=PD, rel_words=RW),
                       best_ms={k: round(v, 4) for k, v in best.items()}, median_ms={k: round(v, 4) for k, v in med.items()},
                       load_Mhash_per_s=round((hashes + B) / best["load_kernel_ms"] / 1e3, 2) if best["load_kernel_ms"] else None,
                       restored_per_s=round(W / best["restore_wall_ms"] * 1e3),
                       gather_GBps=round(gather_bytes / best["restore_kernel_ms"] / 1e6, 1) if best["restore_kernel_ms"] else None)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
