#!/usr/bin/env python3
"""Rate of taking the device-resident witnesses back across a block on one GPU, on the synthetic
accumulator and witness shape of tools/ms_store_rate.py: a real AOCL of 2^13 + 1 leaves, a block of K addition records
and M removal records, every witness a membership proof with 24 inactive entries (authentic paths of height 10, chunks
of 8 indices), 21 indices in the window and an AOCL path of 13 digests.  Every witness is accepted (checked).

Per witness count, every repeat refills one store, brings it across the block (nhip_ms_store_update, not timed) and
then measures, with wall time around the call and HIP events around its launches (nhip_timing_*):
  * revert   : nhip_ms_store_revert of that block, the store's tip passed as msa_expected;
  * reupload : the yardstick, the only way back without it: nhip_ms_store_retain of nothing plus nhip_ms_store_append
               of all witnesses as they were before the block, from pageable memory (both entry points unchanged; the
               host's re-derivation of those witnesses is not timed);
  * plan     : nhip_ms_revert_plan alone (host only), the part of the call that is neither kernel nor copy;
  * batch    : nhip_ms_revert_batch with the witnesses after the block passed from host memory.
Warm-up first, then best and median of --repeats.  After the warm-up's revert the store is read and compared byte for
byte with what was appended, and with the batch call's outputs.  One JSON line per witness count.

    python tools/ms_revert_rate.py [--witnesses 1024,8192,65536] [--additions 64] [--records 8] [--repeats 5]
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
HEIGHT, CHUNK_LEN, INACTIVE, WINDOW, AOCL_HEIGHT = 10, 8, 24, 2000, 13
B0 = 1 << HEIGHT
N0 = 8 * B0 + 1  # batch index B0; two AOCL peaks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--witnesses", default="1024,8192,65536")
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
        lib = ctx.lib
        rel_all = np.sort(rng.integers(0, 4096, size=(B0, CHUNK_LEN), dtype=np.uint32), axis=1)
        words = np.concatenate([np.full((B0, 1), CHUNK_LEN + 1, dtype=np.uint64), np.full((B0, 1), CHUNK_LEN, dtype=np.uint64),
                                rel_all.astype(np.uint64)], axis=1)
        leaves = ctx.hash_varlen(data=words.reshape(-1), offsets=np.arange(B0 + 1, dtype=np.uint64) * np.uint64(CHUNK_LEN + 2))
        nodes = ctx.mtree_build(leaves)
        heap = np.concatenate([nodes, leaves])  # heap order: node i, leaf ci at B0 + ci
        path_all = np.stack([heap[((B0 + np.arange(B0)) >> lvl) ^ 1] for lvl in range(HEIGHT)], axis=1)  # (B0, HEIGHT, 5)
        window = np.sort(rng.integers(0, 1 << 20, size=WINDOW, dtype=np.uint32))
        A0 = 1 << AOCL_HEIGHT
        aocl_leaves = rng.integers(0, P, size=(A0 + 1, 5), dtype=np.uint64)
        anodes = ctx.mtree_build(aocl_leaves[:A0])
        aheap = np.concatenate([anodes, aocl_leaves[:A0]])
        before = MS.MutatorSetAccumulator(MS.MmrAccumulator(np.stack([anodes[1], aocl_leaves[A0]]), N0),
                                          MS.MmrAccumulator(nodes[1:2], B0), window)

        def index_sets(n):
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
        z = lambda dtype, *shape: np.zeros(shape, dtype=dtype)  # noqa: E731
        blk = dict(verdict=z(np.uint8, 1), status=z(np.uint8, 1), bad_record=z(np.uint64, 1), aocl_peaks=z(np.uint64, 64, 5),
                   aocl_n_peaks=z(np.uint32, 1), aocl_num_leafs=z(np.uint64, 1), swbf_peaks=z(np.uint64, 64, 5),
                   swbf_n_peaks=z(np.uint32, 1), swbf_num_leafs=z(np.uint64, 1),
                   active_off=np.array([0, WINDOW + 45 * M], dtype=np.uint64), active=z(np.uint32, WINDOW + 45 * M),
                   n_active=z(np.uint64, 1))
        cout = L.MsApplyOut(*(blk[f].ctypes.data for f, _ in L.MsApplyOut._fields_))

        def measured(call, stats, name):
            ctx.timing_read(reset=True)
            t0 = time.perf_counter()
            call()
            wall = time.perf_counter() - t0
            stats.setdefault(name + "_wall_ms", []).append(wall * 1e3)
            stats.setdefault(name + "_kernel_ms", []).append(ctx.timing_read(reset=True)[0])

        def arrays(W, A, E, PD, RW):
            o = dict(status=z(np.uint8, max(W, 1)), aocl_path_off=z(np.uint64, W + 1), aocl_path=z(np.uint64, max(A, 1), 5),
                     entry_off=z(np.uint64, W + 1), chunk_index=z(np.uint64, max(E, 1)), path_off=z(np.uint64, E + 1),
                     path=z(np.uint64, max(PD, 1), 5), rel_off=z(np.uint64, E + 1), rel=z(np.uint32, max(RW, 1)))
            return o, L.MsUpdated(*(o[f].ctypes.data for f, _ in L.MsUpdated._fields_[:9]), A, E, PD, RW)

        for W in (int(x) for x in args.witnesses.split(",")):
            mn, dist, ci_in = index_sets(W)
            packed = dictionaries(ci_in)
            cc = packed._c()
            l = rng.integers(0, A0, size=W, dtype=np.uint64)
            leaf = np.ascontiguousarray(aocl_leaves[l.astype(np.int64)])
            apath = np.ascontiguousarray(np.stack([aheap[((A0 + l.astype(np.int64)) >> lvl) ^ 1] for lvl in range(AOCL_HEIGHT)],
                                                  axis=1)).reshape(-1, 5)
            apath_off = np.arange(W + 1, dtype=np.uint64) * np.uint64(AOCL_HEIGHT)
            wit_off = np.array([0, W], dtype=np.uint64)
            win = L.MsUpdateIn(wit_off.ctypes.data, ptr(mn), ptr(dist), ptr(l), ptr(leaf), apath_off.ctypes.data, ptr(apath),
                               ctypes.pointer(cc))
            appended = dict(aocl_path_off=apath_off, aocl_path=apath, entry_off=packed.entry_off, chunk_index=packed.chunk_index,
                            path_off=packed.path_off, path=packed.path, rel_off=packed.rel_off, rel=packed.rel)
            status = z(np.uint8, W)
            none = z(np.uint8, W)
            h = ctypes.c_void_p()
            L.check(lib.nhip_ms_store_create(ctx.handle, None, ctypes.byref(h)), "nhip_ms_store_create")

            def refill():
                L.check(lib.nhip_ms_store_retain(h, none.ctypes.data), "nhip_ms_store_retain")
                L.check(lib.nhip_ms_store_append(h, ctypes.byref(win), W), "nhip_ms_store_append")

            def update():
                cin.msa_expected = None
                L.check(lib.nhip_ms_store_update(h, ctypes.byref(cin), ctypes.byref(cout), status.ctypes.data),
                        "nhip_ms_store_update")
                assert blk["status"][0] == MS.OK and (status == MS.OK).all(), status[:16]

            def read_all(fill):
                L.check(lib.nhip_ms_store_read(h, None, W, ctypes.byref(fill)), "nhip_ms_store_read")

            # the store at the tip, read once: the witnesses after the block, for the plan and the batch call
            refill()
            update()
            tip, _keep_tip = MS.MutatorSetAccumulator(
                MS.MmrAccumulator(blk["aocl_peaks"][:int(blk["aocl_n_peaks"][0])].copy(), int(blk["aocl_num_leafs"][0])),
                MS.MmrAccumulator(blk["swbf_peaks"][:int(blk["swbf_n_peaks"][0])].copy(), int(blk["swbf_num_leafs"][0])),
                blk["active"][:int(blk["n_active"][0])].copy())._c()
            tips = (L.Msa * 1)(tip)
            cnt = L.MsUpdated()
            read_all(cnt)
            oa, fill_a = arrays(W, int(cnt.aocl_digests), int(cnt.entries), int(cnt.path_digests), int(cnt.rel_words))
            read_all(fill_a)
            acc = L.MsChunks(oa["entry_off"].ctypes.data, ptr(oa["chunk_index"]), oa["path_off"].ctypes.data, ptr(oa["path"]),
                             oa["rel_off"].ctypes.data, ptr(oa["rel"]))
            win_after = L.MsUpdateIn(wit_off.ctypes.data, ptr(mn), ptr(dist), ptr(l), ptr(leaf), oa["aocl_path_off"].ctypes.data,
                                     ptr(oa["aocl_path"]), ctypes.pointer(acc))
            count = L.MsUpdated()
            cin.msa_expected = tips
            L.check(lib.nhip_ms_revert_plan(ctypes.byref(cin), ctypes.byref(win_after), ctypes.byref(count)), "nhip_ms_revert_plan")
            A, E, PD, RW = int(count.aocl_digests), int(count.entries), int(count.path_digests), int(count.rel_words)
            ob, fill_b = arrays(W, A, E, PD, RW)  # the batch call's outputs
            os_, fill_s = arrays(W, A, E, PD, RW)  # read of all after the revert

            def revert():
                cin.msa_expected = tips
                L.check(lib.nhip_ms_store_revert(h, ctypes.byref(cin), ctypes.byref(cout), status.ctypes.data),
                        "nhip_ms_store_revert")

            def plan():  # the host plan alone (the count pass: nothing is written but the totals)
                L.check(lib.nhip_ms_revert_plan(ctypes.byref(cin), ctypes.byref(win_after), ctypes.byref(count)), "nhip_ms_revert_plan")

            def batch():
                cin.msa_expected = tips
                L.check(lib.nhip_ms_revert_batch(ctx.handle, ctypes.byref(cin), ctypes.byref(cout), ctypes.byref(win_after),
                                                 ctypes.byref(fill_b)), "nhip_ms_revert_batch")

            stats = {}
            for rep in range(args.repeats + 1):  # the first is the warm-up: workspace and store allocation, code load
                s = {} if rep == 0 else stats
                ctx.timing(True)
                refill()
                update()
                measured(revert, s, "revert")
                assert blk["status"][0] == MS.OK and (status == MS.OK).all(), (blk["status"][0], status[:16])
                if rep == 0:
                    read_all(fill_s)
                    assert all(os_[f][:appended[f].shape[0]].tobytes() == appended[f].tobytes() for f in appended), \
                        "the reverted store is not what was appended"
                update()
                measured(refill, s, "reupload")
                measured(plan, s, "plan")
                measured(batch, s, "batch")
                assert blk["status"][0] == MS.OK and (ob["status"][:W] == MS.OK).all()
                if rep == 0:
                    assert all(ob[f].tobytes() == os_[f].tobytes() for f in appended), "the store and the batch call differ"
                ctx.timing(False)
            lib.nhip_ms_store_destroy(h)
            row = {"witnesses": W, "additions": K, "records": M, "entries_before": E, "aocl_digests": A, "path_digests": PD,
                   "rel_words": RW, "upload_MB": round((40 * (A + PD) + 8 * E + 4 * RW + 244 * W) / 1e6, 1), "repeats": args.repeats}
            for name, v in stats.items():
                row[name + "_best"] = round(min(v), 4)
                row[name + "_median"] = round(statistics.median(v), 4)
            row["revert_speedup_wall"] = round(row["reupload_wall_ms_best"] / row["revert_wall_ms_best"], 2)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
