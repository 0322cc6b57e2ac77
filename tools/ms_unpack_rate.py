#!/usr/bin/env python3
"""Rate of unpacking packed removal records on the device (block rule 2.a) on one GPU, over the
batch of tools/ms_apply_rate.py: J independent jobs from one accumulator (swbf_inactive of 2^10 chunks of 8
indices under one peak, a window of 2,000 indices), each with K addition records and M removal records of 24
indices in inactive chunks and 21 in the window.  Every job's records are packed as RemovalRecordList::pack packs
them: the hash-free parts of the restatement tests/ms_pack_ref.py (authentication_structure_node_indices,
Chunk::pack, the dictionary layout) over the tree this tool already holds, and the first job is checked against
the restatement's own pack().

Prints one JSON line, from one run (best of --repeats):
  * unpack_kernel_ms, unpack_wall_ms : nhip_ms_unpack_batch (k_ms_unpack by HIP events; the call end to end);
  * packed_wall_ms / packed_kernel_ms: nhip_ms_apply_batch_packed per call (rules 2.a-2.e);
  * plain_wall_ms / plain_kernel_ms  : nhip_ms_apply_batch on the unpacked records per call, the yardstick;
  * packed_bytes / plain_bytes       : the chunk-dictionary bytes each call stages (for the packed call: the packed
                                       input, the plan's unpacked shape without paths, and 4 bytes per path digest
                                       and 12 per family of device program);
  * unpack_perms_per_s, mtree_perms_per_s, ratio: k_ms_unpack's Tip5 permutations (a sponge per distinct chunk, one
                                       per completed family) per second against nhip_mtree_verify_dev on as many.
The unpacked paths of nhip_ms_unpack_batch are compared with the authentic ones, and every job must be accepted.

    python tools/ms_unpack_rate.py [--jobs 1024] [--additions 64] [--records 8] [--repeats 5]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("neptune-core_amd", "oracle", "tests"):
    p = os.path.join(ROOT, sub)
    if p not in sys.path:
        sys.path.insert(0, p)

P = (1 << 64) - (1 << 32) + 1
HEIGHT, CHUNK_LEN, INACTIVE, WINDOW = 10, 8, 24, 2000
B0 = 1 << HEIGHT
N0 = 8 * B0 + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=1024)
    ap.add_argument("--additions", type=int, default=64)
    ap.add_argument("--records", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    J, K, M = args.jobs, args.additions, args.records

    import ms_pack_ref as PK  # tests/: the restatement (its hash-free parts; pack() for the first job)
    import ms_ref as R
    import neptune_hip as nh
    from neptune_hip import _lib as L
    from neptune_hip import mutator_set as MS

    rng = np.random.default_rng(7)
    with nh.Context(0) as ctx:
        rel_all = np.sort(rng.integers(0, 4096, size=(B0, CHUNK_LEN), dtype=np.uint32), axis=1)
        words = np.concatenate([np.full((B0, 1), CHUNK_LEN + 1, dtype=np.uint64), np.full((B0, 1), CHUNK_LEN, dtype=np.uint64),
                                rel_all.astype(np.uint64)], axis=1)
        leaves = ctx.hash_varlen(data=words.reshape(-1), offsets=np.arange(B0 + 1, dtype=np.uint64) * np.uint64(CHUNK_LEN + 2))
        nodes = ctx.mtree_build(leaves)
        heap = np.concatenate([nodes, leaves])  # heap order: node i, leaf ci at B0 + ci
        path_all = np.stack([heap[((B0 + np.arange(B0)) >> lvl) ^ 1] for lvl in range(HEIGHT)], axis=1)
        window = np.sort(rng.integers(0, 1 << 20, size=WINDOW, dtype=np.uint32))
        before = MS.MutatorSetAccumulator(MS.MmrAccumulator(rng.integers(0, P, size=(2, 5), dtype=np.uint64), N0),
                                          MS.MmrAccumulator(nodes[1:2], B0), window)
        packed_chunk = [np.asarray(PK.chunk_pack([int(x) for x in rel_all[ci]]), dtype=np.uint32) for ci in range(B0)]

        # the records: chunk indices ascending inside a record, as try_unpack returns them
        Rn = J * M
        ci_in = np.sort(np.stack([rng.permutation(B0)[:INACTIVE] for _ in range(Rn)]), axis=1).astype(np.uint64)
        ci_act = np.stack([rng.permutation(256)[:45 - INACTIVE] for _ in range(Rn)]).astype(np.uint64) + np.uint64(B0)
        chunk = np.concatenate([ci_in, ci_act], axis=1)
        index = chunk * np.uint64(4096) + rng.integers(0, 4096, size=chunk.shape, dtype=np.uint64)
        mn = np.zeros((Rn, 2), dtype=np.uint64)
        mn[:, 0] = index.min(axis=1)
        dist = (index - mn[:, :1]).astype(np.uint32)
        E = Rn * INACTIVE
        flat = ci_in.reshape(-1).astype(np.int64)
        plain = MS.PackedChunks(np.arange(Rn + 1, dtype=np.uint64) * np.uint64(INACTIVE), ci_in.reshape(-1).copy(),
                                np.arange(E + 1, dtype=np.uint64) * np.uint64(HEIGHT),
                                np.ascontiguousarray(path_all[flat]).reshape(-1, 5),
                                np.arange(E + 1, dtype=np.uint64) * np.uint64(CHUNK_LEN),
                                np.ascontiguousarray(rel_all[flat]).reshape(-1))

        # the packed lists: one dictionary per job on its first record
        entry_off, keys, path_len, paths, rel_len, rels = np.zeros(Rn + 1, dtype=np.uint64), [], [], [], [], []
        perms = families = 0
        for j in range(J):
            cis = np.unique(ci_in[j * M:(j + 1) * M])
            structure = PK.auth_structure_node_indices(B0, [int(c) for c in cis])
            for k, ci in enumerate(cis):
                keys.append(HEIGHT if k == 0 else PK.IGNORE_TREE_HEIGHT)
                path_len.append(len(structure) if k == 0 else 0)
                rel_len.append(len(packed_chunk[ci]))
                rels.append(packed_chunk[ci])
            paths.append(heap[structure])
            entry_off[j * M + 1:] += np.uint64(len(cis))
            fam = sum(len(np.unique((cis + B0) >> lvl)) for lvl in range(1, HEIGHT + 1))
            families += fam
            perms += fam + len(cis) * ((CHUNK_LEN + 2) // 10 + 1)
        csr = lambda x: np.concatenate([[0], np.cumsum(x)]).astype(np.uint64)  # noqa: E731
        packed = MS.PackedChunks(entry_off, np.asarray(keys, dtype=np.uint64), csr(path_len),
                                 np.ascontiguousarray(np.concatenate(paths)).reshape(-1, 5), csr(rel_len),
                                 np.concatenate(rels).astype(np.uint32))
        # the first job against the restatement's pack()
        recs0 = [R.Record(R.IndexSet(int(mn[r, 0]), [int(d) for d in dist[r]]),
                          [(int(ci), [tuple(int(x) for x in d) for d in path_all[int(ci)]], R.Chunk([int(x) for x in rel_all[int(ci)]]))
                           for ci in ci_in[r]]) for r in range(M)]
        want0 = PK.pack(recs0)[0].target_chunks if M else []
        e1 = int(entry_off[1]) if M else 0
        got0 = [(int(packed.chunk_index[e]), [tuple(int(x) for x in d) for d in packed.path[int(packed.path_off[e]):int(packed.path_off[e + 1])]],
                 [int(x) for x in packed.rel[int(packed.rel_off[e]):int(packed.rel_off[e + 1])]]) for e in range(e1)]
        assert got0 == [(k, [tuple(d) for d in p], list(c.relative_indices)) for k, p, c in want0], "packing differs from the restatement"

        ptr = lambda a: a.ctypes.data if a.size else None  # noqa: E731
        rec_off = np.arange(J + 1, dtype=np.uint64) * np.uint64(M)
        add_off = np.arange(J + 1, dtype=np.uint64) * np.uint64(K)
        additions = rng.integers(0, P, size=(J * K, 5), dtype=np.uint64)
        msas = (L.Msa * J)()
        cm, _keep = before._c()
        for j in range(J):
            msas[j] = cm
        verdict, status, bad = np.zeros(J, dtype=np.uint8), np.zeros(J, dtype=np.uint8), np.zeros(J, dtype=np.uint64)
        cout = L.MsApplyOut(verdict.ctypes.data, status.ctypes.data, bad.ctypes.data)

        def apply_call(chunks, fn, name):
            cc = chunks._c()
            cin = L.MsApplyIn(J, msas, add_off.ctypes.data, ptr(additions), rec_off.ctypes.data, ptr(mn), ptr(dist),
                              ctypes.pointer(cc), None)
            return lambda: L.check(fn(ctx.handle, ctypes.byref(cin), ctypes.byref(cout)), name), (cc, cin)

        # nhip_ms_unpack_batch: sizes, then the fill that is timed
        ust, uleafs = np.zeros(J, dtype=np.uint8), np.zeros(J, dtype=np.uint64)
        pc = packed._c()
        out = L.MsUnpacked(status=ust.ctypes.data, num_leafs_aocl=uleafs.ctypes.data)
        unpack = lambda: L.check(ctx.lib.nhip_ms_unpack_batch(ctx.handle, rec_off.ctypes.data, J, ptr(mn), ptr(dist),  # noqa: E731
                                                              ctypes.byref(pc), ctypes.byref(out)), "nhip_ms_unpack_batch")
        unpack()
        Eu, PD, W = int(out.entries), int(out.path_digests), int(out.rel_words)
        assert (Eu, PD, W) == (E, E * HEIGHT, E * CHUNK_LEN) and (ust == 0).all() and (uleafs == N0).all()
        u = MS.PackedChunks(np.zeros(Rn + 1, dtype=np.uint64), np.zeros(Eu, dtype=np.uint64), np.zeros(Eu + 1, dtype=np.uint64),
                            np.zeros((PD, 5), dtype=np.uint64), np.zeros(Eu + 1, dtype=np.uint64), np.zeros(W, dtype=np.uint32))
        out.entry_off, out.chunk_index, out.path_off = u.entry_off.ctypes.data, ptr(u.chunk_index), u.path_off.ctypes.data
        out.path, out.rel_off, out.rel = ptr(u.path), u.rel_off.ctypes.data, ptr(u.rel)
        out.entries_cap, out.path_cap, out.rel_cap = Eu, PD, W
        unpack()
        for a, b in zip((u.entry_off, u.chunk_index, u.path_off, u.path, u.rel_off, u.rel),
                        (plain.entry_off, plain.chunk_index, plain.path_off, plain.path, plain.rel_off, plain.rel)):
            assert np.array_equal(a, b), "unpacked records differ from the authentic ones"

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

        uw, uk = timed(unpack)
        call_packed, _k1 = apply_call(packed, ctx.lib.nhip_ms_apply_batch_packed, "nhip_ms_apply_batch_packed")
        pw, pk = timed(call_packed)
        assert (status == MS.OK).all() and verdict.all(), status[:16]
        call_plain, _k2 = apply_call(plain, ctx.lib.nhip_ms_apply_batch, "nhip_ms_apply_batch")
        status[:] = 255
        qw, qk = timed(call_plain)
        assert (status == MS.OK).all() and verdict.all(), status[:16]

        depth = 20
        n = max(perms // depth, 1)
        d_root = ctx.upload(rng.integers(0, P, size=5, dtype=np.uint64))
        d_idx = ctx.upload(rng.integers(0, 1 << depth, size=n, dtype=np.uint64))
        d_leaf = ctx.upload(rng.integers(0, P, size=(n, 5), dtype=np.uint64))
        d_path = ctx.upload(rng.integers(0, P, size=(n * depth, 5), dtype=np.uint64))
        d_v = ctx.alloc(n)
        _, mt = timed(lambda: ctx.mtree_verify_dev(d_root, 1, d_idx, d_leaf, d_path, depth, n, d_v))

        nbytes = lambda c, skip=(): sum(getattr(c, f).nbytes for f in ("entry_off", "chunk_index", "path_off", "path", "rel_off", "rel") if f not in skip)  # noqa: E731
        packed_bytes = nbytes(packed) + nbytes(u, skip=("path",)) + 4 * PD + 12 * families
        print(json.dumps({
            "jobs": J, "additions": K, "records": M, "entries": E, "distinct_chunks": int(len(keys)), "families": families,
            "unpacked_path_digests": PD, "packed_structure_digests": int(packed.path.shape[0]),
            "unpack_kernel_ms": uk * 1e3, "unpack_wall_ms": uw * 1e3,
            "packed_wall_ms": pw * 1e3, "packed_kernel_ms": pk * 1e3, "plain_wall_ms": qw * 1e3, "plain_kernel_ms": qk * 1e3,
            "packed_bytes": int(packed_bytes), "plain_bytes": int(nbytes(plain)),
            "unpack_perms": perms, "unpack_perms_per_s": perms / uk if uk else None,
            "mtree_kernel_ms": mt * 1e3, "mtree_perms_per_s": n * depth / mt, "ratio": (perms / uk) / (n * depth / mt) if uk else None,
        }), flush=True)


if __name__ == "__main__":
    main()
