#!/usr/bin/env python3
"""Rate of a block file's mutator-set and transaction rules on one GPU: a synthetic chain of --blocks
blocks (default 64 and 256; pow tree height 10, block proofs of a dozen words) on one archival mutator set, built by
the tests' chain builder (tests/blk_ms_ref.py): every block has --outputs outputs and spends --spends earlier ones,
packed, and its body's accumulator is the true one.  Two ways through the same pairs, in the same run:

  * nhip_blk_ms_check: one call over the file's bytes (host walk, block digests, guesser-fee records, the two apply
    passes, rules 2.f-2.l);
  * the per-pair Python entry points that existed before it, as a caller had to drive them: per pair
    blocks.accumulator_after, then blocks.mutator_set_update_valid_packed, over objects decoded by the test oracle
    and with the guesser-fee records taken from the CPU restatement (neither is timed; the entry points are
    unchanged, so this is what they cost on the commit before).

Prints one JSON line per block count, times in milliseconds as [best, median] of --repeats runs:
  * check_call     : the whole nhip_blk_ms_check call;
  * check_kernels  : its launches alone (HIP events of nhip_timing_* around every launch of the call);
  * per_pair_calls : the two per-pair entry points over all pairs;
  * library        : the first 16 hex digits of libneptune_hip.so's SHA-256.
Every pair must be accepted both ways.

    python tools/blk_ms_rate.py [--blocks 64 256] [--outputs 3] [--spends 1] [--repeats 5]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("neptune-core_amd", "oracle", "tests"):
    p = os.path.join(ROOT, sub)
    if p not in sys.path:
        sys.path.insert(0, p)

HEIGHT = 10
TYPE_SCRIPTS = (tuple(range(101, 106)), tuple(range(201, 206)))  # stand-ins: nothing checks the scripts themselves


def best_median(xs):
    return [round(min(xs), 3), round(statistics.median(xs), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--outputs", type=int, default=3)
    ap.add_argument("--spends", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    import blk_ms_ref as X        # tests/: the chain builder and the restatement
    import ms_pack_cases as PC    # tests/: ms_ref.Record -> library types
    import tip5_ref as T          # oracle/

    import neptune_hip as nh
    import neptune_hip.mutator_set as MS
    from neptune_hip import _lib as L
    from neptune_hip import blocks as NB

    T.use_c_backend()
    lib_hash = hashlib.sha256(open(L.LIB_PATH, "rb").read()).hexdigest()[:16]
    chain = X.Chain(TYPE_SCRIPTS, seed=8, tree_height=HEIGHT)
    chain.add(n_outputs=args.outputs + args.spends)
    t0 = time.perf_counter()
    for _ in range(max(args.blocks) - 1):
        chain.add(n_outputs=args.outputs, spend=chain.unspent(args.spends), fee=1000 + len(chain.blocks))
    build_s = time.perf_counter() - t0

    def lib_msa(m):
        return MS.MutatorSetAccumulator(MS.MmrAccumulator(list(m.aocl.peaks), m.aocl.num_leafs),
                                        MS.MmrAccumulator(list(m.swbf_inactive.peaks), m.swbf_inactive.num_leafs),
                                        list(m.swbf_active))

    with nh.Context(0) as ctx:
        for n in args.blocks:
            data = b"".join(chain.enc[:n])
            recs = NB.blocks_from_bytes(data, HEIGHT)
            params = NB.ms_params(TYPE_SCRIPTS, HEIGHT)
            result = []

            def check():
                result[:] = NB.mutator_set_links(ctx, data, recs, params)

            pairs = []
            for i in range(1, n):
                parent, b = chain.blocks[i - 1], chain.blocks[i]
                k = b["body"]["transaction_kernel"]
                pairs.append((lib_msa(X.body_msa(parent)),
                              X.guesser_fee_addition_records(parent, chain.hashes[i - 1], TYPE_SCRIPTS),
                              PC.to_library(X.to_records(k["inputs"])), [tuple(d) for d in k["outputs"]],
                              lib_msa(X.body_msa(b))))
            verdicts = []

            def per_pair():
                verdicts[:] = [NB.mutator_set_update_valid_packed(ctx, NB.accumulator_after(ctx, before, guesser), inputs,
                                                                  outputs, claimed)
                               for before, guesser, inputs, outputs, claimed in pairs]

            def timed(f, kernels):
                f()  # warm-up: workspace growth, code load
                wall, kern = [], []
                if kernels:
                    ctx.timing(True)
                for _ in range(args.repeats):
                    if kernels:
                        ctx.timing_read(reset=True)
                    t = time.perf_counter()
                    f()
                    wall.append((time.perf_counter() - t) * 1e3)
                    if kernels:
                        kern.append(ctx.timing_read(reset=True)[0])
                if kernels:
                    ctx.timing(False)
                return best_median(wall), (best_median(kern) if kernels else None)

            c_call, c_kern = timed(check, True)
            assert result[0][0] == NB.BLKMS_SKIPPED and all(r == (NB.BLKMS_OK, MS.OK, None) for r in result[1:]), result
            p_call, _ = timed(per_pair, False)
            assert all(v == (True, MS.OK) for v in verdicts), verdicts
            print(json.dumps({"blocks": n, "pairs": n - 1, "file_bytes": len(data),
                              "aocl_leaves": chain.blocks[n - 1]["body"]["aocl"]["leaf_count"],
                              "repeats": args.repeats, "check_call": c_call, "check_kernels": c_kern,
                              "per_pair_calls": p_call, "chain_build_s": round(build_s, 1), "library": lib_hash,
                              "unit": "ms [best, median]"}), flush=True)


if __name__ == "__main__":
    main()
