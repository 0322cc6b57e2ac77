#!/usr/bin/env python3
"""The feed path, arena against in-place, on one GPU: the config-4 job's 4,096 proofs as
wire bytes (bench.tx_stream) to verdicts, through

  * arena    : bench.node_from_bytes, the baseline: scan + decode copy into per-GPU pinned arenas, then
               the DMA (4 host-DRAM passes per proof byte: receive write, decode read, arena write, DMA read);
  * in_place : the same bytes copied once, outside the timed region, into two pinned WireBuffers (the
               stand-in for the network receive), then per batch nhip_wire_scan_txs (no word copied) and
               nhip_group_stream_submit_wire: DMA as the bytes lie, k_wire_words gathers them on the
               device (2 passes: receive write, DMA read).  A scan thread works on batch k + 1 while
               batch k uploads; verdicts are checked inside the timed region;
  * kernel   : the pinned-link rate (one pinned -> device copy of the job's bytes, best of 3, as
               bench.pcie_stream measures it) and k_wire_words alone on the whole batch (HIP events of
               nhip_timing_* around the launch inside nhip_le_words_gpu).

Each leg is a child process of its own under `timeout -k 10`; a leg that fails or times out ends the run
(nothing more is started on the GPU).  Prints one JSON line.  The pass counts are stated from the code
paths, not measured; on one GPU the host is idle, so the two rates are expected to be equal within the
arena leg's own spread (the gain is a host-DRAM one, at 4 or more GPUs per socket).

    python tools/wire_feed.py [--batches 12] [--repeats 3] [--proofs 4096]
"""
import argparse
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("oracle", "neptune-core_amd", ""):
    p = os.path.join(ROOT, sub)
    if p not in sys.path:
        sys.path.insert(0, p)

LEG_TIMEOUT_S = {"arena": 300, "in_place": 300, "kernel": 240}


def job(total):
    import bench
    pool4 = bench.load_pool4()
    claims, proofs, expect, _, _, _ = bench.make_config4(pool4, total, 0.01, 1, 0)
    return bench, pool4["air"], claims, proofs, expect, bench.tx_stream(proofs)


def leg_arena(args):
    bench, air_words, claims, proofs, expect, stream = job(args.proofs)
    runs = [bench.node_from_bytes([0], air_words, claims, proofs, expect, args.batches, stream)
            for _ in range(args.repeats)]
    return {"proofs_per_s": [r["value"] for r in runs], "verdicts_correct": all(r["verdicts_correct"] for r in runs),
            "decode_ms_per_batch": [r["per_batch_ms"]["decode"] for r in runs],
            "submit_ms_per_batch": [r["per_batch_ms"]["submit"] for r in runs],
            "wire_bytes_per_batch": runs[0]["wire_bytes_per_batch"], "proof_bytes_per_batch": runs[0]["proof_bytes_per_batch"]}


def in_place_once(NS, st, bufs, cm, n, size, want, batches):
    """`batches` batches through submit_wire: returns (seconds, verdicts ok, scan ms, submit ms)."""
    import queue as pyqueue
    free = threading.Semaphore(2)
    ready = pyqueue.Queue()
    scan_ms, submit_ms = [], []
    ok = [True]

    def producer(total):
        try:
            for k in range(total):
                free.acquire()  # this buffer's previous batch has been submitted (its bytes are on the GPU)
                t = time.perf_counter()
                spans, ntx, used = bufs[k % 2].scan_txs(span_cap=n, end=size, raw=True)
                scan_ms.append((time.perf_counter() - t) * 1e3)
                if len(spans) != n or ntx != n or used != size:
                    ok[0] = False
                ready.put(spans)
        except Exception as e:  # noqa: BLE001 - surfaces on the consumer side
            ready.put(e)

    def run(total):
        th = threading.Thread(target=producer, args=(total,))
        th.start()
        for k in range(total):
            spans = ready.get()
            if isinstance(spans, Exception):
                raise spans
            t = time.perf_counter()
            r = st.submit_wire(cm, bufs[k % 2].array[:size], spans)
            submit_ms.append((time.perf_counter() - t) * 1e3)
            free.release()
            ok[0] = ok[0] and (r is None or r[0] == want)
        ok[0] = ok[0] and st.finish()[0] == want
        th.join()

    run(2)  # warm: device batches and raw buffers allocated
    scan_ms.clear()
    submit_ms.clear()
    t0 = time.perf_counter()
    run(batches)
    return time.perf_counter() - t0, ok[0], float(np.median(scan_ms)), float(np.median(submit_ms))


def leg_in_place(args):
    import neptune_hip.stark as NS
    bench, air_words, claims, proofs, expect, stream = job(args.proofs)
    n, size = len(proofs), int(stream.size)
    want = [bool(x) for x in expect]
    cm = NS.marshal([NS.Claim(*c) for c in claims], [[] for _ in claims])
    gair = NS.Air([int(w) for w in air_words])
    out = {"proofs_per_s": [], "scan_ms_per_batch": [], "submit_ms_per_batch": [], "verdicts_correct": True}
    with NS.Group([0]) as g, NS.GroupStream(g, gair, NS.Stark.default()) as st:
        bufs = [NS.WireBuffer(g.member(0), size), NS.WireBuffer(g.member(0), size)]
        try:
            for wb in bufs:  # the network receive's stand-in, outside the timed region
                wb.array[:size] = stream
            for _ in range(args.repeats):
                dt, ok, scan, submit = in_place_once(NS, st, bufs, cm, n, size, want, args.batches)
                out["proofs_per_s"].append(n * args.batches / dt)
                out["scan_ms_per_batch"].append(scan)
                out["submit_ms_per_batch"].append(submit)
                out["verdicts_correct"] = out["verdicts_correct"] and ok
        finally:
            for wb in bufs:
                wb.close()
    return out


def leg_kernel(args):
    import neptune_hip as nh
    import neptune_hip.stark as NS
    bench, air_words, claims, proofs, expect, stream = job(args.proofs)
    size = int(stream.size)
    with nh.Context(0) as ctx, NS.WireBuffer(ctx, size) as wb:
        wb.array[:size] = stream
        spans, ntx, used = wb.scan_txs(span_cap=len(proofs), end=size)
        dbuf = ctx.alloc(size)
        link = []
        for _ in range(3):
            t = time.perf_counter()
            dbuf.upload(wb.array[:size])
            link.append(size / (time.perf_counter() - t))
        dbuf.free()
        ms = []
        for _ in range(3):  # the first call also grows the workspace
            ctx.timing(True)
            ctx.timing_read(reset=True)
            words = NS.le_words_gpu(ctx, wb, spans)
            t_ms, launches = ctx.timing_read(reset=True)
            ctx.timing(False)
            assert launches == 1
            ms.append(t_ms)
        off, cnt = spans[len(spans) // 2]
        ok = bool((words[-spans[-1][1]:] == proofs[-1]).all()) and words.size == sum(len(p) for p in proofs) and \
            bool((np.frombuffer(wb.array[off:off + 8 * cnt].tobytes(), dtype="<u8") == proofs[len(spans) // 2]).all())
    return {"pinned_link_GBps": max(link) / 1e9, "k_wire_words_ms": ms, "words": int(words.size), "words_correct": ok,
            "k_wire_words_GBps_in_plus_out": 16 * words.size / (min(ms) * 1e-3) / 1e9}


LEGS = {"arena": leg_arena, "in_place": leg_in_place, "kernel": leg_kernel}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--proofs", type=int, default=4096)
    ap.add_argument("--leg", choices=sorted(LEGS), help="(internal) run one leg in this process")
    args = ap.parse_args()
    if args.leg:
        print("WIRE_FEED_LEG " + json.dumps(LEGS[args.leg](args)), flush=True)
        return 0
    res = {}
    for leg in ("arena", "in_place", "kernel"):
        cmd = ["timeout", "-k", "10", str(LEG_TIMEOUT_S[leg]), sys.executable, os.path.abspath(__file__), "--leg", leg,
               "--batches", str(args.batches), "--repeats", str(args.repeats), "--proofs", str(args.proofs)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("WIRE_FEED_LEG ")]
        if r.returncode != 0 or not line:
            # a fault, an abort or a time limit: nothing more is started on the GPU
            print(json.dumps({"error": f"leg {leg} ended with status {r.returncode}", "stderr": r.stderr[-2000:],
                              "legs": res}))
            return 1
        res[leg] = json.loads(line[-1][len("WIRE_FEED_LEG "):])
    a, w = res["arena"]["proofs_per_s"], res["in_place"]["proofs_per_s"]
    spread = max(a) - min(a)
    out = {"metric": "wire bytes -> verdicts, one MI355X, config-4 job", "unit": "proofs/s",
           "arena_proofs_per_s": float(np.median(a)), "in_place_proofs_per_s": float(np.median(w)),
           "arena_repeats": a, "in_place_repeats": w, "arena_spread": spread,
           "in_place_within_arena_spread": bool(np.median(w) >= np.median(a) - spread),
           "pinned_link_GBps": res["kernel"]["pinned_link_GBps"],
           "host_dram_passes_per_proof_byte": {"arena": 4, "in_place": 2, "stated_from": "the code paths"},
           "host_decode_ms_per_batch_removed": float(np.median(res["arena"]["decode_ms_per_batch"]) -
                                                     np.median(res["in_place"]["scan_ms_per_batch"])),
           "arena_decode_ms_per_batch": float(np.median(res["arena"]["decode_ms_per_batch"])),
           "in_place_scan_ms_per_batch": float(np.median(res["in_place"]["scan_ms_per_batch"])),
           "k_wire_words_ms_per_batch": min(res["kernel"]["k_wire_words_ms"]),
           "verdicts_correct": bool(res["arena"]["verdicts_correct"] and res["in_place"]["verdicts_correct"] and
                                    res["kernel"]["words_correct"]),
           "batches": args.batches, "repeats": args.repeats, "proofs_per_batch": args.proofs,
           "wire_bytes_per_batch": res["arena"]["wire_bytes_per_batch"],
           "caveat": "one GPU, idle host: no speed-up promised; the gain (2 instead of 4 host-DRAM passes) shows "
                     "only at 4 or more GPUs per socket and is unmeasured", "legs": res}
    print(json.dumps(out))
    return 0 if out["verdicts_correct"] else 1


if __name__ == "__main__":
    sys.exit(main())
