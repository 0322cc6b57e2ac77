"""In-place submission: proofs verified from the wire bytes as they lie in a pinned
receive buffer (WireBuffer), found by the scanners, DMA'd run by run and gathered into aligned words on
the device (k_wire_words), against the C oracle and against the arena path on the same bytes.

  * a stream of 10 SingleProof TransferTransactions (the five pool proofs twice, one main-row word
    mutated) plus a small ProofCollection, laid into a WireBuffer at start offsets 0, 1, 4 and 7 so the
    proof spans take different byte shifts: Batch.from_wire's verdicts equal the oracle's (exactly one
    reject) and the arena path's, and the Fiat-Shamir transcripts of an accepting and of the rejecting
    proof equal those of an ordinary Batch over the same words;
  * the same stream from ordinary `bytes` (through the staging);
  * a proof whose first header word w is on the wire as w + p is accepted, as on the arena path;
  * refill_wire of a one-stream, graph-replayed batch first filled with fewer, shorter proofs (raw
    buffer growth, graph recapture);
  * GroupStream.submit_wire over three contexts, LPT and explicit placement, two WireBuffers used
    alternately and overwritten with 0xFF as soon as their submit returns;
  * blk files: the six blocks' random block proofs through scan_blocks and submit_wire are all rejected.
Reference semantics per proof: triton_vm::verify at verifier.rs:60-63."""
import random

import numpy as np
import pytest

import bench
import bincode_ref as B
import coracle as C
import stark_ref as S

pytestmark = pytest.mark.gpu

BAD = 3


def _tx(g, words):
    return B.encode_transfer_transaction({"kernel": B.random_kernel(g), "kind": B.TT_SINGLE_PROOF,
                                          "proof": [int(x) for x in words]})


def _stream(proofs, g):
    """SingleProof txs for `proofs` with one ProofCollection tx of small random proofs in the middle (as
    tests/test_gpu_arena.py builds it); returns (bytes, per proof in stream order: its index in `proofs`
    or "pc")."""
    parts, order = [], []
    mid = len(proofs) // 2
    for i, p in enumerate(proofs):
        if i == mid:
            pc = {"removal_records_integrity": [g.randrange(B.P) for _ in range(33)],
                  "collect_lock_scripts": [B.P + 5, (1 << 64) - 1, 7],
                  "lock_scripts_halt": [[g.randrange(B.P) for _ in range(9)]], "kernel_to_outputs": [1, 2, 3],
                  "collect_type_scripts": [4], "type_scripts_halt": [],
                  "lock_script_hashes": [[1, 2, 3, 4, 5]], "type_script_hashes": [], "kernel_mast_hash": [0] * 5,
                  "salted_inputs_hash": [0] * 5, "salted_outputs_hash": [0] * 5, "merge_bit_mast_path": []}
            parts.append(B.encode_transfer_transaction({"kernel": B.random_kernel(g), "kind": B.TT_PROOF_COLLECTION,
                                                        "proof": pc}))
            order += ["pc"] * 5
        parts.append(_tx(g, p))
        order.append(i)
    return b"".join(parts), order


@pytest.fixture(scope="module")
def job():
    """The 10 proofs (one mutated), their stream, the oracle's verdicts (computed once) and the arena
    path's verdicts on the same bytes."""
    import neptune_hip.stark as NS
    air_words, pool = bench.load_pool()
    hs = sorted(pool)
    air_words = [int(w) for w in air_words]
    claims = [pool[h]["claim"] for h in hs] * 2
    proofs = [np.asarray(pool[h]["proof"], dtype=np.uint64) for h in hs] * 2
    lo, hi = pool[hs[BAD % 5]]["main_rows"]
    proofs[BAD] = proofs[BAD].copy()
    proofs[BAD][(lo + hi) // 2] = np.uint64((int(proofs[BAD][(lo + hi) // 2]) + 1) % S.P)
    data, order = _stream(proofs, random.Random(11))
    want = [bool(x) for x in C.stark_verify_batch(air_words, S.StarkParams(), claims, proofs, threads=8)]
    assert want.count(False) == 1 and not want[BAD]
    gair = NS.Air(air_words)
    idx = [i for i, k in enumerate(order) if k != "pc"]
    nclaims = [NS.Claim(*claims[order[i]]) for i in idx]
    with NS.Group([0, 0, 0]) as g, NS.Arena(g, sum(len(p) for p in proofs) * 4) as a, \
            NS.GroupStream(g, gair, NS.Stark.default()) as st:
        pl, ntx, used = a.ingest_txs(data)
        assert ntx == len(proofs) + 1 and used == len(data)
        sub = NS.Placed(len(idx))
        for j, i in enumerate(idx):
            sub.proofs[j] = pl.proofs[i]
            sub.member_of[j] = pl.member_of[i]
        sub.n = len(idx)
        assert st.submit_placed(NS.marshal(nclaims, [[] for _ in idx]), sub) is None
        arena_verdicts, _ = st.finish()
    return {"air_words": air_words, "gair": gair, "claims": claims, "proofs": proofs, "data": data, "order": order,
            "idx": idx, "nclaims": nclaims, "want": want, "arena": arena_verdicts}


def _single_spans(spans, job):
    assert len(spans) == len(job["order"])
    return [spans[i] for i in job["idx"]]


@pytest.fixture(scope="module")
def plain_transcripts(ctx, job):
    """Transcripts of an accepting proof and of the rejecting one from an ordinary Batch over the words."""
    import neptune_hip.stark as NS
    b = NS.Batch(ctx, job["gair"], NS.Stark.default(), job["nclaims"], job["proofs"])
    v, _ = b.run()
    assert [bool(x) for x in v] == job["want"]
    out = {i: b.transcript(i) for i in (1, BAD)}
    b.close()
    assert out[1][2] == 0 and out[BAD][2] != 0
    return out


@pytest.mark.parametrize("lead", [0, 1, 4, 7])
def test_stream_in_a_wire_buffer_at_any_start_offset(ctx, job, plain_transcripts, lead):
    import neptune_hip.stark as NS
    data = job["data"]
    with NS.WireBuffer(ctx, lead + len(data) + 3) as wb:
        wb.array[:] = 0xEE
        wb.array[lead:lead + len(data)] = np.frombuffer(data, dtype=np.uint8)
        spans, ntx, used = wb.scan_txs(start=lead, end=lead + len(data))
        assert ntx == len(job["proofs"]) + 1 and used == len(data)
        sp = _single_spans(spans, job)
        assert len({off % 8 for off, _ in sp}) > 1  # the proofs do lie at different shifts
        b = NS.Batch.from_wire(ctx, job["gair"], NS.Stark.default(), job["nclaims"], wb, sp)
        wb.array[:] = 0xFF  # the bytes are on the device: the buffer may be reused
        v, all_ok = b.run()
        got = [bool(x) for x in v]
        assert got == job["want"] and got.count(False) == 1 and not all_ok
        assert got == job["arena"]
        for i in (1, BAD):
            assert b.transcript(i) == plain_transcripts[i], i
        b.close()


def test_pageable_source_gives_the_same_verdicts(ctx, job):
    import neptune_hip.stark as NS
    data = b"\x00\x00\x00" + job["data"]  # ordinary bytes, the stream 3 bytes in
    spans, ntx, used = NS.wire_scan_txs(data, start=3)
    sp = _single_spans(spans, job)
    b = NS.Batch.from_wire(ctx, job["gair"], NS.Stark.default(), job["nclaims"], data, sp)
    v, _ = b.run()
    b.close()
    assert [bool(x) for x in v] == job["want"]
    # the one-shot form, and the pool's verdicts unchanged for spans given in another order
    m = NS.marshal(job["nclaims"][::-1], [[] for _ in sp])
    arr, k = NS._span_array(sp[::-1])
    a = np.frombuffer(data, dtype=np.uint8)
    out = np.zeros(k, dtype=np.uint8)
    params = NS.Stark.default().c()
    import ctypes
    assert ctx.lib.nhip_verify_batch_wire(ctx.handle, job["gair"].handle, ctypes.byref(params), m.claims,
                                          a.ctypes.data, a.size, arr, k, out, None) == 0
    assert [bool(x) for x in out] == job["want"][::-1]


def test_non_canonical_header_word_is_reduced_and_accepted(ctx, job):
    import neptune_hip.stark as NS
    words = [int(x) for x in job["proofs"][0]]
    assert words[0] == len(words) - 1 and words[0] + S.P < (1 << 64)
    data = bytearray(b"\x00" * 5 + _tx(random.Random(4), words))
    (off, n), = NS.wire_scan_txs(data, start=5)[0]
    assert n == len(words) and int.from_bytes(data[off:off + 8], "little") == words[0]
    words[0] += S.P  # the same field element, not canonical on the wire (the restatement's encoder reduces)
    data[off:off + 8] = words[0].to_bytes(8, "little")
    data = bytes(data)
    claim = [NS.Claim(*job["claims"][0])]
    with NS.WireBuffer(ctx, len(data)) as wb:
        wb.array[:] = np.frombuffer(data, dtype=np.uint8)
        spans, ntx, _ = wb.scan_txs(start=5)
        assert ntx == 1 and len(spans) == 1
        raw = np.frombuffer(data, dtype="<u8", count=1, offset=spans[0][0])
        assert int(raw[0]) == words[0]  # the wire really holds w + p
        b = NS.Batch.from_wire(ctx, job["gair"], NS.Stark.default(), claim, wb, spans)
        v, all_ok = b.run()
        b.close()
    assert [bool(x) for x in v] == [True] and all_ok
    with NS.Group([0]) as g, NS.Arena(g, len(words) * 8 + 64) as a, \
            NS.GroupStream(g, job["gair"], NS.Stark.default()) as st:
        pl, ntx, _ = a.ingest_txs(data[5:])
        assert pl.words(0)[0] == len(words) - 1
        st.submit_placed(NS.marshal(claim, [[]]), pl)
        assert st.finish() == ([True], True)


def test_refill_wire_grows_the_raw_buffer_and_recaptures_the_graph(ctx, job):
    import neptune_hip.stark as NS
    order = sorted(range(5), key=lambda i: len(job["proofs"][i]))
    small = order[:2]  # fewer, shorter proofs first
    g = random.Random(21)
    data_small = b"\x00" * 6 + b"".join(_tx(g, job["proofs"][i]) for i in small)
    data = job["data"]
    with NS.WireBuffer(ctx, max(len(data_small), len(data) + 1)) as wb:
        wb.array[:len(data_small)] = np.frombuffer(data_small, dtype=np.uint8)
        spans, ntx, _ = wb.scan_txs(start=6, end=len(data_small))
        assert ntx == 2
        b = NS.Batch.from_wire(ctx, job["gair"], NS.Stark.default(), [NS.Claim(*job["claims"][i]) for i in small], wb,
                               spans)
        b.set_streams(1).set_graph(True)
        for _ in range(2):  # the second launch replays the captured graph
            v, all_ok = b.run()
            assert [bool(x) for x in v] == [True, True] and all_ok
        wb.array[1:1 + len(data)] = np.frombuffer(data, dtype=np.uint8)
        spans, ntx, _ = wb.scan_txs(start=1, end=1 + len(data))
        b.refill_wire(job["nclaims"], wb, _single_spans(spans, job))
        wb.array[:] = 0xFF
        for _ in range(2):
            v, all_ok = b.run()
            assert [bool(x) for x in v] == job["want"] and not all_ok
        b.close()


@pytest.mark.parametrize("placed", [False, True], ids=["lpt", "member_of"])
def test_group_stream_submit_wire_with_two_buffers(job, placed):
    import neptune_hip.stark as NS
    cuts = [(0, 4), (4, 7), (7, 10)]
    g0 = random.Random(31)
    results = []
    with NS.Group([0, 0, 0]) as g, NS.GroupStream(g, job["gair"], NS.Stark.default()) as st:
        size = max(sum(len(p) for p in job["proofs"][a:b]) for a, b in cuts) * 8 + (1 << 16)
        bufs = [NS.WireBuffer(g.member(0), size), NS.WireBuffer(g.member(1), size)]
        try:
            for k, (a, b) in enumerate(cuts):
                wb = bufs[k & 1]
                lead = (3, 0, 5)[k]
                data = b"".join(_tx(g0, p) for p in job["proofs"][a:b])
                wb.array[lead:lead + len(data)] = np.frombuffer(data, dtype=np.uint8)
                spans, ntx, used = wb.scan_txs(start=lead, end=lead + len(data))
                assert ntx == b - a and used == len(data)
                claims = [NS.Claim(*c) for c in job["claims"][a:b]]
                member_of = [(i + k) % 3 for i in range(b - a)] if placed else None
                r = st.submit_wire(claims, wb, spans, member_of)
                wb.array[:] = 0xFF  # reused at once: the submit has the bytes on the devices
                if r is not None:
                    results.append(r)
            results.append(st.finish())
            stats = st.stats()
        finally:
            for wb in bufs:
                wb.close()
    assert len(results) == 3
    for (a, b), (v, all_ok) in zip(cuts, results):
        assert v == job["want"][a:b] and all_ok == all(job["want"][a:b])
    assert stats["batches"] == 3 and stats["proofs"] == 10  # each proof verified exactly once


def test_blk_file_block_proofs_in_place():
    import neptune_hip.stark as NS
    air_words, _ = bench.load_pool()
    g0 = random.Random(3)
    blks, want = [], []
    for i in range(6):
        kind = B.SINGLE_PROOF if i % 3 != 1 else B.GENESIS
        proof = [g0.randrange(B.P) for _ in range(g0.randrange(1, 300))] if kind == B.SINGLE_PROOF else None
        blks.append(B.random_block(g0, [], kind, proof, 10))
        if kind == B.SINGLE_PROOF:
            want.append((i, proof))
    data = b"".join(B.encode_block(b) for b in blks)
    gair = NS.Air([int(w) for w in air_words])
    with NS.Group([0, 0]) as g, NS.GroupStream(g, gair, NS.Stark.default()) as st, \
            NS.WireBuffer(g.member(0), len(data)) as wb:
        wb.array[:] = np.frombuffer(data, dtype=np.uint8)
        spans, block_of = wb.scan_blocks(10)
        assert block_of == [i for i, _ in want] and [n for _, n in spans] == [len(p) for _, p in want]
        assert st.submit_wire([NS.Claim([0] * 5) for _ in spans], wb, spans) is None  # NHIP_OK
        v, all_ok = st.finish()
    assert v == [False] * len(want) and all_ok is False  # random words are not proofs
