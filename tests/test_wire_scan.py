"""The in-place feed path's host side, no GPU: the scanners that find the proofs in wire
bytes without copying a word (nhip_wire_scan_txs: transfer_transaction.rs:31-47 streams as received in
peer_loop.rs:315-323; nhip_wire_scan_blocks: import_blocks_from_files.rs:100-115), checked against the
existing per-transaction scan (nhip_tx_scan + nhip_tx_parts) and the bincode restatement, and the
argument checks of nhip_verify_batch_wire, which come before any device use."""
import ctypes
import random

import numpy as np
import pytest

import bincode_ref as B


def _stream(proofs, g):
    """SingleProof txs for `proofs` plus one ProofCollection tx of small random proofs in the middle
    (as tests/test_gpu_arena.py builds it); returns (bytes, per-tx encodings, proof words in stream order)."""
    parts, order = [], []
    mid = len(proofs) // 2
    for i, p in enumerate(proofs):
        if i == mid:
            pc = {"removal_records_integrity": [g.randrange(B.P) for _ in range(33)],
                  "collect_lock_scripts": [B.P + 5, (1 << 64) - 1, 7],  # non-canonical: reduced mod p
                  "lock_scripts_halt": [[g.randrange(B.P) for _ in range(9)]], "kernel_to_outputs": [1, 2, 3],
                  "collect_type_scripts": [4], "type_scripts_halt": [],
                  "lock_script_hashes": [[1, 2, 3, 4, 5]], "type_script_hashes": [], "kernel_mast_hash": [0] * 5,
                  "salted_inputs_hash": [0] * 5, "salted_outputs_hash": [0] * 5, "merge_bit_mast_path": []}
            parts.append(B.encode_transfer_transaction({"kernel": B.random_kernel(g), "kind": B.TT_PROOF_COLLECTION,
                                                        "proof": pc}))
            for name in ("removal_records_integrity", "collect_lock_scripts"):
                order.append([int(x) % B.P for x in pc[name]])
            order.append(pc["lock_scripts_halt"][0])
            for name in ("kernel_to_outputs", "collect_type_scripts"):
                order.append(pc[name])
        parts.append(B.encode_transfer_transaction({"kernel": B.random_kernel(g), "kind": B.TT_SINGLE_PROOF,
                                                    "proof": [int(x) for x in p]}))
        order.append([int(x) for x in p])
    return b"".join(parts), parts, order


def _proofs(g, n=6):
    return [[g.randrange(B.P) for _ in range(g.randrange(1, 120))] for _ in range(n)]


def _tx_spans_by_the_existing_scan(lib, _lib, data):
    """[(byte offset in data, words)] from nhip_tx_scan + nhip_tx_parts, transaction by transaction."""
    out, pos = [], 0
    a = np.frombuffer(data, dtype=np.uint8)
    while pos < len(data):
        tx = _lib.Tx()
        assert lib.nhip_tx_scan(a.ctypes.data + pos, len(data) - pos, ctypes.byref(tx)) == _lib.NHIP_OK
        seq = np.zeros(tx.seq_words + 1, dtype=np.uint64)
        offs = np.zeros(9, dtype=np.uint64)
        spans = np.zeros(2 * tx.n_proofs + 2, dtype=np.uint64)
        dig = np.zeros(5 * tx.n_digests + 5, dtype=np.uint64)
        assert lib.nhip_tx_parts(a.ctypes.data + pos, len(data) - pos, ctypes.byref(tx), seq.ctypes.data,
                                 offs.ctypes.data, spans.ctypes.data, dig.ctypes.data) == _lib.NHIP_OK
        out += [(int(spans[2 * k]) + pos, int(spans[2 * k + 1])) for k in range(tx.n_proofs)]
        pos += tx.size
    return out


def _raw_scan(lib, _lib, data, cap, max_txs=None):
    a = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
    arr = (_lib.Span * max(cap, 1))()
    nt, npf, used = ctypes.c_size_t(99), ctypes.c_size_t(99), ctypes.c_size_t(99)
    rc = lib.nhip_wire_scan_txs(a.ctypes.data, len(data), len(data) if max_txs is None else max_txs, arr, cap,
                                ctypes.byref(nt), ctypes.byref(npf), ctypes.byref(used))
    return rc, nt.value, [(int(arr[i].offset), int(arr[i].len)) for i in range(min(npf.value, cap))], used.value


def test_scan_txs_matches_the_per_transaction_scan_and_the_words():
    import neptune_hip.stark as NS
    from neptune_hip import _lib
    lib = _lib.load()
    g = random.Random(11)
    data, parts, order = _stream(_proofs(g), g)
    for lead in (0, 1, 4, 7):  # the stream at different byte positions of its buffer
        buf = bytes(lead) + data
        spans, ntx, used = NS.wire_scan_txs(buf, start=lead)
        assert ntx == len(parts) and used == len(data)
        assert spans == [(o + lead, n) for o, n in _tx_spans_by_the_existing_scan(lib, _lib, data)]
        assert len(spans) == len(order)
        for (off, n), words in zip(spans, order):
            raw = np.frombuffer(buf, dtype="<u8", count=n, offset=off).astype(object)
            assert [int(x) % B.P for x in raw] == words
            got = np.zeros(max(n, 1), dtype=np.uint64)
            assert lib.nhip_le_words(np.frombuffer(buf, dtype=np.uint8).ctypes.data, len(buf), off, n,
                                     got.ctypes.data) == _lib.NHIP_OK
            assert got[:n].tolist() == words
    assert NS.wire_scan_txs(b"") == ([], 0, 0)
    spans, ntx, used = NS.wire_scan_txs(data, max_txs=2)
    assert ntx == 2 and used == len(parts[0]) + len(parts[1]) and len(spans) == 2


def test_scan_txs_stops_before_the_tx_that_exceeds_span_cap_and_resumes():
    import neptune_hip.stark as NS
    from neptune_hip import _lib
    lib = _lib.load()
    g = random.Random(12)
    data, parts, order = _stream(_proofs(g), g)  # txs: 3 single, the collection (5 proofs), 3 single
    full, _, _ = NS.wire_scan_txs(data)
    rc, ntx, spans, used = _raw_scan(lib, _lib, data, 5)
    # three SingleProof transactions fit; the collection's five proofs would make eight
    assert rc == _lib.NHIP_OK and ntx == 3 and spans == full[:3] and used == sum(len(p) for p in parts[:3])
    seen, pos, rounds = [], 0, 0
    while pos < len(data):
        sp, ntx, used = NS.wire_scan_txs(data, span_cap=5, start=pos)
        assert ntx >= 1 and used > 0
        seen += sp
        pos += used
        rounds += 1
    assert seen == full and rounds == 3
    # max_txs and a NULL count pointer
    a = np.frombuffer(data, dtype=np.uint8)
    arr = (_lib.Span * 64)()
    assert lib.nhip_wire_scan_txs(a.ctypes.data, len(data), 1, arr, 64, None, None, None) == _lib.NHIP_OK
    assert (int(arr[0].offset), int(arr[0].len)) == full[0]


def test_scan_txs_malformed_middle_transaction_reports_the_ones_before_it():
    import neptune_hip.stark as NS
    from neptune_hip import _lib
    lib = _lib.load()
    g = random.Random(8)
    good = [B.encode_transfer_transaction({"kernel": B.random_kernel(g), "kind": B.TT_SINGLE_PROOF,
                                           "proof": [g.randrange(B.P) for _ in range(50)]}) for _ in range(3)]
    bad = bytearray(good[0])
    bad[-8 * 50 - 8 - 4:-8 * 50 - 8] = (7).to_bytes(4, "little")  # TransferTransactionProof variant 7
    data = good[0] + good[1] + bytes(bad) + good[2]
    rc, ntx, spans, used = _raw_scan(lib, _lib, data, 64)
    assert rc == _lib.NHIP_ERR_DECODE and ntx == 2 and len(spans) == 2 and used == len(good[0]) + len(good[1])
    assert spans == NS.wire_scan_txs(good[0] + good[1])[0]
    with pytest.raises(ValueError, match="after 2 transactions"):
        NS.wire_scan_txs(data)
    # a truncated last transaction is malformed too
    rc, ntx, spans, used = _raw_scan(lib, _lib, (good[0] + good[1])[:-3], 64)
    assert rc == _lib.NHIP_ERR_DECODE and ntx == 1 and used == len(good[0])


def test_scan_txs_first_transaction_larger_than_span_cap_is_an_argument_error():
    from neptune_hip import _lib
    lib = _lib.load()
    g = random.Random(13)
    data, parts, order = _stream(_proofs(g, 2), g)  # single, collection (5 proofs), single
    coll = data[len(parts[0]):]
    rc, ntx, spans, used = _raw_scan(lib, _lib, coll, 4)
    assert rc == _lib.NHIP_ERR_ARG and ntx == 0 and spans == [] and used == 0
    rc, ntx, spans, used = _raw_scan(lib, _lib, coll, 5)
    assert rc == _lib.NHIP_OK and ntx == 1 and len(spans) == 5  # then the single's proof does not fit: stop
    rc, ntx, spans, used = _raw_scan(lib, _lib, data, 0)
    assert rc == _lib.NHIP_ERR_ARG and (ntx, used) == (0, 0)
    # not the first: NHIP_OK, stopped before it
    rc, ntx, spans, used = _raw_scan(lib, _lib, data, 4)
    assert rc == _lib.NHIP_OK and ntx == 1 and used == len(parts[0])


def test_scan_blocks_returns_the_single_proof_spans_and_block_of():
    import neptune_hip.stark as NS
    from neptune_hip import _lib
    lib = _lib.load()
    g0 = random.Random(3)
    blks, want = [], []
    for i in range(6):
        kind = B.SINGLE_PROOF if i % 3 != 1 else B.GENESIS
        proof = [g0.randrange(B.P) for _ in range(g0.randrange(1, 300))] if kind == B.SINGLE_PROOF else None
        blks.append(B.random_block(g0, [], kind, proof, 10))
        if kind == B.SINGLE_PROOF:
            want.append((i, proof))
    data = b"".join(B.encode_block(b) for b in blks)
    spans, block_of = NS.wire_scan_blocks(data, 10)
    assert block_of == [i for i, _ in want]
    assert [n for _, n in spans] == [len(p) for _, p in want]
    for (off, n), (_, p) in zip(spans, want):
        assert np.frombuffer(data, dtype="<u8", count=n, offset=off).tolist() == p
    # a short span array is an argument error; a malformed block fails the whole file
    a = np.frombuffer(data, dtype=np.uint8)
    arr = (_lib.Span * 8)()
    npf, nb = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.nhip_wire_scan_blocks(a.ctypes.data, len(data), 10, arr, None, len(want) - 1, ctypes.byref(npf),
                                     ctypes.byref(nb)) == _lib.NHIP_ERR_ARG
    assert lib.nhip_wire_scan_blocks(a.ctypes.data, len(data) - 5, 10, arr, None, 8, ctypes.byref(npf),
                                     ctypes.byref(nb)) == _lib.NHIP_ERR_DECODE
    assert npf.value == 0 and nb.value == 5


def test_verify_batch_wire_argument_checks_need_no_device(golden_dir):
    """Montgomery input form and a span that leaves the buffer are NHIP_ERR_ARG before any device use
    (this runs where no GPU exists; the context is never dereferenced)."""
    import os
    import neptune_hip.stark as NS
    from neptune_hip import _lib
    lib = _lib.load()
    z = np.load(os.path.join(golden_dir, "c3_pool.npz"))
    air = NS.Air([int(w) for w in z["air"]])
    m = NS.marshal([NS.Claim([0] * 5)], [[]])
    data = np.zeros(64, dtype=np.uint8)
    v = np.zeros(1, dtype=np.uint8)

    def call(stark, off, n):
        span = (_lib.Span * 1)()
        span[0].offset, span[0].len = off, n
        params = stark.c()
        return lib.nhip_verify_batch_wire(None, air.handle, ctypes.byref(params), m.claims, data.ctypes.data,
                                          data.size, span, 1, v, None)

    assert call(NS.Stark.default().montgomery(), 0, 8) == _lib.NHIP_ERR_ARG
    assert call(NS.Stark.default(), 1, 8) == _lib.NHIP_ERR_ARG   # 1 + 64 > 64
    assert call(NS.Stark.default(), 65, 0) == _lib.NHIP_ERR_ARG  # offset past the end
    h = ctypes.c_void_p()
    span = (_lib.Span * 1)()
    span[0].offset, span[0].len = 60, 1
    params = NS.Stark.default().c()
    assert lib.nhip_batch_prepare_wire(None, air.handle, ctypes.byref(params), m.claims, data.ctypes.data, data.size,
                                       span, 1, ctypes.byref(h)) == _lib.NHIP_ERR_ARG
    assert h.value is None
