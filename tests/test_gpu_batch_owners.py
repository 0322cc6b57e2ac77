"""Who owns a STARK batch's memory, streams and events (stark_host.cpp: BatchMem, LaunchRes), on the
tiny golden fixture (24 main and 9 aux columns, 8 checks; its 3 proofs and a mutated copy of the first:
the smallest shape that runs every phase).  Every verdict against the fixture's: accept, accept, accept,
reject, which the oracle verifier confirms once.

  * one resident batch refilled from records, wire bytes in a pinned buffer, fewer proofs, more proofs
    (word and raw buffers grow), none, a refused refill, and records again; graph replay in the first
    half, direct launches in the second, one stream and back;
  * nhip_verify_batch / nhip_verify_batch_wire on a context of its own: 1 proof, 8 through wire, none,
    4 through records, 1 through wire (the context's verify scratch grows every buffer and switches
    source), then that context is closed with the scratch in it;
  * a resident batch that was filled from wire bytes once is closed.
Reference semantics per proof: triton_vm::verify at verifier.rs:60-63."""
import ctypes
import json
import os

import numpy as np
import pytest

import stark_ref as S
import tip5_ref as T

pytestmark = pytest.mark.gpu

WANT = [True, True, True, False]


@pytest.fixture(scope="module")
def tiny(golden_dir):
    import neptune_hip.stark as NS
    T.use_c_backend()
    g = json.load(open(os.path.join(golden_dir, "stark_tiny.json")))
    oclaims = [(c["claim"]["digest"], c["claim"]["version"], c["claim"]["input"], c["claim"]["output"])
               for c in g["cases"]]
    proofs = [np.asarray([int(w) for w in c["proof"]], dtype=np.uint64) for c in g["cases"]]
    bad = proofs[0].copy()
    bad[bad.size // 2] = np.uint64((int(bad[bad.size // 2]) + 1) % T.P)
    oclaims, proofs = oclaims + [oclaims[0]], proofs + [bad]
    params = S.StarkParams(**g["params"])
    air, _ = S.synth_air(params, num_sampled=g["num_sampled"], seed=g["seed"])
    assert [S.verify(params, air, c, [int(w) for w in p]) for c, p in zip(oclaims, proofs)] == WANT
    return {"g": g, "gair": NS.Air([int(w) for w in g["air"]]),
            "stark": NS.Stark(num_collinearity_checks=8, num_main=24, num_aux=9),
            "claims": [NS.Claim(*c) for c in oclaims], "proofs": proofs}


def _wire(proofs, lead):
    """The proofs' words as little-endian bytes, `lead` bytes in and 3 bytes apart (so the spans take
    different byte shifts): (bytes, spans)."""
    parts, spans, at = [b"\xEE" * lead], [], lead
    for p in proofs:
        spans.append((at, int(p.size)))
        parts += [p.astype("<u8").tobytes(), b"\xEE" * 3]
        at += 8 * int(p.size) + 3
    return b"".join(parts), spans


def _runs(b, want):
    for _ in range(2):  # with graphs on, the second launch replays the capture
        v, all_ok = b.run()
        assert [bool(x) for x in v] == want and all_ok == all(want)


def test_one_resident_batch_through_every_refill(ctx, tiny):
    import neptune_hip.stark as NS
    from neptune_hip import _lib
    gair, stark, claims, proofs = tiny["gair"], tiny["stark"], tiny["claims"], tiny["proofs"]
    data4, spans4 = _wire(proofs, 5)
    data8, spans8 = _wire(proofs * 2, 2)
    b = NS.Batch(ctx, gair, stark, claims, proofs)  # records, 4 proofs
    with NS.WireBuffer(ctx, len(data8)) as wb:
        b.set_graph(True)
        _runs(b, WANT)
        wb.array[:len(data4)] = np.frombuffer(data4, dtype=np.uint8)
        b.refill_wire(claims, wb, spans4)  # wire, the same 4 proofs
        wb.array[:] = 0xFF
        _runs(b, WANT)
        b.refill(claims[1:2], proofs[1:2])  # records, 1 proof: the batch shrinks
        b.set_streams(1)
        _runs(b, [True])
        wb.array[:len(data8)] = np.frombuffer(data8, dtype=np.uint8)
        b.refill_wire(claims * 2, wb, spans8)  # wire, 8 proofs: the word and raw buffers grow
        wb.array[:] = 0xFF
        _runs(b, WANT * 2)
        b.set_graph(False)
        b.refill([], [])  # nothing
        _runs(b, [])
        # refused: the wire source takes canonical words only; the batch stays empty and refillable
        m = NS.marshal(claims, [[] for _ in claims])
        arr, k = NS._span_array(spans4)
        params = stark.montgomery().c()
        wb.array[:len(data4)] = np.frombuffer(data4, dtype=np.uint8)
        rc = ctx.lib.nhip_batch_refill_wire(ctx.handle, b.handle, gair.handle, ctypes.byref(params), m.claims, wb.ptr,
                                            wb.nbytes, arr, k)
        assert rc == _lib.NHIP_ERR_ARG
        _runs(b, [])
    b.set_streams(2)
    b.refill(claims, proofs)  # records, 4 proofs again
    _runs(b, WANT)
    for i, c in enumerate(tiny["g"]["cases"]):
        xs, idx, fail = b.transcript(i)
        assert fail == 0 and [[str(x) for x in t] for t in xs] == c["samples"] and idx == c["fri_indices"]
    assert b.transcript(3)[2] != 0
    b.close()


def _verify_wire(c, tiny, claims, proofs, lead):
    import neptune_hip.stark as NS
    data, spans = _wire(proofs, lead)
    m = NS.marshal(claims, [[] for _ in spans])
    arr, k = NS._span_array(spans)
    a = np.frombuffer(data, dtype=np.uint8)
    out = np.zeros(max(k, 1), dtype=np.uint8)
    params = tiny["stark"].c()
    assert c.lib.nhip_verify_batch_wire(c.handle, tiny["gair"].handle, ctypes.byref(params), m.claims, a.ctypes.data,
                                        a.size, arr, k, out, None) == 0
    return [bool(x) for x in out[:k]]


def test_verify_scratch_grows_switches_source_and_goes_with_its_context(ctx, tiny):
    import neptune_hip as nh
    import neptune_hip.stark as NS
    gair, stark, claims, proofs = tiny["gair"], tiny["stark"], tiny["claims"], tiny["proofs"]
    with nh.Context(int(os.environ.get("LOCAL_RANK", "0"))) as c:  # its verify scratch starts empty
        assert NS.verify_batch(c, gair, stark, [(claims[2], proofs[2])]) == [True]
        assert _verify_wire(c, tiny, claims * 2, proofs * 2, 7) == WANT * 2
        assert NS.verify_batch(c, gair, stark, []) == []
        assert NS.verify_batch(c, gair, stark, list(zip(claims, proofs))) == WANT
        assert _verify_wire(c, tiny, claims[3:], proofs[3:], 0) == [False]
    # closed with its scratch; the device goes on serving the session's context
    assert NS.verify_batch(ctx, gair, stark, list(zip(claims, proofs))) == WANT


def test_resident_batch_that_used_the_wire_source_once_is_closed(ctx, tiny):
    import neptune_hip.stark as NS
    gair, stark, claims, proofs = tiny["gair"], tiny["stark"], tiny["claims"], tiny["proofs"]
    data, spans = _wire(proofs, 1)
    b = NS.Batch.from_wire(ctx, gair, stark, claims, data, spans)  # ordinary bytes: through the staging
    _runs(b, WANT)
    b.refill(claims[:2], proofs[:2])
    _runs(b, [True, True])
    b.close()
    assert NS.verify_batch(ctx, gair, stark, list(zip(claims, proofs))) == WANT
