"""tests/blk_ms_ref.py (the CPU restatement behind tests/test_gpu_block_ms.py) held to identities read from the
reference, and the host walk nhip_blk_ms_walk held to oracle/bincode_ref.py's decode of the same bytes.  No GPU.

The two encodings' lengths follow from the derive rules (fields last-first, dynamic fields length-prefixed):
  Coin(NativeCurrency) = [5] [4] + 4 limbs + 5 = 11, Coin(TimeLock) = [2] [1] + date + 5 = 8,
  Utxo = [len(coins_enc)] + [n_coins] + ([len(coin)] + coin)* + 5, so 1 + 1 + 12 + 5 = 19 words unlocked and
  1 + 1 + 12 + 9 + 5 = 28 words time-locked."""
import random

import numpy as np
import pytest

import bincode_ref as B
import blk_ms_ref as X
import ms_apply_ref as A
import ms_ref as R

P, H = X.P, 10
TS = (tuple(range(11, 16)), tuple(range(21, 26)))


def _block(height=5, fee=0, timestamp=1000):
    g = random.Random(1)
    k = B.random_kernel(g)
    k["fee"] = fee
    b = B.random_block(g, [], B.GENESIS, tree_height=H, kernel=k)
    b["header"].update(height=height, timestamp=timestamp)
    return b


def _amount(coin):
    return sum(x << (32 * i) for i, x in enumerate(coin[1]))


def test_encodings_are_19_and_28_words():
    locked, unlocked = X.guesser_fee_utxos(_block(fee=12345), TS)
    assert len(X.encode_utxo(unlocked)) == 19 and len(X.encode_utxo(locked)) == 28
    e = X.encode_utxo(locked)
    assert e[:5] == [22, 2, 11, 5, 4] and e[9:14] == list(TS[0]) and e[14:17] == [8, 2, 1]
    assert e[17] == 1000 + X.YEARS_3 and e[18:23] == list(TS[1]) and e[23:] == list(_block()["header"]["lock_script_hash"])
    assert X.encode_utxo(unlocked)[:5] == [13, 1, 11, 5, 4]


@pytest.mark.parametrize("fee", [0, 1, 2, 7, 12345, (1 << 96) + (5 << 64) + (9 << 32) + 3, (1 << 127) - 1])
def test_locked_plus_unlocked_is_the_fee(fee):
    locked, unlocked = X.guesser_fee_utxos(_block(fee=fee), TS)
    assert _amount(locked["coins"][0]) + _amount(unlocked["coins"][0]) == fee
    assert _amount(locked["coins"][0]) == fee // 2
    assert [c[0] for c in locked["coins"]] == [TS[0], TS[1]] and [c[0] for c in unlocked["coins"]] == [TS[0]]


def test_a_fee_of_one_is_all_unlocked():
    locked, unlocked = X.guesser_fee_utxos(_block(fee=1), TS)
    assert _amount(locked["coins"][0]) == 0 and _amount(unlocked["coins"][0]) == 1


def test_no_records_at_height_zero_and_a_negative_fee_is_an_error():
    assert X.guesser_fee_utxos(_block(height=0, fee=5), TS) == []
    assert X.guesser_fee_addition_records(_block(height=0, fee=5), (1,) * 5, TS) == []
    with pytest.raises(X.NegativeFee):
        X.guesser_fee_utxos(_block(fee=-1), TS)
    assert X.guesser_fee_utxos(_block(height=0, fee=-1), TS) == []  # the genesis check comes first


def test_release_date_wraps_mod_p():
    locked, _ = X.guesser_fee_utxos(_block(timestamp=P - 1), TS)
    assert locked["coins"][1][1] == [X.YEARS_3 - 1]


def test_records_are_commitments_and_the_accumulator_after_appends_them():
    b = _block(fee=9)
    b["body"].update(aocl={"leaf_count": 0, "peaks": []}, swbf_inactive={"leaf_count": 0, "peaks": []}, swbf_active=[])
    bh = (5, 4, 3, 2, 1)
    recs = X.guesser_fee_addition_records(b, bh, TS)
    utxos = X.guesser_fee_utxos(b, TS)
    assert recs == [R._hp(R._hp(R.hash_varlen(X.encode_utxo(u)), bh), b["header"]["receiver_digest"]) for u in utxos]
    after = X.mutator_set_accumulator_after(b, bh, TS)
    assert after.aocl.num_leafs == 2 and after.aocl.peaks == [R._hp(recs[0], recs[1])]
    b["header"]["height"] = 0
    assert A.same(X.mutator_set_accumulator_after(b, bh, TS), X.body_msa(b))


def test_block_subsidy_halvings():
    first = 160815 - 21310
    assert X.block_subsidy(0) == X.block_subsidy(first - 1) == X.INITIAL_BLOCK_SUBSIDY == 512 * 10 ** 30
    assert X.block_subsidy(first) == X.INITIAL_BLOCK_SUBSIDY // 2
    assert X.block_subsidy(first + 160815 - 1) == X.INITIAL_BLOCK_SUBSIDY // 2
    assert X.block_subsidy(first + 160815) == X.INITIAL_BLOCK_SUBSIDY // 4
    g = X.INITIAL_BLOCK_SUBSIDY.bit_length()  # after this many halvings nothing is left
    assert X.block_subsidy(first + (g - 2) * 160815) == 1 and X.block_subsidy(first + (g - 1) * 160815) == 0
    assert X.block_subsidy(P - 1) == 0 and X.block_subsidy((1 << 64) - 1) == 0


def test_tx_rules_in_order():
    b = _block(fee=0)
    k = b["body"]["transaction_kernel"]
    k.update(timestamp=1000, coinbase=None, outputs=[], announcements=[])
    assert X.tx_rule(b, 0) == X.OK
    k["timestamp"] = 1001
    assert X.tx_rule(b, 0) == X.TRANSACTION_TIMESTAMP
    k["timestamp"] = 1000
    k["coinbase"] = X.block_subsidy(5)
    assert X.tx_rule(b, 0) == X.OK
    k["coinbase"] += 1
    assert X.tx_rule(b, 0) == X.COINBASE_TOO_BIG
    k["coinbase"] = -1
    assert X.tx_rule(b, 0) == X.NEGATIVE_COINBASE
    k["fee"] = -1
    assert X.tx_rule(b, 0) == X.NEGATIVE_COINBASE
    k["coinbase"] = None
    assert X.tx_rule(b, 0) == X.NEGATIVE_FEE
    k["fee"] = 0
    assert X.tx_rule(b, X.MAX_NUM) == X.OK and X.tx_rule(b, X.MAX_NUM + 1) == X.TOO_MANY_INPUTS
    assert X.tx_rule(b, 4, (3, 9, 9)) == X.TOO_MANY_INPUTS


# ------------------------------------------------------------------ the chain builder and the host walk
@pytest.fixture(scope="module")
def chain():
    c = X.Chain(TS, seed=2901, tree_height=H)
    c.add(n_outputs=7, fee=0)                      # height 0: no guesser records
    c.add(n_outputs=5, fee=11, coinbase=77)
    c.add(n_outputs=3, spend=c.unspent(2), fee=(1 << 100) + 5)
    c.add(n_outputs=0, spend=c.unspent(3), fee=1, coinbase=-4)
    return c


def test_chain_pairs_pass_the_restatement(chain):
    assert [len(a.items) for a in chain.arch_after] == [7, 14, 19, 21]
    for i in range(1, 4):
        got = X.pair_outcome(chain.blocks[i - 1], chain.blocks[i], chain.hashes[i - 1], TS, chain.arch_after[i - 1],
                             chain.triples)
        assert got == ((X.NEGATIVE_COINBASE if i == 3 else X.OK), R.OK, None), i
        assert A.same(chain.arch_after[i - 1].msa(),
                      X.mutator_set_accumulator_after(chain.blocks[i - 1], chain.hashes[i - 1], TS))


def _walk(data):
    from neptune_hip import blocks as NB
    recs = NB.blocks_from_bytes(data, H)
    return recs, NB.mutator_set_parts(data, recs, H)


def test_host_walk_matches_the_oracle_decode(chain):
    g = random.Random(7)
    extra = B.random_block(g, [], B.INVALID, tree_height=H, kernel=B.random_kernel(g, 2, 3, 2))
    data = b"".join(chain.enc) + B.encode_block(extra)
    blocks = B.blocks_from_file(data, H)
    recs, a = _walk(data)
    assert len(recs) == len(blocks) == 5
    u128 = lambda pair: int(pair[0]) | int(pair[1]) << 64  # noqa: E731
    r0 = e0 = 0
    for i, b in enumerate(blocks):
        h, k, body = b["header"], b["body"]["transaction_kernel"], b["body"]
        assert (int(a["height"][i]), int(a["timestamp"][i])) == (h["height"], h["timestamp"])
        assert list(a["receiver_digest"][i]) == h["receiver_digest"] and list(a["lock_script_hash"][i]) == h["lock_script_hash"]
        assert u128(a["fee"][i]) == k["fee"] % (1 << 128)
        assert int(a["coinbase_tag"][i]) == (k["coinbase"] is not None)
        assert u128(a["coinbase"][i]) == (k["coinbase"] or 0) % (1 << 128)
        assert int(a["kernel_timestamp"][i]) == k["timestamp"] and int(a["n_announcements"][i]) == len(k["announcements"])
        for name, mm in (("aocl", body["aocl"]), ("swbf", body["swbf_inactive"])):
            assert int(a[name + "_num_leafs"][i]) == mm["leaf_count"] and int(a[name + "_n_peaks"][i]) == len(mm["peaks"])
            assert [list(d) for d in a[name + "_peaks"][i][:len(mm["peaks"])]] == [list(d) for d in mm["peaks"]]
            assert not a[name + "_peaks"][i][len(mm["peaks"]):].any()
        assert list(a["active"][int(a["active_off"][i]):int(a["active_off"][i + 1])]) == body["swbf_active"]
        assert [list(d) for d in a["outputs"][int(a["out_off"][i]):int(a["out_off"][i + 1])]] == [list(d) for d in k["outputs"]]
        assert int(a["rec_off"][i + 1]) - int(a["rec_off"][i]) == len(k["inputs"]) and int(a["rec_off"][i]) == r0
        for rr in k["inputs"]:
            assert u128(a["minimum"][r0]) == rr["minimum"] and list(a["distances"][r0]) == rr["distances"]
            assert int(a["entry_off"][r0]) == e0 and int(a["entry_off"][r0 + 1]) == e0 + len(rr["chunks"])
            for key, path, rel in rr["chunks"]:
                assert int(a["chunk_index"][e0]) == key
                assert [list(d) for d in a["path"][int(a["path_off"][e0]):int(a["path_off"][e0 + 1])]] == [list(d) for d in path]
                assert list(a["rel"][int(a["rel_off"][e0]):int(a["rel_off"][e0 + 1])]) == list(rel)
                e0 += 1
            r0 += 1
    assert any(len(b["body"]["transaction_kernel"]["inputs"]) for b in blocks[:4])
    assert a["chunk_index"].size == e0 and a["minimum"].shape[0] == r0


def test_host_walk_saturates_peak_counts_and_fails_closed(chain):
    from neptune_hip import _lib, blocks as NB
    g = random.Random(8)
    b = B.random_block(g, [], B.GENESIS, tree_height=H)
    b["body"]["aocl"]["peaks"] = [B._rd(g) for _ in range(70)]
    data = B.encode_block(b)
    recs, a = _walk(data)
    assert int(a["aocl_n_peaks"][0]) == 65 and int(a["swbf_n_peaks"][0]) == len(b["body"]["swbf_inactive"]["peaks"])
    assert [list(d) for d in a["aocl_peaks"][0]] == [list(d) for d in b["body"]["aocl"]["peaks"][:64]]
    # a truncated block does not parse; a block offset past the buffer and an over-tall tree are argument errors
    with pytest.raises(NB.BlockFileError):
        NB.mutator_set_parts(data[:-1], recs, H)
    lib = _lib.load()
    buf = np.frombuffer(data, dtype=np.uint8)
    out = _lib.BlkMsParts()
    import ctypes
    scanned = NB._scanned(recs)
    call = lambda n_bytes, h, blocks=scanned: lib.nhip_blk_ms_walk(buf.ctypes.data, n_bytes, h,  # noqa: E731
                                                                   ctypes.cast(blocks, ctypes.c_void_p), 1, ctypes.byref(out))
    assert call(len(data), H) == _lib.NHIP_OK and out.records == len(b["body"]["transaction_kernel"]["inputs"]) > 0
    assert call(len(data), 65) == _lib.NHIP_ERR_ARG
    assert call(10, H) == _lib.NHIP_ERR_DECODE
    scanned[0].offset = len(data) + 1
    assert call(len(data), H) == _lib.NHIP_ERR_ARG
    assert lib.nhip_blk_ms_walk(buf.ctypes.data, len(data), H, None, 1, ctypes.byref(out)) == _lib.NHIP_ERR_ARG
    # an array too small for the totals
    scanned[0].offset = 0
    some = np.zeros(4096, dtype=np.uint64)
    full = _lib.BlkMsParts(*([some.ctypes.data] * len(_lib.BlkMsParts.ARRAYS)), 0, 0, 0, 0, 0, 0)
    assert lib.nhip_blk_ms_walk(buf.ctypes.data, len(data), H, ctypes.cast(scanned, ctypes.c_void_p), 1,
                                ctypes.byref(full)) == _lib.NHIP_ERR_ARG  # its records do not fit a capacity of 0
