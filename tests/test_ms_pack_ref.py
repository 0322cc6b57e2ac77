"""The CPU restatement of packed removal records (tests/ms_pack_ref.py, block rule 2.a): the reference's own
unit-test inputs (tests/golden/ms_pack_pins.json), pack followed by try_unpack over small archival mutator sets,
and one mutant of a good packed list per error variant and per panic."""
import json
import os

import pytest

import ms_pack_cases as C
import ms_pack_ref as K
import ms_ref as R


@pytest.fixture(scope="module")
def pins(golden_dir):
    return json.load(open(os.path.join(golden_dir, "ms_pack_pins.json")))


def _index_set(pin):
    dist = list(pin["distances"]) + [0] * (R.NUM_TRIALS - len(pin["distances"]))
    return R.IndexSet(int(pin["minimum"]), dist)


def _dictionary(pin):
    leaf = R.chunk_hash([])
    code = {0: leaf, 1: R._hp(leaf, leaf)}
    return [(key, [code[c] for c in path], R.Chunk(list(rel))) for key, path, rel in pin["dictionary"]]


def test_chunk_round_trips(pins):
    for chunk in pins["chunk_round_trips"]["chunks"]:
        assert K.chunk_try_unpack(K.chunk_pack(chunk)) == chunk
    assert K.chunk_pack([]) == [] and K.chunk_try_unpack([]) == []
    assert K.chunk_pack([0xABC]) == [0x001ABC00]  # [len, idx] from the top bit down, zero padded
    for n in (1, 2, 3, 7, 8, 4094, 4095):  # 12 (n + 1) mod 32 takes every value it can
        chunk = [(37 * k + n) % R.CHUNK_SIZE for k in range(n)]
        assert K.chunk_try_unpack(K.chunk_pack(chunk)) == chunk
        assert len(K.chunk_pack(chunk)) == (12 * (n + 1) + 31) // 32


def test_chunk_errors(pins):
    e = pins["chunk_errors"]
    packed = K.chunk_pack(e["base"])
    cases = [([e["payload_too_big"]["word"]] * e["payload_too_big"]["count"], e["payload_too_big"]["status"]),
             (packed + [e["inconsistent_length"]["append"]], e["inconsistent_length"]["status"]),
             (packed[:-1] + [packed[-1] | e["nonzero_trailing_padding"]["or_last"]],
              e["nonzero_trailing_padding"]["status"])]
    assert [s for _, s in cases] == [K.PAYLOAD_TOO_BIG, K.INCONSISTENT_LENGTH, K.NONZERO_TRAILING_PADDING]
    for words, status in cases:
        with pytest.raises(K.UnpackError) as err:
            K.chunk_try_unpack(words)
        assert err.value.status == status


def test_three_chunks_one_tree(pins):
    pin = pins["three_chunks_one_tree"]
    records = [R.Record(_index_set(pin), _dictionary(pin))]
    packed = K.pack(records)
    assert [k for k, _, _ in packed[0].target_chunks] == [2, K.IGNORE_TREE_HEIGHT, K.IGNORE_TREE_HEIGHT]
    assert K.try_unpack(packed) == records


def test_more_chunks_than_index_sets(pins):
    pin = pins["more_chunks_than_index_sets"]
    records = [R.Record(_index_set(pin), _dictionary(pin))]
    rrl = K.from_removal_records(records, pin["num_leafs_aocl"])
    packed = K.encode_as_vec(rrl)
    assert K.decode_from_vec(packed) == rrl
    assert K.try_unpack(packed) == records
    assert K.try_unpack(K.pack(records)) == records


def test_regression_inputs_return(pins):
    for pin in pins["regressions"]["inputs"]:
        records = [R.Record(_index_set(pin), _dictionary(pin))]
        status, out = K.try_unpack_status(records)
        assert status == pin["returns"]["status"]
        if status == 0:
            assert [len(r.target_chunks) for r in out] == pin["returns"]["entries"]
            assert K.decode_from_vec(records).num_leafs_aocl == pin["returns"]["num_leafs_aocl"]
        else:
            observed = K.observed_chunk_indices_from_index_sets([records[0].absolute_indices], 1)
            assert K.estimate_num_leafs_aocl(observed, [12]) == pin["returns"]["num_leafs_aocl"]


def test_too_many_chunks_and_big_index_set(pins):
    pin = pins["too_many_chunks"]
    for num_records in pin["num_records"]:
        for num_chunks in pin["num_chunks"]:
            rec = R.Record(_index_set(pin), [(i, [], R.Chunk([])) for i in range(num_chunks)])
            status, _ = K.try_unpack_status([rec] * num_records)
            assert status not in (0, K.UNPACK_PANIC), (num_records, num_chunks)
    big = pins["big_index_set"]
    rec = R.Record(R.IndexSet(int(big["minimum"]), [big["distance_all"]] * R.NUM_TRIALS), [])
    assert K.try_unpack_status([rec])[0] == big["status"] == K.INDEX_TOO_BIG


@pytest.mark.parametrize("name", sorted(C.good_lists()))
def test_pack_then_unpack_is_the_identity(name):
    records = C.good_lists()[name]
    packed = K.pack(records)
    assert all(not r.target_chunks for r in packed[1:])
    assert [r.absolute_indices for r in packed] == [r.absolute_indices for r in records]
    assert K.try_unpack(packed) == records


def test_the_sets_have_the_shapes_they_are_for():
    a, recs = C.archival(200)
    assert any(set(ci for ci, _, _ in x.target_chunks) & set(ci for ci, _, _ in y.target_chunks)
               for k, x in enumerate(recs) for y in recs[k + 1:])  # records sharing chunks
    for r in recs:
        assert R.can_remove(a.msa(), r) == (True, True, R.OK)
    keys = lambda recs: [k for k, _, _ in K.pack(recs)[0].target_chunks]  # noqa: E731
    assert keys(C.records_of(9)) == [0] and keys(C.records_of(17)) == [1, K.IGNORE_TREE_HEIGHT]  # heights 0 and 1
    assert all(not r.target_chunks for r in C.records_of(3))
    assert keys(C.sparse_trees()) == [1, 66, 67]  # two trees without chunks
    assert keys(C.records_of(41)).count(K.IGNORE_TREE_HEIGHT) >= 1 and keys(C.records_of(200)).count(K.IGNORE_TREE_HEIGHT) >= 1
    sizes = {len(c.relative_indices) for r in C.chunk_sizes() for _, _, c in r.target_chunks}
    assert {K.MAX_UNPACKED_LENGTH, 1, 0} <= sizes


@pytest.mark.parametrize("name", sorted(C.mutants()))
def test_mutant_status(name):
    packed, status = C.mutants()[name]
    assert K.try_unpack_status(packed)[0] == status


def test_every_status_has_a_mutant():
    assert {s for _, s in C.mutants().values()} >= set(range(K.PAYLOAD_TOO_BIG, K.UNPACK_PANIC + 1))
    # the panics: heights out of order, 8 s + 1 past u64, a structure that does not fit its own tree.  A sibling
    # missing while a path is read cannot follow a list that passed the per-tree length assert (the structure's
    # node indices are then exactly the siblings that cannot be computed): removing a node by hand shows the raise
    rrl = K.decode_from_vec(K.pack(C.two_trees()))
    sparse, _ = K.rebuild_nodes(rrl)
    assert (2, 3) in sparse and (2, 2) in sparse and (2, 1) in sparse
    real = K.rebuild_nodes

    def without_node(r):
        s, m = real(r)
        del s[(2, 3)]
        return s, m
    K.rebuild_nodes = without_node
    try:
        with pytest.raises(R.ReferencePanics):
            K.convert_to_vec(rrl)
    finally:
        K.rebuild_nodes = real
