"""The CPU side of the mutator-set checks: the restatement tests/ms_ref.py against the one piece of MMR
arithmetic the reference tree holds (auth_path_node_indices, util_types/archival_mmr.rs:250-281), its
archival builder against its own verifiers, the pure CSR packing of neptune_hip.mutator_set, the binding's
signatures, and the host-side shape validator under ASan + UBSan (tests/native/ms_shape_check.cpp, a
stand-alone program; nothing is preloaded and nothing runs on a GPU)."""
import os
import random
import shutil
import subprocess

import pytest

import ms_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
P = R.P


def _digest(rng):
    return tuple(rng.randrange(P) for _ in range(5))


def leaf_index_to_node_index(leaf_index):
    """twenty-first shared_basic (restated): 1-based post-order index of a leaf."""
    return 2 * leaf_index - bin(leaf_index).count("1") + 1


def leaf_index_to_mt_index_and_peak_index(leaf_index, num_leafs):
    """twenty-first shared_basic (restated, independently of ms_ref.mmr_verify): walk the peaks, tallest
    first, until the one that holds the leaf."""
    first, peak_index = 0, 0
    for h in range(num_leafs.bit_length() - 1, -1, -1):
        if num_leafs >> h & 1:
            if leaf_index < first + (1 << h):
                return (leaf_index - first) + (1 << h), peak_index
            first += 1 << h
            peak_index += 1
    raise AssertionError("leaf index out of bounds")


def auth_path_node_indices(num_leafs, leaf_index):
    """util_types/archival_mmr.rs:250-281, line for line (u64 wrapping arithmetic)."""
    mask = (1 << 64) - 1
    assert leaf_index < num_leafs
    merkle_tree_index, _ = leaf_index_to_mt_index_and_peak_index(leaf_index, num_leafs)
    node_index = leaf_index_to_node_index(leaf_index)
    height = 0
    tree_height = merkle_tree_index.bit_length() - 1
    ret = []
    while merkle_tree_index > 1:
        is_left_sibling = merkle_tree_index & 1 == 0
        height_pow = 1 << (height + 1)
        as_1_or_minus_1 = (2 * int(is_left_sibling) - 1) & mask
        signed_height_pow = (height_pow * as_1_or_minus_1) & mask
        sibling = (node_index + signed_height_pow - as_1_or_minus_1) & mask
        node_index += 1 << ((height + 1) * int(is_left_sibling))
        ret.append(sibling)
        merkle_tree_index >>= 1
        height += 1
    assert tree_height == len(ret)
    return ret


@pytest.mark.parametrize("num_leafs", [1, 2, 3, 8, 11, 12, 255])
def test_builder_paths_have_the_reference_shape(num_leafs):
    rng = random.Random(num_leafs)
    mmr = R.ArchivalMmr([_digest(rng) for _ in range(num_leafs)])
    acc = mmr.accumulator()
    assert len(acc.peaks) == bin(num_leafs).count("1") and acc.num_leafs == num_leafs
    # every node of the MMR by its post-order index, built by appending leaf after leaf
    nodes, stack = {}, []
    for leaf in mmr.leaves:
        nodes[len(nodes) + 1] = leaf
        stack.append((0, len(nodes)))
        while len(stack) > 1 and stack[-1][0] == stack[-2][0]:
            (h, r), (_, l) = stack.pop(), stack.pop()
            nodes[len(nodes) + 1] = R._hp(nodes[l], nodes[r])
            stack.append((h + 1, len(nodes)))
    assert [nodes[i] for _, i in stack] == acc.peaks  # tallest first
    for leaf_index in range(num_leafs):
        want = auth_path_node_indices(num_leafs, leaf_index)
        assert mmr.path_node_indices(leaf_index) == want
        path = mmr.path(leaf_index)
        assert path == [nodes[i] for i in want]
        mt, pk = leaf_index_to_mt_index_and_peak_index(leaf_index, num_leafs)
        assert len(path) == mt.bit_length() - 1
        assert R.mmr_verify(leaf_index, mmr.leaves[leaf_index], path, acc.peaks, num_leafs)
        assert not R.mmr_verify(leaf_index, mmr.leaves[leaf_index], path + [path[-1]] if path else [acc.peaks[0]],
                                acc.peaks, num_leafs)
    assert not R.mmr_verify(num_leafs, mmr.leaves[0], [], acc.peaks, num_leafs)


def test_chunk_encoding_is_length_prefixed_vec():
    # Chunk { relative_indices: Vec<u32> }: [field length = n + 1, n, idx...]
    assert R.chunk_hash([]) == R.hash_varlen([1, 0])
    assert R.chunk_hash([7, 7, 4095]) == R.hash_varlen([4, 3, 7, 7, 4095])


@pytest.fixture(scope="module")
def small_set():
    rng = random.Random(17)
    arch = R.Archival()
    removed = []
    for k in range(41):
        arch.add(_digest(rng), _digest(rng), _digest(rng))
        if k in (3, 12, 20, 33):
            victim = k - 3
            arch.remove(arch.removal_record(victim))
            removed.append(victim)
    return arch, removed


def test_every_proof_the_builder_makes_verifies(small_set):
    arch, removed = small_set
    msa = arch.msa()
    assert msa.batch_index == 5 and msa.swbf_inactive.num_leafs == 5
    inactive_seen = 0
    for leaf_index in range(len(arch.items)):
        proof = arch.membership_proof(leaf_index)
        record = arch.removal_record(leaf_index)
        inactive_seen += len(record.target_chunks)
        if leaf_index in removed:
            assert R.ms_verify(msa, arch.items[leaf_index][0], proof) == (False, R.ALREADY_REMOVED)
            assert R.can_remove(msa, record) == (True, False, R.ALREADY_REMOVED)
        else:
            assert R.ms_verify(msa, arch.items[leaf_index][0], proof) == (True, R.OK)
            assert R.can_remove(msa, record) == (True, True, R.OK)
    assert inactive_seen > 0


def test_ms_ref_rejects_and_panics_where_the_reference_does(small_set):
    arch, removed = small_set
    msa = arch.msa()
    leaf_index = next(i for i in range(len(arch.items)) if i not in removed and arch.removal_record(i).target_chunks)
    rec = arch.removal_record(leaf_index)
    dropped = R.Record(rec.absolute_indices, rec.target_chunks[1:])
    assert R.can_remove(msa, dropped) == (False, False, R.ABSENT_CHUNK)
    ci, path, chunk = rec.target_chunks[0]
    edited = R.Record(rec.absolute_indices, [(ci, path, R.Chunk(chunk.relative_indices + [1]))] + rec.target_chunks[1:])
    assert R.can_remove(msa, edited) == (False, False, R.BAD_MMR_PATH)
    proof = arch.membership_proof(leaf_index)
    item = arch.items[leaf_index][0]
    assert R.ms_verify(msa, arch.items[leaf_index + 1][0], proof) == (False, R.NOT_IN_AOCL)
    proof.target_chunks = proof.target_chunks + [(10 ** 6, [], R.Chunk([]))]  # an invalid extra entry is ignored
    assert R.ms_verify(msa, item, proof) == (True, R.OK)
    far = (msa.batch_index + 257) * R.CHUNK_SIZE
    assert R.can_remove(msa, R.Record(R.IndexSet(far, [0] * 45))) == (False, False, R.OUT_OF_RANGE)
    for minimum in ((msa.batch_index + 256) * R.CHUNK_SIZE, 1 << 127):
        with pytest.raises(R.ReferencePanics):
            R.can_remove(msa, R.Record(R.IndexSet(minimum, [2 ** 32 - 1] * 45 if minimum >> 100 else [0] * 45)))


def test_pack_chunks_round_trips():
    from neptune_hip import mutator_set as MS
    from neptune_hip.mast import AbsoluteIndexSet
    rng = random.Random(3)
    recs = []
    for n_entries in (0, 3, 1, 0, 45):
        tc = [(rng.randrange(2 ** 64), [_digest(rng) for _ in range(rng.randrange(0, 5))],
               MS.Chunk([rng.randrange(4096) for _ in range(rng.randrange(0, 30))])) for _ in range(n_entries)]
        recs.append(MS.RemovalRecord(AbsoluteIndexSet(0, [0] * 45), tc))
    packed = MS.pack_chunks(recs)
    assert list(packed.entry_off) == [0, 0, 3, 4, 4, 49]
    assert packed.path_off[0] == 0 and packed.rel_off[0] == 0
    assert int(packed.path_off[-1]) == packed.path.shape[0] and int(packed.rel_off[-1]) == packed.rel.shape[0]
    back = MS.unpack_chunks(packed)
    assert [[(ci, [tuple(d) for d in p], c.relative_indices) for ci, p, c in r.target_chunks] for r in recs] == \
        [[(ci, p, c.relative_indices) for ci, p, c in tc] for tc in back]
    empty = MS.pack_chunks([])
    assert list(empty.entry_off) == [0] and empty.chunk_index.size == 0


def test_binding_declares_the_mutator_set_entry_points():
    import neptune_hip
    import neptune_hip._lib as L
    from neptune_hip import blocks, mutator_set as MS
    assert neptune_hip.mutator_set is MS and callable(blocks.inputs_removable)
    lib = L.load()
    for name, argc in (("nhip_mmr_verify_batch", 8), ("nhip_ms_can_remove_batch", 9), ("nhip_ms_verify_batch", 12)):
        assert len(L.SIGNATURES[name][0]) == argc and hasattr(lib, name)
    assert lib.nhip_abi_version() >= 2500
    assert (MS.OK, MS.ABSENT_CHUNK, MS.BAD_MMR_PATH, MS.ALREADY_REMOVED, MS.OUT_OF_RANGE, MS.NOT_IN_AOCL) == \
        (R.OK, R.ABSENT_CHUNK, R.BAD_MMR_PATH, R.ALREADY_REMOVED, R.OUT_OF_RANGE, R.NOT_IN_AOCL)
    msa = MS.MutatorSetAccumulator(MS.MmrAccumulator([], 17), MS.MmrAccumulator([], 2))
    assert msa.batch_index == 2 and MS.MutatorSetAccumulator(MS.MmrAccumulator([], 0), MS.MmrAccumulator([], 0)).batch_index == 0


def test_shape_validator_clean_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ absent")
    subprocess.check_call(["make", "-s", "-f", "ms_shape.mk", "-C", NATIVE, f"OUT={tmp_path}"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(tmp_path, "ms_shape_check")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    good, bad = (int(x) for x in r.stdout.split()[1::2])
    assert good >= 6 and bad >= 12, r.stdout
