"""GPU mutator-set checks (k_mmr_verify, k_ms_aocl_leaf, k_ms_chunk_auth, k_ms_records) against the CPU
restatement tests/ms_ref.py, never against themselves: MMR membership, RemovalRecord::validate /
MutatorSetAccumulator::can_remove, MutatorSetAccumulator::verify, Block::validate rule 2.b, and the
entry points' shape errors.  One archival set of 600 additions (75 batches) with 40 removals spread
through them is built once per module and left unchanged."""
import copy
import ctypes
import random

import numpy as np
import pytest

import ms_ref as R

pytestmark = pytest.mark.gpu

P = R.P
U64 = (1 << 64) - 1


def _digest(rng):
    return tuple(rng.randrange(P) for _ in range(5))


def _flip(d, word=2):
    d = list(d)
    d[word] = (d[word] + 1) % P
    return tuple(d)


# ---------------------------------------------------------------- ms_ref -> neptune_hip types
def to_mmr(m):
    from neptune_hip.mutator_set import MmrAccumulator
    return MmrAccumulator(list(m.peaks), m.num_leafs)


def to_msa(msa):
    from neptune_hip.mutator_set import MutatorSetAccumulator
    return MutatorSetAccumulator(to_mmr(msa.aocl), to_mmr(msa.swbf_inactive), list(msa.swbf_active))


def _chunks(target_chunks):
    from neptune_hip.mutator_set import Chunk
    return [(ci, list(path), Chunk(list(c.relative_indices))) for ci, path, c in target_chunks]


def to_record(r):
    from neptune_hip.mast import AbsoluteIndexSet
    from neptune_hip.mutator_set import RemovalRecord
    return RemovalRecord(AbsoluteIndexSet(r.absolute_indices.minimum, list(r.absolute_indices.distances)),
                         _chunks(r.target_chunks))


def to_proof(p):
    from neptune_hip.mutator_set import MsMembershipProof
    return MsMembershipProof(p.sender_randomness, p.receiver_preimage, list(p.auth_path_aocl), p.aocl_leaf_index,
                             _chunks(p.target_chunks))


# ---------------------------------------------------------------- 1. MMR membership
def _mmr_cases():
    """(mmr accumulator, items, expected) per MMR; expected from ms_ref.mmr_verify."""
    rng = random.Random(41)
    out = []
    for num_leafs in (1, 2, 11, 12, 255):
        mmr = R.ArchivalMmr([_digest(rng) for _ in range(num_leafs)])
        acc = mmr.accumulator()
        items = [(i, mmr.leaves[i], mmr.path(i)) for i in range(num_leafs)]  # every leaf: every peak, empty paths
        i = num_leafs - 1  # in the last peak
        j = 0              # in the tallest peak
        leaf, path = mmr.leaves[j], mmr.path(j)
        items.append((j, _flip(leaf), path))                                  # a leaf word flipped
        if path:
            items.append((j, leaf, [_flip(path[0])] + path[1:]))             # a path digest flipped
            items.append((j, leaf, path[:-1]))                               # one short
            items.append((j ^ 1, leaf, path))                                # siblings swapped at level 0
            if len(path) > 1:
                items.append((j ^ 2, leaf, path))                            # ... and at level 1
        items.append((j, leaf, path + [_digest(rng)]))                       # one long
        items.append((num_leafs, leaf, path))                                # leaf_index == num_leafs
        items.append((U64, leaf, path))                                      # leaf_index = 2^64 - 1
        if len(acc.peaks) > 1:
            items.append((i, mmr.leaves[j], mmr.path(i)))                    # wrong leaf for the last peak
        out.append((acc, items))
    return out


def test_mmr_membership_matches_ms_ref(ctx):
    from neptune_hip.mutator_set import mmr_verify_batch
    total = 0
    for acc, items in _mmr_cases():
        want = [R.mmr_verify(i, leaf, path, acc.peaks, acc.num_leafs) for i, leaf, path in items]
        assert want[:acc.num_leafs] == [True] * acc.num_leafs and not any(want[acc.num_leafs:])
        assert mmr_verify_batch(ctx, to_mmr(acc), items) == want
        total += len(items)
        if len(acc.peaks) > 1:
            # the right path against the wrong peak, and n_peaks one short with a leaf in the last peak
            last = acc.num_leafs - 1
            swapped = R.Mmr(acc.peaks[1:] + acc.peaks[:1], acc.num_leafs)
            short = R.Mmr(acc.peaks[:-1], acc.num_leafs)
            for m in (swapped, short):
                w = [R.mmr_verify(i, leaf, path, m.peaks, m.num_leafs) for i, leaf, path in items[:acc.num_leafs]]
                assert not w[last] and w[0] is (m is short)  # leaf 0 sits in the tallest peak
                assert mmr_verify_batch(ctx, to_mmr(m), items[:acc.num_leafs]) == w
    assert total > 300


def test_mmr_batch_of_300_runs_a_second_workgroup_and_its_tail(ctx):
    from neptune_hip.mutator_set import mmr_verify_batch
    rng = random.Random(42)
    mmr = R.ArchivalMmr([_digest(rng) for _ in range(255)])
    acc = mmr.accumulator()
    items = []
    for k in range(300):
        i = rng.randrange(255)
        leaf = mmr.leaves[i] if k % 3 else _flip(mmr.leaves[i], k % 5)
        items.append((i, leaf, mmr.path(i)))
    want = [R.mmr_verify(i, leaf, path, acc.peaks, 255) for i, leaf, path in items]
    assert want.count(True) == 200 and want[299] is (299 % 3 != 0)
    assert mmr_verify_batch(ctx, to_mmr(acc), items) == want


def test_mmr_of_2_pow_63_leaves_climbs_63_levels(ctx):
    from neptune_hip.mutator_set import mmr_verify_batch
    rng = random.Random(43)
    leaf, path = _digest(rng), [_digest(rng) for _ in range(63)]
    acc = leaf
    for sib in path:  # leaf 0: a left child at every level
        acc = R._hp(acc, sib)
    mmr = R.Mmr([acc], 1 << 63)
    items = [(0, leaf, path), (0, leaf, path[:-1]), (1, leaf, path), ((1 << 63) - 1, leaf, path), (1 << 63, leaf, path)]
    want = [R.mmr_verify(i, l, p, mmr.peaks, mmr.num_leafs) for i, l, p in items]
    assert want == [True, False, False, False, False]
    assert mmr_verify_batch(ctx, to_mmr(mmr), items) == want


# ---------------------------------------------------------------- the shared set
class World:
    pass


@pytest.fixture(scope="module")
def world():
    rng = random.Random(2025)
    arch = R.Archival()
    removed = []
    for k in range(600):
        arch.add(_digest(rng), _digest(rng), _digest(rng))
        if k % 15 == 14:  # 40 removals, each of an item added shortly or long before
            victim = rng.randrange(k) if k % 30 == 14 else k - 3
            if victim not in removed:
                arch.remove(arch.removal_record(victim))
                removed.append(victim)
    w = World()
    w.arch, w.removed, w.msa = arch, removed, arch.msa()
    assert w.msa.batch_index == 74 and len(removed) >= 35
    assert sum(1 for ci in range(74) if arch.bloom.get(ci)) >= 20  # inactive chunks are non-empty
    return w


def _can_remove_cases(w):
    """Records of early, late and removed items, and the mutants; each (label, ms_ref record)."""
    arch, msa = w.arch, w.msa
    live = [i for i in range(600) if i not in w.removed]
    cases = [(f"live {i}", arch.removal_record(i)) for i in live[:25] + live[-25:]]
    cases += [(f"removed {i}", arch.removal_record(i)) for i in w.removed[:25]]
    rng = random.Random(7)
    early = [arch.removal_record(i) for i in live[:12]]
    assert all(len(r.target_chunks) >= 3 for r in early)
    for k, rec in enumerate(early):
        tc = rec.target_chunks
        m = copy.deepcopy(rec)
        kind = k % 6
        if kind == 0:
            del m.target_chunks[rng.randrange(len(tc))]
            cases.append(("entry dropped", m))
        elif kind == 1:
            unrequired = next(ci for ci in range(74) if ci not in {c for c, _, _ in tc})
            m.target_chunks.append((unrequired, arch._derived()[1].path(unrequired),
                                    R.Chunk(list(arch.bloom.get(unrequired, [])))))
            cases.append(("extra entry, unrequired chunk index", m))
        elif kind == 2:
            m.target_chunks.insert(1, copy.deepcopy(tc[0]))
            cases.append(("duplicated entry", m))
        elif kind == 3:
            ci, path, chunk = tc[1]
            m.target_chunks[1] = (ci, path, R.Chunk(chunk.relative_indices + [rng.randrange(4096)]))
            cases.append(("chunk edited", m))
        elif kind == 4:
            ci, path, chunk = next(e for e in tc if e[1])
            pos = [e[0] for e in tc].index(ci)
            m.target_chunks[pos] = (ci, [_flip(path[0])] + path[1:], chunk)
            cases.append(("path digest flipped", m))
        else:
            ci, path, chunk = tc[0]
            m.target_chunks[0] = (next(c for c in range(74) if c not in {e[0] for e in tc}), path, chunk)
            cases.append(("wrong chunk_index", m))
    # one index in chunk batch + 257: a future index
    rec = copy.deepcopy(arch.removal_record(live[-1]))
    mn = rec.absolute_indices.minimum
    far = (msa.batch_index + 257) * R.CHUNK_SIZE + 5 - mn
    assert 0 < far < 2 ** 32
    rec.absolute_indices.distances[44] = far
    cases.append(("index in chunk batch + 257", rec))
    return cases


def test_can_remove_and_validate_match_ms_ref(ctx, world):
    from neptune_hip.mutator_set import can_remove_batch
    cases = _can_remove_cases(world)
    want = [R.can_remove(world.msa, rec) for _, rec in cases]
    can = [c for _, c, _ in want]
    assert can.count(True) >= 20 and can.count(False) >= 20
    assert {s for _, _, s in want} == {R.OK, R.ABSENT_CHUNK, R.BAD_MMR_PATH, R.ALREADY_REMOVED, R.OUT_OF_RANGE}
    got = can_remove_batch(ctx, to_msa(world.msa), [to_record(rec) for _, rec in cases])
    for (label, _), g, wnt in zip(cases, got, want):
        assert g == wnt, label
    # the same records against the set with an empty active window
    bare = R.Msa(world.msa.aocl, world.msa.swbf_inactive, [])
    want = [R.can_remove(bare, rec) for _, rec in cases]
    assert want.count((True, True, R.OK)) > can.count(True)  # removed items whose indices were all active
    assert can_remove_batch(ctx, to_msa(bare), [to_record(rec) for _, rec in cases]) == want


def test_can_remove_fails_closed_where_the_reference_panics(ctx, world):
    from neptune_hip.mutator_set import OUT_OF_RANGE, can_remove_batch
    msa = world.msa
    base = world.arch.removal_record(599)
    huge = R.Record(R.IndexSet(1 << 127, [2 ** 32 - 1] * 45), [])
    edge = R.Record(R.IndexSet((msa.batch_index + 256) * R.CHUNK_SIZE,
                               [d % R.CHUNK_SIZE for d in base.absolute_indices.distances]), [])  # all in that chunk
    saturating = R.Record(R.IndexSet((1 << 128) - 1, [0] + [1] * 44), [])
    below = R.Record(R.IndexSet((msa.batch_index + 255) * R.CHUNK_SIZE, [0] * 45), [])  # the last chunk in range
    for rec in (huge, edge, saturating):
        with pytest.raises(R.ReferencePanics):
            R.can_remove(msa, rec)
    assert R.can_remove(msa, below) == (True, True, R.OK)
    got = can_remove_batch(ctx, to_msa(msa), [to_record(r) for r in (huge, edge, saturating, below)])
    assert got == [(False, False, OUT_OF_RANGE)] * 3 + [(True, True, R.OK)]


@pytest.mark.parametrize("n_added", [0, 1, 8, 9])
def test_can_remove_at_small_aocl_sizes(ctx, n_added):
    from neptune_hip.mutator_set import can_remove_batch
    rng = random.Random(100 + n_added)
    arch = R.Archival()
    for _ in range(n_added):
        arch.add(_digest(rng), _digest(rng), _digest(rng))
    if n_added:
        arch.remove(arch.removal_record(0))
    msa = arch.msa()
    assert msa.aocl.num_leafs == n_added and msa.batch_index == (1 if n_added == 9 else 0)
    records = [arch.removal_record(i) for i in range(n_added)]
    records.append(R.Record(R.IndexSet(7, list(range(45))), []))  # all in chunk 0
    records.append(R.Record(R.IndexSet(4096, [0] * 45), []))       # all in chunk 1: active at every size here
    want = [R.can_remove(msa, r) for r in records]
    if n_added:
        assert want[0] == (True, False, R.ALREADY_REMOVED)
    if n_added == 9:
        assert want[-2] == (False, False, R.ABSENT_CHUNK) and any(r.target_chunks for r in records)
    assert can_remove_batch(ctx, to_msa(msa), [to_record(r) for r in records]) == want


# ---------------------------------------------------------------- 3. verify
def test_verify_matches_ms_ref(ctx, world):
    from neptune_hip.mutator_set import verify_batch
    arch, msa = world.arch, world.msa
    live = [i for i in range(600) if i not in world.removed]
    chosen = live[:100] + live[-100:] + world.removed
    cases = [(f"item {i}", arch.items[i][0], arch.membership_proof(i)) for i in chosen]
    rng = random.Random(9)
    for k, i in enumerate(live[100:112]):
        item, proof = arch.items[i][0], arch.membership_proof(i)
        assert len(proof.target_chunks) >= 2 and proof.auth_path_aocl
        kind = k % 6
        if kind == 0:
            cases.append(("wrong item", _flip(item), proof))
        elif kind == 1:
            proof.receiver_preimage = _flip(proof.receiver_preimage)
            cases.append(("wrong receiver_preimage", item, proof))
        elif kind == 2:
            proof.aocl_leaf_index = 600 + rng.randrange(3)
            cases.append(("aocl_leaf_index >= num_leafs", item, proof))
        elif kind == 3:
            proof.auth_path_aocl = [_flip(proof.auth_path_aocl[0])] + proof.auth_path_aocl[1:]
            cases.append(("AOCL path flipped", item, proof))
        elif kind == 4:
            del proof.target_chunks[rng.randrange(len(proof.target_chunks))]
            cases.append(("required entry missing", item, proof))
        else:
            unrequired = next(c for c in range(74) if c not in {e[0] for e in proof.target_chunks})
            proof.target_chunks.append((unrequired, [_digest(rng)], R.Chunk([1, 2, 3])))
            cases.append(("invalid extra entry", item, proof))
    # a required entry whose chunk was edited: the authentication of a needed chunk fails
    item, proof = arch.items[live[112]][0], arch.membership_proof(live[112])
    ci, path, chunk = proof.target_chunks[0]
    proof.target_chunks[0] = (ci, path, R.Chunk(chunk.relative_indices + [9]))
    cases.append(("required chunk edited", item, proof))
    want = [R.ms_verify(msa, item, proof) for _, item, proof in cases]
    assert want[:200] == [(True, R.OK)] * 200
    assert want[200:200 + len(world.removed)] == [(False, R.ALREADY_REMOVED)] * len(world.removed)
    by_label = {label: w for (label, _, _), w in zip(cases, want)}
    assert by_label["invalid extra entry"] == (True, R.OK)
    assert by_label["required entry missing"] == (False, R.ABSENT_CHUNK)
    assert by_label["required chunk edited"] == (False, R.BAD_MMR_PATH)
    assert by_label["wrong item"] == by_label["aocl_leaf_index >= num_leafs"] == (False, R.NOT_IN_AOCL)
    got = verify_batch(ctx, to_msa(msa), [item for _, item, _ in cases], [to_proof(p) for _, _, p in cases])
    for (label, _, _), g, wnt in zip(cases, got, want):
        assert g == wnt, label


# ---------------------------------------------------------------- 4. Block::validate rule 2.b
def test_inputs_removable_names_the_first_bad_record(ctx, world):
    from neptune_hip.blocks import inputs_removable
    live = [i for i in range(600) if i not in world.removed]
    records = [world.arch.removal_record(i) for i in live[:9]]
    assert all(R.can_remove(world.msa, r)[1] for r in records)
    msa = to_msa(world.msa)
    assert inputs_removable(ctx, msa, [to_record(r) for r in records]) == (True, None)
    assert inputs_removable(ctx, msa, []) == (True, None)
    bad = copy.deepcopy(records)
    del bad[4].target_chunks[0]
    bad[7] = world.arch.removal_record(world.removed[0])
    assert [R.can_remove(world.msa, r)[1] for r in bad] == [True] * 4 + [False] + [True] * 2 + [False, True]
    assert inputs_removable(ctx, msa, [to_record(r) for r in bad]) == (False, 4)


# ---------------------------------------------------------------- 5. shapes
def test_empty_batches_zero_entries_and_bad_offsets(ctx, world):
    from neptune_hip import _lib as L
    from neptune_hip import mutator_set as MS
    lib, h = ctx.lib, ctx.handle
    msa = to_msa(world.msa)
    assert MS.mmr_verify_batch(ctx, msa.aocl, []) == [] and MS.can_remove_batch(ctx, msa, []) == []
    assert MS.verify_batch(ctx, msa, [], []) == []
    cm, _keep = msa._c()
    # n = 0 through the C ABI itself
    assert lib.nhip_mmr_verify_batch(h, ctypes.byref(cm.aocl), None, None, None, None, 0, None) == L.NHIP_OK
    assert lib.nhip_ms_can_remove_batch(h, ctypes.byref(cm), None, None, None, 0, None, None, None) == L.NHIP_OK
    assert lib.nhip_ms_verify_batch(h, ctypes.byref(cm), None, None, None, None, None, None, None, 0, None,
                                    None) == L.NHIP_OK
    # a record with zero entries (all its indices active)
    rec = to_record(world.arch.removal_record(599))
    assert rec.target_chunks == []
    assert MS.can_remove_batch(ctx, msa, [rec]) == [(True, True, MS.OK)]
    # non-monotone offsets
    recs = [to_record(world.arch.removal_record(i)) for i in (0, 1)]
    mn = np.zeros((2, 2), dtype=np.uint64)
    dist = np.zeros((2, 45), dtype=np.uint32)
    out = [np.zeros(2, dtype=np.uint8) for _ in range(3)]

    def call(packed):
        cc = packed._c()
        return lib.nhip_ms_can_remove_batch(h, ctypes.byref(cm), mn.ctypes.data, dist.ctypes.data, ctypes.byref(cc), 2,
                                            out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data)

    assert call(MS.pack_chunks(recs)) == L.NHIP_OK
    for name in ("entry_off", "path_off", "rel_off"):
        packed = MS.pack_chunks(recs)
        off = getattr(packed, name)
        assert len(off) >= 3
        off[-2] = off[-1] + 1
        assert call(packed) == L.NHIP_ERR_ARG, name
    leaf = np.zeros((2, 5), dtype=np.uint64)
    idx = np.zeros(2, dtype=np.uint64)
    v = np.zeros(2, dtype=np.uint8)
    path = np.zeros((3, 5), dtype=np.uint64)
    for off, want in (([0, 2, 3], L.NHIP_OK), ([0, 2, 1], L.NHIP_ERR_ARG), ([1, 2, 3], L.NHIP_ERR_ARG)):
        o = np.asarray(off, dtype=np.uint64)
        assert lib.nhip_mmr_verify_batch(h, ctypes.byref(cm.aocl), idx.ctypes.data, leaf.ctypes.data, o.ctypes.data,
                                         path.ctypes.data, 2, v.ctypes.data) == want
    assert lib.nhip_mmr_verify_batch(h, ctypes.byref(cm.aocl), idx.ctypes.data, leaf.ctypes.data,
                                     np.asarray([0, 2, 3], dtype=np.uint64).ctypes.data, None, 2,
                                     v.ctypes.data) == L.NHIP_ERR_ARG


# ---------------------------------------------------------------- 6. one workspace under every staged call
def test_workspace_regrows_between_staged_calls_on_one_context(world):
    """The host-buffer calls carve their device buffers out of one grow-only workspace per context (1 MiB at
    first): small calls of different layouts, a call past 1 MiB that frees and regrows it (70,000 pairs,
    3 x 2.8 MB), and small calls again on the regrown one, each against its oracle."""
    import os

    import coracle as C
    import mast_ref as M
    import neptune_hip as nh
    import tip5_ref as T
    from neptune_hip.mast import mast_hash_batch
    from neptune_hip.mutator_set import can_remove_batch
    rng = np.random.default_rng(77)
    l1, r1 = (rng.integers(0, P, size=(1, 5), dtype=np.uint64) for _ in range(2))
    want1 = [int(x) for x in T.hash_pair([int(x) for x in l1[0]], [int(x) for x in r1[0]])]
    objs = [[[int(x) for x in rng.integers(0, P, size=int(rng.integers(0, 12)), dtype=np.uint64)] for _ in range(5)]
            for _ in range(3)]
    big_l, big_r = (rng.integers(0, P, size=(70000, 5), dtype=np.uint64) for _ in range(2))
    live = [i for i in range(600) if i not in world.removed]
    records = [world.arch.removal_record(i) for i in live[:6] + live[-6:] + world.removed[:12]]
    want_rm = [R.can_remove(world.msa, rec) for rec in records]
    assert {c for _, c, _ in want_rm} == {True, False}
    with nh.Context(int(os.environ.get("LOCAL_RANK", "0"))) as c:  # a context of its own: its workspace starts unallocated
        first = c.hash_pair(l1, r1)
        assert [int(x) for x in first[0]] == want1
        assert mast_hash_batch(c, objs) == [M.mast_hash(o) for o in objs]
        big = c.hash_pair(big_l, big_r)
        assert all((big[i] == C.hash_pair(big_l[i], big_r[i])).all() for i in range(70000))
        assert can_remove_batch(c, to_msa(world.msa), [to_record(rec) for rec in records]) == want_rm
        last = c.hash_pair(l1, r1)
        assert (last == first).all() and [int(x) for x in last[0]] == want1
