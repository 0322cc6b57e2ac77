"""GPU: the device-resident archival mutator set (nhip_ms_archive_*: k_ms_arch_chunk_digests, k_ms_arch_level,
k_ms_arch_tail, k_ms_arch_peaks, k_ms_arch_gather) against `ms_ref.Archival` / `ms_ref.ArchivalMmr`,
which derive everything from scratch, never against the archive itself: the accumulator, every leaf's path in both
MMRs, leaf ranges, restored membership proofs and dictionaries field by field.  The sets come from
tests/ms_update_cases.py, built once and left unchanged; each test asserts that its data reaches what it claims."""
import copy
import ctypes

import numpy as np
import pytest

import ms_apply_ref as A
import ms_archive_cases as AC
import ms_ref as R
import ms_update_cases as C
import ms_update_ref as U

pytestmark = pytest.mark.gpu

T = AC.TAIL_NODES
COUNTS = (0, 1, 2, 3, 7, 8, 9, 16, 17, 255, 256, 257, 600, 4 * T + 3)


@pytest.fixture(scope="module")
def cases():
    return C.cases()


def new_archive(ctx, arch, initial=None):
    from neptune_hip.mutator_set import Archive
    a = Archive(ctx, initial)
    a.load(*AC.load_args(arch))
    return a


def advance(arch, adds, recs):
    """The archival set after a block; `arch` stays as it is."""
    a = A.clone(arch)
    for it in adds:
        a.add(*it)
    for r in copy.deepcopy(list(recs)):
        a.remove(r)
    return a


def tuples(path):
    return [tuple(int(x) for x in d) for d in path]


def same_mmrs(archive, aocl, swbf):
    """Both MMRs of `archive` against the models: the peaks, every leaf's path (every node that is not a peak is some
    leaf's sibling, so this covers every node), the leaves."""
    acc = archive.accumulator()
    for got, model in ((acc.aocl, aocl), (acc.swbf_inactive, swbf)):
        want = model.accumulator()
        assert got.num_leafs == want.num_leafs and tuples(got.peaks) == [tuple(p) for p in want.peaks]
    for which, model in ((0, aocl), (1, swbf)):
        n = model.num_leafs
        paths = archive.aocl_paths(range(n)) if which == 0 else archive.swbf_paths(range(n))
        assert len(paths) == n
        for i in range(n):
            assert paths[i] == model.path(i), (which, n, i)
        assert tuples(archive.leaves(which, 0, n)) == model.leaves
        if n >= 3:
            assert tuples(archive.leaves(which, 1, n - 2)) == model.leaves[1:n - 1]
            assert tuples(archive.leaves(which, n - 1, 1)) == model.leaves[n - 1:]
        assert archive.leaves(which, n, 0).shape == (0, 5)


# ---------------------------------------------------------------- 1. load equals from-scratch
@pytest.mark.parametrize("n_leafs", COUNTS)
def test_load_equals_from_scratch(ctx, n_leafs):
    from neptune_hip.mutator_set import Archive
    leaves, chunks, window = AC.random_archive(n_leafs, 9000 + n_leafs)
    if n_leafs == 4 * T + 3:
        # two levels of the AOCL are read by a k_ms_arch_level launch each before the tail: those of 4 T + 3 and of
        # 2 T + 1 nodes have more than T, the next has T
        assert n_leafs > T and n_leafs >> 1 > T and n_leafs >> 2 <= T
    if len(chunks) >= 3:
        lengths = {len(ch) for ch in chunks}
        assert 0 in lengths and any(l % 2 for l in lengths)
    aocl, swbf = AC.model_mmrs(leaves, chunks)
    with Archive(ctx) as archive:
        assert archive.counts() == (0, 0, 0, 0, 0)
        archive.load(leaves, chunks, window)
        words = sum(len(ch) for ch in chunks)
        assert archive.counts() == (n_leafs, len(chunks), len(window), words, 0)
        assert archive.accumulator().swbf_active == window
        same_mmrs(archive, aocl, swbf)


def test_load_from_capacities_of_one(ctx, cases):
    """Initial capacities of 1 everywhere: the level arrays, the table and the arena are sized by the load."""
    from neptune_hip.mutator_set import Archive
    leaves, chunks, window = AC.load_args(cases.arch)
    aocl, swbf = AC.model_mmrs(leaves, chunks)
    assert swbf.accumulator().peaks == cases.msa.swbf_inactive.peaks
    for initial in (dict(aocl_leafs=1, chunks=1, rel_words=1), dict(aocl_leafs=5000, chunks=3, rel_words=100000)):
        with Archive(ctx, initial) as archive:
            archive.load(leaves, chunks, window)
            assert A.same(C.back_msa(archive.accumulator()), cases.msa)
            same_mmrs(archive, aocl, swbf)


# ---------------------------------------------------------------- 3. the chunk edges, through restore_dictionaries
def test_chunk_edges_word_for_word(ctx, cases):
    arch = cases.arch
    b = cases.msa.batch_index
    empty = [ci for ci in range(b) if not arch.bloom.get(ci)]
    repeated = [ci for ci in range(b) if len(set(arch.bloom.get(ci, []))) < len(arch.bloom.get(ci, []))]
    if not repeated:  # a second removal of an item whose indices are set already: every word twice
        arch = A.clone(arch)
        arch.remove(arch.removal_record(cases.removed[0]))
        repeated = [ci for ci in range(b) if len(set(arch.bloom.get(ci, []))) < len(arch.bloom.get(ci, []))]
    assert empty and repeated
    from neptune_hip.mast import AbsoluteIndexSet
    with new_archive(ctx, arch) as archive:
        # one index set per chunk, 45 indices inside it: its dictionary is that chunk alone
        sets = [AbsoluteIndexSet(ci * R.CHUNK_SIZE, list(range(45))) for ci in range(b)]
        got = archive.restore_dictionaries(sets)
        swbf = AC.model_mmrs(*AC.load_args(arch)[:2])[1]
        for ci, (st, tc) in enumerate(got):
            assert st == R.OK and AC.plain_chunks(tc) == [(ci, swbf.path(ci), list(arch.bloom.get(ci, [])))], ci
        assert AC.plain_chunks(got[empty[0]][1])[0][2] == []
        words = AC.plain_chunks(got[repeated[0]][1])[0][2]
        assert len(words) > len(set(words)) and words == sorted(words)
        # a set that spans chunks on both sides of the batch index keeps the inactive ones only
        wide = AbsoluteIndexSet((b - 2) * R.CHUNK_SIZE + 5, [k * 1000 for k in range(45)])
        (st, tc), = archive.restore_dictionaries([wide])
        assert st == R.OK and [e[0] for e in AC.plain_chunks(tc)] == [b - 2, b - 1]
        assert max(wide.to_array()) // R.CHUNK_SIZE > b


# ---------------------------------------------------------------- 4. restore equals the model and verifies
def _two_blocks(cases):
    """The set of 600 after 300 additions and then six removals (as tests/test_gpu_ms_store.py's first two blocks), and
    the third block: twenty additions and three removals."""
    c = cases
    arch1 = advance(c.arch, c.adds300, [])
    recs2 = [arch1.removal_record(i) for i in c.low[:6]]
    arch2 = advance(arch1, [], recs2)
    adds3 = c.adds20
    recs3 = [arch2.removal_record(i) for i in c.low[6:9]]
    return arch2, c.removed + c.low[:6], adds3, recs3, advance(arch2, adds3, recs3)


def _plain_proof(p):
    return (tuple(int(x) for x in p.sender_randomness), tuple(int(x) for x in p.receiver_preimage), tuples(p.auth_path_aocl),
            int(p.aocl_leaf_index), AC.plain_chunks(p.target_chunks))


def _restore_all(archive, arch, leafs):
    items = [arch.items[i] for i in leafs]
    return archive.restore_membership_proofs([it[0] for it in items], [it[1] for it in items], [it[2] for it in items], leafs)


def test_restore_equals_the_model_and_verifies(ctx, cases):
    from neptune_hip.mutator_set import verify_batch
    arch2, gone, _, _, _ = _two_blocks(cases)
    n = len(arch2.items)
    assert n == 900 and len(set(gone)) == len(gone) >= 10
    with new_archive(ctx, arch2) as archive:
        assert A.same(C.back_msa(archive.accumulator()), arch2.msa())
        got = _restore_all(archive, arch2, list(range(n)))
        assert [st for st, _ in got] == [R.OK] * n
        for i, (_, p) in enumerate(got):
            assert _plain_proof(p) == _plain_proof(arch2.membership_proof(i)), i
        assert any(len(p.target_chunks) >= 3 for _, p in got) and any(not p.target_chunks for _, p in got)
        # every one of them against the archive's own accumulator: live ones verify, removed ones are ALREADY_REMOVED
        verdicts = verify_batch(ctx, archive.accumulator(), [arch2.items[i][0] for i in range(n)], [p for _, p in got])
        for i, (v, st) in enumerate(verdicts):
            assert (v, st) == ((False, R.ALREADY_REMOVED) if i in gone else (True, R.OK)), i
        # the removal-record form: the dictionary alone
        leafs = list(range(0, n, 7)) + gone[:4]
        dicts = archive.restore_dictionaries([AC.lib_index_set(arch2.index_set(i)) for i in leafs])
        for i, (st, tc) in zip(leafs, dicts):
            assert st == R.OK and AC.plain_chunks(tc) == AC.plain_chunks(arch2.removal_record(i).target_chunks), i
        # a leaf index at and past the count, and both forms of a saturating set, between good ones
        from neptune_hip.mast import AbsoluteIndexSet
        it = arch2.items[5]
        mixed = archive.restore_membership_proofs([it[0]] * 4, [it[1]] * 4, [it[2]] * 4, [5, n, n + 1, 5])
        assert [st for st, _ in mixed] == [R.OK, R.NOT_IN_AOCL, R.NOT_IN_AOCL, R.OK] and mixed[1][1] is None
        assert _plain_proof(mixed[0][1]) == _plain_proof(mixed[3][1]) == _plain_proof(arch2.membership_proof(5))
        sat = AbsoluteIndexSet((1 << 128) - 5, [9] * 45)
        assert archive.restore_dictionaries([sat]) == [(R.OUT_OF_RANGE, None)]


def _aocl_range_by_search(index_set, top):
    """Every batch index whose window [beta C, beta C + W) holds all the indices: the leaf range by brute force."""
    arr = index_set.to_array()
    ok = [beta for beta in range(top) if all(0 <= i - beta * R.CHUNK_SIZE < R.WINDOW_SIZE for i in arr)]
    return ok[0] * R.BATCH_SIZE, ok[-1] * R.BATCH_SIZE + R.BATCH_SIZE - 1


def test_restore_privacy_preserving(ctx, cases):
    arch = cases.arch
    n = 600
    aocl = R.ArchivalMmr([R.aocl_leaf(*it) for it in arch.items])
    with new_archive(ctx, arch) as archive:
        clipped = 0
        for i in (0, 7, cases.live[40], 590, 599):
            s = arch.index_set(i)
            lo, hi = _aocl_range_by_search(s, 200)
            assert lo <= i <= hi
            clipped += hi > n - 1
            paths, dictionary = archive.restore_privacy_preserving(AC.lib_index_set(s))
            want_leafs = list(range(lo, min(hi, n - 1) + 1))
            assert [l for l, _ in paths] == want_leafs
            assert [p for _, p in paths] == [aocl.path(l) for l in want_leafs]
            assert AC.plain_chunks(dictionary) == AC.plain_chunks(arch.removal_record(i).target_chunks)
        assert clipped  # the clip at the leaf count was reached
        from neptune_hip.mast import AbsoluteIndexSet
        with pytest.raises(ValueError):  # a range that begins past the AOCL
            archive.restore_privacy_preserving(AbsoluteIndexSet(100 * R.CHUNK_SIZE + R.WINDOW_SIZE - 1, [0] * 45))


def test_restored_witnesses_cross_a_block_in_a_store(ctx, cases):
    """Restored witnesses go into a WitnessStore as they come, cross the next block there, and equal a fresh restore
    from an archive of the set after that block."""
    from neptune_hip.mutator_set import MutatorSetUpdate, Witness, WitnessStore
    arch2, gone, adds3, recs3, arch3 = _two_blocks(cases)
    leafs = [i for i in range(0, 900, 6) if i not in gone]
    assert len(leafs) > 100
    with new_archive(ctx, arch2) as archive, WitnessStore(ctx) as store:
        restored = _restore_all(archive, arch2, leafs)
        records = archive.restore_dictionaries([AC.lib_index_set(arch2.index_set(i)) for i in leafs[:10]])
        wits = [Witness(AC.lib_index_set(arch2.index_set(i)), p.target_chunks, i, list(R.aocl_leaf(*arch2.items[i])),
                        p.auth_path_aocl) for i, (_, p) in zip(leafs, restored)]
        wits += [Witness(AC.lib_index_set(arch2.index_set(i)), tc) for i, (_, tc) in zip(leafs[:10], records)]
        store.append(wits)
        assert all(st == (True, True, True, R.OK) for st in store.check(archive.accumulator()))
        update = MutatorSetUpdate([C.to_record(r) for r in recs3], [A.commitment(*it) for it in adds3])
        job, statuses = store.update(archive.accumulator(), update)
        assert job[1] == R.OK and statuses == [R.OK] * len(wits)
        assert A.same(C.back_msa(job[3]), arch3.msa())
        crossed = store.read()
    assert U.batch_after(arch2.msa(), len(adds3)) > arch2.msa().batch_index  # the block slides the window
    with new_archive(ctx, arch3) as after:
        fresh = _restore_all(after, arch3, leafs)
        fresh_records = after.restore_dictionaries([AC.lib_index_set(arch3.index_set(i)) for i in leafs[:10]])
    for k, (i, (st, w)) in enumerate(zip(leafs + leafs[:10], crossed)):
        assert st == R.OK
        if k < len(leafs):
            p = fresh[k][1]
            assert tuples(w.auth_path_aocl) == tuples(p.auth_path_aocl), i
            assert AC.plain_chunks(w.target_chunks) == AC.plain_chunks(p.target_chunks), i
        else:
            assert AC.plain_chunks(w.target_chunks) == AC.plain_chunks(fresh_records[k - len(leafs)][1]), i


# ---------------------------------------------------------------- 7. arguments
def test_load_shape_errors_leave_the_archive_empty(ctx):
    import neptune_hip._lib as L
    from neptune_hip.mutator_set import Archive
    leaves, chunks, window = AC.random_archive(40, 77)
    rel_off = [0]
    for ch in chunks:
        rel_off.append(rel_off[-1] + len(ch))
    rel = [x for ch in chunks for x in ch]
    first = next(c for c, ch in enumerate(chunks) if len(ch) >= 2 and ch[0] != ch[-1])
    lo, hi = rel_off[first], rel_off[first + 1]

    def edited(**kw):
        a = dict(leaves=leaves, rel_off=list(rel_off), rel=list(rel), active=list(window))
        for name, f in kw.items():
            a[name] = f(a[name])
        return a

    def swap(v, i, j):
        v = list(v)
        v[i], v[j] = v[j], v[i]
        return v

    bad = {
        "an unsorted chunk": edited(rel=lambda v: swap(v, lo, hi - 1)),
        "a relative index of 4096": edited(rel=lambda v: v[:hi - 1] + [4096] + v[hi:]),
        "an unsorted window": edited(active=lambda v: swap(v, 0, len(v) - 1)),
        "a window word of 2^20": edited(active=lambda v: v[:-1] + [1 << 20]),
        "offsets that start at 1": edited(rel_off=lambda v: [1] + v[1:]),
        "offsets that decrease": edited(rel_off=lambda v: v[:1] + [v[-1]] + v[2:]),
        "one chunk short of the batch index": edited(rel_off=lambda v: v[:-1]),
        "one chunk past the batch index": edited(rel_off=lambda v: v + [v[-1]]),
    }
    assert window[0] != window[-1] and rel_off[1] < rel_off[-1] and len(chunks) == 4
    with Archive(ctx) as archive:
        for label, a in bad.items():
            assert archive.load_raw(a["leaves"], a["rel_off"], a["rel"], a["active"]) == L.NHIP_ERR_ARG, label
            assert archive.counts() == (0, 0, 0, 0, 0), label
        archive.load(leaves, chunks, window)  # and the unedited arrays load
        assert archive.counts()[:3] == (40, 4, len(window))
        assert archive.load_raw(leaves, rel_off, rel, window) == L.NHIP_ERR_ARG  # not empty any more
        aocl, swbf = AC.model_mmrs(leaves, chunks)
        same_mmrs(archive, aocl, swbf)


def test_out_of_range_reads_and_sizing(ctx, cases):
    import neptune_hip._lib as L
    lib = ctx.lib
    with new_archive(ctx, cases.arch) as archive:
        h = archive._h
        total = ctypes.c_size_t(12345)
        for which, n in ((0, 600), (1, 74)):
            idx = np.asarray([0, n, 1], dtype=np.uint64)
            off, path = np.full(4, 7, dtype=np.uint64), np.full((64, 5), 7, dtype=np.uint64)
            for args in ((None, None, 0), (off.ctypes.data, path.ctypes.data, 64)):
                assert lib.nhip_ms_archive_paths(h, which, idx.ctypes.data, 3, *args, ctypes.byref(total)) == L.NHIP_ERR_ARG
            out = np.full((3, 5), 7, dtype=np.uint64)
            assert lib.nhip_ms_archive_leaves(h, which, n - 1, 2, out.ctypes.data) == L.NHIP_ERR_ARG
            assert lib.nhip_ms_archive_leaves(h, which, n + 1, 0, out.ctypes.data) == L.NHIP_ERR_ARG
            assert total.value == 12345 and (off == 7).all() and (path == 7).all() and (out == 7).all()
        assert lib.nhip_ms_archive_paths(h, 2, None, 0, None, None, 0, ctypes.byref(total)) == L.NHIP_ERR_ARG
        # two-call sizing of paths: the count, a capacity one too small, the exact capacity
        idx = np.asarray([3, 599, 64], dtype=np.uint64)
        assert lib.nhip_ms_archive_paths(h, 0, idx.ctypes.data, 3, None, None, 0, ctypes.byref(total)) == L.NHIP_OK
        want = sum(((int(i) ^ 600).bit_length() - 1) for i in idx)
        assert total.value == want
        off, path = np.full(4, 7, dtype=np.uint64), np.full((want, 5), 7, dtype=np.uint64)
        assert lib.nhip_ms_archive_paths(h, 0, idx.ctypes.data, 3, off.ctypes.data, path.ctypes.data, want - 1,
                                         ctypes.byref(total)) == L.NHIP_ERR_ARG
        assert (off == 7).all() and (path == 7).all()
        assert lib.nhip_ms_archive_paths(h, 0, idx.ctypes.data, 3, off.ctypes.data, path.ctypes.data, want,
                                         ctypes.byref(total)) == L.NHIP_OK
        aocl = R.ArchivalMmr([R.aocl_leaf(*it) for it in cases.arch.items])
        assert [tuples(path[int(off[k]):int(off[k + 1])]) for k in range(3)] == [aocl.path(int(i)) for i in idx]
        # ... and of restore: the count pass reads the mirror alone; a capacity one too small leaves the outputs alone
        leafs = cases.live[:30]
        sets = [AC.lib_index_set(cases.arch.index_set(i)) for i in leafs]
        totals, o = archive.restore_raw(sets, leafs)
        A_, E, PD, RW = totals
        assert A_ and E and PD and RW
        import neptune_hip.mutator_set as MS

        class S:
            def __init__(self, s):
                self.absolute_indices = s
        mn, dist = MS._index_arrays([S(s) for s in sets])
        li = np.asarray(leafs, dtype=np.uint64)
        for short in range(4):
            caps = [A_, E, PD, RW]
            caps[short] -= 1
            arrays = [np.full(k, 0xAB, dtype=dt) for k, dt in
                      ((30, np.uint8), (31, np.uint64), (5 * A_, np.uint64), (31, np.uint64), (E, np.uint64), (E + 1, np.uint64),
                       (5 * PD, np.uint64), (E + 1, np.uint64), (RW, np.uint32))]
            before = [a.copy() for a in arrays]
            cout = L.MsUpdated(*(a.ctypes.data for a in arrays), *caps)
            assert lib.nhip_ms_archive_restore(h, mn.ctypes.data, dist.ctypes.data, li.ctypes.data, 30,
                                               ctypes.byref(cout)) == L.NHIP_ERR_ARG, short
            assert all((a == b).all() for a, b in zip(arrays, before)), short
        # the host plan gives the same shape from the integers alone
        lengths = [len(cases.arch.bloom.get(ci, [])) for ci in range(74)]
        totals_plan, plan = MS.restore_plan(600, lengths, sets, leafs)
        assert totals_plan == totals
        for f in ("status", "aocl_path_off", "entry_off", "chunk_index", "path_off", "rel_off"):
            assert (plan[f] == o[f]).all(), f
        # an accumulator whose window capacity is one short
        n_active = archive.counts()[2]
        assert n_active
        z = lambda dtype, *shape: np.zeros(shape, dtype=dtype)  # noqa: E731
        a = dict(verdict=z(np.uint8, 1), status=z(np.uint8, 1), bad_record=z(np.uint64, 1),
                 aocl_peaks=z(np.uint64, 1, 64, 5), aocl_n_peaks=z(np.uint32, 1), aocl_num_leafs=z(np.uint64, 1),
                 swbf_peaks=z(np.uint64, 1, 64, 5), swbf_n_peaks=z(np.uint32, 1), swbf_num_leafs=z(np.uint64, 1),
                 active_off=np.asarray([0, n_active - 1], dtype=np.uint64), active=z(np.uint32, n_active),
                 n_active=z(np.uint64, 1))
        cout = L.MsApplyOut(*(a[f].ctypes.data for f, _ in L.MsApplyOut._fields_))
        assert lib.nhip_ms_archive_accumulator(h, ctypes.byref(cout)) == L.NHIP_ERR_ARG
        assert not a["aocl_peaks"].any() and not a["active"].any() and a["aocl_num_leafs"][0] == 0


def test_an_empty_archive(ctx):
    from neptune_hip.mast import AbsoluteIndexSet
    from neptune_hip.mutator_set import Archive
    with Archive(ctx, dict(aocl_leafs=1, chunks=1, rel_words=1)) as archive:
        acc = archive.accumulator()
        assert (acc.aocl.num_leafs, list(acc.aocl.peaks), acc.swbf_inactive.num_leafs, list(acc.swbf_active)) == (0, [], 0, [])
        assert archive.aocl_paths([]) == [] and archive.swbf_paths([]) == []
        s = AbsoluteIndexSet(17, list(range(45)))
        assert archive.restore_dictionaries([s]) == [(R.NOT_IN_AOCL, None)]
        archive.load([], [], [])  # nothing is still empty: a load may follow
        leaves, chunks, window = AC.random_archive(9, 5)
        archive.load(leaves, chunks, window)
        assert archive.counts()[:3] == (9, 1, len(window))
