"""nhip_ms_archive_restore_plan, the host half of nhip_ms_archive_restore, through ctypes (no GPU): every shape array
and every status against the membership proofs and removal records `ms_ref.Archival` derives from scratch for the set
of 600 of tests/ms_update_cases.py, the statuses at the edges (a leaf index at and past the count, an empty archive, a
saturating index set, a chunk index at b + 255 and b + 256), the two-call sizing and the shape errors."""
import ctypes

import numpy as np
import pytest

import ms_archive_cases as AC
import ms_ref as R
import ms_update_cases as C


@pytest.fixture(scope="module")
def cases():
    return C.cases()


@pytest.fixture(scope="module")
def lengths(cases):
    return [len(cases.arch.bloom.get(ci, [])) for ci in range(cases.msa.batch_index)]


def test_abi_and_signatures():
    import neptune_hip._lib as L
    import neptune_hip.mutator_set as MS
    lib = L.load()
    assert lib.nhip_abi_version() >= 3200
    for name, argc in (("nhip_ms_archive_create", 3), ("nhip_ms_archive_destroy", 1), ("nhip_ms_archive_count", 6),
                       ("nhip_ms_archive_load", 8), ("nhip_ms_archive_apply", 3), ("nhip_ms_archive_accumulator", 2), ("nhip_ms_archive_paths", 8),
                       ("nhip_ms_archive_leaves", 5), ("nhip_ms_archive_restore", 6), ("nhip_ms_archive_restore_plan", 8)):
        assert len(L.SIGNATURES[name][0]) == argc and hasattr(lib, name), name
    assert ctypes.sizeof(L.MsArchiveCaps) == 3 * ctypes.sizeof(ctypes.c_size_t)
    for method in ("load", "apply", "accumulator", "counts", "aocl_paths", "swbf_paths", "leaves", "restore_membership_proofs",
                   "restore_dictionaries", "restore_privacy_preserving", "close"):
        assert callable(getattr(MS.Archive, method)), method


def test_every_leaf_of_the_set_of_600(cases, lengths):
    import neptune_hip.mutator_set as MS
    arch = cases.arch
    n = len(arch.items)
    assert n == 600 and cases.removed and sum(lengths) > 0 and 0 in lengths
    sets = [AC.lib_index_set(arch.index_set(i)) for i in range(n)]
    totals, o = MS.restore_plan(n, lengths, sets, list(range(n)))
    assert not o["status"].any()
    want = [arch.membership_proof(i) for i in range(n)]
    got = AC.plan_shapes(o, n)
    for i in range(n):
        assert got[i] == (len(want[i].auth_path_aocl),) + AC.shape_of(want[i].target_chunks), i
    assert any(len(g[1]) >= 3 for g in got) and any(len(g[1]) == 0 for g in got)
    assert all(g[1] == sorted(set(g[1])) for g in got)  # strictly ascending keys
    assert totals == (int(o["aocl_path_off"][-1]), int(o["entry_off"][-1]), int(o["path_off"][-1]), int(o["rel_off"][-1]))
    assert not o["aocl_path"].any() and not o["path"].any() and not o["rel"].any()  # the plan hashes and copies nothing


def test_removal_record_form(cases, lengths):
    import neptune_hip.mutator_set as MS
    arch = cases.arch
    leafs = cases.live[::9] + cases.removed[:3]
    sets = [AC.lib_index_set(arch.index_set(i)) for i in leafs]
    _, o = MS.restore_plan(600, lengths, sets, [None] * len(leafs))
    assert not o["status"].any()
    for g, i in zip(AC.plan_shapes(o, len(leafs)), leafs):
        assert g == (0,) + AC.shape_of(arch.removal_record(i).target_chunks), i
    # both forms in one call, interleaved
    mixed = [i if k % 2 else None for k, i in enumerate(leafs)]
    _, o2 = MS.restore_plan(600, lengths, sets, mixed)
    for g, i, l in zip(AC.plan_shapes(o2, len(leafs)), leafs, mixed):
        assert g[0] == (0 if l is None else len(arch.membership_proof(i).auth_path_aocl)) and g[1:] == \
            AC.shape_of(arch.removal_record(i).target_chunks)


def test_statuses_at_the_edges(cases, lengths):
    import neptune_hip.mutator_set as MS
    from neptune_hip.mast import AbsoluteIndexSet
    arch = cases.arch
    b = cases.msa.batch_index
    good = AC.lib_index_set(arch.index_set(cases.live[0]))
    saturating = AbsoluteIndexSet((1 << 128) - 5, list(good.distances))
    assert max(good.distances) >= 5
    at_255 = AbsoluteIndexSet((b + 255) * R.CHUNK_SIZE, [0] * 44 + [R.CHUNK_SIZE - 1])
    at_256 = AbsoluteIndexSet((b + 255) * R.CHUNK_SIZE, [0] * 44 + [R.CHUNK_SIZE])
    sets = [good, good, good, saturating, at_255, at_256, saturating, good]
    leafs = [599, 600, 601, 3, None, None, 600, cases.live[0]]
    _, o = MS.restore_plan(600, lengths, sets, leafs)
    assert [int(x) for x in o["status"]] == [R.OK, R.NOT_IN_AOCL, R.NOT_IN_AOCL, R.OUT_OF_RANGE, R.OK, R.OUT_OF_RANGE,
                                             R.NOT_IN_AOCL, R.OK]  # NOT_IN_AOCL comes first
    shapes = AC.plan_shapes(o, len(sets))
    for k, st in enumerate(o["status"]):
        if st != R.OK:
            assert shapes[k] == (0, [], [], []), k  # no digest and no entry
    assert shapes[4] == (0, [], [], [])  # inside the window: nothing inactive
    assert shapes[7] == (len(arch.membership_proof(cases.live[0]).auth_path_aocl),) + \
        AC.shape_of(arch.membership_proof(cases.live[0]).target_chunks)
    # an empty archive: whatever is asked is not in the AOCL
    _, o = MS.restore_plan(0, [], [good, good], [0, None])
    assert [int(x) for x in o["status"]] == [R.NOT_IN_AOCL] * 2 and AC.plan_shapes(o, 2) == [(0, [], [], [])] * 2
    # nothing asked
    totals, o = MS.restore_plan(600, lengths, [], [])
    assert totals == (0, 0, 0, 0) and list(o["entry_off"]) == [0]


def _raw_call(lengths, sets, leafs, cout):
    import neptune_hip._lib as L
    import neptune_hip.mutator_set as MS

    class S:
        def __init__(self, s):
            self.absolute_indices = s
    mn, dist = MS._index_arrays([S(s) for s in sets])
    li = np.asarray([AC.NONE if l is None else l for l in leafs], dtype=np.uint64)
    lens = np.asarray(lengths, dtype=np.uint64)
    return L.load().nhip_ms_archive_restore_plan(600, lens.ctypes.data, lens.size, mn.ctypes.data, dist.ctypes.data,
                                                 li.ctypes.data, len(sets), ctypes.byref(cout))


def test_two_call_sizing_and_short_capacities(cases, lengths):
    import neptune_hip._lib as L
    arch = cases.arch
    leafs = cases.live[:40]
    sets = [AC.lib_index_set(arch.index_set(i)) for i in leafs]
    count = L.MsUpdated()
    assert _raw_call(lengths, sets, leafs, count) == L.NHIP_OK
    A, E, PD, RW = (int(getattr(count, f)) for f in ("aocl_digests", "entries", "path_digests", "rel_words"))
    assert A and E and PD and RW
    for short in range(4):
        caps = [A, E, PD, RW]
        caps[short] -= 1
        arrays = [np.full(k, 0xAB, dtype=dt) for k, dt in
                  ((40, np.uint8), (41, np.uint64), (5 * A, np.uint64), (41, np.uint64), (E, np.uint64), (E + 1, np.uint64),
                   (5 * PD, np.uint64), (E + 1, np.uint64), (RW, np.uint32))]
        before = [a.copy() for a in arrays]
        cout = L.MsUpdated(*(a.ctypes.data for a in arrays), *caps)
        assert _raw_call(lengths, sets, leafs, cout) == L.NHIP_ERR_ARG, short
        assert all((a == b).all() for a, b in zip(arrays, before)), short  # outputs untouched
        assert (cout.aocl_digests, cout.entries, cout.path_digests, cout.rel_words) == (0, 0, 0, 0)
    # a fill without an offset array is a shape error too
    cout = L.MsUpdated(status=np.zeros(40, dtype=np.uint8).ctypes.data, chunk_index=np.zeros(E, dtype=np.uint64).ctypes.data,
                       aocl_cap=A, entries_cap=E, path_cap=PD, rel_cap=RW)
    assert _raw_call(lengths, sets, leafs, cout) == L.NHIP_ERR_ARG
    # the chunk table has to be the batch index long
    assert _raw_call(lengths[:-1], sets, leafs, L.MsUpdated()) == L.NHIP_ERR_ARG
    assert _raw_call(lengths + [0], sets, leafs, L.MsUpdated()) == L.NHIP_ERR_ARG


def test_aocl_range_restates_the_reference():
    """`AbsoluteIndexSet::aocl_range` (absolute_index_set.rs:174-220) on its own edge cases, and: an item's own leaf
    index lies in the range of its index set."""
    import neptune_hip.mutator_set as MS
    from neptune_hip.mast import AbsoluteIndexSet
    assert MS.aocl_range(AbsoluteIndexSet(0, [R.WINDOW_SIZE - 1] * 45)) == (0, 7)
    with pytest.raises(ValueError):
        MS.aocl_range(AbsoluteIndexSet(0, [R.WINDOW_SIZE] * 45))
    assert MS.aocl_range(AbsoluteIndexSet(R.CHUNK_SIZE, [0] * 45)) == (0, 15)
    assert MS.aocl_range(AbsoluteIndexSet(R.CHUNK_SIZE - 1, [0] * 44 + [R.WINDOW_SIZE - R.CHUNK_SIZE])) == (0, 7)
    assert MS.aocl_range(AbsoluteIndexSet(R.CHUNK_SIZE, [0] * 44 + [R.WINDOW_SIZE - 1])) == (8, 15)
    c = C.cases()
    for i in c.live[::25] + [0, 599]:
        lo, hi = MS.aocl_range(AC.lib_index_set(c.arch.index_set(i)))
        assert lo <= i <= hi and lo % 8 == 0 and hi % 8 == 7, i
