"""GPU: the restore plan decided on the device (nhip_ms_archive_restore_shape: k_ms_rst_keys, k_ms_rst_scan_*,
k_ms_rst_entries) against the host plan (`restore_plan`, nhip_ms_archive_restore_plan), array for array
and total for total.  The index sets are built by hand (tests/ms_restore_cases.py); each test asserts that its data
reaches what it claims.  The witness counts straddle the kernels' geometry, which the header names."""
import numpy as np
import pytest

import ms_archive_cases as AC
import ms_ref as R
import ms_restore_cases as RC
import ms_update_cases as C

pytestmark = pytest.mark.gpu

T = AC.TAIL_NODES
FIELDS = ("status", "aocl_path_off", "entry_off", "chunk_index", "path_off", "rel_off")


@pytest.fixture(scope="module")
def cases():
    return C.cases()


@pytest.fixture(scope="module")
def archives(ctx, cases):
    """`{n_leafs: (archive, chunk lengths)}`, loaded once and only read"""
    from neptune_hip.mutator_set import Archive
    out = {}
    for n in (0, 1, 9, 600, 4 * T + 3):
        leaves, chunks, window = AC.load_args(cases.arch) if n == 600 else AC.random_archive(n, 4400 + n)
        if n == 600 and not chunks[0]:  # the set of 600 leaves its first chunk empty: both end chunks hold words here
            chunks[0] = [5, 77, 4000]
        a = Archive(ctx)
        if n:
            a.load(leaves, chunks, window)
        out[n] = (a, [len(ch) for ch in chunks])
    yield out
    for a, _ in out.values():
        a.close()


def same_as_the_host_plan(archive, n_leafs, lengths, witnesses):
    from neptune_hip.mutator_set import restore_plan
    sets, leafs = RC.as_args(witnesses)
    want_totals, want = restore_plan(n_leafs, lengths, sets, leafs)
    got_totals, got = archive.restore_shape(sets, leafs)
    assert got_totals == want_totals
    for f in FIELDS:
        assert got[f].shape == want[f].shape and (got[f] == want[f]).all(), (f, len(witnesses))
    assert not got["aocl_path"].any() and not got["path"].any() and not got["rel"].any()  # left alone
    return want_totals, want


def test_every_edge_is_reached_and_decided_as_the_host_plan_decides_it(archives):
    archive, lengths = archives[600]
    b = 74
    assert len(lengths) == b and lengths[0] and lengths[b - 1] and 0 in lengths
    empty = lengths.index(0)
    edges = RC.edge_sets(600) + [("the empty chunk", empty * R.CHUNK_SIZE, list(range(45)), None)]
    _, o = same_as_the_host_plan(archive, 600, lengths, edges)
    shapes = dict(zip((e[0] for e in edges), zip((int(x) for x in o["status"]), AC.plan_shapes(o, len(edges)))))
    keys = lambda label: shapes[label][1][1]  # noqa: E731
    ok = lambda label: shapes[label][0] == R.OK  # noqa: E731
    assert ok("one chunk, key 0") and keys("one chunk, key 0") == [0]
    assert ok("key b - 1 alone") and keys("key b - 1 alone") == [b - 1]
    assert ok("45 distinct chunks") and keys("45 distinct chunks") == list(range(45))
    assert ok("all at or above b") and keys("all at or above b") == []
    assert ok("straddles b") and keys("straddles b") == [b - 2, b - 1]
    assert ok("keys 0 and b - 1") and keys("keys 0 and b - 1") == [0, b - 1]
    assert ok("a, c, a, c") and keys("a, c, a, c") == [0, 3]
    assert ok("descending") and keys("descending") == list(range(45))
    assert ok("chunk b + 255") and keys("chunk b + 255") == []
    assert ok("the last index of chunk b + 255")
    for label in ("chunk b + 256", "one past chunk b + 255", "the carry into the high word", "the wrap", "a high word"):
        assert shapes[label] == (R.OUT_OF_RANGE, (0, [], [], [])), label
    for label in ("leaf index n", "leaf index 2^64 - 2", "past the AOCL and saturating"):
        assert shapes[label] == (R.NOT_IN_AOCL, (0, [], [], [])), label
    assert ok("leaf index 0") and shapes["leaf index 0"][1][0] == (0 ^ 600).bit_length() - 1
    assert ok("leaf index n - 1") and shapes["leaf index n - 1"][1][0] == (599 ^ 600).bit_length() - 1
    assert ok("no leaf index") and shapes["no leaf index"][1][0] == 0
    # path lengths and word counts of the entries: from the table, with an empty chunk among them
    lens = shapes["45 distinct chunks"][1]
    assert lens[2] == [(k ^ b).bit_length() - 1 for k in range(45)] and lens[3] == lengths[:45] and any(lens[3])
    assert shapes["the empty chunk"] == (R.OK, (0, [empty], [(empty ^ b).bit_length() - 1], [0]))


@pytest.mark.parametrize("n_leafs", (0, 1, 9, 4 * T + 3))
def test_other_archives(archives, n_leafs):
    archive, lengths = archives[n_leafs]
    edges = RC.edge_sets(n_leafs)
    for count in (1, 2, len(edges), 257):
        totals, o = same_as_the_host_plan(archive, n_leafs, lengths, RC.cycled(edges, count, start=count % 5))
        if n_leafs == 0:  # the empty archive: nobody is in the AOCL, nothing is owned
            assert totals == (0, 0, 0, 0) and (o["status"] == R.NOT_IN_AOCL).all()
        elif count >= len(edges):
            assert {R.OK, R.OUT_OF_RANGE, R.NOT_IN_AOCL} == {int(x) for x in o["status"]}
            assert (n_leafs <= 9) == (totals[1] <= count)  # at most one chunk below b, or many
    if n_leafs == 4 * T + 3:
        assert totals[1] > 257 and totals[3] > 0


def _counts():
    import neptune_hip._lib as L
    W, S = L.MS_RESTORE_WAVES, L.MS_RESTORE_SCAN_WIDTH
    return sorted({1, 2, W - 1, W, W + 1, 2 * W + 1, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 4 * S + 3})


def test_witness_counts_straddle_the_kernels_geometry(archives):
    import neptune_hip._lib as L
    archive, lengths = archives[600]
    edges = RC.edge_sets(600)
    W, S = L.MS_RESTORE_WAVES, L.MS_RESTORE_SCAN_WIDTH
    counts = _counts()
    for edge in (W, S, 2 * S):  # the waves of a workgroup, a scan tile, the carry into the second and the third tile
        assert {edge - 1, edge, edge + 1} <= set(counts)
    for count in counts:
        same_as_the_host_plan(archive, 600, lengths, RC.cycled(edges, count, start=count % 7))


def test_entry_counts_straddle_the_scan_tile_and_the_carry_segment(archives):
    """The entries are scanned by the same kernels over a count that lives on the device: entry counts one below, at
    and one past a tile, and one below, at and one past what the carry wave takes with one tile a lane (past it a
    lane carries a segment of tiles), reached with 45-key witnesses and topped up with one-key witnesses."""
    import neptune_hip._lib as L
    archive, lengths = archives[600]
    edges = RC.edge_sets(600)
    full = next(e for e in edges if e[0] == "45 distinct chunks")
    one = next(e for e in edges if e[0] == "one chunk, key 0")
    bad = next(e for e in edges if e[0] == "the wrap")
    S, lanes = L.MS_RESTORE_SCAN_WIDTH, L.MS_RESTORE_CARRY_LANES
    for target in (S - 1, S, S + 1, S * lanes - 1, S * lanes, S * lanes + 1, 2 * S * lanes + 1):
        witnesses = []
        for k in range(target // 45):
            witnesses += [full, bad] if k % 3 == 0 else [full]
        witnesses += [one] * (target % 45)
        assert len(witnesses) < 5000
        totals, _ = same_as_the_host_plan(archive, 600, lengths, witnesses)
        assert totals[1] == target
