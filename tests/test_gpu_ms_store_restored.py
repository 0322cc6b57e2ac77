"""GPU: restored witnesses handed to a store device to device (nhip_ms_store_append_restored: the shape kernels,
k_ms_arch_gather_own, k_ms_rst_hand) against the two-call path it replaces (`Archive` restore, then
`WitnessStore.append`), against `restore_plan`, and against `ms_ref`, which derives everything from scratch: never
against the new call itself.  The sets come from tests/ms_update_cases.py and tests/ms_archive_cases.py, built once
and left unchanged; each test asserts that its data reaches what it claims."""
import copy
import ctypes

import numpy as np
import pytest

import ms_apply_ref as A
import ms_archive_cases as AC
import ms_ref as R
import ms_update_cases as C

pytestmark = pytest.mark.gpu

UNIT = 1024  # MS_ARCHIVE_GATHER_UNIT: 8-byte destination words per work unit of the gather (2 UNIT chunk words)


@pytest.fixture(scope="module")
def cases():
    return C.cases()


def advance(arch, adds, recs):
    a = A.clone(arch)
    for it in adds:
        a.add(*it)
    for r in copy.deepcopy(list(recs)):
        a.remove(r)
    return a


@pytest.fixture(scope="module")
def blocks(cases):
    """The set of 900 after two blocks, what is gone from it, the third block and the set after it (as
    tests/test_gpu_ms_archive.py builds them)."""
    c = cases
    arch1 = advance(c.arch, c.adds300, [])
    arch2 = advance(arch1, [], [arch1.removal_record(i) for i in c.low[:6]])
    adds3 = c.adds20
    recs3 = [arch2.removal_record(i) for i in c.low[6:9]]
    return arch2, c.removed + c.low[:6], adds3, recs3, advance(arch2, adds3, recs3)


def new_archive(ctx, arch):
    from neptune_hip.mutator_set import Archive
    a = Archive(ctx)
    a.load(*AC.load_args(arch))
    return a


def tuples(path):
    return [tuple(int(x) for x in d) for d in path]


def plain(read):
    """`WitnessStore.read`'s result, field by field, in plain integers"""
    return [(int(st), int(w.absolute_indices.minimum), [int(d) for d in w.absolute_indices.distances], w.aocl_leaf_index,
             tuple(int(x) for x in w.aocl_leaf), tuples(w.auth_path_aocl), AC.plain_chunks(w.target_chunks)) for st, w in read]


def wanted(arch, leafs):
    """`(index sets, leaf indices)`: the membership proof of every leaf in `leafs`; a `(leaf, None)` pair asks for
    that leaf's dictionary alone"""
    sets = [AC.lib_index_set(arch.index_set(l[0] if isinstance(l, tuple) else l)) for l in leafs]
    return sets, [None if isinstance(l, tuple) else l for l in leafs]


def host_append(store, archive, sets, leafs, leaves):
    """The two-call path: restore to the host, append from the host.  `leaves[i]`: the commitment of witness i."""
    from neptune_hip.mutator_set import Witness
    status, paths, dictionaries = archive._restore(sets, leafs)
    assert status == [R.OK] * len(sets)
    store.append([Witness(s, dictionaries[i], l, () if l is None else list(leaves[i]), paths[i])
                  for i, (s, l) in enumerate(zip(sets, leafs))])


def own_leaves(arch, leafs):
    return [None if l is None else R.aocl_leaf(*arch.items[l]) for l in leafs]


def same_stores(a, b):
    assert a.counts() == b.counts()
    ra, rb = plain(a.read()), plain(b.read())
    assert len(ra) == len(rb) == len(a) == len(b)
    for k, (x, y) in enumerate(zip(ra, rb)):
        assert x == y, k
    return rb


# ---------------------------------------------------------------- 1, 2. equal to the two-call path; the mirror is right
def test_equal_to_the_two_call_path_and_across_a_block_and_back(ctx, blocks):
    from neptune_hip.mutator_set import MutatorSetUpdate, WitnessStore
    arch2, gone, adds3, recs3, arch3 = blocks
    proofs = [i for i in range(0, 900, 6) if i not in gone]
    asked = proofs + [(i, None) for i in proofs[:10]]
    sets, leafs = wanted(arch2, asked)
    assert len(proofs) > 100 and len(arch2.items) == 900
    with new_archive(ctx, arch2) as archive, WitnessStore(ctx) as sa, WitnessStore(ctx) as sb:
        host_append(sa, archive, sets, leafs, own_leaves(arch2, leafs))
        assert sb.append_restored(archive, sets, leafs) == [R.OK] * len(sets)
        got = same_stores(sa, sb)
        acc = archive.accumulator()
        assert sa.check(acc) == sb.check(acc) == [(True, True, True, R.OK)] * len(sets)
        # ... and both are what ms_ref derives from scratch, so they cannot agree on something wrong
        for k, (l, w) in enumerate(zip(asked, got)):
            if k < len(proofs):
                p = arch2.membership_proof(l)
                assert (w[3], w[4], w[5]) == (l, tuple(R.aocl_leaf(*arch2.items[l])), tuples(p.auth_path_aocl)), l
                assert w[6] == AC.plain_chunks(p.target_chunks), l
            else:
                assert (w[3], w[4], w[5]) == (None, (), []) and w[6] == AC.plain_chunks(arch2.removal_record(l[0]).target_chunks)
        assert any(len(w[6]) >= 3 for w in got) and any(not w[6] for w in got)
        # ---- the mirror: both cross block 3, equal a fresh restore behind it, come back, are thinned and read
        update = MutatorSetUpdate([C.to_record(r) for r in recs3], [A.commitment(*it) for it in adds3])
        (ja, wa), (jb, wb) = sa.update(acc, update), sb.update(acc, update)
        assert ja[1] == jb[1] == R.OK and wa == wb == [R.OK] * len(sets)
        assert A.same(C.back_msa(jb[3]), arch3.msa())
        crossed = same_stores(sa, sb)
        with new_archive(ctx, arch3) as after, WitnessStore(ctx) as fresh:
            host_append(fresh, after, *wanted(arch3, asked), own_leaves(arch3, leafs))
            assert plain(fresh.read()) == crossed
        assert crossed != got
        (ja, wa), (jb, wb) = sa.revert(acc, update), sb.revert(acc, update)
        assert ja[1] == jb[1] == R.OK and wa == wb == [R.OK] * len(sets)
        assert same_stores(sa, sb) == got
        keep = [k % 2 == 0 for k in range(len(sets))]
        sa.retain(keep), sb.retain(keep)
        assert same_stores(sa, sb) == got[::2]
        chosen = [5, 0, len(sb) - 1, 5]
        assert plain(sa.read(chosen)) == plain(sb.read(chosen)) == [got[::2][k] for k in chosen]


# ---------------------------------------------------------------- 3. behind existing witnesses, and growth
def test_behind_existing_witnesses_from_capacities_of_one(ctx, blocks):
    from neptune_hip.mutator_set import WitnessStore
    arch2 = blocks[0]
    one = dict(witnesses=1, aocl_digests=1, entries=1, path_digests=1, rel_words=1)
    order = list(range(899, -1, -1))
    steps = [order[:1], order[1:66], [(l, None) if k % 9 == 0 else l for k, l in enumerate(order[66:366])]]
    ordinary, last = order[366:400], order[400:470] + [(3, None)]
    assert [len(s) for s in steps] == [1, 65, 300]
    with new_archive(ctx, arch2) as archive, WitnessStore(ctx, one) as sa, WitnessStore(ctx, one) as sb:
        odd = False
        for step in steps + [ordinary, last]:
            sets, leafs = wanted(arch2, step)
            host_append(sa, archive, sets, leafs, own_leaves(arch2, leafs))
            if step is ordinary:
                host_append(sb, archive, sets, leafs, own_leaves(arch2, leafs))
            else:
                odd |= sb.counts()[4] % 2 == 1  # the chunk words' pool begins on an odd word
                assert sb.append_restored(archive, sets, leafs) == [R.OK] * len(sets)
            same_stores(sa, sb)
        assert odd and len(sb) == 1 + 65 + 300 + len(ordinary) + len(last)
        acc = archive.accumulator()
        assert sa.check(acc) == sb.check(acc) and all(c[0] for c in sb.check(acc))


# ---------------------------------------------------------------- 4. the leaves
def test_the_callers_commitments_and_the_archives_own(ctx, blocks):
    from neptune_hip.mutator_set import WitnessStore
    arch2, gone = blocks[0], blocks[1]
    live = [i for i in range(0, 900, 31) if i not in gone]
    sets, leafs = wanted(arch2, live + [(live[0], None)])
    leaves = own_leaves(arch2, leafs)
    wrong = 7
    leaves[wrong] = tuple((x + 1) % R.P for x in leaves[wrong])
    assert len(live) > wrong + 2
    with new_archive(ctx, arch2) as archive, WitnessStore(ctx) as sa, WitnessStore(ctx) as sb, WitnessStore(ctx) as sc:
        acc = archive.accumulator()
        host_append(sa, archive, sets, leafs, leaves)
        assert sb.append_restored(archive, sets, leafs, leaves) == [R.OK] * len(sets)
        same_stores(sa, sb)
        assert sa.check(acc) == sb.check(acc)
        assert [k for k, c in enumerate(sb.check(acc)) if not c[0]] == [wrong]
        # None: the device stores the archive's own leaf, which every check then hashes from
        assert sc.append_restored(archive, sets, leafs) == [R.OK] * len(sets)
        assert all(c == (True, True, True, R.OK) for c in sc.check(acc))
        for (_, w), l in zip(sc.read(), leafs):
            assert tuple(w.aocl_leaf) == (() if l is None else tuple(int(x) for x in archive.leaves(0, l, 1)[0]))
            assert l is None or tuple(w.aocl_leaf) == tuple(R.aocl_leaf(*arch2.items[l]))


# ---------------------------------------------------------------- 5. all or nothing
def test_all_or_nothing_and_arguments(ctx, blocks):
    import neptune_hip as nh
    import neptune_hip._lib as L
    from neptune_hip.mast import AbsoluteIndexSet
    from neptune_hip.mutator_set import Archive, WitnessStore, restore_plan
    arch2 = blocks[0]
    sets, leafs = wanted(arch2, [10, 20, 30, (40, None), 50])
    bad_sets = sets[:2] + [sets[2]] + sets[2:4] + [AbsoluteIndexSet((1 << 128) - 5, [9] * 45)] + sets[4:]
    bad_leafs = leafs[:2] + [900] + leafs[2:4] + [7] + leafs[4:]
    lengths = [len(ch) for ch in AC.load_args(arch2)[1]]
    want = [int(x) for x in restore_plan(900, lengths, bad_sets, bad_leafs)[1]["status"]]
    assert want == [R.OK, R.OK, R.NOT_IN_AOCL, R.OK, R.OK, R.OUT_OF_RANGE, R.OK]
    with new_archive(ctx, arch2) as archive, WitnessStore(ctx) as sa, WitnessStore(ctx) as sb:
        first, first_leafs = wanted(arch2, [1, 2])
        for s in (sa, sb):
            host_append(s, archive, first, first_leafs, own_leaves(arch2, first_leafs))
        before = (sb.counts(), plain(sb.read()))
        assert sb.append_restored(archive, bad_sets, bad_leafs) == want
        assert (sb.counts(), plain(sb.read())) == before and len(sb) == 2
        host_append(sa, archive, sets, leafs, own_leaves(arch2, leafs))
        assert sb.append_restored(archive, sets, leafs) == [R.OK] * 5
        after = same_stores(sa, sb)
        # n == 0 changes nothing
        assert sb.append_restored(archive, [], []) == []
        assert ctx.lib.nhip_ms_store_append_restored(sb._h, archive._h, None, None, None, None, 0, None) == L.NHIP_OK
        assert plain(sb.read()) == after
        # an archive of another context
        with nh.Context(0) as other, Archive(other) as foreign:
            foreign.load(*AC.random_archive(9, 5))
            mn = np.zeros((1, 2), dtype=np.uint64)
            dist = np.zeros((1, 45), dtype=np.uint32)
            li = np.zeros(1, dtype=np.uint64)
            st = np.full(1, 0xAB, dtype=np.uint8)
            assert ctx.lib.nhip_ms_store_append_restored(sb._h, foreign._h, mn.ctypes.data, dist.ctypes.data, li.ctypes.data,
                                                         None, 1, st.ctypes.data) == L.NHIP_ERR_ARG
            assert st[0] == 0xAB
        assert sb.counts() == sa.counts() and plain(sb.read()) == after


# ---------------------------------------------------------------- 6. the gather's edges
def test_gather_edges_word_for_word(ctx):
    import random
    from neptune_hip.mast import AbsoluteIndexSet
    from neptune_hip.mutator_set import Archive, WitnessStore
    leaves, chunks, window = AC.random_archive(100, 6100)
    rng = random.Random(61)
    long_, exact, empty, odd = 2, 5, 7, 9
    chunks[long_] = sorted(rng.randrange(R.CHUNK_SIZE) for _ in range(4100))
    chunks[exact] = sorted(rng.randrange(R.CHUNK_SIZE) for _ in range(2 * UNIT))
    chunks[empty] = []
    chunks[odd] = sorted(rng.randrange(R.CHUNK_SIZE) for _ in range(5))
    assert len(chunks) == 12 and len(set(chunks[long_])) < 4100 and len(chunks[long_]) > 2 * 2 * UNIT  # an owner past two units
    inside = lambda ci: AbsoluteIndexSet(ci * R.CHUNK_SIZE, list(range(45)))  # noqa: E731
    first = [inside(odd)]
    second = [inside(long_), inside(empty), inside(exact), AbsoluteIndexSet(long_ * R.CHUNK_SIZE, [t % 2 * 3 * R.CHUNK_SIZE for t in range(45)]),
              inside(empty), inside(long_)]
    swbf = AC.model_mmrs(leaves, chunks)[1]
    with Archive(ctx) as archive, WitnessStore(ctx) as sa, WitnessStore(ctx) as sb:
        archive.load(leaves, chunks, window)
        for sets in (first, second):
            none = [None] * len(sets)
            host_append(sa, archive, sets, none, none)
            assert sb.counts()[4] == (0 if sets is first else 5)  # the second gather begins on an odd word
            assert sb.append_restored(archive, sets, none) == [R.OK] * len(sets)
        got = same_stores(sa, sb)
        _, aocl_digests, entries, path_digests, rel_words = sb.counts()
        assert aocl_digests == 0 and 0 < 5 * path_digests < UNIT          # a pool below one unit
        assert rel_words - 5 >= 3 * 2 * UNIT                               # ... and one across three and more
        keys = [[odd], [long_], [empty], [exact], [long_, exact], [empty], [long_]]
        for w, ks in zip(got, keys):
            assert w[6] == [(ci, swbf.path(ci), list(chunks[ci])) for ci in ks]
