"""GPU: the archival mutator set across blocks (nhip_ms_archive_apply: k_ms_arch_chunks, k_ms_arch_chunk_digests,
k_ms_arch_ancestors and the compaction's k_ms_arch_gather around the block part of nhip_ms_apply_batch)
against `ms_ref.Archival` advanced by the same blocks and derived from scratch, never against the archive itself: the
accumulator, every leaf's path in both MMRs, every chunk word for word, block after block."""
import ctypes

import numpy as np
import pytest

import ms_apply_ref as A
import ms_archive_cases as AC
import ms_ref as R
import ms_update_cases as C
from test_gpu_ms_archive import _restore_all, _plain_proof, advance, new_archive, same_mmrs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return C.cases()


def block_args(adds, recs):
    from neptune_hip.mutator_set import MutatorSetUpdate
    return MutatorSetUpdate([C.to_record(r) for r in recs], [A.commitment(*it) for it in adds])


def same_as_model(archive, arch):
    """The whole archive against the set derived from scratch: accumulator, both MMRs node for node, every chunk."""
    from neptune_hip.mast import AbsoluteIndexSet
    leaves, chunks, window = AC.load_args(arch)
    msa = arch.msa()
    assert A.same(C.back_msa(archive.accumulator()), msa)
    counts = archive.counts()
    assert counts[:4] == (len(leaves), len(chunks), len(window), sum(len(ch) for ch in chunks))
    aocl, swbf = AC.model_mmrs(leaves, chunks)
    same_mmrs(archive, aocl, swbf)
    got = archive.restore_dictionaries([AbsoluteIndexSet(ci * R.CHUNK_SIZE, list(range(45))) for ci in range(len(chunks))])
    for ci, (st, tc) in enumerate(got):
        assert st == R.OK and AC.plain_chunks(tc) == [(ci, swbf.path(ci), chunks[ci])], ci


def apply_ok(archive, arch, adds, recs):
    """One accepted block: block_out equals the archive's accumulator afterwards and the model's; the set after."""
    job = archive.apply(C.to_msa(arch.msa()), block_args(adds, recs))
    assert job[:3] == (True, R.OK, None), job[:3]
    after = advance(arch, adds, recs)
    assert A.same(C.back_msa(job[3]), after.msa())
    assert A.same(C.back_msa(archive.accumulator()), C.back_msa(job[3]))
    return after


# ---------------------------------------------------------------- 2. block after block
def test_one_block_from_the_set_of_600(ctx, cases):
    group = [cases.adds600[3], cases.removals, cases.both, cases.born]
    assert [(len(cs.adds), len(cs.recs)) for cs in group] == [(300, 0), (0, 12), (20, 12), (300, 0)]
    for cs in group:
        with new_archive(ctx, cs.arch) as archive:
            after = apply_ok(archive, cs.arch, cs.adds, cs.recs)
            same_as_model(archive, after)


def _three_blocks(cases):
    c = cases
    arch1 = advance(c.arch, c.adds300, [])
    recs2 = [arch1.removal_record(i) for i in c.low[:6]]
    arch2 = advance(arch1, [], recs2)
    recs3 = [arch2.removal_record(i) for i in c.low[6:9]]
    return [(c.arch, c.adds300, []), (arch1, [], recs2), (arch2, c.adds20, recs3)]


def test_three_consecutive_blocks(ctx, cases):
    blocks = _three_blocks(cases)
    with new_archive(ctx, cases.arch) as archive:
        for arch, adds, recs in blocks:
            after = apply_ok(archive, arch, adds, recs)
            same_as_model(archive, after)
        # fresh witnesses at the last tip
        leafs = list(range(0, 920, 9))
        for i, (st, p) in zip(leafs, _restore_all(archive, after, leafs)):
            assert st == R.OK and _plain_proof(p) == _plain_proof(after.membership_proof(i)), i


@pytest.mark.parametrize("k", (1, 8, 9, 17))
def test_from_an_empty_archive(ctx, cases, k):
    """Genesis-style additions: 1 and 8 slide nothing, 9 slides the window once, 17 twice."""
    from neptune_hip.mutator_set import Archive
    adds = cases.adds300[:k]
    empty = R.Archival()
    assert AC.batch_index(k) == {1: 0, 8: 0, 9: 1, 17: 2}[k]
    with Archive(ctx) as archive:
        after = apply_ok(archive, empty, adds, [])
        same_as_model(archive, after)
        again = cases.adds300[20:29]
        after2 = apply_ok(archive, after, again, [after.removal_record(0)])
        same_as_model(archive, after2)


# ---------------------------------------------------------------- 3. the chunk edges
def test_chunk_edges_of_a_block(ctx, cases):
    c = cases
    arch, b0 = c.arch, c.msa.batch_index
    adds = c.adds20
    b1 = AC.batch_index(600 + len(adds))
    assert b1 > b0
    sets = {i: arch.index_set(i).to_array() for i in c.live}
    # (a) a record with an index in a chunk the same block slides out
    slid = next(i for i in c.live if any(b0 <= x // R.CHUNK_SIZE < b1 for x in sets[i]))
    # (b) two records with one absolute index below b1 in common: the word is kept twice
    owner, pair = {}, None
    for i in c.live:
        for x in sets[i]:
            if x // R.CHUNK_SIZE < b1 and x in owner and owner[x] != i:
                pair = (owner[x], i, x)
                break
            owner[x] = i
        if pair:
            break
    assert pair is not None
    # (c) a record that hits a chunk of 0 words
    empties = {ci for ci in range(b0) if not arch.bloom.get(ci)}
    bare = next(i for i in c.live if any(x // R.CHUNK_SIZE in empties for x in sets[i]))
    leafs = sorted({slid, pair[0], pair[1], bare})
    recs = [arch.removal_record(i) for i in leafs]
    with new_archive(ctx, arch) as archive:
        after = apply_ok(archive, arch, adds, recs)
        same_as_model(archive, after)
        ci, rel = pair[2] // R.CHUNK_SIZE, pair[2] % R.CHUNK_SIZE
        assert after.bloom[ci].count(rel) >= 2
        hit = next(x // R.CHUNK_SIZE for x in sets[bare] if x // R.CHUNK_SIZE in empties)
        assert after.bloom[hit] and not arch.bloom.get(hit)


def test_a_slide_of_more_than_256_chunks(ctx, cases):
    """2,100 additions on a set of 9: chunks 1 .. 262 are created, those from c - b0 = 256 on from beyond the old window
    (empty).  (`cases().tail` reaches this edge for an accumulator of 2^40 leaves, which no archive can hold.)"""
    import random
    rng = random.Random(5)
    arch, _ = cases.small_sets[9]
    adds = [tuple(tuple(rng.randrange(R.P) for _ in range(5)) for _ in range(3)) for _ in range(2100)]
    b0, b1 = arch.msa().batch_index, AC.batch_index(9 + 2100)
    assert b1 - b0 > 256 and arch.msa().swbf_active
    with new_archive(ctx, arch) as archive:
        after = apply_ok(archive, arch, adds, [])
        assert all(not after.bloom.get(ci) for ci in range(b0 + 256, b1))
        assert any(after.bloom.get(ci) for ci in range(b0, b0 + 256))
        same_as_model(archive, after)


# ---------------------------------------------------------------- 5. rejections leave no trace
def _snapshot(archive, arch):
    n, b = len(arch.items), arch.msa().batch_index
    leafs = list(range(0, n, 11))
    return (archive.counts(), C.back_msa(archive.accumulator()), archive.aocl_paths(range(n)), archive.swbf_paths(range(b)),
            [(st, _plain_proof(p)) for st, p in _restore_all(archive, arch, leafs)])


def test_rejections_leave_no_trace(ctx, cases):
    c = cases
    arch, msa = c.arch, c.msa
    with new_archive(ctx, arch) as archive:
        before = _snapshot(archive, arch)
        for cs in c.rejected_jobs:  # 2.b, 2.c, 2.d
            job = archive.apply(C.to_msa(msa), block_args(cs.adds, cs.recs))
            want = cs.want[0]
            assert job[:3] == want[:3] and job[1] != R.OK and job[3] is None, cs.label
            assert _snapshot(archive, arch) == before, cs.label
        assert [cs.want[0][1] for cs in c.rejected_jobs] == [R.ALREADY_REMOVED, A.DUPLICATE_RECORD, A.UPDATE_IMPOSSIBLE]
        # 2.e: an expected accumulator that is not the one after
        job = archive.apply(C.to_msa(msa), block_args(c.adds20, c.twelve[:2]), expected=C.to_msa(msa))
        assert job[:2] == (False, A.UPDATE_MISMATCH)
        assert _snapshot(archive, arch) == before
        # an msa_before that is not the archive's: one peak, one window word, a count, each in turn
        def edited(f):
            m = C.back_msa(C.to_msa(msa))
            f(m)
            return C.to_msa(m)
        wrong = {
            "an AOCL peak": edited(lambda m: m.aocl.peaks.__setitem__(1, C.flip(m.aocl.peaks[1]))),
            "an SWBF peak": edited(lambda m: m.swbf_inactive.peaks.__setitem__(0, C.flip(m.swbf_inactive.peaks[0]))),
            "a window word": edited(lambda m: m.swbf_active.__setitem__(3, m.swbf_active[3] ^ 1)),
            "a window word fewer": edited(lambda m: m.swbf_active.pop()),
        }
        assert len(msa.aocl.peaks) >= 2 and len(msa.swbf_active) > 4
        for label, given in wrong.items():
            job = archive.apply(given, block_args(c.adds20, c.twelve[:2]))
            assert job == (False, A.INCONSISTENT, None, None), label
            assert _snapshot(archive, arch) == before, label
        # the leaf count of another set (a self-consistent accumulator, not this archive's)
        other = c.arch601.msa()
        job = archive.apply(C.to_msa(other), block_args(c.adds20, []))
        assert job == (False, A.INCONSISTENT, None, None)
        assert _snapshot(archive, arch) == before
        # and the archive still takes the block it should
        after = apply_ok(archive, arch, c.adds20, c.twelve[:2])
        same_as_model(archive, after)


# ---------------------------------------------------------------- 6. growth and compaction
def test_growth_and_compaction(ctx, cases):
    from neptune_hip.mutator_set import Archive
    c = cases
    small, _ = c.small_sets[9]

    def run(initial):
        dead_seen, compacted, arch = [], 0, small
        with Archive(ctx, initial) as archive:
            archive.load(*AC.load_args(small))
            blocks = [(c.adds300[:150], []), (c.adds300[150:], [])] + \
                [(c.adds300[7 * k:7 * k + 2] if k % 2 else [], None) for k in range(8)]
            removed = set()
            for k, (adds, recs) in enumerate(blocks):
                if recs is None:  # eight removals of early items: they hit the low chunks again and again
                    pick = [i for i in range(8 * k, 8 * k + 40) if i not in removed][:8]
                    removed |= set(pick)
                    recs = [arch.removal_record(i) for i in pick]
                    assert len(recs) == 8
                live0, dead0 = archive.counts()[3:]
                arch = apply_ok(archive, arch, adds, recs)
                live1, dead1 = archive.counts()[3:]
                assert live1 == sum(len(v) for ci, v in arch.bloom.items() if ci < arch.msa().batch_index)
                compacted += dead0 > 0 and dead1 == 0
                dead_seen.append(dead1)
                assert dead1 <= live1  # compaction runs as soon as dead words exceed live words
            same_as_model(archive, arch)
            final = (archive.counts()[:4], C.back_msa(archive.accumulator()),
                     archive.aocl_paths(range(len(arch.items))), archive.swbf_paths(range(arch.msa().batch_index)))
        return final, dead_seen, compacted, arch

    tight, dead_seen, compacted, arch = run(dict(aocl_leafs=1, chunks=1, rel_words=1))
    # the set of 9 loads into level arrays of 16 and 1 slots, a table of one chunk and an arena of its words: 317 leaves,
    # 39 chunks and their words force every array to grow, more than once
    assert len(arch.items) == 9 + 300 + 8 and arch.msa().batch_index > 32
    assert any(dead_seen) and compacted >= 2, (dead_seen, compacted)
    roomy, _, _, _ = run(dict(aocl_leafs=4096, chunks=1024, rel_words=1 << 16))
    assert tight == roomy


# ---------------------------------------------------------------- 7. arguments
def test_apply_arguments(ctx, cases):
    import neptune_hip._lib as L
    from neptune_hip.mutator_set import PackedApply
    c = cases
    with new_archive(ctx, c.arch) as archive:
        counts = archive.counts()
        two = PackedApply([(C.to_msa(c.msa), block_args(c.adds20[:1], []))] * 2)
        assert ctx.lib.nhip_ms_archive_apply(archive._h, ctypes.byref(two.cin), ctypes.byref(two.cout)) == L.NHIP_ERR_ARG
        none = PackedApply([])
        assert ctx.lib.nhip_ms_archive_apply(archive._h, ctypes.byref(none.cin), ctypes.byref(none.cout)) == L.NHIP_ERR_ARG
        one = PackedApply([(C.to_msa(c.msa), block_args(c.adds20[:1], []))])
        assert ctx.lib.nhip_ms_archive_apply(None, ctypes.byref(one.cin), ctypes.byref(one.cout)) == L.NHIP_ERR_ARG
        assert ctx.lib.nhip_ms_archive_apply(archive._h, None, ctypes.byref(one.cout)) == L.NHIP_ERR_ARG
        assert ctx.lib.nhip_ms_archive_apply(archive._h, ctypes.byref(one.cin), None) == L.NHIP_ERR_ARG
        assert archive.counts() == counts and not np.asarray(two.arrays["status"]).any()
