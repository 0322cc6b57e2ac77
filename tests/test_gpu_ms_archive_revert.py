"""GPU: the archival mutator set back across blocks (nhip_ms_archive_revert: the block part's tip check, then
k_ms_arch_unmerge, k_ms_arch_chunk_digests, k_ms_arch_ancestors, the window and the closing peak check)
against `ms_ref.Archival` derived from scratch (`arch` before the block, `advance(arch, adds, recs)` after), never
against the archive itself.  "Equal to the model" is tests/test_gpu_ms_archive_apply.py's `same_as_model`: the
accumulator, every leaf's path in both MMRs, every chunk word for word, the counts.  The blocks are those of
tests/ms_archive_revert_cases.py, which tests/test_ms_archive_revert_ref.py holds to the reference's record-by-record
way back; each test asserts that its data reaches what it claims."""
import ctypes

import numpy as np
import pytest

import ms_apply_ref as A
import ms_archive_cases as AC
import ms_archive_revert_cases as RC
import ms_ref as R
import ms_update_cases as C
from test_gpu_ms_archive import _plain_proof, _restore_all, _two_blocks, new_archive, tuples
from test_gpu_ms_archive_apply import _snapshot, apply_ok, block_args, same_as_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return C.cases()


def revert_ok(archive, arch, adds, recs, expected=None):
    """One block taken back: block_out is the tip the block leads to, the archive's accumulator is the set before's."""
    job = archive.revert(C.to_msa(arch.msa()), block_args(adds, recs), expected=expected)
    assert job[:3] == (True, R.OK, None), job[:3]
    assert A.same(C.back_msa(job[3]), RC.advance(arch, adds, recs).msa())
    assert A.same(C.back_msa(archive.accumulator()), arch.msa())


def restores_as(archive, arch, step=37):
    leafs = list(range(0, len(arch.items), step))
    for i, (st, p) in zip(leafs, _restore_all(archive, arch, leafs)):
        assert st == R.OK and _plain_proof(p) == _plain_proof(arch.membership_proof(i)), i


# ---------------------------------------------------------------- 1. one block forward and back
@pytest.mark.parametrize("which", range(4))
def test_apply_then_revert(ctx, cases, which):
    arch, adds, recs = RC.one_block_group(cases)[which]
    with new_archive(ctx, arch) as archive:
        apply_ok(archive, arch, adds, recs)
        revert_ok(archive, arch, adds, recs)
        same_as_model(archive, arch)
        restores_as(archive, arch)


@pytest.mark.parametrize("which", range(4))
def test_load_then_revert(ctx, cases, which):
    """The archive loaded at the set after the block: other arena offsets than an apply leaves, and no dead words."""
    arch, adds, recs = RC.one_block_group(cases)[which]
    after = RC.advance(arch, adds, recs)
    with new_archive(ctx, after) as archive:
        assert archive.counts()[4] == 0
        revert_ok(archive, arch, adds, recs)
        same_as_model(archive, arch)
        restores_as(archive, arch)


def test_forward_three_back_three_and_the_other_fork(ctx, cases):
    blocks = RC.three_blocks(cases)
    with new_archive(ctx, cases.arch) as archive:
        for arch, adds, recs in blocks:
            same_as_model(archive, apply_ok(archive, arch, adds, recs))
        for arch, adds, recs in reversed(blocks):
            revert_ok(archive, arch, adds, recs)
            same_as_model(archive, arch)
        # the other fork: a shorter block over slots the abandoned blocks wrote; a stale slot read would show here
        arch, adds, recs = RC.fork_block(cases)
        assert 0 < len(adds) < len(blocks[0][1]) and adds[0] != blocks[0][1][0]
        same_as_model(archive, apply_ok(archive, arch, adds, recs))
        revert_ok(archive, arch, adds, recs)
        same_as_model(archive, arch)


@pytest.mark.parametrize("k", (1, 8, 9, 17))
def test_from_an_empty_archive(ctx, cases, k):
    """1 and 8 additions slide nothing, 9 slide the window once, 17 twice; back down to nothing, and a load follows."""
    from neptune_hip.mutator_set import Archive
    adds = cases.adds300[:k]
    empty = R.Archival()
    assert AC.batch_index(k) == {1: 0, 8: 0, 9: 1, 17: 2}[k]
    with Archive(ctx) as archive:
        same_as_model(archive, apply_ok(archive, empty, adds, []))
        revert_ok(archive, empty, adds, [])
        assert archive.counts() == (0, 0, 0, 0, 0)
        small, _ = cases.small_sets[9]
        archive.load(*AC.load_args(small))
        same_as_model(archive, small)


# ---------------------------------------------------------------- 2. the chunk edges
def test_chunk_edges_of_a_revert(ctx, cases):
    from neptune_hip.mast import AbsoluteIndexSet
    arch, adds, recs, f = RC.edge_block(cases)

    def words(archive, ci):
        (st, tc), = archive.restore_dictionaries([AbsoluteIndexSet(ci * R.CHUNK_SIZE, list(range(45)))])
        assert st == R.OK
        return AC.plain_chunks(tc)[0][2]

    for loaded in (False, True):
        with new_archive(ctx, RC.advance(arch, adds, recs) if loaded else arch) as archive:
            if not loaded:
                apply_ok(archive, arch, adds, recs)
            assert archive.counts()[1] == f["b1"]
            ci, rel = f["pair"] // R.CHUNK_SIZE, f["pair"] % R.CHUNK_SIZE
            copies = words(archive, ci).count(rel)
            revert_ok(archive, arch, adds, recs)
            assert archive.counts()[1] == f["b0"] <= f["slid"]  # the chunk the block created is gone
            assert words(archive, ci).count(rel) == copies - 2 == arch.bloom.get(ci, []).count(rel)
            ci, rel = f["held"] // R.CHUNK_SIZE, f["held"] % R.CHUNK_SIZE
            assert words(archive, ci).count(rel) == arch.bloom[ci].count(rel) >= 1  # one copy stays
            assert words(archive, f["bare"]) == []
            same_as_model(archive, arch)


def test_a_slide_of_more_than_256_chunks(ctx, cases):
    arch, adds, recs = RC.long_slide(cases)
    with new_archive(ctx, arch) as archive:
        apply_ok(archive, arch, adds, recs)
        assert archive.counts()[1] - arch.msa().batch_index > 256
        revert_ok(archive, arch, adds, recs)
        same_as_model(archive, arch)


# ---------------------------------------------------------------- 3. rejections leave no trace
def test_rejections_leave_no_trace(ctx, cases):
    import neptune_hip._lib as L
    from neptune_hip.mutator_set import PackedApply
    c = cases
    arch, msa = c.arch, c.msa
    adds, recs = c.adds20, c.twelve[:2]
    tip = RC.advance(arch, adds, recs)
    with new_archive(ctx, tip) as archive:
        before = _snapshot(archive, tip)
        for cs in c.rejected_jobs:  # 2.b, 2.c, 2.d: the block part's say
            job = archive.revert(C.to_msa(msa), block_args(cs.adds, cs.recs))
            assert job[:3] == cs.want[0][:3] and job[1] != R.OK, cs.label
            assert _snapshot(archive, tip) == before, cs.label
        assert [cs.want[0][1] for cs in c.rejected_jobs] == [R.ALREADY_REMOVED, A.DUPLICATE_RECORD, A.UPDATE_IMPOSSIBLE]
        # 2.e: an expected accumulator that is not the one after the block
        job = archive.revert(C.to_msa(msa), block_args(adds, recs), expected=C.to_msa(msa))
        assert job[:2] == (False, A.UPDATE_MISMATCH)
        assert _snapshot(archive, tip) == before
        # an msa_before that is not the block's: a peak of either MMR, a window word, a count
        def edited(f):
            m = C.back_msa(C.to_msa(msa))
            f(m)
            return C.to_msa(m)
        wrong = {
            "an AOCL peak": edited(lambda m: m.aocl.peaks.__setitem__(1, C.flip(m.aocl.peaks[1]))),
            "an SWBF peak": edited(lambda m: m.swbf_inactive.peaks.__setitem__(0, C.flip(m.swbf_inactive.peaks[0]))),
            "a window word": edited(lambda m: m.swbf_active.__setitem__(3, m.swbf_active[3] ^ 1)),
            "a window word fewer": edited(lambda m: m.swbf_active.pop()),
            "the leaf count of another set": C.to_msa(c.arch601.msa()),
        }
        assert len(msa.aocl.peaks) >= 2 and len(msa.swbf_active) > 4
        for label, given in wrong.items():
            job = archive.revert(given, block_args(adds, recs))
            assert not job[0] and job[1] != R.OK, label
            assert _snapshot(archive, tip) == before, label
        # a block with one addition record changed: it leads to another tip
        other = list(adds)
        other[7] = (C.flip(other[7][0]),) + tuple(other[7][1:])
        job = archive.revert(C.to_msa(msa), block_args(other, recs))
        assert job[:3] == (False, A.UPDATE_MISMATCH, None)
        assert _snapshot(archive, tip) == before
        # ... one record fewer, too
        job = archive.revert(C.to_msa(msa), block_args(adds, recs[:1]))
        assert job[:3] == (False, A.UPDATE_MISMATCH, None)
        assert _snapshot(archive, tip) == before
        # n_jobs != 1, and absent arguments
        counts = archive.counts()
        lib = ctx.lib
        two = PackedApply([(C.to_msa(msa), block_args(adds, recs))] * 2)
        assert lib.nhip_ms_archive_revert(archive._h, ctypes.byref(two.cin), ctypes.byref(two.cout)) == L.NHIP_ERR_ARG
        none = PackedApply([])
        assert lib.nhip_ms_archive_revert(archive._h, ctypes.byref(none.cin), ctypes.byref(none.cout)) == L.NHIP_ERR_ARG
        one = PackedApply([(C.to_msa(msa), block_args(adds, recs))])
        assert lib.nhip_ms_archive_revert(None, ctypes.byref(one.cin), ctypes.byref(one.cout)) == L.NHIP_ERR_ARG
        assert lib.nhip_ms_archive_revert(archive._h, None, ctypes.byref(one.cout)) == L.NHIP_ERR_ARG
        assert lib.nhip_ms_archive_revert(archive._h, ctypes.byref(one.cin), None) == L.NHIP_ERR_ARG
        assert archive.counts() == counts and not np.asarray(two.arrays["status"]).any()
        # the right block on an archive one block further
        more = c.adds300[40:49]
        further = apply_ok(archive, tip, more, [])
        at_further = _snapshot(archive, further)
        job = archive.revert(C.to_msa(msa), block_args(adds, recs))
        assert job[:3] == (False, A.UPDATE_MISMATCH, None)
        assert _snapshot(archive, further) == at_further
        revert_ok(archive, tip, more, [])
        assert _snapshot(archive, tip)[1:] == before[1:]  # the dead words apart, as before
        # a block of nothing at the tip is a no-op
        revert_ok(archive, tip, [], [])
        assert _snapshot(archive, tip)[1:] == before[1:]
        # and the archive still takes the block it should, the tip given as msa_expected
        revert_ok(archive, arch, adds, recs, expected=C.to_msa(tip.msa()))
        same_as_model(archive, arch)


# ---------------------------------------------------------------- 4. growth and compaction
def test_growth_and_compaction(ctx, cases):
    """Ten blocks from the set of 9, each applied, taken back and applied again, then all ten taken back; from
    capacities of 1 and from generous ones.  The arena's words in use (live + dead, from `counts`) pass the loaded
    words, which with a capacity of 1 asked for are the arena's capacity: it grew."""
    from neptune_hip.mutator_set import Archive
    c = cases
    small, _ = c.small_sets[9]
    loaded_words = sum(len(ch) for ch in AC.load_args(small)[1])

    def run(initial):
        compacted, tail_max, arch, done = 0, 0, small, []
        with Archive(ctx, initial) as archive:
            archive.load(*AC.load_args(small))
            blocks = [(c.adds300[:150], []), (c.adds300[150:], [])] + \
                [(c.adds300[7 * k:7 * k + 2] if k % 2 else [], None) for k in range(8)]
            removed = set()

            def step(f, *args):
                nonlocal compacted, tail_max
                dead0 = archive.counts()[4]
                out = f(archive, *args)
                live1, dead1 = archive.counts()[3:]
                compacted += dead0 > 0 and dead1 == 0
                tail_max = max(tail_max, live1 + dead1)
                assert dead1 <= live1  # compaction runs as soon as dead words exceed live words
                return out

            for k, (adds, recs) in enumerate(blocks):
                if recs is None:  # eight removals of early items: they hit the low chunks again and again
                    pick = [i for i in range(8 * k, 8 * k + 40) if i not in removed][:8]
                    removed |= set(pick)
                    recs = [arch.removal_record(i) for i in pick]
                    assert len(recs) == 8
                step(apply_ok, arch, adds, recs)
                step(revert_ok, arch, adds, recs)
                live = archive.counts()[3]
                assert live == sum(len(v) for ci, v in arch.bloom.items() if ci < arch.msa().batch_index)
                done.append((arch, adds, recs))
                arch = step(apply_ok, arch, adds, recs)
            same_as_model(archive, arch)
            tip = (archive.counts()[:4], C.back_msa(archive.accumulator()),
                   archive.aocl_paths(range(len(arch.items))), archive.swbf_paths(range(arch.msa().batch_index)))
            for before, adds, recs in reversed(done):
                step(revert_ok, before, adds, recs)
            same_as_model(archive, small)
            final = (tip, archive.counts()[:4], archive.aocl_paths(range(9)))
        return final, compacted, tail_max, arch

    tight, compacted, tail_max, arch = run(dict(aocl_leafs=1, chunks=1, rel_words=1))
    assert len(arch.items) == 9 + 300 + 8 and arch.msa().batch_index > 32
    assert compacted >= 1 and tail_max > max(loaded_words, 1), (compacted, tail_max, loaded_words)
    roomy, _, _, _ = run(dict(aocl_leafs=4096, chunks=1024, rel_words=1 << 16))
    assert tight == roomy


# ---------------------------------------------------------------- 5. with the witness store
def test_store_and_archive_go_back_together(ctx, cases):
    """Witnesses restored at the tip and taken back by `WitnessStore.revert` over the same block equal a fresh restore
    from the reverted archive."""
    from neptune_hip.mutator_set import MutatorSetUpdate, Witness, WitnessStore
    arch2, gone, adds3, recs3, arch3 = _two_blocks(cases)
    leafs = [i for i in range(0, 900, 6) if i not in gone]
    assert len(leafs) > 100 and arch3.msa().batch_index > arch2.msa().batch_index
    with new_archive(ctx, arch3) as archive, WitnessStore(ctx) as store:
        restored = _restore_all(archive, arch3, leafs)
        assert all(st == R.OK for st, _ in restored)
        store.append([Witness(AC.lib_index_set(arch3.index_set(i)), p.target_chunks, i, list(R.aocl_leaf(*arch3.items[i])),
                              p.auth_path_aocl) for i, (_, p) in zip(leafs, restored)])
        update = MutatorSetUpdate([C.to_record(r) for r in recs3], [A.commitment(*it) for it in adds3])
        job, statuses = store.revert(C.to_msa(arch2.msa()), update, expected=archive.accumulator())
        assert job[1] == R.OK and statuses == [R.OK] * len(leafs)
        revert_ok(archive, arch2, adds3, recs3)
        fresh = _restore_all(archive, arch2, leafs)
        crossed = store.read()
        assert all(st == (True, True) for st in [x[:2] for x in store.check(archive.accumulator())])
    for i, (st, w), (fst, p) in zip(leafs, crossed, fresh):
        assert st == R.OK and fst == R.OK
        assert tuples(w.auth_path_aocl) == tuples(p.auth_path_aocl), i
        assert AC.plain_chunks(w.target_chunks) == AC.plain_chunks(p.target_chunks), i
