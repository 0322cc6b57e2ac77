"""GPU: the device-resident witness store (nhip_ms_store_*: k_ms_store_gather, k_ms_store_seal, k_ms_store_check_seal
around the kernels of nhip_ms_update_batch) against the CPU restatement tests/ms_update_ref.py over
`ms_ref.Archival`, never against the store itself: statuses, AOCL paths, keys, paths, chunks and the accumulator
after, field by field, block after block.  The sets and items come from tests/ms_update_cases.py, built once and left
unchanged; each test asserts that its data reaches what it claims."""
import copy
import ctypes
import random

import numpy as np
import pytest

import ms_apply_ref as A
import ms_ref as R
import ms_update_cases as C
import ms_update_ref as U

pytestmark = pytest.mark.gpu

UNIT = 1024  # NHIP_MS_STORE_GATHER_UNIT: 8-byte destination words per work unit of k_ms_store_gather


@pytest.fixture(scope="module")
def cases():
    return C.cases()


def block_args(msa, adds, recs):
    from neptune_hip.mutator_set import MutatorSetUpdate
    return C.to_msa(msa), MutatorSetUpdate([C.to_record(r) for r in recs], [A.commitment(*it) for it in adds])


def advance(arch, adds, recs):
    """The archival set after a block; `arch` stays as it is."""
    a = A.clone(arch)
    for it in adds:
        a.add(*it)
    for r in copy.deepcopy(list(recs)):
        a.remove(r)
    return a


def slots_zero(w):
    return (not any(x for d in w.auth_path_aocl for x in d) and
            not any(ci or any(x for d in path for x in d) or any(ch.relative_indices) for ci, path, ch in w.target_chunks))


def same_job(job, want):
    assert job[:3] == want[:3], (job[:3], want[:3])
    if want[3] is None:
        assert job[3] is None
    else:
        assert A.same(C.back_msa(job[3]), want[3])


def same_witnesses(got, want, label=""):
    """got: `read()`'s; want: the helper's [(status, witness after or None)]"""
    assert len(got) == len(want), label
    for k, ((st, w), (want_st, want_w)) in enumerate(zip(got, want)):
        assert st == want_st, (label, k, st, want_st)
        if want_st == R.OK:
            assert C.plain(w) == C.plain(want_w), (label, k)
        else:
            assert slots_zero(w), (label, k)


def new_store(ctx, wits, initial=None):
    from neptune_hip.mutator_set import WitnessStore
    s = WitnessStore(ctx, initial)
    s.append([C.to_witness(w) for w in wits])
    return s


def run_block(store, msa, adds, recs, want, label=""):
    """One update against the helper's outcome `want` = (job, [(status, witness)]); nothing is read."""
    job, statuses = store.update(*block_args(msa, adds, recs))
    same_job(job, want[0])
    assert statuses == [st for st, _ in want[1]], label
    return job


@pytest.fixture(scope="module")
def mini(cases):
    """Twenty additions and three removals on the set of 600 with 90 witnesses, three of them the block's own
    records."""
    c = cases
    everyone = c.both.wits[:-12]
    wits = everyone[::7] + [U.as_witness(r) for r in c.twelve[:3]]
    assert 80 <= len(wits) <= 100 and sum(w.aocl_leaf_index is None for w in wits) >= 4
    return C.Case("mini", c.arch, c.msa, c.adds20, c.twelve[:3], wits)


# ---------------------------------------------------------------- 1. one block equals the restatement
def test_one_block_equals_the_restatement(ctx, cases):
    group = [cases.adds600[3], cases.removals, cases.both, cases.born]
    assert [(len(cs.adds), len(cs.recs)) for cs in group] == [(300, 0), (0, 12), (20, 12), (300, 0)]
    assert any(w.aocl_leaf_index is not None and w.aocl_leaf_index >= 600 for w in cases.born.wits)
    for cs in group:
        assert cs.want[0][1] == R.OK and all(st == R.OK for st, _ in cs.want[1])
        with new_store(ctx, cs.wits) as store:
            assert len(store) == len(cs.wits) and store.counts()[0] == len(cs.wits)
            run_block(store, cs.msa, cs.adds, cs.recs, cs.want, cs.label)
            same_witnesses(store.read(), cs.want[1], cs.label)


# ---------------------------------------------------------------- 2. three blocks, nothing read in between
def _three_blocks(cases):
    c = cases
    arch0 = c.arch
    blocks = []  # (archival set before, additions, removal records)
    adds1 = c.adds300
    arch1 = advance(arch0, adds1, [])
    blocks.append((arch0, adds1, []))
    recs2 = [arch1.removal_record(i) for i in c.low[:6]]
    arch2 = advance(arch1, [], recs2)
    blocks.append((arch1, [], recs2))
    adds3 = c.adds20
    recs3 = [arch2.removal_record(i) for i in c.low[6:9]]
    arch3 = advance(arch2, adds3, recs3)
    blocks.append((arch2, adds3, recs3))
    leafs = c.live[::5]
    rec_leafs = [i for i in c.live[3::40] if i not in c.low][:8]
    wits0 = [U.proof_witness(arch0, i) for i in leafs] + [U.record_witness(arch0, i) for i in rec_leafs]
    final = [(R.OK, U.proof_witness(arch3, i)) for i in leafs] + [(R.OK, U.record_witness(arch3, i)) for i in rec_leafs]
    return blocks, wits0, final


def test_three_consecutive_blocks(ctx, cases):
    blocks, wits0, final = _three_blocks(cases)
    assert len(wits0) > 100
    # the helper's outcome block by block: each block's witnesses are the last block's results
    wants, wits = [], wits0
    for arch, adds, recs in blocks:
        want = U.outcome(arch, arch.msa(), adds, recs, wits)
        assert want[0][1] == R.OK and all(st == R.OK for st, _ in want[1])
        wants.append(want)
        wits = [w for _, w in want[1]]
    (a0, adds1, _), (a1, _, recs2), _ = blocks
    assert U.batch_after(a0.msa(), len(adds1)) > a0.msa().batch_index  # block 1 slides the window
    held = {ci for _, w in wants[0][1] for ci, _, _ in w.target_chunks}
    hit = {ci for r in recs2 for ci in C.chunks_of(r.absolute_indices, a1.msa().batch_index)}
    assert held & hit  # block 2's removals fall in chunks the witnesses hold
    changed = sum(C.plain(a)[5] != C.plain(b)[5] for (_, a), (_, b) in zip(wants[0][1], wants[1][1]))
    assert changed
    n0, old_peaks = 600, [tuple(p) for p in a0.msa().aocl.peaks]
    grows = takes_peak = takes_new = 0
    for w, (_, new) in zip(wits0, wants[0][1]):
        if w.aocl_leaf_index is None:
            continue
        l, before, after = w.aocl_leaf_index, w.auth_path_aocl, new.auth_path_aocl
        grows += len(after) - len(before) >= 2
        for t in range(len(before), len(after)):
            takes_peak += tuple(after[t]) in old_peaks
            takes_new += ((((l >> t) ^ 1) + 1) << t) > n0
    assert grows and takes_peak and takes_new
    # derived from scratch against the final set: what the chained outcomes give as well
    assert [C.plain(w) for _, w in wants[2][1]] == [C.plain(w) for _, w in final]

    with new_store(ctx, wits0) as store:
        for (arch, adds, recs), want in zip(blocks, wants):
            run_block(store, arch.msa(), adds, recs, want)
        got = store.read()
        same_witnesses(got, final, "three blocks")
    with new_store(ctx, wits0) as store:  # the same sequence, read after every block
        for (arch, adds, recs), want in zip(blocks, wants):
            run_block(store, arch.msa(), adds, recs, want)
            each = store.read()
            same_witnesses(each, want[1], "read after every block")
        assert [(st, C.plain(w)) for st, w in each] == [(st, C.plain(w)) for st, w in got]


# ---------------------------------------------------------------- 3. append between blocks, born in the block
def test_append_between_blocks_and_born_in_the_block(ctx, cases):
    c = cases
    arch0, adds1, adds2 = c.arch, c.adds300[:9], c.adds20
    arch1 = advance(arch0, adds1, [])
    arch2 = advance(arch1, adds2, [])
    old = [U.proof_witness(arch0, i) for i in c.live[:60:3]]
    want1 = U.outcome(arch0, arch0.msa(), adds1, [], old)
    n0, n1 = arch1.msa().aocl.num_leafs, arch2.msa().aocl.num_leafs
    assert (n0, n1) == (609, 629)
    born = U.Wit(arch2.index_set(615), [], 615, R.aocl_leaf(*arch2.items[615]), [])
    late = [U.proof_witness(arch1, i) for i in (c.live[100], 604, 608)] + [born, U.record_witness(arch1, c.live[101])]
    assert born.auth_path_aocl == [] and n0 <= born.aocl_leaf_index < n1
    both = [w for _, w in want1[1]] + late
    want2 = U.outcome(arch1, arch1.msa(), adds2, [], both)
    assert all(st == R.OK for st, _ in want1[1] + want2[1])
    with new_store(ctx, old) as store:
        run_block(store, arch0.msa(), adds1, [], want1)
        store.append([C.to_witness(w) for w in late])
        assert len(store) == len(old) + 5
        run_block(store, arch1.msa(), adds2, [], want2)
        got = store.read()
        same_witnesses(got, want2[1])
        assert len(got[len(old) + 3][1].auth_path_aocl) == ((615 ^ n1).bit_length() - 1) > 0


# ---------------------------------------------------------------- 4. retain
def test_retain(ctx, mini):
    W = len(mini.wits)
    masks = {"every third dropped": [k % 3 != 2 for k in range(W)], "the first only": [k == 0 for k in range(W)],
             "the last only": [k == W - 1 for k in range(W)], "none": [False] * W, "all": [True] * W}
    for label, mask in masks.items():
        kept = [w for w, k in zip(mini.wits, mask) if k]
        want = U.outcome(mini.arch, mini.msa, mini.adds, mini.recs, kept)
        assert want[0][1] == R.OK
        with new_store(ctx, mini.wits) as store:
            store.retain(mask)
            assert len(store) == len(kept) == store.counts()[0]
            same_witnesses(store.read(), [(R.OK, w) for w in kept], label)
            run_block(store, mini.msa, mini.adds, mini.recs, want, label)
            same_witnesses(store.read(), want[1], label)


# ---------------------------------------------------------------- 5. read selections
def test_read_selections(ctx, mini):
    from neptune_hip import _lib as L
    W = len(mini.wits)
    with new_store(ctx, mini.wits) as store:
        run_block(store, mini.msa, mini.adds, mini.recs, mini.want)
        everything = [(st, C.plain(w)) for st, w in store.read(None)]
        assert [p for _, p in everything] == [C.plain(w) for _, w in mini.want[1]]
        for sel in ([], list(range(W))[::-1], [3, 3, 0, W - 1, 3], [W // 2]):
            idx, totals, o = store.read_raw(sel)  # raises unless the count pass and the fill agree
            assert idx == sel and totals == (int(o["aocl_path_off"][-1]), int(o["entry_off"][-1]),
                                             int(o["path_off"][-1]), int(o["rel_off"][-1]))
            assert [(st, C.plain(w)) for st, w in store.read(sel)] == [everything[i] for i in sel], sel
        # an index equal to W: an argument error, the outputs as they were
        _, (A_, E, PD, RW), o = store.read_raw([0, 1])
        for a in o.values():
            a.reshape(-1).view(np.uint8)[:] = 0xCD
        sel = np.asarray([0, W], dtype=np.uint64)
        out = L.MsUpdated(*(o[f].ctypes.data for f, _ in L.MsUpdated._fields_[:9]), A_, E, PD, RW)
        assert ctx.lib.nhip_ms_store_read(store._h, sel.ctypes.data, 2, ctypes.byref(out)) == L.NHIP_ERR_ARG
        assert all((a.reshape(-1).view(np.uint8) == 0xCD).all() for a in o.values())
        assert ctx.lib.nhip_ms_store_read(store._h, None, W - 1, ctypes.byref(out)) == L.NHIP_ERR_ARG  # "all" is W


# ---------------------------------------------------------------- 6. gather edges
def _synthetic(rng, n_aocl, chunk_lens, path_lens=None, removal=False):
    from neptune_hip.mast import AbsoluteIndexSet
    from neptune_hip.mutator_set import Chunk, Witness
    dig = lambda: tuple(rng.randrange(1, R.P) for _ in range(5))  # noqa: E731
    path_lens = path_lens or [rng.randrange(0, 4) for _ in chunk_lens]
    tc = [(rng.randrange(1, 1 << 40), [dig() for _ in range(p)], Chunk([rng.randrange(1, 4096) for _ in range(n)]))
          for n, p in zip(chunk_lens, path_lens)]
    idx = AbsoluteIndexSet(rng.randrange(1 << 100), [rng.randrange(1 << 20) for _ in range(45)])
    if removal:
        return Witness(idx, tc)
    return Witness(idx, tc, rng.randrange(1 << 40), dig(), [dig() for _ in range(n_aocl)])


def test_gather_edges(ctx):
    from neptune_hip import _lib as L
    from neptune_hip.mutator_set import WitnessStore
    assert L.MS_STORE_GATHER_UNIT == UNIT
    rng = random.Random(61)
    wits = [
        _synthetic(rng, 3, []),                                  # 0: no dictionary entries
        _synthetic(rng, 0, [0, 1, 3, 5], removal=True),          # 1: no AOCL part, a chunk of 0 words, odd counts
        _synthetic(rng, 0, [7]),                                 # 2: an empty AOCL path; its chunk begins at word 9
        _synthetic(rng, 2, [2 * UNIT + 501], [300]),             # 3: longer than a unit in the paths and the words
        _synthetic(rng, 1, [2 * UNIT - 1], [0]),                 # 4
        _synthetic(rng, 1, [1], [0]),                            # 5
        _synthetic(rng, 1, [1], [0]),                            # 6
        _synthetic(rng, 5, [0] * (UNIT - 1), [0] * (UNIT - 1)),  # 7: one key short of a unit
    ] + [_synthetic(rng, rng.randrange(0, 6), [rng.randrange(0, 12) for _ in range(rng.randrange(0, 5))]) for _ in range(40)]
    assert 5 * 300 > UNIT and sum(len(c.relative_indices) for _, _, c in wits[1].target_chunks) % 2 == 1
    plain = [C.plain(w) for w in wits]
    with WitnessStore(ctx) as store:
        store.append(wits[:5])
        store.append(wits[5:])
        assert [(st, C.plain(w)) for st, w in store.read()] == [(R.OK, p) for p in plain]
        order = list(range(len(wits)))[::-1]
        assert [C.plain(w) for _, w in store.read(order)] == [plain[i] for i in order]
        # totals one below, equal to and one above a unit: chunk words (2 * UNIT u32), then keys (UNIT words)
        for sel, pool, total in (([4], 3, 2 * UNIT - 1), ([4, 5], 3, 2 * UNIT), ([4, 5, 6], 3, 2 * UNIT + 1),
                                 ([6, 5, 4], 3, 2 * UNIT + 1), ([7], 1, UNIT - 1), ([7, 5], 1, UNIT), ([5, 7, 6], 1, UNIT + 1)):
            _, totals, _ = store.read_raw(sel)
            assert totals[pool] == total, (sel, totals)
            assert [C.plain(w) for _, w in store.read(sel)] == [plain[i] for i in sel], sel
        # a range that begins on a 4-byte boundary that is no 8-byte boundary, in the source and in the destination
        _, _, o = store.read_raw([1, 2, 3])
        assert int(o["rel_off"][4]) % 2 == 1 and int(o["rel_off"][5]) % 2 == 0
        mask = [k % 2 == 1 or k == 3 for k in range(len(wits))]
        store.retain(mask)
        kept = [p for p, k in zip(plain, mask) if k]
        assert [(st, C.plain(w)) for st, w in store.read()] == [(R.OK, p) for p in kept]
        store.append(wits[:2])
        assert [C.plain(w) for _, w in store.read()] == kept + plain[:2]


# ---------------------------------------------------------------- 7. sticky status
def test_sticky_status(ctx, cases):
    c, cs = cases, cases.with_mutants
    want1 = cs.want
    bad = c.mutant_at
    assert {want1[1][k][0] for k in bad} == {R.NOT_IN_AOCL, R.OUT_OF_RANGE, R.ABSENT_CHUNK, R.BAD_MMR_PATH}
    assert want1[0][1] == R.OK and all(want1[1][k][0] == R.OK for k in range(19) if k not in bad)
    arch1 = advance(cs.arch, cs.adds, cs.recs)
    adds2, recs2 = c.adds20[:10], [arch1.removal_record(c.low[5])]
    good1 = [w for k, (_, w) in enumerate(want1[1]) if k not in bad]
    good2 = U.outcome(arch1, arch1.msa(), adds2, recs2, good1)
    assert good2[0][1] == R.OK and all(st == R.OK for st, _ in good2[1])
    it = iter(good2[1])
    want2 = [(want1[1][k][0], None) if k in bad else next(it) for k in range(19)]
    with new_store(ctx, cs.wits) as store:
        run_block(store, cs.msa, cs.adds, cs.recs, want1)
        got1 = store.read()
        same_witnesses(got1, want1[1], "block 1")
        assert sum(len(got1[k][1].target_chunks) for k in bad) > 0  # planned slots, zero, not absent
        job, statuses = store.update(*block_args(arch1.msa(), adds2, recs2))
        same_job(job, good2[0])
        assert statuses == [st for st, _ in want2]
        same_witnesses(store.read(), want2, "block 2")
        verdicts = store.check(C.to_msa(advance(arch1, adds2, recs2).msa()))
        for k in range(19):
            if k in bad:
                assert verdicts[k] == (False, False, False, want1[1][k][0]), k
            else:
                assert verdicts[k][:2] == (True, True), k
        store.retain([k not in bad for k in range(19)])
        same_witnesses(store.read(), good2[1], "the rest")


# ---------------------------------------------------------------- 8. a rejected job changes nothing
def test_job_rejected_leaves_the_store_unchanged(ctx, cases):
    c = cases
    rej, nb = c.rejected_jobs, c.neighbours[0]
    assert [cs.want[0][:3] for cs in rej] == [(False, R.ALREADY_REMOVED, 1), (False, A.DUPLICATE_RECORD, 2),
                                              (False, A.UPDATE_IMPOSSIBLE, 1)]
    wits = nb.wits
    assert all([C.plain(a) for a in cs.wits] == [C.plain(a) for a in wits] for cs in rej)
    with new_store(ctx, wits) as store:
        before = {f: a.tobytes() for f, a in store.read_raw()[2].items()}
        counts = store.counts()
        for cs in rej:
            job, statuses = store.update(*block_args(cs.msa, cs.adds, cs.recs))
            same_job(job, cs.want[0])
            assert statuses == [U.JOB_REJECTED] * len(wits)
        # 2.e: the block is fine, the expected accumulator is not
        msa, upd = block_args(nb.msa, nb.adds, nb.recs)
        job, statuses = store.update(msa, upd, expected=msa)
        assert job[:2] == (False, A.UPDATE_MISMATCH) and statuses == [U.JOB_REJECTED] * len(wits)
        assert {f: a.tobytes() for f, a in store.read_raw()[2].items()} == before and store.counts() == counts
        run_block(store, nb.msa, nb.adds, nb.recs, nb.want)
        same_witnesses(store.read(), nb.want[1])


# ---------------------------------------------------------------- 9. growth
def test_growth_from_tiny_capacities(ctx, mini):
    caps = dict(witnesses=1, aocl_digests=2, entries=1, path_digests=2, rel_words=3)
    from neptune_hip.mutator_set import WitnessStore
    with WitnessStore(ctx, caps) as store:
        store.append([C.to_witness(w) for w in mini.wits[:1]])
        store.append([C.to_witness(w) for w in mini.wits[1:40]])
        store.append([C.to_witness(w) for w in mini.wits[40:]])
        before = store.counts()
        assert all(x > y for x, y in zip(before, (1, 2, 1, 2, 3)))
        same_witnesses(store.read(), [(R.OK, w) for w in mini.wits])
        run_block(store, mini.msa, mini.adds, mini.recs, mini.want)
        after = store.counts()
        assert after[0] == before[0] and after[1] >= before[1] and all(x > y for x, y in zip(after[2:], before[2:]))
        same_witnesses(store.read(), mini.want[1])


# ---------------------------------------------------------------- 10. check
def test_check_against_the_accumulators(ctx, mini):
    from neptune_hip import mutator_set as MS
    after = mini.want[0][3]
    with new_store(ctx, mini.wits) as store:
        run_block(store, mini.msa, mini.adds, mini.recs, mini.want)
        now = store.check(C.to_msa(after))
        removed = [r.absolute_indices.to_array() for r in mini.recs]
        own = [k for k, w in enumerate(mini.wits) if w.absolute_indices.to_array() in removed]
        assert len(own) >= 3
        for k, v in enumerate(now):
            assert v == ((True, True, False, MS.ALREADY_REMOVED) if k in own else (True, True, True, MS.OK)), k
        # against the accumulator before: what the batch calls give for the same data passed from the host
        got = [w for _, w in store.read()]
        recs = [MS.RemovalRecord(w.absolute_indices, w.target_chunks) for w in got]
        before = C.to_msa(mini.msa)
        want_rec = MS.can_remove_batch(ctx, before, recs)
        proofs = [(k, w) for k, w in enumerate(got) if w.aocl_leaf_index is not None]
        member = MS.mmr_verify_batch(ctx, before.aocl, [(w.aocl_leaf_index, w.aocl_leaf, w.auth_path_aocl) for _, w in proofs])
        want_member = [True] * len(got)
        for (k, _), m in zip(proofs, member):
            want_member[k] = m
        stale = store.check(before)
        assert stale == [(m,) + r for m, r in zip(want_member, want_rec)]
        assert not all(want_member) and any(not r[0] for r in want_rec)  # the block changed what they hold


# ---------------------------------------------------------------- 11. agreement with the batch call
def test_agreement_with_the_batch_call(ctx, mini):
    from neptune_hip.mutator_set import update_witnesses_batch
    batch = update_witnesses_batch(ctx, [mini.gpu()])[0]
    with new_store(ctx, mini.wits) as store:
        job, statuses = store.update(*block_args(mini.msa, mini.adds, mini.recs))
        assert job[:3] == batch[:3] and statuses == [st for st, _ in batch[4]]
        assert [C.plain(w) for _, w in store.read()] == [C.plain(w) for _, w in batch[4]]


# ---------------------------------------------------------------- 12. argument errors
def test_argument_errors_leave_everything_untouched(ctx, mini):
    from neptune_hip import _lib as L
    from neptune_hip import mutator_set as MS
    lib = ctx.lib
    with new_store(ctx, mini.wits[:20]) as store:
        W = len(store)
        before = {f: a.tobytes() for f, a in store.read_raw()[2].items()}
        counts = store.counts()
        pa = MS.PackedApply([block_args(mini.msa, mini.adds, mini.recs)] * 2)
        status = np.full(W, 0xAB, dtype=np.uint8)

        def update(n_jobs, out=ctypes.byref(pa.cout)):
            cin = L.MsApplyIn(*(getattr(pa.cin, f) for f, _ in L.MsApplyIn._fields_))
            cin.n_jobs = n_jobs
            return lib.nhip_ms_store_update(store._h, ctypes.byref(cin), out, status.ctypes.data)

        assert update(0) == L.NHIP_ERR_ARG and update(2) == L.NHIP_ERR_ARG
        assert update(1, out=None) == L.NHIP_ERR_ARG
        assert (status == 0xAB).all() and not pa.arrays["status"].any() and not pa.arrays["aocl_num_leafs"].any()
        pw = MS.PackedWitnesses([C.to_witness(w) for w in mini.wits[20:30]])

        def append(**kw):
            w = L.MsUpdateIn(*(getattr(pw.win, f) for f, _ in L.MsUpdateIn._fields_))
            for f, v in kw.items():
                setattr(w, f, v)
            return lib.nhip_ms_store_append(store._h, ctypes.byref(w), pw.n)

        for f in ("minimum", "distances", "aocl_leaf_index", "aocl_leaf", "aocl_path_off", "aocl_path", "chunks"):
            assert append(**{f: None}) == L.NHIP_ERR_ARG, f
        off = pw.aocl_path_off.copy()
        off[0] = 1
        assert append(aocl_path_off=off.ctypes.data) == L.NHIP_ERR_ARG
        off = pw.aocl_path_off.copy()
        off[3], off[4] = off[4] + 1, off[3]
        assert append(aocl_path_off=off.ctypes.data) == L.NHIP_ERR_ARG
        ro = pw.packed.rel_off.copy()
        ro[1], ro[2] = ro[2] + 1, ro[1]
        bad = L.MsChunks(pw.chunks.entry_off, pw.chunks.chunk_index, pw.chunks.path_off, pw.chunks.path, ro.ctypes.data,
                         pw.chunks.rel)
        assert append(chunks=ctypes.pointer(bad)) == L.NHIP_ERR_ARG
        assert lib.nhip_ms_store_append(store._h, None, 3) == L.NHIP_ERR_ARG
        assert lib.nhip_ms_store_read(store._h, None, W, None) == L.NHIP_ERR_ARG
        assert lib.nhip_ms_store_retain(store._h, None) == L.NHIP_ERR_ARG
        cm, _keep = C.to_msa(mini.msa)._c()
        v = np.full(W, 0xAB, dtype=np.uint8)
        assert lib.nhip_ms_store_check(store._h, ctypes.byref(cm), v.ctypes.data, None, v.ctypes.data, v.ctypes.data) == L.NHIP_ERR_ARG
        assert lib.nhip_ms_store_check(store._h, None, *([v.ctypes.data] * 4)) == L.NHIP_ERR_ARG
        assert (v == 0xAB).all()
        assert {f: a.tobytes() for f, a in store.read_raw()[2].items()} == before and store.counts() == counts
        assert append() == L.NHIP_OK and store.counts()[0] == W + 10  # the same arguments, unbroken
        # the statuses may be left out: the update is the same
        one = MS.PackedApply([block_args(mini.msa, mini.adds, mini.recs)])
        assert lib.nhip_ms_store_update(store._h, ctypes.byref(one.cin), ctypes.byref(one.cout), None) == L.NHIP_OK
        assert int(one.arrays["status"][0]) == R.OK
        got = store.read_raw(range(30))[2]  # ten of them were appended past the Python object
        want = mini.want[1][:30]
        assert not got["status"].any() and len(got["status"]) == 30
        assert [int(x) for x in np.diff(got["aocl_path_off"])] == [len(w.auth_path_aocl) for _, w in want]
