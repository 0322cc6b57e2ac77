"""GPU: membership proofs and removal records taken back across a block (nhip_ms_revert_batch and
nhip_ms_store_revert: k_ms_revert_nodes, k_ms_rev_admit, k_ms_rev_paths, k_ms_rev_chunks, the verification by
k_mmr_verify and k_ms_chunk_auth_jobs, k_ms_rev_seal, k_ms_store_seal) against the CPU restatement
tests/ms_revert_ref.py, which tests/test_ms_revert_ref.py holds to witnesses derived from scratch over
`ms_ref.Archival`; never against the kernels themselves.  Statuses, AOCL paths, keys, paths, chunks and the accumulator
after, field by field.  The sets and jobs come from tests/ms_update_cases.py, built once and left unchanged; the
witnesses after a block are tests/ms_update_ref.py's.  Each test asserts that its data reaches what it claims."""
import copy
import ctypes
import random

import numpy as np
import pytest

import ms_apply_ref as A
import ms_ref as R
import ms_revert_ref as V
import ms_update_cases as C
import ms_update_ref as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return C.cases()


class Back:
    """One revert job: the block of `cs` (or other records / witnesses on its set), the witnesses as they stand after
    it, and the helper's answer `want` = (job outcome, [(status, witness before or None)])."""

    def __init__(self, label, arch, msa, adds, recs, after, job=None):
        self.label, self.arch, self.msa, self.adds, self.recs, self.after = label, arch, msa, adds, recs, after
        self.want = V.outcome(arch, msa, adds, recs, after, job=job)
        self.blk = V.Block(msa, len(adds), recs)

    def gpu(self):
        from neptune_hip.mutator_set import MutatorSetUpdate
        return (C.to_msa(self.msa), MutatorSetUpdate([C.to_record(r) for r in self.recs], [A.commitment(*it) for it in self.adds]),
                [C.to_witness(w) for w in self.after])


_backs = {}


def back_of(cs, job=None):
    """The revert of a case of tests/ms_update_cases.py, once per process."""
    if cs.label not in _backs:
        assert cs.want[0][1] == R.OK and all(st == R.OK for st, _ in cs.want[1]), cs.label
        _backs[cs.label] = Back(cs.label, cs.arch, cs.msa, cs.adds, cs.recs, [w for _, w in cs.want[1]], job)
    return _backs[cs.label]


def compare(group, got):
    for b, g in zip(group, got):
        job = b.want[0]
        assert g[:3] == job[:3], (b.label, g[:3], job[:3])
        if job[3] is None:
            assert g[3] is None, b.label
        else:
            assert A.same(C.back_msa(g[3]), job[3]), b.label
        assert len(g[4]) == len(b.want[1])
        for k, ((st, w), (want_st, want_w)) in enumerate(zip(g[4], b.want[1])):
            assert st == want_st, (b.label, k, st, want_st)
            assert C.plain(w) == C.plain(want_w), (b.label, k)


def run(ctx, group):
    """The jobs of `group` in one call; every output against the helper's.  Returns the device's results."""
    from neptune_hip.mutator_set import revert_witnesses_batch
    got = revert_witnesses_batch(ctx, [b.gpu() for b in group])
    compare(group, got)
    return got


def all_ok_and_from_scratch(b, cs):
    """The helper's answer is the from-scratch witnesses before the block, so the device is held to `Archival`."""
    assert b.want[0][1] == R.OK
    assert [(st, C.plain(w)) for st, w in b.want[1]] == [(R.OK, C.plain(w)) for w in cs.wits], b.label


def advance(arch, adds, recs):
    a = A.clone(arch)
    for it in adds:
        a.add(*it)
    for r in copy.deepcopy(list(recs)):
        a.remove(r)
    return a


# ---------------------------------------------------------------- 1. the batch form equals the helper
def test_additions_only(ctx, cases):
    group = [back_of(cs) for cs in cases.adds600]
    assert [len(b.adds) for b in group] == [0, 1, 9, 300] and [b.blk.b1 - b.blk.b0 for b in group] == [0, 1, 2, 38]
    for b, cs in zip(group, cases.adds600):
        all_ok_and_from_scratch(b, cs)
    assert [C.plain(w) for w in group[0].after] == [C.plain(w) for _, w in group[0].want[1]]  # no addition: unchanged
    big = group[3]
    shorter = [len(a.auth_path_aocl) - len(w.auth_path_aocl) for a, (_, w) in zip(big.after, big.want[1])]
    assert max(shorter) >= 2 and sum(s > 0 for s in shorter) == 85
    assert sum(len(w.target_chunks) < len(a.target_chunks) for a, (_, w) in zip(big.after, big.want[1])) == 579
    assert any(len(a.target_chunks) - len(w.target_chunks) >= 5 for a, (_, w) in zip(big.after, big.want[1]))
    run(ctx, group)


def test_removals_only(ctx, cases):
    one, twelve = back_of(cases.one), back_of(cases.removals)
    all_ok_and_from_scratch(one, cases.one)
    all_ok_and_from_scratch(twelve, cases.removals)
    assert len(one.recs) == 1 and len(twelve.recs) == 12 and len(twelve.after) == 592
    assert sum(w.aocl_leaf_index is None for w in twelve.after) == 32  # removal-record witnesses, the block's own too
    blk = twelve.blk
    touched = sorted(blk.by_chunk)
    assert any(ci ^ 1 in blk.by_chunk and V.ilog2(ci ^ blk.b0) >= 1 for ci in touched)  # siblings at level 0
    assert any(2 <= V.ilog2(x ^ y) < V.ilog2(x ^ blk.b0) for x in touched for y in touched)  # ... that meet above level 1
    held = [(ci, blk.replaced(ci)) for w in twelve.after for ci, _, _ in w.target_chunks]
    assert any(0 in r for _, r in held) and any(r and max(r) >= 2 for _, r in held)
    assert any(r and len(r) < V.ilog2(ci ^ blk.b0) for ci, r in held)  # replaced and kept digests in one path
    assert any(ci in blk.by_chunk for ci, _ in held) and any(ci not in blk.by_chunk and r for ci, r in held)
    run(ctx, [one, twelve])


def test_additions_and_removals_all_witnesses(ctx, cases):
    b = back_of(cases.both)
    all_ok_and_from_scratch(b, cases.both)
    assert len(b.after) == 592 and 8 * 592 > 256 and sum(len(w.target_chunks) for w in b.after) > 2048
    assert any(len(ch.relative_indices) % 2 for w in b.after for _, _, ch in w.target_chunks)  # odd chunk lengths
    run(ctx, [b])


def _tiny():
    """A set of 40 with no removal before: every inactive chunk is empty.  The block removes one item whose index set
    reaches below the window, so after it a chunk holds that block's words alone, and before it none."""
    arch, removed = C.build(40, 4040, every=1000)
    assert not removed and arch.msa().batch_index == 4
    victim = next(i for i in range(40) if C.chunks_of(arch.index_set(i), 4))
    adds = C._items(random.Random(41), 3)
    recs = [arch.removal_record(victim)]
    wits = [U.proof_witness(arch, i) for i in range(40)] + [U.record_witness(arch, victim)]
    return C.Case("40 + 3, one removal from empty chunks", arch, arch.msa(), adds, recs, wits)


def test_several_jobs_one_rejected_and_the_small_edges(ctx, cases):
    by = {cs.label: cs for cs in cases.small}
    tiny = _tiny()
    picked = [by["1 + 1"], by["8 + 1"], by["8 + 9"], by["255 + 9"], by["256 + 9"], tiny] + cases.extra
    group = [back_of(cs) for cs in picked]
    for b, cs in zip(group, picked):
        all_ok_and_from_scratch(b, cs)
    first = group[0]
    assert any(not w.target_chunks for w in first.after)  # a witness with no entries
    slide = group[1]
    assert slide.blk.b0 == 0 and slide.blk.b1 == 1  # the first slide ever, taken back: all of a witness's entries drop
    assert any(a.target_chunks and not w.target_chunks for a, (_, w) in zip(slide.after, slide.want[1]))
    t = back_of(tiny)
    assert any(len(ch.relative_indices) == 0 and len(ach.relative_indices) > 0
               for a, (_, w) in zip(t.after, t.want[1]) for (_, _, ach), (_, _, ch) in zip(a.target_chunks, w.target_chunks))
    # a rejected job between accepted ones: the same record twice
    both = back_of(cases.both)
    rejected = Back("2.c between accepted jobs", both.arch, both.msa, both.adds, [both.recs[0], both.recs[1], both.recs[0]],
                    both.after[:7])
    assert rejected.want[0][:3] == (False, A.DUPLICATE_RECORD, 2) and rejected.want[1] == [(V.JOB_REJECTED, None)] * 7
    group = group[:3] + [rejected] + group[3:]
    run(ctx, group)
    run(ctx, group[::-1])


def test_an_index_two_records_insert(ctx, cases):
    """Two records with one absolute index in common: the chunk holds two copies after the block and both go."""
    c = cases
    recs = copy.deepcopy(c.twelve[:4])
    found = None
    for x in range(4):
        for y in range(4):
            if x == y:
                continue
            ix, iy = recs[x].absolute_indices, recs[y].absolute_indices
            for ci in set(C.chunks_of(ix, 74)) & set(C.chunks_of(iy, 74)):
                mine = [t for t, d in enumerate(iy.distances) if (iy.minimum + d) // R.CHUNK_SIZE == ci and d != 0]
                theirs = [i for i in ix.to_array() if i // R.CHUNK_SIZE == ci and i >= iy.minimum]
                if mine and theirs and theirs[0] not in iy.to_array():
                    found = (x, y, mine[0], theirs[0])
    assert found is not None
    x, y, t, index = found
    recs[y].absolute_indices.distances[t] = index - recs[y].absolute_indices.minimum
    assert index in recs[x].absolute_indices.to_array() and index in recs[y].absolute_indices.to_array()
    ci = index // R.CHUNK_SIZE
    wits = [w for w in c.both.wits if any(k == ci for k, _, _ in w.target_chunks)][:12] + c.both.wits[:30]
    fwd = U.outcome(c.arch, c.msa, c.adds20[:3], recs, wits)
    assert fwd[0][1] == R.OK and all(st == R.OK for st, _ in fwd[1])
    b = Back("one index from two records", c.arch, c.msa, c.adds20[:3], recs, [w for _, w in fwd[1]])
    assert b.blk.by_chunk[ci].count(index % R.CHUNK_SIZE) == 2
    assert [(st, C.plain(w)) for st, w in b.want[1]] == [(R.OK, C.plain(w)) for w in wits]
    holder = next(w for w in b.after if any(k == ci for k, _, _ in w.target_chunks))
    assert [ch for k, _, ch in holder.target_chunks if k == ci][0].relative_indices.count(index % R.CHUNK_SIZE) >= 2
    run(ctx, [b])


def test_wide(ctx, cases):
    cs = cases.wide
    b = back_of(cs, job=cs.want[0])
    assert b.blk.n0 == (1 << 40) + 5 and b.blk.b0 == 1 << 37 and not cs.recs  # leaf indices past 2^40; no dictionary
    n0 = b.blk.n0
    for (st, w), before in zip(b.want[1], cs.wits):
        if before.aocl_leaf_index < n0:
            assert st == R.OK and C.plain(w) == C.plain(before)
        else:
            assert st == R.NOT_IN_AOCL
    assert [st for st, _ in b.want[1]].count(R.OK) == 3
    run(ctx, [b])


def test_paths_of_37_levels(ctx):
    """A Bloom-filter MMR of 2^37 chunks (tests/ms_revert_cases.py): the record's entries, the witnesses' entries and
    every reverted path are 37 digests, the old levels are kept up to height 36 and read at heights 0, 1, 10 and 36."""
    import ms_revert_cases as D
    d = D.deep()
    b = Back("2^37 chunks", None, d.msa, d.adds, [d.rec], d.after, job=d.job)
    blk = b.blk
    assert blk.b0 == blk.b1 == 1 << 37 and sorted(blk.by_chunk) == [d.ci2, d.ci] and blk.by_chunk[d.ci2] == [17, 17]
    assert all(len(path) == 37 for _, path, _ in d.rec.target_chunks) and len(d.rec.target_chunks) == 2
    assert all(len(path) == 37 for w in d.after for _, path, _ in w.target_chunks)
    assert blk.replaced(d.sib) == [0, 1] and 10 in blk.replaced(d.c10) and blk.replaced(d.c36) == [36]
    assert blk.replaced(d.ci) == [1] and blk.replaced(d.ci2) == [1]
    # the helper's answer is the witnesses taken from the tree before the block, which verify against its peak
    assert [st for st, _ in b.want[1]] == [R.OK] * 6 + [R.NOT_IN_AOCL]
    assert [C.plain(w) for _, w in b.want[1][:6]] == [C.plain(w) for w in d.before]
    assert all(len(path) == 37 for _, w in b.want[1][:4] for _, path, _ in w.target_chunks)
    assert all(V.verification(d.msa, w) == R.OK for w in d.before)
    assert any(len(ch.relative_indices) == 0 for _, _, ch in b.want[1][0][1].target_chunks)
    # digest 36 of the far witness differs on the two sides of the block: the device has to replace it
    far_after, far_before = d.after[2], d.before[2]
    assert far_after.target_chunks[0][1][36] != far_before.target_chunks[0][1][36]
    assert far_after.target_chunks[0][1][:36] == far_before.target_chunks[0][1][:36]
    stale = Back("2^37 chunks, a stale witness", None, d.msa, d.adds, [d.rec], [d.after[2], d.before[1], d.after[3]], job=d.job)
    assert [st for st, _ in stale.want[1]] == [R.OK, R.BAD_MMR_PATH, R.OK]
    run(ctx, [b, stale])


# ---------------------------------------------------------------- 2. one mutant per status
def _edit(w, **kw):
    m = copy.deepcopy(w)
    for name, f in kw.items():
        setattr(m, name, f(getattr(m, name)))
    return m


def _entry(tc, k, path=None, rel=None, key=None):
    ci, p, ch = tc[k]
    return tc[:k] + [(ci if key is None else key, p if path is None else path, ch if rel is None else R.Chunk(rel))] + tc[k + 1:]


def _mutants(cases):
    both = back_of(cases.both)
    blk, after = both.blk, both.after
    proofs = [w for w in after if w.aocl_leaf_index is not None]
    deep = next(w for w in proofs if V.ilog2(w.aocl_leaf_index ^ blk.n0) >= 2)

    def entry_where(pred):
        for w in proofs:
            for k, (ci, path, ch) in enumerate(w.target_chunks):
                if ci < blk.b0 and pred(ci, path, ch):
                    return w, k
        raise AssertionError("no such entry")

    w_kept, k_kept = entry_where(lambda ci, p, ch: len(blk.replaced(ci)) < V.ilog2(ci ^ blk.b0))
    t_kept = next(t for t in range(V.ilog2(w_kept.target_chunks[k_kept][0] ^ blk.b0))
                  if t not in blk.replaced(w_kept.target_chunks[k_kept][0]))
    w_rep, k_rep = entry_where(lambda ci, p, ch: blk.replaced(ci))
    t_rep = blk.replaced(w_rep.target_chunks[k_rep][0])[0]
    w_word, k_word = entry_where(lambda ci, p, ch: ci in blk.by_chunk and
                                 any(v not in blk.by_chunk[ci] for v in ch.relative_indices))
    ci_word, _, ch_word = w_word.target_chunks[k_word]
    p_word = next(p for p, v in enumerate(ch_word.relative_indices) if v not in blk.by_chunk[ci_word])
    changed = list(ch_word.relative_indices)
    changed[p_word] ^= 1
    missing = list(ch_word.relative_indices)
    missing.remove(blk.by_chunk[ci_word][0])
    w_long, k_long = entry_where(lambda ci, p, ch: len(p) >= 1)
    arch_after = advance(cases.arch, cases.both.adds, cases.both.recs)
    born = U.proof_witness(arch_after, blk.n0 + 5)
    flip_at = lambda path, t: list(path[:t]) + [C.flip(path[t])] + list(path[t + 1:])  # noqa: E731
    mutants = [
        ("a kept AOCL digest flipped", R.NOT_IN_AOCL, _edit(deep, auth_path_aocl=lambda p: flip_at(p, 1))),
        ("a kept dictionary digest flipped", R.BAD_MMR_PATH,
         _edit(w_kept, target_chunks=lambda tc: _entry(tc, k_kept, path=flip_at(tc[k_kept][1], t_kept)))),
        ("a digest the revert replaces flipped", R.OK,
         _edit(w_rep, target_chunks=lambda tc: _entry(tc, k_rep, path=flip_at(tc[k_rep][1], t_rep)))),
        ("a chunk word changed", R.BAD_MMR_PATH, _edit(w_word, target_chunks=lambda tc: _entry(tc, k_word, rel=changed))),
        ("a block index missing from the chunk", R.BAD_MMR_PATH,
         _edit(w_word, target_chunks=lambda tc: _entry(tc, k_word, rel=missing))),
        ("a wrong key", R.ABSENT_CHUNK, _edit(w_kept, target_chunks=lambda tc: _entry(tc, k_kept, key=tc[k_kept][0] ^ (1 << 20)))),
        ("a path one digest short", R.BAD_MMR_PATH,
         _edit(w_long, target_chunks=lambda tc: _entry(tc, k_long, path=list(tc[k_long][1][:-1])))),
        ("born in the block", R.NOT_IN_AOCL, born),
    ]
    good = proofs[:40:4]
    wits = []
    for k, (_, _, m) in enumerate(mutants):
        wits += [good[k], m]
    wits.append(good[8])
    return both, mutants, wits, (w_rep, k_rep, t_rep)


def test_one_mutant_per_status_between_good_witnesses(ctx, cases):
    from neptune_hip import mutator_set as MS
    both, mutants, wits, (w_rep, k_rep, t_rep) = _mutants(cases)
    b = Back("eight mutants", both.arch, both.msa, both.adds, both.recs, wits)
    got_st = [st for st, _ in b.want[1]]
    assert [got_st[k] for k in range(1, 17, 2)] == [want for _, want, _ in mutants]
    assert all(got_st[k] == R.OK for k in range(0, 17, 2))
    # the replaced digest is not read: the flipped witness reverts to what the true one reverts to
    true_back = V.revert_witness(b.blk, w_rep)
    assert C.plain(b.want[1][5][1]) == C.plain(true_back)
    assert tuple(true_back.target_chunks[k_rep][1][t_rep]) != tuple(w_rep.target_chunks[k_rep][1][t_rep])
    run(ctx, [b])
    # every failed witness's slots are zero, in the planned shape
    pu = MS.PackedUpdate([b.gpu()], revert=True)
    assert pu.run(ctx.lib, ctx.handle) == 0
    o = pu.out
    assert [int(x) for x in o["status"]] == got_st
    planned = 0
    for k, st in enumerate(got_st):
        if st == R.OK:
            continue
        a0, a1 = int(o["aocl_path_off"][k]), int(o["aocl_path_off"][k + 1])
        e0, e1 = int(o["entry_off"][k]), int(o["entry_off"][k + 1])
        p0, p1, r0, r1 = int(o["path_off"][e0]), int(o["path_off"][e1]), int(o["rel_off"][e0]), int(o["rel_off"][e1])
        assert not o["aocl_path"][a0:a1].any() and not o["chunk_index"][e0:e1].any()
        assert not o["path"][p0:p1].any() and not o["rel"][r0:r1].any()
        planned += (a1 - a0) + (e1 - e0) + (p1 - p0) + (r1 - r0)
    assert planned > 50


# ---------------------------------------------------------------- 3. the store
def block_args(msa, adds, recs):
    from neptune_hip.mutator_set import MutatorSetUpdate
    return C.to_msa(msa), MutatorSetUpdate([C.to_record(r) for r in recs], [A.commitment(*it) for it in adds])


def new_store(ctx, wits, initial=None):
    from neptune_hip.mutator_set import WitnessStore
    s = WitnessStore(ctx, initial)
    s.append([C.to_witness(w) for w in wits])
    return s


def slots_zero(w):
    return (not any(x for d in w.auth_path_aocl for x in d) and
            not any(ci or any(x for d in path for x in d) or any(ch.relative_indices) for ci, path, ch in w.target_chunks))


def same_witnesses(got, want, label=""):
    assert len(got) == len(want), label
    for k, ((st, w), (want_st, want_w)) in enumerate(zip(got, want)):
        assert st == want_st, (label, k, st, want_st)
        if want_st == R.OK:
            assert C.plain(w) == C.plain(want_w), (label, k)
        else:
            assert slots_zero(w), (label, k)


def raw(store):
    return {f: a.tobytes() for f, a in store.read_raw()[2].items()}


@pytest.fixture(scope="module")
def mini(cases):
    """Twenty additions and three removals on the set of 600 with some 90 witnesses, three of them the block's own
    records (the fixture of tests/test_gpu_ms_store.py)."""
    c = cases
    everyone = c.both.wits[:-12]
    wits = everyone[::7] + [U.as_witness(r) for r in c.twelve[:3]]
    assert 80 <= len(wits) <= 100
    return C.Case("mini", c.arch, c.msa, c.adds20, c.twelve[:3], wits)


def test_update_then_revert_reads_back_what_was_appended(ctx, mini):
    from neptune_hip import mutator_set as MS
    W = len(mini.wits)
    assert 80 <= W <= 100 and mini.want[0][1] == R.OK
    b = Back("mini back", mini.arch, mini.msa, mini.adds, mini.recs, [w for _, w in mini.want[1]])
    assert all(st == R.OK for st, _ in b.want[1])
    with new_store(ctx, mini.wits) as store:
        appended, counts = raw(store), store.counts()
        job, statuses = store.update(*block_args(mini.msa, mini.adds, mini.recs))
        assert job[1] == R.OK and statuses == [R.OK] * W and raw(store) != appended
        tip = job[3]
        job, statuses = store.revert(*block_args(mini.msa, mini.adds, mini.recs), expected=tip)
        assert job[:3] == (True, R.OK, None) and A.same(C.back_msa(job[3]), mini.want[0][3])
        assert statuses == [R.OK] * W
        assert raw(store) == appended and store.counts() == counts
        # check(msa_before): every witness valid where the store now stands
        verdicts = store.check(C.to_msa(mini.msa))
        assert all(v[0] and v[1] and v[3] in (MS.OK, MS.ALREADY_REMOVED) for v in verdicts)
        assert sum(v[2] for v in verdicts) >= 80
        # the store form agrees byte for byte with the batch form
        store.update(*block_args(mini.msa, mini.adds, mini.recs))
        pu = MS.PackedUpdate([b.gpu()], revert=True)
        assert pu.run(ctx.lib, ctx.handle) == 0
        job, statuses = store.revert(*block_args(mini.msa, mini.adds, mini.recs))
        assert statuses == [int(x) for x in pu.out["status"]]
        assert raw(store) == {f: a.tobytes() for f, a in pu.out.items()}
    compare([b], MS.revert_witnesses_batch(ctx, [b.gpu()]))


def _chain(cases):
    c = cases
    arch0 = c.arch
    adds1 = c.adds300[:40]
    arch1 = advance(arch0, adds1, [])
    recs2 = [arch1.removal_record(i) for i in c.low[:6]]
    arch2 = advance(arch1, [], recs2)
    adds3 = c.adds20
    recs3 = [arch2.removal_record(i) for i in c.low[6:9]]
    arch3 = advance(arch2, adds3, recs3)
    blocks = [(arch0, adds1, []), (arch1, [], recs2), (arch2, adds3, recs3)]
    leafs = c.live[::9]
    rec_leafs = [i for i in c.live[3::40] if i not in c.low][:6]
    tips = [[U.proof_witness(a, i) for i in leafs] + [U.record_witness(a, i) for i in rec_leafs]
            for a in (arch0, arch1, arch2, arch3)]
    other_adds, other_recs = c.adds300[100:111], [arch0.removal_record(i) for i in c.low[9:11]]
    fork = advance(arch0, other_adds, other_recs)
    fork_tip = [U.proof_witness(fork, i) for i in leafs] + [U.record_witness(fork, i) for i in rec_leafs]
    return blocks, tips, (other_adds, other_recs, fork, fork_tip)


def test_three_blocks_forward_three_back_then_another_fork(ctx, cases):
    blocks, tips, (other_adds, other_recs, fork, fork_tip) = _chain(cases)
    assert len(tips[0]) > 60
    assert U.batch_after(blocks[0][0].msa(), len(blocks[0][1])) > blocks[0][0].msa().batch_index  # block 1 slides
    assert [C.plain(w) for w in tips[3]] != [C.plain(w) for w in tips[2]] != [C.plain(w) for w in tips[1]]
    msas = [a.msa() for a, _, _ in blocks] + [advance(*blocks[2]).msa()]
    for reading in (False, True):
        with new_store(ctx, tips[0]) as store:
            for k, (arch, adds, recs) in enumerate(blocks):
                job, statuses = store.update(*block_args(arch.msa(), adds, recs))
                assert job[1] == R.OK and set(statuses) == {R.OK}
                if reading:
                    same_witnesses(store.read(), [(R.OK, w) for w in tips[k + 1]], f"forward {k}")
            same_witnesses(store.read(), [(R.OK, w) for w in tips[3]], "the tip")
            for k in (2, 1, 0):
                arch, adds, recs = blocks[k]
                job, statuses = store.revert(*block_args(arch.msa(), adds, recs), expected=C.to_msa(msas[k + 1]))
                assert job[:3] == (True, R.OK, None) and set(statuses) == {R.OK}, k
                if reading:
                    same_witnesses(store.read(), [(R.OK, w) for w in tips[k]], f"back {k}")
            same_witnesses(store.read(), [(R.OK, w) for w in tips[0]], "the fork point")
            job, statuses = store.update(*block_args(blocks[0][0].msa(), other_adds, other_recs))
            assert job[1] == R.OK and A.same(C.back_msa(job[3]), fork.msa()) and set(statuses) == {R.OK}
            same_witnesses(store.read(), [(R.OK, w) for w in fork_tip], "the other fork")


def test_sticky_through_a_revert_and_newly_failed_becomes_sticky(ctx, cases):
    c = cases
    arch0, adds, recs = c.arch, c.adds20, c.twelve[:2]
    arch1 = advance(arch0, adds, recs)
    good = [U.proof_witness(arch0, i) for i in c.live[:24:3]]
    victim = next(k for k, w in enumerate(good) if w.target_chunks and w.target_chunks[0][1])
    forged = copy.deepcopy(good[victim])
    ci, path, ch = forged.target_chunks[0]
    forged.target_chunks[0] = (ci, [C.flip(path[0])] + list(path[1:]), ch)
    wits = good[:victim] + [forged] + good[victim + 1:]
    born = U.proof_witness(arch1, 607)
    late = U.proof_witness(arch1, c.live[30])
    with new_store(ctx, wits) as store:
        job, statuses = store.update(*block_args(arch0.msa(), adds, recs))
        assert job[1] == R.OK and [k for k, st in enumerate(statuses) if st != R.OK] == [victim]
        assert statuses[victim] == R.BAD_MMR_PATH
        store.append([C.to_witness(born), C.to_witness(late)])
        W = len(store)
        job, statuses = store.revert(*block_args(arch0.msa(), adds, recs), expected=C.to_msa(arch1.msa()))
        assert job[1] == R.OK
        want = [(R.OK, w) for w in good] + [(R.NOT_IN_AOCL, None), (R.OK, U.proof_witness(arch0, c.live[30]))]
        want[victim] = (R.BAD_MMR_PATH, None)  # sticky through the revert
        assert statuses == [st for st, _ in want] and len(statuses) == W
        got = store.read()
        same_witnesses(got, want, "after the revert")
        # the newly failed one is sticky from here on
        job, statuses = store.update(*block_args(arch0.msa(), adds, recs))
        assert job[1] == R.OK and statuses[W - 2] == R.NOT_IN_AOCL and statuses[victim] == R.BAD_MMR_PATH
        assert [st for k, st in enumerate(statuses) if k not in (victim, W - 2)] == [R.OK] * (W - 2)
        verdicts = store.check(C.to_msa(arch1.msa()))
        assert verdicts[W - 2] == (False, False, False, R.NOT_IN_AOCL) and verdicts[W - 1][:2] == (True, True)


def test_rejected_jobs_and_a_wrong_tip_leave_the_store_unchanged(ctx, cases):
    c = cases
    rej, nb = c.rejected_jobs, c.neighbours[0]
    assert [cs.want[0][:3] for cs in rej] == [(False, R.ALREADY_REMOVED, 1), (False, A.DUPLICATE_RECORD, 2),
                                              (False, A.UPDATE_IMPOSSIBLE, 1)]
    after = [w for _, w in nb.want[1]]
    with new_store(ctx, after) as store:
        before, counts = raw(store), store.counts()
        for cs in rej:  # rules 2.b, 2.c, 2.d
            job, statuses = store.revert(*block_args(cs.msa, cs.adds, cs.recs))
            assert job[:3] == cs.want[0][:3] and statuses == [V.JOB_REJECTED] * len(after)
            assert raw(store) == before and store.counts() == counts
        # 2.e: the block is fine, but it did not lead to the accumulator given as the tip
        msa, upd = block_args(nb.msa, nb.adds, nb.recs)
        job, statuses = store.revert(msa, upd, expected=msa)
        assert job[:2] == (False, A.UPDATE_MISMATCH) and statuses == [V.JOB_REJECTED] * len(after)
        assert raw(store) == before and store.counts() == counts
        job, statuses = store.revert(msa, upd, expected=C.to_msa(nb.want[0][3]))
        assert job[1] == R.OK and statuses == [R.OK] * len(after)
        same_witnesses(store.read(), [(R.OK, w) for w in nb.wits])


def test_argument_errors_leave_everything_untouched(ctx, mini):
    from neptune_hip import _lib as L
    from neptune_hip import mutator_set as MS
    lib = ctx.lib
    after = [w for _, w in mini.want[1]][:20]
    with new_store(ctx, after) as store:
        W = len(store)
        before, counts = raw(store), store.counts()
        pa = MS.PackedApply([block_args(mini.msa, mini.adds, mini.recs)] * 2)
        status = np.full(W, 0xAB, dtype=np.uint8)

        def revert(n_jobs, out=ctypes.byref(pa.cout), **kw):
            cin = L.MsApplyIn(*(getattr(pa.cin, f) for f, _ in L.MsApplyIn._fields_))
            cin.n_jobs = n_jobs
            for f, v in kw.items():
                setattr(cin, f, v)
            return lib.nhip_ms_store_revert(store._h, ctypes.byref(cin), out, status.ctypes.data)

        assert revert(0) == L.NHIP_ERR_ARG and revert(2) == L.NHIP_ERR_ARG
        assert revert(1, out=None) == L.NHIP_ERR_ARG and revert(1, add_off=None) == L.NHIP_ERR_ARG
        assert lib.nhip_ms_store_revert(store._h, None, ctypes.byref(pa.cout), status.ctypes.data) == L.NHIP_ERR_ARG
        assert lib.nhip_ms_store_revert(None, ctypes.byref(pa.cin), ctypes.byref(pa.cout), status.ctypes.data) == L.NHIP_ERR_ARG
        assert (status == 0xAB).all() and not pa.arrays["status"].any() and not pa.arrays["aocl_num_leafs"].any()
        assert raw(store) == before and store.counts() == counts
        # the batch form: a missing output, a capacity one short
        pu = MS.PackedUpdate([(C.to_msa(mini.msa), block_args(mini.msa, mini.adds, mini.recs)[1],
                               [C.to_witness(w) for w in after])], revert=True)
        assert pu.run(lib) == L.NHIP_OK
        for a in pu.out.values():
            a.reshape(-1).view(np.uint8)[:] = 0xCD
        short = L.MsUpdated(*(getattr(pu.cout, g) for g, _ in L.MsUpdated._fields_))
        short.path_cap -= 1
        args = (ctypes.byref(pu.apply.cin), ctypes.byref(pu.apply.cout), ctypes.byref(pu.win))
        assert lib.nhip_ms_revert_batch(ctx.handle, *args, ctypes.byref(short)) == L.NHIP_ERR_ARG
        assert lib.nhip_ms_revert_batch(ctx.handle, *args, None) == L.NHIP_ERR_ARG
        assert lib.nhip_ms_revert_batch(None, *args, ctypes.byref(pu.cout)) == L.NHIP_ERR_ARG
        assert all((a.reshape(-1).view(np.uint8) == 0xCD).all() for a in pu.out.values())
        # the statuses may be left out: the revert is the same
        one = MS.PackedApply([block_args(mini.msa, mini.adds, mini.recs)])
        assert lib.nhip_ms_store_revert(store._h, ctypes.byref(one.cin), ctypes.byref(one.cout), None) == L.NHIP_OK
        assert int(one.arrays["status"][0]) == R.OK
        same_witnesses(store.read(), [(R.OK, w) for w in mini.wits[:20]])
    # an empty store: the block part alone
    with MS.WitnessStore(ctx) as store:
        job, statuses = store.revert(*block_args(mini.msa, mini.adds, mini.recs))
        assert job[1] == R.OK and statuses == [] and A.same(C.back_msa(job[3]), mini.want[0][3])


def test_revert_membership_proofs(ctx, cases):
    """The wallet's call: items and proofs in, the index sets and leaves derived on the device."""
    from neptune_hip import mutator_set as MS
    cs = cases.both
    b = back_of(cs)
    arch_after = advance(cs.arch, cs.adds, cs.recs)
    leafs = cases.live[:12] + [603]
    items = [arch_after.items[l][0] for l in leafs]
    mps = [arch_after.membership_proof(l) for l in leafs]
    proofs = [MS.MsMembershipProof(m.sender_randomness, m.receiver_preimage, m.auth_path_aocl, m.aocl_leaf_index,
                                   C._chunks(m.target_chunks)) for m in mps]
    msa, upd = block_args(cs.msa, cs.adds, cs.recs)
    status, after, out = MS.revert_membership_proofs(ctx, msa, upd, items, proofs)
    assert status == R.OK and A.same(C.back_msa(after), b.want[0][3])
    assert [st for st, _ in out] == [R.OK] * 12 + [R.NOT_IN_AOCL]
    for l, (_, p) in zip(leafs[:12], out):
        want = cs.arch.membership_proof(l)
        assert [tuple(int(x) for x in d) for d in p.auth_path_aocl] == [tuple(d) for d in want.auth_path_aocl]
        got_tc = [(int(ci), [tuple(int(x) for x in d) for d in path], [int(x) for x in ch.relative_indices])
                  for ci, path, ch in p.target_chunks]
        assert got_tc == [(ci, [tuple(d) for d in path], list(ch.relative_indices)) for ci, path, ch in want.target_chunks]
