"""GPU batched mutator-set updates (k_ms_chunk_auth_jobs, k_ms_records_jobs, k_ms_apply behind
nhip_ms_apply_batch) against the CPU restatement tests/ms_apply_ref.py over `ms_ref.Archival`, never against
themselves: Block::validate rules 2.b-2.e and Block::mutator_set_accumulator_after.  The archival sets, the jobs
and their expected outcomes are built once per module (`cases`) and left unchanged; each test asserts that its
jobs exercise what it claims."""
import copy
import ctypes
import itertools
import random

import numpy as np
import pytest

import ms_apply_ref as A
import ms_ref as R

pytestmark = pytest.mark.gpu

P = R.P


def _digest(rng):
    return tuple(rng.randrange(P) for _ in range(5))


def _flip(d, word=2):
    d = list(d)
    d[word] = (d[word] + 1) % P
    return tuple(d)


# ---------------------------------------------------------------- ms_ref -> neptune_hip types and back
def to_mmr(m):
    from neptune_hip.mutator_set import MmrAccumulator
    return MmrAccumulator(list(m.peaks), m.num_leafs)


def to_msa(msa):
    from neptune_hip.mutator_set import MutatorSetAccumulator
    return MutatorSetAccumulator(to_mmr(msa.aocl), to_mmr(msa.swbf_inactive), list(msa.swbf_active))


def to_record(r):
    from neptune_hip.mast import AbsoluteIndexSet
    from neptune_hip.mutator_set import Chunk, RemovalRecord
    return RemovalRecord(AbsoluteIndexSet(r.absolute_indices.minimum, list(r.absolute_indices.distances)),
                         [(ci, list(path), Chunk(list(c.relative_indices))) for ci, path, c in r.target_chunks])


def back(msa):
    if msa is None:
        return None
    return R.Msa(R.Mmr([tuple(d) for d in msa.aocl.peaks], msa.aocl.num_leafs),
                 R.Mmr([tuple(d) for d in msa.swbf_inactive.peaks], msa.swbf_inactive.num_leafs),
                 list(msa.swbf_active))


# ---------------------------------------------------------------- the jobs
class Case:
    """One job: the archival set behind `msa` (None for a synthetic accumulator), the update, the expected
    accumulator handed to the device (or None), and the helper's outcome `want`."""

    def __init__(self, label, arch, msa, adds, recs, expected=None, want=None):
        self.label, self.arch, self.msa, self.adds, self.recs, self.expected = label, arch, msa, adds, recs, expected
        self.want = want if want is not None else A.outcome(arch, msa, adds, recs, expected)

    def gpu(self):
        from neptune_hip.mutator_set import MutatorSetUpdate
        return to_msa(self.msa), MutatorSetUpdate([to_record(r) for r in self.recs], [A.commitment(*it) for it in self.adds])


def _items(rng, k):
    return [(_digest(rng), _digest(rng), _digest(rng)) for _ in range(k)]


def _build(n, seed, every=15):
    """An archival set of n additions with removals spread through them (as test_gpu_mutator_set.py's)."""
    rng = random.Random(seed)
    arch, removed = R.Archival(), []
    for k in range(n):
        arch.add(_digest(rng), _digest(rng), _digest(rng))
        if k % every == every - 1:
            victim = rng.randrange(k) if k % (2 * every) == every - 1 else k - 3
            if victim not in removed:
                arch.remove(arch.removal_record(victim))
                removed.append(victim)
    return arch, removed


def _forged(rec):
    """The same index set in another order: equal to `rec` for rule 2.d, distinct from it for rule 2.c."""
    m = copy.deepcopy(rec)
    d = m.absolute_indices.distances
    i = next(i for i in range(1, 45) if d[i] != d[0])
    d[0], d[i] = d[i], d[0]
    return m


class Cases:
    pass


@pytest.fixture(scope="module")
def cases():
    c = Cases()
    rng = random.Random(31)
    arch, removed = _build(600, 2025)
    msa = arch.msa()
    assert msa.batch_index == 74 and len(removed) >= 35 and len(msa.swbf_active) > 500
    live = [i for i in range(600) if i not in removed]
    c.arch, c.msa, c.removed, c.live = arch, msa, removed, live

    # additions only
    c.adds600 = [Case(f"600 + {k}", arch, msa, _items(rng, k), []) for k in (0, 1, 7, 8, 9, 300, 2100)]
    c.small = []
    c.small_sets = {}
    for n0 in (0, 1, 8, 255, 256):
        a, _ = _build(n0, 500 + n0, every=4)
        c.small_sets[n0] = a
        for k in (1, 9):
            c.small.append(Case(f"{n0} + {k}", a, a.msa(), _items(rng, k), []))

    # removals only, and both
    low = [i for i in live if i < 100][:12]
    c.twelve = [arch.removal_record(i) for i in low]
    c.one = Case("one removal", arch, msa, [], c.twelve[:1])
    c.removals = Case("twelve removals", arch, msa, [], c.twelve)
    c.both = Case("20 additions, twelve removals", arch, msa, _items(rng, 20), c.twelve)

    # rejections
    recs = c.twelve[:3]
    flipped = copy.deepcopy(recs)
    ci, path, chunk = next(e for e in flipped[1].target_chunks if e[1])
    pos = [e[0] for e in flipped[1].target_chunks].index(ci)
    flipped[1].target_chunks[pos] = (ci, [_flip(path[0])] + list(path[1:]), chunk)
    dropped = copy.deepcopy(recs)
    del dropped[2].target_chunks[0]
    forged = _forged(recs[0])
    off_leafs = R.Msa(msa.aocl, R.Mmr(msa.swbf_inactive.peaks, msa.swbf_inactive.num_leafs + 1), msa.swbf_active)
    off_peaks = R.Msa(R.Mmr(list(msa.aocl.peaks) + [_digest(rng)], msa.aocl.num_leafs), msa.swbf_inactive, msa.swbf_active)
    c.rejected = [
        Case("path digest flipped", arch, msa, [], flipped),
        Case("entry dropped", arch, msa, _items(rng, 2), dropped),
        Case("same record twice", arch, msa, [], [recs[0], recs[1], recs[0]]),
        Case("forged second record", arch, msa, [], [recs[0], forged]),
        Case("forged first record", arch, msa, [], [forged, recs[1], recs[0]]),
        Case("swbf num_leafs off by one", arch, off_leafs, _items(rng, 1), recs),
        Case("aocl n_peaks off by one", arch, off_peaks, [], recs),
    ]

    # rule 2.e on the job with additions and removals
    right = c.both.want[3]
    assert len(right.swbf_active) > 100 and right.swbf_active == sorted(right.swbf_active)

    def edit(**kw):
        m = copy.deepcopy(right)
        for name, f in kw.items():
            setattr(m, name, f(getattr(m, name)))
        return m

    c.rule_2e = [Case(label, arch, msa, c.both.adds, c.twelve, expected=e) for label, e in (
        ("expected right", right),
        ("aocl peak word", edit(aocl=lambda m: R.Mmr([_flip(m.peaks[0], 4)] + m.peaks[1:], m.num_leafs))),
        ("swbf peak word", edit(swbf_inactive=lambda m: R.Mmr(m.peaks[:-1] + [_flip(m.peaks[-1], 0)], m.num_leafs))),
        ("num_leafs", edit(aocl=lambda m: R.Mmr(m.peaks, m.num_leafs ^ 1))),
        ("window word", edit(swbf_active=lambda w: w[:7] + [w[7] + 1] + w[8:])),
        ("window word dropped", edit(swbf_active=lambda w: w[:-1])),
        ("window descending", edit(swbf_active=lambda w: w[::-1])),
    )]

    # 64-bit arithmetic: accumulators whose leaves cannot be materialised
    n0 = (1 << 40) + 5
    big = R.Msa(R.Mmr([_digest(rng) for _ in range(3)], n0), R.Mmr([_digest(rng)], (n0 - 1) // 8),
                sorted([5, 100, 4095, 4096] + [rng.randrange(1 << 20) for _ in range(46)]))
    big_adds = _items(rng, 9)
    after = big
    for it in big_adds:
        after = A.msa_add(after, A.commitment(*it))
    assert after.swbf_inactive.num_leafs == (1 << 37) + 1 and len(after.swbf_active) <= 47
    full = R.Msa(R.Mmr([_digest(rng) for _ in range(64)], (1 << 64) - 1),
                 R.Mmr([_digest(rng) for _ in range(61)], ((1 << 64) - 2) // 8), [])
    c.wide = [Case("2^40 + 5 leaves, 9 additions", None, big, big_adds, [], want=(True, R.OK, None, after)),
              Case("2^64 - 1 leaves, 1 addition", None, full, _items(rng, 1), [], want=(False, A.INCONSISTENT, None, None))]

    # single-record jobs, accepted (a live item) and rejected in rule 2.b (a removed one) in turn, from the
    # set of 600 and from the small sets
    c.singles = []
    for k in range(28):
        i = removed[k] if k % 2 else live[20 + k]
        c.singles.append(Case(f"record of item {i}", arch, msa, _items(rng, k % 3), [arch.removal_record(i)]))
    for n0 in (8, 255, 256):
        a = c.small_sets[n0]
        for i in (0, n0 - 1, n0 - 2):
            c.singles.append(Case(f"{n0}: record of item {i}", a, a.msa(), _items(rng, 1), [a.removal_record(i)]))
    return c


def run(ctx, group):
    """The jobs of `group` in one call; every output against the helper's.  Returns the device's results."""
    from neptune_hip.mutator_set import apply_update_batch
    expected = None
    if any(cs.expected is not None for cs in group):
        # one call takes an expected accumulator for every job or for none
        expected = [to_msa(cs.expected if cs.expected is not None else (cs.want[3] or cs.msa)) for cs in group]
    got = apply_update_batch(ctx, [cs.gpu() for cs in group], expected)
    for cs, g in zip(group, got):
        assert g[:3] == cs.want[:3], (cs.label, g[:3], cs.want[:3])
        if cs.want[3] is None:
            assert g[3] is None, cs.label
        else:
            assert A.same(back(g[3]), cs.want[3]), cs.label
    return got


# ---------------------------------------------------------------- additions only
def test_additions_only_from_the_set_of_600(ctx, cases):
    group = cases.adds600
    assert [len(cs.adds) for cs in group] == [0, 1, 7, 8, 9, 300, 2100]
    assert all(cs.want[:3] == (True, R.OK, None) for cs in group)
    slides = [cs.want[3].swbf_inactive.num_leafs - 74 for cs in group]
    assert slides == [0, 1, 1, 1, 2, 38, 263]  # item 600 slides the window; 263 slides pass its 256 chunks
    last = group[-1]
    arch = A.clone(cases.arch)
    for it in last.adds:
        arch.add(*it)
    assert all(not arch.bloom.get(74 + c) for c in range(256, 263)) and any(arch.bloom.get(74 + c) for c in range(256))
    assert last.want[3].swbf_active == [] and group[0].want[3].swbf_active == cases.msa.swbf_active
    run(ctx, group)


def test_additions_at_small_sizes(ctx, cases):
    group = cases.small
    by = {cs.label: cs for cs in group}
    assert by["0 + 1"].want[3].swbf_inactive.num_leafs == 0 and by["1 + 9"].want[3].swbf_inactive.num_leafs == 1
    assert by["8 + 1"].want[3].swbf_inactive.num_leafs == 1 and by["8 + 1"].msa.swbf_inactive.num_leafs == 0  # the first slide
    assert len(by["255 + 1"].msa.aocl.peaks) == 8 and len(by["255 + 1"].want[3].aocl.peaks) == 1  # eight peaks merge
    assert len(by["256 + 9"].want[3].aocl.peaks) == 3
    assert sum(1 for cs in group if cs.msa.swbf_active) >= 6  # the slid chunks are not all empty
    run(ctx, group)


# ---------------------------------------------------------------- removals, and both
def test_removals_only(ctx, cases):
    msa = cases.msa
    per_record = [{i // R.CHUNK_SIZE for i in r.absolute_indices.to_array() if i // R.CHUNK_SIZE < 74} for r in cases.twelve]
    touched = set().union(*per_record)
    assert any(sum(ci in s for s in per_record) >= 2 for ci in touched)         # a chunk with indices of two records
    assert any(ci % 2 == 0 and ci + 1 in touched for ci in touched)             # siblings 2j, 2j + 1
    assert len(msa.swbf_inactive.peaks) == 3                                    # 74 = 64 + 8 + 2
    assert sum(1 for lo, hi in ((0, 64), (64, 72), (72, 74)) if any(lo <= ci < hi for ci in touched)) >= 2
    assert cases.one.want[:3] == cases.removals.want[:3] == (True, R.OK, None)
    assert cases.removals.want[3].swbf_inactive.peaks != msa.swbf_inactive.peaks
    assert len(cases.removals.want[3].swbf_active) > len(msa.swbf_active)
    run(ctx, [cases.one, cases.removals])


def test_additions_and_removals(ctx, cases):
    cs, msa = cases.both, cases.msa
    after = cs.want[3]
    assert cs.want[:3] == (True, R.OK, None) and after.batch_index == 77
    chunks = [i // R.CHUNK_SIZE for r in cases.twelve for i in r.absolute_indices.to_array()]
    slid = [ci for ci in chunks if 74 <= ci < 77]
    assert slid and any(any((ci - 74) * R.CHUNK_SIZE <= x < (ci - 73) * R.CHUNK_SIZE for x in msa.swbf_active) for ci in slid)
    assert any(ci >= 77 for ci in chunks)
    run(ctx, [cs])


# ---------------------------------------------------------------- rejections
def test_rejections_name_the_rule_and_the_record(ctx, cases):
    want = {cs.label: cs.want[:3] for cs in cases.rejected}
    assert want == {
        "path digest flipped": (False, R.BAD_MMR_PATH, 1),
        "entry dropped": (False, R.ABSENT_CHUNK, 2),
        "same record twice": (False, A.DUPLICATE_RECORD, 2),
        "forged second record": (False, A.UPDATE_IMPOSSIBLE, 1),
        "forged first record": (False, A.UPDATE_IMPOSSIBLE, 2),  # the other order blames the other record
        "swbf num_leafs off by one": (False, A.INCONSISTENT, None),
        "aocl n_peaks off by one": (False, A.INCONSISTENT, None),
    }
    forged = cases.rejected[3].recs[1]
    assert all(R.can_remove(cases.msa, r)[1] for r in cases.rejected[3].recs) and A.distinct(cases.rejected[3].recs) is None
    assert sorted(forged.absolute_indices.to_array()) == sorted(cases.twelve[0].absolute_indices.to_array())
    run(ctx, cases.rejected)


def test_rule_2e_compares_every_field(ctx, cases):
    want = [cs.want[:2] for cs in cases.rule_2e]
    assert want == [(True, R.OK)] + [(False, A.UPDATE_MISMATCH)] * 6
    assert sorted(cases.rule_2e[-1].expected.swbf_active) == cases.both.want[3].swbf_active
    run(ctx, cases.rule_2e)


def test_64_bit_leaf_counts(ctx, cases):
    run(ctx, cases.wide)


# ---------------------------------------------------------------- one call of 70 jobs
def test_one_call_of_70_jobs_equals_the_jobs_alone(ctx, cases):
    from neptune_hip.mutator_set import PackedApply, apply_update_batch
    pools = [cases.adds600 + cases.small + [cases.one, cases.removals, cases.both] + cases.rule_2e + cases.wide,
             cases.rejected + cases.singles]
    # accepted and rejected jobs interleaved
    group = [cs for pair in itertools.zip_longest(*pools) for cs in pair if cs is not None][:70]
    assert len(group) == 70
    sizes = {cs.msa.aocl.num_leafs for cs in group}
    assert len(sizes) >= 7
    verdicts = [cs.want[0] for cs in group]
    assert verdicts.count(True) >= 25 and verdicts.count(False) >= 25
    assert {cs.want[1] for cs in group} >= {R.OK, R.BAD_MMR_PATH, R.ABSENT_CHUNK, R.ALREADY_REMOVED, A.INCONSISTENT,
                                            A.DUPLICATE_RECORD, A.UPDATE_IMPOSSIBLE, A.UPDATE_MISMATCH}
    got = run(ctx, group)
    for cs, g in zip(group, got):
        exp = None if cs.expected is None else [to_msa(cs.expected)]
        alone = apply_update_batch(ctx, [cs.gpu()], exp)[0]
        assert alone[:3] == g[:3], cs.label
        assert (alone[3] is None) == (g[3] is None), cs.label
        if g[3] is not None:
            assert A.same(back(alone[3]), back(g[3])), cs.label
    # the same call twice on one context: equal bytes
    expected = [to_msa(cs.expected if cs.expected is not None else (cs.want[3] or cs.msa)) for cs in group]
    outs = []
    for _ in range(2):
        pa = PackedApply([cs.gpu() for cs in group], expected)
        assert pa.call(ctx) == 0
        a = pa.arrays
        blob = [a[f].tobytes() for f in ("verdict", "status", "bad_record", "aocl_n_peaks", "aocl_num_leafs",
                                         "swbf_n_peaks", "swbf_num_leafs", "n_active")]
        for j in range(70):
            blob.append(a["aocl_peaks"][j, :int(a["aocl_n_peaks"][j])].tobytes())
            blob.append(a["swbf_peaks"][j, :int(a["swbf_n_peaks"][j])].tobytes())
            lo = int(a["active_off"][j])
            blob.append(a["active"][lo:lo + int(a["n_active"][j])].tobytes())
        outs.append(b"".join(blob))
    assert outs[0] == outs[1]


# ---------------------------------------------------------------- block helpers
def test_block_helpers(ctx, cases):
    from neptune_hip import blocks
    from neptune_hip import mutator_set as MS
    cs = cases.both
    msa, recs = to_msa(cases.msa), [to_record(r) for r in cases.twelve]
    adds = [A.commitment(*it) for it in cs.adds]
    claimed = to_msa(cs.want[3])
    assert blocks.mutator_set_update_valid(ctx, msa, recs, adds, claimed) == (True, MS.OK)
    gone = to_record(cases.arch.removal_record(cases.removed[0]))
    assert blocks.mutator_set_update_valid(ctx, msa, recs[:2] + [gone], adds, claimed) == (False, MS.ALREADY_REMOVED)
    assert blocks.mutator_set_update_valid(ctx, msa, recs + recs[:1], adds, claimed) == (False, MS.DUPLICATE_RECORD)
    forged = to_record(_forged(cases.twelve[0]))
    assert blocks.mutator_set_update_valid(ctx, msa, recs + [forged], adds, claimed) == (False, MS.UPDATE_IMPOSSIBLE)
    assert blocks.mutator_set_update_valid(ctx, msa, recs, adds[:-1], claimed) == (False, MS.UPDATE_MISMATCH)
    fee = cases.adds600[4]  # 9 guesser-fee addition records
    after = blocks.accumulator_after(ctx, msa, [A.commitment(*it) for it in fee.adds])
    assert A.same(back(after), fee.want[3])
    with pytest.raises(ValueError):
        blocks.accumulator_after(ctx, to_msa(cases.rejected[5].msa), adds)


# ---------------------------------------------------------------- shapes
def test_shape_errors_leave_the_outputs_untouched(ctx, cases):
    from neptune_hip import _lib as L
    from neptune_hip.mutator_set import PackedApply, apply_update_batch
    assert apply_update_batch(ctx, []) == []
    jobs = [cases.one.gpu(), cases.adds600[1].gpu(), cases.rejected[2].gpu()]

    def fresh():
        pa = PackedApply(jobs)
        for name in ("verdict", "status", "bad_record", "aocl_peaks", "aocl_n_peaks", "aocl_num_leafs", "swbf_peaks",
                     "swbf_n_peaks", "swbf_num_leafs", "n_active", "active"):
            pa.arrays[name].reshape(-1).view(np.uint8)[:] = 0xAB
        return pa

    def untouched(pa):
        return all((pa.arrays[name].reshape(-1).view(np.uint8) == 0xAB).all()
                   for name in ("verdict", "status", "bad_record", "aocl_peaks", "aocl_n_peaks", "aocl_num_leafs",
                                "swbf_peaks", "swbf_n_peaks", "swbf_num_leafs", "n_active", "active"))

    pa = fresh()
    assert pa.call(ctx) == L.NHIP_OK and not untouched(pa)
    assert [int(x) for x in pa.arrays["status"]] == [R.OK, R.OK, A.DUPLICATE_RECORD]
    empty = L.MsApplyIn(0, None, None, None, None, None, None, None, None)
    assert ctx.lib.nhip_ms_apply_batch(ctx.handle, ctypes.byref(empty), ctypes.byref(L.MsApplyOut())) == L.NHIP_OK
    for field in ("additions", "minimum", "msa_before", "rec_off"):  # null with a non-zero count
        pa = fresh()
        setattr(pa.cin, field, None)
        assert pa.call(ctx) == L.NHIP_ERR_ARG and untouched(pa), field
    pa = fresh()
    pa.cout.status = None
    assert pa.call(ctx) == L.NHIP_ERR_ARG and untouched(pa)
    for name in ("add_off", "rec_off"):  # offsets decreasing
        pa = fresh()
        off = pa.arrays[name]
        off[-2] = off[-1] + 1
        assert pa.call(ctx) == L.NHIP_ERR_ARG and untouched(pa), name
    pa = fresh()  # the first window's capacity one short
    off = pa.arrays["active_off"].copy()
    assert int(off[1]) == len(cases.msa.swbf_active) + 45
    off[1:] -= np.uint64(1)
    pa.cout.active_off = off.ctypes.data
    assert pa.call(ctx) == L.NHIP_ERR_ARG and untouched(pa)
