"""The jobs of tests/test_ms_update_plan.py (host plan, no GPU) and tests/test_gpu_ms_update.py — TEST HELPER ONLY
(not collected).  Every job is built on `ms_ref.Archival` sets (or `ms_update_ref.Tail` for a leaf count nobody can
materialise) with its expected outcome from tests/ms_update_ref.py, once per process (`cases()`), and left unchanged.
Witnesses and records with a wanted property are found by deterministic search over the set; the tests assert that
the search found what they claim to exercise."""
import copy
import functools
import random

import ms_apply_ref as A
import ms_ref as R
import ms_update_ref as U

P = R.P


def _digest(rng):
    return tuple(rng.randrange(P) for _ in range(5))


def flip(d, word=2):
    d = list(d)
    d[word] = (d[word] + 1) % P
    return tuple(d)


def _items(rng, k):
    return [(_digest(rng), _digest(rng), _digest(rng)) for _ in range(k)]


def build(n, seed, every=15):
    """An archival set of n additions with removals spread through them (as tests/test_gpu_ms_apply.py builds)."""
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


# ---------------------------------------------------------------- ms_ref -> neptune_hip types and back
def to_mmr(m):
    from neptune_hip.mutator_set import MmrAccumulator
    return MmrAccumulator(list(m.peaks), m.num_leafs)


def to_msa(msa):
    from neptune_hip.mutator_set import MutatorSetAccumulator
    return MutatorSetAccumulator(to_mmr(msa.aocl), to_mmr(msa.swbf_inactive), list(msa.swbf_active))


def _index_set(s):
    from neptune_hip.mast import AbsoluteIndexSet
    return AbsoluteIndexSet(s.minimum, list(s.distances))


def _chunks(tc):
    from neptune_hip.mutator_set import Chunk
    return [(ci, list(path), Chunk(list(c.relative_indices))) for ci, path, c in tc]


def to_record(r):
    from neptune_hip.mutator_set import RemovalRecord
    return RemovalRecord(_index_set(r.absolute_indices), _chunks(r.target_chunks))


def to_witness(w):
    from neptune_hip.mutator_set import Witness
    return Witness(_index_set(w.absolute_indices), _chunks(w.target_chunks), w.aocl_leaf_index, list(w.aocl_leaf),
                   list(w.auth_path_aocl))


def back_msa(msa):
    if msa is None:
        return None
    return R.Msa(R.Mmr([tuple(d) for d in msa.aocl.peaks], msa.aocl.num_leafs),
                 R.Mmr([tuple(d) for d in msa.swbf_inactive.peaks], msa.swbf_inactive.num_leafs),
                 list(msa.swbf_active))


def plain(w):
    """A witness (either library's or the helper's) as plain comparable data."""
    if w is None:
        return None
    return (w.absolute_indices.minimum, tuple(w.absolute_indices.distances), w.aocl_leaf_index,
            tuple(int(x) for x in w.aocl_leaf) if w.aocl_leaf_index is not None else (),
            [tuple(int(x) for x in d) for d in w.auth_path_aocl],
            [(int(ci), [tuple(int(x) for x in d) for d in path], [int(x) for x in c.relative_indices])
             for ci, path, c in w.target_chunks])


class Case:
    """One job: the archival set behind `msa`, the update, the witnesses, and the helper's answer `want` =
    (job outcome, [(status, witness after or None)])."""

    def __init__(self, label, arch, msa, adds, recs, wits, want=None):
        self.label, self.arch, self.msa, self.adds, self.recs, self.wits = label, arch, msa, adds, recs, wits
        self.want = want if want is not None else U.outcome(arch, msa, adds, recs, wits)
        self.commitments = [A.commitment(*it) for it in adds]

    def gpu(self):
        from neptune_hip.mutator_set import MutatorSetUpdate
        return (to_msa(self.msa), MutatorSetUpdate([to_record(r) for r in self.recs], self.commitments),
                [to_witness(w) for w in self.wits])

    @property
    def n1(self):
        return self.msa.aocl.num_leafs + len(self.adds)

    @property
    def b1(self):
        return U.batch_after(self.msa, len(self.adds))


class Cases:
    pass


def chunks_of(index_set, below):
    return sorted({i // R.CHUNK_SIZE for i in index_set.to_array() if i // R.CHUNK_SIZE < below})


@functools.lru_cache(maxsize=1)
def cases():
    c = Cases()
    rng = random.Random(47)
    arch, removed = build(600, 2025)
    msa = arch.msa()
    assert msa.batch_index == 74
    live = [i for i in range(600) if i not in removed]
    c.arch, c.msa, c.removed, c.live = arch, msa, removed, live
    proofs = {i: U.proof_witness(arch, i) for i in live}
    rec_of = live[5:200:10][:20]
    records20 = [U.record_witness(arch, i) for i in rec_of]
    assert len(records20) == 20
    everyone = [proofs[i] for i in live] + records20
    c.everyone_leafs = list(live) + [None] * 20

    # 1. additions only
    c.adds300 = _items(rng, 300)
    c.adds600 = [Case(f"600 + {k}", arch, msa, c.adds300[:k], [], everyone) for k in (0, 1, 9, 300)]
    arch601 = A.clone(arch)
    arch601.add(*_items(rng, 1)[0])
    live601 = live + [600]
    c.arch601 = arch601
    c.adds601 = Case("601 + 3", arch601, arch601.msa(), _items(rng, 3), [],
                     [U.proof_witness(arch601, i) for i in live601] + [U.record_witness(arch601, i) for i in rec_of])

    # 2. small sets
    c.small, c.small_sets = [], {}
    for n0 in (1, 8, 9, 255, 256):
        seed = 500 + n0
        while True:  # for the set of 8: one whose first slide ever gives a live item its first dictionary entry
            a, gone = build(n0, seed, every=4)
            alive = [i for i in range(n0) if i not in gone]
            if n0 != 8 or any(0 in chunks_of(a.index_set(i), 1) for i in alive):
                break
            seed += 1000
        c.small_sets[n0] = (a, gone)
        wits = [U.proof_witness(a, i) for i in alive] + [U.record_witness(a, i) for i in alive[:4]]
        for k in (1, 9):
            c.small.append(Case(f"{n0} + {k}", a, a.msa(), _items(rng, k), [], wits))

    # light jobs for the call of thirty: three additions, and a single record, on the small sets
    c.extra = []
    for n0 in (1, 8, 9, 255, 256):
        a, gone = c.small_sets[n0]
        alive = [i for i in range(n0) if i not in gone]
        wits = [U.proof_witness(a, i) for i in alive[-6:]] + [U.record_witness(a, i) for i in alive[:2]]
        c.extra.append(Case(f"{n0} + 3", a, a.msa(), _items(rng, 3), [], wits))
        if n0 >= 255:
            c.extra.append(Case(f"{n0} + 2, one removal", a, a.msa(), _items(rng, 2), [a.removal_record(alive[1])], wits))

    # 3. removals only: the job's own records as witnesses too
    low = [i for i in live if i < 100][:12]
    c.low = low
    c.twelve = [arch.removal_record(i) for i in low]
    own = [U.as_witness(r) for r in c.twelve]
    c.one = Case("one removal", arch, msa, [], c.twelve[:1], everyone + own[:1])
    c.removals = Case("twelve removals", arch, msa, [], c.twelve, everyone + own)

    # 4. both
    c.adds20 = _items(rng, 20)
    c.both = Case("20 additions, twelve removals", arch, msa, c.adds20, c.twelve, everyone + own)

    # 5. born in the block (the k = 300 job; its items are leaves 600 .. 899)
    after300 = A.clone(arch)
    for it in c.adds300:
        after300.add(*it)
    c.born_at = [600, 601, 750, 898, 899]
    born = [U.Wit(after300.index_set(l), [], l, R.aocl_leaf(*after300.items[l]), []) for l in c.born_at]
    c.born = Case("600 + 300, born in the block", arch, msa, c.adds300, [], [proofs[live[0]]] + born + [proofs[live[1]]])

    # 6. one rejection per witness status, each between good witnesses
    good = [proofs[i] for i in live[:40:4]]
    rich = next(w for w in good if len(w.target_chunks) >= 3 and all(len(e[1]) for e in w.target_chunks))
    other = next(w for w in good if w is not rich and w.target_chunks)

    def edit(w, **kw):
        m = copy.deepcopy(w)
        for name, f in kw.items():
            setattr(m, name, f(getattr(m, name)))
        return m

    def swap(tc):
        return [tc[1], tc[0]] + tc[2:]

    def word(tc):
        ci, path, chunk = tc[0]
        rel = list(chunk.relative_indices)
        rel = [rel[0] ^ 1] + rel[1:] if rel else [7]
        return [(ci, path, R.Chunk(rel))] + tc[1:]

    extra = next(e for e in other.target_chunks if e[0] not in [x[0] for x in rich.target_chunks])
    born_wrong = U.Wit(after300.index_set(600), [], 600, flip(R.aocl_leaf(*after300.items[600])), [])
    c.mutants = [
        ("saturating index set", R.OUT_OF_RANGE, edit(rich, absolute_indices=lambda s: R.IndexSet((1 << 128) - 5, s.distances))),
        ("entry dropped", R.ABSENT_CHUNK, edit(rich, target_chunks=lambda tc: tc[1:])),
        ("entry extra", R.ABSENT_CHUNK, edit(rich, target_chunks=lambda tc: sorted(tc + [extra], key=lambda e: e[0]))),
        ("entries swapped", R.ABSENT_CHUNK, edit(rich, target_chunks=swap)),
        ("path digest flipped", R.BAD_MMR_PATH,
         edit(rich, target_chunks=lambda tc: [(tc[0][0], [flip(tc[0][1][0])] + list(tc[0][1][1:]), tc[0][2])] + tc[1:])),
        ("chunk word changed", R.BAD_MMR_PATH, edit(rich, target_chunks=word)),
        ("aocl digest flipped", R.NOT_IN_AOCL, edit(rich, auth_path_aocl=lambda p: [flip(p[0])] + list(p[1:]))),
        ("leaf index past the block", R.NOT_IN_AOCL, edit(rich, aocl_leaf_index=lambda l: 609)),
        ("born with a wrong leaf", R.NOT_IN_AOCL, born_wrong),
    ]
    with_bad = []
    for k, (_, _, m) in enumerate(c.mutants):
        with_bad += [good[k], m]
    with_bad.append(good[9])
    c.mutant_at = list(range(1, 18, 2))
    c.reject_adds = c.adds300[:9]
    c.with_mutants = Case("nine rejected witnesses", arch, msa, c.reject_adds, c.twelve[:2], with_bad)
    c.without_mutants = Case("the good witnesses alone", arch, msa, c.reject_adds, c.twelve[:2], good[:10])

    recs = c.twelve[:3]
    gone = arch.removal_record(removed[0])
    forged = copy.deepcopy(recs[0])
    d = forged.absolute_indices.distances
    i = next(i for i in range(1, 45) if d[i] != d[0])
    d[0], d[i] = d[i], d[0]
    c.rejected_jobs = [
        Case("2.b: a record already removed", arch, msa, c.adds20[:2], [recs[0], gone], good[:5]),
        Case("2.c: the same record twice", arch, msa, [], [recs[0], recs[1], recs[0]], good[:5]),
        Case("2.d: a forged record", arch, msa, c.adds20[:1], [recs[0], forged], good[:5]),
    ]
    c.neighbours = [Case("neighbour before", arch, msa, c.adds20[:2], recs[:1], good[:5]),
                    Case("neighbour after", arch, msa, [], recs[1:], good[3:8])]

    # 7. 2^40 + 5 leaves
    base = 1 << 40
    pool = _items(rng, 60)
    inside = []  # items whose index sets stay inside the window when the batch index goes from 2^37 to 2^37 + 1
    for it in pool:
        local = len(inside)
        if local == 14:
            break
        rel = R.absolute_index_set(*it, base + local)
        lo = rel[0] - ((base + local) // 8) * R.CHUNK_SIZE
        if lo >= R.CHUNK_SIZE:
            inside.append(it)
    assert len(inside) == 14
    window = sorted(rng.randrange(R.CHUNK_SIZE, 1 << 20) for _ in range(50))
    tail = U.Tail(base, _digest(rng), _digest(rng), inside[:5], window)
    job, wits, got = tail.outcome(inside[5:], [0, 3, 4, 5, 13])
    c.tail = tail
    c.wide = Case("2^40 + 5 leaves, 9 additions", None, tail.msa(), inside[5:], [], wits, want=(job, got))
    return c


def everything(c):
    return (c.adds600 + [c.adds601] + c.small + [c.one, c.removals, c.both, c.born, c.with_mutants, c.without_mutants]
            + c.rejected_jobs + c.neighbours + [c.wide] + c.extra)
