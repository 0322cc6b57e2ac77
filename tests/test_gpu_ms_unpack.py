"""GPU unpacking of packed removal records, block rule 2.a (k_ms_unpack behind nhip_ms_unpack_batch and
nhip_ms_apply_batch_packed), against the CPU restatement tests/ms_pack_ref.py, never against itself: every job's
unpacked records equal the restatement's and the records they were packed from, and rules 2.a-2.e in one call equal
nhip_ms_apply_batch on the restatement-unpacked records.  The lists are tests/ms_pack_cases.py's, built once."""
import copy
import json
import os
import random

import pytest

import ms_apply_ref as A
import ms_pack_cases as C
import ms_pack_ref as K
import ms_ref as R

pytestmark = pytest.mark.gpu


def _unpack(ctx, jobs):
    """`jobs`: C.batch() rows.  The device's answer against the restatement's; returns it."""
    from neptune_hip.mutator_set import unpack_removal_records_batch
    got = unpack_removal_records_batch(ctx, [C.to_library(p) for _, p, _, _ in jobs])
    assert len(got) == len(jobs)
    for (name, _, status, records), (st, recs) in zip(jobs, got):
        assert st == status, (name, st, status)
        if status == 0:
            assert C.from_library(recs) == records, name
        else:
            assert recs is None, name
    return got


# ---------------------------------------------------------------- nhip_ms_unpack_batch
def test_empty_cases(ctx, golden_dir):
    assert _unpack(ctx, []) == []
    _unpack(ctx, [("no records", [], 0, [])])
    pin = json.load(open(os.path.join(golden_dir, "ms_pack_pins.json")))["regressions"]["inputs"][0]
    recs = [R.Record(R.IndexSet(int(pin["minimum"]), list(pin["distances"])), []) for _ in range(3)]
    status, out = K.try_unpack_status(recs)
    assert status == 0 and all(not r.target_chunks for r in out) and K.decode_from_vec(recs).num_leafs_aocl == 1
    _unpack(ctx, [("empty dictionary", recs, status, out), ("no records", [], 0, [])])


def test_one_tree_of_height_zero(ctx):
    recs = C.records_of(9)
    packed = K.pack(recs)
    assert [(k, len(p)) for k, p, _ in packed[0].target_chunks] == [(0, 0)]  # empty structure ...
    assert any(r.target_chunks for r in recs) and all(not p for r in recs for _, p, _ in r.target_chunks)  # ... and path
    _unpack(ctx, [("a9", packed, 0, recs)])


def test_trees_without_chunks_and_more_chunks_than_trees(ctx):
    rows = {n: (n, p, s, r) for n, p, s, r in C.batch()}
    keys = lambda n: [k for k, _, _ in rows[n][1][0].target_chunks]  # noqa: E731
    assert keys("sparse_trees") == [1, 66, 67]
    assert keys("a41").count(K.IGNORE_TREE_HEIGHT) >= 1 and keys("a200").count(K.IGNORE_TREE_HEIGHT) >= 3
    got = _unpack(ctx, [rows[n] for n in ("sparse_trees", "a41", "a200", "two_trees")])
    assert sum(len(p) for r in got[2][1] for _, p, _ in r.target_chunks) > 20  # shared ancestors rebuilt


def test_unequal_jobs_with_the_largest_and_the_smallest_chunk(ctx):
    rows = {n: (n, p, s, r) for n, p, s, r in C.batch()}
    sizes = [len(c.relative_indices) for r in rows["chunk_sizes"][3] for _, _, c in r.target_chunks]
    assert K.MAX_UNPACKED_LENGTH in sizes and 1 in sizes and 0 in sizes
    _unpack(ctx, [rows["a3"], rows["chunk_sizes"], rows["a17"], rows["a200"]])


def test_mixed_batch_equals_the_jobs_alone(ctx):
    jobs = list(C.batch())
    assert {s for _, _, s, _ in jobs} >= set(range(K.PAYLOAD_TOO_BIG, K.UNPACK_PANIC + 1)) | {0}
    together = _unpack(ctx, jobs)
    again = _unpack(ctx, jobs)  # the same context, its workspace now warm
    for k, job in enumerate(jobs):
        alone = _unpack(ctx, [job])[0]
        assert alone == together[k] == again[k], job[0]


# ---------------------------------------------------------------- nhip_ms_apply_batch_packed
def to_msa(msa):
    from neptune_hip.mutator_set import MmrAccumulator, MutatorSetAccumulator
    mmr = lambda m: MmrAccumulator(list(m.peaks), m.num_leafs)  # noqa: E731
    return MutatorSetAccumulator(mmr(msa.aocl), mmr(msa.swbf_inactive), list(msa.swbf_active))


def _flip(d, word=2):
    d = list(d)
    d[word] = (d[word] + 1) % R.P
    return tuple(d)


def _items(rng, k):
    return [(C.digest(rng), C.digest(rng), C.digest(rng)) for _ in range(k)]


def _small(n0, seed):
    rng = random.Random(seed)
    a = R.Archival()
    for k in range(n0):
        a.add(C.digest(rng), C.digest(rng), C.digest(rng))
        if k % 4 == 3:
            a.remove(a.removal_record(k - 3))
    return a


@pytest.fixture(scope="module")
def apply_jobs():
    """[(label, msa, additions, packed list, expected | None)], jobs that fail 2.a interleaved."""
    rng = random.Random(41)
    arch, recs = C.archival(200)
    msa = arch.msa()
    packed = K.pack(recs)
    jobs = [("four records, five additions", msa, _items(rng, 5), packed, None)]
    flipped = copy.deepcopy(packed)
    e = next(e for e, (_, p, _) in enumerate(flipped[0].target_chunks) if p)
    k, p, c = flipped[0].target_chunks[e]
    flipped[0].target_chunks[e] = (k, [_flip(p[0])] + list(p[1:]), c)
    jobs.append(("structure digest flipped", msa, [], flipped, None))                       # BAD_MMR_PATH
    jobs.append(("a removed item", msa, _items(rng, 1), K.pack([arch.removal_record(0)] + recs[:1]), None))
    tiny = _small(8, 508)
    jobs.append(("records of a later set", tiny.msa(), [], K.pack([arch.removal_record(199)]), None))  # OUT_OF_RANGE
    later = A.clone(arch)
    for it in _items(rng, 16):
        later.add(*it)
    i = next(i for i in range(8, 200) if any(24 <= x // R.CHUNK_SIZE < 26 for x in arch.index_set(i).to_array()))
    jobs.append(("a chunk that became inactive", later.msa(), [], K.pack([arch.removal_record(i)]), None))  # ABSENT
    jobs.append(("same record twice", msa, [], K.pack([recs[0], recs[1], recs[0]]), None))
    forged = copy.deepcopy(recs[0])
    d = forged.absolute_indices.distances
    j = next(j for j in range(1, 45) if d[j] != d[0])
    d[0], d[j] = d[j], d[0]
    jobs.append(("forged second record", msa, [], K.pack([recs[0], forged]), None))
    off = R.Msa(msa.aocl, R.Mmr(msa.swbf_inactive.peaks, msa.swbf_inactive.num_leafs + 1), msa.swbf_active)
    jobs.append(("swbf num_leafs off by one", off, _items(rng, 1), packed, None))
    for n0 in (0, 1, 8, 255, 256):
        a = _small(n0, 500 + n0)
        live = [i for i in range(n0) if n0 >= 255 and i % 4 != 0][-2:]
        jobs.append((f"{n0} + 9", a.msa(), _items(rng, 9), K.pack([a.removal_record(i) for i in live]), None))
    n0 = (1 << 40) + 5
    big = R.Msa(R.Mmr([C.digest(rng) for _ in range(3)], n0), R.Mmr([C.digest(rng)], (n0 - 1) // 8),
                sorted([5, 100, 4095, 4096] + [rng.randrange(1 << 20) for _ in range(46)]))
    jobs.append(("2^40 + 5 leaves, 9 additions", big, _items(rng, 9), [], None))
    bad = [(n, msa, _items(rng, 2), m, None) for n, (m, s) in sorted(C.mutants().items()) if s]
    out = []
    while jobs or bad:
        if jobs:
            out.append(jobs.pop(0))
        if bad:
            out.append(bad.pop(0))
    # rule 2.e: the first job again with the right and with a wrong expected accumulator
    first = out[0]
    right = A.outcome(arch, msa, first[2], recs)[3]
    wrong = copy.deepcopy(right)
    wrong.aocl = R.Mmr([_flip(wrong.aocl.peaks[0], 4)] + wrong.aocl.peaks[1:], wrong.aocl.num_leafs)
    with_expected = [first[:4] + (right,), first[:4] + (wrong,), out[1][:4] + (msa,)]
    return out, with_expected


def _run_apply(ctx, jobs):
    from neptune_hip.mutator_set import MutatorSetUpdate, apply_update_batch, apply_update_batch_packed
    expected = None if jobs[0][4] is None else [to_msa(e) for _, _, _, _, e in jobs]
    packed_jobs, plain_jobs, plain_of = [], [], []
    for label, msa, adds, packed, _ in jobs:
        commitments = [A.commitment(*it) for it in adds]
        packed_jobs.append((to_msa(msa), MutatorSetUpdate(C.to_library(packed), commitments)))
        status, recs = K.try_unpack_status(packed)
        plain_of.append((status, len(plain_jobs)))
        if status == 0:
            plain_jobs.append((to_msa(msa), MutatorSetUpdate(C.to_library(recs), commitments)))
    plain = apply_update_batch(ctx, plain_jobs, None if expected is None else
                               [e for e, (s, _) in zip(expected, plain_of) if s == 0])
    got = apply_update_batch_packed(ctx, packed_jobs, expected)
    for (label, *_), (status, k), g in zip(jobs, plain_of, got):
        if status:
            assert g == (False, status, None, None), label
        else:
            assert g == plain[k], (label, g[:3], plain[k][:3])
    return got


def test_rules_2a_to_2e_in_one_call(ctx, apply_jobs):
    jobs, _ = apply_jobs
    got = _run_apply(ctx, jobs)
    from neptune_hip import mutator_set as MS
    seen = {g[1] for g in got}
    assert seen >= {MS.OK, MS.ABSENT_CHUNK, MS.BAD_MMR_PATH, MS.ALREADY_REMOVED, MS.OUT_OF_RANGE, MS.INCONSISTENT,
                    MS.DUPLICATE_RECORD, MS.UPDATE_IMPOSSIBLE} | set(range(MS.UNPACK_PAYLOAD_TOO_BIG, MS.UNPACK_PANIC + 1))
    by = {j[0]: g for j, g in zip(jobs, got)}
    assert by["four records, five additions"][:3] == (True, MS.OK, None)
    assert by["2^40 + 5 leaves, 9 additions"][3].swbf_inactive.num_leafs == (1 << 37) + 1
    assert by["256 + 9"][0] and by["255 + 9"][0] and by["0 + 9"][3].aocl.num_leafs == 9
    assert _run_apply(ctx, jobs) == got  # twice on one context


def test_rule_2e_over_packed_lists(ctx, apply_jobs):
    from neptune_hip import mutator_set as MS
    _, jobs = apply_jobs
    got = _run_apply(ctx, jobs)
    assert [g[:2] for g in got[:2]] == [(True, MS.OK), (False, MS.UPDATE_MISMATCH)] and got[2][1] >= MS.UNPACK_PAYLOAD_TOO_BIG


def test_block_rule_wrapper(ctx, apply_jobs):
    from neptune_hip import blocks
    from neptune_hip import mutator_set as MS
    _, jobs = apply_jobs
    for (label, msa, adds, packed, expected), want in zip(jobs[:2], ((True, MS.OK), (False, MS.UPDATE_MISMATCH))):
        got = blocks.mutator_set_update_valid_packed(ctx, to_msa(msa), C.to_library(packed),
                                                     [A.commitment(*it) for it in adds], to_msa(expected))
        assert got == want, label
