"""Packed removal-record lists for the rule 2.a tests — TEST HELPER ONLY (not collected): small archival mutator
sets (ms_ref.Archival) with the removal sets of DESIGN.md §6f, hand-built lists for the shapes an archival set
of this size does not reach, and mutants of a good packed list with one change each, at least one per status."""
from __future__ import annotations

import copy
import functools
import random

import ms_pack_ref as K
import ms_ref as R

P = R.P
# additions -> (records already removed, records in the list)
SETS = {3: (0, 2), 9: (1, 2), 17: (2, 3), 41: (4, 3), 200: (7, 4), 600: (11, 6)}


def digest(rng):
    return tuple(rng.randrange(P) for _ in range(5))


@functools.lru_cache(maxsize=None)
def archival(additions: int):
    """(Archival, records): `SETS[additions]` records of the items after those already removed."""
    # the seeds of the two smallest sets were searched for records that touch an inactive chunk (a 1/256 chance
    # per index at these sizes); tests/test_ms_pack_ref.py asserts that they do
    rng = random.Random(2800 + additions + 1000 * {9: 62, 17: 4}.get(additions, 0))
    a = R.Archival()
    for _ in range(additions):
        a.add(digest(rng), digest(rng), digest(rng))
    removed, m = SETS[additions]
    for i in range(removed):
        a.remove(a.removal_record(i))
    return a, [a.removal_record(removed + i) for i in range(m)]


def records_of(additions: int):
    return copy.deepcopy(archival(additions)[1])


def index_set(chunk_indices, active_chunk=None):
    """An index set whose 45 indices fall into `chunk_indices` (all used), the rest into the first."""
    cis = list(chunk_indices)
    mn = min(cis) * R.CHUNK_SIZE
    dist = [(ci - min(cis)) * R.CHUNK_SIZE + 7 * k for k, ci in enumerate(cis)]
    dist += [3] * (R.NUM_TRIALS - len(dist))
    if active_chunk is not None:
        dist[-1] = (active_chunk - min(cis)) * R.CHUNK_SIZE
    return R.IndexSet(mn, dist)


def sparse_trees(seed=1):
    """One record with the single inactive chunk 13 in a tree of height 1: the estimate is 14 SWBF leaves, so the
    trees of heights 2 and 3 have no chunk and are `key + 64` entries."""
    rng = random.Random(seed)
    rec = R.Record(index_set([13]), [(13, [digest(rng)], R.Chunk([5, 9, 9, 4000]))])
    return [rec]


def chunk_sizes(seed=2):
    """Chunks of 4,095 indices and of 1 index (and an empty one) in one tree of height 2."""
    rng = random.Random(seed)
    big = sorted(rng.randrange(R.CHUNK_SIZE) for _ in range(K.MAX_UNPACKED_LENGTH))
    leaves = [R.chunk_hash(c) for c in (big, [77], [], [1, 2, 3])]
    mmr = R.ArchivalMmr(leaves)
    chunks = [big, [77], [], [1, 2, 3]]
    recs = [R.Record(index_set([0, 1], active_chunk=9), [(ci, mmr.path(ci), R.Chunk(list(chunks[ci]))) for ci in (0, 1)]),
            R.Record(index_set([1, 2]), [(ci, mmr.path(ci), R.Chunk(list(chunks[ci]))) for ci in (1, 2)])]
    return recs


def two_trees():
    """Five SWBF leaves (trees of heights 2 and 0), three records over the chunks 0, 1 and 4: one chunk more than
    trees, a structure of one digest for the tall tree, an active index in chunk 9."""
    chunks = [[392, 1192, 2453, 527, 2430, 2423, 257, 290, 2807, 122], [77], [5], [6], [0] * 6]
    mmr = R.ArchivalMmr([R.chunk_hash(c) for c in chunks])
    entry = lambda ci: (ci, mmr.path(ci), R.Chunk(list(chunks[ci])))  # noqa: E731
    return [R.Record(index_set([0, 4], active_chunk=9), [entry(0), entry(4)]),
            R.Record(index_set([1, 4]), [entry(1), entry(4)]),
            R.Record(index_set([0]), [entry(0)])]


def good_lists():
    """name -> unpacked records whose pack / try_unpack round trip is the identity."""
    out = {"a%d" % n: records_of(n) for n in (3, 9, 17, 41, 200)}
    out["sparse_trees"] = sparse_trees()
    out["chunk_sizes"] = chunk_sizes()
    out["two_trees"] = two_trees()
    out["no_records"] = []
    return out


def mutants():
    """name -> (packed list, status): each one change of pack(two_trees()) or of pack(sparse_trees())."""
    base = K.pack(two_trees())
    d0 = base[0].target_chunks
    assert [k for k, _, _ in d0] == [0, 2, K.IGNORE_TREE_HEIGHT] and [len(p) for _, p, _ in d0] == [0, 1, 0]
    sp = K.pack(sparse_trees())
    assert [k for k, _, _ in sp[0].target_chunks] == [1, 2 + 64, 3 + 64]
    out = {}

    def mutant(name, status, edit, src=base):
        m = copy.deepcopy(src)
        edit(m)
        out[name] = (m, status)

    def entry(m, e, key=None, path=None, rel=None):
        k, p, c = m[0].target_chunks[e]
        m[0].target_chunks[e] = (k if key is None else key, p if path is None else path,
                                 c if rel is None else R.Chunk(rel))

    words = lambda m, e: list(m[0].target_chunks[e][2].relative_indices)  # noqa: E731
    mutant("payload_too_big", K.PAYLOAD_TOO_BIG, lambda m: entry(m, 1, rel=[1] * (K.MAX_PACKED_LENGTH + 1)))
    mutant("inconsistent_length", K.INCONSISTENT_LENGTH, lambda m: entry(m, 1, rel=words(m, 1) + [0]))
    mutant("nonzero_trailing_padding", K.NONZERO_TRAILING_PADDING,
           lambda m: entry(m, 1, rel=words(m, 1)[:-1] + [words(m, 1)[-1] | 1]))
    mutant("illegal_tree_height", K.ILLEGAL_TREE_HEIGHT, lambda m: entry(m, 2, key=128))
    mutant("duplicate_tree_heights", K.DUPLICATE_TREE_HEIGHTS, lambda m: entry(m, 1, key=0))
    # the chunk error of an entry comes before that entry's duplicate check
    mutant("chunk_error_before_duplicate", K.INCONSISTENT_LENGTH,
           lambda m: entry(m, 1, key=0, rel=words(m, 1) + [0]))
    mutant("index_too_big", K.INDEX_TOO_BIG, lambda m: setattr(m[1].absolute_indices, "minimum", 1 << 76))
    mutant("inconsistent_chunks", K.INCONSISTENT_CHUNKS, lambda m: m[0].target_chunks.pop())
    mutant("structure_count", K.STRUCTURE_COUNT, lambda m: m[0].target_chunks.pop(), src=sp)
    mutant("structure_length", K.STRUCTURE_LENGTH, lambda m: entry(m, 1, path=d0[1][1] * 2))
    mutant("heights_not_ascending", K.UNPACK_PANIC, lambda m: entry(m, 0, key=3))
    # sorted lengths agree, the lengths per tree do not: the tall tree's structure given to the tree of height 0
    mutant("structure_on_wrong_tree", K.UNPACK_PANIC,
           lambda m: (entry(m, 0, path=d0[1][1]), entry(m, 1, path=[])))
    mutant("estimate_overflows", K.UNPACK_PANIC, lambda m: entry(m, 2, key=61 + 64), src=sp)
    # a key + 64 entry's chunk is neither unpacked nor checked; a dictionary on a later record is scanned too
    mutant("ignored_chunk_unchecked", 0, lambda m: entry(m, 1, rel=[1] * (K.MAX_PACKED_LENGTH + 1)), src=sp)
    mutant("dictionary_on_second_record", 0, lambda m: m[1].target_chunks.append(m[0].target_chunks.pop()))
    return out


def to_library(records):
    """ms_ref.Record -> neptune_hip.mutator_set.RemovalRecord."""
    import neptune_hip.mutator_set as MS
    from neptune_hip.mast import AbsoluteIndexSet
    return [MS.RemovalRecord(AbsoluteIndexSet(int(r.absolute_indices.minimum), list(r.absolute_indices.distances)),
                             [(int(k), [tuple(d) for d in p], MS.Chunk(list(c.relative_indices)))
                              for k, p, c in r.target_chunks]) for r in records]


def from_library(records):
    return [R.Record(R.IndexSet(int(r.absolute_indices.minimum), [int(d) for d in r.absolute_indices.distances]),
                     [(int(k), [tuple(int(x) for x in d) for d in p], R.Chunk([int(x) for x in c.relative_indices]))
                      for k, p, c in r.target_chunks]) for r in records]


@functools.lru_cache(maxsize=None)
def batch():
    """[(name, packed list, status, unpacked records | None)]: every good list packed, and every mutant, the good
    ones interleaved with the failing ones; the restatement's answer beside each."""
    good = [(n, K.pack(recs)) for n, recs in sorted(good_lists().items())]
    bad = [(n, m) for n, (m, _) in sorted(mutants().items())]
    jobs = []
    while good or bad:
        if bad:
            jobs.append(bad.pop(0))
        if good:
            jobs.append(good.pop(0))
    return [(n, p) + K.try_unpack_status(p) for n, p in jobs]
