"""A revert job whose dictionary paths are 37 levels, for tests/test_ms_revert_ref.py (no GPU) and
tests/test_gpu_ms_revert.py — TEST HELPER ONLY (not collected).

Nobody can materialise 2^37 chunks, so the Bloom filter's MMR is a sparse tree: a handful of real chunks under one
peak of height 37, every subtree that holds none of them a fixed random digest.  Every node above a real chunk is
hashed from its children, so a path taken from the tree authenticates against its root, and the tree built twice,
with the chunk contents before and after a block, gives the witnesses on both sides of it from scratch: no update
and no revert code is involved.  The AOCL is `ms_update_ref.Tail`'s (a random tall peak of 2^40 leaves, then real
items whose index sets lie in the window).  The block has three additions (no slide: b0 = b1 = 2^37) and one
removal record with indices in two inactive chunks whose parents are siblings, one index twice."""
import functools
import random

import ms_ref as R
import ms_update_ref as U

HEIGHT = 37
B0 = 1 << HEIGHT


class SparseTree:
    def __init__(self, chunks, seed):
        self.chunks, self.seed, self.memo = {ci: sorted(rel) for ci, rel in chunks.items()}, seed, {}

    def node(self, t, q):
        if (t, q) not in self.memo:
            if not any(ci >> t == q for ci in self.chunks):
                rng = random.Random(f"{self.seed}:{t}:{q}")  # a subtree with no real chunk: the same in every tree
                d = tuple(rng.randrange(R.P) for _ in range(5))
            elif t == 0:
                d = R.chunk_hash(self.chunks[q])
            else:
                d = R._hp(self.node(t - 1, 2 * q), self.node(t - 1, 2 * q + 1))
            self.memo[(t, q)] = d
        return self.memo[(t, q)]

    def root(self):
        return self.node(HEIGHT, 0)

    def path(self, ci):
        return [self.node(t, (ci >> t) ^ 1) for t in range(HEIGHT)]

    def dictionary(self, index_set):
        keys = sorted({i // R.CHUNK_SIZE for i in index_set.to_array() if i // R.CHUNK_SIZE < B0})
        return [(ci, self.path(ci), R.Chunk(list(self.chunks[ci]))) for ci in keys]


class Deep:
    pass


def _index_set(indices):
    mn = min(indices)
    return R.IndexSet(mn, [i - mn for i in indices])


@functools.lru_cache(maxsize=1)
def deep():
    d = Deep()
    rng = random.Random(3737)
    dig = lambda: tuple(rng.randrange(R.P) for _ in range(5))  # noqa: E731
    ci, ci2 = B0 - 5, B0 - 7  # the touched chunks: ...11011 and ...11001, siblings at level 1
    sib, c10, c36 = ci ^ 1, ci ^ (1 << 10), ci ^ (1 << 36)
    before = {ci: [5, 77, 900], ci2: [], sib: [1, 2, 3], c10: [7], c36: [10, 4000], c36 ^ 1: []}
    in_window = lambda n: [B0 * R.CHUNK_SIZE + rng.randrange(1 << 20) for _ in range(n)]  # noqa: E731
    at = lambda c, rel: c * R.CHUNK_SIZE + rel  # noqa: E731
    rec_indices = [at(ci, 40), at(ci, 3000), at(ci2, 17), at(ci2, 17)] + in_window(41)
    after = dict(before)
    after[ci] = sorted(before[ci] + [40, 3000])
    after[ci2] = [17, 17]
    t0, t1 = SparseTree(before, 37), SparseTree(after, 37)
    rec_set = _index_set(rec_indices)
    d.rec = R.Record(rec_set, t0.dictionary(rec_set))
    window0 = sorted(rng.randrange(1 << 20) for _ in range(50))
    window1 = sorted(window0 + [i - B0 * R.CHUNK_SIZE for i in rec_indices[4:]])
    items = [(dig(), dig(), dig()) for _ in range(8)]
    d.adds = items[5:]
    tail = U.Tail(1 << 40, dig(), t0.root(), items[:5], window0)
    d.msa = tail.msa(swbf=R.Mmr([t0.root()], B0), window=window0)
    d.msa_after = tail.msa(items=items, swbf=R.Mmr([t1.root()], B0), window=window1)
    d.job = (True, R.OK, None, d.msa_after)
    sets = [rec_set,                                                           # the record's own
            _index_set([at(sib, 9), at(ci, 5)] + in_window(43)),               # its sibling at level 0, and the chunk itself
            _index_set([at(c36, 10 + k) for k in range(20)] + [at(c36 ^ 1, k) for k in range(25)]),  # the peak's other half: digest 36
            _index_set([at(c10, 7), at(ci2, 2000)] + in_window(43))]           # digest 10, and a chunk left with 0 words
    d.before = [U.Wit(s, t0.dictionary(s)) for s in sets] + [tail.witness(items[:5], i) for i in (0, 3)]
    d.after = [U.Wit(s, t1.dictionary(s)) for s in sets] + [tail.witness(items, i) for i in (0, 3, 6)]
    d.ci, d.ci2, d.sib, d.c10, d.c36 = ci, ci2, sib, c10, c36
    d.trees = (t0, t1)
    return d
