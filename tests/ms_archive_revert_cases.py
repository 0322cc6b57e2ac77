"""Constructions shared by tests/test_ms_archive_revert_ref.py (no GPU) and tests/test_gpu_ms_archive_revert.py — TEST
HELPER ONLY (not collected).  Blocks as `(arch, adds, recs)`: the archival set before, the items added, the ms_ref
removal records; truth is `ms_ref.Archival` derived from scratch (`arch` before, `advance(arch, adds, recs)` after).
The sets come from tests/ms_update_cases.py, imported and left unchanged."""
import copy
import random

import ms_apply_ref as A
import ms_archive_cases as AC
import ms_ref as R


def advance(arch, adds, recs):
    """The archival set after a block; `arch` stays as it is."""
    a = A.clone(arch)
    for it in adds:
        a.add(*it)
    for r in copy.deepcopy(list(recs)):
        a.remove(r)
    return a


def one_block_group(c):
    """From the set of 600: additions alone, removals alone, both, and 300 additions (b 74 -> 112)."""
    group = [c.adds600[3], c.removals, c.both, c.born]
    assert [(len(cs.adds), len(cs.recs)) for cs in group] == [(300, 0), (0, 12), (20, 12), (300, 0)]
    return [(cs.arch, cs.adds, cs.recs) for cs in group]


def small_blocks(c):
    """One block on each small set (1, 8, 9, 255, 256 leaves): nine additions and, where an item is live, a removal."""
    out = []
    for n0, (arch, gone) in sorted(c.small_sets.items()):
        alive = [i for i in range(n0) if i not in gone]
        recs = [arch.removal_record(alive[0])] if alive else []
        out.append((arch, c.adds300[n0 % 7:n0 % 7 + 9], recs))
    return out


def long_slide(c):
    """2,100 additions on the set of 9 with one removal: chunks 1 .. 262 are created, those from c - b0 = 256 on from
    beyond the old window (empty)."""
    rng = random.Random(5)
    arch, gone = c.small_sets[9]
    adds = [tuple(tuple(rng.randrange(R.P) for _ in range(5)) for _ in range(3)) for _ in range(2100)]
    alive = [i for i in range(9) if i not in gone]
    recs = [arch.removal_record(alive[0])]
    b0, b1 = arch.msa().batch_index, AC.batch_index(9 + 2100)
    assert b1 - b0 > 256 and arch.msa().swbf_active
    return arch, adds, recs


def three_blocks(c):
    """Three consecutive blocks from the set of 600: 300 additions, six removals, 20 additions with three removals."""
    arch1 = advance(c.arch, c.adds300, [])
    recs2 = [arch1.removal_record(i) for i in c.low[:6]]
    arch2 = advance(arch1, [], recs2)
    recs3 = [arch2.removal_record(i) for i in c.low[6:9]]
    return [(c.arch, c.adds300, []), (arch1, [], recs2), (arch2, c.adds20, recs3)]


def fork_block(c):
    """A different block on the set of 600, the other fork: fewer and other additions than any of `three_blocks`, and
    records of other items."""
    adds = c.adds300[100:137]
    recs = [c.arch.removal_record(i) for i in c.low[9:12]]
    return c.arch, adds, recs


def edge_block(c):
    """One block on the set of 600 that reaches every chunk edge of a revert; each predicate is asserted here.
    Returns `(arch, adds, recs, facts)`, facts naming the chunks and words the test looks at afterwards."""
    arch, b0 = c.arch, c.msa.batch_index
    adds = c.adds20
    b1 = AC.batch_index(600 + len(adds))
    assert b1 > b0
    sets = {i: arch.index_set(i).to_array() for i in c.live}
    # (a) two records sharing an absolute index below b0: two copies leave one chunk
    owner, pair = {}, None
    for i in c.live:
        for x in sets[i]:
            if x // R.CHUNK_SIZE < b0 and x in owner and owner[x] != i:
                pair = (owner[x], i, x)
                break
            owner[x] = i
        if pair:
            break
    assert pair is not None
    # (b) a record with an index the chunk already held before the block: one copy stays
    held = next((i, x) for i in c.live for x in sets[i]
                if x // R.CHUNK_SIZE < b0 and x % R.CHUNK_SIZE in arch.bloom.get(x // R.CHUNK_SIZE, []))
    # (c) a record that hits a chunk of 0 words: the chunk is left with 0 words
    empties = {ci for ci in range(b0) if not arch.bloom.get(ci)}
    bare = next(i for i in c.live if any(x // R.CHUNK_SIZE in empties for x in sets[i]))
    # (d) a record with an index in a chunk the block itself creates: the whole chunk is dropped
    slid = next(i for i in c.live if any(b0 <= x // R.CHUNK_SIZE < b1 for x in sets[i]))
    leafs = sorted({pair[0], pair[1], held[0], bare, slid})
    recs = [arch.removal_record(i) for i in leafs]
    after = advance(arch, adds, recs)
    hit = sorted({x // R.CHUNK_SIZE for i in leafs for x in sets[i] if x // R.CHUNK_SIZE < b0})
    lengths = {len(after.bloom.get(ci, [])) % 2 for ci in hit} | {len(arch.bloom.get(ci, [])) % 2 for ci in hit}
    assert lengths == {0, 1}  # odd and even chunk lengths, before and after
    facts = dict(pair=pair[2], held=held[1], bare=next(x // R.CHUNK_SIZE for x in sets[bare] if x // R.CHUNK_SIZE in empties),
                 slid=next(x // R.CHUNK_SIZE for x in sets[slid] if b0 <= x // R.CHUNK_SIZE < b1), b0=b0, b1=b1)
    ci, rel = facts["pair"] // R.CHUNK_SIZE, facts["pair"] % R.CHUNK_SIZE
    assert after.bloom[ci].count(rel) - arch.bloom.get(ci, []).count(rel) == 2
    ci, rel = facts["held"] // R.CHUNK_SIZE, facts["held"] % R.CHUNK_SIZE
    assert arch.bloom[ci].count(rel) >= 1 and after.bloom[ci].count(rel) > arch.bloom[ci].count(rel)
    assert after.bloom[facts["bare"]] and not arch.bloom.get(facts["bare"])
    assert after.bloom.get(facts["slid"]) and facts["slid"] >= b0
    return arch, adds, recs, facts
