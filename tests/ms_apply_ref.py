"""CPU restatement of a block's mutator-set update over tests/ms_ref.py — TEST HELPER ONLY (not collected).

Block::validate rules 2.b-2.e (neptune-core/src/protocol/consensus/block/mod.rs:816-849) and
MutatorSetUpdate::apply_to_accumulator (block/mutator_set_update.rs:107-153):
  * apply: the reference's loop on `ms_ref.Archival`, which derives every accumulator from all leaves
    from scratch and so shares no algorithm with the kernels: add the items, then for each record in
    order rebuild its chunks from the current archival state, evaluate `ms_ref.can_remove` (the 2.d
    flag) and `Archival.remove` it.
  * distinct: rule 2.c, `AbsoluteIndexSet::to_vec()` arrays compared element by element.
  * mmr_append / msa_add: the sequential accumulator-only form (add_helper,
    util_types/mutator_set/mutator_set_accumulator.rs:67-97; window_slides, :494-496), for accumulators
    whose leaves cannot be materialised.  The MMR append (peaks tallest first, equal heights merge)
    rests on util_types/archival_mmr.rs.
  * outcome: the job semantics of nhip_ms_apply_batch in its order of steps, built from the above.
"""
from __future__ import annotations

import copy
from typing import List, Optional, Sequence, Tuple

import ms_ref as R

INCONSISTENT, DUPLICATE_RECORD, UPDATE_IMPOSSIBLE, UPDATE_MISMATCH = range(6, 10)


def clone(arch: R.Archival) -> R.Archival:
    out = R.Archival()
    out.items = list(arch.items)
    out.bloom = {ci: list(rel) for ci, rel in arch.bloom.items()}
    return out


def commitment(item, sender_randomness, receiver_preimage) -> Tuple[int, ...]:
    """AdditionRecord::canonical_commitment: the AOCL leaf."""
    return R.aocl_leaf(item, sender_randomness, receiver_preimage)


def apply(archival: R.Archival, additions, records) -> Tuple[Optional[int], R.Msa]:
    """`additions`: (item, sender_randomness, receiver_preimage) triples.  Changes `archival`.  Returns the
    first record whose can_remove fails inside the loop (None: every one passes) and the accumulator after."""
    for it in additions:
        archival.add(*it)
    flag = None
    for j, rec in enumerate(records):
        current = R.Record(rec.absolute_indices, archival._target_chunks(rec.absolute_indices))
        if flag is None and not R.can_remove(archival.msa(), current)[1]:
            flag = j
        archival.remove(rec)
    return flag, archival.msa()


def distinct(records) -> Optional[int]:
    """The first record whose index array equals an earlier record's, or None."""
    seen = set()
    for j, rec in enumerate(records):
        key = tuple(rec.absolute_indices.to_array())
        if key in seen:
            return j
        seen.add(key)
    return None


def mmr_append(peaks: Sequence[Tuple[int, ...]], num_leafs: int, leaf) -> Tuple[List[Tuple[int, ...]], int]:
    peaks = [tuple(int(x) for x in d) for d in peaks] + [tuple(int(x) for x in leaf)]
    t = num_leafs
    while t & 1:
        right = peaks.pop()
        left = peaks.pop()
        peaks.append(R._hp(left, right))
        t >>= 1
    return peaks, num_leafs + 1


def msa_add(msa: R.Msa, canonical_commitment) -> R.Msa:
    """add_helper on the accumulator alone."""
    item_index = msa.aocl.num_leafs
    aocl = R.Mmr(*mmr_append(msa.aocl.peaks, msa.aocl.num_leafs, canonical_commitment))
    swbf, active = msa.swbf_inactive, sorted(msa.swbf_active)
    if item_index != 0 and item_index % R.BATCH_SIZE == 0:  # window_slides
        slid = [i for i in active if i < R.CHUNK_SIZE]
        swbf = R.Mmr(*mmr_append(swbf.peaks, swbf.num_leafs, R.chunk_hash(slid)))
        active = [i - R.CHUNK_SIZE for i in active if i >= R.CHUNK_SIZE]
    return R.Msa(aocl, swbf, active)


def consistent(msa: R.Msa, n_additions: int) -> bool:
    n0 = msa.aocl.num_leafs
    return (bin(n0).count("1") == len(msa.aocl.peaks)
            and bin(msa.swbf_inactive.num_leafs).count("1") == len(msa.swbf_inactive.peaks)
            and msa.swbf_inactive.num_leafs == max(n0 - 1, 0) // R.BATCH_SIZE and n0 + n_additions < 1 << 64)


def same(a: R.Msa, b: R.Msa) -> bool:
    """Field by field; the windows in their given order."""
    def mmr(m):
        return m.num_leafs, [tuple(int(x) for x in d) for d in m.peaks]
    return (mmr(a.aocl) == mmr(b.aocl) and mmr(a.swbf_inactive) == mmr(b.swbf_inactive)
            and [int(x) for x in a.swbf_active] == [int(x) for x in b.swbf_active])


def outcome(arch: R.Archival, msa_before: R.Msa, additions, records, expected: Optional[R.Msa] = None):
    """(verdict, status, bad record, accumulator after or None) of one job.  `arch`: the archival set behind
    `msa_before` (left unchanged); `msa_before` may differ from `arch.msa()` in the consistency cases only."""
    if not consistent(msa_before, len(additions)):
        return False, INCONSISTENT, None, None
    for j, rec in enumerate(records):
        _, can, status = R.can_remove(msa_before, rec)
        if not can:
            return False, status, j, None
    dup = distinct(records)
    if dup is not None:
        return False, DUPLICATE_RECORD, dup, None
    flag, after = apply(clone(arch), additions, copy.deepcopy(list(records)))
    if flag is not None:
        return False, UPDATE_IMPOSSIBLE, flag, None
    if expected is not None and not same(after, expected):
        return False, UPDATE_MISMATCH, None, after
    return True, R.OK, None, after
