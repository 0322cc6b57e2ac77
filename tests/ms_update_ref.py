"""CPU restatement of bringing membership proofs and removal records across a block over
tests/ms_ref.py — TEST HELPER ONLY (not collected).

The reference updates a witness one addition record and one removal record at a time
(MsMembershipProof::batch_update_from_addition / batch_update_from_remove, ms_membership_proof.rs:76-270,417-468;
RemovalRecord::batch_update_from_addition / batch_update_from_remove, removal_record.rs:49-200).  With sorted
dictionaries the result, for valid inputs, is the witness a fresh `prove` or `drop` gives against the mutator set
after the block, and that is what this helper returns: it clones the `ms_ref.Archival` set behind the job, adds the
additions, removes the records in order, and takes `membership_proof(l)` or the dictionary of the index set from
the set after.  `Archival` derives every proof from all leaves from scratch and shares no algorithm with the kernels.

  * Wit: a witness (index set, dictionary, optional AOCL part); a removal record has leaf_index None.
  * admission: the per-witness status against the accumulator before, in the order of nhip_ms_update_batch.
  * outcome: (the job's outcome as ms_apply_ref.outcome gives it, [(status, Wit after or None)]).
  * tail_*: the same for an accumulator whose leaves cannot be materialised (a random tall peak, then real
    leaves): the AOCL above the tall peak is an MMR of its own as long as it does not grow to that height.
"""
from __future__ import annotations

import copy
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import ms_apply_ref as A
import ms_ref as R

JOB_REJECTED = 20


@dataclass
class Wit:
    absolute_indices: R.IndexSet
    target_chunks: List[Tuple[int, List[Tuple[int, ...]], R.Chunk]] = field(default_factory=list)
    aocl_leaf_index: Optional[int] = None
    aocl_leaf: Tuple[int, ...] = ()
    auth_path_aocl: List[Tuple[int, ...]] = field(default_factory=list)


def proof_witness(arch: R.Archival, leaf_index: int) -> Wit:
    """The membership proof of item `leaf_index` against `arch` as a witness."""
    mp = arch.membership_proof(leaf_index)
    return Wit(arch.index_set(leaf_index), mp.target_chunks, leaf_index, R.aocl_leaf(*arch.items[leaf_index]),
               mp.auth_path_aocl)


def record_witness(arch: R.Archival, leaf_index: int) -> Wit:
    r = arch.removal_record(leaf_index)
    return Wit(r.absolute_indices, r.target_chunks)


def as_witness(record) -> Wit:
    return Wit(record.absolute_indices, record.target_chunks)


def batch_after(msa: R.Msa, n_additions: int) -> int:
    return max(msa.aocl.num_leafs + n_additions - 1, 0) // R.BATCH_SIZE


def admission(msa: R.Msa, commitments, wit: Wit) -> int:
    """`commitments`: the block's addition records.  The first failure, or OK."""
    n0, n1 = msa.aocl.num_leafs, msa.aocl.num_leafs + len(commitments)
    b0, b1 = msa.batch_index, batch_after(msa, len(commitments))
    l = wit.aocl_leaf_index
    if l is not None:
        if l >= n1:
            return R.NOT_IN_AOCL
        if l < n0:
            if not R.mmr_verify(l, wit.aocl_leaf, wit.auth_path_aocl, msa.aocl.peaks, n0):
                return R.NOT_IN_AOCL
        elif tuple(wit.aocl_leaf) != tuple(commitments[l - n0]) or len(wit.auth_path_aocl) != 0:
            return R.NOT_IN_AOCL
    raw = [d + wit.absolute_indices.minimum for d in wit.absolute_indices.distances]
    if any(i > R.U128_MAX or i // R.CHUNK_SIZE > b1 + 255 for i in raw):
        return R.OUT_OF_RANGE
    if [ci for ci, _, _ in wit.target_chunks] != sorted({i // R.CHUNK_SIZE for i in raw if i // R.CHUNK_SIZE < b0}):
        return R.ABSENT_CHUNK
    for ci, path, chunk in wit.target_chunks:
        if not R.mmr_verify(ci, R.chunk_hash(chunk.relative_indices), path, msa.swbf_inactive.peaks,
                            msa.swbf_inactive.num_leafs):
            return R.BAD_MMR_PATH
    return R.OK


def outcome(arch: R.Archival, msa_before: R.Msa, additions, records, witnesses, expected=None):
    """`additions`: (item, sender_randomness, receiver_preimage) triples.  Leaves `arch` unchanged."""
    job = A.outcome(arch, msa_before, additions, records, expected)
    if job[1] != R.OK:
        return job, [(JOB_REJECTED, None)] * len(witnesses)
    after = A.clone(arch)
    for it in additions:
        after.add(*it)
    for rec in copy.deepcopy(list(records)):
        after.remove(rec)
    commitments = [A.commitment(*it) for it in additions]
    out = []
    for w in witnesses:
        st = admission(msa_before, commitments, w)
        if st != R.OK:
            out.append((st, None))
            continue
        chunks = after._target_chunks(w.absolute_indices)
        if w.aocl_leaf_index is None:
            out.append((st, Wit(w.absolute_indices, chunks)))
        else:
            path = after._derived()[0].path(w.aocl_leaf_index)
            out.append((st, Wit(w.absolute_indices, chunks, w.aocl_leaf_index, tuple(w.aocl_leaf), path)))
    return job, out


def shapes(results):
    """(aocl path lengths, entry counts, keys, path lengths, chunk lengths) of the witnesses after, flat, in order."""
    alen, ecnt, keys, plen, rlen = [], [], [], [], []
    for _, w in results:
        alen.append(len(w.auth_path_aocl))
        ecnt.append(len(w.target_chunks))
        for ci, path, chunk in w.target_chunks:
            keys.append(ci)
            plen.append(len(path))
            rlen.append(len(chunk.relative_indices))
    return alen, ecnt, keys, plen, rlen


# ---------------------------------------------------------------- accumulators with a tall peak nobody can open
class Tail:
    """An AOCL of `base` leaves under one random peak (base a power of two) followed by real items, with every index
    set of the real items inside the active window before and after the block: no witness has a dictionary."""

    def __init__(self, base: int, tall_peak, swbf_peak, items, window):
        assert base & (base - 1) == 0 and len(items) < base
        self.base, self.tall, self.swbf_peak, self.items, self.window = base, tuple(tall_peak), tuple(swbf_peak), list(items), sorted(window)

    def _mmr(self, items) -> R.ArchivalMmr:
        return R.ArchivalMmr([R.aocl_leaf(*it) for it in items])

    def msa(self, items=None, swbf=None, window=None) -> R.Msa:
        items = self.items if items is None else items
        n = self.base + len(items)
        small = self._mmr(items).accumulator()
        swbf = swbf if swbf is not None else R.Mmr([self.swbf_peak], (n - 1) // R.BATCH_SIZE)
        return R.Msa(R.Mmr([self.tall] + list(small.peaks), n), swbf, self.window if window is None else window)

    def index_set(self, items, local: int) -> R.IndexSet:
        return R.IndexSet(*R.absolute_index_set(*items[local], self.base + local))

    def witness(self, items, local: int) -> Wit:
        return Wit(self.index_set(items, local), [], self.base + local, R.aocl_leaf(*items[local]), self._mmr(items).path(local))

    def outcome(self, additions, locals_):
        """The job (no removal records) and the witnesses at the given local leaf indices, before and after."""
        before = self.msa()
        after = before
        for it in additions:
            after = A.msa_add(after, A.commitment(*it))
        all_items = self.items + list(additions)
        wits = [self.witness(self.items, i) if i < len(self.items) else
                Wit(self.index_set(all_items, i), [], self.base + i, R.aocl_leaf(*all_items[i]), []) for i in locals_]
        got = [(R.OK, self.witness(all_items, i)) for i in locals_]
        return (True, R.OK, None, after), wits, got
