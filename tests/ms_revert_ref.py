"""CPU restatement of taking membership proofs and removal records back across a block over
tests/ms_ref.py — TEST HELPER ONLY (not collected).

The reference walks an abandoned block backwards record by record (MsMembershipProof::revert_update_from_remove and
revert_update_from_batch_addition, ms_membership_proof.rs:380-413,517-557; state/mod.rs:1392-1497).  This helper
states the end state in Python integers: a job is a job of nhip_ms_apply_batch (msa_before, addition records,
removal records valid against msa_before), the witnesses stand at the accumulator after it and are taken to
msa_before.  With n0 / n1 the AOCL leaf counts and b0 / b1 the batch indices before / after:

  * the AOCL path keeps its first ilog2(l ^ n0) digests;
  * the dictionary keeps the entries with key < b0, in order;
  * a kept chunk loses one copy of every index the block's records put into that chunk (`Chunk::remove_once`);
  * a kept path keeps its first ilog2(key ^ b0) digests, and digest t becomes the *old* value of node
    (t, (key >> t) ^ 1) where that node is a chunk a block record touches or an ancestor of one.  The old values
    come from the block's records alone: a record's entry holds the chunk and its path before the block.

tests/test_ms_revert_ref.py holds this against witnesses derived from scratch (`ms_ref.Archival`) before the block.

  * revert_witness: the end state of one witness, or None when a chunk lacks a copy the block inserted.
  * admission:      the per-witness status on the witness as it stands after the block (integers only).
  * outcome:        (the job's outcome as ms_apply_ref.outcome gives it, [(status, Wit before or None)]): admission,
                    the end state, then the verification of every reverted witness against msa_before.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import ms_apply_ref as A
import ms_ref as R
import ms_update_ref as U

JOB_REJECTED = U.JOB_REJECTED
Wit = U.Wit


def ilog2(x: int) -> int:
    return x.bit_length() - 1


class Block:
    """What the revert reads of a block: its indices by touched chunk and the old value of every node above one."""

    def __init__(self, msa_before: R.Msa, n_additions: int, records):
        self.n0 = msa_before.aocl.num_leafs
        self.n1 = self.n0 + n_additions
        self.b0 = msa_before.batch_index
        self.b1 = U.batch_after(msa_before, n_additions)
        self.by_chunk: Dict[int, List[int]] = {}
        self.old: Dict[Tuple[int, int], Tuple[int, ...]] = {}
        for rec in records:
            for i in rec.absolute_indices.to_array():
                if i // R.CHUNK_SIZE < self.b0:
                    self.by_chunk.setdefault(i // R.CHUNK_SIZE, []).append(i % R.CHUNK_SIZE)
            for ci, path, chunk in rec.target_chunks:
                node, q = R.chunk_hash(chunk.relative_indices), ci
                self.old[(0, q)] = node
                for t, sib in enumerate(path):
                    node = R._hp(sib, node) if q & 1 else R._hp(node, sib)
                    q >>= 1
                    self.old[(t + 1, q)] = node

    def replaced(self, key: int) -> List[int]:
        """The heights of `key`'s path before the block whose digest the block changed."""
        return [t for t in range(ilog2(key ^ self.b0)) if (t, (key >> t) ^ 1) in self.old]


def revert_witness(blk: Block, w: Wit) -> Optional[Wit]:
    """`w` after the block -> before it, by shape; None when a kept chunk lacks a copy of a block index."""
    l = w.aocl_leaf_index
    aocl = list(w.auth_path_aocl[:ilog2(l ^ blk.n0)]) if l is not None else []
    entries = []
    for key, path, chunk in w.target_chunks:
        if key >= blk.b0:
            continue
        rel = list(chunk.relative_indices)
        for v in blk.by_chunk.get(key, []):
            if v not in rel:
                return None
            rel.remove(v)
        new_path = [blk.old.get((t, (key >> t) ^ 1), tuple(path[t])) for t in range(ilog2(key ^ blk.b0))]
        entries.append((key, new_path, R.Chunk(rel)))
    return Wit(w.absolute_indices, entries, l, tuple(w.aocl_leaf), aocl)


def admission(blk: Block, w: Wit) -> int:
    """Integer and word comparisons on the witness after the block; the first failure, or OK."""
    l = w.aocl_leaf_index
    if l is not None and (l >= blk.n0 or len(w.auth_path_aocl) != ilog2(l ^ blk.n1)):
        return R.NOT_IN_AOCL
    raw = [d + w.absolute_indices.minimum for d in w.absolute_indices.distances]
    if any(i > R.U128_MAX or i // R.CHUNK_SIZE > blk.b1 + 255 for i in raw):
        return R.OUT_OF_RANGE
    if [ci for ci, _, _ in w.target_chunks] != sorted({i // R.CHUNK_SIZE for i in raw if i // R.CHUNK_SIZE < blk.b1}):
        return R.ABSENT_CHUNK
    if any(len(path) != ilog2(ci ^ blk.b1) for ci, path, _ in w.target_chunks):
        return R.BAD_MMR_PATH
    return R.OK


def verification(msa_before: R.Msa, w: Wit) -> int:
    """The reference's assert after each reverted block: the witness authenticates against the accumulator before."""
    if w.aocl_leaf_index is not None and not R.mmr_verify(w.aocl_leaf_index, w.aocl_leaf, w.auth_path_aocl,
                                                          msa_before.aocl.peaks, msa_before.aocl.num_leafs):
        return R.NOT_IN_AOCL
    for ci, path, chunk in w.target_chunks:
        if not R.mmr_verify(ci, R.chunk_hash(chunk.relative_indices), path, msa_before.swbf_inactive.peaks,
                            msa_before.swbf_inactive.num_leafs):
            return R.BAD_MMR_PATH
    return R.OK


def outcome(arch_before, msa_before: R.Msa, additions, records, witnesses_after, expected=None, job=None):
    """`additions`: (item, sender_randomness, receiver_preimage) triples; `witnesses_after`: as they stand after the
    block.  `job`: the job's outcome where no archival set can be built behind `msa_before`.  Leaves everything
    unchanged."""
    if job is None:
        job = A.outcome(arch_before, msa_before, additions, records, expected)
    if job[1] != R.OK:
        return job, [(JOB_REJECTED, None)] * len(witnesses_after)
    blk = Block(msa_before, len(additions), records)
    out = []
    for w in witnesses_after:
        st = admission(blk, w)
        back = revert_witness(blk, w) if st == R.OK else None
        if st == R.OK and back is None:
            st = R.BAD_MMR_PATH
        if st == R.OK:
            st = verification(msa_before, back)
        out.append((st, back if st == R.OK else None))
    return job, out


def shapes(blk: Block, witnesses_after):
    """(aocl path lengths, entry counts, keys, path lengths, chunk lengths) of the end state laid out by shape alone,
    flat, in order: what nhip_ms_revert_plan writes for witnesses that pass admission."""
    alen, ecnt, keys, plen, rlen = [], [], [], [], []
    for w in witnesses_after:
        l = w.aocl_leaf_index
        alen.append(ilog2(l ^ blk.n0) if l is not None and l < blk.n0 else 0)
        kept = [(ci, ch) for ci, _, ch in w.target_chunks if ci < blk.b0]
        ecnt.append(len(kept))
        for ci, ch in kept:
            keys.append(ci)
            plen.append(ilog2(ci ^ blk.b0))
            rlen.append(max(len(ch.relative_indices) - len(blk.by_chunk.get(ci, [])), 0))
    return alen, ecnt, keys, plen, rlen
