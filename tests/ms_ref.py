"""CPU restatement of neptune-core's mutator-set checks over the Tip5 oracle — TEST HELPER ONLY (not collected).

The checks (paths relative to neptune-core/src/util_types/):
  * mmr_verify: twenty-first `MmrMembershipProof::verify(leaf_index, leaf, peaks, num_leafs)`.  The crate
    is not in the reference tree; the restatement rests on the path shape that
    archival_mmr.rs:250-281 (`auth_path_node_indices`) fixes, which tests/test_ms_ref.py checks.
  * chunk_hash: `Tip5::hash(chunk)`, the hash_varlen of `Chunk { relative_indices: Vec<u32> }`'s
    BFieldCodec encoding [n + 1, n, idx...] (mutator_set/removal_record/chunk.rs:39-42; the layout rule is
    the one neptune-core/src/tasm/claims/new_claim.rs pins for Claim).
  * validate: `RemovalRecord::validate`, mutator_set/removal_record.rs:202-251, with
    `split_by_activity`, mutator_set/removal_record/absolute_index_set.rs:140-160.
  * can_remove: `MutatorSetAccumulator::can_remove`, mutator_set/mutator_set_accumulator.rs:187-222.
  * ms_verify: `MutatorSetAccumulator::verify`, mutator_set/mutator_set_accumulator.rs:252-339.
Where the reference would panic (`ActiveWindow::contains`, mutator_set/active_window.rs:153-159) or
truncate (`as u64`, mutator_set/shared.rs:24) these raise `ReferencePanics`.

`Archival` is a small archival mutator set: it keeps every AOCL leaf and the whole Bloom filter as
{chunk_index: sorted list}, and derives the accumulator and every membership proof from scratch
(no incremental update code): peaks from the binary decomposition of num_leafs, paths as Merkle
paths inside the leaf's subtree.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Sequence, Tuple

import coracle  # oracle/: the C restatement of Tip5 (checked against tip5_ref and the KATs)

P = (1 << 64) - (1 << 32) + 1
WINDOW_SIZE, CHUNK_SIZE, BATCH_SIZE, NUM_TRIALS = 1 << 20, 1 << 12, 1 << 3, 45  # mutator_set/shared.rs:12-15
OK, ABSENT_CHUNK, BAD_MMR_PATH, ALREADY_REMOVED, OUT_OF_RANGE, NOT_IN_AOCL = range(6)
U128_MAX = (1 << 128) - 1


class ReferencePanics(Exception):
    """The reference panics or truncates on this input."""


@dataclass
class Mmr:
    peaks: List[Tuple[int, ...]]
    num_leafs: int


@dataclass
class Msa:
    aocl: Mmr
    swbf_inactive: Mmr
    swbf_active: List[int]

    @property
    def batch_index(self) -> int:  # util_types/mutator_set.rs:74-76
        return max(self.aocl.num_leafs - 1, 0) // BATCH_SIZE


@dataclass
class Chunk:
    relative_indices: List[int]


@dataclass
class IndexSet:
    minimum: int
    distances: List[int]

    def to_array(self) -> List[int]:  # absolute_index_set.rs:125-131 (saturating)
        return [min(d + self.minimum, U128_MAX) for d in self.distances]


@dataclass
class Record:
    absolute_indices: IndexSet
    target_chunks: List[Tuple[int, List[Tuple[int, ...]], Chunk]] = field(default_factory=list)


@dataclass
class MembershipProof:
    sender_randomness: Tuple[int, ...]
    receiver_preimage: Tuple[int, ...]
    auth_path_aocl: List[Tuple[int, ...]]
    aocl_leaf_index: int
    target_chunks: List[Tuple[int, List[Tuple[int, ...]], Chunk]] = field(default_factory=list)


# Tip5 through the C oracle's permutation (tip5_ref's own backend switch is left alone: it is global)
def _hp(a, b) -> Tuple[int, ...]:
    """Tip5::hash_pair: FixedLength domain, capacity words 1."""
    return tuple(coracle.permutation_list([int(x) for x in a] + [int(x) for x in b] + [1] * 6)[:5])


def _absorb(data: Sequence[int]) -> List[int]:
    """Tip5::init() then pad_and_absorb_all: a 1, then zeros to a multiple of the rate 10."""
    data = [int(x) for x in data] + [1]
    data += [0] * (-len(data) % 10)
    state = [0] * 16
    for k in range(0, len(data), 10):
        state = coracle.permutation_list(data[k:k + 10] + state[10:])
    return state


def hash_varlen(data: Sequence[int]) -> Tuple[int, ...]:
    return tuple(_absorb(data)[:5])


def absolute_index_set(item, sender_randomness, receiver_preimage, aocl_leaf_index: int) -> Tuple[int, List[int]]:
    """AbsoluteIndexSet::compute (absolute_index_set.rs:86-113), as oracle/mast_ref.py restates it."""
    state = _absorb(list(item) + list(sender_randomness) + list(receiver_preimage) +
                    [aocl_leaf_index & 0xFFFFFFFF, aocl_leaf_index >> 32])
    rel: List[int] = []
    while len(rel) < NUM_TRIALS:
        out, state = state[:10], coracle.permutation_list(state)
        rel += [(e & 0xFFFFFFFF) % WINDOW_SIZE for e in out if e != P - 1]
    rel = rel[:NUM_TRIALS]
    return min(rel) + (aocl_leaf_index // BATCH_SIZE) * CHUNK_SIZE, [x - min(rel) for x in rel]


def mmr_verify(leaf_index: int, leaf, path, peaks, num_leafs: int) -> bool:
    if leaf_index >= num_leafs:
        return False
    h = (leaf_index ^ num_leafs).bit_length() - 1
    mt_index = (leaf_index & ((1 << h) - 1)) + (1 << h)
    peak_index = bin(num_leafs).count("1") - bin(num_leafs & ((1 << h) - 1)).count("1") - 1
    if len(path) != h or peak_index >= len(peaks):
        return False
    acc = tuple(int(x) for x in leaf)
    for sib in path:
        acc = _hp(sib, acc) if mt_index & 1 else _hp(acc, sib)
        mt_index >>= 1
    return acc == tuple(int(x) for x in peaks[peak_index])


def chunk_hash(relative_indices: Sequence[int]) -> Tuple[int, ...]:
    n = len(relative_indices)
    return hash_varlen([n + 1, n] + [int(x) for x in relative_indices])


def _split(msa: Msa, indices: IndexSet):
    """split_by_activity: ({inactive chunk index: indices}, active indices), or None for a future index."""
    arr = indices.to_array()
    if any(i >> 12 >= 1 << 64 for i in arr):
        raise ReferencePanics("(index / CHUNK_SIZE) as u64 truncates")
    lo, hi = msa.batch_index, msa.batch_index + WINDOW_SIZE // CHUNK_SIZE
    if any(i // CHUNK_SIZE > hi for i in arr):
        return None
    if any(i // CHUNK_SIZE == hi for i in arr):
        raise ReferencePanics("ActiveWindow::contains: index >= WINDOW_SIZE")
    inactive: Dict[int, List[int]] = {}
    active = []
    for i in arr:
        if i // CHUNK_SIZE < lo:
            inactive.setdefault(i // CHUNK_SIZE, []).append(i)
        else:
            active.append(i)
    return inactive, active


def _get(target_chunks, chunk_index):  # ChunkDictionary::get: the first entry with the key
    for ci, path, chunk in target_chunks:
        if ci == chunk_index:
            return path, chunk
    return None


def validate(msa: Msa, record) -> Tuple[bool, int]:
    split = _split(msa, record.absolute_indices)
    if split is None:
        return False, OUT_OF_RANGE
    if set(split[0]) != {ci for ci, _, _ in record.target_chunks}:
        return False, ABSENT_CHUNK
    for ci, path, chunk in record.target_chunks:
        if not mmr_verify(ci, chunk_hash(chunk.relative_indices), path, msa.swbf_inactive.peaks,
                          msa.swbf_inactive.num_leafs):
            return False, BAD_MMR_PATH
    return True, OK


def can_remove(msa: Msa, record) -> Tuple[bool, bool, int]:
    """(validate, can_remove, status)"""
    ok, status = validate(msa, record)
    if not ok:
        return False, False, status
    start = msa.batch_index * CHUNK_SIZE
    for index in record.absolute_indices.to_array():
        if index < start:
            _, chunk = _get(record.target_chunks, index // CHUNK_SIZE)
            if index % CHUNK_SIZE not in chunk.relative_indices:
                return True, True, OK
        elif index - start not in msa.swbf_active:
            return True, True, OK
    return True, False, ALREADY_REMOVED


def aocl_leaf(item, sender_randomness, receiver_preimage) -> Tuple[int, ...]:
    return _hp(_hp(item, sender_randomness), _hp(receiver_preimage, [0] * 5))


def ms_verify(msa: Msa, item, proof) -> Tuple[bool, int]:
    if msa.aocl.num_leafs <= proof.aocl_leaf_index:
        return False, NOT_IN_AOCL
    leaf = aocl_leaf(item, proof.sender_randomness, proof.receiver_preimage)
    if not mmr_verify(proof.aocl_leaf_index, leaf, proof.auth_path_aocl, msa.aocl.peaks, msa.aocl.num_leafs):
        return False, NOT_IN_AOCL
    mn, dist = absolute_index_set(item, proof.sender_randomness, proof.receiver_preimage, proof.aocl_leaf_index)
    split = _split(msa, IndexSet(mn, dist))
    if split is None:
        return False, OUT_OF_RANGE
    inactive, active = split
    start = msa.batch_index * CHUNK_SIZE
    has_absent, paths_ok = False, True
    for ci, indices in inactive.items():
        got = _get(proof.target_chunks, ci)
        if got is None:
            return False, ABSENT_CHUNK
        path, chunk = got
        paths_ok &= mmr_verify(ci, chunk_hash(chunk.relative_indices), path, msa.swbf_inactive.peaks,
                               msa.swbf_inactive.num_leafs)
        has_absent |= any(i % CHUNK_SIZE not in chunk.relative_indices for i in indices)
    has_absent |= any(i - start not in msa.swbf_active for i in active)
    if not paths_ok:
        return False, BAD_MMR_PATH
    return (True, OK) if has_absent else (False, ALREADY_REMOVED)


# ---------------------------------------------------------------- archival builder
class ArchivalMmr:
    """All leaves of an MMR; peaks and paths derived on demand (and cached per leaf count)."""

    def __init__(self, leaves: Sequence[Tuple[int, ...]]):
        self.leaves = [tuple(int(x) for x in d) for d in leaves]
        self.num_leafs = len(self.leaves)
        self.trees = []  # (first leaf, height, layers), tallest first
        first = 0
        for h in range(self.num_leafs.bit_length() - 1, -1, -1):
            if self.num_leafs >> h & 1:
                layers = [self.leaves[first:first + (1 << h)]]
                while len(layers[-1]) > 1:
                    prev = layers[-1]
                    layers.append([_hp(prev[2 * k], prev[2 * k + 1]) for k in range(len(prev) // 2)])
                self.trees.append((first, h, layers))
                first += 1 << h

    def accumulator(self) -> Mmr:
        return Mmr([layers[-1][0] for _, _, layers in self.trees], self.num_leafs)

    def _tree(self, leaf_index: int):
        for first, h, layers in self.trees:
            if first <= leaf_index < first + (1 << h):
                return first, h, layers
        raise IndexError(leaf_index)

    def path(self, leaf_index: int) -> List[Tuple[int, ...]]:
        first, h, layers = self._tree(leaf_index)
        local = leaf_index - first
        return [layers[k][(local >> k) ^ 1] for k in range(h)]

    def path_node_indices(self, leaf_index: int) -> List[int]:
        """MMR node indices (1-based, post-order) of the path's siblings: the subtree of height k whose
        last leaf is r closes the MMR of m = r + 1 leaves, which has 2m - popcount(m) nodes, the last
        tz(m) - k of them that subtree's ancestors."""
        first, h, _ = self._tree(leaf_index)
        local = leaf_index - first
        out = []
        for k in range(h):
            m = first + (((local >> k) ^ 1) + 1 << k)
            tz = (m & -m).bit_length() - 1
            out.append(2 * m - bin(m).count("1") - (tz - k))
        return out


class Archival:
    def __init__(self):
        self.items: List[Tuple[Tuple[int, ...], Tuple[int, ...], Tuple[int, ...]]] = []
        self.bloom: Dict[int, List[int]] = {}  # absolute chunk index -> sorted relative indices (with repeats)
        self._cache = None

    def add(self, item, sender_randomness, receiver_preimage) -> int:
        self.items.append(tuple(tuple(int(x) for x in d) for d in (item, sender_randomness, receiver_preimage)))
        self._cache = None
        return len(self.items) - 1

    def remove(self, record) -> None:
        """Sets the record's indices (remove_helper, mutator_set_accumulator.rs:124-182)."""
        for index in record.absolute_indices.to_array():
            c = self.bloom.setdefault(index // CHUNK_SIZE, [])
            c.append(index % CHUNK_SIZE)
            c.sort()
        self._cache = None

    def _derived(self):
        if self._cache is None:
            n = len(self.items)
            batch = max(n - 1, 0) // BATCH_SIZE
            aocl = ArchivalMmr([aocl_leaf(*it) for it in self.items])
            swbf = ArchivalMmr([chunk_hash(self.bloom.get(ci, [])) for ci in range(batch)])
            active = sorted((ci - batch) * CHUNK_SIZE + r for ci, rel in self.bloom.items() if ci >= batch for r in rel)
            self._cache = (aocl, swbf, Msa(aocl.accumulator(), swbf.accumulator(), active))
        return self._cache

    def msa(self) -> Msa:
        return self._derived()[2]

    def index_set(self, leaf_index: int) -> IndexSet:
        return IndexSet(*absolute_index_set(*self.items[leaf_index], leaf_index))

    def _target_chunks(self, indices: IndexSet):
        _, swbf, msa = self._derived()
        cis = sorted({i // CHUNK_SIZE for i in indices.to_array() if i // CHUNK_SIZE < msa.batch_index})
        return [(ci, swbf.path(ci), Chunk(list(self.bloom.get(ci, [])))) for ci in cis]

    def membership_proof(self, leaf_index: int) -> MembershipProof:
        aocl = self._derived()[0]
        _, sr, rp = self.items[leaf_index]
        return MembershipProof(sr, rp, aocl.path(leaf_index), leaf_index,
                               self._target_chunks(self.index_set(leaf_index)))

    def removal_record(self, leaf_index: int) -> Record:
        """`MutatorSetAccumulator::drop` (mutator_set_accumulator.rs:342-353)."""
        indices = self.index_set(leaf_index)
        return Record(indices, self._target_chunks(indices))
