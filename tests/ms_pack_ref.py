"""CPU restatement of neptune-core's packed removal records (block rule 2.a) over ms_ref's types — TEST HELPER
ONLY (not collected).

Paths relative to neptune-core/src/util_types/mutator_set/removal_record/:
  * chunk_pack / chunk_try_unpack: `Chunk::pack` / `Chunk::try_unpack`, chunk.rs:148-304: the 12-bit fields
    [len, idx...] as one big-endian bit string over u32 words, zero padded.
  * pack: `RemovalRecordList::pack`, removal_record_list.rs:646-649 = convert_from_vec (:674-696),
    from_removal_records (:118-264), compressed_chunk_dictionary (:328-368), encode_as_vec (:406-420).  Only a
    generator of test data: where the reference asserts, this asserts.
  * try_unpack: `RemovalRecordList::try_unpack`, :653-658 = decode_from_vec (:548-618) with
    observed_chunk_indices_from_index_sets (:622-642) and estimate_num_leafs_aocl (:283-316),
    validate_consistency (:453-543), convert_to_vec (:705-883).  Step by step, quirks included.

The reference's errors are `UnpackError(status)` with the NHIP_MS_* value of the variant; where it panics this
raises `ms_ref.ReferencePanics`.  twenty-first is not in the reference tree: `MerkleTree::
authentication_structure_node_indices` is taken as oracle/stark_ref.py:292-302 states it (siblings needed minus
nodes computable, descending node index), and `leaf_index_to_mt_index_and_peak_index` / `get_peak_heights` as
ms_ref.mmr_verify uses them.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Sequence, Tuple

import ms_ref as M
from ms_ref import CHUNK_SIZE, BATCH_SIZE, Chunk, IndexSet, Record, ReferencePanics

PAYLOAD_TOO_BIG, INCONSISTENT_LENGTH, NONZERO_TRAILING_PADDING, ILLEGAL_TREE_HEIGHT, DUPLICATE_TREE_HEIGHTS, \
    INDEX_TOO_BIG, INCONSISTENT_CHUNKS, STRUCTURE_COUNT, STRUCTURE_LENGTH, UNPACK_PANIC = range(10, 20)
MAX_PACKED_LENGTH, MAX_UNPACKED_LENGTH = 1536, 4095  # chunk.rs:22-23
IGNORE_TREE_HEIGHT, TREE_HEIGHT_OFFSET = (1 << 64) - 1, 64  # removal_record_list.rs:97,102
U64 = 1 << 64


class UnpackError(Exception):
    def __init__(self, status: int):
        super().__init__(status)
        self.status = status


# ---------------------------------------------------------------- Chunk::pack / try_unpack
def chunk_pack(relative_indices: Sequence[int]) -> List[int]:
    if not relative_indices:
        return []
    assert all(0 <= x < CHUNK_SIZE for x in relative_indices) and len(relative_indices) <= MAX_UNPACKED_LENGTH
    fields = [len(relative_indices)] + [int(x) for x in relative_indices]
    bits = 0
    for f in fields:
        bits = bits << 12 | f
    width = 12 * len(fields)
    bits <<= -width % 32
    words = (width + 31) // 32
    return [bits >> 32 * (words - 1 - k) & 0xFFFFFFFF for k in range(words)]


def chunk_try_unpack(words: Sequence[int]) -> List[int]:
    if not words:
        return []
    if len(words) > MAX_PACKED_LENGTH:
        raise UnpackError(PAYLOAD_TOO_BIG)
    indicated = words[0] >> 20 & 0xFFF
    if ((indicated + 1) * 12 + 31) // 32 != len(words):
        raise UnpackError(INCONSISTENT_LENGTH)
    bits = 0
    for w in words:
        bits = bits << 32 | int(w)
    total = 32 * len(words)
    fields = [bits >> (total - 12 * (k + 1)) & 0xFFF for k in range(indicated + 1)]
    tail = -((indicated + 1) * 12) % 32
    if words[-1] & ((1 << tail) - 1):
        raise UnpackError(NONZERO_TRAILING_PADDING)
    return fields[1:]


# ---------------------------------------------------------------- twenty-first's MMR shape
def peak_heights(num_leafs: int) -> List[int]:
    """get_peak_heights: tallest first."""
    return [h for h in range(63, -1, -1) if num_leafs >> h & 1]


def mt_and_peak_index(leaf_index: int, num_leafs: int) -> Tuple[int, int]:
    """leaf_index_to_mt_index_and_peak_index, for leaf_index < num_leafs."""
    h = (leaf_index ^ num_leafs).bit_length() - 1
    mask = (1 << h) - 1
    return (leaf_index & mask) + (1 << h), bin(num_leafs).count("1") - bin(num_leafs & mask).count("1") - 1


def auth_structure_node_indices(num_leafs: int, leaf_indices: Sequence[int]) -> List[int]:
    needed, computable = set(), set()
    for li in leaf_indices:
        assert li < num_leafs
        node = li + num_leafs
        while node > 1:
            computable.add(node)
            needed.add(node ^ 1)
            node >>= 1
    return sorted(needed - computable, reverse=True)


def swbfi_leaf_count(num_leafs_aocl: int) -> int:  # util_types/mutator_set.rs:74-76
    return max(num_leafs_aocl - 1, 0) // BATCH_SIZE


def estimate_num_leafs_aocl(observed_chunk_indices: Sequence[int], path_lengths: Sequence[int]) -> int:
    """:283-316.  path_lengths: tallest first."""
    s = max(observed_chunk_indices, default=0)
    if list(path_lengths) != sorted(path_lengths, reverse=True):
        raise ReferencePanics("observed authentication path lengths were not sorted")
    if any(a == b for a, b in zip(path_lengths, path_lengths[1:])):
        raise ReferencePanics("observed authentication path lengths contains duplicates")
    for h in path_lengths:
        w = 1 << h
        if not s & w:
            s = (s | w) & (U64 - 1 - (w - 1))
    if s * BATCH_SIZE + 1 >= U64:
        raise ReferencePanics("swbfi_leaf_count_estimate * BATCH_SIZE + 1 overflows u64")
    return s * BATCH_SIZE + 1


@dataclass
class RemovalRecordList:  # :31-53
    index_sets: List[IndexSet]
    authentication_structures: List[List[Tuple[int, ...]]]  # by ascending tree height
    chunks: List[List[int]]  # unpacked relative indices, by ascending chunk index
    num_leafs_aocl: int


def _inactive_chunk_indices(index_sets: Sequence[IndexSet], window_start: int) -> List[int]:
    return sorted({i // CHUNK_SIZE for s in index_sets for i in s.to_array() if i < window_start})


# ---------------------------------------------------------------- pack (test-data generator)
def from_removal_records(records: Sequence[Record], num_leafs_aocl: int) -> RemovalRecordList:
    n = swbfi_leaf_count(num_leafs_aocl)
    heights = peak_heights(n)
    leaves, chunks, sparse = set(), {}, {}

    def put(key, digest):
        assert sparse.setdefault(key, digest) == digest, "removal records disagree about a node"

    for r in records:
        for ci, path, chunk in r.target_chunks:
            rel = [int(x) for x in chunk.relative_indices]
            assert chunks.setdefault(ci, rel) == rel, "distinct chunks for the same chunk index"
            node, peak = mt_and_peak_index(ci, n)
            h = len(path)
            assert heights[peak] == h, "authentication path length disagrees with the tree heights"
            leaves.add((h, ci))
            run = M.chunk_hash(rel)
            for sib in path:
                sib = tuple(int(x) for x in sib)
                put((h, node), run)
                put((h, node ^ 1), sib)
                run = M._hp(run, sib) if node & 1 == 0 else M._hp(sib, run)
                node >>= 1
            put((h, node), run)
    structures = []
    for h in sorted(heights):
        mine = [ci & ((1 << h) - 1) for hh, ci in leaves if hh == h]
        structures.append([sparse[(h, ni)] for ni in auth_structure_node_indices(1 << h, mine)])
    return RemovalRecordList([r.absolute_indices for r in records], structures,
                             [chunks[ci] for ci in sorted(chunks)], num_leafs_aocl)


def convert_from_vec(records: Sequence[Record]) -> RemovalRecordList:
    observed = sorted({ci for r in records for ci, _, _ in r.target_chunks})
    lengths = sorted({len(p) for r in records for _, p, _ in r.target_chunks}, reverse=True)
    return from_removal_records(records, estimate_num_leafs_aocl(observed, lengths))


def encode_as_vec(rrl: RemovalRecordList) -> List[Record]:
    heights = sorted(peak_heights(swbfi_leaf_count(rrl.num_leafs_aocl)))
    assert len(heights) == len(rrl.authentication_structures)  # zip_eq
    window_start = swbfi_leaf_count(rrl.num_leafs_aocl) * CHUNK_SIZE
    assert len(_inactive_chunk_indices(rrl.index_sets, window_start)) == len(rrl.chunks)
    dictionary = []
    for k in range(max(len(heights), len(rrl.chunks))):
        packed = chunk_pack(rrl.chunks[k]) if k < len(rrl.chunks) else None
        if k >= len(heights):
            dictionary.append((IGNORE_TREE_HEIGHT, [], Chunk(packed)))
        elif packed is None:
            dictionary.append((heights[k] + TREE_HEIGHT_OFFSET, list(rrl.authentication_structures[k]), Chunk([])))
        else:
            dictionary.append((heights[k], list(rrl.authentication_structures[k]), Chunk(packed)))
    return [Record(s, dictionary if k == 0 else []) for k, s in enumerate(rrl.index_sets)]


def pack(records: Sequence[Record]) -> List[Record]:
    return encode_as_vec(convert_from_vec(records))


# ---------------------------------------------------------------- try_unpack
def observed_chunk_indices_from_index_sets(index_sets: Sequence[IndexSet], number: int) -> List[int]:
    out = []
    for s in index_sets:
        for i in s.to_array():
            if i // CHUNK_SIZE >= U64:
                raise UnpackError(INDEX_TOO_BIG)
            out.append(i // CHUNK_SIZE)
    return sorted(set(out))[:number]


def decode_from_vec(records: Sequence[Record]) -> RemovalRecordList:
    index_sets, structures, chunks, heights = [], [], [], []
    for r in records:
        index_sets.append(r.absolute_indices)
        for key, path, chunk in r.target_chunks:
            if key < TREE_HEIGHT_OFFSET:
                heights.append(key)
                structures.append([tuple(int(x) for x in d) for d in path])
                chunks.append(chunk_try_unpack(chunk.relative_indices))
            elif key < 2 * TREE_HEIGHT_OFFSET:
                heights.append(key - TREE_HEIGHT_OFFSET)
                structures.append([tuple(int(x) for x in d) for d in path])
            elif key == IGNORE_TREE_HEIGHT:
                chunks.append(chunk_try_unpack(chunk.relative_indices))
            else:
                raise UnpackError(ILLEGAL_TREE_HEIGHT)
            if len(set(heights)) != len(heights):
                raise UnpackError(DUPLICATE_TREE_HEIGHTS)
    observed = observed_chunk_indices_from_index_sets(index_sets, len(chunks))
    rrl = RemovalRecordList(index_sets, structures, chunks, estimate_num_leafs_aocl(observed, heights[::-1]))
    validate_consistency(rrl)
    return rrl


def _leaves_by_tree(observed: Sequence[int], n: int) -> Dict[int, List[int]]:
    """{tree height: Merkle leaf indices inside that tree} of the SWBF leaves `observed` (all < n)."""
    heights = peak_heights(n)
    out: Dict[int, List[int]] = {h: [] for h in heights}
    for ci in observed:
        node, peak = mt_and_peak_index(ci, n)
        out[heights[peak]].append(node ^ (1 << heights[peak]))
    return out


def validate_consistency(rrl: RemovalRecordList) -> None:
    n = swbfi_leaf_count(rrl.num_leafs_aocl)
    observed = _inactive_chunk_indices(rrl.index_sets, n * CHUNK_SIZE)
    if len(observed) != len(rrl.chunks):
        raise UnpackError(INCONSISTENT_CHUNKS)
    by_tree = _leaves_by_tree(observed, n)
    if len(rrl.authentication_structures) != len(by_tree):
        raise UnpackError(STRUCTURE_COUNT)
    expected = sorted(len(auth_structure_node_indices(1 << h, mlis)) for h, mlis in by_tree.items())
    if expected != sorted(len(s) for s in rrl.authentication_structures):
        raise UnpackError(STRUCTURE_LENGTH)


def rebuild_nodes(rrl: RemovalRecordList, leaf_hashes=None):
    """The first half of convert_to_vec (:706-822): ({(height, node index): digest}, {chunk index: chunk})."""
    n = swbfi_leaf_count(rrl.num_leafs_aocl)
    heights = peak_heights(n)
    assert len(heights) == len(rrl.authentication_structures)
    window_start = rrl.num_leafs_aocl // BATCH_SIZE * CHUNK_SIZE
    all_ci = _inactive_chunk_indices(rrl.index_sets, window_start)[:len(rrl.chunks)]
    master = dict(zip(all_ci, rrl.chunks))
    sparse = {}
    for ci, chunk in zip(all_ci, rrl.chunks):
        node, peak = mt_and_peak_index(ci, n)
        sparse[(heights[peak], node)] = M.chunk_hash(chunk)
    for h, structure in zip(sorted(heights), rrl.authentication_structures):
        mine = [node ^ (1 << h) for hh, node in sparse if hh == h]
        nodes = auth_structure_node_indices(1 << h, mine)
        if len(nodes) != len(structure):
            raise ReferencePanics("Have authentication structure of len %d but node indices of len %d"
                                  % (len(structure), len(nodes)))
        for ni, d in zip(nodes, structure):
            sparse[(h, ni)] = d
    for h in heights:
        while True:
            have = sorted(node for hh, node in sparse if hh == h)
            absent = [a >> 1 for a, b in zip(have, have[1:]) if a == b ^ 1 and a >> 1 not in have]
            if not absent:
                break
            for parent in absent:
                sparse[(h, parent)] = M._hp(sparse[(h, 2 * parent)], sparse[(h, 2 * parent + 1)])
    return sparse, master


def convert_to_vec(rrl: RemovalRecordList) -> List[Record]:
    sparse, master = rebuild_nodes(rrl)
    n = swbfi_leaf_count(rrl.num_leafs_aocl)
    heights = peak_heights(n)
    window_start = rrl.num_leafs_aocl // BATCH_SIZE * CHUNK_SIZE
    out = []
    for s in rrl.index_sets:
        target_chunks = []
        for ci in _inactive_chunk_indices([s], window_start):
            if ci not in master:
                raise ReferencePanics("master chunks dictionary should contain entries for all chunk indices")
            node, peak = mt_and_peak_index(ci, n)
            path = []
            while node != 1:
                if (heights[peak], node ^ 1) not in sparse:
                    raise ReferencePanics("node on authentication path must live in sparse mmr dictionary")
                path.append(sparse[(heights[peak], node ^ 1)])
                node >>= 1
            target_chunks.append((ci, path, Chunk(list(master[ci]))))
        out.append(Record(s, target_chunks))
    return out


def try_unpack(records: Sequence[Record]) -> List[Record]:
    return convert_to_vec(decode_from_vec(records))


def try_unpack_status(records: Sequence[Record]):
    """(status, records | None) as the library reports it: 0, the error's value, or UNPACK_PANIC."""
    try:
        return 0, try_unpack(records)
    except UnpackError as e:
        return e.status, None
    except ReferencePanics:
        return UNPACK_PANIC, None
