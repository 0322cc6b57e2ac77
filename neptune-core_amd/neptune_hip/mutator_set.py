"""Host mirror of neptune-core's mutator-set checks (util_types/mutator_set/) over the C ABI: the
consensus step after "the proof verifies", batched.

* `mmr_verify_batch(ctx, mmr, items)` — twenty-first `MmrMembershipProof::verify`, as called bare in
  application/loops/peer_loop.rs:1235 and protocol/peer.rs:824.
* `can_remove_batch(ctx, msa, records)` — `RemovalRecord::validate` (removal_record.rs:202-251) and
  `MutatorSetAccumulator::can_remove` (mutator_set_accumulator.rs:187-222) for many records:
  protocol/consensus/block/mod.rs:816-822, transaction_kernel.rs:129,145.
* `verify_batch(ctx, msa, items, proofs)` — `MutatorSetAccumulator::verify`
  (mutator_set_accumulator.rs:252-339): state/wallet/wallet_state.rs:1796,1958.

* `apply_update_batch(ctx, jobs, expected=None)` — `Block::validate` rules 2.b-2.e
  (protocol/consensus/block/mod.rs:816-849) and `Block::mutator_set_accumulator_after`
  (mod.rs:369-378) for many independent `(msa_before, MutatorSetUpdate)` jobs: the accumulator after
  each update, computed on the device.

* `unpack_removal_records_batch(ctx, jobs)` — `RemovalRecordList::try_unpack`
  (removal_record/removal_record_list.rs:653-658), block rule 2.a, for many packed lists; `unpack_plan_batch(jobs)`
  is its host half (statuses and shapes, no GPU), and `apply_update_batch_packed(ctx, jobs, expected=None)` is
  rules 2.a-2.e in one call over packed lists.

* `update_witnesses_batch(ctx, jobs)` — `MsMembershipProof::batch_update_from_addition` / `batch_update_from_remove`
  (ms_membership_proof.rs:76-270,417-468) and `RemovalRecord::batch_update_from_addition` / `batch_update_from_remove`
  (removal_record.rs:49-200) over whole blocks, as the end state; `update_plan_batch(jobs)` is its
  host half (the shapes, no GPU), `update_membership_proofs` and `update_removal_records` are the wallet's and the
  mempool's calls (state/wallet/wallet_state.rs:1375,1481; state/mod.rs:1537,1557,2507,2522).

* `revert_witnesses_batch(ctx, jobs)` — `MsMembershipProof::revert_update_from_remove` /
  `revert_update_from_batch_addition` (ms_membership_proof.rs:380-413,517-557) over whole blocks, as the end state
  (DESIGN.md §6j): witnesses standing after a block taken back to the accumulator before it, each verified there;
  `revert_plan_batch(jobs)` is its host half, `revert_membership_proofs` the wallet's call during a reorganisation
  (state/mod.rs:1392-1497), and `WitnessStore.revert` the same for witnesses resident on the device.

The types mirror the reference's over numpy; every verdict is the device's.  Where the reference
would panic or truncate (an index past the active window, or >= 2^76) the record is rejected with
`OUT_OF_RANGE`.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import check
from .mast import NUM_TRIALS, AbsoluteIndexSet

CHUNK_SIZE = 1 << 12
BATCH_SIZE = 1 << 3
OK, ABSENT_CHUNK, BAD_MMR_PATH, ALREADY_REMOVED, OUT_OF_RANGE, NOT_IN_AOCL = range(6)
INCONSISTENT, DUPLICATE_RECORD, UPDATE_IMPOSSIBLE, UPDATE_MISMATCH = range(6, 10)  # apply_update_batch only
# rule 2.a (unpack_removal_records_batch, apply_update_batch_packed): try_unpack's errors, then "the reference panics"
UNPACK_PAYLOAD_TOO_BIG, UNPACK_INCONSISTENT_LENGTH, UNPACK_NONZERO_TRAILING_PADDING, UNPACK_ILLEGAL_TREE_HEIGHT, \
    UNPACK_DUPLICATE_TREE_HEIGHTS, UNPACK_INDEX_TOO_BIG, UNPACK_INCONSISTENT_CHUNKS, UNPACK_STRUCTURE_COUNT, \
    UNPACK_STRUCTURE_LENGTH, UNPACK_PANIC = range(10, 20)
STATUS_NAMES = ("OK", "ABSENT_CHUNK", "BAD_MMR_PATH", "ALREADY_REMOVED", "OUT_OF_RANGE", "NOT_IN_AOCL",
                "INCONSISTENT", "DUPLICATE_RECORD", "UPDATE_IMPOSSIBLE", "UPDATE_MISMATCH")
UNPACK_STATUS_NAMES = ("UNPACK_PAYLOAD_TOO_BIG", "UNPACK_INCONSISTENT_LENGTH", "UNPACK_NONZERO_TRAILING_PADDING",
                       "UNPACK_ILLEGAL_TREE_HEIGHT", "UNPACK_DUPLICATE_TREE_HEIGHTS", "UNPACK_INDEX_TOO_BIG",
                       "UNPACK_INCONSISTENT_CHUNKS", "UNPACK_STRUCTURE_COUNT", "UNPACK_STRUCTURE_LENGTH", "UNPACK_PANIC")


JOB_REJECTED, UPDATE_INTERNAL = 20, 21  # update_witnesses_batch only (a witness's status)
UPDATE_STATUS_NAMES = ("JOB_REJECTED", "UPDATE_INTERNAL")


def status_name(status: int) -> str:
    """The name of any NHIP_MS_* status, the rule 2.a and the witness ones included."""
    return (STATUS_NAMES + UNPACK_STATUS_NAMES + UPDATE_STATUS_NAMES)[status]


def _digests(x, n=None) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(x, dtype=np.uint64)).reshape(-1, 5)
    if n is not None and a.shape[0] != n:
        raise ValueError("digest count")
    return a


@dataclass
class MmrAccumulator:
    """twenty-first `MmrAccumulator`: the peaks (tallest first) and the leaf count."""
    peaks: Sequence[Sequence[int]]
    num_leafs: int

    def _c(self):
        p = _digests(self.peaks) if len(self.peaks) else np.zeros((0, 5), dtype=np.uint64)
        return _lib.Mmr(p.ctypes.data if p.size else None, p.shape[0], int(self.num_leafs)), p


@dataclass
class MutatorSetAccumulator:
    """mutator_set_accumulator.rs:32-36; `swbf_active` is `ActiveWindow::sbf`."""
    aocl: MmrAccumulator
    swbf_inactive: MmrAccumulator
    swbf_active: Sequence[int] = ()

    @property
    def batch_index(self) -> int:
        """`get_batch_index` (util_types/mutator_set.rs:74-76)."""
        return max(int(self.aocl.num_leafs) - 1, 0) // BATCH_SIZE

    def _c(self):
        a, ka = self.aocl._c()
        s, ks = self.swbf_inactive._c()
        act = np.ascontiguousarray(np.asarray(self.swbf_active, dtype=np.uint32)).reshape(-1)
        return _lib.Msa(a, s, act.ctypes.data if act.size else None, act.size), (ka, ks, act)


@dataclass
class Chunk:
    relative_indices: Sequence[int] = ()


@dataclass
class RemovalRecord:
    """removal_record.rs:40-43.  `target_chunks`: the chunk dictionary in its order, entries
    `(chunk_index, mmr_path, Chunk)` with `mmr_path` a list of digests (leaf sibling first)."""
    absolute_indices: AbsoluteIndexSet
    target_chunks: List[Tuple[int, Sequence[Sequence[int]], Chunk]] = field(default_factory=list)


@dataclass
class MsMembershipProof:
    """ms_membership_proof.rs:51-57: randomness, the AOCL authentication path and the chunk dictionary."""
    sender_randomness: Sequence[int]
    receiver_preimage: Sequence[int]
    auth_path_aocl: Sequence[Sequence[int]]
    aocl_leaf_index: int
    target_chunks: List[Tuple[int, Sequence[Sequence[int]], Chunk]] = field(default_factory=list)


@dataclass
class PackedChunks:
    """The chunk dictionaries of n records, flattened (`nhip_ms_chunks`)."""
    entry_off: np.ndarray
    chunk_index: np.ndarray
    path_off: np.ndarray
    path: np.ndarray
    rel_off: np.ndarray
    rel: np.ndarray

    def _c(self):
        return _lib.MsChunks(_ptr(self.entry_off), _ptr(self.chunk_index), _ptr(self.path_off), _ptr(self.path),
                             _ptr(self.rel_off), _ptr(self.rel))


def pack_paths(paths: Sequence[Sequence[Sequence[int]]]) -> Tuple[np.ndarray, np.ndarray]:
    """CSR form of ragged digest paths: `off[n + 1]` in digests, the digests back to back."""
    off = np.zeros(len(paths) + 1, dtype=np.uint64)
    if len(paths):
        off[1:] = np.cumsum([len(p) for p in paths], dtype=np.uint64)
    flat = [d for p in paths for d in p]
    data = _digests(flat) if flat else np.zeros((0, 5), dtype=np.uint64)
    return off, data


def pack_chunks(records) -> PackedChunks:
    """Pure CSR packing of the `target_chunks` of `records` (RemovalRecords or MsMembershipProofs)."""
    entries = [e for r in records for e in r.target_chunks]
    entry_off = np.zeros(len(records) + 1, dtype=np.uint64)
    if len(records):
        entry_off[1:] = np.cumsum([len(r.target_chunks) for r in records], dtype=np.uint64)
    chunk_index = np.asarray([int(ci) for ci, _, _ in entries], dtype=np.uint64)
    path_off, path = pack_paths([p for _, p, _ in entries])
    rel_off = np.zeros(len(entries) + 1, dtype=np.uint64)
    if entries:
        rel_off[1:] = np.cumsum([len(c.relative_indices) for _, _, c in entries], dtype=np.uint64)
    rel = np.asarray([int(x) for _, _, c in entries for x in c.relative_indices], dtype=np.uint32)
    return PackedChunks(entry_off, chunk_index, path_off, path, rel_off, rel)


def unpack_chunks(packed: PackedChunks) -> List[List[Tuple[int, List[Tuple[int, ...]], Chunk]]]:
    """Inverse of `pack_chunks`: the `target_chunks` list of every record."""
    out = []
    for i in range(len(packed.entry_off) - 1):
        tc = []
        for e in range(int(packed.entry_off[i]), int(packed.entry_off[i + 1])):
            p = packed.path[int(packed.path_off[e]):int(packed.path_off[e + 1])]
            r = packed.rel[int(packed.rel_off[e]):int(packed.rel_off[e + 1])]
            tc.append((int(packed.chunk_index[e]), [tuple(int(x) for x in d) for d in p], Chunk([int(x) for x in r])))
        out.append(tc)
    return out


def _ptr(a: np.ndarray):
    return a.ctypes.data if a.size else None


def mmr_verify_batch(ctx, mmr: MmrAccumulator, items) -> List[bool]:
    """`items`: `(leaf_index, leaf_digest, path)` triples, all against `mmr`."""
    n = len(items)
    if n == 0:
        return []
    cm, _keep = mmr._c()
    leaf_index = np.asarray([int(i) for i, _, _ in items], dtype=np.uint64)
    leaves = _digests([l for _, l, _ in items], n)
    off, path = pack_paths([p for _, _, p in items])
    v = np.zeros(n, dtype=np.uint8)
    check(ctx.lib.nhip_mmr_verify_batch(ctx.handle, ctypes.byref(cm), leaf_index.ctypes.data, leaves.ctypes.data,
                                        off.ctypes.data, _ptr(path), n, v.ctypes.data), "nhip_mmr_verify_batch")
    return [bool(x) for x in v]


def can_remove_batch(ctx, msa: MutatorSetAccumulator, records: Sequence[RemovalRecord]) -> List[Tuple[bool, bool, int]]:
    """`(validate, can_remove, status)` of every record against `msa`."""
    n = len(records)
    if n == 0:
        return []
    cm, _keep = msa._c()
    mn, dist = _index_arrays(records)
    packed = pack_chunks(records)
    cc = packed._c()
    valid, can, status = (np.zeros(n, dtype=np.uint8) for _ in range(3))
    check(ctx.lib.nhip_ms_can_remove_batch(ctx.handle, ctypes.byref(cm), mn.ctypes.data, dist.ctypes.data,
                                           ctypes.byref(cc), n, valid.ctypes.data, can.ctypes.data,
                                           status.ctypes.data), "nhip_ms_can_remove_batch")
    return [(bool(valid[i]), bool(can[i]), int(status[i])) for i in range(n)]


def verify_batch(ctx, msa: MutatorSetAccumulator, items, proofs: Sequence[MsMembershipProof]) -> List[Tuple[bool, int]]:
    """`(verdict, status)` of `msa.verify(item, proof)` for every pair."""
    n = len(proofs)
    if len(items) != n:
        raise ValueError("one membership proof per item")
    if n == 0:
        return []
    cm, _keep = msa._c()
    it = _digests(items, n)
    sr = _digests([p.sender_randomness for p in proofs], n)
    rp = _digests([p.receiver_preimage for p in proofs], n)
    leaf = np.asarray([int(p.aocl_leaf_index) for p in proofs], dtype=np.uint64)
    off, path = pack_paths([p.auth_path_aocl for p in proofs])
    packed = pack_chunks(proofs)
    cc = packed._c()
    v, status = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    check(ctx.lib.nhip_ms_verify_batch(ctx.handle, ctypes.byref(cm), it.ctypes.data, sr.ctypes.data, rp.ctypes.data,
                                       leaf.ctypes.data, off.ctypes.data, _ptr(path), ctypes.byref(cc), n,
                                       v.ctypes.data, status.ctypes.data), "nhip_ms_verify_batch")
    return [(bool(v[i]), int(status[i])) for i in range(n)]


@dataclass
class MutatorSetUpdate:
    """block/mutator_set_update.rs:14-21: the removal records of a block in block order, and its addition
    records (each an `AdditionRecord::canonical_commitment` digest)."""
    removals: Sequence[RemovalRecord] = ()
    additions: Sequence[Sequence[int]] = ()


def _index_arrays(records):
    n = len(records)
    mn = np.zeros((n, 2), dtype=np.uint64)
    dist = np.zeros((n, NUM_TRIALS), dtype=np.uint32)
    for i, r in enumerate(records):
        m = int(r.absolute_indices.minimum)
        mn[i] = (m & (2 ** 64 - 1), m >> 64)
        dist[i] = np.asarray(r.absolute_indices.distances, dtype=np.uint32)
    return mn, dist


def _csr(counts) -> np.ndarray:
    off = np.zeros(len(counts) + 1, dtype=np.uint64)
    if len(counts):
        off[1:] = np.cumsum(counts, dtype=np.uint64)
    return off


class PackedApply:
    """The arguments of one `nhip_ms_apply_batch` call over numpy arrays: `cin` / `cout` are the C structs,
    `arrays` keeps every array they point into alive (and lets a caller read the outputs)."""

    def __init__(self, jobs, expected=None):
        n = self.n = len(jobs)
        if expected is not None and len(expected) != n:
            raise ValueError("one expected accumulator per job")
        self._keep = []
        self.before = (_lib.Msa * max(n, 1))()
        for j, (msa, _) in enumerate(jobs):
            self.before[j], k = msa._c()
            self._keep.append(k)
        self.expected = None
        if expected is not None:
            self.expected = (_lib.Msa * max(n, 1))()
            for j, msa in enumerate(expected):
                self.expected[j], k = msa._c()
                self._keep.append(k)
        adds = [d for _, u in jobs for d in u.additions]
        records = [r for _, u in jobs for r in u.removals]
        mn, dist = _index_arrays(records)
        self.packed = pack_chunks(records)
        self.chunks = self.packed._c()
        z = lambda dtype, *shape: np.zeros(shape, dtype=dtype)  # noqa: E731
        self.arrays = a = dict(
            additions=_digests(adds) if adds else z(np.uint64, 0, 5),
            add_off=_csr([len(u.additions) for _, u in jobs]), rec_off=_csr([len(u.removals) for _, u in jobs]),
            minimum=mn, distances=dist, verdict=z(np.uint8, n), status=z(np.uint8, n), bad_record=z(np.uint64, n),
            aocl_peaks=z(np.uint64, n, 64, 5), aocl_n_peaks=z(np.uint32, n), aocl_num_leafs=z(np.uint64, n),
            swbf_peaks=z(np.uint64, n, 64, 5), swbf_n_peaks=z(np.uint32, n), swbf_num_leafs=z(np.uint64, n),
            active_off=_csr([len(msa.swbf_active) + NUM_TRIALS * len(u.removals) for msa, u in jobs]),
            n_active=z(np.uint64, n))
        a["active"] = z(np.uint32, max(int(a["active_off"][-1]), 1))
        self.cin = _lib.MsApplyIn(n, self.before, a["add_off"].ctypes.data, _ptr(a["additions"]),
                                  a["rec_off"].ctypes.data, _ptr(mn), _ptr(dist), ctypes.pointer(self.chunks),
                                  self.expected)
        self.cout = _lib.MsApplyOut(*(a[f].ctypes.data for f, _ in _lib.MsApplyOut._fields_))

    def call(self, ctx, packed=False) -> int:
        """`packed`: the removals are packed lists (`nhip_ms_apply_batch_packed`)."""
        fn = ctx.lib.nhip_ms_apply_batch_packed if packed else ctx.lib.nhip_ms_apply_batch
        return fn(ctx.handle, ctypes.byref(self.cin), ctypes.byref(self.cout))


def apply_update_batch(ctx, jobs, expected=None, _packed=False):
    """`jobs`: `(MutatorSetAccumulator before, MutatorSetUpdate)` pairs, independent of each other;
    `expected`: one `MutatorSetAccumulator` per job, or None.  Per job `(verdict, status, bad_record,
    msa_after)`: `bad_record` is the position in the job's removals of the record the status blames
    (None when it blames none), and `msa_after` is the accumulator after the update when the status is
    OK or UPDATE_MISMATCH, else None.  The steps and their order are those of `nhip_ms_apply_batch`."""
    n = len(jobs)
    if n == 0:
        return []
    pa = PackedApply(jobs, expected)
    check(pa.call(ctx, _packed), "nhip_ms_apply_batch_packed" if _packed else "nhip_ms_apply_batch")
    return _apply_results(pa)


def _apply_results(pa):
    a = pa.arrays
    out = []
    for j in range(pa.n):
        after = None
        status = int(a["status"][j])
        if status in (OK, UPDATE_MISMATCH):
            mmrs = [MmrAccumulator([tuple(int(x) for x in d) for d in a[w + "_peaks"][j, :int(a[w + "_n_peaks"][j])]],
                                   int(a[w + "_num_leafs"][j])) for w in ("aocl", "swbf")]
            lo = int(a["active_off"][j])
            after = MutatorSetAccumulator(mmrs[0], mmrs[1], [int(x) for x in a["active"][lo:lo + int(a["n_active"][j])]])
        bad = int(a["bad_record"][j])
        out.append((bool(a["verdict"][j]), status, None if bad == 2 ** 64 - 1 else bad, after))
    return out


def apply_update_batch_packed(ctx, jobs, expected=None):
    """`apply_update_batch` over jobs whose `removals` are packed lists (`RemovalRecordList::pack`): block rules
    2.a-2.e in one call.  A job whose list does not unpack has verdict False, its `UNPACK_*` status, no blamed
    record and no accumulator.  The unpacked paths are produced and consumed on the device."""
    return apply_update_batch(ctx, jobs, expected, _packed=True)


class PackedLists:
    """The arguments of `nhip_ms_unpack_plan` / `nhip_ms_unpack_batch` for `jobs`, each a packed list of
    `RemovalRecord`s (an entry's key in the place of its chunk index, its authentication structure in the place of
    its path, its chunk's packed words as the relative indices)."""

    def __init__(self, jobs):
        self.n = len(jobs)
        records = [r for job in jobs for r in job]
        self.n_records = len(records)
        self.rec_off = _csr([len(job) for job in jobs])
        self.minimum, self.distances = _index_arrays(records)
        self.index_sets = [r.absolute_indices for r in records]
        self.packed = pack_chunks(records)
        self.chunks = self.packed._c()

    def run(self, lib, handle=None):
        """Both calls of the two-call pattern.  `(status, num_leafs_aocl, PackedChunks)`; with no `handle` the host
        plan alone, whose `path` stays zero."""
        n = self.n
        status, leafs = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint64)
        out = _lib.MsUnpacked(status=_ptr(status), num_leafs_aocl=_ptr(leafs))
        args = (self.rec_off.ctypes.data, n, _ptr(self.minimum), _ptr(self.distances), ctypes.byref(self.chunks),
                ctypes.byref(out))
        name = "nhip_ms_unpack_plan" if handle is None else "nhip_ms_unpack_batch"
        call = (lambda: lib.nhip_ms_unpack_plan(*args)) if handle is None else \
            (lambda: lib.nhip_ms_unpack_batch(handle, *args))
        check(call(), name)
        E, PD, W = int(out.entries), int(out.path_digests), int(out.rel_words)
        u = PackedChunks(np.zeros(self.n_records + 1, dtype=np.uint64), np.zeros(E, dtype=np.uint64),
                         np.zeros(E + 1, dtype=np.uint64), np.zeros((PD, 5), dtype=np.uint64),
                         np.zeros(E + 1, dtype=np.uint64), np.zeros(W, dtype=np.uint32))
        out.entry_off, out.chunk_index, out.path_off = u.entry_off.ctypes.data, _ptr(u.chunk_index), u.path_off.ctypes.data
        out.path, out.rel_off, out.rel = _ptr(u.path), u.rel_off.ctypes.data, _ptr(u.rel)
        out.entries_cap, out.path_cap, out.rel_cap = E, PD, W
        check(call(), name)
        return status, leafs, u


def unpack_plan_batch(jobs):
    """The host half of `unpack_removal_records_batch` (no GPU): `(status, num_leafs_aocl, PackedChunks)` over all
    records of all jobs, the paths' digests left zero."""
    return PackedLists(jobs).run(_lib.load())


def unpack_removal_records_batch(ctx, jobs):
    """`RemovalRecordList::try_unpack` of every packed list in `jobs`: per job `(status, records)`, the records
    None unless the status is OK.  Every status is the host plan's integer decision; every path digest is the
    device's."""
    pl = PackedLists(jobs)
    status, _, u = pl.run(ctx.lib, ctx.handle)
    dictionaries = unpack_chunks(u)
    out = []
    for j in range(pl.n):
        lo, hi = int(pl.rec_off[j]), int(pl.rec_off[j + 1])
        recs = [RemovalRecord(pl.index_sets[r], dictionaries[r]) for r in range(lo, hi)]
        out.append((int(status[j]), recs if int(status[j]) == OK else None))
    return out


# ---------------------------------------------------------------- witnesses across a block
@dataclass
class Witness:
    """What `nhip_ms_update_batch` brings up to date: an index set and a chunk dictionary, and for a membership
    proof its AOCL part (leaf index, the addition record's canonical commitment, authentication path).
    `aocl_leaf_index` None: a removal record."""
    absolute_indices: AbsoluteIndexSet
    target_chunks: List[Tuple[int, Sequence[Sequence[int]], Chunk]] = field(default_factory=list)
    aocl_leaf_index: Optional[int] = None
    aocl_leaf: Sequence[int] = ()
    auth_path_aocl: Sequence[Sequence[int]] = ()


class PackedUpdate:
    """The arguments of `nhip_ms_update_plan` / `nhip_ms_update_batch` over numpy arrays.  `jobs`: `(msa_before,
    MutatorSetUpdate, witnesses)` triples.  `apply` is the block half (`PackedApply`), `win` the witnesses' struct,
    `out` the output arrays once `plan` or `run` has sized them.  `revert`: the same structs for
    `nhip_ms_revert_plan` / `nhip_ms_revert_batch`, the witnesses standing after the block."""

    def __init__(self, jobs, expected=None, revert=False):
        self.n = len(jobs)
        self.plan_name, self.batch_name = (("nhip_ms_revert_plan", "nhip_ms_revert_batch") if revert else
                                           ("nhip_ms_update_plan", "nhip_ms_update_batch"))
        self.apply = PackedApply([(m, u) for m, u, _ in jobs], expected)
        wits = self.witnesses = [w for _, _, ws in jobs for w in ws]
        W = self.n_witnesses = len(wits)
        self.wit_off = _csr([len(ws) for _, _, ws in jobs])
        self.minimum, self.distances = _index_arrays(wits)
        self.leaf_index = np.asarray([2 ** 64 - 1 if w.aocl_leaf_index is None else int(w.aocl_leaf_index) for w in wits],
                                     dtype=np.uint64)
        self.leaf = np.zeros((W, 5), dtype=np.uint64)
        for i, w in enumerate(wits):
            if w.aocl_leaf_index is not None:
                self.leaf[i] = np.asarray([int(x) for x in w.aocl_leaf], dtype=np.uint64)
        self.aocl_path_off, self.aocl_path = pack_paths([w.auth_path_aocl for w in wits])
        self.packed = pack_chunks(wits)
        self.chunks = self.packed._c()
        self.win = _lib.MsUpdateIn(self.wit_off.ctypes.data, _ptr(self.minimum), _ptr(self.distances),
                                   _ptr(self.leaf_index), _ptr(self.leaf), self.aocl_path_off.ctypes.data,
                                   _ptr(self.aocl_path), ctypes.pointer(self.chunks))
        self.out = None
        self.cout = None

    def _call(self, lib, handle):
        if handle is None:
            return getattr(lib, self.plan_name)(ctypes.byref(self.apply.cin), ctypes.byref(self.win), ctypes.byref(self.cout))
        return getattr(lib, self.batch_name)(handle, ctypes.byref(self.apply.cin), ctypes.byref(self.apply.cout),
                                             ctypes.byref(self.win), ctypes.byref(self.cout))

    def run(self, lib, handle=None) -> int:
        """Both calls of the two-call pattern; with no `handle` the host plan alone (statuses, digests and chunk
        words stay zero).  Returns the second call's code; `out` holds the arrays."""
        W = self.n_witnesses
        self.cout = _lib.MsUpdated()
        rc = getattr(lib, self.plan_name)(ctypes.byref(self.apply.cin), ctypes.byref(self.win), ctypes.byref(self.cout))
        if rc != _lib.NHIP_OK:
            return rc
        A, E, PD, RW = (int(getattr(self.cout, f)) for f in ("aocl_digests", "entries", "path_digests", "rel_words"))
        z = lambda dtype, *shape: np.zeros(shape, dtype=dtype)  # noqa: E731
        o = self.out = dict(status=z(np.uint8, W), aocl_path_off=z(np.uint64, W + 1), aocl_path=z(np.uint64, A, 5),
                            entry_off=z(np.uint64, W + 1), chunk_index=z(np.uint64, E), path_off=z(np.uint64, E + 1),
                            path=z(np.uint64, PD, 5), rel_off=z(np.uint64, E + 1), rel=z(np.uint32, RW))
        # a zero-size array still gets an address: only the count pass has null array pointers
        self._pad = {f: (a if a.size else np.zeros(1, dtype=a.dtype)) for f, a in o.items()}
        self.cout = _lib.MsUpdated(*(self._pad[f].ctypes.data for f, _ in _lib.MsUpdated._fields_[:9]), A, E, PD, RW)
        return self._call(lib, handle)

    def dictionaries(self) -> PackedChunks:
        o = self.out
        return PackedChunks(o["entry_off"], o["chunk_index"], o["path_off"], o["path"], o["rel_off"], o["rel"])


def update_plan_batch(jobs):
    """The host half of `update_witnesses_batch` (no GPU): the output arrays as `nhip_ms_update_plan` lays them out
    (`aocl_path_off`, `entry_off`, `chunk_index`, `path_off`, `rel_off`; the rest zero)."""
    pu = PackedUpdate(jobs)
    check(pu.run(_lib.load()), "nhip_ms_update_plan")
    return pu.out


def update_witnesses_batch(ctx, jobs, expected=None):
    """`jobs`: `(MutatorSetAccumulator before, MutatorSetUpdate, [Witness])` triples, independent of each other.  Per
    job `(verdict, status, bad_record, msa_after, witnesses)` with the first four as `apply_update_batch` gives them
    and `witnesses` a list of `(status, Witness after the block or None)`: a witness is brought up to date only when
    its job's status is OK and it passes admission against `msa_before` (the order of `nhip_ms_update_batch`)."""
    return _witnesses_batch(ctx, jobs, expected, False)


def _witnesses_batch(ctx, jobs, expected, revert):
    if len(jobs) == 0:
        return []
    pu = PackedUpdate(jobs, expected, revert)
    check(pu.run(ctx.lib, ctx.handle), pu.batch_name)
    block = _apply_results(pu.apply)
    o = pu.out
    dictionaries = unpack_chunks(pu.dictionaries())
    out = []
    for j in range(pu.n):
        ws = []
        for i in range(int(pu.wit_off[j]), int(pu.wit_off[j + 1])):
            st, old = int(o["status"][i]), pu.witnesses[i]
            if st != OK:
                ws.append((st, None))
                continue
            path = [tuple(int(x) for x in d) for d in o["aocl_path"][int(o["aocl_path_off"][i]):int(o["aocl_path_off"][i + 1])]]
            ws.append((st, Witness(old.absolute_indices, dictionaries[i], old.aocl_leaf_index, old.aocl_leaf, path)))
        out.append(block[j] + (ws,))
    return out


def update_membership_proofs(ctx, msa_before: MutatorSetAccumulator, update: MutatorSetUpdate, items,
                             proofs: Sequence[MsMembershipProof]):
    """The wallet's step after a block (wallet_state.rs:1375,1481): every monitored UTXO's membership proof brought
    up to the accumulator after `update`.  The index sets (`AbsoluteIndexSet::compute`) and the AOCL leaves
    (`hash_pair(hash_pair(item, sender_randomness), hash_pair(receiver_preimage, 0))`) are derived on the device.
    `(job status, msa_after or None, [(status, MsMembershipProof or None)])`."""
    return _membership_proofs(ctx, msa_before, update, items, proofs, False)


def _membership_proofs(ctx, msa_before, update, items, proofs, revert):
    if len(items) != len(proofs):
        raise ValueError("one membership proof per item")
    wits = []
    if len(proofs):
        it = _digests(items, len(proofs))
        sr = _digests([p.sender_randomness for p in proofs], len(proofs))
        rp = _digests([p.receiver_preimage for p in proofs], len(proofs))
        sets = AbsoluteIndexSet.compute_batch(ctx, it, sr, rp, [int(p.aocl_leaf_index) for p in proofs])
        leaves = ctx.hash_pair(ctx.hash_pair(it, sr), ctx.hash_pair(rp, np.zeros_like(rp)))
        wits = [Witness(s, list(p.target_chunks), int(p.aocl_leaf_index), [int(x) for x in leaf], list(p.auth_path_aocl))
                for s, p, leaf in zip(sets, proofs, leaves)]
    _, status, _, after, ws = _witnesses_batch(ctx, [(msa_before, update, wits)], None, revert)[0]
    out = [(st, None if w is None else MsMembershipProof(p.sender_randomness, p.receiver_preimage, w.auth_path_aocl,
                                                         p.aocl_leaf_index, w.target_chunks))
           for (st, w), p in zip(ws, proofs)]
    return status, after, out


def update_removal_records(ctx, msa_before: MutatorSetAccumulator, update: MutatorSetUpdate,
                           records: Sequence[RemovalRecord]):
    """The mempool's step after a block (state/mod.rs:1537,1557,2507,2522): every pending transaction's removal records
    brought up to the accumulator after `update`.  `(job status, msa_after or None, [(status, RemovalRecord or
    None)])`."""
    wits = [Witness(r.absolute_indices, list(r.target_chunks)) for r in records]
    _, status, _, after, ws = update_witnesses_batch(ctx, [(msa_before, update, wits)])[0]
    return status, after, [(st, None if w is None else RemovalRecord(w.absolute_indices, w.target_chunks)) for st, w in ws]


# ---------------------------------------------------------------- witnesses back across a block
def revert_plan_batch(jobs):
    """The host half of `revert_witnesses_batch` (no GPU): the output arrays as `nhip_ms_revert_plan` lays them out
    (`aocl_path_off`, `entry_off`, `chunk_index`, `path_off`, `rel_off`; the rest zero)."""
    pu = PackedUpdate(jobs, revert=True)
    check(pu.run(_lib.load()), "nhip_ms_revert_plan")
    return pu.out


def revert_witnesses_batch(ctx, jobs, expected=None):
    """`jobs`: `(MutatorSetAccumulator before, MutatorSetUpdate, [Witness])` triples as `update_witnesses_batch` takes
    them, but the witnesses stand at the accumulator *after* the block and are taken back to `msa_before`
    (`expected`: that accumulator after, checked by rule 2.e).  Per job `(verdict, status, bad_record, msa_after,
    witnesses)`, `witnesses` a list of `(status, Witness before the block or None)`: a witness comes back only when
    its job's status is OK, it passes admission and, reverted, it authenticates against `msa_before` (the order of
    `nhip_ms_revert_batch`)."""
    return _witnesses_batch(ctx, jobs, expected, True)


def revert_membership_proofs(ctx, msa_before: MutatorSetAccumulator, update: MutatorSetUpdate, items,
                             proofs: Sequence[MsMembershipProof]):
    """The wallet's step for an abandoned block during a reorganisation (state/mod.rs:1392-1497): every monitored
    UTXO's membership proof, standing after `update`, taken back to `msa_before`.  A proof born in the block gets
    NOT_IN_AOCL.  `(job status, msa_after or None, [(status, MsMembershipProof or None)])`."""
    return _membership_proofs(ctx, msa_before, update, items, proofs, True)


# ---------------------------------------------------------------- witnesses resident on the device
class PackedWitnesses:
    """The witness half of `PackedUpdate` alone: `win` is the `nhip_ms_update_in` of `witnesses` as one job."""

    def __init__(self, witnesses):
        wits = self.witnesses = list(witnesses)
        W = self.n = len(wits)
        self.wit_off = _csr([W])
        self.minimum, self.distances = _index_arrays(wits)
        self.leaf_index = np.asarray([2 ** 64 - 1 if w.aocl_leaf_index is None else int(w.aocl_leaf_index) for w in wits],
                                     dtype=np.uint64)
        self.leaf = np.zeros((W, 5), dtype=np.uint64)
        for i, w in enumerate(wits):
            if w.aocl_leaf_index is not None:
                self.leaf[i] = np.asarray([int(x) for x in w.aocl_leaf], dtype=np.uint64)
        self.aocl_path_off, self.aocl_path = pack_paths([w.auth_path_aocl for w in wits])
        self.packed = pack_chunks(wits)
        self.chunks = self.packed._c()
        self.win = _lib.MsUpdateIn(self.wit_off.ctypes.data, _ptr(self.minimum), _ptr(self.distances),
                                   _ptr(self.leaf_index), _ptr(self.leaf), self.aocl_path_off.ctypes.data,
                                   _ptr(self.aocl_path), ctypes.pointer(self.chunks))


class WitnessStore:
    """Membership proofs and removal records kept on the device across blocks (`nhip_ms_store_*`): `append` uploads
    witnesses once, `update` brings all of them across one block where they lie (only the block goes up and one
    status byte per witness comes back), `revert` takes all of them back across one when the tip moves to another
    fork, `read` copies chosen ones out, `retain` drops the others, `check` answers
    "which of them verify / can still be removed" against an accumulator.  Witnesses keep their positions
    `0 .. len - 1` in insertion order until `retain`.  A witness whose status after an update is not OK keeps that
    status (and zeroed slots) until `retain` drops it.  `initial`: a dict of initial capacities (`witnesses`,
    `aocl_digests`, `entries`, `path_digests`, `rel_words`), or None."""

    def __init__(self, ctx, initial=None):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        caps = _lib.MsStoreCaps(**initial) if initial else None
        check(ctx.lib.nhip_ms_store_create(ctx.handle, ctypes.byref(caps) if caps else None, ctypes.byref(self._h)),
              "nhip_ms_store_create")
        self._fixed = []  # per witness: (index set, leaf index, leaf), which no block changes

    def close(self):
        if self._h:
            self.ctx.lib.nhip_ms_store_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __len__(self):
        return len(self._fixed)

    def counts(self):
        """`(witnesses, aocl_digests, entries, path_digests, rel_words)` from the host mirror."""
        c = (ctypes.c_uint64 * 5)()
        check(self.ctx.lib.nhip_ms_store_count(self._h, *(ctypes.addressof(c) + 8 * i for i in range(5))),
              "nhip_ms_store_count")
        return tuple(int(x) for x in c)

    def append(self, witnesses):
        pw = PackedWitnesses(witnesses)
        check(self.ctx.lib.nhip_ms_store_append(self._h, ctypes.byref(pw.win), pw.n), "nhip_ms_store_append")
        self._fixed += [(w.absolute_indices, w.aocl_leaf_index, w.aocl_leaf) for w in pw.witnesses]

    def append_restored(self, archive, index_sets, aocl_leaf_indices, aocl_leaves=None):
        """`archive.restore_raw` + `append` in one call, device to device (`nhip_ms_store_append_restored`): the
        restore's shape is decided on the device, the gather writes into the store's own pools, and no path digest
        and no chunk word crosses to the host.  Returns the restore's status per witness.  All or nothing: unless
        every status is OK the store is unchanged; filter and call again.  `aocl_leaves`: the callers' commitments
        (anything where the leaf index is None), or None for the archive's own leaves at the leaf indices."""
        n = len(index_sets)
        if n == 0:
            return []

        class _S:  # _index_arrays reads `.absolute_indices`
            def __init__(self, s):
                self.absolute_indices = s
        sets = list(index_sets)
        mn, dist = _index_arrays([_S(s) for s in sets])
        leafs = [None if l is None else int(l) for l in aocl_leaf_indices]
        li = np.asarray([2 ** 64 - 1 if l is None else l for l in leafs], dtype=np.uint64)
        leaf = None
        if aocl_leaves is not None:
            leaf = np.zeros((n, 5), dtype=np.uint64)
            for i, l in enumerate(leafs):
                if l is not None:
                    leaf[i] = np.asarray([int(x) for x in aocl_leaves[i]], dtype=np.uint64)
        status = np.zeros(n, dtype=np.uint8)
        check(self.ctx.lib.nhip_ms_store_append_restored(self._h, archive._h, _ptr(mn), _ptr(dist), _ptr(li),
                                                         None if leaf is None else _ptr(leaf), n, _ptr(status)),
              "nhip_ms_store_append_restored")
        out = [int(x) for x in status]
        if any(st != OK for st in out):
            return out
        for i, l in enumerate(leafs):  # what `read` hands back beside the device's arrays
            if l is None:
                given = ()
            elif leaf is not None:
                given = tuple(int(x) for x in leaf[i])
            else:
                given = tuple(int(x) for x in archive.leaves(0, l, 1)[0])
            self._fixed.append((sets[i], l, given))
        return out

    def append_restored_membership_proofs(self, archive, items, sender_randomness, receiver_preimages,
                                          aocl_leaf_indices, aocl_leaves=None):
        """`append_restored` for items, as `Archive.restore_membership_proofs` takes them: the index sets are computed
        on the device (`nhip_absolute_index_sets`)."""
        n = len(aocl_leaf_indices)
        if n == 0:
            return []
        it, sr, rp = _digests(items, n), _digests(sender_randomness, n), _digests(receiver_preimages, n)
        leafs = [int(l) for l in aocl_leaf_indices]
        sets = AbsoluteIndexSet.compute_batch(self.ctx, it, sr, rp, leafs)
        return self.append_restored(archive, sets, leafs, aocl_leaves)

    def update(self, msa_before, update, expected=None):
        """One block: `((verdict, status, bad_record, msa_after), [status of every witness])`.  Unless the block's
        status is OK the store is unchanged and every witness status is JOB_REJECTED."""
        return self._cross("nhip_ms_store_update", msa_before, update, expected)

    def revert(self, msa_before, update, expected=None):
        """One block back: the store stands at the accumulator after `update` (`expected`, when given, is checked to
        be that accumulator) and is taken to `msa_before`.  Returns what `update` returns, under the same contract;
        a witness born in the block, or one that does not authenticate against `msa_before`, fails and stays failed."""
        return self._cross("nhip_ms_store_revert", msa_before, update, expected)

    def _cross(self, name, msa_before, update, expected):
        pa = PackedApply([(msa_before, update)], None if expected is None else [expected])
        status = np.zeros(max(len(self), 1), dtype=np.uint8)
        check(getattr(self.ctx.lib, name)(self._h, ctypes.byref(pa.cin), ctypes.byref(pa.cout), status.ctypes.data), name)
        return _apply_results(pa)[0], [int(x) for x in status[:len(self)]]

    def read_raw(self, indices=None):
        """Both calls of the two-call pattern: `(sel, count-pass totals, the output arrays)`."""
        if indices is None:
            sel, n = None, len(self)
        else:
            sel = np.ascontiguousarray(np.asarray(list(indices), dtype=np.uint64))
            n = sel.size
        cout = _lib.MsUpdated()
        p_sel = None if sel is None else (sel.ctypes.data if n else None)
        if sel is not None and n == 0:
            p_sel = np.zeros(1, dtype=np.uint64).ctypes.data  # an empty selection, not "all"
        check(self.ctx.lib.nhip_ms_store_read(self._h, p_sel, n, ctypes.byref(cout)), "nhip_ms_store_read")
        totals = tuple(int(getattr(cout, f)) for f in ("aocl_digests", "entries", "path_digests", "rel_words"))
        A, E, PD, RW = totals
        z = lambda dtype, *shape: np.zeros(shape, dtype=dtype)  # noqa: E731
        o = dict(status=z(np.uint8, n), aocl_path_off=z(np.uint64, n + 1), aocl_path=z(np.uint64, A, 5),
                 entry_off=z(np.uint64, n + 1), chunk_index=z(np.uint64, E), path_off=z(np.uint64, E + 1),
                 path=z(np.uint64, PD, 5), rel_off=z(np.uint64, E + 1), rel=z(np.uint32, RW))
        pad = {f: (a if a.size else np.zeros(1, dtype=a.dtype)) for f, a in o.items()}
        cout = _lib.MsUpdated(*(pad[f].ctypes.data for f, _ in _lib.MsUpdated._fields_[:9]), A, E, PD, RW)
        check(self.ctx.lib.nhip_ms_store_read(self._h, p_sel, n, ctypes.byref(cout)), "nhip_ms_store_read")
        filled = tuple(int(getattr(cout, f)) for f in ("aocl_digests", "entries", "path_digests", "rel_words"))
        if filled != totals:
            raise _lib.NhipError("nhip_ms_store_read: the count pass and the fill disagree")
        return (list(range(n)) if sel is None else [int(x) for x in sel]), totals, o

    def read(self, indices=None):
        """`[(status, Witness)]` of the chosen witnesses (None: all), in the order asked; a witness whose status is
        not OK comes with its zeroed slots."""
        sel, _, o = self.read_raw(indices)
        dictionaries = unpack_chunks(PackedChunks(o["entry_off"], o["chunk_index"], o["path_off"], o["path"],
                                                  o["rel_off"], o["rel"]))
        out = []
        for i, w in enumerate(sel):
            idx, leaf_index, leaf = self._fixed[w]
            path = [tuple(int(x) for x in d) for d in o["aocl_path"][int(o["aocl_path_off"][i]):int(o["aocl_path_off"][i + 1])]]
            out.append((int(o["status"][i]), Witness(idx, dictionaries[i], leaf_index, leaf, path)))
        return out

    def retain(self, mask):
        mask = [bool(x) for x in mask]
        if len(mask) != len(self):
            raise ValueError("one flag per witness")
        keep = np.asarray(mask, dtype=np.uint8)
        check(self.ctx.lib.nhip_ms_store_retain(self._h, _ptr(keep)), "nhip_ms_store_retain")
        self._fixed = [f for f, k in zip(self._fixed, mask) if k]

    def check(self, msa):
        """`[(aocl_member, valid, can_remove, status)]` of every witness against `msa`."""
        n = len(self)
        cm, _keep = msa._c()
        a = [np.zeros(max(n, 1), dtype=np.uint8) for _ in range(4)]
        check(self.ctx.lib.nhip_ms_store_check(self._h, ctypes.byref(cm), *(x.ctypes.data for x in a)),
              "nhip_ms_store_check")
        return [(bool(a[0][i]), bool(a[1][i]), bool(a[2][i]), int(a[3][i])) for i in range(n)]


# ---------------------------------------------------------------- the archival mutator set on the device
WINDOW_SIZE = 1 << 20


def aocl_range(index_set: AbsoluteIndexSet) -> Tuple[int, int]:
    """`AbsoluteIndexSet::aocl_range` (absolute_index_set.rs:174-220): the inclusive range of AOCL leaf indices an
    item with this index set can have, whatever the AOCL's length.  An index is a relative index below WINDOW_SIZE
    plus `batch_index * CHUNK_SIZE`, and a batch holds BATCH_SIZE leaves: the lowest batch is the first whose window
    reaches the largest index, the highest the last whose window begins at or before the smallest.  ValueError where
    the reference gives AbsoluteIndexExceedsTheoreticalBound."""
    mn, spread = int(index_set.minimum), max(int(d) for d in index_set.distances)
    if spread >= WINDOW_SIZE:
        raise ValueError("AbsoluteIndexExceedsTheoreticalBound")
    lo_batch = -(-max(mn + spread - (WINDOW_SIZE - 1), 0) // CHUNK_SIZE)
    hi_batch = mn // CHUNK_SIZE
    lo, hi = lo_batch * BATCH_SIZE, hi_batch * BATCH_SIZE + BATCH_SIZE - 1
    if lo_batch >= 1 << 64 or hi_batch >= 1 << 64 or lo >= 1 << 64 or hi >= 1 << 64:
        raise ValueError("AbsoluteIndexExceedsTheoreticalBound")
    return lo, hi


class Archive:
    """`ArchivalMutatorSet` (util_types/mutator_set/archival_mutator_set.rs) resident on the device
    (`nhip_ms_archive_*`): every node of both MMRs, every chunk and the window.  `load` uploads a whole set once and
    builds every digest on the device; `apply` advances it across one block and `revert` takes it back across one; `accumulator` reads the `MutatorSetAccumulator`; `aocl_paths`, `swbf_paths`
    and `leaves` are the archival MMRs' `prove_membership` and `get_leaf_range_inclusive`;
    `restore_membership_proofs`, `restore_dictionaries` and `restore_privacy_preserving` make fresh witnesses, in
    the form `WitnessStore.append` takes.  `initial`: a dict of initial capacities (`aocl_leafs`, `chunks`,
    `rel_words`), or None."""

    def __init__(self, ctx, initial=None):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        caps = _lib.MsArchiveCaps(**initial) if initial else None
        check(ctx.lib.nhip_ms_archive_create(ctx.handle, ctypes.byref(caps) if caps else None, ctypes.byref(self._h)),
              "nhip_ms_archive_create")

    def close(self):
        if self._h:
            self.ctx.lib.nhip_ms_archive_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def counts(self):
        """`(aocl_leafs, chunks, n_active, rel_live, rel_dead)` from the host mirror."""
        c = (ctypes.c_uint64 * 5)()
        check(self.ctx.lib.nhip_ms_archive_count(self._h, *(ctypes.addressof(c) + 8 * i for i in range(5))),
              "nhip_ms_archive_count")
        return tuple(int(x) for x in c)

    def load_raw(self, leaves, rel_off, rel, active) -> int:
        """`nhip_ms_archive_load` over arrays as given; the return code."""
        leaves = np.ascontiguousarray(np.asarray(leaves, dtype=np.uint64)).reshape(-1, 5)
        rel_off = np.ascontiguousarray(np.asarray(rel_off, dtype=np.uint64)).reshape(-1)
        rel = np.ascontiguousarray(np.asarray(rel, dtype=np.uint32)).reshape(-1)
        active = np.ascontiguousarray(np.asarray(active, dtype=np.uint32)).reshape(-1)
        return self.ctx.lib.nhip_ms_archive_load(self._h, _ptr(leaves), leaves.shape[0], _ptr(rel_off), _ptr(rel),
                                                 max(rel_off.size, 1) - 1, _ptr(active), active.size)

    def load(self, aocl_leaves, chunks, active=()):
        """Into an empty archive: the AOCL leaves (addition records' canonical commitments), chunk c's relative
        indices `chunks[c]` (sorted) for every c below the batch index, and the window (sorted)."""
        rel_off = _csr([len(ch) for ch in chunks])
        rel = [int(x) for ch in chunks for x in ch]
        leaves = _digests(aocl_leaves) if len(aocl_leaves) else np.zeros((0, 5), dtype=np.uint64)
        check(self.load_raw(leaves, rel_off, rel, list(active)), "nhip_ms_archive_load")

    def apply(self, msa_before, update, expected=None):
        """One block (`ArchivalState::update_mutator_set`'s forward step): `(verdict, status, bad_record, msa_after)`
        as `apply_update_batch` gives them.  `msa_before` has to be the archive's own accumulator (else INCONSISTENT);
        unless the status is OK the archive is unchanged."""
        pa = PackedApply([(msa_before, update)], None if expected is None else [expected])
        check(self.ctx.lib.nhip_ms_archive_apply(self._h, ctypes.byref(pa.cin), ctypes.byref(pa.cout)),
              "nhip_ms_archive_apply")
        return _apply_results(pa)[0]

    def revert(self, msa_before, update, expected=None):
        """One block back (`ArchivalState::update_mutator_set`'s walk over an abandoned block): the archive stands at
        the accumulator after `update` and is taken to `msa_before`.  `(verdict, status, bad_record, msa_after)` as
        `apply` gives them, `msa_after` being the tip the block leads to; UPDATE_MISMATCH if that is not the archive's
        own accumulator.  Unless the status is OK the archive is unchanged."""
        pa = PackedApply([(msa_before, update)], None if expected is None else [expected])
        check(self.ctx.lib.nhip_ms_archive_revert(self._h, ctypes.byref(pa.cin), ctypes.byref(pa.cout)),
              "nhip_ms_archive_revert")
        return _apply_results(pa)[0]

    def accumulator(self) -> MutatorSetAccumulator:
        n_active = self.counts()[2]
        z = lambda dtype, *shape: np.zeros(shape, dtype=dtype)  # noqa: E731
        a = dict(verdict=z(np.uint8, 1), status=z(np.uint8, 1), bad_record=z(np.uint64, 1),
                 aocl_peaks=z(np.uint64, 1, 64, 5), aocl_n_peaks=z(np.uint32, 1), aocl_num_leafs=z(np.uint64, 1),
                 swbf_peaks=z(np.uint64, 1, 64, 5), swbf_n_peaks=z(np.uint32, 1), swbf_num_leafs=z(np.uint64, 1),
                 active_off=np.asarray([0, n_active], dtype=np.uint64), active=z(np.uint32, max(n_active, 1)),
                 n_active=z(np.uint64, 1))
        cout = _lib.MsApplyOut(*(a[f].ctypes.data for f, _ in _lib.MsApplyOut._fields_))
        check(self.ctx.lib.nhip_ms_archive_accumulator(self._h, ctypes.byref(cout)), "nhip_ms_archive_accumulator")
        mmrs = [MmrAccumulator([tuple(int(x) for x in d) for d in a[w + "_peaks"][0, :int(a[w + "_n_peaks"][0])]],
                               int(a[w + "_num_leafs"][0])) for w in ("aocl", "swbf")]
        return MutatorSetAccumulator(mmrs[0], mmrs[1], [int(x) for x in a["active"][:int(a["n_active"][0])]])

    def paths_raw(self, which: int, leaf_indices):
        """Both calls of the two-call pattern: `(path_off, path)`."""
        idx = np.ascontiguousarray(np.asarray(list(leaf_indices), dtype=np.uint64))
        n = idx.size
        total = ctypes.c_size_t()
        check(self.ctx.lib.nhip_ms_archive_paths(self._h, which, _ptr(idx), n, None, None, 0, ctypes.byref(total)),
              "nhip_ms_archive_paths")
        off = np.zeros(n + 1, dtype=np.uint64)
        path = np.zeros((max(total.value, 1), 5), dtype=np.uint64)
        filled = ctypes.c_size_t()
        check(self.ctx.lib.nhip_ms_archive_paths(self._h, which, _ptr(idx), n, off.ctypes.data, path.ctypes.data,
                                                 total.value, ctypes.byref(filled)), "nhip_ms_archive_paths")
        if filled.value != total.value:
            raise _lib.NhipError("nhip_ms_archive_paths: the count pass and the fill disagree")
        return off, path[:total.value]

    def _paths(self, which, leaf_indices):
        off, path = self.paths_raw(which, leaf_indices)
        return [[tuple(int(x) for x in d) for d in path[int(off[i]):int(off[i + 1])]] for i in range(off.size - 1)]

    def aocl_paths(self, leaf_indices):
        """`MmrMembershipProof`s of AOCL leaves: a list of digest lists, leaf sibling first."""
        return self._paths(0, leaf_indices)

    def swbf_paths(self, chunk_indices):
        return self._paths(1, chunk_indices)

    def leaves(self, which: int, first: int, n: int) -> np.ndarray:
        """Leaves `first .. first + n - 1` of the AOCL (`which` 0) or of the SWBF MMR (1): n x 5 words."""
        out = np.zeros((n, 5), dtype=np.uint64)
        check(self.ctx.lib.nhip_ms_archive_leaves(self._h, which, first, n, _ptr(out)), "nhip_ms_archive_leaves")
        return out

    def restore_raw(self, index_sets, aocl_leaf_indices):
        """Both calls of the two-call pattern of `nhip_ms_archive_restore`: `(count-pass totals, output arrays)`."""
        return _restore_two_calls(lambda mn, dist, li, n, cout: self.ctx.lib.nhip_ms_archive_restore(
            self._h, _ptr(mn), _ptr(dist), _ptr(li), n, cout), "nhip_ms_archive_restore", index_sets, aocl_leaf_indices)

    def restore_shape(self, index_sets, aocl_leaf_indices):
        """`restore_plan` decided on the device from the archive's own chunk table (`nhip_ms_archive_restore_shape`):
        `(totals, output arrays)` in the same form, digests and chunk words zero."""
        return _restore_two_calls(lambda mn, dist, li, n, cout: self.ctx.lib.nhip_ms_archive_restore_shape(
            self._h, _ptr(mn), _ptr(dist), _ptr(li), n, cout), "nhip_ms_archive_restore_shape", index_sets,
            aocl_leaf_indices)

    def _restore(self, index_sets, aocl_leaf_indices):
        _, o = self.restore_raw(index_sets, aocl_leaf_indices)
        dictionaries = unpack_chunks(PackedChunks(o["entry_off"], o["chunk_index"], o["path_off"], o["path"],
                                                  o["rel_off"], o["rel"]))
        paths = [[tuple(int(x) for x in d) for d in o["aocl_path"][int(o["aocl_path_off"][i]):int(o["aocl_path_off"][i + 1])]]
                 for i in range(len(index_sets))]
        return [int(x) for x in o["status"]], paths, dictionaries

    def restore_membership_proofs(self, items, sender_randomness, receiver_preimages, aocl_leaf_indices):
        """`ArchivalMutatorSet::restore_membership_proof` (archival_mutator_set.rs:298-346) for many items:
        `[(status, MsMembershipProof or None)]`.  The index sets are computed on the device
        (`nhip_absolute_index_sets`)."""
        n = len(aocl_leaf_indices)
        if n == 0:
            return []
        it, sr, rp = _digests(items, n), _digests(sender_randomness, n), _digests(receiver_preimages, n)
        leafs = [int(l) for l in aocl_leaf_indices]
        sets = AbsoluteIndexSet.compute_batch(self.ctx, it, sr, rp, leafs)
        status, paths, dictionaries = self._restore(sets, leafs)
        return [(st, None if st != OK else
                 MsMembershipProof(tuple(int(x) for x in sr[i]), tuple(int(x) for x in rp[i]), paths[i], leafs[i],
                                   dictionaries[i])) for i, st in enumerate(status)]

    def restore_dictionaries(self, index_sets):
        """The chunk dictionaries of index sets against the archive's tip: `[(status, target_chunks or None)]`, as
        the refresh of old removal records needs them (state/archival_state.rs:1156-1179)."""
        if len(index_sets) == 0:
            return []
        status, _, dictionaries = self._restore(list(index_sets), [None] * len(index_sets))
        return [(st, dictionaries[i] if st == OK else None) for i, st in enumerate(status)]

    def restore_privacy_preserving(self, index_set):
        """`restore_membership_proof_privacy_preserving` (archival_mutator_set.rs:350-406):
        `(aocl_auth_paths, dictionary)`, the first a list of `(leaf index, path)` for every leaf index the index set
        admits (`aocl_range`, clipped to the leaf count), the second its `target_chunks`.  ValueError where the
        reference returns an error: a range that begins past the AOCL, an index set outside what the archive serves."""
        lo, hi = aocl_range(index_set)
        n = self.counts()[0]
        if lo >= n:
            raise ValueError("RequestedAoclAuthPathOutOfBounds")
        (status, dictionary), = self.restore_dictionaries([index_set])
        if status != OK:
            raise ValueError(status_name(status))
        leafs = list(range(lo, min(hi, n - 1) + 1))
        return list(zip(leafs, self.aocl_paths(leafs))), dictionary


def _restore_two_calls(call, name, index_sets, aocl_leaf_indices):
    n = len(index_sets)

    class _S:  # _index_arrays reads `.absolute_indices`
        def __init__(self, s):
            self.absolute_indices = s
    mn, dist = _index_arrays([_S(s) for s in index_sets])
    li = np.asarray([2 ** 64 - 1 if l is None else int(l) for l in aocl_leaf_indices], dtype=np.uint64)
    cout = _lib.MsUpdated()
    check(call(mn, dist, li, n, ctypes.byref(cout)), name)
    totals = tuple(int(getattr(cout, f)) for f in ("aocl_digests", "entries", "path_digests", "rel_words"))
    A, E, PD, RW = totals
    z = lambda dtype, *shape: np.zeros(shape, dtype=dtype)  # noqa: E731
    o = dict(status=z(np.uint8, n), aocl_path_off=z(np.uint64, n + 1), aocl_path=z(np.uint64, A, 5),
             entry_off=z(np.uint64, n + 1), chunk_index=z(np.uint64, E), path_off=z(np.uint64, E + 1),
             path=z(np.uint64, PD, 5), rel_off=z(np.uint64, E + 1), rel=z(np.uint32, RW))
    pad = {f: (a if a.size else np.zeros(1, dtype=a.dtype)) for f, a in o.items()}
    cout = _lib.MsUpdated(*(pad[f].ctypes.data for f, _ in _lib.MsUpdated._fields_[:9]), A, E, PD, RW)
    check(call(mn, dist, li, n, ctypes.byref(cout)), name)
    filled = tuple(int(getattr(cout, f)) for f in ("aocl_digests", "entries", "path_digests", "rel_words"))
    if filled != totals:
        raise _lib.NhipError(name + ": the count pass and the fill disagree")
    return totals, o


def restore_plan(aocl_leafs: int, chunk_lengths, index_sets, aocl_leaf_indices):
    """The host half of `Archive.restore_*` (no GPU, `nhip_ms_archive_restore_plan`): `(totals, output arrays)` with
    the statuses, the offset arrays and the keys; digests and chunk words stay zero."""
    lens = np.ascontiguousarray(np.asarray(list(chunk_lengths), dtype=np.uint64))
    lib = _lib.load()
    return _restore_two_calls(lambda mn, dist, li, n, cout: lib.nhip_ms_archive_restore_plan(
        int(aocl_leafs), _ptr(lens), lens.size, _ptr(mn), _ptr(dist), _ptr(li), n, cout),
        "nhip_ms_archive_restore_plan", index_sets, aocl_leaf_indices)
