"""Block files and peer transactions over the C ABI: bincode decoded
natively (csrc/bincode.cpp) straight into the verifier's inputs.

* `blocks_from_file_without_record(path)` — state/archival_state/import_blocks_from_files.rs:100-115:
  every `Block` of a blk file (bincode, back to back), as `BlockRecord`s.  A malformed block
  fails the whole file (the reference's `?`), with `BlockFileError.n_good` blocks before it.
* `blocks_to_validate(ctx, records)` — what `Block::validate` rules 1.a-1.d read
  (`verifier.BlockToValidate`): the transaction kernels' and then the bodies' MAST hashes
  (`MastHash::mast_hash`, block_body.rs:175-182, transaction_kernel.rs:246-277) in two GPU calls
  for the whole file, the appendix claims and the block proof.  `validate_block_file` then runs
  the bootstrap import's proof checks (state/mod.rs:2226-2272) for a file in ONE verifier batch.
* `TransferTransaction.from_bytes(data)` — protocol/peer/transfer_transaction.rs:31-47: the kernel's
  MAST sequences and the `TransactionProof` (SingleProof words or a `ProofCollection`), ready for
  `verifier.transactions_are_valid`.
* `block_digests` / `chain_links` / `chain_params` — `Block::hash`, and `Block::validate` rules 0.a-0.g with
  `Block::has_proof_of_work` for every (parent, child) pair of a file, each one call.
* `guesser_fee_addition_records` / `mutator_set_links` / `validate_chain_file` — the parent's guesser-fee addition
  records, and `Block::validate` rules 2.a-2.l for every (parent, child) pair of a file, each one call over the
  file's bytes; `mutator_set_parts` is the host walk behind them.
Proof words are copied once, reduced mod p, from the file bytes into numpy buffers that the
verifier stages without further conversion, or, given an `arena` (`stark.Arena`, round 6), straight
into pinned memory on a GPU's NUMA node (nhip_arena_ingest_blocks / _spans), from where the
verifier DMAs them as they lie.
"""
from __future__ import annotations

import ctypes
import mmap
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import NHIP_ERR_DECODE, check
from .stark import Claim

POW_TREE_HEIGHT = 29   # pow.rs:33-37 (production POW_MEMORY_PARAMETER = 2^29)
GENESIS_KIND, INVALID_KIND, SINGLE_PROOF_KIND = 0, 1, 2


class BlockFileError(ValueError):
    def __init__(self, msg, n_good):
        super().__init__(msg)
        self.n_good = n_good


def _buf(data) -> Tuple[np.ndarray, int]:
    a = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
    return a, len(data)


def _words(lib, a, n, offset, count) -> np.ndarray:
    out = np.zeros(max(count, 1), dtype=np.uint64)
    check(lib.nhip_le_words(a.ctypes.data, n, offset, count, out.ctypes.data), "nhip_le_words")
    return out[:count]


@dataclass
class BlockRecord:
    """One block of a blk file: header fields the callers print, the MAST sequences (kernel 8,
    body 2-4), the appendix claims and the block proof (`proof_kind` as block/mod.rs:114-119)."""
    offset: int
    size: int
    height: int
    timestamp: int
    prev_block_digest: Tuple[int, ...]
    kernel_sequences: List[np.ndarray]
    body_tail_sequences: List[np.ndarray]
    appendix: List[Claim]
    proof_kind: int
    proof: Optional[np.ndarray]


def blocks_from_bytes(data, pow_tree_height: int = POW_TREE_HEIGHT, arena=None) -> List[BlockRecord]:
    """`arena`: decode the block proofs into it (pinned, on its GPUs' nodes) instead of numpy
    buffers; each record's `proof` is then a view of the arena (valid until the arena's reset)."""
    lib = _lib.load()
    in_arena = {}
    if arena is not None:
        placed, block_of = arena.ingest_blocks(data, pow_tree_height)
        in_arena = {b: placed.words(i) for i, b in enumerate(block_of)}
    a, n = _buf(data)
    count = ctypes.c_size_t(0)
    rc = lib.nhip_blk_scan(a.ctypes.data, n, pow_tree_height, None, 0, ctypes.byref(count))
    if rc == NHIP_ERR_DECODE:
        raise BlockFileError(f"malformed block after {count.value} blocks", count.value)
    check(rc, "nhip_blk_scan")
    blocks = (_lib.BlkBlock * max(count.value, 1))()
    check(lib.nhip_blk_scan(a.ctypes.data, n, pow_tree_height, ctypes.cast(blocks, ctypes.c_void_p), count.value,
                            ctypes.byref(count)), "nhip_blk_scan")
    out = []
    for i in range(count.value):
        b = blocks[i]
        offs = np.zeros(12, dtype=np.uint64)
        words = np.zeros(max(int(b.seq_words), 1), dtype=np.uint64)
        check(lib.nhip_blk_sequences(a.ctypes.data, n, pow_tree_height, ctypes.byref(b), words.ctypes.data,
                                     words.size, offs.ctypes.data), "nhip_blk_sequences")
        seqs = [words[int(offs[j]):int(offs[j + 1])] for j in range(11)]
        cw = np.zeros(max(int(b.claim_words), 1), dtype=np.uint64)
        cl = (_lib.Claim * max(b.n_claims, 1))()
        check(lib.nhip_blk_claims(a.ctypes.data, n, ctypes.byref(b), cw.ctypes.data,
                                  ctypes.cast(cl, ctypes.c_void_p)), "nhip_blk_claims")
        claims = [Claim([int(x) for x in c.program_digest], int(c.version),
                        [int(c.input[k]) for k in range(c.input_len)],
                        [int(c.output[k]) for k in range(c.output_len)]) for c in cl[:b.n_claims]]
        proof = None
        if b.proof_kind == SINGLE_PROOF_KIND:
            proof = in_arena[i] if i in in_arena else _words(lib, a, n, int(b.proof_offset), int(b.proof_len))
        out.append(BlockRecord(int(b.offset), int(b.size), int(b.height), int(b.timestamp),
                               tuple(int(x) for x in b.prev_block_digest), seqs[:8], seqs[8:], claims,
                               int(b.proof_kind), proof))
    return out


def blocks_from_file_without_record(path: str, pow_tree_height: int = POW_TREE_HEIGHT, arena=None) -> List[BlockRecord]:
    """import_blocks_from_files.rs:100-115 (the file is memory-mapped, as there)."""
    if os.path.getsize(path) == 0:
        return []
    with open(path, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as m:
        return blocks_from_bytes(m, pow_tree_height, arena)


def blocks_to_validate(ctx, records: Sequence[BlockRecord]):
    """Kernel MAST hashes, then body MAST hashes (sequence 1 = the kernel hash's encoding), each
    for all blocks in one GPU call; returns `verifier.BlockToValidate`s."""
    from .mast import mast_hash_batch
    from .verifier import BlockToValidate, GENESIS, INVALID, SINGLE_PROOF
    if not records:
        return []
    txk = mast_hash_batch(ctx, [r.kernel_sequences for r in records])
    body = mast_hash_batch(ctx, [[list(h)] + list(r.body_tail_sequences) for h, r in zip(txk, records)])
    kinds = {GENESIS_KIND: GENESIS, INVALID_KIND: INVALID, SINGLE_PROOF_KIND: SINGLE_PROOF}
    return [BlockToValidate(list(bh), list(th), r.appendix, kinds[r.proof_kind], r.proof)
            for r, th, bh in zip(records, txk, body)]


def validate_block_file(ctx, path: str, verifier, programs, network=None,
                        pow_tree_height: int = POW_TREE_HEIGHT, arena=None) -> List[Optional[str]]:
    """Rules 1.a-1.d for every block of a blk file, all block proofs in one verifier batch;
    `arena`: the block proofs decoded straight into pinned memory (DMA'd from there)."""
    from .verifier import Network, validate_block_proofs
    recs = blocks_from_file_without_record(path, pow_tree_height, arena)
    return validate_block_proofs(ctx, blocks_to_validate(ctx, recs), verifier, programs,
                                 network if network is not None else Network.MAIN)


# application/config/network.rs:66-130 and consensus_rule_set.rs:9-14,50-70, per `verifier.Network`:
# (minimum_block_time ms, target_block_interval ms, difficulty_reset_interval ms or 0, genesis difficulty limb 0,
#  first HardforkAlpha height or 0 = always, allows_mock_pow)
_CHAIN_RULES = {"main": (60_000, 588_000, 0, 100_000_000, 15_000, False),
                "testnet": (60_000, 588_000, 0, 100_000, 120, False),
                "testnet-mock": (100, 588_000, 2 * 588_000, 100_000, 0, False),
                "regtest": (1, 100, 0, 6_000, 0, True)}
LINK_OK, LINK_SKIPPED, LINK_BLOCK_HEIGHT, LINK_PREV_BLOCK_DIGEST, LINK_BLOCK_MMR_UPDATE, LINK_MINIMUM_BLOCK_TIME, \
    LINK_DIFFICULTY, LINK_CUMULATIVE_POW, LINK_FUTURE_DATING = range(9)


def chain_params(network, now: int, pow_tree_height: int = POW_TREE_HEIGHT) -> "_lib.ChainParams":
    """The chain-rule parameters of `network` (a `verifier.Network`) and the validator's clock `now`
    (a Timestamp: milliseconds), as `nhip_blk_chain_check` reads them."""
    mn, target, reset, genesis, alpha, mock = _CHAIN_RULES[network.value]
    p = _lib.ChainParams()
    p.minimum_block_time_ms, p.target_block_interval_ms, p.difficulty_reset_interval_ms = mn, target, reset
    p.genesis_difficulty[0] = genesis
    p.hardfork_alpha_height, p.now_ms = alpha, int(now)
    p.pow_tree_height, p.allows_mock_pow = pow_tree_height, 1 if mock else 0
    return p


def difficulty_target(difficulty: Sequence[int]) -> Tuple[int, ...]:
    """`Difficulty::target` (difficulty_control.rs:69-76) of five u32 limbs, as a digest (host only)."""
    d, out = np.array([int(x) for x in difficulty], dtype=np.uint32), np.zeros(5, dtype=np.uint64)
    check(_lib.load().nhip_difficulty_target(d.ctypes.data, out.ctypes.data), "nhip_difficulty_target")
    return tuple(int(x) for x in out)


def difficulty_control(new_timestamp: int, old_timestamp: int, old_difficulty: Sequence[int], target_block_interval: int,
                       previous_block_height: int) -> List[int]:
    """`difficulty_control` (difficulty_control.rs:441-486); times in milliseconds (host only)."""
    d, out = np.array([int(x) for x in old_difficulty], dtype=np.uint32), np.zeros(5, dtype=np.uint32)
    check(_lib.load().nhip_difficulty_control(new_timestamp, old_timestamp, d.ctypes.data, target_block_interval,
                                              previous_block_height, out.ctypes.data), "nhip_difficulty_control")
    return [int(x) for x in out]


def _scanned(records) -> "ctypes.Array":
    """The records as `nhip_blk_block`s: the chain entry points walk each block again from its offset."""
    blocks = (_lib.BlkBlock * max(len(records), 1))()
    for b, r in zip(blocks, records):
        b.offset, b.size = r.offset, r.size
    return blocks


def block_digests(ctx, data, records: Sequence[BlockRecord], pow_tree_height: int = POW_TREE_HEIGHT,
                  with_mast_paths: bool = False):
    """`Block::hash` (block/mod.rs:189-195,317) of every record of `data` in one call (`nhip_blk_digests`):
    an (n, 5) uint64 array; with `with_mast_paths`, also each block's `PowMastPaths` (block/mod.rs:946-962)
    as (pow 3, header 2, kernel 1) digest tuples."""
    a, n = _buf(data)
    m = len(records)
    out = np.zeros((max(m, 1), 5), dtype=np.uint64)
    mast = (_lib.PowMastPaths * max(m, 1))() if with_mast_paths else None
    check(ctx.lib.nhip_blk_digests(ctx.handle, a.ctypes.data, n, pow_tree_height,
                                   ctypes.cast(_scanned(records), ctypes.c_void_p), m, out.ctypes.data,
                                   ctypes.cast(mast, ctypes.c_void_p) if with_mast_paths else None), "nhip_blk_digests")
    if not with_mast_paths:
        return out[:m]
    dig = lambda d: tuple(int(x) for x in d)  # noqa: E731
    return out[:m], [(tuple(dig(d) for d in p.pow), tuple(dig(d) for d in p.header), tuple(dig(d) for d in p.kernel))
                     for p in mast[:m]]


def chain_links(ctx, data, records: Sequence[BlockRecord], network, now: int, parent_of=None,
                pow_tree_height: int = POW_TREE_HEIGHT, params=None) -> List[Tuple[int, bool]]:
    """`Block::validate` rules 0.a-0.g and `Block::has_proof_of_work` (block/mod.rs:726-782,920-942) for every
    (parent, child) pair of `records` in one call (`nhip_blk_chain_check`): `[(status, pow_ok)]` with `status`
    one of `LINK_*`.  `parent_of[i]`: the record that is block i's parent, -1 to skip the pair; by default the
    block before it in the file, and the first block is skipped.  `params`: a `ChainParams` instead of
    `chain_params(network, now)`."""
    a, n = _buf(data)
    m = len(records)
    par = np.arange(-1, m - 1, dtype=np.int64) if parent_of is None else np.asarray(parent_of, dtype=np.int64)
    if par.shape != (m,):
        raise ValueError("parent_of needs one entry per record")
    par = np.ascontiguousarray(par) if m else np.zeros(1, dtype=np.int64)
    p = params if params is not None else chain_params(network, now, pow_tree_height)
    status, pow_ok = np.zeros(max(m, 1), dtype=np.uint8), np.zeros(max(m, 1), dtype=np.uint8)
    check(ctx.lib.nhip_blk_chain_check(ctx.handle, a.ctypes.data, n, ctypes.byref(p),
                                       ctypes.cast(_scanned(records), ctypes.c_void_p), m, par.ctypes.data,
                                       status.ctypes.data, pow_ok.ctypes.data, None), "nhip_blk_chain_check")
    return [(int(s), bool(k)) for s, k in zip(status[:m], pow_ok[:m])]


def inputs_removable(ctx, msa_before, removal_records) -> Tuple[bool, Optional[int]]:
    """`Block::validate` rule 2.b (protocol/consensus/block/mod.rs:816-822): every input of the block
    passes `msa_before.can_remove`, all records in one GPU call.  Returns `(True, None)`, or `False` and
    the position of the first record that fails (the one the reference's loop stops at)."""
    from .mutator_set import can_remove_batch
    for i, (_, can, _) in enumerate(can_remove_batch(ctx, msa_before, removal_records)):
        if not can:
            return False, i
    return True, None


def mutator_set_update_valid(ctx, msa_before, removal_records, addition_records, msa_claimed) -> Tuple[bool, int]:
    """`Block::validate` rules 2.b-2.e (protocol/consensus/block/mod.rs:816-849) in the reference's order,
    one GPU call: every input removable, the removal records distinct, the update applicable, and the
    accumulator after it equal to `msa_claimed` (the one the block commits to).  Returns `(ok, status)`
    with `status` one of `neptune_hip.mutator_set`'s."""
    from .mutator_set import MutatorSetUpdate, apply_update_batch
    update = MutatorSetUpdate(list(removal_records), list(addition_records))
    verdict, status, _, _ = apply_update_batch(ctx, [(msa_before, update)], [msa_claimed])[0]
    return verdict, status


def mutator_set_update_valid_packed(ctx, msa_before, packed_inputs, addition_records, msa_claimed) -> Tuple[bool, int]:
    """`Block::validate` rules 2.a-2.e (mod.rs:811-849) in one GPU call: `packed_inputs` is the block body's
    `transaction_kernel.inputs` as the block carries them (`RemovalRecordList::pack`); they are unpacked on the
    device (2.a) into the buffers `mutator_set_update_valid`'s kernels read.  Returns `(ok, status)`; a list that
    does not unpack gives `(False, UNPACK_*)`."""
    from .mutator_set import MutatorSetUpdate, apply_update_batch_packed
    update = MutatorSetUpdate(list(packed_inputs), list(addition_records))
    verdict, status, _, _ = apply_update_batch_packed(ctx, [(msa_before, update)], [msa_claimed])[0]
    return verdict, status


def accumulator_after(ctx, msa, guesser_fee_addition_records):
    """`Block::mutator_set_accumulator_after` (mod.rs:369-378): `msa` with the guesser-fee addition records
    applied, an update with additions only.  Raises when `msa` is inconsistent."""
    from .mutator_set import MutatorSetUpdate, apply_update_batch
    verdict, status, _, after = apply_update_batch(ctx, [(msa, MutatorSetUpdate((), list(guesser_fee_addition_records)))])[0]
    if not verdict:
        raise ValueError(f"mutator set accumulator rejected: status {status}")
    return after


# ---------------------------------------------------------------- mutator-set and transaction rules
BLKMS_OK, BLKMS_SKIPPED, BLKMS_UNPACK, BLKMS_PARENT_NEGATIVE_FEE, BLKMS_PARENT_MSA_INCONSISTENT, \
    BLKMS_REMOVAL_RECORDS_VALIDITY, BLKMS_REMOVAL_RECORDS_UNIQUENESS, BLKMS_UPDATE_IMPOSSIBLE, BLKMS_UPDATE_INTEGRITY, \
    BLKMS_TRANSACTION_TIMESTAMP, BLKMS_COINBASE_TOO_BIG, BLKMS_NEGATIVE_COINBASE, BLKMS_NEGATIVE_FEE, \
    BLKMS_TOO_MANY_INPUTS, BLKMS_TOO_MANY_OUTPUTS, BLKMS_TOO_MANY_ANNOUNCEMENTS = range(16)
# the rule each status stands for, as `validate_chain_file` names it
BLKMS_RULES = (None, None, "2.a", "2.b parent fee", "2.b parent accumulator", "2.b", "2.c", "2.d", "2.e", "2.f", "2.g",
               "2.h", "2.i", "2.j", "2.k", "2.l")
LINK_RULES = (None, None, "0.a", "0.b", "0.c", "0.d", "0.e", "0.f", "0.g")
GUESSER_OK, GUESSER_NEGATIVE_FEE = 0, 1


def ms_params(type_scripts, pow_tree_height: int = POW_TREE_HEIGHT, max_num: Optional[int] = None) -> "_lib.BlkMsParams":
    """`nhip_blk_ms_params`.  `type_scripts`: `(NativeCurrency.hash(), TimeLock.hash())`, two digests that come from
    tasm-lib code generation (as `verifier.ConsensusPrograms`), or a ready `BlkMsParams`, returned as it is.
    `max_num`: one value for the three limits of rules 2.j-2.l instead of 1 << 14."""
    if isinstance(type_scripts, _lib.BlkMsParams):
        return type_scripts
    native_currency, time_lock = type_scripts
    p = _lib.BlkMsParams()
    _lib.load().nhip_blk_ms_params_default(ctypes.byref(p))
    for q in range(5):
        p.native_currency_hash[q], p.time_lock_hash[q] = int(native_currency[q]), int(time_lock[q])
    p.pow_tree_height = pow_tree_height
    if max_num is not None:
        p.max_num_inputs = p.max_num_outputs = p.max_num_announcements = int(max_num)
    return p


_PARTS_DTYPES = dict(coinbase_tag=np.uint8, aocl_n_peaks=np.uint32, swbf_n_peaks=np.uint32, active=np.uint32,
                     distances=np.uint32, rel=np.uint32)


def mutator_set_parts(data, records: Sequence[BlockRecord], pow_tree_height: int = POW_TREE_HEIGHT) -> dict:
    """The host walk `nhip_blk_ms_walk` (no GPU, hashes nothing): what rules 2.a-2.l and the guesser-fee records read
    of every record of `data`, as numpy arrays named and shaped as `nhip_blk_ms_parts` says.  The inputs are the
    packed list as it lies in the file (an entry's key in `chunk_index`)."""
    lib = _lib.load()
    a, n = _buf(data)
    m = len(records)
    blocks = ctypes.cast(_scanned(records), ctypes.c_void_p)
    out = _lib.BlkMsParts()
    rc = lib.nhip_blk_ms_walk(a.ctypes.data, n, pow_tree_height, blocks, m, ctypes.byref(out))
    if rc == NHIP_ERR_DECODE:
        raise BlockFileError("malformed block", 0)
    check(rc, "nhip_blk_ms_walk")
    A, O, R, E, PD, W = (int(getattr(out, f)) for f in _lib.BlkMsParts.TOTALS)
    shapes = dict(height=(m,), timestamp=(m,), receiver_digest=(m, 5), lock_script_hash=(m, 5), fee=(m, 2),
                  coinbase=(m, 2), coinbase_tag=(m,), kernel_timestamp=(m,), n_announcements=(m,), aocl_num_leafs=(m,),
                  swbf_num_leafs=(m,), aocl_n_peaks=(m,), swbf_n_peaks=(m,), aocl_peaks=(m, 64, 5), swbf_peaks=(m, 64, 5),
                  active_off=(m + 1,), active=(A,), out_off=(m + 1,), outputs=(O, 5), rec_off=(m + 1,), minimum=(R, 2),
                  distances=(R, 45), entry_off=(R + 1,), chunk_index=(E,), path_off=(E + 1,), path=(PD, 5),
                  rel_off=(E + 1,), rel=(W,))
    arrays = {f: np.zeros(shapes[f], dtype=_PARTS_DTYPES.get(f, np.uint64)) for f in _lib.BlkMsParts.ARRAYS}
    # a zero-size array still gets an address: only the count pass has null array pointers
    pad = {f: (v if v.size else np.zeros(1, dtype=v.dtype)) for f, v in arrays.items()}
    out = _lib.BlkMsParts(*(pad[f].ctypes.data for f in _lib.BlkMsParts.ARRAYS), A, O, R, E, PD, W)
    check(lib.nhip_blk_ms_walk(a.ctypes.data, n, pow_tree_height, blocks, m, ctypes.byref(out)), "nhip_blk_ms_walk")
    return arrays


def _digest_arg(digests, m):
    if digests is None:
        return None, None
    d = np.ascontiguousarray(np.asarray(digests, dtype=np.uint64)).reshape(-1, 5)
    if d.shape[0] != m:
        raise ValueError("digests needs one digest per record")
    return d, (d.ctypes.data if m else None)


def guesser_fee_addition_records(ctx, data, records: Sequence[BlockRecord], type_scripts, digests=None,
                                 pow_tree_height: int = POW_TREE_HEIGHT):
    """`BlockKernel::guesser_fee_addition_records` (block_kernel.rs:47-93) of every record of `data` in one call
    (`nhip_blk_guesser_fee_records`): per block `(status, [locked, unlocked])` with `status` one of `GUESSER_*` and the
    list empty for a block at height 0 or with a negative fee.  `digests`: the blocks' `Block::hash` as
    `block_digests` or `nhip_blk_chain_check` gave them; by default they are computed here."""
    a, n = _buf(data)
    m = len(records)
    p = ms_params(type_scripts, pow_tree_height)
    _keep, dptr = _digest_arg(digests, m)
    rec = np.zeros((max(m, 1), 2, 5), dtype=np.uint64)
    nrec, status = np.zeros(max(m, 1), dtype=np.uint8), np.zeros(max(m, 1), dtype=np.uint8)
    check(ctx.lib.nhip_blk_guesser_fee_records(ctx.handle, a.ctypes.data, n, ctypes.byref(p),
                                               ctypes.cast(_scanned(records), ctypes.c_void_p), m, dptr, rec.ctypes.data,
                                               nrec.ctypes.data, status.ctypes.data), "nhip_blk_guesser_fee_records")
    return [(int(status[i]), [tuple(int(x) for x in rec[i, k]) for k in range(int(nrec[i]))]) for i in range(m)]


def mutator_set_links(ctx, data, records: Sequence[BlockRecord], type_scripts, parent_of=None, digests=None,
                      pow_tree_height: int = POW_TREE_HEIGHT) -> List[Tuple[int, int, Optional[int]]]:
    """`Block::validate` rules 2.a-2.l (block/mod.rs:811-891) for every (parent, child) pair of `records` in one call
    (`nhip_blk_ms_check`): `[(status, ms_status, bad_record)]` with `status` one of `BLKMS_*`, `ms_status` the
    `neptune_hip.mutator_set` status behind rules 2.a-2.e and `bad_record` the input it blames (None: none).
    `parent_of` and `digests` as in `chain_links` and `guesser_fee_addition_records`."""
    a, n = _buf(data)
    m = len(records)
    par = np.arange(-1, m - 1, dtype=np.int64) if parent_of is None else np.asarray(parent_of, dtype=np.int64)
    if par.shape != (m,):
        raise ValueError("parent_of needs one entry per record")
    par = np.ascontiguousarray(par) if m else np.zeros(1, dtype=np.int64)
    p = ms_params(type_scripts, pow_tree_height)
    _keep, dptr = _digest_arg(digests, m)
    status, ms_status = np.zeros(max(m, 1), dtype=np.uint8), np.zeros(max(m, 1), dtype=np.uint8)
    bad = np.zeros(max(m, 1), dtype=np.uint64)
    check(ctx.lib.nhip_blk_ms_check(ctx.handle, a.ctypes.data, n, ctypes.byref(p),
                                    ctypes.cast(_scanned(records), ctypes.c_void_p), m, par.ctypes.data, dptr,
                                    status.ctypes.data, ms_status.ctypes.data, bad.ctypes.data), "nhip_blk_ms_check")
    return [(int(status[i]), int(ms_status[i]), None if int(bad[i]) == 2 ** 64 - 1 else int(bad[i])) for i in range(m)]


def validate_chain_file(ctx, path: str, verifier, programs, type_scripts, now: int, network=None,
                        pow_tree_height: int = POW_TREE_HEIGHT) -> List[Optional[str]]:
    """`Block::validate` over one blk file, every block against the block before it (the first block's pair is
    skipped: only its rules 1.a-1.d are checked): `chain_links`, `validate_block_proofs` and `mutator_set_links`, each
    one pass over the file.  Per block the first failing rule in the reference's order (0.x, the proof of work, 1.x,
    2.x), as a string, or None.  Rule 1.e (the block's size) is not covered."""
    from .verifier import Network, validate_block_proofs
    network = network if network is not None else Network.MAIN
    if os.path.getsize(path) == 0:
        return []
    with open(path, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as m:
        recs = blocks_from_bytes(m, pow_tree_height)
        links = chain_links(ctx, m, recs, network, now, pow_tree_height=pow_tree_height)
        proofs = validate_block_proofs(ctx, blocks_to_validate(ctx, recs), verifier, programs, network)
        ms = mutator_set_links(ctx, m, recs, type_scripts, pow_tree_height=pow_tree_height)
    out: List[Optional[str]] = []
    for (link, pow_ok), proof, (st, _, _) in zip(links, proofs, ms):
        if LINK_RULES[link] is not None:
            out.append(LINK_RULES[link])
        elif link != LINK_SKIPPED and not pow_ok:
            out.append("proof of work")
        elif proof is not None:
            out.append(proof)
        else:
            out.append(BLKMS_RULES[st])
    return out


@dataclass
class TransferTransaction:
    """transfer_transaction.rs:31-47: `kernel_sequences` (the kernel's 8 MAST sequences) and the
    proof as a `verifier.TransactionProof`."""
    kernel_sequences: List[np.ndarray]
    proof: object
    size: int

    @staticmethod
    def from_bytes(data, arena=None) -> "TransferTransaction":
        """`arena`: the member proofs decoded straight into it (pinned, nhip_arena_ingest_spans)."""
        from .verifier import PROOF_COLLECTION, SINGLE_PROOF, ProofCollection, TransactionProof
        lib = _lib.load()
        a, n = _buf(data)
        t = _lib.Tx()
        rc = lib.nhip_tx_scan(a.ctypes.data, n, ctypes.byref(t))
        if rc == NHIP_ERR_DECODE:
            raise ValueError("malformed TransferTransaction")
        check(rc, "nhip_tx_scan")
        seq = np.zeros(max(int(t.seq_words), 1), dtype=np.uint64)
        offs = np.zeros(9, dtype=np.uint64)
        spans = np.zeros(2 * t.n_proofs, dtype=np.uint64)
        dig = np.zeros(max(5 * t.n_digests, 1), dtype=np.uint64)
        check(lib.nhip_tx_parts(a.ctypes.data, n, ctypes.byref(t), seq.ctypes.data, offs.ctypes.data,
                                spans.ctypes.data, dig.ctypes.data), "nhip_tx_parts")
        seqs = [seq[int(offs[j]):int(offs[j + 1])] for j in range(8)]
        if arena is not None:
            pl = arena.ingest_spans(a[:n], [(int(spans[2 * i]), int(spans[2 * i + 1])) for i in range(t.n_proofs)])
            proofs = [pl.words(i) for i in range(t.n_proofs)]
        else:
            proofs = [_words(lib, a, n, int(spans[2 * i]), int(spans[2 * i + 1])) for i in range(t.n_proofs)]
        if t.kind == 1:
            return TransferTransaction(seqs, TransactionProof(SINGLE_PROOF, proofs[0]), int(t.size))
        d = [tuple(int(x) for x in dig[5 * i:5 * i + 5]) for i in range(t.n_digests)]
        nl, nt = int(t.n_lock_scripts), int(t.n_type_scripts)
        lh, th = int(t.n_lock_hashes), int(t.n_type_hashes)
        pc = ProofCollection(
            removal_records_integrity=proofs[0], collect_lock_scripts=proofs[1],
            lock_scripts_halt=proofs[2:2 + nl], kernel_to_outputs=proofs[2 + nl],
            collect_type_scripts=proofs[3 + nl], type_scripts_halt=proofs[4 + nl:4 + nl + nt],
            lock_script_hashes=d[:lh], type_script_hashes=d[lh:lh + th], kernel_mast_hash=d[lh + th],
            salted_inputs_hash=d[lh + th + 1], salted_outputs_hash=d[lh + th + 2],
            merge_bit_mast_path=d[lh + th + 3:])
        return TransferTransaction(seqs, TransactionProof(PROOF_COLLECTION, pc), int(t.size))
