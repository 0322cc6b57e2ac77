"""CPU restatement of the link from a parent block to its child's mutator-set and transaction rules in Python
integers — TEST HELPER ONLY (not collected).

Over ms_ref.Archival, ms_apply_ref, ms_pack_ref.pack / try_unpack, bincode_ref (block dicts, BFieldCodec helpers) and
block_chain_ref.block_hash.  Paths relative to neptune-core/src/protocol/consensus/ unless a directory is given:

  * encode_coin / encode_utxo        transaction/utxo.rs:29-32,71-74 under the derive rules bincode_ref states (fields
                                     last-first, dynamic fields length-prefixed) — unpinned
  * guesser_fee_utxos                block/block_kernel.rs:47-67 (total_guesser_reward block/block_body.rs:160-169,
                                     Timestamp::years proof_abstractions/timestamp.rs:126-128, TimeLock::until
                                     type_scripts/time_lock.rs:39-44)
  * guesser_fee_addition_records     block/block_kernel.rs:73-93 with commit, util_types/mutator_set.rs:49-54
  * mutator_set_accumulator_after    block/mod.rs:369-378 (ms_apply_ref.msa_add per record)
  * block_subsidy                    block/mod.rs:393-408, block/block_height.rs:46-47,60-65
  * tx_rule                          block/mod.rs:851-891 (2.f-2.l)
  * pair_outcome                     block/mod.rs:811-891 (2.a-2.l) in nhip_blk_ms_check's statuses
`Chain` builds real chains for the tests: every block's inputs spend earlier outputs of an archival mutator set,
packed, and its body's accumulator is the true one.  A guesser-fee record enters the archival set as the item
(Tip5::hash(utxo), block hash, receiver preimage) with the header's receiver_digest = hash_pair(preimage, 0), so
that its AOCL leaf is the record.
"""
from __future__ import annotations

import copy
import random
from typing import List, Optional, Sequence, Tuple

import bincode_ref as B
import block_chain_ref as C
import ms_apply_ref as A
import ms_pack_ref as K
import ms_ref as R

P = B.P
YEARS_3 = 94_670_208_000                       # Timestamp::years(3), in ms
BLOCKS_PER_GENERATION, NUM_BLOCKS_SKIPPED_BECAUSE_REBOOT = 160815, 21310
INITIAL_BLOCK_SUBSIDY = 128 * 4 * 10 ** 30     # 128 coins in nau
MAX_NUM = 1 << 14                              # MAX_NUM_INPUTS_OUTPUTS_ANNOUNCEMENTS
OK, SKIPPED, UNPACK, PARENT_NEGATIVE_FEE, PARENT_MSA_INCONSISTENT, REMOVAL_RECORDS_VALIDITY, \
    REMOVAL_RECORDS_UNIQUENESS, UPDATE_IMPOSSIBLE, UPDATE_INTEGRITY, TRANSACTION_TIMESTAMP, COINBASE_TOO_BIG, \
    NEGATIVE_COINBASE, NEGATIVE_FEE, TOO_MANY_INPUTS, TOO_MANY_OUTPUTS, TOO_MANY_ANNOUNCEMENTS = range(16)
GUESSER_OK, GUESSER_NEGATIVE_FEE = 0, 1


class NegativeFee(Exception):
    """BlockValidationError::NegativeFee out of total_guesser_reward."""


# ------------------------------------------------------------------ encodings
def encode_coin(coin) -> List[int]:
    """Coin {type_script_hash, state}: state (dynamic) first, then the digest."""
    type_script_hash, state = coin
    return B._dyn(B._vec_static(state, lambda x: [x])) + [int(x) for x in type_script_hash]


def encode_utxo(utxo) -> List[int]:
    """Utxo {lock_script_hash, coins}: coins (dynamic, dynamic items) first, then the digest."""
    return B._dyn(B._vec_dyn(utxo["coins"], encode_coin)) + [int(x) for x in utxo["lock_script_hash"]]


def guesser_fee_utxos(block, type_scripts) -> List[dict]:
    native_currency, time_lock = type_scripts
    h = block["header"]
    if h["height"] % P == 0:
        return []
    fee = block["body"]["transaction_kernel"]["fee"]
    if fee < 0:
        raise NegativeFee()
    timelocked = fee // 2          # i128 / 2 of a non-negative amount
    unlocked = fee - timelocked
    date = (h["timestamp"] % P + YEARS_3) % P
    coin = lambda amount: (native_currency, B._u128(amount))  # noqa: E731
    return [{"lock_script_hash": h["lock_script_hash"], "coins": [coin(timelocked), (time_lock, [date])]},
            {"lock_script_hash": h["lock_script_hash"], "coins": [coin(unlocked)]}]


def guesser_fee_addition_records(block, block_hash, type_scripts) -> List[Tuple[int, ...]]:
    rd = block["header"]["receiver_digest"]
    return [R._hp(R._hp(R.hash_varlen(encode_utxo(u)), block_hash), rd) for u in guesser_fee_utxos(block, type_scripts)]


def body_msa(block) -> R.Msa:
    b = block["body"]
    mmr = lambda m: R.Mmr([tuple(int(x) for x in d) for d in m["peaks"]], m["leaf_count"])  # noqa: E731
    return R.Msa(mmr(b["aocl"]), mmr(b["swbf_inactive"]), [int(x) for x in b["swbf_active"]])


def mutator_set_accumulator_after(block, block_hash, type_scripts) -> R.Msa:
    msa = body_msa(block)
    for rec in guesser_fee_addition_records(block, block_hash, type_scripts):
        msa = A.msa_add(msa, rec)
    return msa


# ------------------------------------------------------------------ rules 2.f-2.l
def block_subsidy(height: int) -> int:
    reward = INITIAL_BLOCK_SUBSIDY
    generation = min(height + NUM_BLOCKS_SKIPPED_BECAUSE_REBOOT, (1 << 64) - 1) // BLOCKS_PER_GENERATION
    for _ in range(generation):
        reward //= 2
        if reward == 0:
            return 0
    return reward


def tx_rule(block, n_inputs: int, max_num=(MAX_NUM, MAX_NUM, MAX_NUM)) -> int:
    h, k = block["header"], block["body"]["transaction_kernel"]
    if k["timestamp"] % P > h["timestamp"] % P:
        return TRANSACTION_TIMESTAMP
    if k["coinbase"] is not None:
        if k["coinbase"] > block_subsidy(h["height"] % P):
            return COINBASE_TOO_BIG
        if k["coinbase"] < 0:
            return NEGATIVE_COINBASE
    if k["fee"] < 0:
        return NEGATIVE_FEE
    if n_inputs > max_num[0]:
        return TOO_MANY_INPUTS
    if len(k["outputs"]) > max_num[1]:
        return TOO_MANY_OUTPUTS
    if len(k["announcements"]) > max_num[2]:
        return TOO_MANY_ANNOUNCEMENTS
    return OK


# ------------------------------------------------------------------ rules 2.a-2.l
def to_records(inputs) -> List[R.Record]:
    """bincode_ref removal-record dicts -> ms_ref.Records (the packed list as the block carries it)."""
    return [R.Record(R.IndexSet(rr["minimum"], list(rr["distances"])),
                     [(k, [tuple(d) for d in p], R.Chunk(list(rel))) for k, p, rel in rr["chunks"]]) for rr in inputs]


def from_records(records) -> List[dict]:
    return [{"minimum": r.absolute_indices.minimum, "distances": list(r.absolute_indices.distances),
             "chunks": [(k, [tuple(d) for d in p], list(c.relative_indices)) for k, p, c in r.target_chunks]}
            for r in records]


def pair_outcome(parent, child, parent_hash, type_scripts, arch_before: R.Archival, triples,
                 max_num=(MAX_NUM, MAX_NUM, MAX_NUM)):
    """(status, ms_status, bad_record) of one (parent, child) pair, both decoded block dicts.  `arch_before`: the
    archival set behind the parent's accumulator after (left unchanged); `triples`: {canonical commitment: (item,
    sender_randomness, receiver_preimage)} for the child's outputs."""
    status, records = K.try_unpack_status(to_records(child["body"]["transaction_kernel"]["inputs"]))
    if status:
        return UNPACK, status, None
    try:
        guesser = guesser_fee_addition_records(parent, parent_hash, type_scripts)
    except NegativeFee:
        return PARENT_NEGATIVE_FEE, R.OK, None
    outputs = [tuple(int(x) for x in d) for d in child["body"]["transaction_kernel"]["outputs"]]
    if not A.consistent(body_msa(parent), len(guesser)):
        return PARENT_MSA_INCONSISTENT, A.INCONSISTENT, None
    msa_before = mutator_set_accumulator_after(parent, parent_hash, type_scripts)
    if not A.consistent(msa_before, len(outputs)):
        return PARENT_MSA_INCONSISTENT, A.INCONSISTENT, None
    _, st, bad, _ = A.outcome(arch_before, msa_before, [triples[d] for d in outputs], records, body_msa(child))
    if st == A.DUPLICATE_RECORD:
        return REMOVAL_RECORDS_UNIQUENESS, st, bad
    if st == A.UPDATE_IMPOSSIBLE:
        return UPDATE_IMPOSSIBLE, st, bad
    if st == A.UPDATE_MISMATCH:
        return UPDATE_INTEGRITY, st, None
    if st != R.OK:
        return REMOVAL_RECORDS_VALIDITY, st, bad
    return tx_rule(child, len(records), max_num), R.OK, None


# ------------------------------------------------------------------ a real chain
def _digest(g) -> Tuple[int, ...]:
    return tuple(g.randrange(P) for _ in range(5))


class Chain:
    """Blocks on one archival mutator set.  blocks[i] (dict), enc[i] (bytes), hashes[i], arch_after[i] (the archival
    set behind block i's accumulator after, guesser records included), triples (for pair_outcome)."""

    def __init__(self, type_scripts, seed=2900, tree_height=10, proof_words=12):
        self.ts, self.g, self.h, self.proof_words = type_scripts, random.Random(seed), tree_height, proof_words
        self.arch = R.Archival()
        self.blocks, self.enc, self.hashes, self.arch_after, self.triples = [], [], [], [], {}
        self.arch_body = []  # the archival set behind each block's body accumulator (before its guesser records)
        self.spent, self.spends = set(), []  # spent leaves, and block by block

    def new_outputs(self, n):
        out = []
        for _ in range(n):
            t = (_digest(self.g), _digest(self.g), _digest(self.g))
            self.triples[A.commitment(*t)] = t
            out.append(t)
        return out

    def add(self, n_outputs=2, spend: Sequence[int] = (), fee=0, coinbase=None, timestamp=None, height=None,
            records=None, edit=None, keep=True):
        """One more block on the tip.  `spend`: AOCL leaf indices whose removal records (against the tip's accumulator
        after) are its inputs; `records`: the unpacked records instead.  `edit(block)`: a change made before the block
        is encoded and hashed (its body's accumulator stays the true one of the unedited update).  keep=False: the
        block is returned as (block, bytes, hash) and the chain is left as it was."""
        g = self.g
        arch = A.clone(self.arch)
        recs = [arch.removal_record(l) for l in spend] if records is None else copy.deepcopy(list(records))
        outs = self.new_outputs(n_outputs)
        kernel = B.random_kernel(g, 0, 0, 0)
        kernel["inputs"] = from_records(K.pack(recs)) if recs else []
        kernel["outputs"] = [A.commitment(*t) for t in outs]
        kernel["fee"], kernel["coinbase"] = fee, coinbase
        b = B.random_block(g, [], B.SINGLE_PROOF, [g.randrange(P) for _ in range(self.proof_words)], self.h, kernel)
        hd = b["header"]
        hd["height"] = len(self.blocks) if height is None else height
        hd["timestamp"] = (1_700_000_000_000 + 600_000 * len(self.blocks)) if timestamp is None else timestamp
        kernel["timestamp"] = hd["timestamp"] % P
        rp = _digest(g)
        hd["receiver_digest"] = R._hp(rp, (0,) * 5)
        A.apply(arch, outs, copy.deepcopy(recs))
        msa = arch.msa()
        body = A.clone(arch)
        mm = lambda m: {"leaf_count": m.num_leafs, "peaks": [tuple(d) for d in m.peaks]}  # noqa: E731
        b["body"].update(aocl=mm(msa.aocl), swbf_inactive=mm(msa.swbf_inactive), swbf_active=list(msa.swbf_active))
        if edit is not None:
            edit(b)
        enc = B.encode_block(b)
        b = B.r_block(B.R(enc), self.h)  # as a decoder sees it
        bh = C.block_hash(b)
        try:
            for u in guesser_fee_utxos(b, self.ts):
                arch.add(R.hash_varlen(encode_utxo(u)), bh, rp)
        except NegativeFee:
            pass
        if keep:
            self.arch = arch
            self.blocks.append(b)
            self.enc.append(enc)
            self.hashes.append(bh)
            self.arch_after.append(A.clone(arch))
            self.arch_body.append(body)
            self.spent.update(spend)
            self.spends.append(list(spend))
        return b, enc, bh

    def fork(self, upto: int, seed: int) -> "Chain":
        """A chain of its own that shares blocks[:upto] (and the triples) with this one."""
        f = Chain(self.ts, seed, self.h, self.proof_words)
        for k in ("blocks", "enc", "hashes", "arch_after", "arch_body", "spends"):
            setattr(f, k, list(getattr(self, k)[:upto]))
        f.arch = A.clone(self.arch_after[upto - 1])
        f.spent = {l for sp in f.spends for l in sp}
        f.triples = self.triples
        return f

    @property
    def num_leafs(self) -> int:
        return len(self.arch.items)

    def unspent(self, k, touching_chunk: Optional[int] = None) -> List[int]:
        """k unspent leaves, lowest first; with touching_chunk, leaves whose index set has an index in that chunk."""
        out = []
        for l in range(self.num_leafs):
            if l in self.spent:
                continue
            if touching_chunk is not None and \
                    all(i // R.CHUNK_SIZE != touching_chunk for i in self.arch.index_set(l).to_array()):
                continue
            out.append(l)
            if len(out) == k:
                break
        assert len(out) == k, "not enough unspent leaves"
        return out
