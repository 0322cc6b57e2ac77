"""CPU restatement of `Block::hash`, the PoW MAST paths, `Block::validate` rules 0.a-0.g and
`Block::has_proof_of_work` in Python integers — TEST HELPER ONLY (not collected).

Over the oracle modules bincode_ref (block dicts and BFieldCodec helpers), mast_ref (MastHash::mast_hash),
pow_ref (Pow::validate, fast_mast_hash, digest order) and tip5_ref.  Paths relative to
neptune-core/src/protocol/consensus/block/ unless a directory is given:

  * header_sequences      block_header.rs:204-215, the eight field encodings; pow.encode() = nonce ++ path_b ++
                          path_a ++ root (pow.rs:196-197), guesser_receiver_data last-first
                          (guesser_receiver_data.rs:15-18)
  * kernel_sequences      block_kernel.rs:112-119: header hash, body hash, appendix.encode()
  * block_sequences       mod.rs:192-194: kernel hash, proof.encode()
  * body_mast_hash        block_body.rs:175-182 (sequence 1 = the transaction kernel's MAST hash)
  * appendix_encoding     block_appendix.rs:31-33 with Claim as neptune-core/src/tasm/claims/new_claim.rs:38-100 pins it
  * proof_encoding        mod.rs:114-119, the derived enum (bfieldcodec_derive: [variant] + fields, a dynamic
                          field length-prefixed; Proof(Vec<BFieldElement>) = [n + 1, n, items]) — unpinned
  * mast_path             proof_abstractions/mast_hash.rs:41-45: the authentication structure of one leaf,
                          siblings from the leaf up
  * pow_mast_paths        mod.rs:946-962
  * block_hash            mod.rs:317 / 189-195
  * difficulty_new / difficulty_target / safe_mul_fixed_point_rational / pow_add / difficulty_control
                          difficulty_control.rs:51-65, 69-76, 82-109, 258-283, 441-486
  * should_reset_difficulty  mod.rs:903-913
  * link_status           mod.rs:726-782 (0.a-0.g in order)
  * has_proof_of_work     mod.rs:920-942, is_valid_mock_pow :994-996, pow_verify :1013-1024
Timestamps and heights are Goldilocks elements (timestamp.rs:61-91, block_height.rs:67-69): + and - are field
operations, comparisons are on canonical values.  Where the reference panics (a zero difficulty in `target`,
a zero interval) these raise `ReferencePanics`.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import bincode_ref as B
import mast_ref as M
import pow_ref as PW
import tip5_ref as T

P = B.P
DIFFICULTY_MINIMUM = [6000, 0, 0, 0, 0]          # difficulty_control.rs:47
DIFFICULTY_MAXIMUM = [0xFFFFFFFF] * 5
FUTUREDATING_LIMIT = 5 * 60 * 1000              # mod.rs:106
OK, SKIPPED, BLOCK_HEIGHT, PREV_BLOCK_DIGEST, BLOCK_MMR_UPDATE, MINIMUM_BLOCK_TIME, DIFFICULTY, CUMULATIVE_POW, \
    FUTURE_DATING = range(9)                     # block_validation_error.rs:12-31, after OK and SKIPPED


class ReferencePanics(Exception):
    """The reference panics on this input."""


@dataclass
class Params:
    """application/config/network.rs:66-130 and consensus_rule_set.rs:50-70, and the validator's clock."""
    minimum_block_time: int = 1
    target_block_interval: int = 100
    difficulty_reset_interval: Optional[int] = None
    genesis_difficulty: List[int] = field(default_factory=lambda: list(DIFFICULTY_MINIMUM))
    hardfork_alpha_height: int = 0               # first height under HardforkAlpha; 0: always
    now: int = 0
    tree_height: int = 10
    allows_mock_pow: bool = False


# ------------------------------------------------------------------ encodings and MASTs
def hv(words) -> Tuple[int, ...]:
    return tuple(int(x) for x in T.hash_varlen([int(w) for w in words]))


def header_sequences(h) -> List[List[int]]:
    return [[h["version"] % P], [h["height"] % P], [int(x) for x in h["prev_block_digest"]], [h["timestamp"] % P],
            PW.encode_pow(h["pow_root"], h["path_a"], h["path_b"], h["nonce"]),
            list(h["cumulative_proof_of_work"]), list(h["difficulty"]),
            [int(x) for x in h["lock_script_hash"]] + [int(x) for x in h["receiver_digest"]]]


def encode_claim(c) -> List[int]:
    out, inp = [int(x) % P for x in c["output"]], [int(x) % P for x in c["input"]]
    return [len(out) + 1, len(out)] + out + [len(inp) + 1, len(inp)] + inp + [c["version"]] + \
        [int(x) for x in c["program_digest"]]


def appendix_encoding(claims) -> List[int]:
    vec = [len(claims)] + [w for c in claims for w in B._dyn(encode_claim(c))]
    return B._dyn(vec)


def proof_prefix(kind: int, n: int) -> List[int]:
    return [kind, n + 2, n + 1, n] if kind == B.SINGLE_PROOF else [kind]


def proof_encoding(kind: int, proof) -> List[int]:
    if kind != B.SINGLE_PROOF:
        return [kind]
    return proof_prefix(kind, len(proof)) + [int(x) % P for x in proof]


def mast_levels(sequences) -> List[List[Tuple[int, ...]]]:
    """mast_hash.rs:22-39: the Merkle tree over hash_varlen(sequence), padded with Digest::default()."""
    level = [hv(s) for s in sequences]
    while len(level) & (len(level) - 1):
        level.append((0,) * 5)
    levels = [level]
    while len(level) > 1:
        level = [tuple(int(x) for x in T.hash_pair(list(level[2 * i]), list(level[2 * i + 1])))
                 for i in range(len(level) // 2)]
        levels.append(level)
    return levels


def mast_path(sequences, index: int) -> List[Tuple[int, ...]]:
    out = []
    for level in mast_levels(sequences)[:-1]:
        out.append(level[index ^ 1])
        index >>= 1
    return out


def mast_verify(root, index: int, path, sequence) -> bool:
    """The check `MastHash::mast_path`'s users make: climb from hash_varlen(sequence) to the root."""
    run = hv(sequence)
    for sib in path:
        run = PW.hp(sib, run) if index & 1 else PW.hp(run, sib)
        index >>= 1
    return tuple(run) == tuple(root)


def body_mast_hash(body) -> Tuple[int, ...]:
    txk = M.mast_hash(B.kernel_mast_sequences(body["transaction_kernel"]))
    return M.mast_hash([list(txk)] + B.body_tail_sequences(body))


def kernel_sequences(b) -> List[List[int]]:
    return [list(M.mast_hash(header_sequences(b["header"]))), list(body_mast_hash(b["body"])),
            appendix_encoding(b["appendix"])]


def block_sequences(b) -> List[List[int]]:
    return [list(M.mast_hash(kernel_sequences(b))), proof_encoding(b["proof_kind"], b["proof"])]


def block_hash(b) -> Tuple[int, ...]:
    return M.mast_hash(block_sequences(b))


def pow_mast_paths(b):
    """(pow [3], header [2], kernel [1]): BlockHeaderField::Pow = 4, BlockKernelField::Header = 0,
    BlockField::Kernel = 0 (the fields' positions in the mast_sequences above)."""
    return (mast_path(header_sequences(b["header"]), 4), mast_path(kernel_sequences(b), 0),
            mast_path(block_sequences(b), 0))


# ------------------------------------------------------------------ consensus integers
def gl_add(a: int, b: int) -> int: return (a + b) % P
def gl_sub(a: int, b: int) -> int: return (a - b) % P


def difficulty_new(d: Sequence[int]) -> List[int]:
    return list(DIFFICULTY_MINIMUM) if all(x <= m for x, m in zip(d, DIFFICULTY_MINIMUM)) else list(d)


def _big(limbs) -> int:
    return sum(int(x) << (32 * i) for i, x in enumerate(limbs))


def difficulty_target(d: Sequence[int]) -> Tuple[int, ...]:
    den = _big(d)
    if den == 0:
        raise ReferencePanics("division by zero")
    t = (P ** 5 - 1) // den          # Digest([BFieldElement::MAX; 5]) as a BigUint, element 0 the lowest digit
    return tuple((t // P ** i) % P for i in range(5))


def safe_mul_fixed_point_rational(d: Sequence[int], lo: int, hi: int) -> Tuple[List[int], int]:
    M32 = 0xFFFFFFFF
    new, carry = [0] * 6, 0
    for i in range(5):
        s = carry + d[i] * lo
        new[i], carry = s & M32, s >> 32
    new[5], carry = carry, 0
    for i in range(5):
        s = carry + d[i] * hi
        digit = new[i + 1] + (s & M32)
        new[i + 1], carry = digit & M32, (s >> 32) + (digit >> 32)
    return difficulty_new(new[1:]), carry


def _i64(v: int) -> int:
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def difficulty_control(new_ts: int, old_ts: int, old_difficulty: Sequence[int], target_block_interval: int,
                       previous_block_height: int) -> List[int]:
    if previous_block_height == 0:
        return list(old_difficulty)
    if target_block_interval == 0:
        raise ReferencePanics("division by zero")
    delta_t = gl_sub(new_ts, old_ts)
    absolute_error = _i64(_i64(delta_t) - _i64(target_block_interval))   # a release build wraps
    relative_error = absolute_error * ((1 << 32) // target_block_interval)
    clamped = max(-1 << 32, min(4 << 32, relative_error))
    one_plus = (1 << 32) + ((-clamped) >> 4)
    new, overflow = safe_mul_fixed_point_rational(old_difficulty, one_plus & 0xFFFFFFFF, (one_plus >> 32) & 0xFFFFFFFF)
    return list(DIFFICULTY_MAXIMUM) if overflow > 0 else new


def pow_add(pow_limbs: Sequence[int], difficulty: Sequence[int]) -> List[int]:
    v = (_big(pow_limbs) + _big(difficulty)) % (1 << 192)
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(6)]


def should_reset_difficulty(p: Params, current_ts: int, previous_ts: int) -> bool:
    if p.difficulty_reset_interval is None:
        return False
    return gl_sub(current_ts, previous_ts) >= p.difficulty_reset_interval


# ------------------------------------------------------------------ rules
def mmr_append(mmr, leaf):
    """twenty-first MmrAccumulator::append of one leaf.  An accumulator whose peak count is not
    popcount(leaf_count) is refused here (None): the library fails such a parent closed as BLOCK_MMR_UPDATE,
    where the reference would carry it through `append`."""
    n, peaks = mmr["leaf_count"], [tuple(int(x) for x in pk) for pk in mmr["peaks"]]
    if len(peaks) != bin(n).count("1") or n == (1 << 64) - 1:
        return None
    acc = tuple(int(x) for x in leaf)
    k = n
    while k & 1:
        acc = PW.hp(peaks.pop(), acc)
        k >>= 1
    return {"leaf_count": n + 1, "peaks": peaks + [acc]}


def link_status(parent, child, p: Params, parent_hash=None) -> int:
    ph, ch = parent["header"], child["header"]
    if gl_add(ph["height"] % P, 1) != ch["height"] % P:
        return BLOCK_HEIGHT
    parent_hash = tuple(parent_hash) if parent_hash is not None else block_hash(parent)
    if parent_hash != tuple(int(x) for x in ch["prev_block_digest"]):
        return PREV_BLOCK_DIGEST
    after = mmr_append(parent["body"]["block_mmr_accumulator"], parent_hash)
    cm = child["body"]["block_mmr_accumulator"]
    if after is None or after["leaf_count"] != cm["leaf_count"] or \
            after["peaks"] != [tuple(int(x) for x in pk) for pk in cm["peaks"]]:
        return BLOCK_MMR_UPDATE
    if gl_add(ph["timestamp"] % P, p.minimum_block_time % P) > ch["timestamp"] % P:
        return MINIMUM_BLOCK_TIME
    if should_reset_difficulty(p, ch["timestamp"] % P, ph["timestamp"] % P):
        expected = difficulty_new(p.genesis_difficulty)
    else:
        expected = difficulty_control(ch["timestamp"] % P, ph["timestamp"] % P, ph["difficulty"],
                                      p.target_block_interval % P, ph["height"] % P)
    if list(ch["difficulty"]) != expected:
        return DIFFICULTY
    if list(ch["cumulative_proof_of_work"]) != pow_add(ph["cumulative_proof_of_work"], ph["difficulty"]):
        return CUMULATIVE_POW
    if ch["timestamp"] % P >= gl_add(p.now % P, FUTUREDATING_LIMIT):
        return FUTURE_DATING
    return OK


def has_proof_of_work(child, parent_header, p: Params, child_hash=None) -> bool:
    ch = child["header"]
    if should_reset_difficulty(p, ch["timestamp"] % P, parent_header["timestamp"] % P) and \
            list(ch["difficulty"]) == difficulty_new(p.genesis_difficulty):
        return True
    target = difficulty_target(parent_header["difficulty"])
    child_hash = tuple(child_hash) if child_hash is not None else block_hash(child)
    if p.allows_mock_pow and PW.digest_le(child_hash, target):
        return True
    reboot = gl_add(parent_header["height"] % P, 1) < p.hardfork_alpha_height
    return PW.validate(p.tree_height, tuple(ch["pow_root"]), [tuple(d) for d in ch["path_a"]],
                       [tuple(d) for d in ch["path_b"]], tuple(ch["nonce"]), pow_mast_paths(child), target, reboot,
                       tuple(ch["prev_block_digest"]))
