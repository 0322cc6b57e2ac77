"""GPU block digests and header-chain rules (k_block_proof_leaf, k_block_masts, k_block_links behind
nhip_blk_digests / nhip_blk_chain_check) against the CPU restatement tests/block_chain_ref.py, never against
themselves, with pow tree height H = 10.  The blocks, the two chains and every expected value are built once per
module and left unchanged.

A block's proof of work is found with the existing GPU guesser (nhip_pow_preprocess / nhip_pow_guess_batch) at
Difficulty::MINIMUM and confirmed by pow_ref.validate on the CPU before it is used as an expected accept.

"A target one below the digest": the target is Difficulty::target of the parent's difficulty, so it cannot be set
to an arbitrary digest.  The test uses the two neighbouring difficulties that straddle the digest: with
d = floor((p^5 - 1) / digest) the target is >= the digest (accept), with d + 1 it is below it (reject)."""
import copy
import ctypes
import random

import numpy as np
import pytest

import bincode_ref as B
import block_chain_ref as R
import pow_ref as W
import tip5_ref as T

pytestmark = pytest.mark.gpu

P, H = R.P, 10
PROOF_WORDS = [0, 1, 7, 8, 9, 10, 11, 19, 20, 21, 2003]   # item counts around every absorb boundary, and a long one
BIG_WORD = (10, 1234)                                    # (block with 2,003 words is PROOF_WORDS[10], word index)


def _claim(g):
    return {"program_digest": B._rd(g), "version": g.getrandbits(8), "input": [g.randrange(P) for _ in range(g.randrange(4))],
            "output": [g.randrange(P) for _ in range(g.randrange(4))]}


def _random_block(g, kind, proof=()):
    b = B.random_block(g, [_claim(g) for _ in range(g.randrange(3))], kind, list(proof), tree_height=H)
    b["header"]["version"] = g.randrange(P)
    return b


def _shifted(data: bytes, k: int) -> np.ndarray:
    """`data` at byte k of a 64-byte-aligned position inside a larger array: the gather's byte shift is k."""
    big = np.zeros(len(data) + 256, dtype=np.uint8)
    base = (-big.ctypes.data) % 64
    view = big[base + k:base + k + len(data)]
    view[:] = np.frombuffer(data, dtype=np.uint8)
    assert view.ctypes.data % 64 == k
    return view


def _records(data):
    from neptune_hip import blocks as NB
    return NB.blocks_from_bytes(data, H)


def _dig(x):
    return tuple(int(v) for v in x)


# ================================================================== digests
@pytest.fixture(scope="module")
def digest_blocks():
    T.use_c_backend()
    g = random.Random(2700)
    blocks = [_random_block(g, B.GENESIS), _random_block(g, B.INVALID)]
    blocks += [_random_block(g, B.SINGLE_PROOF, [g.randrange(P) for _ in range(n)]) for n in PROOF_WORDS]
    # one proof word >= p in the bytes: the dict holds its residue 5, the bytes hold p + 5
    bi, wi = 2 + BIG_WORD[0], BIG_WORD[1]
    blocks[bi]["proof"][wi] = 5
    enc = [bytearray(B.encode_block(b)) for b in blocks]
    at = len(enc[bi]) - 8 * (len(blocks[bi]["proof"]) - wi)
    assert int.from_bytes(enc[bi][at:at + 8], "little") == 5
    enc[bi][at:at + 8] = (P + 5).to_bytes(8, "little")
    want = [(R.block_hash(b), R.pow_mast_paths(b)) for b in blocks]
    return blocks, [bytes(e) for e in enc], want


def _check_digests(ctx, data, records, want):
    from neptune_hip import blocks as NB
    dig, mast = NB.block_digests(ctx, data, records, H, with_mast_paths=True)
    for i, (wd, wm) in enumerate(want):
        assert _dig(dig[i]) == wd, i
        assert tuple(tuple(p) for p in mast[i][0]) == tuple(wm[0]), i
        assert tuple(tuple(p) for p in mast[i][1]) == tuple(wm[1]), i
        assert tuple(tuple(p) for p in mast[i][2]) == tuple(wm[2]), i


@pytest.mark.parametrize("shift", range(8))
def test_digests_and_mast_paths_at_every_byte_shift(ctx, digest_blocks, shift):
    blocks, enc, want = digest_blocks
    assert len(blocks) == 13
    data = _shifted(b"".join(enc), shift)
    recs = _records(data)
    assert [r.proof_kind for r in recs] == [b["proof_kind"] for b in blocks]
    _check_digests(ctx, data, recs, want)


def test_digests_five_unequal_alone_and_reversed(ctx, digest_blocks):
    """Five blocks: the second wave has one live row beside three idle ones, and the rows of the first wave end at
    different times.  Then all thirteen in reversed order (every block in another row, beside other neighbours)."""
    blocks, enc, want = digest_blocks
    pick = [12, 0, 5, 9, 3]  # 2,003 words, Genesis, 8, 19 and 1 words
    data = _shifted(b"".join(enc[i] for i in pick), 3)
    _check_digests(ctx, data, _records(data), [want[i] for i in pick])
    order = list(reversed(range(13)))
    data = _shifted(b"".join(enc[i] for i in order), 5)
    _check_digests(ctx, data, _records(data), [want[i] for i in order])
    one = _shifted(enc[12], 1)
    _check_digests(ctx, one, _records(one), [want[12]])


def test_digests_prefix_boundary_lengths(ctx):
    """Item counts 5, 6, 15, 16: with the four prefix words counted in, the padding's 1 lands in the last rate
    word and at a fresh chunk's first word (PROOF_WORDS' boundaries are those of the items alone)."""
    g = random.Random(2701)
    blocks = [_random_block(g, B.SINGLE_PROOF, [g.randrange(P) for _ in range(n)]) for n in (5, 6, 15, 16)]
    data = _shifted(b"".join(B.encode_block(b) for b in blocks), 6)
    _check_digests(ctx, data, _records(data), [(R.block_hash(b), R.pow_mast_paths(b)) for b in blocks])


def test_body_hash_is_blocks_to_validate_s(ctx, digest_blocks):
    """The body MAST hash inside the digest is the one `blocks_to_validate` computes: the kernel and block MASTs
    rebuilt on the CPU over that hash give nhip_blk_digests' digest."""
    from neptune_hip import blocks as NB
    import mast_ref as M
    blocks, enc, want = digest_blocks
    pick = [1, 4, 12]
    data = b"".join(enc[i] for i in pick)
    recs = _records(data)
    dig = NB.block_digests(ctx, data, recs, H)
    for k, (i, v) in enumerate(zip(pick, NB.blocks_to_validate(ctx, recs))):
        b = blocks[i]
        assert _dig(v.body_mast_hash) == R.body_mast_hash(b["body"])
        kernel = M.mast_hash([list(M.mast_hash(R.header_sequences(b["header"]))), [int(x) for x in v.body_mast_hash],
                              R.appendix_encoding(b["appendix"])])
        assert M.mast_hash([list(kernel), R.proof_encoding(b["proof_kind"], b["proof"])]) == _dig(dig[k])


# ================================================================== proof of work with the existing guesser
def _solve(ctx, b, target, reboot, seed):
    """Fill b's pow field with a solution found by the GPU guesser; returns the guess digest."""
    from neptune_hip.pow import Pow, PowMastPaths
    h = b["header"]
    mast = R.pow_mast_paths(b)
    pm = PowMastPaths(*mast)
    buf = Pow.preprocess(ctx, H, pm, reboot, h["prev_block_digest"])
    try:
        picker = buf.index_picker_preimage(pm)
        rng = np.random.default_rng(seed)
        for _ in range(6):
            nonces = rng.integers(0, P, size=(1 << 15, 5), dtype=np.uint64)
            dig, idx, ok = Pow.guess(ctx, buf, pm, picker, nonces, target)
            hit = np.flatnonzero(ok)
            if hit.size:
                k = int(hit[0])
                h["nonce"] = [int(x) for x in nonces[k]]
                h["pow_root"] = list(buf.root())
                h["path_a"] = [list(d) for d in buf.path(int(idx[k][0]))]
                h["path_b"] = [list(d) for d in buf.path(int(idx[k][1]))]
                return _dig(dig[k])
    finally:
        buf.close()
    raise AssertionError("no nonce met the target in 196,608 guesses at difficulty 6,000")


def test_guess_digest_is_the_block_digest(ctx):
    """nhip_pow_preprocess / nhip_pow_guess_batch with the paths nhip_blk_digests derives: once the winning nonce and
    its authentication paths are written into the header, nhip_blk_digests gives the guess digest."""
    from neptune_hip import blocks as NB
    from neptune_hip.pow import Pow, PowMastPaths
    T.use_c_backend()
    g = random.Random(2702)
    b = _random_block(g, B.SINGLE_PROOF, [g.randrange(P) for _ in range(33)])
    data = B.encode_block(b)
    _, mast = NB.block_digests(ctx, data, _records(data), H, with_mast_paths=True)
    assert (tuple(mast[0][0]), tuple(mast[0][1]), tuple(mast[0][2])) == tuple(tuple(p) for p in R.pow_mast_paths(b))
    pm = PowMastPaths(*mast[0])
    for reboot in (True, False):
        buf = Pow.preprocess(ctx, H, pm, reboot, b["header"]["prev_block_digest"])
        nonce = [g.randrange(P) for _ in range(5)]
        dig, idx, _ = Pow.guess(ctx, buf, pm, buf.index_picker_preimage(pm), [nonce], (P - 1,) * 5)
        c = copy.deepcopy(b)
        c["header"].update(nonce=nonce, pow_root=list(buf.root()), path_a=[list(d) for d in buf.path(int(idx[0][0]))],
                           path_b=[list(d) for d in buf.path(int(idx[0][1]))])
        buf.close()
        data2 = B.encode_block(c)
        assert _dig(NB.block_digests(ctx, data2, _records(data2), H)[0]) == _dig(dig[0]) == R.block_hash(c)


# ================================================================== links
T0 = 1_754_420_400_000


def _params(**kw):
    base = dict(minimum_block_time=1, target_block_interval=100, difficulty_reset_interval=None,
                genesis_difficulty=list(R.DIFFICULTY_MINIMUM), hardfork_alpha_height=0, now=T0 + 10_000_000,
                tree_height=H, allows_mock_pow=False)
    base.update(kw)
    return R.Params(**base)


def _c_params(p: R.Params):
    import neptune_hip._lib as L
    c = L.ChainParams()
    c.minimum_block_time_ms, c.target_block_interval_ms = p.minimum_block_time, p.target_block_interval
    c.difficulty_reset_interval_ms = p.difficulty_reset_interval or 0
    for i, x in enumerate(p.genesis_difficulty):
        c.genesis_difficulty[i] = x
    c.hardfork_alpha_height, c.now_ms = p.hardfork_alpha_height, p.now
    c.pow_tree_height, c.allows_mock_pow = p.tree_height, 1 if p.allows_mock_pow else 0
    return c


def _child_of(g, parent, p: R.Params, dt, n_proof=12):
    """A block that satisfies rules 0.a-0.g after `parent` (its pow field still random)."""
    ph = parent["header"]
    b = _random_block(g, B.SINGLE_PROOF, [g.randrange(P) for _ in range(n_proof)])
    h = b["header"]
    h["height"] = R.gl_add(ph["height"], 1)
    h["prev_block_digest"] = list(R.block_hash(parent))
    h["timestamp"] = R.gl_add(ph["timestamp"], dt)
    if R.should_reset_difficulty(p, h["timestamp"], ph["timestamp"]):
        h["difficulty"] = R.difficulty_new(p.genesis_difficulty)
    else:
        h["difficulty"] = R.difficulty_control(h["timestamp"], ph["timestamp"], ph["difficulty"], p.target_block_interval,
                                               ph["height"])
    h["cumulative_proof_of_work"] = R.pow_add(ph["cumulative_proof_of_work"], ph["difficulty"])
    after = R.mmr_append(parent["body"]["block_mmr_accumulator"], R.block_hash(parent))
    b["body"]["block_mmr_accumulator"] = {"leaf_count": after["leaf_count"], "peaks": [list(x) for x in after["peaks"]]}
    return b


class Pairs:
    """Blocks and (parent, child) pairs for one nhip_blk_chain_check call."""

    def __init__(self):
        self.blocks, self.parent_of, self.names = [], [], []

    def add(self, block, parent=-1, name=""):
        self.blocks.append(block)
        self.parent_of.append(parent)
        self.names.append(name)
        return len(self.blocks) - 1

    def run(self, ctx, p: R.Params, order=None):
        from neptune_hip import blocks as NB
        order = list(range(len(self.blocks))) if order is None else order
        pos = {b: k for k, b in enumerate(order)}
        data = b"".join(B.encode_block(self.blocks[i]) for i in order)
        par = [pos[self.parent_of[i]] if self.parent_of[i] >= 0 else -1 for i in order]
        got = NB.chain_links(ctx, data, _records(data), None, 0, parent_of=par, pow_tree_height=H, params=_c_params(p))
        return [got[pos[i]] for i in range(len(self.blocks))]

    def expected(self, p: R.Params):
        out = []
        for b, par in zip(self.blocks, self.parent_of):
            if par < 0:
                out.append((R.SKIPPED, False))
                continue
            parent = self.blocks[par]
            try:
                pow_ok = R.has_proof_of_work(b, parent["header"], p)
            except R.ReferencePanics:
                pow_ok = False
            out.append((R.link_status(parent, b, p), pow_ok))
        return out


@pytest.fixture(scope="module")
def chain(ctx):
    """Six blocks from a synthetic genesis on RegTest-like parameters, every proof of work found by the GPU guesser
    (HardforkAlpha rules) and confirmed on the CPU; and a sixth block of its own for the mock-PoW chain, solved by
    mock PoW only (a digest under the target, no valid authentication paths)."""
    T.use_c_backend()
    g = random.Random(2703)
    p = _params()
    genesis = _random_block(g, B.GENESIS)
    gh = genesis["header"]
    gh.update(height=0, timestamp=T0, difficulty=list(R.DIFFICULTY_MINIMUM), cumulative_proof_of_work=[0] * 6)
    genesis["body"]["block_mmr_accumulator"] = {"leaf_count": 0, "peaks": []}
    blocks = [genesis]
    for k, dt in enumerate([100, 1, 100, 700, 40, 100]):   # the minimum, the target, 7 x the target, under it
        b = _child_of(g, blocks[-1], p, dt)
        ph = blocks[-1]["header"]
        target = R.difficulty_target(ph["difficulty"])
        d = _solve(ctx, b, target, reboot=False, seed=40 + k)
        h = b["header"]
        assert W.validate(H, tuple(h["pow_root"]), [tuple(x) for x in h["path_a"]], [tuple(x) for x in h["path_b"]],
                          tuple(h["nonce"]), R.pow_mast_paths(b), target, False, tuple(h["prev_block_digest"]))
        assert d == R.block_hash(b) and W.digest_le(d, target)
        blocks.append(b)
    # the mock-PoW block: random pow fields until the digest meets the target (fast_mast_hash over the fixed paths)
    mock = _child_of(g, blocks[5], p, 100)
    mast, mh = R.pow_mast_paths(mock), mock["header"]
    target = R.difficulty_target(blocks[5]["header"]["difficulty"])
    for i in range(200_000):   # ~6,000 tries expected, about a second
        mh["nonce"] = [i, 0, 0, 0, 0]
        if W.digest_le(W.fast_mast_hash(mast, mh["pow_root"], mh["path_a"], mh["path_b"], mh["nonce"]), target):
            break
    assert W.digest_le(R.block_hash(mock), target)
    assert not R.has_proof_of_work(mock, blocks[5]["header"], p)   # no valid paths: only mock PoW accepts it
    return blocks, mock


def test_both_chains_are_accepted(ctx, chain):
    blocks, mock = chain
    for mock_allowed, last in ((True, mock), (False, blocks[6])):
        p = _params(allows_mock_pow=mock_allowed)
        pairs = Pairs()
        for i, b in enumerate(blocks[:6] + [last]):
            pairs.add(b, i - 1)
        got = pairs.run(ctx, p)
        assert got == pairs.expected(p)
        assert got == [(R.SKIPPED, False)] + [(R.OK, True)] * 6
    # the default parent is the block before it in the file
    from neptune_hip import blocks as NB
    data = b"".join(B.encode_block(b) for b in blocks)
    got = NB.chain_links(ctx, data, _records(data), None, 0, pow_tree_height=H, params=_c_params(_params()))
    assert got == [(R.SKIPPED, False)] + [(R.OK, True)] * 6
    # the mock-solved block without mock PoW: the link holds, the proof of work does not
    pairs = Pairs()
    pairs.add(blocks[5])
    pairs.add(mock, 0)
    assert pairs.run(ctx, _params())[1] == (R.OK, False)


def _mutants(blocks):
    """(name, parent, child, expected status or None = unchanged OK): one field of one block changed each."""
    def child(i, f):
        c = copy.deepcopy(blocks[i])
        f(c)
        return c

    def setter(key, fn, where="header"):
        def f(c):
            tgt = c[where] if where == "header" else c["body"]["block_mmr_accumulator"]
            tgt[key] = fn(tgt[key])
        return f

    flip0 = lambda v: [(v[0] + 1) % P] + list(v[1:])          # noqa: E731
    limb0 = lambda v: [v[0] ^ 1] + list(v[1:])                # noqa: E731
    out = [
        ("height", 2, child(3, setter("height", lambda v: v + 1)), R.BLOCK_HEIGHT),
        ("prev digest", 2, child(3, setter("prev_block_digest", flip0)), R.PREV_BLOCK_DIGEST),
        ("mmr peak", 3, child(4, setter("peaks", lambda v: [flip0(v[0])] + v[1:], "mmr")), R.BLOCK_MMR_UPDATE),
        ("mmr last peak", 4, child(5, setter("peaks", lambda v: v[:-1] + [flip0(v[-1])], "mmr")), R.BLOCK_MMR_UPDATE),
        ("mmr leaf count", 3, child(4, setter("leaf_count", lambda v: v + 1, "mmr")), R.BLOCK_MMR_UPDATE),
        ("timestamp under the minimum", 1, child(2, setter("timestamp", lambda v: v - 1)), R.MINIMUM_BLOCK_TIME),
        ("difficulty", 4, child(5, setter("difficulty", limb0)), R.DIFFICULTY),
        ("cumulative pow", 4, child(5, setter("cumulative_proof_of_work", limb0)), R.CUMULATIVE_POW),
        # two rules at once: the earlier one is the status
        ("height and prev digest", 2,
         child(3, lambda c: (setter("height", lambda v: v + 1)(c), setter("prev_block_digest", flip0)(c))), R.BLOCK_HEIGHT),
        ("difficulty and cumulative pow", 4,
         child(5, lambda c: (setter("difficulty", limb0)(c), setter("cumulative_proof_of_work", limb0)(c))), R.DIFFICULTY),
        ("mmr peak and timestamp", 1,
         child(2, lambda c: (setter("timestamp", lambda v: v - 1)(c),
                             setter("peaks", lambda v: [flip0(v[0])] + v[1:], "mmr")(c))), R.BLOCK_MMR_UPDATE),
        # proof-of-work mutants: the link status stays OK
        ("wrong nonce", 2, child(3, setter("nonce", flip0)), None),
        ("flipped path word", 2, child(3, setter("path_a", lambda v: v[:4] + [flip0(v[4])] + v[5:])), None),
        ("flipped root", 2, child(3, setter("pow_root", flip0)), None),
    ]
    return out


def test_one_mutant_per_status_and_pow_mutants(ctx, chain):
    blocks, _ = chain
    p = _params()
    pairs = Pairs()
    for i, b in enumerate(blocks):
        pairs.add(b, i - 1, f"block {i}")
    want_status = {}
    for name, par, c, status in _mutants(blocks):
        want_status[pairs.add(c, par, name)] = status
    # an inconsistent parent accumulator (peak count != popcount) fails closed
    bad_parent = copy.deepcopy(blocks[3])
    bad_parent["body"]["block_mmr_accumulator"]["peaks"].append(B._rd(random.Random(1)))
    k = pairs.add(bad_parent, 2, "parent with a surplus peak")
    fixed = copy.deepcopy(blocks[4])
    fixed["header"]["prev_block_digest"] = list(R.block_hash(bad_parent))
    want_status[pairs.add(fixed, k, "child of the inconsistent parent")] = R.BLOCK_MMR_UPDATE
    # a parent whose leaf count cannot grow (2^64 - 1 leaves, 64 peaks: consistent, but append would overflow)
    full_parent = copy.deepcopy(blocks[3])
    g = random.Random(2)
    full_parent["body"]["block_mmr_accumulator"] = {"leaf_count": (1 << 64) - 1, "peaks": [B._rd(g) for _ in range(64)]}
    k = pairs.add(full_parent, 2, "parent with 2^64 - 1 leaves")
    child = copy.deepcopy(blocks[4])
    child["header"]["prev_block_digest"] = list(R.block_hash(full_parent))
    child["body"]["block_mmr_accumulator"] = {"leaf_count": 0, "peaks": []}   # what a wrapping count would give
    want_status[pairs.add(child, k, "child of the full parent")] = R.BLOCK_MMR_UPDATE
    got, want = pairs.run(ctx, p), pairs.expected(p)
    for i, name in enumerate(pairs.names):
        assert got[i] == want[i], name
    for i, status in want_status.items():
        if status is None:
            assert got[i] == (R.OK, False), pairs.names[i]
        else:
            assert got[i][0] == status, pairs.names[i]
    assert {got[i][0] for i in want_status} >= {R.BLOCK_HEIGHT, R.PREV_BLOCK_DIGEST, R.BLOCK_MMR_UPDATE,
                                                R.MINIMUM_BLOCK_TIME, R.DIFFICULTY, R.CUMULATIVE_POW}
    # future dating: `now` moved so that block 6's timestamp is exactly the limit, then one millisecond inside it
    ts = blocks[6]["header"]["timestamp"]
    pairs = Pairs()
    pairs.add(blocks[5])
    pairs.add(blocks[6], 0)
    late = _params(now=ts - R.FUTUREDATING_LIMIT)
    assert pairs.run(ctx, late)[1] == (R.FUTURE_DATING, True) == pairs.expected(late)[1]
    ontime = _params(now=ts - R.FUTUREDATING_LIMIT + 1)
    assert pairs.run(ctx, ontime)[1] == (R.OK, True) == pairs.expected(ontime)[1]


def test_pairs_one_per_call_equal_one_call(ctx, chain):
    blocks, mock = chain
    p = _params(allows_mock_pow=True)
    pairs = Pairs()
    for i, b in enumerate(blocks):
        pairs.add(b, i - 1)
    pairs.add(mock, 5)
    for name, par, c, _ in _mutants(blocks):
        pairs.add(c, par, name)
    together = pairs.run(ctx, p)
    assert together == pairs.expected(p)
    for i, par in enumerate(pairs.parent_of):
        if par < 0:
            continue
        single = Pairs()
        single.add(pairs.blocks[par])
        single.add(pairs.blocks[i], 0)
        assert single.run(ctx, p) == [(R.SKIPPED, False), together[i]], pairs.names[i]


def test_target_straddles_the_digest(ctx, chain):
    """The parent's difficulty moved to the two neighbours that straddle block 3's digest: accepted with
    d = floor((p^5 - 1) / digest), refused with d + 1; the link status (the parent's digest changed) is the same."""
    blocks, _ = chain
    digest = sum(x * P ** i for i, x in enumerate(R.block_hash(blocks[3])))
    d = (P ** 5 - 1) // digest
    assert 6000 <= d < (1 << 160) - 1
    pairs = Pairs()
    for dd in (d, d + 1):
        parent = copy.deepcopy(blocks[2])
        parent["header"]["difficulty"] = [(dd >> (32 * i)) & 0xFFFFFFFF for i in range(5)]
        k = pairs.add(parent)
        pairs.add(blocks[3], k)
    p = _params()
    got = pairs.run(ctx, p)
    assert got == pairs.expected(p)
    assert got[1] == (R.PREV_BLOCK_DIGEST, True) and got[3] == (R.PREV_BLOCK_DIGEST, False)
    # and through mock PoW, whose comparison is the digest's alone
    pm = _params(allows_mock_pow=True)
    bad = copy.deepcopy(blocks[3])
    bad["header"]["nonce"][0] ^= 1   # no valid proof of work; its own digest decides
    digest = sum(x * P ** i for i, x in enumerate(R.block_hash(bad)))
    d = (P ** 5 - 1) // digest
    pairs = Pairs()
    for dd in (d, d + 1):
        parent = copy.deepcopy(blocks[2])
        parent["header"]["difficulty"] = [(dd >> (32 * i)) & 0xFFFFFFFF for i in range(5)]
        pairs.add(bad, pairs.add(parent))
    got = pairs.run(ctx, pm)
    assert got == pairs.expected(pm) and [g[1] for g in got] == [False, True, False, False]


def test_reset_interval_network_skips_the_pow_check(ctx, chain):
    blocks, _ = chain
    g = random.Random(2704)
    p = _params(difficulty_reset_interval=1000, genesis_difficulty=[100_000, 0, 0, 0, 0])
    late = _child_of(g, blocks[4], p, 1000)        # the gap is the interval: reset, garbage pow field
    assert late["header"]["difficulty"] == [100_000, 0, 0, 0, 0]
    early = _child_of(g, blocks[4], p, 999)        # one millisecond short: no reset, the garbage pow is refused
    wrong = copy.deepcopy(late)
    wrong["header"]["difficulty"] = list(blocks[4]["header"]["difficulty"])   # reset gap, not the genesis difficulty
    pairs = Pairs()
    k = pairs.add(blocks[4])
    for b in (late, early, wrong):
        pairs.add(b, k)
    got = pairs.run(ctx, p)
    assert got == pairs.expected(p)
    assert got[1:] == [(R.OK, True), (R.OK, False), (R.DIFFICULTY, False)]


def test_reorganised_buffer_through_parent_of(ctx, chain):
    """Children before their parents, two children of one parent, and a -1 entry that is skipped."""
    blocks, mock = chain
    p = _params(allows_mock_pow=True)
    pairs = Pairs()
    for i, b in enumerate(blocks):
        pairs.add(b, i - 1)
    pairs.add(mock, 5)                 # block 6's sibling
    pairs.parent_of[3] = -1            # a pair the caller does not want checked
    order = [7, 6, 3, 0, 5, 2, 4, 1]
    got = pairs.run(ctx, p, order)
    assert got == pairs.expected(p)
    assert got[3] == (R.SKIPPED, False) and got[0] == (R.SKIPPED, False)
    assert [got[i] for i in (1, 2, 4, 5, 6, 7)] == [(R.OK, True)] * 6


def test_hardfork_height_picks_the_rule_set(ctx, chain):
    """Block 3 (height 3) was solved under HardforkAlpha.  With the threshold at 3 it is validated under
    HardforkAlpha, at 4 under Reboot; a Reboot solution of the same block the other way round."""
    blocks, _ = chain
    reboot_block = copy.deepcopy(blocks[3])
    target = R.difficulty_target(blocks[2]["header"]["difficulty"])
    _solve(ctx, reboot_block, target, reboot=True, seed=77)
    pairs = Pairs()
    pairs.add(blocks[2])
    pairs.add(blocks[3], 0)
    pairs.add(reboot_block, 0)
    for alpha, want in ((3, [True, False]), (4, [False, True]), (0, [True, False])):
        p = _params(hardfork_alpha_height=alpha)
        got = pairs.run(ctx, p)
        for b, g_ in zip((blocks[3], reboot_block), got[1:]):
            h = b["header"]
            ref = W.validate(H, tuple(h["pow_root"]), [tuple(x) for x in h["path_a"]], [tuple(x) for x in h["path_b"]],
                             tuple(h["nonce"]), R.pow_mast_paths(b), target, alpha != 0 and 3 < alpha,
                             tuple(h["prev_block_digest"]))
            assert g_ == (R.OK, ref)
        assert [g_[1] for g_ in got[1:]] == want


# ================================================================== 130 blocks: three workgroups, non-trivial integers
BIG_N = 130                                   # k_block_links / k_block_masts: workgroups of 64, 64 and 2 lanes
MAXIMUM = (1 << 160) - 1
MMR_MERGES = (1, 2, 5, 31, 63)                # leaf counts 2^k - 1: k merges, no peak kept


def _limbs(v, n):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def _synthetic_parent(g, **header):
    """A parent no rule is checked on: a consistent block MMR (5 leaves, 2 peaks), a timestamp near T0, a height
    that is not genesis; `header` overrides."""
    b = _random_block(g, B.SINGLE_PROOF, [g.randrange(P) for _ in range(g.randrange(13))])
    b["header"].update(height=1000 + g.randrange(1000), timestamp=T0 + g.randrange(1_000_000))
    b["header"].update(header)
    b["body"]["block_mmr_accumulator"] = {"leaf_count": 5, "peaks": [B._rd(g), B._rd(g)]}
    return b


def _big_pairs(seed=2705):
    """130 synthetic blocks for one call (no proof of work is solved): accepted pairs with multi-limb integers, one
    mutant per pair that fails exactly the rule in question, and children of parents with difficulties 1, 2, 3 and 7
    whose digest decides mock proof of work.  Returns (pairs, order in the buffer, accepted, mutants, mock)."""
    T.use_c_backend()
    g = random.Random(seed)
    p = _params(allows_mock_pow=True)
    pairs, accepted, mutants, mock = Pairs(), [], {}, []

    def accept(parent, dt, name, mutate, status, mutant_parent=None):
        k = pairs.add(parent, -1, "parent: " + name)
        child = _child_of(g, parent, p, dt, n_proof=g.randrange(13))
        accepted.append(pairs.add(child, k, name))
        if mutant_parent is not None:            # the rule reads the parent: a pair of its own
            k = pairs.add(mutant_parent, -1, "mutant parent: " + name)
            bad = _child_of(g, mutant_parent, p, dt, n_proof=g.randrange(13))
        else:
            bad = copy.deepcopy(child)
            mutate(bad)
        mutants[pairs.add(bad, k, "mutant: " + name)] = status

    def flip_difficulty(c):
        c["header"]["difficulty"][3] ^= 1

    def flip_pow(c):
        c["header"]["cumulative_proof_of_work"][5] ^= 1

    def flip_peak(c):
        pk = c["body"]["block_mmr_accumulator"]["peaks"]
        pk[-1] = [(pk[-1][0] + 1) % P] + list(pk[-1][1:])

    # multi-limb difficulties: unchanged at the target interval, raised to the MAXIMUM overflow, lowered
    for dv, dt in ((1 << 32, 100), ((1 << 95) + 12345, 700), (MAXIMUM, 40)):
        accept(_synthetic_parent(g, difficulty=_limbs(dv, 5)), dt, f"difficulty {dv:#x}", flip_difficulty, R.DIFFICULTY)
    # cumulative proof of work that carries through every limb and wraps
    accept(_synthetic_parent(g, cumulative_proof_of_work=[0xFFFFFFFF] * 6, difficulty=[6000, 0, 0, 0, 0]), 100,
           "pow carries through six limbs", flip_pow, R.CUMULATIVE_POW)
    # the child's timestamp wraps past p: p - 1 + 100 = 99, and p - 1 + minimum_block_time = 0 <= 99.  One
    # millisecond earlier the parent's p - 2 + 1 = p - 1 does not wrap and is above the child's 98.
    accept(_synthetic_parent(g, timestamp=P - 1), 100, "timestamp wraps past p", None, R.MINIMUM_BLOCK_TIME,
           mutant_parent=_synthetic_parent(g, timestamp=P - 2))
    # height p - 1, whose child has height 0
    accept(_synthetic_parent(g, height=P - 1), 100, "height p - 1", lambda c: c["header"].update(height=1), R.BLOCK_HEIGHT)
    # block MMRs: 2^k - 1 leaves (k merges, no peak kept) and 2^40 leaves (no merge)
    for k in MMR_MERGES:
        parent = _synthetic_parent(g)
        parent["body"]["block_mmr_accumulator"] = {"leaf_count": (1 << k) - 1, "peaks": [B._rd(g) for _ in range(k)]}
        accept(parent, 100, f"mmr with 2^{k} - 1 leaves", flip_peak, R.BLOCK_MMR_UPDATE)
    parent = _synthetic_parent(g)
    parent["body"]["block_mmr_accumulator"] = {"leaf_count": 1 << 40, "peaks": [B._rd(g)]}
    accept(parent, 100, "mmr with 2^40 leaves", flip_peak, R.BLOCK_MMR_UPDATE)
    # mock proof of work: Difficulty::target does not clamp, so the targets are (p^5 - 1) / 1, 2, 3 and 7
    roots = [pairs.add(_synthetic_parent(g, difficulty=[d, 0, 0, 0, 0]), -1, f"parent: difficulty {d}") for d in (1, 2, 3, 7)]
    while len(pairs.blocks) < BIG_N:
        k = roots[len(mock) % 4]
        mock.append(pairs.add(_child_of(g, pairs.blocks[k], p, 100, n_proof=g.randrange(13)), k, "mock pow child"))
    # the buffer's order: shuffled, then a mock parent and an accepted child in the last workgroup's two lanes
    order = list(range(BIG_N))
    g.shuffle(order)
    for pos, blk in ((128, roots[1]), (129, accepted[0])):
        at = order.index(blk)
        order[at], order[pos] = order[pos], order[at]
    return pairs, order, accepted, mutants, mock, p


@pytest.fixture(scope="module")
def big():
    pairs, order, accepted, mutants, mock, p = _big_pairs()
    want = pairs.expected(p)
    hashes = [R.block_hash(b) for b in pairs.blocks]
    # all on the reference: the shape of the call and both mock verdicts
    assert len(pairs.blocks) == BIG_N and len(mock) >= 40
    pos = {b: k for k, b in enumerate(order)}
    wg = [(pos[i] // 64, pos[par] // 64) for i, par in enumerate(pairs.parent_of) if par >= 0]
    assert sum(c < q for c, q in wg) >= 5 and sum(c > q for c, q in wg) >= 5        # parent_of across workgroups
    assert any(c == 2 for c, _ in wg) and any(q == 2 and c != 2 for c, q in wg)     # and into / out of the last one
    assert all(want[i] == (R.OK, False) for i in accepted)                          # targets far below any digest
    assert all(want[i][0] == s for i, s in mutants.items())
    verdicts = []
    for i in mock:
        target = R.difficulty_target(pairs.blocks[pairs.parent_of[i]]["header"]["difficulty"])
        verdicts.append(W.digest_le(hashes[i], target))
        assert want[i] == (R.OK, verdicts[-1])
    assert verdicts.count(True) >= 5 and verdicts.count(False) >= 5
    return pairs, order, p, want, hashes


def test_130_blocks_links_and_mock_pow_over_three_workgroups(ctx, big):
    """One nhip_blk_chain_check call: every status and pow_ok is the reference's, the accepted pairs with multi-limb
    difficulties, a wrapping cumulative pow, a wrapping timestamp, height p - 1 and block MMRs of up to 63 merges, their
    mutants, and mock proof of work against targets of difficulties 1, 2, 3 and 7."""
    pairs, order, p, want, _ = big
    got = pairs.run(ctx, p, order)
    for i, name in enumerate(pairs.names):
        assert got[i] == want[i], (i, name)


def test_130_block_digests_over_three_workgroups(ctx, big):
    from neptune_hip import blocks as NB
    pairs, order, _, _, hashes = big
    data = b"".join(B.encode_block(pairs.blocks[i]) for i in order)
    dig = NB.block_digests(ctx, data, _records(data), H)
    assert len(dig) == BIG_N
    for k, i in enumerate(order):
        assert _dig(dig[k]) == hashes[i], (k, pairs.names[i])


# ================================================================== errors
def test_argument_errors(ctx, chain):
    import neptune_hip._lib as L
    from neptune_hip import blocks as NB
    blocks, _ = chain
    data = b"".join(B.encode_block(b) for b in blocks[:3])
    recs = _records(data)
    for bad in ([-1, 0, 3], [-1, -2, 1], [3, 0, 1]):
        with pytest.raises(L.NhipError, match="invalid argument"):
            NB.chain_links(ctx, data, recs, None, 0, parent_of=bad, pow_tree_height=H, params=_c_params(_params()))
    a = np.frombuffer(data, dtype=np.uint8)
    scanned = NB._scanned(recs)
    par = np.array([-1, 0, 1], dtype=np.int64)
    cp = _c_params(_params())
    st, ok, dig = np.full(3, 0xAA, np.uint8), np.full(3, 0xAA, np.uint8), np.full(15, 7, np.uint64)
    call = lambda *args: ctx.lib.nhip_blk_chain_check(ctx.handle, *args)   # noqa: E731
    sc = ctypes.cast(scanned, ctypes.c_void_p)
    # a null pointer with n > 0
    assert call(None, len(data), ctypes.byref(cp), sc, 3, par.ctypes.data, st.ctypes.data, ok.ctypes.data, None) == L.NHIP_ERR_ARG
    assert call(a.ctypes.data, len(data), ctypes.byref(cp), None, 3, par.ctypes.data, st.ctypes.data, ok.ctypes.data, None) == L.NHIP_ERR_ARG
    assert call(a.ctypes.data, len(data), ctypes.byref(cp), sc, 3, None, st.ctypes.data, ok.ctypes.data, None) == L.NHIP_ERR_ARG
    assert call(a.ctypes.data, len(data), ctypes.byref(cp), sc, 3, par.ctypes.data, None, ok.ctypes.data, None) == L.NHIP_ERR_ARG
    assert call(a.ctypes.data, len(data), ctypes.byref(cp), sc, 3, par.ctypes.data, st.ctypes.data, None, None) == L.NHIP_ERR_ARG
    assert call(a.ctypes.data, len(data), None, sc, 3, par.ctypes.data, st.ctypes.data, ok.ctypes.data, None) == L.NHIP_ERR_ARG
    assert ctx.lib.nhip_blk_digests(ctx.handle, a.ctypes.data, len(data), H, sc, 3, None, None) == L.NHIP_ERR_ARG
    assert ctx.lib.nhip_blk_digests(ctx.handle, None, len(data), H, sc, 3, dig.ctypes.data, None) == L.NHIP_ERR_ARG
    assert ctx.lib.nhip_blk_digests(ctx.handle, a.ctypes.data, len(data), 33, sc, 3, dig.ctypes.data, None) == L.NHIP_ERR_ARG
    # n = 0 is NHIP_OK and touches nothing
    assert call(None, 0, ctypes.byref(cp), None, 0, None, st.ctypes.data, ok.ctypes.data, dig.ctypes.data) == L.NHIP_OK
    assert ctx.lib.nhip_blk_digests(ctx.handle, None, 0, H, None, 0, dig.ctypes.data, None) == L.NHIP_OK
    assert (st == 0xAA).all() and (ok == 0xAA).all() and (dig == 7).all()
    # a failed call leaves the outputs alone; a good one after it works
    assert call(a.ctypes.data, len(data), ctypes.byref(cp), sc, 3, par.ctypes.data, st.ctypes.data, ok.ctypes.data,
                dig.ctypes.data) == L.NHIP_OK
    assert list(st) == [R.SKIPPED, R.OK, R.OK] and list(ok) == [0, 1, 1]
    assert [_dig(dig[5 * i:5 * i + 5]) for i in range(3)] == [R.block_hash(b) for b in blocks[:3]]
    # a truncated buffer is a decode error, not a status byte
    scanned[2].size -= 1
    assert call(a.ctypes.data, len(data) - 1, ctypes.byref(cp), sc, 3, par.ctypes.data, st.ctypes.data, ok.ctypes.data,
                None) == L.NHIP_ERR_DECODE
