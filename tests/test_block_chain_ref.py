"""The CPU side of the block digests and the header-chain rules: the restatement
tests/block_chain_ref.py held to itself where the reference gives an identity (fast_mast_hash over the restated
paths = the restated Block::hash; every mast_path verifies against its MAST root; target(d) is the floor of
(p^5 - 1) / d), and the library's host-only exports nhip_blk_header, nhip_difficulty_target and
nhip_difficulty_control held to the restatement.  No GPU."""
import ctypes
import random

import numpy as np
import pytest

import bincode_ref as B
import block_chain_ref as R
import mast_ref as M
import pow_ref as PW
import tip5_ref as T

P = R.P
H = 3  # pow tree height of the synthetic blocks (the layouts do not depend on it)
MINIMUM, MAXIMUM = R.DIFFICULTY_MINIMUM, R.DIFFICULTY_MAXIMUM
DIFFICULTY_EDGES = [MINIMUM, [5999, 0, 0, 0, 0], [1, 0, 0, 0, 0], MAXIMUM, [0, 1, 0, 0, 0], [0, 0, 0, 0, 1 << 31]]


@pytest.fixture(scope="module", autouse=True)
def _fast_tip5():
    T.use_c_backend()


def _claim(g):
    return {"program_digest": B._rd(g), "version": g.getrandbits(8), "input": [g.randrange(P) for _ in range(g.randrange(4))],
            "output": [g.randrange(P) for _ in range(g.randrange(4))]}


def _block(g, kind=None, n_proof=None):
    kind = g.choice([B.GENESIS, B.INVALID, B.SINGLE_PROOF]) if kind is None else kind
    proof = [g.randrange(P) for _ in range(g.randrange(30) if n_proof is None else n_proof)]
    b = B.random_block(g, [_claim(g) for _ in range(g.randrange(3))], kind, proof, tree_height=H)
    b["header"]["version"] = g.randrange(P)
    return b


def test_fast_mast_hash_over_the_restated_paths_is_the_block_hash():
    g = random.Random(11)
    for _ in range(6):
        b = _block(g)
        h = b["header"]
        assert PW.fast_mast_hash(R.pow_mast_paths(b), h["pow_root"], h["path_a"], h["path_b"], h["nonce"]) == R.block_hash(b)


def test_every_mast_path_verifies_against_its_root():
    g = random.Random(12)
    for _ in range(4):
        b = _block(g)
        pow_, header, kernel = R.pow_mast_paths(b)
        assert (len(pow_), len(header), len(kernel)) == (3, 2, 1)
        hs, ks, bs = R.header_sequences(b["header"]), R.kernel_sequences(b), R.block_sequences(b)
        assert R.mast_verify(M.mast_hash(hs), 4, pow_, hs[4])
        assert R.mast_verify(M.mast_hash(ks), 0, header, ks[0])
        assert R.mast_verify(M.mast_hash(bs), 0, kernel, bs[0])
        assert not R.mast_verify(M.mast_hash(hs), 5, pow_, hs[4])
        for f in range(8):  # every header field's own path
            assert R.mast_verify(M.mast_hash(hs), f, R.mast_path(hs, f), hs[f])


def _difficulties(g, n):
    return DIFFICULTY_EDGES + [[g.getrandbits(g.choice([1, 13, 32])) for _ in range(5)] for _ in range(n)]


def test_target_is_the_floor_of_the_quotient():
    g = random.Random(13)
    for d in _difficulties(g, 200):
        if not any(d):
            continue
        t = sum(x * P ** i for i, x in enumerate(R.difficulty_target(d)))
        den = sum(x << (32 * i) for i, x in enumerate(d))
        assert t * den <= P ** 5 - 1 < (t + 1) * den
    with pytest.raises(R.ReferencePanics):
        R.difficulty_target([0] * 5)
    assert R.difficulty_new([6000, 0, 0, 0, 0]) == MINIMUM and R.difficulty_new([17, 0, 0, 0, 0]) == MINIMUM
    assert R.difficulty_new([6001, 0, 0, 0, 0]) == [6001, 0, 0, 0, 0] and R.difficulty_new([0, 1, 0, 0, 0]) == [0, 1, 0, 0, 0]


def _lib():
    import neptune_hip._lib as L
    return L, L.load()


def test_abi_declares_the_chain_entry_points():
    L, lib = _lib()
    for name, argc in (("nhip_blk_header", 7), ("nhip_difficulty_target", 2), ("nhip_difficulty_control", 6),
                       ("nhip_blk_digests", 8), ("nhip_blk_chain_check", 10)):
        assert len(L.SIGNATURES[name][0]) == argc and hasattr(lib, name)
    assert lib.nhip_abi_version() >= 2700
    assert ctypes.sizeof(L.ChainParams) == 72 and ctypes.sizeof(L.PowMastPaths) == 240


def test_difficulty_target_matches_the_restatement():
    _, lib = _lib()
    g = random.Random(14)
    for d in _difficulties(g, 200):
        lim, out = np.array(d, dtype=np.uint32), np.zeros(5, dtype=np.uint64)
        rc = lib.nhip_difficulty_target(lim.ctypes.data, out.ctypes.data)
        if not any(d):
            assert rc == L_ERR_ARG
            continue
        assert rc == 0 and tuple(int(x) for x in out) == R.difficulty_target(d), d
    zero = np.zeros(5, dtype=np.uint32)
    assert lib.nhip_difficulty_target(zero.ctypes.data, np.zeros(5, dtype=np.uint64).ctypes.data) == L_ERR_ARG


L_ERR_ARG = 4


def _control_cases(g, n):
    target, minimum = 588_000, 60_000
    t0 = 1_754_420_400_000
    cases = []
    for d in DIFFICULTY_EDGES:
        if not any(d):
            continue
        cases += [(t0 + target, t0, d, target, 0),                 # a genesis parent
                  (t0 + minimum, t0, d, target, 7),                 # a block time of the minimum
                  (t0 + target, t0, d, target, 7),                  # exactly the target
                  (t0 + 5 * target, t0, d, target, 7),              # 5 x the target
                  (t0 + 1000 * target, t0, d, target, 7),           # 1000 x the target
                  (t0, t0 + 1, d, target, 7),                       # the field difference wraps to p - 1
                  (3, P - 5, d, target, 7),                         # wraps to a small positive difference
                  (t0 + 1, t0, d, 1, 7), (t0 + 100, t0, d, 100, 1), (t0 + 99, t0, d, 100, 1),
                  (t0 + 7, t0, d, (1 << 32) + 1, 2), (t0 + 7, t0, d, P - 1, 2)]
    for _ in range(n):
        d = [g.getrandbits(g.choice([1, 13, 32])) for _ in range(5)]
        interval = g.choice([100, 588_000, g.randrange(1, 1 << 33), g.randrange(1, P)])
        old = g.randrange(P)
        new = g.choice([(old + g.randrange(10 * interval)) % P, g.randrange(P)])
        cases.append((new, old, d, interval, g.choice([0, 1, g.getrandbits(20)])))
    return cases


def test_difficulty_control_matches_the_restatement():
    _, lib = _lib()
    g = random.Random(15)
    seen = set()
    for new, old, d, interval, height in _control_cases(g, 200):
        lim, out = np.array(d, dtype=np.uint32), np.zeros(5, dtype=np.uint32)
        assert lib.nhip_difficulty_control(new, old, lim.ctypes.data, interval, height, out.ctypes.data) == 0
        want = R.difficulty_control(new, old, d, interval, height)
        assert [int(x) for x in out] == want, (new, old, d, interval, height)
        seen.add("max" if want == MAXIMUM else "min" if want == MINIMUM else "same" if want == list(d) else "other")
    assert seen == {"max", "min", "same", "other"}
    assert lib.nhip_difficulty_control(1, 0, np.array(MINIMUM, dtype=np.uint32).ctypes.data, 0, 3,
                                       np.zeros(5, dtype=np.uint32).ctypes.data) == L_ERR_ARG


def test_python_mirror_of_the_host_exports():
    from neptune_hip import blocks as NB
    import neptune_hip._lib as L
    assert NB.difficulty_target(MINIMUM) == R.difficulty_target(MINIMUM)
    assert NB.difficulty_control(1_000_700, 1_000_000, [70_000, 0, 0, 0, 0], 100, 4) == \
        R.difficulty_control(1_000_700, 1_000_000, [70_000, 0, 0, 0, 0], 100, 4)
    with pytest.raises(L.NhipError):
        NB.difficulty_target([0] * 5)
    from neptune_hip.verifier import Network
    p = NB.chain_params(Network.REGTEST, 123)
    assert (p.minimum_block_time_ms, p.target_block_interval_ms, p.allows_mock_pow, p.now_ms) == (1, 100, 1, 123)
    assert list(p.genesis_difficulty) == MINIMUM and p.hardfork_alpha_height == 0
    p = NB.chain_params(Network.MAIN, 5, pow_tree_height=10)
    assert (p.minimum_block_time_ms, p.target_block_interval_ms, p.difficulty_reset_interval_ms) == (60_000, 588_000, 0)
    assert list(p.genesis_difficulty) == [100_000_000, 0, 0, 0, 0] and p.hardfork_alpha_height == 15_000
    assert NB.chain_params(Network.TESTNET_MOCK, 5).difficulty_reset_interval_ms == 2 * 588_000
    assert NB.chain_params(Network.TESTNET, 5).hardfork_alpha_height == 120 and p.pow_tree_height == 10


def test_pow_add_and_reset_restatement_edges():
    assert R.pow_add([0xFFFFFFFF] * 6, [1, 0, 0, 0, 0]) == [0] * 6                # wraps
    assert R.pow_add([0xFFFFFFFF, 0, 0, 0, 0, 7], [1, 0, 0, 0, 0xFFFFFFFF]) == [0, 1, 0, 0, 0xFFFFFFFF, 7]
    p = R.Params(difficulty_reset_interval=1000)
    assert R.should_reset_difficulty(p, 2000, 1000) and not R.should_reset_difficulty(p, 1999, 1000)
    assert R.should_reset_difficulty(p, 5, 10)                                    # the difference wraps: huge
    assert not R.should_reset_difficulty(R.Params(), 1 << 40, 0)


def test_blk_header_matches_the_restatement():
    L, lib = _lib()
    g = random.Random(16)
    blocks = [_block(g) for _ in range(200)]
    blocks[3]["body"]["block_mmr_accumulator"] = {"leaf_count": (1 << 64) - 1, "peaks": [B._rd(g) for _ in range(64)]}
    blocks[4]["body"]["block_mmr_accumulator"] = {"leaf_count": 5, "peaks": [B._rd(g) for _ in range(70)]}
    blocks[5]["proof_kind"], blocks[5]["proof"] = B.SINGLE_PROOF, [P - 1, 0, 1]
    data = b"".join(B.encode_block(b) for b in blocks)
    a = np.frombuffer(data, dtype=np.uint8)
    count = ctypes.c_size_t(0)
    scanned = (L.BlkBlock * len(blocks))()
    assert lib.nhip_blk_scan(a.ctypes.data, len(data), H, ctypes.cast(scanned, ctypes.c_void_p), len(blocks),
                             ctypes.byref(count)) == 0 and count.value == len(blocks)
    kinds = set()
    for b, s in zip(blocks, scanned):
        out = L.BlkHeader()
        assert lib.nhip_blk_header(a.ctypes.data, len(data), H, ctypes.byref(s), ctypes.byref(out), None, 0) == 0
        nw = int(out.appendix_words + out.prefix_words)
        words = np.zeros(nw, dtype=np.uint64)
        assert lib.nhip_blk_header(a.ctypes.data, len(data), H, ctypes.byref(s), ctypes.byref(out), words.ctypes.data,
                                   nw - 1) == L_ERR_ARG
        assert lib.nhip_blk_header(a.ctypes.data, len(data), H, ctypes.byref(s), ctypes.byref(out), words.ctypes.data,
                                   nw) == 0
        h = b["header"]
        assert (out.version, out.height, out.timestamp) == (h["version"], h["height"], h["timestamp"])
        for name, got in (("prev_block_digest", out.prev_block_digest), ("pow_root", out.pow_root),
                          ("nonce", out.pow_nonce), ("receiver_digest", out.receiver_digest),
                          ("lock_script_hash", out.lock_script_hash), ("difficulty", out.difficulty),
                          ("cumulative_proof_of_work", out.cumulative_proof_of_work)):
            assert [int(x) for x in got] == [int(x) for x in h[name]], name
        for name, off in (("path_a", out.path_a_offset), ("path_b", out.path_b_offset)):
            got = np.frombuffer(data, dtype="<u8", count=5 * H, offset=int(off))
            assert [int(x) for x in got] == [x for d in h[name] for x in d], name
        mm = b["body"]["block_mmr_accumulator"]
        assert out.mmr_num_leafs == mm["leaf_count"] and out.mmr_n_peaks == min(len(mm["peaks"]), 65)
        assert [[int(x) for x in pk] for pk in out.mmr_peaks[:min(len(mm["peaks"]), 64)]] == mm["peaks"][:64]
        app = R.appendix_encoding(b["appendix"])
        n_proof = len(b["proof"]) if b["proof_kind"] == B.SINGLE_PROOF else 0
        assert [int(x) for x in words] == app + R.proof_prefix(b["proof_kind"], n_proof)
        assert out.appendix_words == len(app)
        if b["proof_kind"] == B.SINGLE_PROOF:
            assert (out.proof_offset, out.proof_len) == (s.proof_offset, s.proof_len) and out.proof_len == n_proof
            got = np.frombuffer(data, dtype="<u8", count=n_proof, offset=int(out.proof_offset))
            assert R.proof_encoding(b["proof_kind"], b["proof"])[4:] == [int(x) % P for x in got]
        kinds.add(b["proof_kind"])
    assert kinds == {B.GENESIS, B.INVALID, B.SINGLE_PROOF}
    # a truncated block is a decode error, a block outside the buffer an argument error
    out = L.BlkHeader()
    assert lib.nhip_blk_header(a.ctypes.data, int(scanned[0].size) - 1, H, ctypes.byref(scanned[0]), ctypes.byref(out),
                               None, 0) == 5
    assert lib.nhip_blk_header(a.ctypes.data, 10, H, ctypes.byref(scanned[1]), ctypes.byref(out), None, 0) == L_ERR_ARG
