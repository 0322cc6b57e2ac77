"""The work k_fri, k_deep_rows8 and k_ood_air do beside their products, against the oracle: the
two-adic root tables (FRI's g^(2^q) and w^(2^q), DEEP's z w, the OOD zerofier's 1 / w), the check
lanes' 1 / x as a power of the domain generator, the last codeword's barycentric sum with several
points per lane behind one inversion, and DEEP's quotient-segment combination taken after the row
passes.

The five pool proofs (log2 heights 9, 10, 11, 12, 16: every FRI depth the config-4 workload has, last
codewords of 512 points) in batches of 1, 5 and 65 (one proof past the 64-proof boundary of the fused
small-batch kernels and the 1,024-thread OOD kernel) in both input forms: verdicts, fail words and
Fiat-Shamir transcripts equal the oracle's.  The height-23 deep-FRI proof alone (fused plan + FRI
launch, 16 folding rounds).  Mutants of the height-9 and height-16 proofs reject in the oracle's fail
phase: a quotient-segment word of the first, the 33rd and the last revealed row (the 32-row passes of
k_deep_rows8), a last-codeword word at index 0 and L - 1 (first and last lane of the barycentric
chain), a last-polynomial coefficient.  One parameter set with 53 checks (not a multiple of 32)."""
import json
import os

import numpy as np
import pytest

import stark_ref as S
import tip5_ref as T

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")

FAIL_MERKLE_QUOT = 1 << 4
FAIL_FRI_LAST_ROOT = 1 << 6
FAIL_FRI_LAST_AGREE = 1 << 7
FAIL_FRI_DEGREE = 1 << 8
FAIL_FRI_EVAL = 1 << 9
FAIL_DEEP = 1 << 10
# the oracle's first error (stark_ref._verify / fri_verify) -> the fail bit of that phase (stark.hpp)
PHASE = {
    "quotient codeword authentication failure": FAIL_MERKLE_QUOT,
    "FRI: bad Merkle root for last codeword": FAIL_FRI_LAST_ROOT,
    "FRI: last codeword mismatch": FAIL_FRI_LAST_AGREE,
    "FRI: last polynomial degree too high": FAIL_FRI_DEGREE,
    "FRI: last polynomial evaluation mismatch": FAIL_FRI_EVAL,
    "combination codeword mismatch": FAIL_DEEP,
}


def _oracle(params, air, claim, proof):
    """(accepted, first error, samples, indices) of the oracle verifier."""
    tr = {}
    try:
        S._verify(params, air, claim, [int(w) for w in proof], tr)
    except S.VerifyError as e:
        return False, str(e), None, None
    samples = [tuple(x) for tag, vals in tr["sponge_samples"] if tag != "fri_indices" for x in vals]
    indices = [v for tag, vals in tr["sponge_samples"] if tag == "fri_indices" for v in vals]
    return True, None, samples, indices


def _bump(x, c):
    y = list(x)
    y[c] = (y[c] + 1) % S.P
    return tuple(y)


def _mutants(proof, params):
    """[(name, words, fail bits the change must set beside the oracle's phase)] of one proof."""
    items = S.decode_proof([int(w) for w in proof], params)
    assert S.encode_proof(items, params) == [int(w) for w in proof]
    kinds = [k for k, _ in items]

    def changed(kind, edit):
        out = [(k, pl) for k, pl in items]
        i = kinds.index(kind)
        out[i] = (kind, edit(out[i][1]))
        return np.array(S.encode_proof(out, params), dtype=np.uint64)

    muts = []
    k = params.num_collinearity_checks
    for row in sorted({0, min(32, k - 1), k - 1}):
        def edit(rows, row=row):
            rows = [list(r) for r in rows]
            q = row % len(rows[row])
            rows[row][q] = _bump(rows[row][q], row % 3)
            return rows
        muts.append((f"quotient row {row}", changed(S.QUOT_SEGMENTS_ELEMENTS, edit), FAIL_DEEP))
    L = len(items[kinds.index(S.FRI_CODEWORD)][1])
    for i in (0, L - 1):
        def edit(cw, i=i):
            cw = list(cw)
            cw[i] = _bump(cw[i], i % 3)
            return cw
        muts.append((f"last codeword {i}", changed(S.FRI_CODEWORD, edit), FAIL_FRI_EVAL))

    def edit(poly):
        poly = list(poly)
        poly[len(poly) // 2] = _bump(poly[len(poly) // 2], 1)
        return poly
    muts.append(("last polynomial", changed(S.FRI_POLYNOMIAL, edit), FAIL_FRI_EVAL))
    return muts


@pytest.fixture(scope="module")
def pool():
    T.use_c_backend()
    z = np.load(os.path.join(GOLDEN, "c3_pool.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    air = S.AirCircuit.from_words([int(w) for w in z["air"]])
    params = S.StarkParams()
    claims, proofs, want = [], [], []
    for h in meta["heights"]:
        c = meta["claims"][str(h)]
        claims.append((c["digest"], c["version"], c["input"], c["output"]))
        proofs.append(z[f"proof_{h}"].astype(np.uint64))
        ok, _, samples, indices = _oracle(params, air, claims[-1], proofs[-1])
        assert ok
        want.append((samples, indices))
    return [int(w) for w in z["air"]], air, params, meta["heights"], claims, proofs, want


def _batch(ctx, NS, air_words, stark, claims, proofs, montgomery):
    cl = [NS.Claim(*c) for c in claims]
    if montgomery:
        return NS.Batch(ctx, NS.Air(air_words), stark.montgomery(), [NS.montgomery_claim(c) for c in cl],
                        [NS.to_montgomery(p) for p in proofs])
    return NS.Batch(ctx, NS.Air(air_words), stark, cl, proofs)


@pytest.mark.parametrize("montgomery", [False, True], ids=["canonical", "montgomery"])
@pytest.mark.parametrize("n", [1, 5, 65])
def test_pool_proofs_in_small_and_two_stream_batches(ctx, pool, n, montgomery):
    import neptune_hip.stark as NS
    air_words, _, _, heights, claims, proofs, want = pool
    # one proof: the tallest (the deepest FRI); 65: the five heights 13 times over
    pick = [len(proofs) - 1] if n == 1 else [i % len(proofs) for i in range(n)]
    b = _batch(ctx, NS, air_words, NS.Stark.default(), [claims[i] for i in pick], [proofs[i] for i in pick], montgomery)
    v, ok = b.run()
    assert ok and all(bool(x) for x in v)
    for j, i in enumerate(pick):
        xs, idx, fail = b.transcript(j)
        assert fail == 0 and (xs, idx) == want[i], (j, heights[i])
    b.close()


def test_height_23_proof_alone(ctx):
    """deep_fri.npz's tallest proof as a batch of one: the fused plan + FRI launch and the 1,024-thread
    OOD kernel, 16 folding rounds, a 32-bit-wide domain index range."""
    import neptune_hip.stark as NS
    z = np.load(os.path.join(GOLDEN, "deep_fri.npz"))
    m = json.loads(bytes(z["meta"]).decode())["cases"]["23"]
    air_words = [int(w) for w in np.load(os.path.join(GOLDEN, "c3_pool.npz"))["air"]]
    b = NS.Batch(ctx, NS.Air(air_words), NS.Stark.default(),
                 [NS.Claim(m["digest"], m["version"], m["input"], m["output"])], [z["proof_23"]])
    v, ok = b.run()
    xs, idx, fail = b.transcript(0)
    assert ok and bool(v[0]) and fail == 0
    assert xs == [tuple(int(c) for c in x) for x in z["samples_23"]] and idx == [int(i) for i in z["indices_23"]]
    b.close()


@pytest.mark.parametrize("height", [9, 16])
def test_mutants_reject_in_the_oracles_phase(ctx, pool, height):
    import neptune_hip.stark as NS
    air_words, air, params, heights, claims, proofs, _ = pool
    i = heights.index(height)
    muts = _mutants(proofs[i], params)
    assert len(muts) == 6
    phases = []
    for name, words, _ in muts:
        ok, err, _, _ = _oracle(params, air, claims[i], words)
        assert not ok and err in PHASE, (name, err)
        phases.append(PHASE[err])
    for montgomery in (False, True):
        b = _batch(ctx, NS, air_words, NS.Stark.default(), [claims[i]] * (len(muts) + 1),
                   [proofs[i]] + [w for _, w, _ in muts], montgomery)
        v, ok = b.run()
        assert [bool(x) for x in v] == [True] + [False] * len(muts)
        assert b.transcript(0, max_xfe=1)[2] == 0
        for j, (name, _, also) in enumerate(muts):
            fail = b.transcript(j + 1, max_xfe=1)[2]
            # the oracle's phase and the phase the changed words enter as values; a changed last
            # codeword may also disagree with a folded value (an index on the changed point)
            assert fail & phases[j] and fail & also, (name, montgomery, fail)
            assert fail & ~(phases[j] | also | FAIL_FRI_LAST_AGREE) == 0, (name, montgomery, fail)
        b.close()


def test_53_checks(ctx):
    """Stark::new(160, 3): 53 collinearity checks (32 + 21: a part-filled second wave of check lanes,
    a part-filled second row pass), expansion 8.  The accepting proof's transcript equals the
    oracle's; a quotient-segment word of the first, the 33rd and the last row changed rejects."""
    import coracle as C
    import neptune_hip.stark as NS
    import stark_prover_fast as SP
    T.use_c_backend()
    params = S.StarkParams(security_level=160, log2_fri_expansion=3)
    k = params.num_collinearity_checks
    assert k == 53
    air, recipe = S.synth_air(params, seed=1)
    claim = ([2, 7, 1, 8, 2], 0, [8, 1], [8, 2, 8])
    proof, _ = SP.prove(params, air, recipe, claim, 4, seed=53)
    proof = np.array([int(w) for w in proof], dtype=np.uint64)
    ok, _, samples, indices = _oracle(params, air, claim, proof)
    assert ok
    muts = [w for name, w, _ in _mutants(proof, params) if name.startswith("quotient")]
    assert len(muts) == 3
    cases = [proof] + muts
    stark = NS.Stark(160, 3, k, params.num_main, params.num_aux, params.num_quotient_segments)
    b = NS.Batch(ctx, NS.Air(air.to_words()), stark, [NS.Claim(*claim)] * len(cases), cases)
    v, _ = b.run()
    xs, idx, fail = b.transcript(0)
    assert fail == 0 and xs == samples and idx == indices and len(idx) == k
    want = C.stark_verify_batch(air.to_words(), params, [claim] * len(cases), cases, threads=4)
    assert [bool(x) for x in v] == [bool(x) for x in want] == [True, False, False, False]
    for j in range(1, len(cases)):
        assert b.transcript(j, max_xfe=1)[2] & FAIL_DEEP, j
    b.close()
