"""k_ood_air's paths against the oracle: the segment-by-segment program loop, the batched zerofier
inversion and the wave-uniform terminal folds, in the 1,024-thread kernel (batches up to
OOD_WIDE_MAX_PROOFS = 64 proofs) and the 256-thread one (65 proofs, the first size past it), for the
synthetic AIR and its triton-air-sized bloat compiled at step widths 64, 512 and 1,024 and with the
LDS part of the slots capped (the global-slot path).  The five pool proofs accept with the oracle's
transcripts; each with one word of its OOD main row changed rejects in the OOD phase.  The derived
challenges (Challenges::new) fold claim inputs and outputs of 0, 1, 63, 64, 65 and 129 words, the
chunk boundaries of the terminal fold (n + 1 entries over up to 64 lanes)."""
import json
import os

import numpy as np
import pytest

import stark_ref as S
import tip5_ref as T

pytestmark = pytest.mark.gpu

FAIL_OOD = 1 << 1
WIDE_MAX = 64  # OOD_WIDE_MAX_PROOFS (stark_launch_plan.hpp)


def _transcript(params, air, claim, proof):
    tr = {}
    assert S.verify(params, air, claim, proof, tr)
    samples = [tuple(x) for tag, vals in tr["sponge_samples"] if tag != "fri_indices" for x in vals]
    indices = [v for tag, vals in tr["sponge_samples"] if tag == "fri_indices" for v in vals]
    return samples, indices


def _used_main_columns(air):
    """Main-row columns (current row) the constraints read, in column order."""
    reach, st = set(), [c for cs in air.constraints for c in cs]
    while st:
        i = st.pop()
        if i in reach:
            continue
        reach.add(i)
        op, a, b, _ = air.nodes[i]
        if op in (S.OP_ADD, S.OP_SUB, S.OP_MUL):
            st += [a, b]
    return sorted({air.nodes[i][2] for i in reach
                   if air.nodes[i][0] == S.OP_INPUT and air.nodes[i][1] == S.INPUT_MAIN_CURR})


@pytest.fixture(scope="module")
def pool():
    """The five pool proofs with the oracle's transcripts, and a copy of each with one word of its
    OOD main row (a column the constraints read) changed; the two AIRs."""
    T.use_c_backend()
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "c3_pool.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    syn = S.AirCircuit.from_words([int(w) for w in z["air"]])
    params = S.StarkParams()
    cols = _used_main_columns(syn)
    claims, proofs, flipped, want = [], [], [], []
    for k, h in enumerate(meta["heights"]):
        c = meta["claims"][str(h)]
        claim = (c["digest"], c["version"], c["input"], c["output"])
        proof = z[f"proof_{h}"].astype(np.uint64)
        plist = [int(w) for w in proof]
        want.append(_transcript(params, syn, claim, plist))
        items = S.decode_proof(plist, params)
        pos = 2
        for kind, _ in items:
            if kind == S.OOD_MAIN_ROW:
                break
            pos += 1 + plist[pos]
        col = cols[(k * len(cols)) // len(meta["heights"])]
        at = pos + 1 + 1 + 3 * col + k % 3  # the item's words: element count, then 3 words per column
        m = proof.copy()
        m[at] = np.uint64((int(m[at]) + 1) % S.P)
        claims.append(claim)
        proofs.append(proof)
        flipped.append(m)
    assert not any(S.verify(params, syn, claims[k], [int(w) for w in flipped[k]]) for k in (0, 1))
    return {"synthetic": syn, "triton-size": S.bloat_air(syn, 24000)}, claims, proofs, flipped, want


@pytest.mark.parametrize("name", ["synthetic", "triton-size"])
@pytest.mark.parametrize("width,lds_cap", [(64, 0), (512, 0), (1024, 0), (512, 600)])
def test_pool_proofs_accept_and_flipped_ood_rows_reject(ctx, pool, name, width, lds_cap):
    import neptune_hip.stark as NS
    airs, claims, proofs, flipped, want = pool
    gair = NS.Air(airs[name].to_words(), lds_slots=lds_cap, step_width=width)
    info = gair.info()
    assert (info["global_slots"] > 0) == bool(lds_cap), info
    n = len(proofs)
    for reps in (1, (WIDE_MAX + n) // n):  # 5 proofs: 1,024-thread kernel; 65: the 256-thread one
        good = NS.Batch(ctx, gair, NS.Stark.default(), [NS.Claim(*c) for c in claims] * reps, proofs * reps)
        assert (reps == 1 and n <= WIDE_MAX) or n * reps == WIDE_MAX + 1
        v, ok = good.run()
        assert ok and all(bool(x) for x in v)
        for i in list(range(n)) + list(range(n * (reps - 1), n * reps)):
            xs, idx, fail = good.transcript(i)
            assert fail == 0 and (xs, idx) == want[i % n], (reps, i)
        good.close()
        bad = NS.Batch(ctx, gair, NS.Stark.default(), [NS.Claim(*c) for c in claims] * reps, flipped * reps)
        v, ok = bad.run()
        assert not ok and not any(bool(x) for x in v)
        for i in range(n * reps):
            assert bad.transcript(i)[2] & FAIL_OOD, (reps, i)
        bad.close()


def test_derived_challenges_at_the_fold_boundaries(ctx):
    import neptune_hip.stark as NS
    import stark_prover_const as K
    T.use_c_backend()
    params = S.StarkParams()
    air, recipe = S.synth_air(params, seed=1)
    lens = (0, 1, 63, 64, 65, 129)
    rng = np.random.default_rng(0x7E12)
    claims, proofs, want = [], [], []
    for k, n_in in enumerate(lens):
        n_out = lens[len(lens) - 1 - k]  # every length once as the input's and once as the output's
        claim = ([8, k, 7, 7, 7], 0, [int(v) for v in rng.integers(0, S.P, size=n_in, dtype=np.uint64)],
                 [int(v) for v in rng.integers(0, S.P, size=n_out, dtype=np.uint64)])
        proof, _ = K.prove(params, air, recipe, claim, 8, seed=100 + k)
        claims.append(claim)
        proofs.append(proof)
        want.append(_transcript(params, air, claim, proof))
    gair = NS.Air(air.to_words())
    n = len(proofs)
    for reps in (1, (WIDE_MAX + n) // n):  # 6 proofs (1,024-thread kernel) and 66 (256-thread)
        b = NS.Batch(ctx, gair, NS.Stark.default(), [NS.Claim(*c) for c in claims] * reps, proofs * reps)
        v, ok = b.run()
        assert ok and all(bool(x) for x in v)
        for i in list(range(n)) + list(range(n * (reps - 1), n * reps)):
            xs, idx, fail = b.transcript(i)
            assert fail == 0 and (xs, idx) == want[i % n], (reps, i)
        b.close()
        # a claim with one input or output word changed: another terminal, the oracle rejects, so do we
        wrong = []
        for c in claims:
            c2 = [c[0], c[1], list(c[2]), list(c[3])]
            tgt = c2[2] if c2[2] else c2[3]
            tgt[len(tgt) // 2] = (tgt[len(tgt) // 2] + 1) % S.P
            wrong.append(tuple(c2))
        assert not S.verify(params, air, wrong[2], proofs[2])
        b = NS.Batch(ctx, gair, NS.Stark.default(), [NS.Claim(*c) for c in wrong] * reps, proofs * reps)
        v, ok = b.run()
        assert not ok and not any(bool(x) for x in v)
        b.close()
