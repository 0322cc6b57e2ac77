"""CPU side of the table-shape tests (table_shapes_cases.py): the shape list hits every property the
kernels branch on, and for every shape the Python oracle and the C oracle agree on the accepting
proofs and on every mutant, none of which the oracle accepts: the fixtures are right before a GPU
sees them.  The synthetic AIR generator at its smallest shapes, which once did not return."""
import numpy as np
import pytest

import stark_ref as S
import table_shapes_cases as TS


def test_shape_list_covers_every_property():
    TS.assert_coverage(TS.SHAPES)
    assert len(set(TS.SHAPES)) == len(TS.SHAPES)


def test_coverage_predicate_names_what_is_missing():
    """The predicate is not vacuous: the two shapes the suite had before miss most properties, the
    list without its wide shapes or without its Q = 64 shape has gaps, and a shape outside dims_from's
    range is named."""
    gaps = TS.coverage_gaps([(24, 9, 4), (379, 88, 4)])
    for what in ("a width with % 10 == 0", "a width with % 10 == 1", "a width below 10", "Q == 1", f"Q == {TS.Q_MAX}",
                 "M % 8 == 1", "3A % 8 == 1", "M on a multiple of 8 * DEEP_UNROLL"):
        assert what in gaps, what
    assert any(g.startswith("a wide shape") for g in gaps)
    assert TS.coverage_gaps(TS.SHAPES[:-2]) and TS.coverage_gaps([s for s in TS.SHAPES if s[2] != TS.Q_MAX])
    with pytest.raises(AssertionError):
        TS.assert_coverage(TS.SHAPES + [(2018, 10, 4)])  # M + 3A = 2048: outside dims_from's range


@pytest.mark.parametrize("shape", TS.SHAPES, ids=TS.IDS)
def test_oracles_agree_on_proofs_and_mutants(shape):
    import coracle as C
    c = TS.case(shape)
    names = [name for name, _, _ in c.mutants]
    assert len(names) == (6 if shape[0] >= 10 else 5), names
    # the Python oracle rejects every mutant, in the phase of the word that was changed
    for (name, _, phase), err in zip(c.mutants, c.mutant_errors):
        assert err is not None and TS.PHASE.get(err) == phase, (name, err)
    claims = c.claims + [c.claims[0]] * len(c.mutants)
    proofs = c.proofs + [w for _, w, _ in c.mutants]
    got = C.stark_verify_batch(c.air_words, c.params, claims, proofs, threads=4)
    assert [int(v) for v in got] == [1] * len(c.proofs) + [0] * len(c.mutants)
    # three distinct proofs, distinct transcripts
    assert len({p.tobytes() for p in c.proofs}) == 3 and len({tuple(w[1]) for w in c.want}) == 3
    for samples, indices in c.want:
        k, (M, A, Q) = c.params.num_collinearity_checks, shape
        assert len(indices) == k == 80
        # challenges, quotient weights, z, the M + A + Q + 3 weights, the FRI alphas, the last point
        assert len(samples) >= 59 + c.air.num_constraints + 1 + M + A + Q + 3 + 1


def test_synth_air_smallest_shapes():
    """synth_air's combination loop drew constraint types for ever when no two base constraints
    shared one (M = 7, A = 1: three targets); it now stops at the base constraints.  M = 5, A = 1 is
    the smallest shape (no main target at all); below it the generator raises at once."""
    import stark_prover_fast as SP
    for (M, A, Q), seed in (((7, 1, 3), 1), ((7, 1, 3), 0x5EED), ((5, 1, 1), 1), ((6, 2, 2), 3)):
        params = S.StarkParams(num_main=M, num_aux=A, num_quotient_segments=Q)
        air, recipe = S.synth_air(params, seed=seed)
        assert air.num_constraints >= len(recipe.targets) == (M - 1 - 4) + A
        claim = TS.CLAIMS[0]
        proof, _ = SP.prove(params, air, recipe, claim, TS.LOG2_HEIGHT, seed=seed)
        assert S.verify(params, air, claim, [int(w) for w in proof])
    # a type pair exists: the requested count is reached as before
    air, recipe = S.synth_air(S.StarkParams(num_main=24, num_aux=9), seed=7)
    assert air.num_constraints == int(1.6 * len(recipe.targets)) and recipe.combos
    # no pair and an explicit count that needs combinations: an error, not a loop
    params = S.StarkParams(num_main=5, num_aux=1, num_quotient_segments=1)
    assert S.synth_air(params, seed=1, num_constraints=1)[0].num_constraints == 1
    with pytest.raises(ValueError):
        S.synth_air(params, seed=1, num_constraints=2)
    for M, A in ((4, 1), (0, 3), (8, 0)):
        with pytest.raises(ValueError):
            S.synth_air(S.StarkParams(num_main=M, num_aux=A), seed=1)


def _decodes(NS, shape_params, air_shape):
    """nhip_proof_decodes of a (7, 1, 3) proof's words under `shape_params` with the AIR of
    `air_shape`: True / False, or NhipError for refused arguments."""
    M, A, Q = shape_params
    air, _ = S.synth_air(S.StarkParams(num_main=air_shape[0], num_aux=air_shape[1]), seed=1)
    c = TS.case((7, 1, 3))
    return NS.proof_decodes(NS.Air(air.to_words()), NS.Stark(160, 2, 80, M, A, Q), NS.Claim(*c.claims[0]), c.proofs[0])


def test_dims_from_limits():
    """dims_from (air_host.cpp) through nhip_proof_decodes: M + 3A = 2047 is taken and 2048 refused
    (DEEP_ROW_WORDS_MAX), Q = 0 and Q = 65 are refused, and so are column counts other than the AIR's.
    A refusal is NHIP_ERR_ARG (NhipError); a shape that is taken decodes (True for the shape's own
    proof, False for another shape's words)."""
    import neptune_hip.stark as NS
    from neptune_hip import NhipError
    assert _decodes(NS, (7, 1, 3), (7, 1)) is True
    for M, A in ((2017, 10), (19, 676), (10, 679)):
        assert M + 3 * A == 2047
        assert _decodes(NS, (M, A, 4), (M, A)) is False  # taken; the words are another shape's
    for M, A in ((2018, 10), (20, 676), (8, 680), (2048, 1)):
        assert M + 3 * A >= 2048
        with pytest.raises(NhipError):
            _decodes(NS, (M, A, 4), (M, A))
    for Q in (0, 65):
        with pytest.raises(NhipError):
            _decodes(NS, (7, 1, Q), (7, 1))
    assert _decodes(NS, (7, 1, 64), (7, 1)) is False and _decodes(NS, (7, 1, 1), (7, 1)) is False
    for M, A in ((8, 1), (7, 2), (6, 1)):
        with pytest.raises(NhipError):
            _decodes(NS, (M, A, 3), (7, 1))
