"""The STARK kernels at table shapes other than 24 x 9 and 379 x 88 (table_shapes_cases.py: the shapes,
what each width selects in the kernels, and the predicate that the list hits all of it), against the
oracle, never against another GPU run.  Per shape:

  * accepting proofs in every launch form of a small batch, verdict 1, fail word 0 and every squeezed
    sample and FRI index equal to stark_ref._verify's (the Fiat-Shamir absorbs, the row hashes through
    the Merkle roots, OOD and DEEP, exactly):
      3 proofs on one stream   k_fs_rows_small (pair replay + 16-lane rows fused), k_mp_climb,
                               k_plan_fri_small, k_ood_air<1024>
      3 proofs on two streams  k_fs_replay_wide (pair), k_hash_rows_wide, k_ood_air<1024>
      33 proofs                past ROWS_WIDE_MAX_PROOFS / MP_CLIMB_MAX_PROOFS: the lane-form
                               k_hash_rows, per-level Merkle hashing and the tail
      65 proofs                past OOD_WIDE_MAX_PROOFS: k_ood_air<256>
    in canonical and Montgomery input form at 3 and 33 proofs;
  * the three Fiat-Shamir replay forms (row, pair, quad) forced on the 33-proof batch.  The form is
    read at each launch; a captured graph keeps the form it was captured with, so no graph batch here;
  * mutants of one word (revealed rows, OOD items): the verdicts of the Python and the C oracle, the
    fail bit of the oracle's first failing phase, and for a revealed-row word nothing beside its
    tree's FAIL_MERKLE_* bit and FAIL_DEEP."""
import pytest

import table_shapes_cases as TS

pytestmark = pytest.mark.gpu

TS.assert_coverage(TS.SHAPES)  # on the CPU, at collection: before any GPU run

ROWS_WIDE_MAX_PROOFS = 32  # = MP_CLIMB_MAX_PROOFS (stark_launch_plan.hpp)
OOD_WIDE_MAX_PROOFS = 64   # stark_launch_plan.hpp
FS_FORMS = {"row": 0, "pair": 1, "quad": 2}  # FsForm (stark_launch_plan.hpp)


@pytest.fixture(scope="module")
def fs_form():
    import neptune_hip.stark as NS
    yield NS.set_fs_form
    NS.set_fs_form(-1)


def _run_accepting(ctx, c, n, streams, montgomery):
    """A batch of n proofs (the shape's three distinct ones, repeated) accepts with the oracle's
    transcripts; checked on the first and the last three proofs."""
    import neptune_hip.stark as NS
    M, A, Q = c.shape
    stark = NS.Stark(160, 2, 80, M, A, Q)
    pick = [i % len(c.proofs) for i in range(n)]
    claims = [NS.Claim(*c.claims[i]) for i in pick]
    proofs = [c.proofs[i] for i in pick]
    if montgomery:
        stark = stark.montgomery()
        mont = [NS.to_montgomery(p) for p in c.proofs]
        claims, proofs = [NS.montgomery_claim(cl) for cl in claims], [mont[i] for i in pick]
    b = NS.Batch(ctx, NS.Air(c.air_words), stark, claims, proofs).set_streams(streams)
    try:
        v, ok = b.run()
        assert ok and [int(x) for x in v] == [1] * n, (c.shape, n, streams, montgomery, [int(x) for x in v])
        for j in sorted(set(list(range(min(3, n))) + list(range(max(0, n - 3), n)))):
            xs, idx, fail = b.transcript(j)
            assert fail == 0, (c.shape, n, streams, montgomery, j, fail)
            assert xs == c.want[pick[j]][0], (c.shape, n, streams, montgomery, j, "samples")
            assert idx == c.want[pick[j]][1], (c.shape, n, streams, montgomery, j, "indices")
    finally:
        b.close()


@pytest.mark.parametrize("n,streams", [(3, 1), (3, 2), (ROWS_WIDE_MAX_PROOFS + 1, 2), (OOD_WIDE_MAX_PROOFS + 1, 2)],
                         ids=["3-one-stream", "3-two-streams", "33", "65"])
@pytest.mark.parametrize("shape", TS.SHAPES, ids=TS.IDS)
def test_accepting_proofs_in_every_launch_form(ctx, shape, n, streams):
    c = TS.case(shape)
    _run_accepting(ctx, c, n, streams, False)
    if n <= ROWS_WIDE_MAX_PROOFS + 1:
        _run_accepting(ctx, c, n, streams, True)


@pytest.mark.parametrize("form", list(FS_FORMS))
@pytest.mark.parametrize("shape", TS.SHAPES, ids=TS.IDS)
def test_fiat_shamir_forms(ctx, fs_form, shape, form):
    c = TS.case(shape)
    fs_form(FS_FORMS[form])
    try:
        _run_accepting(ctx, c, ROWS_WIDE_MAX_PROOFS + 1, 2, False)
    finally:
        fs_form(-1)


@pytest.mark.parametrize("shape", TS.SHAPES, ids=TS.IDS)
def test_mutants_reject_in_the_oracles_phase(ctx, shape):
    import coracle as C
    import neptune_hip.stark as NS
    c = TS.case(shape)
    M, A, Q = shape
    phases = []
    for (name, _, phase), err in zip(c.mutants, c.mutant_errors):
        assert err in TS.PHASE and TS.PHASE[err] == phase, (name, err)  # no mutant the oracle accepts
        phases.append(phase)
    cases = [c.proofs[0]] + [w for _, w, _ in c.mutants]
    claims = [c.claims[0]] * len(cases)
    want = C.stark_verify_batch(c.air_words, c.params, claims, cases, threads=4)
    assert [int(x) for x in want] == [1] + [0] * len(c.mutants)
    for montgomery in (False, True):
        stark = NS.Stark(160, 2, 80, M, A, Q)
        gclaims, gcases = [NS.Claim(*cl) for cl in claims], cases
        if montgomery:
            stark = stark.montgomery()
            gclaims, gcases = [NS.montgomery_claim(cl) for cl in gclaims], [NS.to_montgomery(p) for p in cases]
        b = NS.Batch(ctx, NS.Air(c.air_words), stark, gclaims, gcases)
        try:
            v, ok = b.run()
            assert not ok and [int(x) for x in v] == [int(x) for x in want], (shape, montgomery, [int(x) for x in v])
            assert b.transcript(0, max_xfe=1)[2] == 0
            for j, (name, _, phase) in enumerate(c.mutants):
                fail = b.transcript(j + 1, max_xfe=1)[2]
                assert fail & phase, (shape, montgomery, name, fail)
                if phase in (TS.FAIL_MERKLE_MAIN, TS.FAIL_MERKLE_AUX, TS.FAIL_MERKLE_QUOT):
                    assert fail & ~(phase | TS.FAIL_DEEP) == 0, (shape, montgomery, name, fail)
        finally:
            b.close()


def test_batch_prepare_refuses_shapes_outside_the_range(ctx):
    """nhip_batch_prepare with M + 3A = 2048, Q = 0, Q = 65 or another column count than the AIR's:
    NHIP_ERR_ARG before anything is staged."""
    import neptune_hip.stark as NS
    import stark_ref as S
    from neptune_hip import NhipError
    c = TS.case((7, 1, 3))
    claims, proofs = [NS.Claim(*c.claims[0])], [c.proofs[0]]
    wide, _ = S.synth_air(S.StarkParams(num_main=2018, num_aux=10), seed=1)
    for air_words, shape in ((wide.to_words(), (2018, 10, 4)), (c.air_words, (7, 1, 0)), (c.air_words, (7, 1, 65)),
                             (c.air_words, (8, 1, 3)), (c.air_words, (7, 2, 3))):
        with pytest.raises(NhipError):
            NS.Batch(ctx, NS.Air(air_words), NS.Stark(160, 2, 80, *shape), claims, proofs)
