"""The Merkle multiproof path at chosen index patterns, values of k and authentication-structure
lengths (merkle_index_cases.py: the configurations, the patterns and the predicate that the pinned
proofs reach all of them), against the oracle, never against another GPU run.  Per configuration:

  * accepting proofs, a batch cycling through the configuration's heights (trees with and without
    b-tree groups, short last codewords beside long ones), in every launch form of the path; which
    kernels run is read from plan_launch (MI.hash_steps restates its hash schedule) and pinned by
    stats()["mp_hash_kernel_launches"]:
      3 proofs on one stream    the plan fused in k_plan_fri_small (256 threads whatever k), k_mp_climb
      3 proofs on two streams   k_mp_plan<128> (k <= 128) or k_mp_plan<256>, k_mp_climb
      33 proofs                 per-level k_mp_hash_wide (k = 256: levels 0 and 1 k_mp_hash), then
                                k_mp_hash_tail
      33, climb-from forced     k_mp_hash_wide levels hand over to k_mp_climb from a level above 0
      33, climb-from 0          per-level launches, never a hand-over
      k = 256, 50 or so         level 0's multiproof ops past MP_WIDE_MAX_OPS: the lane-form k_mp_hash (7 waves)
    in canonical and Montgomery input form at 3 and 33 proofs.  Verdict 1, fail word 0 and every sample
    and index equal to the oracle's on the first and the last three proofs, and tip5_perms_merkle
    equal to the sum of MI.merkle_ops over the batch: a plan that hashes a duplicate twice or does not
    merge a sibling pair still reaches the root, only the count shows it;
  * mutant batches, the accepting proof first: at most 32 proofs (k_mp_climb skips the MPS_NONE ops)
    and 33 or more (k_mp_hash_wide and k_mp_hash_tail skip them), in both input forms.  The verdicts
    are the C oracle's; every mutant's fail word holds the bit of the oracle's first error and nothing
    outside Mutant.allowed (for a length, order or digest mutant: that tree's bit alone, so the other
    three trees of the shared plan pass); the batch's tip5_perms_merkle is below the unmutated
    batch's, since the ops of a tree whose structure ran out are skipped and counted out."""
import pytest

import merkle_index_cases as MI

pytestmark = pytest.mark.gpu

MI.assert_coverage()  # on the CPU, at collection: before any GPU run

N_SMALL = 3
N_LEVELS = MI.MP_CLIMB_MAX_PROOFS + 1


@pytest.fixture(scope="module")
def climb_from():
    import neptune_hip._lib as L
    lib = L.load()

    def set_ops(ops):
        assert lib.nhip_set_climb_from_ops(int(ops)) == 0

    yield set_ops
    set_ops(-1)


def _stark(NS, c):
    M, A, Q = MI.SHAPE
    return NS.Stark(c.sec, c.log2_exp, c.k, M, A, Q)


def _batch(ctx, c, claims, proofs, montgomery, streams=2):
    import neptune_hip.stark as NS
    stark = _stark(NS, c)
    claims = [NS.Claim(*cl) for cl in claims]
    if montgomery:
        stark = stark.montgomery()
        claims, proofs = [NS.montgomery_claim(cl) for cl in claims], [NS.to_montgomery(p) for p in proofs]
    return NS.Batch(ctx, NS.Air(c.air_words), stark, claims, proofs).set_streams(streams)


def _run_accepting(ctx, c, n, streams, montgomery, steps):
    """A batch of n proofs (the configuration's, in turn) accepts with the oracle's transcripts, hashes
    as many pairs as the oracle does and launches the planned hash kernels."""
    pick = [i % len(c.proofs) for i in range(n)]
    b = _batch(ctx, c, [c.claims[i] for i in pick], [c.proofs[i] for i in pick], montgomery, streams)
    what = (c.name, n, streams, montgomery)
    try:
        v, ok = b.run()
        assert ok and [int(x) for x in v] == [1] * n, (what, [int(x) for x in v])
        for j in sorted(set(list(range(min(3, n))) + list(range(max(0, n - 3), n)))):
            xs, idx, fail = b.transcript(j)
            assert fail == 0, (what, j, fail)
            assert xs == c.want[pick[j]][0], (what, j, "samples")
            assert idx == c.want[pick[j]][1], (what, j, "indices")
        s = b.stats()
        print(what, "tip5_perms_merkle", s["tip5_perms_merkle"], "reference", sum(c.ops[i] for i in pick),
              "launches", s["mp_hash_kernel_launches"], steps)
        assert s["tip5_perms_merkle"] == sum(c.ops[i] for i in pick), what
        assert s["mp_hash_kernel_launches"] == len(steps), (what, steps)
    finally:
        b.close()


@pytest.mark.parametrize("n,streams", [(N_SMALL, 1), (N_SMALL, 2), (N_LEVELS, 2)],
                         ids=["3-one-stream", "3-two-streams", "33"])
@pytest.mark.parametrize("name", MI.NAMES)
def test_accepting_proofs_in_every_launch_form(ctx, name, n, streams):
    c = MI.case(name)
    steps = MI.hash_steps(c.k, [c.shapes[i % len(c.proofs)] for i in range(n)])
    kinds = [kd for kd, _ in steps]
    if n == N_SMALL:
        assert kinds == ["climb"]
    else:  # k = 256: the capacity of 33 proofs puts levels 0 and 1 past MP_WIDE_MAX_OPS already
        assert kinds[-1] == "tail" and set(kinds[:-1]) == ({"wide"} if c.k < 256 else {"level7", "wide"})
    for montgomery in (False, True):
        _run_accepting(ctx, c, n, streams, montgomery, steps)


@pytest.mark.parametrize("mode", ["forced", "never"])
@pytest.mark.parametrize("name", MI.NAMES)
def test_climb_from_a_level_above_zero(ctx, climb_from, name, mode):
    c = MI.case(name)
    shapes = [c.shapes[i % len(c.proofs)] for i in range(N_LEVELS)]
    ops = MI.climb_from_for(c.k, shapes) if mode == "forced" else 0
    steps = MI.hash_steps(c.k, shapes, ops)
    if mode == "forced":
        assert steps[-1][0] == "climb" and steps[-1][1] > 0
    else:
        assert steps == MI.hash_steps(c.k, shapes) and steps[-1][0] == "tail"
    climb_from(ops)
    try:
        _run_accepting(ctx, c, N_LEVELS, 2, False, steps)
    finally:
        climb_from(-1)


def test_lane_form_level_of_the_256_check_set(ctx):
    """k = 256, a batch whose level 0 holds more than MP_WIDE_MAX_OPS hash ops by the reference count
    (plan_launch sizes the level by its capacity, which is no smaller): the 7-wave k_mp_hash."""
    c = MI.case("k256")
    n = MI.lane_form_batch(c)
    pick = [i % len(c.proofs) for i in range(n)]
    assert sum(c.level_ops(i, 0, lcw=False) for i in pick) > MI.MP_WIDE_MAX_OPS
    steps = MI.hash_steps(c.k, [c.shapes[i] for i in pick])
    assert steps[0] == ("level7", 0)
    _run_accepting(ctx, c, n, 2, False, steps)


def _run_mutants(ctx, c, muts, n, montgomery, want_all):
    """The accepting proof, the mutants, then the accepting proof again up to n proofs."""
    good, claim = c.proofs[c.mutated], c.claims[c.mutated]
    proofs = [good] + [m.words for m in muts]
    proofs += [good] * max(0, n - len(proofs))
    want = [1] + [want_all[m.name] for m in muts] + [1] * (len(proofs) - 1 - len(muts))
    what = (c.name, len(proofs), montgomery)
    b = _batch(ctx, c, [claim] * len(proofs), proofs, montgomery)
    try:
        v, ok = b.run()
        assert not ok and [int(x) for x in v] == want, (what, [int(x) for x in v])
        for j in [0] + list(range(len(muts) + 1, len(proofs))):
            assert b.transcript(j, max_xfe=1)[2] == 0, (what, j)
        for j, m in enumerate(muts):
            fail = b.transcript(j + 1, max_xfe=1)[2]
            assert fail & m.bit, (what, m.name, fail)
            assert fail & ~m.allowed == 0, (what, m.name, fail)
        perms = b.stats()["tip5_perms_merkle"]
        print(what, "tip5_perms_merkle", perms, "unmutated", len(proofs) * c.ops[c.mutated])
        if any(m.kind == "short" for m in muts):
            assert perms < len(proofs) * c.ops[c.mutated], what
    finally:
        b.close()


@pytest.mark.parametrize("name", MI.NAMES)
def test_mutants_fail_their_own_tree_alone(ctx, name):
    import coracle as C
    c = MI.case(name)
    ms = c.mutants
    claim = c.claims[c.mutated]
    want = C.stark_verify_batch(c.air_words, c.params, [claim] * len(ms), [m.words for m in ms], threads=4)
    assert [int(x) for x in want] == [0] * len(ms)  # no mutant the oracle accepts
    want_all = {m.name: int(x) for m, x in zip(ms, want)}
    chunk = MI.MP_CLIMB_MAX_PROOFS - N_SMALL
    for montgomery in (False, True):
        for at in range(0, len(ms), chunk):  # k_mp_climb: 3 + m proofs, at most 32
            part = ms[at:at + chunk]
            _run_mutants(ctx, c, part, N_SMALL + len(part), montgomery, want_all)
        _run_mutants(ctx, c, ms, N_LEVELS, montgomery, want_all)  # per-level launches: 33 proofs or more
