"""CPU side of the Merkle index-pattern tests (merkle_index_cases.py): the pinned proofs reach every
pattern the multiproof plan branches on, the Python and the C oracle accept every proof and reject
every mutant with the expected first error, the reference hash count equals a count of the oracle's own
hash_pair calls, and the restated launch schedule selects the kernels the GPU test names: the fixtures
are right before a GPU sees them."""
import pytest

import merkle_index_cases as MI
import stark_ref as S
import table_shapes_cases as TS
import tip5_ref as T


def test_cases_reach_every_pattern():
    MI.assert_coverage()


def test_coverage_predicate_names_what_is_missing():
    """The predicate is not vacuous: a set without its four-wave configurations, without the k = 8 one
    or with a single configuration has gaps, and names them."""
    cases = [MI.case(n) for n in MI.NAMES]
    gaps = MI.coverage_gaps([c for c in cases if MI.waves(c.k) != 4])
    assert "dup in a group 0 at 4 wave(s)" in gaps and "a proof of k = 256" in gaps
    assert "spread at k = 8" in MI.coverage_gaps([c for c in cases if c.k != 8])
    gaps = MI.coverage_gaps([MI.case("k1")])
    for what in ("dup in a group 0 at 1 wave(s)", "sibling in a b-tree of a round >= 1",
                 "a dup-first mutant of main at 1 wave(s)", "k = 1 and 2: last codewords of 8 and 16"):
        assert what in gaps, what


def test_patterns_on_hand_made_lists():
    """patterns() on lists whose answer is plain (tree of 16 leaves)."""
    p = MI.patterns(4, [4, 4, 5])
    assert p["dup"] and p["sibling"] and p["dup_sibling"] and not p["mult3"] and not p["no_dup"]
    assert not p["first_dup"] and not p["last_dup"] and p["distinct"] == 2 and not p["leaf0"] and not p["leafN1"]
    assert not p["inner_merge"] and not p["odd_even"]  # one pair, nothing beside it
    p = MI.patterns(4, [0, 15, 15, 2, 15])
    assert p["mult3"] and p["first_dup"] and p["last_dup"] and p["leaf0"] and p["leafN1"] and p["inner_merge"]
    assert p["odd_even"] and not p["sibling"] and not p["spread"]
    p = MI.patterns(4, [1, 6, 8, 13])
    assert p["spread"] and p["no_dup"] and p["auth_len"] == 8 and MI.group_ops(4, [1, 6, 8, 13]) == 4 + 4 + 2 + 1
    assert MI.patterns(4, [1, 6, 8, 9])["spread"] is False


@pytest.mark.parametrize("name", MI.NAMES)
def test_reference_hash_count(name):
    """merkle_ops (the closed form over the indices) against the hash_pair calls the oracle makes
    while it verifies the proof: merkle_multiproof_root's, counted, plus the L - 1 parents of the last
    codeword's tree, which fri_verify builds whole (merkle_nodes of L leaves)."""
    c = MI.case(name)
    real = T.hash_pair
    for i, proof in enumerate(c.proofs):
        calls = [0]

        def counted(l, r):
            calls[0] += 1
            return real(l, r)

        T.hash_pair = counted
        try:
            S._verify(c.params, c.air, c.claims[i], [int(w) for w in proof], {})
        finally:
            T.hash_pair = real
        h, R = c.shapes[i]
        assert c.ops[i] == calls[0] + (1 << (h - R)) - 1, (name, i)
        assert c.ops[i] == sum(c.level_ops(i, l) for l in range(h)), (name, i)
        for (gh, lv), p in zip(c.groups[i], c.patterns[i]):
            assert len(lv) == c.k and p["distinct"] <= c.k and all(0 <= v < (1 << gh) for v in lv)


@pytest.mark.parametrize("name", MI.NAMES)
def test_oracles_agree_on_proofs_and_mutants(name):
    import coracle as C
    c = MI.case(name)
    ms = c.mutants
    assert len({m.name for m in ms}) == len(ms)
    for m in ms:  # the Python oracle's first error is that tree's authentication failure
        ok, err, _, _ = TS.oracle(c.params, c.air, c.claims[c.mutated], m.words)
        assert not ok and err == m.error and m.bit is not None, (name, m.name, err)
        assert m.bit in MI.MERKLE_BITS + (MI.FAIL_MERKLE_FRI,) and m.allowed & m.bit
        if m.kind in ("short", "long", "order") or m.kind.startswith("digest"):
            assert m.allowed == m.bit, m.name
    claims = c.claims + [c.claims[c.mutated]] * len(ms)
    proofs = c.proofs + [m.words for m in ms]
    got = C.stark_verify_batch(c.air_words, c.params, claims, proofs, threads=4)
    assert [int(v) for v in got] == [1] * len(c.proofs) + [0] * len(ms)
    assert len({p.tobytes() for p in c.proofs}) == len(c.proofs)
    for samples, indices in c.want:
        assert len(indices) == c.k


def test_aux_alone_one_short_is_among_the_mutants():
    for name in MI.NAMES:
        assert any(m.name == "aux authentication structure: last digest dropped" and m.allowed == TS.FAIL_MERKLE_AUX
                   for m in MI.case(name).mutants), name


def test_launch_schedule_of_the_batches():
    """hash_steps (plan_launch restated) for the batches the GPU test runs: one climb up to 32 proofs;
    from 33 on per-level launches and a tail; a forced climb-from threshold hands over at a level above 0; the
    k = 256 lane-form batch has its level 0 above MP_WIDE_MAX_OPS by the reference count already."""
    for name in MI.NAMES:
        c = MI.case(name)
        m = len(c.proofs)
        assert MI.hash_steps(c.k, [c.shapes[i % m] for i in range(3)]) == [("climb", 0)]
        shapes = [c.shapes[i % m] for i in range(33)]
        steps = MI.hash_steps(c.k, shapes)
        assert steps == MI.hash_steps(c.k, shapes, 0), name
        # (k = 256: 33 proofs' capacity puts levels 0 and 1 past MP_WIDE_MAX_OPS already)
        body = {kd for kd, _ in steps[:-1]}
        assert steps[-1][0] == "tail" and body == ({"wide"} if c.k < 256 else {"level7", "wide"}), (name, steps)
        forced = MI.hash_steps(c.k, shapes, MI.climb_from_for(c.k, shapes))
        assert forced[-1][0] == "climb" and forced[-1][1] > 0 and len(forced) < len(steps), (name, forced)
    c = MI.case("k256")
    n = MI.lane_form_batch(c)
    pick = [i % len(c.proofs) for i in range(n)]
    assert sum(c.level_ops(i, 0, lcw=False) for i in pick) > MI.MP_WIDE_MAX_OPS and 33 < n <= 96
    assert MI.hash_steps(c.k, [c.shapes[i] for i in pick])[0] == ("level7", 0)
