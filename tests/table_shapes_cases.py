"""Table shapes (num_main M, num_aux A, num_quotient_segments Q) for the STARK kernels that branch on
the row widths, with the proofs, oracle transcripts and mutants of each: shared by
test_table_shapes_host.py (the set covers every property; the Python and the C oracle agree on every
proof and mutant) and test_gpu_table_shapes.py (the GPU against those oracle results).

What the widths select in the kernels (stark_kernels.hip):
  * row hashing (k_hash_rows, hash_rows_wide_body) and the Fiat-Shamir absorbs (k_fs_replay_wide row
    and pair, k_fs_replay_quad) take a row of `width` words as width // 10 full chunks and one padded
    chunk of rem = width % 10 words, then a 1, then zeros: rem == 0 (the padded chunk is the 1 alone),
    rem == 1, rem == 9, a width below 10 (the first chunk is the padded one), exactly 10, 20 or more;
  * k_deep_rows8's lane q8 of a row takes words q8, q8 + 8, ... of the main row and of the aux row in
    steps of 8 * DEEP_UNROLL words and then one at a time: every residue mod 8 of M and of 3A, a width
    below, on and just past a multiple of 8 * DEEP_UNROLL, and a row of nearly DEEP_ROW_WORDS_MAX words
    (the carry-free accumulators at their bound);
  * z^Q, the quotient segments' sums and every sample's offset behind the M + A + Q + 3 weights.

Every proof is made here, at test time, by stark_prover_fast at log2 padded height 4 (under 0.2 s for
the small shapes, about 1.5 s for the two wide ones)."""
import functools

import numpy as np

import stark_ref as S
import tip5_ref as T

DEEP_UNROLL = 8  # stark_kernels.hip: static constexpr uint32_t DEEP_UNROLL = 8
DEEP_STRIDE = 8 * DEEP_UNROLL  # words a row's 8 lanes take per unrolled iteration
DEEP_ROW_WORDS_MAX = 2048  # kernels.hpp; dims_from (air_host.cpp) takes M + 3A below it
DEEP_LANE_TERMS_MAX = (DEEP_ROW_WORDS_MAX - 1 + 14) // 8  # kernels.hpp: 258
TIP5_RATE = 10
Q_MAX = 64  # dims_from: 1 <= num_quotient_segments <= 64

# (M, A, Q): row widths M, 3A, 3Q
SHAPES = [
    (10, 3, 1),      # widths 10, 9, 3
    (20, 10, 2),     # 20, 30, 6
    (7, 1, 3),       # 7, 3, 9: every row a single padded chunk; the smallest AIR with main targets
    (64, 7, 5),      # 64, 21, 15: M on a multiple of 8 * DEEP_UNROLL, 3A % 10 == 1
    (65, 43, 64),    # 65, 129, 192: M and 3A one past a multiple, the largest Q
    (11, 64, 4),     # 11, 192, 12: 3A on a multiple, M % 10 == 1
    (13, 6, 7),      # 13, 18, 21
    (30, 5, 1),      # 30, 15, 3
    (2017, 10, 4),   # 2017, 30, 12: M + 3A = 2047, 253 + 4 = 257 terms per lane, M-heavy
    (19, 676, 4),    # 19, 2028, 12: M + 3A = 2047, 3 + 254 = 257 terms per lane, A-heavy
]
IDS = ["%d-%d-%d" % s for s in SHAPES]


def widths(shape):
    M, A, Q = shape
    return (M, 3 * A, 3 * Q)


def lane_terms(shape):
    """Most words one lane of k_deep_rows8 accumulates: ceil(M / 8) + ceil(3A / 8)."""
    M, A, _ = shape
    return -(-M // 8) + -(-3 * A // 8)


def coverage_gaps(shapes):
    """The properties (module doc) that no shape of the list has, as words; [] when all are hit."""
    gaps = []

    def need(what, found):
        if not found:
            gaps.append(what)

    ws = [w for s in shapes for w in widths(s)]
    for rem in (0, 1, 9):
        need(f"a width with % 10 == {rem}", any(w % TIP5_RATE == rem for w in ws))
    need("a width below 10", any(0 < w < TIP5_RATE for w in ws))
    need("a width of exactly 10", TIP5_RATE in ws)
    need("a width of at least 20 with % 10 == 0", any(w >= 2 * TIP5_RATE and w % TIP5_RATE == 0 for w in ws))
    for name, vals in (("M", [s[0] for s in shapes]), ("3A", [3 * s[1] for s in shapes])):
        for r in range(8):
            need(f"{name} % 8 == {r}", any(v % 8 == r for v in vals))
        need(f"{name} below 8 * DEEP_UNROLL", any(0 < v < DEEP_STRIDE for v in vals))
        need(f"{name} on a multiple of 8 * DEEP_UNROLL", any(v > 0 and v % DEEP_STRIDE == 0 for v in vals))
        need(f"{name} one past a multiple of 8 * DEEP_UNROLL", any(v > DEEP_STRIDE and v % DEEP_STRIDE == 1 for v in vals))
    qs = [s[2] for s in shapes]
    need("Q == 1", 1 in qs)
    need("Q == 2", 2 in qs)
    need("an odd Q of at least 5", any(q >= 5 and q % 2 == 1 for q in qs))
    need(f"Q == {Q_MAX}", Q_MAX in qs)
    need("a wide shape: 2040 <= M + 3A < 2048 with DEEP_LANE_TERMS_MAX - 1 terms or more per lane",
         any(2040 <= s[0] + 3 * s[1] < DEEP_ROW_WORDS_MAX and lane_terms(s) >= DEEP_LANE_TERMS_MAX - 1 for s in shapes))
    need("every shape inside dims_from's range",
         all(s[0] + 3 * s[1] < DEEP_ROW_WORDS_MAX and 1 <= s[2] <= Q_MAX for s in shapes))
    return gaps


def assert_coverage(shapes):
    gaps = coverage_gaps(shapes)
    assert not gaps, "the shape list misses: " + "; ".join(gaps)


# ---------------------------------------------------------------------------- oracle results
FAIL_OOD = 1 << 1
FAIL_MERKLE_MAIN = 1 << 2
FAIL_MERKLE_AUX = 1 << 3
FAIL_MERKLE_QUOT = 1 << 4
FAIL_FRI_LAST_ROOT = 1 << 6
FAIL_FRI_LAST_AGREE = 1 << 7
FAIL_FRI_DEGREE = 1 << 8
FAIL_FRI_EVAL = 1 << 9
FAIL_DEEP = 1 << 10
# the oracle's first error (stark_ref._verify / fri_verify) -> the fail bit of that phase (stark.hpp)
PHASE = {
    "out-of-domain quotient value mismatch": FAIL_OOD,
    "main codeword authentication failure": FAIL_MERKLE_MAIN,
    "aux codeword authentication failure": FAIL_MERKLE_AUX,
    "quotient codeword authentication failure": FAIL_MERKLE_QUOT,
    "FRI: bad Merkle root for last codeword": FAIL_FRI_LAST_ROOT,
    "FRI: last codeword mismatch": FAIL_FRI_LAST_AGREE,
    "FRI: last polynomial degree too high": FAIL_FRI_DEGREE,
    "FRI: last polynomial evaluation mismatch": FAIL_FRI_EVAL,
    "combination codeword mismatch": FAIL_DEEP,
}


def oracle(params, air, claim, proof):
    """(accepted, first error, samples, indices) of the oracle verifier."""
    tr = {}
    try:
        S._verify(params, air, claim, [int(w) for w in proof], tr)
    except S.VerifyError as e:
        return False, str(e), None, None
    samples = [tuple(x) for tag, vals in tr["sponge_samples"] if tag != "fri_indices" for x in vals]
    indices = [v for tag, vals in tr["sponge_samples"] if tag == "fri_indices" for v in vals]
    return True, None, samples, indices


def _bump_x(x, c):
    y = list(x)
    y[c] = (y[c] + 1) % S.P
    return tuple(y)


def mutants(proof, params):
    """[(name, words, the oracle's phase)] of one proof: one word + 1 mod p each, through decode_proof /
    encode_proof (the stream stays well-formed).  A revealed-row word fails its tree's authentication
    (and may fail DEEP, which takes the same rows as values); an OOD word changes the quotient
    identity's sides (and, absorbed, every later sample)."""
    words = [int(w) for w in proof]
    items = S.decode_proof(words, params)
    assert S.encode_proof(items, params) == words
    kinds = [k for k, _ in items]
    M = params.num_main

    def changed(kind, edit):
        out = list(items)
        i = kinds.index(kind)  # the first item of the kind (OOD rows: the current row)
        out[i] = (kind, edit(out[i][1]))
        return np.array(S.encode_proof(out, params), dtype=np.uint64)

    def main_word(row, col):
        def edit(rows):
            rows = [list(r) for r in rows]
            rows[row][col] = (rows[row][col] + 1) % S.P
            return rows
        return edit

    def last_x_word_of_last_row(rows):
        rows = [list(r) for r in rows]
        rows[-1][-1] = _bump_x(rows[-1][-1], 2)
        return rows

    def x_word(i, c):
        def edit(xs):
            xs = list(xs)
            xs[i] = _bump_x(xs[i], c)
            return xs
        return edit

    muts = [
        ("last word of the last main row", changed(S.MAIN_ROWS, main_word(-1, M - 1)), FAIL_MERKLE_MAIN),
        ("last word of the last aux row", changed(S.AUX_ROWS, last_x_word_of_last_row), FAIL_MERKLE_AUX),
        ("last word of the last quotient row", changed(S.QUOT_SEGMENTS_ELEMENTS, last_x_word_of_last_row),
         FAIL_MERKLE_QUOT),
    ]
    if M >= TIP5_RATE:  # the last word before the padded chunk of the first main row
        muts.append(("last full-chunk word of the first main row",
                     changed(S.MAIN_ROWS, main_word(0, TIP5_RATE * (M // TIP5_RATE) - 1)), FAIL_MERKLE_MAIN))
    muts += [
        ("word 0 of the OOD quotient segments", changed(S.OOD_QUOT_SEGMENTS, x_word(0, 0)), FAIL_OOD),
        ("last word of the OOD aux row", changed(S.OOD_AUX_ROW, x_word(-1, 2)), FAIL_OOD),
    ]
    return muts


CLAIMS = [
    ([2, 7, 1, 8, 2], 0, [8, 1], [8, 2, 8]),
    ([3, 1, 4, 1, 5], 0, [9, 2, 6], [5, 3]),
    ([1, 6, 1, 8, 0], 0, [], [3, 3, 9, 8, 8]),
]
LOG2_HEIGHT = 4


class ShapeCase:
    """One shape's AIR, three distinct accepting proofs (claims and prover seeds differ) with the
    oracle's transcripts, and the mutants of the first proof with the oracle's first error."""

    def __init__(self, shape):
        import stark_prover_fast as SP
        T.use_c_backend()
        M, A, Q = shape
        self.shape = shape
        self.params = S.StarkParams(num_main=M, num_aux=A, num_quotient_segments=Q)
        self.air, recipe = S.synth_air(self.params, seed=1 + M + A + Q)
        self.air_words = self.air.to_words()
        self.claims = list(CLAIMS)
        self.proofs, self.want = [], []
        for i, claim in enumerate(self.claims):
            proof, _ = SP.prove(self.params, self.air, recipe, claim, LOG2_HEIGHT, seed=100 * i + M + Q)
            proof = np.array([int(w) for w in proof], dtype=np.uint64)
            ok, err, samples, indices = oracle(self.params, self.air, claim, proof)
            assert ok, (shape, i, err)
            self.proofs.append(proof)
            self.want.append((samples, indices))
        self.mutants = mutants(self.proofs[0], self.params)
        self.mutant_errors = [oracle(self.params, self.air, self.claims[0], w)[1] for _, w, _ in self.mutants]


@functools.lru_cache(maxsize=None)
def case(shape):
    return ShapeCase(shape)
