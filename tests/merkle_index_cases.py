"""Revealed-leaf index patterns and authentication-structure lengths for the Merkle multiproof path
(stark_kernels.hip: mp_plan_body, k_mp_plan<128|256>, k_plan_fri_small, k_mp_hash, k_mp_hash_wide,
k_mp_hash_tail, k_mp_climb, mp_roots_body), with the proofs, oracle transcripts, reference hash counts
and mutants of each configuration: shared by test_merkle_index_host.py (the set reaches every pattern;
the Python and the C oracle agree on every proof and mutant; the reference count is right) and
test_gpu_merkle_index.py (the GPU against those oracle results).

What the plan does is decided by the leaf indices Fiat-Shamir samples, so a pattern cannot be asked
for: the prover seeds below were found by a search on the CPU (a few hundred seeds per configuration
and height) and are pinned, and coverage_gaps() recomputes every pattern from the oracle's indices
when the tests are collected and names what the set no longer reaches.

Tree groups of a proof with FRI domain N = 2^h and R folding rounds, as mp_plan_body forms them and
fri_verify checks them: group 0 is the four trees of height h (main, aux, quotient, FRI round-0
a-values) at the leaves idx % N; group 1 + r is the b-tree of round r, of height h - r, at the leaves
((idx % (N >> r)) + (N >> r) / 2) % (N >> r).

Patterns of one group (patterns()):
  dup            some leaf revealed twice (kept once by the plan, compared in mp_roots_body)
  mult3          some leaf revealed three times or more (a chain of duplicate records)
  sibling        leaves 2q and 2q + 1 both revealed (an op with no authentication digest)
  inner_merge    two revealed nodes that are siblings at level 1 or above: their paths first meet in
                 a parent at level 2 or above
  dup_sibling    a duplicated leaf whose sibling is revealed as well
  leaf0, leafN1  leaf 0 / leaf N - 1 (node keys 2^h and 2^(h+1) - 1: both ends of the sort)
  odd_even       an unpaired odd and an unpaired even leaf (the digest goes left / right)
  no_dup         every revealed leaf distinct
  first_dup      the first sorted slot is a duplicate: the largest leaf is revealed twice
  last_dup       the list's last slot (k - 1) reveals a leaf that an earlier slot reveals too
  spread         k distinct, pairwise non-sibling leaves (no op of level 0 is paired)
and the numbers `distinct` (leaves kept) and `auth_len` (digests of the authentication structure).

Required (coverage_gaps): every pattern but `spread` in a group 0 at one wave of index slots
(k <= 64), at two (65..128) and at four (129..256); every pattern but no_dup, leaf0 and leafN1 in a
b-tree of a round >= 1; `spread` at k = 8; a k = 256 proof (every slot of the 256-thread plan holds an
index).  Nothing of the list is left out.

Every proof is made here, at test time, by stark_prover_fast at table shape (10, 3, 1)."""
import functools

import numpy as np

import stark_ref as S
import table_shapes_cases as TS
import tip5_ref as T

SHAPE = (10, 3, 1)
CLAIMS = TS.CLAIMS
FAIL_MERKLE_FRI = 1 << 5  # stark.hpp
MERKLE_BITS = (TS.FAIL_MERKLE_MAIN, TS.FAIL_MERKLE_AUX, TS.FAIL_MERKLE_QUOT)
TREE_ERRORS = ("main codeword authentication failure", "aux codeword authentication failure",
               "quotient codeword authentication failure")

# stark_launch_plan.hpp / kernels.hpp
MP_CLIMB_MAX_PROOFS = 32
MP_WIDE_MAX_OPS = 48 * 1024
MP_TAIL_MAX_OPS = 256
MP_TAIL_LEVELS_MAX = 32
MP_SMALL_MAX_PROOFS = 4096
CLIMB_FROM_MIN_LEVELS = 24
CLIMB_FROM_OPS_DEFAULT = 4096
CLIMB_FROM_MIN_REST = 3


def phase(err):
    """The oracle's first error -> the fail bit of that check (stark.hpp)."""
    if err is not None and err.startswith("FRI: bad Merkle authentication"):
        return FAIL_MERKLE_FRI
    return TS.PHASE.get(err)


def waves(k):
    """Waves of index slots: wg_count_scan2's partial sums cover 1, 2 or 4 of them."""
    return 1 if k <= 64 else 2 if k <= 128 else 4


# name -> (security level, log2 FRI expansion, num_collinearity_checks, AIR seed,
#          [(log2 padded height, prover seed), ...], index of the proof the mutants are made of)
# Heights: one with R = 0 (k = 8: log2 height 0, a domain of 64; the oracle's own degree check refuses
# its heights 1 and 2), one with R = 1 and one with R >= 3; k = 1 and 2 have no R = 0 height that the
# oracle takes and stand at heights 7 and 9 (7 to 10 FRI responses, last codewords of 8 and 16 values).
CONFIGS = {
    "k1": (160, 2, 1, 3, [(7, 1), (9, 1)], 0),
    "k2": (160, 2, 2, 3, [(7, 1), (9, 16)], 0),
    "k8": (160, 2, 8, 3, [(0, 2), (3, 1), (6, 63)], 2),
    "k64": (160, 2, 64, 3, [(4, 1), (7, 16), (9, 5)], 2),
    "k65": (160, 2, 65, 3, [(4, 48), (7, 26), (9, 58)], 2),
    "k80": (160, 2, 80, 3, [(4, 5), (7, 1), (9, 3)], 2),
    "k128": (160, 2, 128, 3, [(4, 1), (7, 1), (10, 1)], 2),
    "k129": (160, 2, 129, 3, [(4, 1), (7, 44), (10, 42)], 2),
    "k256": (256, 1, 256, 3, [(2, 5), (8, 1), (11, 1)], 2),
}
NAMES = list(CONFIGS)


def params_of(name):
    sec, log2_exp, k, _, _, _ = CONFIGS[name]
    M, A, Q = SHAPE
    p = S.StarkParams(sec, log2_exp, M, A, Q, num_collinearity_checks=k)
    assert p.num_collinearity_checks == k
    return p


def domain_shape(params, log2_ph):
    """(log2 N, R) of a proof of this padded height."""
    N = params.fri_domain(1 << log2_ph).length
    return N.bit_length() - 1, params.fri_num_rounds(N)


def groups(params, log2_ph, indices):
    """[(tree height, leaf of each index slot)] of the proof's tree groups (module doc)."""
    h, R = domain_shape(params, log2_ph)
    out = [(h, [i % (1 << h) for i in indices])]
    for r in range(R):
        n = 1 << (h - r)
        out.append((h - r, [((i % n) + n // 2) % n for i in indices]))
    return out


def patterns(h, leaves):
    """The patterns (module doc) of one tree group: name -> bool, and the two numbers."""
    N, k = 1 << h, len(leaves)
    count = {}
    for v in leaves:
        count[v] = count.get(v, 0) + 1
    dups = [v for v, c in count.items() if c > 1]
    nodes, inner = set(count), False
    for _ in range(1, h):
        nodes = {v >> 1 for v in nodes}
        inner = inner or any(v ^ 1 in nodes for v in nodes)
    unpaired = [v for v in count if v ^ 1 not in count]
    return {
        "dup": bool(dups),
        "mult3": any(c >= 3 for c in count.values()),
        "sibling": any(v ^ 1 in count for v in count),
        "inner_merge": inner,
        "dup_sibling": any(v ^ 1 in count for v in dups),
        "leaf0": 0 in count,
        "leafN1": N - 1 in count,
        "odd_even": any(v & 1 for v in unpaired) and any(not v & 1 for v in unpaired),
        "no_dup": not dups,
        "first_dup": count[max(count)] > 1,
        "last_dup": leaves[-1] in leaves[:-1],
        "spread": len(count) == k and not any(v ^ 1 in count for v in count),
        "distinct": len(count),
        "auth_len": len(S.auth_structure_node_indices(N, leaves)),
    }


GROUP0 = ("dup", "mult3", "sibling", "inner_merge", "dup_sibling", "leaf0", "leafN1", "odd_even", "no_dup",
          "first_dup", "last_dup")
B_TREE = ("dup", "mult3", "sibling", "inner_merge", "dup_sibling", "odd_even", "first_dup", "last_dup")


def group_ops(h, leaves):
    """hash_pair calls of merkle_multiproof_root for one accepted tree: one per distinct parent node,
    sum over levels l = 1..h of |{(leaf + 2^h) >> l}|."""
    return sum(len({(v + (1 << h)) >> l for v in leaves}) for l in range(1, h + 1))


def merkle_ops(params, log2_ph, indices, level=None, lcw=True):
    """Tip5 permutations of an accepting proof's Merkle checks, from the oracle's indices alone: four
    times group 0's (main, aux, quotient and FRI round-0 a-tree open the same leaves), each b-tree's,
    and the L - 1 parents of the last codeword's tree of L leaves (fri_verify builds all of it;
    proof_codec.hpp counts the same L - 1 as perms_lcw).  This is what nhip_batch_stats'
    tip5_perms_merkle sums: the ops the plan reserved, minus those of trees it gave up, plus perms_lcw.
    level: the parents of that one level only (level 0: the parents of the leaves), with or without
    the last codeword's."""
    gs = groups(params, log2_ph, indices)
    h, R = domain_shape(params, log2_ph)
    last = 1 << (h - R)
    if level is None:
        return sum((4 if g == 0 else 1) * group_ops(gh, lv) for g, (gh, lv) in enumerate(gs)) + last - 1
    per = sum((4 if g == 0 else 1) * len({(v + (1 << gh)) >> (level + 1) for v in lv})
              for g, (gh, lv) in enumerate(gs) if level < gh)
    return per + ((last >> (level + 1)) if lcw else 0)


def hash_steps(k, shapes, climb_from=-1):
    """plan_launch's Merkle hash launches (stark_launch_plan.hpp, restated) for a batch of proofs of
    the given (log2 N, R) shapes: [(kind, first level)], kind one of climb / tail / wide / level7.
    climb_from: nhip_set_climb_from_ops's value (-1: by depth, 0: never)."""
    n = len(shapes)
    if n <= MP_CLIMB_MAX_PROOFS:
        return [("climb", 0)]
    levels = max(h for h, _ in shapes)
    cap = [0] * levels  # mp_capacities (stark_layout.hpp): min(k, 2^(h - 1 - l)) per tree and level
    for h0, R in shapes:
        for h in [h0] * 4 + [h0 - r for r in range(R)]:
            for l in range(h):
                cap[l] += min(k, 1 << (h - 1 - l))
    max_lcw = max(1 << (h - R) for h, R in shapes)
    hash_levels = max(levels, max_lcw.bit_length() - 1)

    def ops(l):
        return (cap[l] if l < levels else 0) + (max_lcw >> (l + 1)) * n

    tail0 = hash_levels
    while tail0 > 0 and hash_levels - tail0 < MP_TAIL_LEVELS_MAX and ops(tail0 - 1) <= MP_TAIL_MAX_OPS:
        tail0 -= 1
    if hash_levels - tail0 < 2:
        tail0 = hash_levels
    limit = CLIMB_FROM_OPS_DEFAULT if hash_levels >= CLIMB_FROM_MIN_LEVELS else 0
    if climb_from >= 0:
        limit = climb_from
    steps = []
    for l in range(hash_levels):
        if limit and ops(l) <= limit and hash_levels - l >= CLIMB_FROM_MIN_REST:
            steps.append(("climb", l))
            break
        if l == tail0:
            steps.append(("tail", l))
            break
        if ops(l) == 0:
            continue
        steps.append(("wide" if ops(l) <= MP_WIDE_MAX_OPS else "level7" if n < MP_SMALL_MAX_PROOFS else "level6", l))
    return steps


def level_ops_bound(k, shapes, l):
    """The op count plan_launch sizes level l by (hash_steps' ops): capacity, not the ops planned."""
    n = len(shapes)
    cap = sum(min(k, 1 << (h - 1 - l)) for h0, R in shapes for h in [h0] * 4 + [h0 - r for r in range(R)] if l < h)
    return cap + (max(1 << (h - R) for h, R in shapes) >> (l + 1)) * n


def climb_from_for(k, shapes):
    """A threshold for nhip_set_climb_from_ops at which the per-level launches of this batch hand over
    to k_mp_climb above level 0: the bound of the first level that is smaller than level 0's and
    leaves CLIMB_FROM_MIN_REST levels."""
    levels = max(max(h for h, _ in shapes), max(h - R for h, R in shapes))
    for l in range(1, levels - CLIMB_FROM_MIN_REST + 1):
        if level_ops_bound(k, shapes, l) < level_ops_bound(k, shapes, 0):
            return level_ops_bound(k, shapes, l)
    raise AssertionError("no level to hand over at")


def lane_form_batch(c):
    """The smallest batch of c's proofs in turn whose multiproof ops of level 0 alone, by the reference
    count and without the last codewords' parents, exceed MP_WIDE_MAX_OPS: plan_launch's bound is no
    smaller, so level 0 runs the lane-form k_mp_hash, its multiproof blocks alone past the bound."""
    n, ops = 0, 0
    while ops <= MP_WIDE_MAX_OPS:
        ops += c.level_ops(n % len(c.proofs), 0, lcw=False)
        n += 1
    return n


# ---------------------------------------------------------------------------- mutants
class Mutant:
    """name, the proof's words, the oracle's first error, its fail bit, and the bits the fail word may
    hold beside it (allowed includes the bit)."""

    def __init__(self, name, words, error, allowed, kind, tree):
        self.name, self.words, self.error, self.kind, self.tree = name, words, error, kind, tree
        self.bit = phase(error)
        self.allowed = self.bit | allowed


def _bump(v):
    return (int(v) + 1) % S.P


def mutants(proof, params, log2_ph, indices):
    """Mutants of one accepting proof through decode_proof / encode_proof (the stream stays
    well-formed).  Which checks take the changed values, from _verify's and fri_verify's control flow:
      * an authentication structure (length, order or one digest word) is read by that tree's Merkle
        check alone: exactly the tree's bit;
      * a revealed main / aux / quotient row is hashed into its tree's leaf and combined by DEEP:
        the tree's bit, and FAIL_DEEP may join it;
      * a FRI response's leaf is that round's a- or b-value: FAIL_MERKLE_FRI, and the folded values no
        longer meet the last codeword (FAIL_FRI_LAST_AGREE); response 0's leaves are also DEEP's
        right-hand sides (FAIL_DEEP).
    kind: short / long (length), order, digest, dup-first / dup-last (one copy of a leaf revealed twice).
    tree: main, aux, quot, or fri<r> for FRI response r."""
    words = [int(w) for w in proof]
    items = S.decode_proof(words, params)
    assert S.encode_proof(items, params) == words
    kinds = [kd for kd, _ in items]
    h, R = domain_shape(params, log2_ph)
    gs = groups(params, log2_ph, indices)
    auth_at = [i for i, kd in enumerate(kinds) if kd == S.AUTH_STRUCTURE]
    rows_at = [kinds.index(kd) for kd in (S.MAIN_ROWS, S.AUX_ROWS, S.QUOT_SEGMENTS_ELEMENTS)]
    fri_at = [i for i, kd in enumerate(kinds) if kd == S.FRI_RESPONSE]
    assert len(auth_at) == 3 and len(fri_at) == R + 1
    out = []

    def add(name, at, payload, error, allowed, kind, tree):
        changed = list(items)
        changed[at] = (kinds[at], payload)
        out.append(Mutant(name, np.array(S.encode_proof(changed, params), dtype=np.uint64), error, allowed, kind, tree))

    def lengths(auth, full):
        more = auth + [list(auth[-1]) if auth else [0] * 5]
        cuts = [("last digest dropped", auth[:-1], "short"), ("one digest appended", more, "long"),
                ("emptied", [], "short")]
        if full:
            cuts.insert(1, ("first digest dropped", auth[1:], "short"))
            if len(auth) >= 2 and auth[0] != auth[1]:
                cuts.append(("first two digests swapped", [auth[1], auth[0]] + auth[2:], "order"))
        return [c for c in cuts if c[1] != auth]

    def first_last_dup(leaves):
        for v in leaves:
            at = [j for j, w in enumerate(leaves) if w == v]
            if len(at) > 1:
                return [("dup-first", at[0]), ("dup-last", at[-1])]
        return []

    def sibling_digests(gh, leaves):
        """(odd / even, position in the authentication structure) of a digest that is the sibling of
        an unpaired odd leaf, and of an unpaired even one."""
        nodes = S.auth_structure_node_indices(1 << gh, leaves)
        found = {}
        for j, ni in enumerate(nodes):
            if ni >= (1 << gh):  # a leaf's sibling: ni ^ 1 is revealed and ni is not
                found.setdefault("odd" if (ni ^ 1) & 1 else "even", j)
        return sorted(found.items())

    tree_names = ("main", "aux", "quot")
    for t in range(3):
        auth = [list(d) for d in items[auth_at[t]][1]]
        for what, cut, kind in lengths(auth, True):
            add(f"{tree_names[t]} authentication structure: {what}", auth_at[t], cut, TREE_ERRORS[t], 0, kind,
                tree_names[t])
        for kind, j in first_last_dup(gs[0][1]):
            rows = [list(r) for r in items[rows_at[t]][1]]
            rows[j][0] = _bump(rows[j][0]) if t == 0 else TS._bump_x(rows[j][0], 0)
            add(f"{tree_names[t]} row of slot {j}: one copy of a leaf revealed twice", rows_at[t], rows,
                TREE_ERRORS[t], TS.FAIL_DEEP, kind, tree_names[t])
    for side, j in sibling_digests(*gs[0]):
        auth = [list(d) for d in items[auth_at[0]][1]]
        auth[j][0] = _bump(auth[j][0])
        add(f"main authentication structure: digest {j}, sibling of an unpaired {side} leaf", auth_at[0], auth,
            TREE_ERRORS[0], 0, "digest-" + side, "main")
    for r in range(R + 1):
        auth, leaves = items[fri_at[r]][1]
        auth, leaves = [list(d) for d in auth], list(leaves)
        error = "FRI: bad Merkle authentication " + ("(round 0, a)" if r == 0 else f"(round {r - 1}, b)")
        for what, cut, kind in lengths(auth, False):
            add(f"FRI response {r} authentication structure: {what}", fri_at[r], (cut, leaves), error, 0, kind,
                f"fri{r}")
        extra = TS.FAIL_FRI_LAST_AGREE | (TS.FAIL_DEEP if r == 0 else 0)
        for kind, j in first_last_dup(gs[r][1]):
            lv = list(leaves)
            lv[j] = TS._bump_x(lv[j], 0)
            add(f"FRI response {r} leaf of slot {j}: one copy of a leaf revealed twice", fri_at[r], (auth, lv), error,
                extra, kind, f"fri{r}")
        if r == R and R >= 1:  # the smallest b-tree
            for side, j in sibling_digests(*gs[r]):
                au = [list(d) for d in auth]
                au[j][4] = _bump(au[j][4])
                add(f"FRI response {r} authentication structure: digest {j}, sibling of an unpaired {side} leaf",
                    fri_at[r], (au, leaves), error, 0, "digest-" + side, f"fri{r}")
    return out


# ---------------------------------------------------------------------------- the cases
class IndexCase:
    """One configuration: its AIR, one accepting proof per pinned (height, seed) with the oracle's
    transcript, tree groups, patterns and reference hash count, and the mutants of one of them."""

    def __init__(self, name):
        import stark_prover_fast as SP
        T.use_c_backend()
        sec, log2_exp, k, air_seed, pinned, mutate = CONFIGS[name]
        self.name, self.k, self.sec, self.log2_exp = name, k, sec, log2_exp
        self.params = params_of(name)
        self.air, recipe = S.synth_air(self.params, seed=air_seed)
        self.air_words = self.air.to_words()
        self.claims, self.proofs, self.want, self.heights, self.shapes = [], [], [], [], []
        self.groups, self.patterns, self.ops = [], [], []
        for i, (log2_ph, seed) in enumerate(pinned):
            claim = CLAIMS[0]
            proof, _ = SP.prove(self.params, self.air, recipe, claim, log2_ph, seed=seed)
            proof = np.array([int(w) for w in proof], dtype=np.uint64)
            ok, err, samples, indices = TS.oracle(self.params, self.air, claim, proof)
            assert ok, (name, log2_ph, seed, err)
            gs = groups(self.params, log2_ph, indices)
            self.claims.append(claim)
            self.proofs.append(proof)
            self.want.append((samples, indices))
            self.heights.append(log2_ph)
            self.shapes.append(domain_shape(self.params, log2_ph))
            self.groups.append(gs)
            self.patterns.append([patterns(gh, lv) for gh, lv in gs])
            self.ops.append(merkle_ops(self.params, log2_ph, indices))
        self.mutated = mutate
        self._mutants = None

    @property
    def mutants(self):
        if self._mutants is None:
            i = self.mutated
            self._mutants = mutants(self.proofs[i], self.params, self.heights[i], self.want[i][1])
        return self._mutants

    def level_ops(self, i, level, lcw=True):
        return merkle_ops(self.params, self.heights[i], self.want[i][1], level, lcw)


@functools.lru_cache(maxsize=None)
def case(name):
    return IndexCase(name)


def coverage_gaps(cases):
    """What the module doc requires and the cases do not reach, as words; [] when all is reached."""
    gaps = []

    def need(what, found):
        if not found:
            gaps.append(what)

    for w in (1, 2, 4):
        g0 = [c.patterns[i][0] for c in cases if waves(c.k) == w for i in range(len(c.proofs))]
        for name in GROUP0:
            need(f"{name} in a group 0 at {w} wave(s)", any(p[name] for p in g0))
        need(f"no_dup at k >= 64 in a group 0 at {w} wave(s)",
             any(ps[0]["no_dup"] for c in cases if waves(c.k) == w and c.k >= 64 for ps in c.patterns))
        for tree in ("main", "aux", "quot", "fri0"):
            for kind in ("dup-first", "dup-last"):
                need(f"a {kind} mutant of {tree} at {w} wave(s)",
                     any(m.kind == kind and m.tree == tree for c in cases if waves(c.k) == w for m in c.mutants))
    later = [p for c in cases for ps in c.patterns for p in ps[2:]]  # group 1 + r, r >= 1
    for name in B_TREE:
        need(f"{name} in a b-tree of a round >= 1", any(p[name] for p in later))
    need("a dup mutant of a b-tree of a round >= 1",
         any(m.kind.startswith("dup") and m.tree.startswith("fri") and int(m.tree[3:]) >= 2
             for c in cases for m in c.mutants))
    need("digest mutants beside an unpaired odd and an unpaired even leaf",
         {"digest-odd", "digest-even"} <= {m.kind for c in cases for m in c.mutants})
    need("spread at k = 8", any(c.k == 8 and any(ps[0]["spread"] for ps in c.patterns) for c in cases))
    need("a proof of k = 256", any(c.k == 256 for c in cases))
    for c in cases:
        rs = [R for _, R in c.shapes]
        need(f"{c.name}: a proof with R = 1" if c.k > 2 else f"{c.name}: 7 to 10 FRI responses",
             1 in rs if c.k > 2 else all(7 <= R + 1 <= 10 for R in rs))
        need(f"{c.name}: a proof with R >= 3", max(rs) >= 3)
        need(f"{c.name}: a proof with R = 0", 0 in rs or c.k <= 8)
        need(f"{c.name}: length mutants of every structure",
             {m.tree for m in c.mutants if m.kind == "short"} >= {"main", "aux", "quot"} | {
                 f"fri{r}" for r in range(c.shapes[c.mutated][1] + 1)})
    need("k = 1 and 2: last codewords of 8 and 16",
         {1 << (h - R) for c in cases if c.k <= 2 for h, R in c.shapes} == {8, 16})
    return gaps


def assert_coverage(names=None):
    gaps = coverage_gaps([case(n) for n in (names or NAMES)])
    assert not gaps, "the index cases miss: " + "; ".join(gaps)
