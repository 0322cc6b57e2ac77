"""GPU rules 2.a-2.l from a block file's bytes (k_guesser_fee_records, k_blk_ms_rules and the two apply passes behind
nhip_blk_guesser_fee_records / nhip_blk_ms_check) against the CPU restatement tests/blk_ms_ref.py, never against
themselves, with pow tree height 10 and block proofs of a dozen words.  One real chain on an archival mutator set
(blocks whose inputs spend earlier outputs, packed; every body's accumulator the true one), its mutants and every
expected value are built once per module and left unchanged.  Equality is exact everywhere.

The chain's AOCL leaf counts are chosen for the link: block 0 is at height 0 (no guesser records); block 1's body has
15 leaves, so its second guesser record (leaf 16) slides the window; block 2's has 24, so its first one does; block
3's has 30, so neither does (and its child's first output does).  The children of blocks 1 and 2 each spend a leaf
with an index in the chunk that only that slide made inactive."""
import ctypes
import random

import numpy as np
import pytest

import blk_ms_ref as X
import ms_apply_ref as A
import ms_pack_cases as PC
import ms_pack_ref as K
import ms_ref as R

pytestmark = pytest.mark.gpu

P, H = X.P, 10
TS = ((1 << 63) + 5, 2, P - 1, 4, 5), (6, (1 << 63) | 12345, 8, 9, P - 2)   # both with a word >= 2^63
BIG_FEE = (7 << 96) + (5 << 64) + (9 << 32) + 3                             # all four limbs non-zero


def _dig(x):
    return tuple(int(v) for v in x)


class World:
    """The chain, the mutant pairs on it and what the restatement says of each."""

    def __init__(self):
        c = self.chain = X.Chain(TS, seed=2931, tree_height=H)
        c.add(n_outputs=7, fee=5)                                                  # height 0: its fee makes no records
        c.add(n_outputs=8, fee=12345, coinbase=X.block_subsidy(1))                 # 15 leaves; odd fee; coinbase = subsidy
        assert [len(a.items) for a in c.arch_body] == [7, 15] and c.num_leafs == 17
        self.slid = [c.unspent(1, touching_chunk=1)[0]]
        c.add(n_outputs=7, spend=self.slid + c.unspent(1), fee=BIG_FEE)            # 24 leaves: slides on the first record
        assert len(c.arch_body[2].items) == 24 and c.num_leafs == 26
        self.slid.append(c.unspent(1, touching_chunk=2)[0])
        c.add(n_outputs=4, spend=[self.slid[1]], fee=1, timestamp=P - 1)           # 30 leaves; p - 1: the time lock wraps
        assert len(c.arch_body[3].items) == 30 and c.num_leafs == 32
        c.add(n_outputs=3, spend=c.unspent(2), fee=0)                              # its first output slides the window
        c.add(n_outputs=2, spend=c.unspent(3), fee=2)
        self.n_base = len(c.blocks)
        # pairs: (name, parent block, child block, parent hash, archival set behind the parent's accumulator after)
        self.pairs = [("chain%d" % i, c.blocks[i - 1], c.blocks[i], c.hashes[i - 1], c.arch_after[i - 1], None)
                      for i in range(1, self.n_base)]
        self.enc = list(c.enc)
        self.parent_of = [-1] + list(range(self.n_base - 1))
        self.names = ["genesis"] + [p[0] for p in self.pairs]
        tip = self.n_base - 1
        kernel = lambda b: b["body"]["transaction_kernel"]  # noqa: E731

        def child(name, parent=tip, chain=c, max_num=None, **kw):
            """One more block on `chain`'s tip, not kept; its pair's parent is block `parent` of the buffer."""
            b, enc, _ = chain.add(keep=False, **kw)
            self.pairs.append((name, chain.blocks[-1], b, chain.hashes[-1], chain.arch_after[-1], max_num))
            self.enc.append(enc)
            self.parent_of.append(parent)
            self.names.append(name)

        def ed(**fields):
            return lambda b: kernel(b).update(fields)

        ts = 1_700_000_000_000 + 600_000 * self.n_base   # the header timestamp of a child of the tip
        # 2.a: every unpack error class of ms_pack_cases
        for name, (packed, status) in sorted(PC.mutants().items()):
            if status:
                child("unpack_" + name, edit=ed(inputs=X.from_records(packed)))
        # 2.b: the slid chunk absent (records made against the parent's body accumulator, before the slide) is built
        # below on the forks; here a corrupted path and an already-removed record
        touching = [l for l in range(c.num_leafs) if l not in c.spent
                    and any(len(p) for _, p, _ in c.arch.removal_record(l).target_chunks)]
        assert touching, "no unspent leaf with a non-empty chunk path"

        def corrupt_path(b):
            for rr in kernel(b)["inputs"]:
                for e, (k, path, rel) in enumerate(rr["chunks"]):
                    if path:
                        path = [tuple(path[0][:2]) + ((path[0][2] + 1) % P,) + tuple(path[0][3:])] + list(path[1:])
                        rr["chunks"][e] = (k, path, rel)
                        return
            raise AssertionError("no structure digest to corrupt")
        child("bad_path", spend=touching[:1], edit=corrupt_path)
        child("already_removed", spend=[sorted(c.spent)[0]])
        # 2.c, and 2.c before 2.f
        free = c.unspent(4)
        child("two_equal_records", spend=[free[0], free[1], free[0]])
        child("duplicate_and_timestamp", spend=[free[0], free[0]], edit=ed(timestamp=ts + 1))
        # 2.d: three hand-made records in the active window (no dictionary needed); the third's indices are the first's
        # and the second's, so it is removable before the block and not once they are applied
        base = c.arch.msa().batch_index * R.CHUNK_SIZE + 100
        one, two = R.IndexSet(base, [3 * k for k in range(45)]), R.IndexSet(base + 1000, [3 * k for k in range(45)])
        both = R.IndexSet(base, [3 * k for k in range(22)] + [1000 + 3 * k for k in range(22, 45)])
        child("update_impossible", records=[R.Record(one), R.Record(two), R.Record(both)])
        # 2.e: one peak word, the leaf count, one window word
        def peak(b):
            first = b["body"]["aocl"]["peaks"][0]
            b["body"]["aocl"]["peaks"][0] = (first[0] ^ 1,) + tuple(first[1:])

        def leafs(b): b["body"]["swbf_inactive"]["leaf_count"] += 1  # noqa: E704
        def window(b): b["body"]["swbf_active"][-1] += 1  # noqa: E704
        child("wrong_peak", spend=free[:1], edit=peak)
        child("wrong_leaf_count", edit=leafs)
        child("wrong_window_word", spend=free[:2], edit=window)
        # 2.f-2.i; the block's height is the tip's + 1
        child("timestamp_equal", edit=ed(timestamp=ts))
        child("timestamp_plus_one", edit=ed(timestamp=ts + 1))
        sub = X.block_subsidy(self.n_base)
        child("coinbase_is_subsidy", coinbase=sub)
        child("coinbase_too_big", coinbase=sub + 1)
        child("coinbase_negative", coinbase=-1)
        child("fee_negative", fee=-1)
        child("coinbase_negative_and_fee_negative", coinbase=-1, fee=-1)
        # 2.j with a limit of its own, 2.k and 2.l at the real one
        child("inputs_at_limit", spend=free[:3], max_num=3)
        child("inputs_over_limit", spend=free[:3], max_num=2)
        child("outputs_at_limit", n_outputs=X.MAX_NUM)
        child("outputs_over_limit", n_outputs=X.MAX_NUM + 1)
        child("announcements_at_limit", edit=ed(announcements=[[]] * X.MAX_NUM))
        child("announcements_over_limit", edit=ed(announcements=[[7]] + [[]] * X.MAX_NUM))
        # forks: a parent of their own in the buffer, then its child
        def fork(name, upto, parent_kw, child_kw, records_from_body=None):
            f = c.fork(upto, seed=len(self.enc))
            if parent_kw is not None:
                f.add(**parent_kw)
                self.enc.append(f.enc[-1])
                self.parent_of.append(upto - 1)
                self.names.append(name + "_parent")
                self.pairs.append((name + "_parent", f.blocks[-2], f.blocks[-1], f.hashes[-2], f.arch_after[-2], None))
                at = len(self.enc) - 1
            else:
                at = upto - 1
            if records_from_body is not None:
                child_kw = dict(child_kw, records=[f.arch_body[-1].removal_record(l) for l in records_from_body])
            child(name, parent=at, chain=f, **child_kw)

        fork("parent_fee_negative", self.n_base, dict(n_outputs=1, fee=-1), dict(n_outputs=1))
        def drop_peak(b): b["body"]["aocl"]["peaks"].pop()  # noqa: E704
        fork("parent_msa_inconsistent", self.n_base, dict(n_outputs=1, edit=drop_peak), dict(n_outputs=1))
        # the children of blocks 1 and 2 with their records made before the slide: the slid chunk is absent
        fork("absent_chunk_slide_on_second", 2, None, dict(n_outputs=7), records_from_body=[self.slid[0]])
        fork("absent_chunk_slide_on_first", 3, None, dict(n_outputs=4), records_from_body=[self.slid[1]])

        self.data = b"".join(self.enc)
        self.n = len(self.enc)
        self.want = {}
        for name, parent, b, ph, arch, max_num in self.pairs:
            mx = (X.MAX_NUM,) * 3 if max_num is None else (max_num, X.MAX_NUM, X.MAX_NUM)
            self.want[name] = X.pair_outcome(parent, b, ph, TS, arch, c.triples, mx)
        self.max_num_of = {name: m for name, _, _, _, _, m in self.pairs if m is not None}

@pytest.fixture(scope="module")
def world():
    return World()


def _records(data):
    from neptune_hip import blocks as NB
    return NB.blocks_from_bytes(data, H)


def _links(ctx, w, data, recs, parent_of, names, digests=None):
    """nhip_blk_ms_check over the buffer; the pairs with a limit of their own are checked in a call of their own."""
    from neptune_hip import blocks as NB
    got = NB.mutator_set_links(ctx, data, recs, NB.ms_params(TS, H), parent_of, digests)
    for limit in sorted({w.max_num_of[n] for n in names if n in w.max_num_of}):
        p = NB.ms_params(TS, H)
        p.max_num_inputs = limit
        other = NB.mutator_set_links(ctx, data, recs, p, parent_of, digests)
        for i, name in enumerate(names):
            if w.max_num_of.get(name) == limit:
                got[i] = other[i]
    return got


def test_restatement_covers_every_status(world):
    """The fixture itself: the chain is accepted, and the mutants reach every status the entry point can give."""
    w = world
    for i in range(1, w.n_base):
        assert w.want["chain%d" % i] == (X.OK, R.OK, None), i
    seen = {s for s, _, _ in w.want.values()}
    assert seen == set(range(16)) - {X.SKIPPED}, sorted(seen)
    assert w.want["update_impossible"] == (X.UPDATE_IMPOSSIBLE, A.UPDATE_IMPOSSIBLE, 2)
    assert {ms for s, ms, _ in w.want.values() if s == X.UNPACK} == set(range(10, 20))
    for name in ("timestamp_equal", "coinbase_is_subsidy", "inputs_at_limit", "outputs_at_limit", "announcements_at_limit"):
        assert w.want[name] == (X.OK, R.OK, None), name
    assert w.want["absent_chunk_slide_on_second"] == w.want["absent_chunk_slide_on_first"] == \
        (X.REMOVAL_RECORDS_VALIDITY, R.ABSENT_CHUNK, 0)
    assert w.want["duplicate_and_timestamp"][0] == X.REMOVAL_RECORDS_UNIQUENESS
    assert w.want["coinbase_negative_and_fee_negative"][0] == X.NEGATIVE_COINBASE
    assert w.want["bad_path"][:2] == (X.REMOVAL_RECORDS_VALIDITY, R.BAD_MMR_PATH)
    assert w.want["already_removed"][:2] == (X.REMOVAL_RECORDS_VALIDITY, R.ALREADY_REMOVED)
    # the slid chunk is in the dictionaries of the accepted children, and only the slide made it inactive
    for i, chunk in ((2, 1), (3, 2)):
        _, recs = K.try_unpack_status(X.to_records(w.chain.blocks[i]["body"]["transaction_kernel"]["inputs"]))
        assert any(ci == chunk for r in recs for ci, _, _ in r.target_chunks)
        assert X.body_msa(w.chain.blocks[i - 1]).batch_index == chunk
        assert w.chain.arch_after[i - 1].msa().batch_index == chunk + 1


def test_guesser_fee_records_equal_the_restatement(ctx, world):
    from neptune_hip import blocks as NB
    w = world
    recs = _records(w.data)
    got = NB.guesser_fee_addition_records(ctx, w.data, recs, TS, pow_tree_height=H)
    blocks = w.chain.blocks + [b for _, _, b, _, _, _ in w.pairs[w.n_base - 1:]]
    assert len(got) == len(blocks) == w.n
    digests = NB.block_digests(ctx, w.data, recs, H)
    for i, (b, (status, records)) in enumerate(zip(blocks, got)):
        try:
            want = (X.GUESSER_OK, X.guesser_fee_addition_records(b, _dig(digests[i]), TS))
        except X.NegativeFee:
            want = (X.GUESSER_NEGATIVE_FEE, [])
        assert (status, records) == want, w.names[i]
    assert [len(r) for _, r in got[:w.n_base]] == [0] + [2] * (w.n_base - 1)
    assert sum(s == X.GUESSER_NEGATIVE_FEE for s, _ in got) == 3
    # with the digests passed in: the same records
    assert NB.guesser_fee_addition_records(ctx, w.data, recs, TS, digests, pow_tree_height=H) == got
    # the base chain's digests are the restatement's, so its records stand on block_chain_ref.block_hash
    assert [_dig(d) for d in digests[:w.n_base]] == [_dig(h) for h in w.chain.hashes]


def test_every_pair_equals_the_restatement(ctx, world):
    w = world
    recs = _records(w.data)
    got = _links(ctx, w, w.data, recs, w.parent_of, w.names)
    assert got[0] == (X.SKIPPED, R.OK, None)
    for i in range(1, w.n):
        assert got[i] == w.want[w.names[i]], (w.names[i], got[i], w.want[w.names[i]])
    assert all(got[i] == (X.OK, R.OK, None) for i in range(1, w.n_base))


def test_accepted_pairs_equal_the_two_existing_calls(ctx, world):
    """accumulator_after, then mutator_set_update_valid_packed, fed with the restatement's decode of the blocks."""
    from neptune_hip import blocks as NB
    import neptune_hip.mutator_set as MS
    w = world

    def lib_msa(m):
        return MS.MutatorSetAccumulator(MS.MmrAccumulator(list(m.aocl.peaks), m.aocl.num_leafs),
                                        MS.MmrAccumulator(list(m.swbf_inactive.peaks), m.swbf_inactive.num_leafs),
                                        list(m.swbf_active))
    for i in range(1, w.n_base):
        parent, b = w.chain.blocks[i - 1], w.chain.blocks[i]
        guesser = X.guesser_fee_addition_records(parent, w.chain.hashes[i - 1], TS)
        before = NB.accumulator_after(ctx, lib_msa(X.body_msa(parent)), guesser)
        k = b["body"]["transaction_kernel"]
        got = NB.mutator_set_update_valid_packed(ctx, before, PC.to_library(X.to_records(k["inputs"])),
                                                 [tuple(d) for d in k["outputs"]], lib_msa(X.body_msa(b)))
        assert got == (True, MS.OK), i


def test_one_pair_per_call_equals_one_call(ctx, world):
    from neptune_hip import blocks as NB
    w = world
    pick = [1, 2, 3] + [i for i, n in enumerate(w.names) if n in ("bad_path", "two_equal_records", "wrong_peak",
                                                                  "coinbase_too_big", "absent_chunk_slide_on_first",
                                                                  "parent_fee_negative", "unpack_index_too_big")]
    assert len(pick) == 10
    recs = _records(w.data)
    for i in pick:
        pair = [recs[w.parent_of[i]], recs[i]]
        got = NB.mutator_set_links(ctx, w.data, pair, TS, [-1, 0], pow_tree_height=H)
        assert got[0] == (X.SKIPPED, R.OK, None) and got[1] == w.want[w.names[i]], w.names[i]


def test_shuffled_buffer_and_skipped_pairs(ctx, world):
    w = world
    order = list(range(w.n))
    random.Random(5).shuffle(order)
    data = b"".join(w.enc[i] for i in order)
    where = {old: new for new, old in enumerate(order)}
    parent_of = [-1 if w.parent_of[old] < 0 else where[w.parent_of[old]] for old in order]
    names = [w.names[old] for old in order]
    skip = [k for k, name in enumerate(names) if name in ("chain2", "wrong_peak", "fee_negative")]
    for k in skip:
        parent_of[k] = -1
    got = _links(ctx, w, data, _records(data), parent_of, names)
    for k, name in enumerate(names):
        want = (X.SKIPPED, R.OK, None) if parent_of[k] < 0 else w.want[name]
        assert got[k] == want, name


def test_130_pairs_and_digests_passed_in(ctx, world):
    from neptune_hip import blocks as NB
    w = world
    small = [i for i in range(w.n) if len(w.enc[i]) < 20_000]   # without the two blocks of 16,384 outputs
    assert len(small) >= 40 and all(w.parent_of[i] in small or w.parent_of[i] < 0 for i in small)
    copies = 130 // (len(small) - 1) + 1
    data = b"".join(w.enc[i] for i in small) * copies
    where = {old: new for new, old in enumerate(small)}
    parent_of, names = [], []
    for c in range(copies):
        for old in small:
            # copies after the first stand on the first copy's parents: a pair spans workgroups
            parent_of.append(-1 if w.parent_of[old] < 0 else where[w.parent_of[old]] + (0 if c % 2 else c * len(small)))
            names.append(w.names[old])
    recs = _records(data)
    assert sum(p >= 0 for p in parent_of) >= 130
    got = _links(ctx, w, data, recs, parent_of, names)
    for k, name in enumerate(names):
        assert got[k] == ((X.SKIPPED, R.OK, None) if parent_of[k] < 0 else w.want[name]), (k, name)
    digests = NB.block_digests(ctx, data, recs, H)
    assert _links(ctx, w, data, recs, parent_of, names, digests) == got
    # digests that are not the blocks': the records change, and with them every accepted pair's accumulator
    wrong = digests.copy()
    wrong[:, 0] ^= np.uint64(1)
    bad = NB.mutator_set_links(ctx, data, recs, TS, parent_of, wrong, pow_tree_height=H)
    assert bad[1] == got[1] == (X.OK, R.OK, None)               # the parent at height 0 has no records
    assert bad[2] == (X.UPDATE_INTEGRITY, A.UPDATE_MISMATCH, None) and got[2] == (X.OK, R.OK, None)


def test_argument_errors_leave_the_outputs_untouched(ctx, world):
    from neptune_hip import _lib, blocks as NB
    w = world
    data = b"".join(w.enc[:3])
    recs = _records(data)
    buf = np.frombuffer(data, dtype=np.uint8)
    scanned = ctypes.cast(NB._scanned(recs), ctypes.c_void_p)
    p = NB.ms_params(TS, H)
    status, ms, rec_n, gst = (np.full(3, 0xAA, dtype=np.uint8) for _ in range(4))
    bad = np.full(3, 0xAAAA, dtype=np.uint64)
    rec = np.full((3, 2, 5), 0xAAAA, dtype=np.uint64)

    def check(parent_of, n_bytes=len(data), blocks=scanned, status_ptr=status.ctypes.data, params=p):
        par = np.asarray(parent_of, dtype=np.int64)
        return ctx.lib.nhip_blk_ms_check(ctx.handle, buf.ctypes.data, n_bytes, ctypes.byref(params), blocks, 3,
                                         par.ctypes.data, None, status_ptr, ms.ctypes.data, bad.ctypes.data)

    def guesser(n_bytes=len(data), blocks=scanned, rec_ptr=rec.ctypes.data):
        return ctx.lib.nhip_blk_guesser_fee_records(ctx.handle, buf.ctypes.data, n_bytes, ctypes.byref(p), blocks, 3, None,
                                                    rec_ptr, rec_n.ctypes.data, gst.ctypes.data)
    assert check([-1, 3, 1]) == _lib.NHIP_ERR_ARG and check([-2, 0, 1]) == _lib.NHIP_ERR_ARG
    assert check([-1, 0, 1], status_ptr=None) == _lib.NHIP_ERR_ARG and check([-1, 0, 1], blocks=None) == _lib.NHIP_ERR_ARG
    assert guesser(rec_ptr=None) == _lib.NHIP_ERR_ARG and guesser(blocks=None) == _lib.NHIP_ERR_ARG
    tall = NB.ms_params(TS, 33)
    assert check([-1, 0, 1], params=tall) == _lib.NHIP_ERR_ARG
    # a buffer shorter than the last block is the caller's error; a BlockProof variant that does not exist is a block
    # that does not parse
    assert check([-1, 0, 1], n_bytes=len(data) - 9) == _lib.NHIP_ERR_ARG and guesser(n_bytes=len(data) - 9) == _lib.NHIP_ERR_ARG
    good = buf
    broken = bytearray(data)
    at = len(data) - 8 * 12 - 8 - 4
    assert int.from_bytes(broken[at:at + 4], "little") == 2 and int.from_bytes(broken[at + 4:at + 12], "little") == 12
    broken[at] = 9
    buf = np.frombuffer(bytes(broken), dtype=np.uint8)
    assert check([-1, 0, 1]) == _lib.NHIP_ERR_DECODE and guesser() == _lib.NHIP_ERR_DECODE
    buf = good
    for a in (status, ms, rec_n, gst):
        assert (a == 0xAA).all()
    assert (bad == 0xAAAA).all() and (rec == 0xAAAA).all()
    assert check([-1, 0, 1]) == _lib.NHIP_OK and list(status) == [X.SKIPPED, X.OK, X.OK]
    assert guesser() == _lib.NHIP_OK and list(rec_n) == [0, 2, 2] and list(gst) == [0, 0, 0]
    # no blocks: nothing to do, nothing read
    assert ctx.lib.nhip_blk_ms_check(ctx.handle, None, 0, ctypes.byref(p), None, 0, None, None, None, None, None) == _lib.NHIP_OK


def test_validate_chain_file_names_the_first_failing_rule(ctx, tmp_path):
    """Rules 0.x, 1.x and 2.x over one file, on the testnet with mock proofs: blocks two reset intervals apart at the
    genesis difficulty need no work (has_proof_of_work's reset branch), a block proof is the one-word valid mock, and
    every header links to the block before it."""
    from neptune_hip import blocks as NB
    from neptune_hip import verifier as V
    import bincode_ref as B
    import block_chain_ref as C
    import mast_ref as M
    import tip5_ref as T
    T.use_c_backend()
    d = lambda k: [k, 3 * k, 5 * k, 7 * k, 11 * k]  # noqa: E731
    progs = V.ConsensusPrograms(d(1001), d(1002), d(1003), d(1004), single_proof=d(1005), block_program=d(1006))
    genesis_difficulty, step, t0 = [100_000, 0, 0, 0, 0], 2 * 588_000, 1_700_000_000_000
    c = X.Chain(TS, seed=2977, tree_height=H, proof_words=1)

    def linked(extra=None):
        def edit(b):
            hd, k = b["header"], b["body"]["transaction_kernel"]
            b["body"]["block_mmr_accumulator"] = {"leaf_count": 0, "peaks": []}
            if c.blocks:
                parent = c.blocks[-1]
                hd["prev_block_digest"] = list(c.hashes[-1])
                b["body"]["block_mmr_accumulator"] = C.mmr_append(parent["body"]["block_mmr_accumulator"], c.hashes[-1])
                hd["cumulative_proof_of_work"] = C.pow_add(parent["header"]["cumulative_proof_of_work"],
                                                           parent["header"]["difficulty"])
            hd["difficulty"] = list(genesis_difficulty)
            b["proof"] = [V.MOCK_VALID[0]]
            if extra:
                extra(b)
            claim = V.single_proof_claim(M.mast_hash(B.kernel_mast_sequences(k)), progs)
            b["appendix"] = [{"program_digest": list(claim.program_digest), "version": claim.version,
                              "input": list(claim.input), "output": list(claim.output)}]
        return edit

    def late_kernel(b): b["body"]["transaction_kernel"]["timestamp"] += 1  # noqa: E704

    def wrong_pow(b):
        b["header"]["cumulative_proof_of_work"][0] ^= 1
        b["body"]["transaction_kernel"]["coinbase"] = -1

    def bad_proof(b):
        b["proof"] = [V.MOCK_INVALID[0]]
        b["body"]["transaction_kernel"]["fee"] = -1
    plan = [(dict(n_outputs=7), None), (dict(n_outputs=8, fee=9), None), (dict(n_outputs=2, fee=3), None),
            (dict(n_outputs=1), late_kernel), (dict(n_outputs=1), wrong_pow), (dict(n_outputs=1), bad_proof)]
    for i, (kw, extra) in enumerate(plan):
        spend = c.unspent(1) if i >= 2 else ()
        c.add(spend=spend, timestamp=t0 + step * i, edit=linked(extra), **kw)
    path = tmp_path / "blk0.dat"
    path.write_bytes(b"".join(c.enc))
    got = NB.validate_chain_file(ctx, str(path), V.Verifier(ctx, None), progs, TS, now=t0 + step * len(plan),
                                 network=V.Network.TESTNET_MOCK, pow_tree_height=H)
    assert got == [None, None, None, "2.f", "0.f", V.PROOF_VALIDITY]
    # the three passes it is made of, on the same bytes
    data = path.read_bytes()
    recs = NB.blocks_from_bytes(data, H)
    links = NB.chain_links(ctx, data, recs, V.Network.TESTNET_MOCK, t0 + step * len(plan), pow_tree_height=H)
    assert [s for s, _ in links] == [NB.LINK_SKIPPED, NB.LINK_OK, NB.LINK_OK, NB.LINK_OK, NB.LINK_CUMULATIVE_POW, NB.LINK_OK]
    assert all(ok for _, ok in links[1:])
    ms = NB.mutator_set_links(ctx, data, recs, TS, pow_tree_height=H)
    assert [s for s, _, _ in ms] == [X.SKIPPED, X.OK, X.OK, X.TRANSACTION_TIMESTAMP, X.NEGATIVE_COINBASE, X.NEGATIVE_FEE]
