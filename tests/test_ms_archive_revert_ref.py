"""No GPU: the record-by-record way back across a block (tests/ms_archive_revert_ref.py: revert_remove,
add_is_reversible, revert_add, slide_window_back in the reference's order) returns exactly the set before the block,
`AC.load_args(arch)`, from the set after it, `AC.load_args(advance(arch, adds, recs))`.  This is the truth the end state
of nhip_ms_archive_revert is held to on the GPU; the helper's panics are the reference's."""
import pytest

import ms_archive_cases as AC
import ms_archive_revert_cases as RC
import ms_archive_revert_ref as RR
import ms_update_cases as C


@pytest.fixture(scope="module")
def cases():
    return C.cases()


def _back(arch, adds, recs):
    before = AC.load_args(arch)
    after = AC.load_args(RC.advance(arch, adds, recs))
    got = RR.revert_block(after, adds, recs)
    assert got == ([tuple(l) for l in before[0]], before[1], before[2])
    return before, after


def test_one_block_from_the_set_of_600(cases):
    for arch, adds, recs in RC.one_block_group(cases):
        before, after = _back(arch, adds, recs)
        assert after != before


def test_the_small_sets(cases):
    blocks = RC.small_blocks(cases)
    assert [len(a.items) for a, _, _ in blocks] == [1, 8, 9, 255, 256] and any(recs for _, _, recs in blocks)
    for arch, adds, recs in blocks:
        _back(arch, adds, recs)


def test_a_slide_of_more_than_256_chunks(cases):
    arch, adds, recs = RC.long_slide(cases)
    before, after = _back(arch, adds, recs)
    assert len(after[1]) - len(before[1]) > 256


def test_the_chunk_edges_and_three_blocks(cases):
    arch, adds, recs, _ = RC.edge_block(cases)
    _back(arch, adds, recs)
    for arch, adds, recs in RC.three_blocks(cases) + [RC.fork_block(cases)]:
        _back(arch, adds, recs)


def test_a_block_that_was_not_the_last_panics(cases):
    """The reference's asserts: another block's additions, and records the set never took."""
    c = cases
    after = AC.load_args(RC.advance(c.arch, c.adds20, c.twelve))
    with pytest.raises(RR.RevertPanics):
        RR.revert_block(after, c.adds300[:20], c.twelve)
    with pytest.raises(RR.RevertPanics):
        RR.revert_block(AC.load_args(RC.advance(c.arch, c.adds20, c.twelve[:3])), c.adds20, c.twelve)
