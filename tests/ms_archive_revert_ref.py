"""Helper of tests/test_ms_archive_revert_ref.py and tests/test_gpu_ms_archive_revert.py — TEST HELPER ONLY (not
collected).  The reference's way back across a block, record by record and in its order, on the plain triple
`(leaves, chunks, window)` that `ms_archive_cases.load_args` gives: `ArchivalState::update_mutator_set`
(state/archival_state.rs:1293-1335) calls `revert_remove` for every removal record, then `add_is_reversible` and
`revert_add` for every addition in reverse (util_types/mutator_set/archival_mutator_set.rs:417-490); `Chunk::subtract`
(removal_record/chunk.rs:114-126) and `ActiveWindow::remove` / `slide_window_back` (active_window.rs:100-110) take one
copy of an index at a time and panic where there is none.  Nothing here knows the end state the device computes."""
import ms_ref as R


class RevertPanics(Exception):
    """Where the reference panics or an assert of its fails: the block was not the last one applied."""


def batch_index(n_leafs):
    return max(n_leafs - 1, 0) // R.BATCH_SIZE


def _take_one(words, x, what):
    if x not in words:
        raise RevertPanics(what)
    words.remove(x)  # the first match


def revert_remove(leaves, chunks, window, index_set):
    """`revert_remove` for one record's indices (a list of absolute indices)."""
    start = batch_index(len(leaves)) * R.CHUNK_SIZE
    difference = {}
    for index in index_set:
        if index >= start:
            _take_one(window, index - start, "ActiveWindow::remove: the index is not set")
        else:
            difference.setdefault(index // R.CHUNK_SIZE, []).append(index % R.CHUNK_SIZE)
    for ci, words in difference.items():
        for x in sorted(words):
            _take_one(chunks[ci], x, "Chunk::subtract: the index is not in the chunk")


def window_slides_back(removed_index):
    return removed_index != 0 and removed_index % R.BATCH_SIZE == 0


def revert_add(leaves, chunks, window, commitment):
    """`add_is_reversible`, then `revert_add`, for one addition."""
    if not leaves or tuple(leaves[-1]) != tuple(commitment):
        raise RevertPanics("Addition record must be in sync with block being rolled back.")
    removed = len(leaves) - 1
    leaves.pop()
    if not window_slides_back(removed):
        return
    last = chunks.pop()
    if any(x >= R.WINDOW_SIZE - R.CHUNK_SIZE for x in window):
        raise RevertPanics("slide_window_back: the last chunk of the window is not empty")
    window[:] = sorted([x + R.CHUNK_SIZE for x in window] + list(last))


def revert_block(state, adds, recs):
    """`(leaves, chunks, window)` after the block of `adds` (items) and `recs` (ms_ref records), taken back across it:
    a new triple; `state` stays as it is."""
    leaves, chunks, window = [tuple(l) for l in state[0]], [list(ch) for ch in state[1]], list(state[2])
    for r in recs:
        revert_remove(leaves, chunks, window, r.absolute_indices.to_array())
    for it in reversed(list(adds)):
        revert_add(leaves, chunks, window, R.aocl_leaf(*it))
    return leaves, chunks, window
