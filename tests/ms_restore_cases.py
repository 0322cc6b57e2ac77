"""Helpers of tests/test_gpu_ms_restore_shape.py and tests/test_gpu_ms_store_restored.py — TEST HELPER ONLY (not
collected): index sets built by hand so that every decision of the restore plan is reached.  Truth is the host plan
(`restore_plan`), the two-call path and `ms_ref`, never the calls under test."""
import ms_ref as R

NONE = None
C = R.CHUNK_SIZE


def edge_sets(n_leafs):
    """`[(label, minimum, distances, leaf index or None)]` for an archive of n_leafs leaves; bad witnesses lie
    between good ones, so that a wrong scan shifts a neighbour."""
    b = max(n_leafs - 1, 0) // R.BATCH_SIZE
    last = max(n_leafs - 1, 0)
    step = lambda first, d: [first + t * d for t in range(45)]  # noqa: E731
    out = [("one chunk, key 0", 0, step(0, 1), 0)]
    if b:
        out.append(("key b - 1 alone", (b - 1) * C, step(0, 3), last))
    out += [
        ("45 distinct chunks", 0, step(0, C), NONE),
        ("chunk b + 256", (b + 256) * C, step(0, 1), 0),
        ("all at or above b", b * C, step(0, C), 0),
    ]
    if b >= 2:
        out.append(("straddles b", (b - 2) * C + 5, step(0, 1000), 1 if n_leafs > 1 else 0))
        out.append(("keys 0 and b - 1", 0, [0 if t % 3 else (b - 1) * C + t for t in range(45)], last))
    out += [
        ("a, c, a, c", 0, [3 * C + t if t % 2 else t for t in range(45)], last),
        ("past the AOCL and saturating", 2 ** 128 - 5, [9] * 45, n_leafs),
        ("descending", 0, [(44 - t) * C for t in range(45)], NONE),
        ("chunk b + 255", (b + 255) * C, step(0, 90), 0),
        ("the carry into the high word", 2 ** 64 - 1, [1] * 45, 0),
        ("the last index of chunk b + 255", (b + 255) * C, step(C - 45, 1), last),
        ("one past chunk b + 255", (b + 255) * C, step(C - 44, 1), last),
        ("a high word", 2 ** 64, step(0, 1), 0),
        ("leaf index 0", 5, step(0, 7), 0),
        ("the wrap", 2 ** 128 - 5, [9] * 45, 0),
        ("leaf index n - 1", 5, step(0, 7), last),
        ("leaf index n", 5, step(0, 7), n_leafs),
        ("no leaf index", 5, step(0, 7), NONE),
        ("leaf index 2^64 - 2", 5, step(0, 7), 2 ** 64 - 2),
        ("one chunk again", C, step(7, 2), last),
    ]
    return out


def cycled(edges, count, start=0):
    return [edges[(start + k) % len(edges)] for k in range(count)]


def as_args(witnesses):
    """`(index sets, leaf indices)` as `restore_plan` and `Archive.restore_shape` take them"""
    from neptune_hip.mast import AbsoluteIndexSet
    return [AbsoluteIndexSet(mn, list(d)) for _, mn, d, _ in witnesses], [li for _, _, _, li in witnesses]
