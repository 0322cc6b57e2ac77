"""Helpers of tests/test_ms_archive_plan.py (host plan, no GPU) and tests/test_gpu_ms_archive.py — TEST HELPER ONLY
(not collected).  Truth is `ms_ref.Archival` / `ms_ref.ArchivalMmr`, which derive everything from scratch; the sets
come from tests/ms_update_cases.py, imported and left unchanged."""
import random

import ms_ref as R

NONE = 2 ** 64 - 1
TAIL_NODES = 256  # NHIP_MS_ARCHIVE_TAIL_NODES (tests/test_ms_archive_host.py checks it against the header)


def batch_index(n_leafs):
    return max(n_leafs - 1, 0) // R.BATCH_SIZE


def load_args(arch):
    """`Archive.load`'s arguments for an `Archival` set: leaves, the chunks below the batch index, the window."""
    msa = arch.msa()
    leaves = [R.aocl_leaf(*it) for it in arch.items]
    chunks = [list(arch.bloom.get(ci, [])) for ci in range(msa.batch_index)]
    return leaves, chunks, list(msa.swbf_active)


def random_archive(n_leafs, seed):
    """Random leaf digests, chunks of random lengths 0 to 13 (length 0 and odd lengths among them wherever there are
    three chunks or more) and a random window: `(leaves, chunks, window)`."""
    rng = random.Random(seed)
    leaves = [tuple(rng.randrange(R.P) for _ in range(5)) for _ in range(n_leafs)]
    lengths = [rng.randrange(14) for _ in range(batch_index(n_leafs))]
    for k, forced in enumerate((0, 13, 1)):
        if len(lengths) >= 3:
            lengths[(7 * k + 1) % len(lengths)] = forced
    chunks = [sorted(rng.randrange(R.CHUNK_SIZE) for _ in range(l)) for l in lengths]
    window = sorted(rng.randrange(R.WINDOW_SIZE) for _ in range(rng.randrange(1, 40)))
    return leaves, chunks, window


def model_mmrs(leaves, chunks):
    return R.ArchivalMmr(leaves), R.ArchivalMmr([R.chunk_hash(ch) for ch in chunks])


def lib_index_set(s):
    from neptune_hip.mast import AbsoluteIndexSet
    return AbsoluteIndexSet(s.minimum, list(s.distances))


def plain_chunks(tc):
    return [(int(ci), [tuple(int(x) for x in d) for d in path], [int(x) for x in c.relative_indices]) for ci, path, c in tc]


def shape_of(tc):
    """keys, path lengths and chunk lengths of a dictionary"""
    return [int(ci) for ci, _, _ in tc], [len(p) for _, p, _ in tc], [len(c.relative_indices) for _, _, c in tc]


def plan_shapes(o, n):
    """`restore_plan`'s arrays as per-witness `(aocl path length, keys, path lengths, chunk lengths)`"""
    out = []
    for i in range(n):
        lo, hi = int(o["entry_off"][i]), int(o["entry_off"][i + 1])
        out.append((int(o["aocl_path_off"][i + 1]) - int(o["aocl_path_off"][i]),
                    [int(x) for x in o["chunk_index"][lo:hi]],
                    [int(o["path_off"][e + 1]) - int(o["path_off"][e]) for e in range(lo, hi)],
                    [int(o["rel_off"][e + 1]) - int(o["rel_off"][e]) for e in range(lo, hi)]))
    return out
