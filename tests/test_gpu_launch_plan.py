"""The launch schedule (csrc/stark_launch_plan.hpp) end to end: batches of 1, 5, 33, 65 and 513 proofs
(the pool's proofs and one mutant, repeated) launched directly on two streams, on one stream, replayed
from a graph, with the climb-from rule off and forced, and with each Fiat-Shamir form forced.  Every
mode gives the direct two-stream run's verdicts, and launches as many Merkle hash kernels as the code
did before the schedule was split from the enqueue (LAUNCHES, recorded there).  A direct launch reports
every phase, a replayed one none; a timed one reports the hash and row launches' own durations."""
import numpy as np
import pytest

import bench
import stark_ref as S

pytestmark = pytest.mark.gpu

PHASES = ("ms_device_decode", "ms_fiat_shamir", "ms_row_hash", "ms_merkle", "ms_merkle_hash", "ms_ood_air", "ms_fri",
          "ms_deep", "ms_device_total")
MODES = ("two_streams", "timed", "graph", "climb_from_0", "climb_from_4096", "fs_row", "fs_pair", "fs_quad",
         "one_stream", "one_stream_timed", "one_stream_graph")
# stats()["merkle_hash_launches"] per batch size, in MODES order: recorded by running _launches() below
# on commit f6e89ce (the parent of the commit that split the schedule from the enqueue)
LAUNCHES = {
    1: [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
    5: [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
    33: [16, 16, 16, 16, 12, 16, 16, 16, 16, 16, 16],
    65: [17, 17, 17, 17, 14, 17, 17, 17, 17, 17, 17],
    513: [19, 19, 19, 19, 16, 19, 19, 19, 19, 19, 19],
}


@pytest.fixture(scope="module")
def pool():
    return _pool()


def _pool():
    air_words, pool = bench.load_pool()
    hs = sorted(pool)
    claims = [pool[h]["claim"] for h in hs]
    proofs = [np.asarray(pool[h]["proof"], dtype=np.uint64) for h in hs]
    bad = proofs[2].copy()
    lo, hi = pool[hs[2]]["main_rows"]
    bad[(lo + hi) // 2] = np.uint64((int(bad[(lo + hi) // 2]) + 1) % S.P)
    return [int(w) for w in air_words], claims + [claims[2]], proofs + [bad]


def _launches(ctx, pool, n):
    """Run every mode on an n-proof batch; the Merkle hash launches of each, in MODES order."""
    import neptune_hip._lib as L
    import neptune_hip.stark as NS
    lib = L.load()
    air_words, claims, proofs = pool
    m = len(proofs)
    b = NS.Batch(ctx, NS.Air(air_words), NS.Stark.default(), [NS.Claim(*claims[i % m]) for i in range(n)],
                 [proofs[i % m] for i in range(n)])
    want = [i % m != m - 1 for i in range(n)]  # the mutant is the pool's last entry
    out = {}

    def run(mode, phases):
        v, ok = b.run()
        s = b.stats()
        assert [bool(x) for x in v] == want and ok == all(want), mode
        if phases:
            assert all(s[f] > 0 for f in PHASES), (mode, {f: s[f] for f in PHASES})
        else:
            assert all(s[f] == 0 for f in PHASES), (mode, {f: s[f] for f in PHASES})
        out[mode] = s["merkle_hash_launches"]
        return s

    try:
        for streams, base in ((2, "two_streams"), (1, "one_stream")):
            b.set_streams(streams)
            s = run(base, True)
            assert s["ms_mp_hash_exec"] == 0 and s["ms_row_hash_exec"] == 0
            b.set_launch_timing(True)
            s = run("timed" if streams == 2 else "one_stream_timed", True)
            assert s["ms_mp_hash_exec"] > 0 and s["ms_row_hash_exec"] > 0
            b.set_launch_timing(False)
            b.set_graph(True)
            run("graph" if streams == 2 else "one_stream_graph", False)
            run("graph" if streams == 2 else "one_stream_graph", False)  # the replay after the capture's launch
            b.set_graph(False)
            if streams == 1:
                break
            for ops in (0, 4096):
                assert lib.nhip_set_climb_from_ops(ops) == 0
                run(f"climb_from_{ops}", True)
            assert lib.nhip_set_climb_from_ops(-1) == 0
            for form, name in enumerate(("fs_row", "fs_pair", "fs_quad")):
                NS.set_fs_form(form)
                run(name, True)
            NS.set_fs_form(-1)
    finally:
        assert lib.nhip_set_climb_from_ops(-1) == 0
        NS.set_fs_form(-1)
        b.close()
    return [out[mode] for mode in MODES]


@pytest.mark.parametrize("n", sorted(LAUNCHES))
def test_modes_agree_and_launch_what_they_did(ctx, pool, n):
    got = _launches(ctx, pool, n)
    print(n, dict(zip(MODES, got)))
    assert got == LAUNCHES[n]
