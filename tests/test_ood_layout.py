"""The per-kind layout of the compiled OOD program (air_host.cpp air_compile, nhip_air_program and
nhip_air_segments) on the host, no GPU.  k_ood_air runs a step as three loops, one per segment (the
copies, the products, the sums and differences), each from its thread 0, and picks the operation by
the segment, so the bounds must partition every step and every instruction must be of its segment's
kind.  The program holds no padding: one instruction per live circuit node and one copy per
constraint.  A 64-lane pass with one product pays an XFE product on the whole wave, so the list
scheduler hands out products in multiples of 64 where the ready list allows: for the
triton-air-sized AIR at the default width sum_s ceil(products of step s / 64) lies below the 253
product-holding passes of the schedule before (floor: ceil(13,284 / 64) = 208)."""
import numpy as np
import pytest

import bench
import stark_ref as S

OOD_ADD, OOD_SUB, OOD_MUL, OOD_LOAD, OOD_ACC = 2, 3, 4, 5, 6


@pytest.fixture(scope="module")
def airs():
    a, _ = bench.load_pool()
    syn = S.AirCircuit.from_words([int(x) for x in a])
    return {"synthetic": syn, "triton-size": S.bloat_air(syn, 24000)}


def _live_nodes(air):
    reach, st = set(), [c for cs in air.constraints for c in cs]
    while st:
        i = st.pop()
        if i in reach:
            continue
        reach.add(i)
        op, a, b, _ = air.nodes[i]
        if op in (S.OP_ADD, S.OP_SUB, S.OP_MUL):
            st += [a, b]
    return reach


def _mul_waves(seg):
    return int(sum(-(-int(n) // 64) for n in seg[:, 2] - seg[:, 1]))


@pytest.mark.parametrize("name", ["synthetic", "triton-size"])
@pytest.mark.parametrize("width,lds_cap", [(None, None), (256, None), (1024, None), (512, 600)])
def test_segments_partition_each_step_by_kind(airs, name, width, lds_cap):
    import neptune_hip.stark as NS
    air = airs[name]
    g = NS.Air(air.to_words(), lds_slots=lds_cap or 0, step_width=width or 0)
    off, ins = g.program()
    seg = g.segments().astype(np.int64)
    steps = len(off) - 1
    assert seg.shape == (steps, 4)
    # the bounds partition the step: [copies | products | sums and differences]
    assert (seg[:, 0] == off[:-1]).all() and (seg[:, 3] == off[1:]).all()
    assert (np.diff(seg, axis=1) >= 0).all()
    ops = ins[:, 0].astype(np.int64)
    kinds = ({OOD_LOAD, OOD_ACC}, {OOD_MUL}, {OOD_ADD, OOD_SUB})
    for s in range(steps):
        for k, allowed in enumerate(kinds):
            got = set(ops[seg[s, k]:seg[s, k + 1]].tolist())
            assert got <= allowed, f"step {s} segment {k}: ops {sorted(got)}"
    # no padding: one instruction per live node, one copy per constraint
    live = _live_nodes(air)
    assert len(ins) == len(live) + air.num_constraints
    assert int((ops == OOD_ACC).sum()) == air.num_constraints
    n_mul = sum(1 for i in live if air.nodes[i][0] == S.OP_MUL)
    assert int((seg[:, 2] - seg[:, 1]).sum()) == n_mul == int((ops == OOD_MUL).sum())
    floor = -(-n_mul // 64)
    waves = _mul_waves(seg)
    assert waves >= floor
    print(f"{name} width {width or 512}: {steps} steps, {n_mul} products in {waves} waves (floor {floor})")


def test_triton_size_products_fill_their_waves(airs):
    """Default width: 13,284 products, floor 208; the schedule before this layout had 253 64-lane
    passes holding a product (231 by steps, the rest from product groups that began mid-wave).  The
    quota schedule reaches 212."""
    import neptune_hip.stark as NS
    g = NS.Air(airs["triton-size"].to_words())
    seg = g.segments().astype(np.int64)
    n_mul = int((seg[:, 2] - seg[:, 1]).sum())
    waves = _mul_waves(seg)
    print(f"sum ceil(MUL_s / 64) = {waves}, products {n_mul}, floor {-(-n_mul // 64)}")
    assert n_mul == 13284
    assert waves < 253
    assert g.info()["global_slots"] == 0
