"""What tests/test_gpu_ch_edges.py relies on, from the host plan alone: the
contraction gadgets of graphs.py have the shape their docstrings state (the
input degrees; every fan contracted with all D out-neighbours above it; the
hub contracted last), and the host hierarchy of each — the GPU contraction's
reference — gives exact distances, checked against the oracle's Dijkstra by
sweeps that use nothing of either contraction."""
import numpy as np
import pytest

import cpd
from graphs import (CH_FAN_D, CH_HUB_D, CH_LANE_EDGE_D, CH_TIE_D, ch_fan_case, ch_hub_case, ch_hub_two_way)
from test_host_cpu import _check_hierarchy_sweeps

FANS = [(D, 3) for D in CH_FAN_D] + [(D, 2) for D in CH_TIE_D]
HUBS = [(D, 3) for D in sorted(set(CH_HUB_D + CH_LANE_EDGE_D))] + [(D, 2) for D in CH_TIE_D]


def _degrees(g):
    out = np.diff(g.row_ptr.astype(np.int64))
    return out, np.bincount(g.dst, minlength=g.n)


@pytest.mark.parametrize("D,wmax", FANS)
def test_fan_is_contracted_with_all_its_targets(D, wmax):
    g, fans = ch_fan_case(D, wmax)
    out, inn = _degrees(g)
    assert np.all(out[fans] == D) and np.all(inn[fans] == 1)
    assert out.max() == D + 3                  # the fans' sources: path, fan, D witnesses
    for f in fans:                             # distinct heads: D arcs are D targets
        assert len(set(g.dst[g.row_ptr[f]:g.row_ptr[f + 1]])) == D
    plan = cpd.Plan(g, threads=2, ch_only=True)
    ch = plan.export_ch()
    assert np.all(np.diff(ch["up_off"].astype(np.int64))[fans] == D)
    assert np.all(ch["rank"][fans] < g.n - D)
    _check_hierarchy_sweeps(g, plan, f"fan D={D} wmax={wmax}")


def _check_hub(g, hub, D, Din):
    out, inn = _degrees(g)
    assert out[hub] == D and inn[hub] == Din + 2
    heads = set(g.dst[g.row_ptr[hub]:g.row_ptr[hub + 1]])
    tails = set(np.repeat(np.arange(g.n), out)[g.dst == hub])
    assert len(heads) == D and len(tails) == Din + 2
    assert heads & tails == {hub - 1, hub + 1}   # every extra in-neighbour sees D targets
    assert np.delete(out, hub).max() <= 3
    plan = cpd.Plan(g, threads=2, ch_only=True)
    assert plan.export_ch()["rank"][hub] == g.n - 1
    return plan


@pytest.mark.parametrize("D,wmax", HUBS)
def test_hub_is_contracted_last(D, wmax):
    g, hub = ch_hub_case(D, wmax)
    plan = _check_hub(g, hub, D, 1)
    _check_hierarchy_sweeps(g, plan, f"hub D={D} wmax={wmax}")


def test_two_way_hub_is_contracted_last():
    g, hub = ch_hub_two_way()
    plan = _check_hub(g, hub, 300, 300)
    _check_hierarchy_sweeps(g, plan, "two-way hub")


def test_hierarchy_only_plans(tmp_path):
    """cpd_hierarchy_create: the plan's own hierarchy on a graph a plan holds,
    a hierarchy and nothing else past the plan's degree limit."""
    from graphs import GRAPHS
    g = GRAPHS["deg8"]()
    a, b = cpd.Plan(g, threads=2).export_ch(), cpd.Plan(g, threads=2, ch_only=True).export_ch()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    g, _ = ch_fan_case(33)
    with pytest.raises(cpd.CpdError, match="out-degree 36 > 15"):
        cpd.Plan(g)
    p = cpd.Plan(g, threads=2, ch_only=True)
    assert p.info()["n"] == g.n and p.info()["ch_up_arcs"] > 0
    for call in (p.order, lambda: p.save(str(tmp_path / "p.plan"))):
        with pytest.raises(cpd.CpdError, match="hierarchy only"):
            call()
    with pytest.raises(cpd.CpdError, match="no_hierarchy"):
        cpd.Plan(g, hierarchy=False, ch_only=True)
    if cpd.device_count() == 0:
        with pytest.raises(cpd.CpdError, match="no GPU visible"):
            cpd.Plan(g, gpu=0, ch_only=True)
