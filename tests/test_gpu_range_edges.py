"""GPU parity at three edges of the build path the other files do not reach,
bit-exact against the CPU oracle:

- distances at the top of the u32 range (saturating adds that wrap, the wide
  row marker 0xFFFFFFFE next to real distances, narrow rows forced off);
- a 32-slab batch (bit 31 of every slab mask);
- level-1 nodes with more than four leaf arcs at 8-bit first-move sets (the
  closed form's tail read from the ascending arrays).

The shapes these tests rely on are pinned in test_host_cpu.py.
"""
import numpy as np
import pytest

import cpd
import oracle
from graphs import TOP, stars, two_cycle, wide_level1
from test_ch_gpu import same_hierarchy
from test_gpu_parity import make_graph

pytestmark = pytest.mark.gpu


def check_debug_rows(g, dev, targets, ref_dist, ref_fm, tag):
    dist, fm = dev.debug_rows(targets)
    for i, t in enumerate(targets):
        np.testing.assert_array_equal(dist[:, i], ref_dist[i], err_msg=f"{tag} dist t={t}")
        np.testing.assert_array_equal(fm[i], ref_fm[i], err_msg=f"{tag} fm t={t}")


def oracle_rows(g, targets):
    """(distances, first-move sets) of the oracle, one row per target."""
    return ([oracle.reverse_dijkstra(g.row_ptr, g.dst, g.w, t) for t in targets],
            [oracle.first_moves(g.row_ptr, g.dst, g.w, t) for t in targets])


# ---------------------------------------------------------------------------
# 1. the top of the range

def wrapping_triples(g, ref_dist):
    """(target, edge) pairs whose w + d(head) is >= 2^32 with d(head) finite,
    from the oracle's numbers in u64: the adds that must saturate."""
    w = g.w.astype(np.uint64)
    cnt = 0
    for d in ref_dist:
        dh = d[g.dst]
        cnt += int(np.count_nonzero((dh != oracle.INF) & (w + dh.astype(np.uint64) >= 1 << 32)))
    return cnt


@pytest.fixture(scope="module", params=sorted(TOP))
def top(request):
    name = request.param
    g = TOP[name]()
    plan = cpd.Plan(g)
    t64 = np.random.default_rng(1).choice(g.n, size=64, replace=False).astype(np.uint32)
    ref_dist, ref_fm = oracle_rows(g, t64)
    tb = np.random.default_rng(6).permutation(g.n)[: min(g.n, 1500)].astype(np.uint32)
    ref_off, ref_runs = oracle.build_rows(g.row_ptr, g.dst, g.w, plan.order(), tb)
    return name, g, plan, t64, ref_dist, ref_fm, tb, ref_off, ref_runs


@pytest.mark.parametrize("narrow", [True, False], ids=["narrow", "wide"])
def test_top_of_range_sweeps_and_first_moves(top, narrow):
    """Distance bounds just under the limit.  Two builds on one device: the
    first full batch's probe finds the group rows wide and turns narrow rows
    off, the second runs after the switch.  On deg8heavy the oracle's u64
    numbers show (edge, target) adds that pass 2^32, so sat_add's overflow
    arm runs; on the scaled deg8 and synth graphs no add can pass it for any
    target (graphs.deg8_heavy_graph has the figures)."""
    name, g, plan, t64, ref_dist, ref_fm, tb, ref_off, ref_runs = top
    if name == "deg8heavy":
        assert wrapping_triples(g, ref_dist) >= 1
    dev = make_graph(plan, 1024, narrow)
    check_debug_rows(g, dev, t64, ref_dist, ref_fm, name)
    for rep in range(2):
        off, runs = dev.build_rows(tb).export()
        np.testing.assert_array_equal(off, ref_off, err_msg=f"{name} build {rep}")
        np.testing.assert_array_equal(runs, ref_runs, err_msg=f"{name} build {rep}")


# ---------------------------------------------------------------------------
# 2. distances beside the wide-row marker

@pytest.mark.parametrize("a", [0xFFFFFFFE, 0xFFFFFFFD], ids=hex)
def test_distance_equal_to_the_wide_row_marker(a):
    """A 2-node cycle (a, 1) with CPD_NARROW on.  a = 0xFFFFFFFE is the wide
    row marker itself: the graph must run without narrow rows.  a = 0xFFFFFFFD
    keeps them, and node 0's group row (distances 0 and a) is kept wide."""
    g = two_cycle(a)
    plan = cpd.Plan(g)
    assert plan.info()["dist_bound"] == a
    dev = make_graph(plan, 1024, True)
    t = np.array([0, 1], np.uint32)
    dist, fm = dev.debug_rows(t)
    assert dist.tolist() == [[0, a], [1, 0]]  # dist[node][target]
    for i in (0, 1):
        np.testing.assert_array_equal(dist[:, i], oracle.reverse_dijkstra(g.row_ptr, g.dst, g.w, i))
        np.testing.assert_array_equal(fm[i], oracle.first_moves(g.row_ptr, g.dst, g.w, i))
    for tg in (t, t[::-1].copy()):
        off, runs = dev.build_rows(tg).export()
        ref_off, ref_runs = oracle.build_rows(g.row_ptr, g.dst, g.w, plan.order(), tg)
        np.testing.assert_array_equal(off, ref_off)
        np.testing.assert_array_equal(runs, ref_runs)


@pytest.mark.parametrize("name,settle", [("synth", 0), ("synth", 3), ("deg8", 0),
                                         ("deg8heavy", 0)])
def test_ch_gpu_identical_at_top_of_range(name, settle):
    """Candidate shortcuts of weight >= 2^32-1 are dropped on both sides: the
    GPU contraction's hierarchy stays the host's, arc for arc."""
    g = TOP[name]()
    same_hierarchy(cpd.Plan(g, settle=settle).export_ch(),
                   cpd.Plan(g, settle=settle, gpu=0).export_ch())


# ---------------------------------------------------------------------------
# 3. a 32-slab batch

B32 = 32768


@pytest.fixture(scope="module")
def slab32():
    g = cpd.synth_road_graph(60, 60, seed=21)
    plan = cpd.Plan(g)
    every = np.arange(g.n, dtype=np.uint32)
    ref_off, ref_runs = oracle.build_rows(g.row_ptr, g.dst, g.w, plan.order(), every)
    ref_mv = oracle.moves_from_runs(ref_off, ref_runs, g.n, 2)  # [target] -> its row
    targets = np.random.default_rng(32).integers(0, g.n, B32 + 1500).astype(np.uint32)
    return g, plan, ref_mv, targets


@pytest.mark.parametrize("narrow", [True, False], ids=["narrow", "wide"])
def test_32_slab_batch(slab32, narrow):
    """batch = 32768, the largest cpd_graph_set_batch takes: 32 slabs, bit 31
    of tmask / live / active.  Targets drawn with replacement; the compact
    rows (export_moves) are compared with the oracle's row of each requested
    target, so duplicates must give identical rows.  Then 31 * 1024 + 1
    targets: 32 active slabs, the last one target and padding."""
    g, plan, ref_mv, targets = slab32
    order = plan.order()
    # lanes of the first batch: its targets in column order
    first = targets[:B32]
    lane_t = first[np.argsort(order[first], kind="stable")]
    for slab in (0, 31):  # a dropped slab bit must show: neighbouring rows differ
        lt = lane_t[1024 * slab: 1024 * (slab + 1)]
        assert np.any(np.any(ref_mv[lt[1:]] != ref_mv[lt[:-1]], axis=1)), slab
    dev = make_graph(plan, B32, narrow)
    assert dev.batch == B32 and dev.move_bits() == 2
    rows = dev.build_rows(targets)  # a full batch, then a partial one
    np.testing.assert_array_equal(first, lane_t[rows.lanes()[:B32]])  # the lane order holds
    mv = rows.export_moves()
    assert mv.shape == (len(targets), ref_mv.shape[1])
    assert np.array_equal(mv, ref_mv[targets]), np.nonzero(np.any(mv != ref_mv[targets], axis=1))[0][:20]
    k = 31 * 1024 + 1
    part = targets[:k]
    lane_p = part[np.argsort(order[part], kind="stable")]
    # slab 31 holds lane_p[-1] and padding (lane 0's target): different rows
    assert np.any(ref_mv[lane_p[-1]] != ref_mv[lane_p[0]])
    mv = dev.build_rows(part).export_moves()
    assert np.array_equal(mv, ref_mv[part]), np.nonzero(np.any(mv != ref_mv[part], axis=1))[0][:20]


# ---------------------------------------------------------------------------
# 4. level-1 nodes with more than four leaf arcs, 8-bit sets

@pytest.fixture(scope="module")
def wide_l1():
    g = stars(300, 3)
    plan = cpd.Plan(g)
    ch, order = plan.export_ch(), plan.order()
    v, cnt = wide_level1(ch)
    hub = int(v[np.argmax(cnt)])  # 7 or more leaf arcs: 6 pendants and the next hub
    a, b = int(ch["dn_off"][hub]), int(ch["dn_off"][hub + 1])
    # the hub's leaf arcs in the ascending list's order: by (column, weight)
    asc = sorted((int(order[h]), int(w), int(h)) for h, w in zip(ch["dn_dst"][a:b], ch["dn_w"][a:b]))
    pend = [h for _, _, h in asc if h >= 300]  # pendants: ids past the ring
    rng = np.random.default_rng(4)
    rest = np.setdiff1d(np.arange(g.n), [hub] + pend)
    t40 = np.concatenate([[hub], pend, rng.choice(rest, 40 - 1 - len(pend), replace=False)])
    t40 = rng.permutation(t40).astype(np.uint32)
    ref_dist, ref_fm = oracle_rows(g, t40)
    # a pendant is entered from its hub alone: d(hub, pendant) is that arc's
    # weight.  One at index >= 4 of the ascending order is decided by the
    # closed form's tail.
    tail = [(w, h) for i, (_, w, h) in enumerate(asc) if i >= 4 and h in pend]
    assert len(pend) >= 5 and tail
    for w, h in tail:
        assert ref_dist[t40.tolist().index(h)][hub] == w
    tall = np.random.default_rng(5).permutation(g.n).astype(np.uint32)
    ref_off, ref_runs = oracle.build_rows(g.row_ptr, g.dst, g.w, order, tall)
    return g, plan, t40, ref_dist, ref_fm, tall, ref_off, ref_runs


@pytest.mark.parametrize("narrow,xy", [(True, False), (False, False), (True, True)],
                         ids=["narrow", "wide", "narrow-xy"])
def test_wide_level1_nodes_8bit(wide_l1, narrow, xy):
    """Hubs with 5..7 pendant leaves: level-1 nodes whose fifth and later
    leaf arcs are read from the ascending arrays (down8_slot, l1_val) and
    whose slab masks come from all their leaves (arc_mask; every node a
    target, two slabs)."""
    g, plan, t40, ref_dist, ref_fm, tall, ref_off, ref_runs = wide_l1
    dev = make_graph(plan, 2048, narrow)
    if xy:
        rng = np.random.default_rng(5)
        dev.set_coords(rng.integers(-1000, 1000, g.n, dtype=np.int32),
                       rng.integers(-1000, 1000, g.n, dtype=np.int32))
    off, runs = dev.build_rows(tall).export()
    np.testing.assert_array_equal(off, ref_off)
    np.testing.assert_array_equal(runs, ref_runs)
    check_debug_rows(g, dev, t40, ref_dist, ref_fm, "stars")
