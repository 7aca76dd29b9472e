"""Costs under several weight sets in one walk (cpd_index_set_weight_sets /
cpd_query_costs / Index.costs), bit-exact against the oracle: every column of
the all-sets mode is oracle.table_search under that set, the sliced mode is
the identity of tests/costs_ref.py (pinned against a lock-step numpy walk in
tests/test_costs_cpu.py).  Every check is exact equality over every query."""
import numpy as np
import pytest

import costs_ref as R
import cpd
import oracle
from graphs import GRAPHS
from test_gpu_paths import draw, one_way_ring, world

pytestmark = pytest.mark.gpu
MODES = ["rle", "dense"]


def congested(g, k):
    """k weight sets: free flow, then synth_congestion at seeds 3, 4, ..."""
    return [None] + [cpd.synth_congestion(g.w, frac=0.3, lo=1.0, hi=3.0, seed=2 + j)
                     for j in range(1, k)]


def check(out, ref):
    costs, hops, fin, st = out
    rc, rh, rf = ref
    assert costs.dtype == np.uint64 and costs.shape == rc.shape
    np.testing.assert_array_equal(costs, rc)
    np.testing.assert_array_equal(hops, rh)
    np.testing.assert_array_equal(fin, rf)
    assert st["queries"] == len(rh)
    assert st["hops"] == int(rh.sum()) and st["finished"] == int(rf.sum())
    assert st["cost"] == (int(rc[:, 0].sum()) if len(rh) else 0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_costs_every_graph(graph, mode):
    g, plan, dev, targets, rows, order, off, runs = world(graph)
    ix = cpd.Index(dev, rows=rows)
    ix.set_mode(mode)
    sets = congested(g, 3)
    s, t = draw(g, targets, 2000, seed=3)
    ref = R.ref_all(g, order, targets, off, runs, s, t, sets)
    ix.set_weight_sets(sets)
    check(ix.costs(s, t), ref)
    if graph == "irregular":  # the unfinished walks are there
        assert 0 < int(ref[2].sum()) < len(s)
    # each column is what the index's own plain walk gives under that set
    for j, w in enumerate(sets):
        ix.set_weights(w)
        cost, hops, fin, _ = ix.query(s, t)
        np.testing.assert_array_equal(cost, ref[0][:, j])
        np.testing.assert_array_equal(hops, ref[1])
        np.testing.assert_array_equal(fin, ref[2])
    # the empty batch
    e = ix.costs(np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    assert e[0].shape == (0, 3) and e[3]["queries"] == 0 and e[3]["cost"] == 0


def ring_world():
    g = one_way_ring()
    plan = cpd.Plan(g, hierarchy=False)
    dev = cpd.Graph(plan)
    order = plan.order()
    targets = np.random.default_rng(5).choice(g.n, size=40, replace=False).astype(np.uint32)
    off, runs = oracle.build_rows(g.row_ptr, g.dst, g.w, order, targets)
    return g, dev, targets, order, off, runs


# adjacency strides 1, 2, 4, 8, 16 slots per column (shift 0..4)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("graph", ["ring", "ring2", "synth", "deg8", "irregular"])
def test_costs_set_counts(graph, mode):
    if graph == "ring":
        g, dev, targets, order, off, runs = ring_world()
        ix = cpd.Index(dev, row_targets=targets, offsets=off, runs=runs)
    else:
        g, plan, dev, targets, rows, order, off, runs = world(graph)
        ix = cpd.Index(dev, rows=rows)
    maxdeg = int(np.diff(g.row_ptr.astype(np.int64)).max())
    shift = {"ring": 0, "ring2": 1, "synth": 2, "deg8": 3, "irregular": 4}[graph]
    assert (1 << shift) >= maxdeg and (shift == 0 or (1 << (shift - 1)) < maxdeg)
    ix.set_mode(mode)
    s, t = draw(g, targets, 1000, seed=11)
    allsets = congested(g, 8)
    for k in (1, 2, 4, 5, 8):  # both sides of the 4- and 8-word records
        ix.set_weight_sets(allsets[:k])
        out = ix.costs(s, t)
        assert out[0].shape == (len(s), k)  # the record's pad words are no columns
        check(out, R.ref_all(g, order, targets, off, runs, s, t, allsets[:k]))
    # sets in another order: a column follows its set, not its place
    ix.set_weight_sets(allsets[:5][::-1])
    check(ix.costs(s, t), R.ref_all(g, order, targets, off, runs, s, t, allsets[:5][::-1]))


@pytest.mark.parametrize("mode", MODES)
def test_costs_sliced(mode):
    g, plan, dev, targets, rows, order, off, runs = world("synth")
    ix = cpd.Index(dev, rows=rows)
    ix.set_mode(mode)
    s, t = draw(g, targets, 2000, seed=12)
    allsets = congested(g, 5)
    for K in (2, 5):
        ix.set_weight_sets(allsets[:K])
        full = R.ref_all(g, order, targets, off, runs, s, t, allsets[:K])
        for S in (1, 3, 7, g.n):
            for k in (-1, 1, 10):
                out = ix.costs(s, t, k_moves=k, slice_moves=S)
                assert out[0].shape == (len(s), 1)
                check(out, R.ref_sliced(g, order, targets, off, runs, s, t, allsets[:K], S,
                                        k_moves=k))
        # a slice at least as long as the longest walk: set 0's column
        longest = int(full[1].max())
        for S in (longest, longest + 1, g.n):
            np.testing.assert_array_equal(ix.costs(s, t, slice_moves=S)[0][:, 0], full[0][:, 0])
        assert np.any(ix.costs(s, t, slice_moves=max(1, longest - 1))[0][:, 0] != full[0][:, 0])
    # equal sets: the plain cost under that set, at any slice length
    ix.set_weight_sets([allsets[2]] * 3)
    ix.set_weights(allsets[2])
    plain = ix.query(s, t)[0]
    ix.set_weights(None)
    for S in (1, 4):
        np.testing.assert_array_equal(ix.costs(s, t, slice_moves=S)[0][:, 0], plain)


# the walk's launch constants (kDenseWaves, kRleWaves in cpd_kernels.hip), which
# the costs kernel shares: past 64 queries per wave a wave's lanes are refilled
@pytest.mark.parametrize("mode,nq", [("dense", 64 * 1024 + 4096), ("rle", 64 * 8192 + 4096)])
def test_costs_lane_refill(mode, nq):
    g, plan, dev, targets, rows, order, off, runs = world("synth", 1200)
    assert len(targets) == g.n == 1200
    ix = cpd.Index(dev, rows=rows)
    ix.set_mode(mode)
    s, t = draw(g, targets, nq, seed=7)
    sets = congested(g, 5)
    ix.set_weight_sets(sets)
    check(ix.costs(s, t), R.ref_all(g, order, targets, off, runs, s, t, sets))
    ix.set_weight_sets(sets[:3])
    check(ix.costs(s, t, slice_moves=3),
          R.ref_sliced(g, order, targets, off, runs, s, t, sets[:3], 3))


@pytest.mark.parametrize("mode", MODES)
def test_costs_wide_sums(mode):
    g, plan, dev, targets, rows, order, off, runs = world("synth")
    ix = cpd.Index(dev, rows=rows)
    ix.set_mode(mode)
    s, t = draw(g, targets, 2000, seed=13)
    top = np.full(len(g.w), 0xFFFFFFFF, np.uint32)
    plain = oracle.table_search(g.row_ptr, g.dst, g.w, order, targets, off, runs, s, t)
    for sets, col in (([top, None], 0), ([None, top], 1)):
        ix.set_weight_sets(sets)
        costs, hops, fin, st = ix.costs(s, t)
        np.testing.assert_array_equal(costs[:, col], hops.astype(np.uint64) * np.uint64(0xFFFFFFFF))
        np.testing.assert_array_equal(costs[:, 1 - col], plain[0])  # the other column: unaffected
        np.testing.assert_array_equal(hops, plain[1])
        assert int(costs[:, col].max()) > 1 << 32
        assert st["cost"] == int(costs[:, 0].astype(object).sum())
    ix.set_weight_sets([top, top])  # sliced over two such sets: still hops * 0xFFFFFFFF
    np.testing.assert_array_equal(ix.costs(s, t, slice_moves=2)[0][:, 0],
                                  plain[1].astype(np.uint64) * np.uint64(0xFFFFFFFF))


def test_costs_index_forms():
    g, plan, dev, targets, rows, order, off, runs = world("synth")
    s, t = draw(g, targets, 2000, seed=8)
    sets = congested(g, 3)
    ref = R.ref_all(g, order, targets, off, runs, s, t, sets)
    refs = R.ref_sliced(g, order, targets, off, runs, s, t, sets, 4)
    bits = dev.move_bits()
    forms = []
    for mode in MODES:
        forms.append((cpd.Index(dev, rows=rows), mode))
        forms.append((cpd.Index(dev, row_targets=targets, offsets=off, runs=runs), mode))
        for b in (bits, 4):  # streamed at the packed width and at 4 bits
            ix = cpd.Index.streamed(dev, targets, int(off[-1]), mode=mode)
            ix.append_moves(oracle.moves_from_runs(off, runs, g.n, b), b)
            forms.append((ix, None))
    for ix, mode in forms:
        if mode:
            ix.set_mode(mode)
        ix.set_weight_sets(sets)
        check(ix.costs(s, t), ref)
        check(ix.costs(s, t, slice_moves=4), refs)


def same(a, b):
    for x, y in zip(a[:-1], b[:-1]):
        np.testing.assert_array_equal(x, y)
    assert {k: v for k, v in a[-1].items() if k != "kernel_ms"} == \
           {k: v for k, v in b[-1].items() if k != "kernel_ms"}


@pytest.mark.parametrize("mode", MODES)
def test_costs_isolation(mode):
    g, plan, dev, targets, rows, order, off, runs = world("synth")
    ix = cpd.Index(dev, rows=rows)
    ix.set_mode(mode)
    s, t = draw(g, targets, 2000, seed=10)
    sets = congested(g, 5)
    wc = cpd.synth_congestion(g.w, frac=0.3, lo=1.0, hi=3.0, seed=9)  # none of the sets
    ix.set_weights(wc)
    q0, p0 = ix.query(s, t), ix.paths(s, t)
    np.testing.assert_array_equal(
        q0[0], oracle.table_search(g.row_ptr, g.dst, wc, order, targets, off, runs, s, t)[0])
    ix.set_weight_sets(sets)
    ref5 = R.ref_all(g, order, targets, off, runs, s, t, sets)
    check(ix.costs(s, t), ref5)
    # the index's own weights, walk and paths are what they were
    same(ix.query(s, t), q0)
    same(ix.paths(s, t), p0)
    # on one prepared batch: the plain run's results are not the costs' and stay
    ix.prepare(s, t)
    ix.run()
    st = ix.costs_run()
    cost = np.empty(len(s), np.uint64)
    cpd._check(cpd.lib.cpd_query_fetch(ix._h, cpd._ptr(cost, cpd.u64p), None, None))
    np.testing.assert_array_equal(cost, q0[0])
    check(ix.costs_fetch() + (st,), ref5)
    # the sets survive a new prepare; 5 sets replaced by 2
    s2, t2 = draw(g, targets, 500, seed=14)
    check(ix.costs(s2, t2), R.ref_all(g, order, targets, off, runs, s2, t2, sets))
    ix.set_weight_sets(sets[3:])
    check(ix.costs(s, t), R.ref_all(g, order, targets, off, runs, s, t, sets[3:]))
    same(ix.query(s, t), q0)
    # fetch before costs on a fresh batch
    ix.prepare(s, t)
    with pytest.raises(cpd.CpdError) as ei:
        ix.costs_fetch()
    assert ei.value.code == cpd.CPD_E_ARG
    rc = cpd.lib.cpd_query_costs_fetch(ix._h, None, None, None)  # the library's own refusal
    assert rc == cpd.CPD_E_ARG
    # 9 sets: refused, the loaded sets stay
    with pytest.raises(cpd.CpdError) as ei:
        ix.set_weight_sets([None] * 9)
    assert ei.value.code == cpd.CPD_E_ARG
    check(ix.costs(s, t), R.ref_all(g, order, targets, off, runs, s, t, sets[3:]))
    # cleared: costs refuses
    ix.set_weight_sets(None)
    with pytest.raises(cpd.CpdError) as ei:
        ix.costs(s, t)
    assert ei.value.code == cpd.CPD_E_ARG
    same(ix.query(s, t), q0)
