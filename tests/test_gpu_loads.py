"""Edge loads (cpd_query_loads / Index.loads): the demand every edge carries
over a batch of table-search walks, bit-exact against the lock-step numpy walk
of tests/loads_ref.py (pinned against the oracle in tests/test_loads_cpu.py).
Every check is exact equality over every (slice, edge) counter."""
import numpy as np
import pytest

import cpd
import loads_ref as L
import oracle
from graphs import GRAPHS
from test_gpu_paths import draw, one_way_ring, world

pytestmark = pytest.mark.gpu
MODES = ["rle", "dense"]


def random_demand(nq, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, nq, dtype=np.uint64).astype(np.uint32)


def fetch(ix, nq):
    cost = np.empty(nq, np.uint64)
    hops = np.empty(nq, np.uint32)
    fin = np.empty(nq, np.uint8)
    cpd._check(cpd.lib.cpd_query_fetch(ix._h, cpd._ptr(cost, cpd.u64p), cpd._ptr(hops, cpd.u32p),
                                       cpd._ptr(fin, cpd.u8p)))
    return cost, hops, fin


def check(ix, out, ref, plain):
    """out = Index.loads' result, ref = loads_ref.walk_loads', plain = the
    index's own plain walk (Index.query) of the same queries."""
    loads, st = out
    rl, rh, rf = ref
    assert loads.dtype == np.uint64 and loads.shape == rl.shape
    np.testing.assert_array_equal(loads, rl)
    pc, ph, pf, pst = plain
    np.testing.assert_array_equal(ph, rh)
    np.testing.assert_array_equal(pf, rf)
    assert {k: v for k, v in st.items() if k != "kernel_ms"} == \
           {k: v for k, v in pst.items() if k != "kernel_ms"}
    cost, hops, fin = fetch(ix, len(rh))
    np.testing.assert_array_equal(cost, pc)
    np.testing.assert_array_equal(hops, ph)
    np.testing.assert_array_equal(fin, pf)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_loads_every_graph(graph, mode):
    g, plan, dev, targets, rows, order, off, runs = world(graph)
    ix = cpd.Index(dev, rows=rows)
    ix.set_mode(mode)
    s, t = draw(g, targets, 2000, seed=3)
    plain = ix.query(s, t)
    for demand in (None, random_demand(len(s), 21)):
        ref = L.walk_loads(g, order, targets, off, runs, s, t, demand)
        check(ix, ix.loads(s, t, demand), ref, plain)
    if graph == "irregular":  # the unfinished walks are there
        assert 0 < int(ref[2].sum()) < len(s)
    # the empty batch
    e, st = ix.loads(np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    assert e.shape == (1, g.m) and e.dtype == np.uint64 and not e.any()
    assert st["queries"] == 0 and st["hops"] == 0


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
def test_loads_strides(graph, mode):
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
    demand = random_demand(len(s), 22)
    plain = ix.query(s, t)
    check(ix, ix.loads(s, t, demand), L.walk_loads(g, order, targets, off, runs, s, t, demand),
          plain)
    check(ix, ix.loads(s, t, demand, slices=3, slice_moves=2),
          L.walk_loads(g, order, targets, off, runs, s, t, demand, K=3, S=2), plain)


@pytest.mark.parametrize("mode", MODES)
def test_loads_k_moves(mode):
    g, plan, dev, targets, rows, order, off, runs = world("synth")
    ix = cpd.Index(dev, rows=rows)
    ix.set_mode(mode)
    s, t = draw(g, targets, 2000, seed=5)
    demand = random_demand(len(s), 23)
    for k in (-1, 1, 10):
        check(ix, ix.loads(s, t, demand, k_moves=k),
              L.walk_loads(g, order, targets, off, runs, s, t, demand, k_moves=k),
              ix.query(s, t, k_moves=k))
    # below the refill limit k_moves = 0 is exact: no move, an all-zero table
    z, st = ix.loads(s, t, demand, k_moves=0)
    assert z.shape == (1, g.m) and not z.any() and st["hops"] == 0


@pytest.mark.parametrize("mode", MODES)
def test_loads_sliced(mode):
    g, plan, dev, targets, rows, order, off, runs = world("synth")
    ix = cpd.Index(dev, rows=rows)
    ix.set_mode(mode)
    s, t = draw(g, targets, 2000, seed=12)
    demand = random_demand(len(s), 24)
    for k in (-1, 10):
        plain = ix.query(s, t, k_moves=k)
        full = L.walk_loads(g, order, targets, off, runs, s, t, demand, k_moves=k)
        longest = int(full[1].max())
        for K in (2, 5, 8):
            for S in (1, 3, 7, g.n):
                out = ix.loads(s, t, demand, k_moves=k, slices=K, slice_moves=S)
                check(ix, out, L.walk_loads(g, order, targets, off, runs, s, t, demand, K=K, S=S,
                                            k_moves=k), plain)
                np.testing.assert_array_equal(out[0].sum(axis=0, dtype=np.uint64), full[0][0])
            # a slice at least as long as the longest walk: everything in plane 0
            for S in (longest, longest + 1):
                pl = ix.loads(s, t, demand, k_moves=k, slices=K, slice_moves=S)[0]
                np.testing.assert_array_equal(pl[0], full[0][0])
                assert not pl[1:].any()
            if longest > 1:
                assert ix.loads(s, t, demand, k_moves=k, slices=K, slice_moves=longest - 1)[0][1].any()


def long_pair(g, order, targets, off, runs, least=20):
    """An (s, t) whose walk finishes after at least `least` moves."""
    s = np.arange(g.n, dtype=np.uint32)
    for tt in targets:
        _, hops, fin = oracle.table_search(g.row_ptr, g.dst, g.w, order, targets, off, runs, s,
                                           np.full(g.n, tt, np.uint32))
        ok = np.nonzero((fin == 1) & (hops >= least))[0]
        if len(ok):
            return int(ok[0]), int(tt)
    raise AssertionError("no walk that long")


# every lane of a wave holds the same counter in every iteration
@pytest.mark.parametrize("mode", MODES)
def test_loads_contention(mode):
    g, plan, dev, targets, rows, order, off, runs = world("synth")
    ix = cpd.Index(dev, rows=rows)
    ix.set_mode(mode)
    a, b = long_pair(g, order, targets, off, runs)
    rs, rt = draw(g, targets, 4096, seed=15)
    s = np.concatenate((np.full(4096, a, np.uint32), rs))
    t = np.concatenate((np.full(4096, b, np.uint32), rt))
    plain = ix.query(s, t)
    for demand in (None, np.full(len(s), 0xFFFFFFFF, np.uint32)):
        ref = L.walk_loads(g, order, targets, off, runs, s, t, demand)
        check(ix, ix.loads(s, t, demand), ref, plain)
        check(ix, ix.loads(s, t, demand, slices=4, slice_moves=6),
              L.walk_loads(g, order, targets, off, runs, s, t, demand, K=4, S=6), plain)
        hot = ref[0][0] >= np.uint64(4096) * np.uint64(1 if demand is None else 0xFFFFFFFF)
        assert int(hot.sum()) >= 20
    assert int(ref[0].max()) > 1 << 32  # no wrap, no lost add


# the walk's launch constants (kDenseWaves, kRleWaves in cpd_kernels.hip), which
# the loads kernel shares: past 64 queries per wave a wave's lanes are refilled
@pytest.mark.parametrize("mode,nq", [("dense", 64 * 1024 + 4096), ("rle", 64 * 8192 + 4096)])
def test_loads_lane_refill(mode, nq):
    g, plan, dev, targets, rows, order, off, runs = world("synth", 1200)
    assert len(targets) == g.n == 1200
    ix = cpd.Index(dev, rows=rows)
    ix.set_mode(mode)
    s, t = draw(g, targets, nq, seed=7)
    demand = random_demand(nq, 25)
    plain = ix.query(s, t)
    check(ix, ix.loads(s, t, demand), L.walk_loads(g, order, targets, off, runs, s, t, demand),
          plain)
    check(ix, ix.loads(s, t, demand, slices=3, slice_moves=5),
          L.walk_loads(g, order, targets, off, runs, s, t, demand, K=3, S=5), plain)


@pytest.mark.parametrize("mode", MODES)
def test_loads_accumulate(mode):
    g, plan, dev, targets, rows, order, off, runs = world("synth")
    ix = cpd.Index(dev, rows=rows)
    ix.set_mode(mode)
    s, t = draw(g, targets, 3000, seed=16)
    demand = random_demand(len(s), 26)
    for K, S in ((1, 0), (3, 4)):
        ix.loads_clear()
        whole = L.walk_loads(g, order, targets, off, runs, s, t, demand, K=K, S=S)[0]
        first = L.walk_loads(g, order, targets, off, runs, s[:1000], t[:1000], demand[:1000], K=K,
                             S=S)[0]
        # the first accumulating call finds no table: it starts from zero
        a, _ = ix.loads(s[:1000], t[:1000], demand[:1000], slices=K, slice_moves=S, accumulate=True)
        np.testing.assert_array_equal(a, first)
        b, _ = ix.loads(s[1000:], t[1000:], demand[1000:], slices=K, slice_moves=S, accumulate=True)
        np.testing.assert_array_equal(b, whole)
        np.testing.assert_array_equal(ix.loads_fetch(), whole)  # a second fetch: the same table
        # mismatched slices with the flag: refused, the table stays
        for k2, s2 in ((2, 4), (3, 5)) if K == 3 else ((2, 4),):
            with pytest.raises(cpd.CpdError) as ei:
                ix.loads(s[:10], t[:10], slices=k2, slice_moves=s2, accumulate=True)
            assert ei.value.code == cpd.CPD_E_ARG
            np.testing.assert_array_equal(ix.loads_fetch(), whole)
        # without the flag a call starts from zero
        c, _ = ix.loads(s[:1000], t[:1000], demand[:1000], slices=K, slice_moves=S)
        np.testing.assert_array_equal(c, first)
    # cleared: fetch refuses, in the mirror and in the library
    ix.loads_clear()
    with pytest.raises(cpd.CpdError) as ei:
        ix.loads_fetch()
    assert ei.value.code == cpd.CPD_E_ARG
    out = np.zeros(g.m, np.uint64)
    assert cpd.lib.cpd_query_loads_fetch(ix._h, cpd._ptr(out, cpd.u64p)) == cpd.CPD_E_ARG
    # a fresh index: the same
    ix2 = cpd.Index(dev, rows=rows)
    assert cpd.lib.cpd_query_loads_fetch(ix2._h, cpd._ptr(out, cpd.u64p)) == cpd.CPD_E_ARG
    # the argument rules
    ix.prepare(s, t)
    for K, S in ((0, 0), (9, 1), (2, 0), (1, 3)):
        with pytest.raises(cpd.CpdError) as ei:
            ix.loads_run(slices=K, slice_moves=S)
        assert ei.value.code == cpd.CPD_E_ARG
    with pytest.raises(ValueError):
        ix.loads_run(demand[:5])
    # an incomplete index
    part = cpd.Index.streamed(dev, targets, int(off[-1]), mode=mode)
    st = cpd.QueryStats()
    assert cpd.lib.cpd_query_loads(part._h, -1, None, 1, 0, 0, cpd.C.byref(st)) == cpd.CPD_E_ARG


def same(a, b, stats=True):
    for x, y in zip(a[:-1], b[:-1]):
        np.testing.assert_array_equal(x, y)
    if stats:
        assert {k: v for k, v in a[-1].items() if k != "kernel_ms"} == \
               {k: v for k, v in b[-1].items() if k != "kernel_ms"}


@pytest.mark.parametrize("mode", MODES)
def test_loads_independence(mode):
    g, plan, dev, targets, rows, order, off, runs = world("synth")
    s, t = draw(g, targets, 2000, seed=10)
    demand = random_demand(len(s), 27)
    wc = cpd.synth_congestion(g.w, frac=0.3, lo=1.0, hi=3.0, seed=9)
    sets = [None, wc]
    ref = L.walk_loads(g, order, targets, off, runs, s, t, demand)
    # what an index that never saw a loads call returns
    clean = cpd.Index(dev, rows=rows)
    clean.set_mode(mode)
    clean.set_weights(wc)
    clean.set_weight_sets(sets)
    q0, p0, c0 = clean.query(s, t), clean.paths(s, t), clean.costs(s, t)
    s0 = clean.search(s[:300], t[:300])
    ix = cpd.Index(dev, rows=rows)
    ix.set_mode(mode)
    np.testing.assert_array_equal(ix.loads(s, t, demand)[0], ref[0])  # free-flow weights
    ix.set_weights(wc)
    ix.set_weight_sets(sets)
    # loads never depend on the weights; cost / st of the call follow them
    out = ix.loads(s, t, demand)
    check(ix, out, ref, q0)
    # the other calls return what they return without it, and leave the table alone
    same(ix.query(s, t), q0)
    same(ix.paths(s, t), p0)
    same(ix.costs(s, t), c0)
    same(ix.search(s[:300], t[:300]), s0, stats=False)  # its stats hold times and sizes
    ix.set_weights(None)
    ix.set_weight_sets(None)
    np.testing.assert_array_equal(ix.loads_fetch(), ref[0])
    # ... and a loads call between them changes nothing of theirs
    ix.set_weights(wc)
    ix.set_weight_sets(sets)
    ix.loads(s, t, demand, slices=2, slice_moves=3)
    same(ix.query(s, t), q0)
    same(ix.paths(s, t), p0)
    same(ix.costs(s, t), c0)
    # like a plain run, a loads call ends the validity of fetched paths
    ix.paths(s, t)
    ix.loads_run(demand)
    with pytest.raises(cpd.CpdError) as ei:
        ix.paths_fetch(0, 10)
    assert ei.value.code == cpd.CPD_E_ARG
    assert cpd.lib.cpd_query_paths_fetch(ix._h, 0, 1, None) == cpd.CPD_E_ARG
