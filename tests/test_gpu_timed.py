"""Timed walks (cpd_query_timed / Index.timed): every move costed, and loaded,
under the weight set of the clock time at which its edge is entered, bit-exact
against the lock-step numpy walk of tests/timed_ref.py (pinned against a plain
per-query loop and the oracle in tests/test_timed_cpu.py).  Every check is
exact equality over every query and every (set, edge) counter."""
import functools

import numpy as np
import pytest

import cpd
import oracle
import timed_ref as T
from graphs import GRAPHS
from test_gpu_costs import congested, ring_world
from test_gpu_loads import long_pair, random_demand, same
from test_gpu_paths import draw, world

pytestmark = pytest.mark.gpu
MODES = ["rle", "dense"]


def index(graph, mode, ntargets=50):
    if graph == "ring":
        g, dev, targets, order, off, runs = ring_world()
        ix = cpd.Index(dev, row_targets=targets, offsets=off, runs=runs)
    else:
        g, plan, dev, targets, rows, order, off, runs = world(graph, ntargets)
        ix = cpd.Index(dev, rows=rows)
    ix.set_mode(mode)
    return ix, g, targets, (g, order, targets, off, runs)


def third_of_median(wd, s, t):
    """About a third of the median plain-walk cost of the batch, at least 1."""
    g, order, targets, off, runs = wd
    cost = oracle.table_search(g.row_ptr, g.dst, g.w, order, targets, off, runs, s, t)[0]
    return max(1, int(np.median(cost)) // 3)


def departures(nq, hi, seed):
    return np.random.default_rng(seed).integers(0, max(1, hi), nq).astype(np.uint64)


def check(out, ref, loads=None):
    """out = Index.timed's result, ref = timed_ref.walk_timed's; loads = the
    fetched table when the call made one."""
    cost, hops, fin, st = out
    rc, rh, rf, rl = ref
    assert cost.dtype == np.uint64 and cost.shape == rc.shape
    np.testing.assert_array_equal(cost, rc)
    np.testing.assert_array_equal(hops, rh)
    np.testing.assert_array_equal(fin, rf)
    assert st["queries"] == len(rh)
    assert st["hops"] == int(rh.sum()) and st["finished"] == int(rf.sum())
    assert st["cost"] == int(rc.astype(object).sum())
    if loads is not None:
        assert loads.dtype == np.uint64 and loads.shape == rl.shape
        np.testing.assert_array_equal(loads, rl)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_timed_every_graph(graph, mode):
    ix, g, targets, wd = index(graph, mode)
    sets = congested(g, 3)
    ix.set_weight_sets(sets)
    s, t = draw(g, targets, 2000, seed=3)
    P = third_of_median(wd, s, t)
    dep = departures(len(s), 3 * P, 31)
    demand = random_demand(len(s), 32)
    ref = T.walk_timed(*wd, s, t, sets, dep, P, demand)
    check(ix.timed(s, t, dep, P), ref)
    check(ix.timed(s, t, dep, P, demand, loads=True), ref, ix.loads_fetch())
    # no departures: everybody leaves at 0; no demand: 1 each
    ref0 = T.walk_timed(*wd, s, t, sets, None, P)
    check(ix.timed(s, t, period=P, loads=True), ref0, ix.loads_fetch())
    if graph == "irregular":  # the unfinished walks and the 0-weight edges are there
        assert 0 < int(ref[2].sum()) < len(s)
        assert (g.w == 0).any() and ref[3][:, g.w == 0].any()
    # the empty batch
    e = ix.timed(np.zeros(0, np.uint32), np.zeros(0, np.uint32), period=P, loads=True)
    assert e[0].shape == (0,) and e[3]["queries"] == 0 and e[3]["cost"] == 0
    z = ix.loads_fetch()
    assert z.shape == (3, g.m) and z.dtype == np.uint64 and not z.any()


# adjacency strides 1, 2, 4, 8, 16 slots per column (shift 0..4), records of 4 and 8 words
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("graph", ["ring", "ring2", "synth", "deg8", "irregular"])
def test_timed_strides(graph, mode):
    ix, g, targets, wd = index(graph, mode)
    maxdeg = int(np.diff(g.row_ptr.astype(np.int64)).max())
    shift = {"ring": 0, "ring2": 1, "synth": 2, "deg8": 3, "irregular": 4}[graph]
    assert (1 << shift) >= maxdeg and (shift == 0 or (1 << (shift - 1)) < maxdeg)
    s, t = draw(g, targets, 1000, seed=11)
    P = third_of_median(wd, s, t)
    demand = random_demand(len(s), 33)
    allsets = congested(g, 5)
    for K in (2, 5):
        ix.set_weight_sets(allsets[:K])
        dep = departures(len(s), K * P, 34 + K)
        ref = T.walk_timed(*wd, s, t, allsets[:K], dep, P, demand)
        check(ix.timed(s, t, dep, P, demand, loads=True), ref, ix.loads_fetch())
        check(ix.timed(s, t, dep, P), ref)
        if graph != "ring":
            assert ref[3][K - 1].any()  # the clock reaches the last set


@pytest.mark.parametrize("mode", MODES)
def test_timed_set_counts(mode):
    ix, g, targets, wd = index("synth", mode)
    s, t = draw(g, targets, 2000, seed=12)
    P = third_of_median(wd, s, t)
    allsets = congested(g, 8)
    for K in (1, 2, 4, 5, 8):  # both sides of the 4- and 8-word records
        ix.set_weight_sets(allsets[:K])
        dep = departures(len(s), K * P, 40 + K)
        ref = T.walk_timed(*wd, s, t, allsets[:K], dep, P)
        out = ix.timed(s, t, dep, P, loads=True)
        check(out, ref, ix.loads_fetch())
        if K == 1:  # one set: the clock cannot matter
            costs = ix.costs(s, t)
            np.testing.assert_array_equal(out[0], costs[0][:, 0])
        else:
            assert all(ref[3][j].any() for j in range(min(K, 3)))
    # sets in another order: a plane follows its set's place in the list
    ix.set_weight_sets(allsets[:5][::-1])
    dep = departures(len(s), 5 * P, 49)
    check(ix.timed(s, t, dep, P, loads=True),
          T.walk_timed(*wd, s, t, allsets[:5][::-1], dep, P), ix.loads_fetch())


@pytest.mark.parametrize("mode", MODES)
def test_timed_period_edges(mode):
    ix, g, targets, wd = index("synth", mode)
    s, t = draw(g, targets, 2000, seed=13)
    nq = len(s)
    sets = congested(g, 4)
    ix.set_weight_sets(sets)
    Pm = third_of_median(wd, s, t)
    rng = np.random.default_rng(50)
    k = rng.integers(0, 6, nq).astype(np.uint64)
    cases = [
        (1, departures(nq, 4, 51)),                                   # P = 1
        (1 << 60, departures(nq, 1 << 62, 52)),                       # P = 2^60
        (Pm, k * np.uint64(Pm)),                                      # exactly on k P
        (Pm, np.maximum(k, np.uint64(1)) * np.uint64(Pm) - np.uint64(1)),  # on k P - 1
        (Pm, departures(nq, 3 * Pm, 53) + np.uint64(1 << 32)),        # >= 2^32 (last set)
        (1 << 33, np.uint64(1 << 33) * (k + np.uint64(1)) - np.uint64(1)
         - departures(nq, 2 * Pm, 54)),                               # just below bounds >= 2^33
        (Pm, np.full(nq, (1 << 63) - 1, np.uint64)),                  # clamped to the last set
        (1 << 60, np.full(nq, (1 << 63) - 1, np.uint64)),
    ]
    for P, dep in cases:
        ref = T.walk_timed(*wd, s, t, sets, dep, P)
        check(ix.timed(s, t, dep, P, loads=True), ref, ix.loads_fetch())
    # the departures near 2^33 k straddle period bounds above 2^32
    P, dep = cases[5]
    j0 = np.minimum(dep // np.uint64(P), np.uint64(3))
    j1 = np.minimum((dep + ref_cost(wd, s, t)) // np.uint64(P), np.uint64(3))
    assert np.any(j0 != j1) and int(dep.max()) >= 1 << 32
    # single weights above 3 P: one move crosses several periods
    heavy = [None, g.w * np.uint32(2), (g.w.astype(np.uint64) * 50).astype(np.uint32),
             g.w * np.uint32(3)]
    P = max(1, int(g.w[g.w > 0].min()) * 50 // 4)
    assert int(heavy[2].max()) > 3 * P
    ix.set_weight_sets(heavy)
    dep = departures(nq, 2 * P, 55) + np.uint64(P)
    out = T.walk_timed_sets(*wd, s, t, heavy, dep, P)
    assert int(out[4].max()) >= 2  # some walk's set rises by two or more in one move
    check(ix.timed(s, t, dep, P, loads=True), out[:4], ix.loads_fetch())
    # weights of 0xFFFFFFFF: the clock is 64-bit
    top = [np.full(g.m, 0xFFFFFFFF, np.uint32), None, np.full(g.m, 0xFFFFFFFF, np.uint32)]
    ix.set_weight_sets(top)
    for P, dep in ((1 << 34, departures(nq, 1 << 34, 56)), (1 << 60, np.full(nq, (1 << 63) - 1,
                                                                            np.uint64))):
        ref = T.walk_timed(*wd, s, t, top, dep, P)
        assert int(ref[0].max()) > 1 << 34
        check(ix.timed(s, t, dep, P, loads=True), ref, ix.loads_fetch())


def ref_cost(wd, s, t):
    g, order, targets, off, runs = wd
    return oracle.table_search(g.row_ptr, g.dst, g.w, order, targets, off, runs, s, t)[0].astype(
        np.uint64)


@pytest.mark.parametrize("mode", MODES)
def test_timed_k_moves(mode):
    ix, g, targets, wd = index("synth", mode)
    s, t = draw(g, targets, 2000, seed=5)
    sets = congested(g, 3)
    ix.set_weight_sets(sets)
    P = third_of_median(wd, s, t)
    dep = departures(len(s), 3 * P, 60)
    demand = random_demand(len(s), 61)
    for k in (-1, 1, 10):
        ref = T.walk_timed(*wd, s, t, sets, dep, P, demand, k_moves=k)
        check(ix.timed(s, t, dep, P, demand, k_moves=k, loads=True), ref, ix.loads_fetch())
    # below the refill limit k_moves = 0 is exact: no move, no cost, an all-zero table
    out = ix.timed(s, t, dep, P, demand, k_moves=0, loads=True)
    assert not out[0].any() and not out[1].any() and out[3]["hops"] == 0 and out[3]["cost"] == 0
    z = ix.loads_fetch()
    assert z.shape == (3, g.m) and not z.any()


# the walk's launch constants (kDenseWaves, kRleWaves in cpd_kernels.hip), which
# the timed kernel shares: past 64 queries per wave a wave's lanes are refilled
@pytest.mark.parametrize("mode,nq", [("dense", 64 * 1024 + 4096), ("rle", 64 * 8192 + 4096)])
def test_timed_lane_refill(mode, nq):
    ix, g, targets, wd = index("synth", mode, 1200)
    assert len(targets) == g.n == 1200
    s, t = draw(g, targets, nq, seed=7)
    sets = congested(g, 3)
    ix.set_weight_sets(sets)
    P = third_of_median(wd, s[:4096], t[:4096])
    dep = departures(nq, 3 * P, 62)
    demand = random_demand(nq, 63)
    ref = T.walk_timed(*wd, s, t, sets, dep, P, demand)
    check(ix.timed(s, t, dep, P, demand, loads=True), ref, ix.loads_fetch())


# every lane of a wave holds the same counter in every iteration
@pytest.mark.parametrize("mode", MODES)
def test_timed_contention(mode):
    ix, g, targets, wd = index("synth", mode)
    a, b = long_pair(*wd)
    rs, rt = draw(g, targets, 4096, seed=15)
    s = np.concatenate((np.full(4096, a, np.uint32), rs))
    t = np.concatenate((np.full(4096, b, np.uint32), rt))
    sets = congested(g, 3)
    ix.set_weight_sets(sets)
    P = third_of_median(wd, s, t)
    demand = np.full(len(s), 0xFFFFFFFF, np.uint32)
    for dep in (None, departures(len(s), 3 * P, 64)):
        ref = T.walk_timed(*wd, s, t, sets, dep, P, demand)
        check(ix.timed(s, t, dep, P, demand, loads=True), ref, ix.loads_fetch())
    assert int(ref[3].max()) > 1 << 32  # no wrap, no lost add


@pytest.mark.parametrize("mode", MODES)
def test_timed_accumulate(mode):
    ix, g, targets, wd = index("synth", mode)
    s, t = draw(g, targets, 3000, seed=16)
    sets = congested(g, 3)
    ix.set_weight_sets(sets)
    P = third_of_median(wd, s, t)
    dep = departures(len(s), 3 * P, 65)
    demand = random_demand(len(s), 66)
    whole = T.walk_timed(*wd, s, t, sets, dep, P, demand)[3]
    first = T.walk_timed(*wd, s[:1000], t[:1000], sets, dep[:1000], P, demand[:1000])[3]
    # the first accumulating call finds no table: it starts from zero
    ix.timed(s[:1000], t[:1000], dep[:1000], P, demand[:1000], loads=True, accumulate=True)
    np.testing.assert_array_equal(ix.loads_fetch(), first)
    ix.timed(s[1000:], t[1000:], dep[1000:], P, demand[1000:], loads=True, accumulate=True)
    np.testing.assert_array_equal(ix.loads_fetch(), whole)
    # another period, another number of sets, a plain loads call: refused, the table stays
    with pytest.raises(cpd.CpdError) as ei:
        ix.timed(s[:10], t[:10], dep[:10], P + 1, loads=True, accumulate=True)
    assert ei.value.code == cpd.CPD_E_ARG
    ix.set_weight_sets(sets[:2])
    with pytest.raises(cpd.CpdError) as ei:
        ix.timed(s[:10], t[:10], dep[:10], P, loads=True, accumulate=True)
    assert ei.value.code == cpd.CPD_E_ARG
    ix.set_weight_sets(sets)
    for K, S in ((3, 4), (1, 0)):
        with pytest.raises(cpd.CpdError) as ei:
            ix.loads(s[:10], t[:10], slices=K, slice_moves=S, accumulate=True)
        assert ei.value.code == cpd.CPD_E_ARG
    ix._load_slices = 3  # the mirror's count of planes: the table is the timed one still
    np.testing.assert_array_equal(ix.loads_fetch(), whole)
    # without the flag a call starts from zero
    ix.timed(s[:1000], t[:1000], dep[:1000], P, demand[:1000], loads=True)
    np.testing.assert_array_equal(ix.loads_fetch(), first)
    # a timed call accumulating onto a plain table of as many planes: refused
    plain = ix.loads(s[:1000], t[:1000], demand[:1000], slices=3, slice_moves=4)[0]
    with pytest.raises(cpd.CpdError) as ei:
        ix.timed(s[:10], t[:10], dep[:10], P, loads=True, accumulate=True)
    assert ei.value.code == cpd.CPD_E_ARG
    ix._load_slices = 3
    np.testing.assert_array_equal(ix.loads_fetch(), plain)
    # a plain accumulate onto the plain table still works
    ix.loads(s[:10], t[:10], slices=3, slice_moves=4, accumulate=True)
    # cleared: the fetch refuses
    ix.timed(s[:10], t[:10], dep[:10], P, loads=True)
    ix.loads_clear()
    with pytest.raises(cpd.CpdError) as ei:
        ix.loads_fetch()
    assert ei.value.code == cpd.CPD_E_ARG
    out = np.zeros(3 * g.m, np.uint64)
    assert cpd.lib.cpd_query_loads_fetch(ix._h, cpd._ptr(out, cpd.u64p)) == cpd.CPD_E_ARG


@pytest.mark.parametrize("mode", MODES)
def test_timed_argument_rules(mode):
    g, plan, dev, targets, rows, order, off, runs = world("synth")
    ix = cpd.Index(dev, rows=rows)
    ix.set_mode(mode)
    s, t = draw(g, targets, 100, seed=17)
    st = cpd.QueryStats()

    def run(ixh, dep, P, flags):
        return cpd.lib.cpd_query_timed(ixh, cpd.C.c_int32(-1), cpd._ptr(dep, cpd.u64p),
                                       cpd.C.c_uint64(P), None, cpd.C.c_uint32(flags),
                                       cpd.C.byref(st))

    ix.prepare(s, t)
    # no sets loaded
    assert run(ix._h, None, 10, 0) == cpd.CPD_E_ARG
    assert "no weight sets" in cpd.lib.cpd_last_error().decode()
    ix.set_weight_sets(congested(g, 2))
    # fetch before run, in the library and in the mirror
    cost = np.zeros(len(s), np.uint64)
    assert cpd.lib.cpd_query_timed_fetch(ix._h, cpd._ptr(cost, cpd.u64p), None, None) == cpd.CPD_E_ARG
    with pytest.raises(cpd.CpdError) as ei:
        ix.timed_fetch()
    assert ei.value.code == cpd.CPD_E_ARG
    # the period's range
    for P in (0, (1 << 60) + 1, (1 << 64) - 1):
        assert run(ix._h, None, P, 0) == cpd.CPD_E_ARG
        assert str(P) in cpd.lib.cpd_last_error().decode()
    # a departure of 2^63 or more: the first one is named
    dep = np.zeros(len(s), np.uint64)
    dep[7], dep[9] = (1 << 63) + 5, (1 << 64) - 1
    assert run(ix._h, dep, 10, 0) == cpd.CPD_E_ARG
    assert str((1 << 63) + 5) in cpd.lib.cpd_last_error().decode()
    # ACCUMULATE without TIMED_LOADS
    assert run(ix._h, None, 10, cpd.LOADS_ACCUMULATE) == cpd.CPD_E_ARG
    assert cpd.lib.cpd_query_timed_fetch(ix._h, cpd._ptr(cost, cpd.u64p), None, None) == cpd.CPD_E_ARG
    # the limits themselves pass
    dep[7], dep[9] = (1 << 63) - 1, 0
    assert run(ix._h, dep, 1 << 60, cpd.TIMED_LOADS | cpd.LOADS_ACCUMULATE) == cpd.CPD_OK
    assert cpd.lib.cpd_query_timed_fetch(ix._h, cpd._ptr(cost, cpd.u64p), None, None) == cpd.CPD_OK
    # a new prepare ends the validity of the results
    ix.prepare(s, t)
    assert cpd.lib.cpd_query_timed_fetch(ix._h, cpd._ptr(cost, cpd.u64p), None, None) == cpd.CPD_E_ARG
    # the mirror's own rules
    with pytest.raises(ValueError):
        ix.timed_run(np.zeros(5, np.uint64), 10)
    with pytest.raises(ValueError):
        ix.timed_run(None, 10, np.zeros(5, np.uint32), loads=True)
    with pytest.raises(ValueError):
        ix.timed_run()
    # an incomplete index
    part = cpd.Index.streamed(dev, targets, int(off[-1]), mode=mode)
    part.set_weight_sets(congested(g, 2))
    assert run(part._h, None, 10, 0) == cpd.CPD_E_ARG
    assert "incomplete" in cpd.lib.cpd_last_error().decode()


@pytest.mark.parametrize("mode", MODES)
def test_timed_independence(mode):
    g, plan, dev, targets, rows, order, off, runs = world("synth")
    wd = (g, order, targets, off, runs)
    s, t = draw(g, targets, 2000, seed=10)
    wc = cpd.synth_congestion(g.w, frac=0.3, lo=1.0, hi=3.0, seed=9)
    sets = [None, wc]
    P = third_of_median(wd, s, t)
    dep = departures(len(s), 2 * P, 67)
    ref = T.walk_timed(*wd, s, t, sets, dep, P)
    # what an index that never saw a timed call returns
    clean = cpd.Index(dev, rows=rows)
    clean.set_mode(mode)
    clean.set_weights(wc)
    clean.set_weight_sets(sets)
    q0, p0, c0 = clean.query(s, t), clean.paths(s, t), clean.costs(s, t)
    s0 = clean.search(s[:300], t[:300])
    ix = cpd.Index(dev, rows=rows)
    ix.set_mode(mode)
    ix.set_weight_sets(sets)
    check(ix.timed(s, t, dep, P, loads=True), ref, ix.loads_fetch())
    ix.set_weights(wc)  # set_weights does not change timed results
    check(ix.timed(s, t, dep, P, loads=True), ref, ix.loads_fetch())
    same(ix.query(s, t), q0)
    same(ix.paths(s, t), p0)
    same(ix.costs(s, t), c0)
    same(ix.search(s[:300], t[:300]), s0, stats=False)  # its stats hold times and sizes
    # a timed call between a run and its fetches changes nothing of theirs
    ix.prepare(s, t)
    ix.run()
    offsets, _ = ix.paths_run()
    ix.costs_run()
    ix.timed_run(dep, P, loads=True)
    cost, hops, fin = (np.empty(len(s), np.uint64), np.empty(len(s), np.uint32),
                       np.empty(len(s), np.uint8))
    cpd._check(cpd.lib.cpd_query_fetch(ix._h, cpd._ptr(cost, cpd.u64p), cpd._ptr(hops, cpd.u32p),
                                       cpd._ptr(fin, cpd.u8p)))
    same((cost, hops, fin, None), q0[:3] + (None,), stats=False)
    np.testing.assert_array_equal(offsets, p0[0])
    np.testing.assert_array_equal(ix.paths_fetch(0, len(s)), p0[1])
    same(ix.costs_fetch() + (None,), c0[:3] + (None,), stats=False)
    check(ix.timed_fetch() + (ref_stats(ref),), ref)


def ref_stats(ref):
    return {"queries": len(ref[1]), "hops": int(ref[1].sum()), "finished": int(ref[2].sum()),
            "cost": int(ref[0].astype(object).sum())}
