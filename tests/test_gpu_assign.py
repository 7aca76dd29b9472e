"""GPU: loads to weights in HBM and the loop around it
(cpd_index_weights_from_loads, cpd_index_get_weights / _weight_sets,
cpd_query_assign) against tests/assign_ref.py, which restates the header in
Python ints (pinned by test_assign_cpu.py).  Every value is compared exactly:
the weights bit for bit, the 128-bit sums, the loop's records."""
import ctypes as C
import re

import numpy as np
import pytest

import costs_ref
import cpd
import oracle
from assign_ref import (BPR, LOOP_ITERS, U32, loop_want, loop_world, ref_weights_from_loads)
from graphs import deg8_graph, irregular_graph, lattice_wide, ring2_graph, scaled_to_bound

pytestmark = pytest.mark.gpu


class Env:
    def index(self, mode="dense"):
        ix = cpd.Index.streamed(self.dev, self.targets, int(self.off[-1]), mode=mode)
        ix.append(self.off, self.runs)
        return ix

    def walk(self, w):
        return oracle.table_search(self.g.row_ptr, self.g.dst, w, self.order, self.targets,
                                   self.off, self.runs, self.s, self.t)

    def search(self, w, **opts):
        return oracle.cpd_search(self.g.row_ptr, self.g.dst, self.g.w, w, self.order,
                                 self.targets, self.off, self.runs, self.s, self.t, **opts)


def make_env(g, ntargets, nq, seed):
    e = Env()
    e.g = g
    e.plan = cpd.Plan(g)
    e.order = e.plan.order()
    e.dev = cpd.Graph(e.plan, batch=1024)
    rng = np.random.default_rng(seed)
    e.targets = rng.choice(g.n, size=ntargets, replace=False).astype(np.uint32)
    e.s = rng.integers(0, g.n, nq).astype(np.uint32)
    e.t = e.targets[rng.integers(0, ntargets, nq)]
    e.off, e.runs = oracle.build_rows(g.row_ptr, g.dst, g.w, e.order, e.targets)
    e.demand = rng.integers(0, 50, nq).astype(np.uint32)
    e.capacity = rng.integers(1, 40, g.m).astype(np.uint32)
    e.capacity[: min(5, g.m)] = 1
    return e


GRAPHS = {
    "synth": lambda: cpd.synth_road_graph(40, 30, seed=7),   # 4 slots per column
    "ring2": ring2_graph,                                    # 2
    "deg8": deg8_graph,                                      # 8
    "irregular": irregular_graph,                            # 16: padding, parallel, 0-weight
    "lattice15": lambda: lattice_wide(20, 15, 15, seed=15),  # 16
}


@pytest.fixture(scope="module", params=sorted(GRAPHS))
def wenv(request):
    return request.param, make_env(GRAPHS[request.param](), 30, 800, 23)


@pytest.fixture(scope="module")
def env():
    return make_env(GRAPHS["synth"](), 40, 1500, 29)


def check_one_plane(ix, e, a, power, load_div, msg):
    """weights_from_loads on the resident one-plane table against the reference
    of the fetched loads; returns the new weights."""
    loads = ix.loads_fetch()
    assert loads.shape == (1, e.g.m)
    info = ix.weights_from_loads(e.capacity, a=a, power=power, load_div=load_div)
    want, tstt, changed = ref_weights_from_loads(e.g.w, loads[0], e.capacity, a[0], a[1], power,
                                                 load_div)
    got = ix.get_weights()
    print(f"{msg}: tstt {info['tstt']} want {tstt}; changed {info['changed']} want {changed}")
    np.testing.assert_array_equal(got, want, err_msg=msg)
    assert (info["tstt"], info["changed"], info["planes"]) == (tstt, changed, 1), msg
    assert info["vdf_ms"] >= 0
    np.testing.assert_array_equal(ix.loads_fetch(), loads, err_msg=msg)  # the table is only read
    return got


def test_one_plane_every_width(wenv):
    name, e = wenv
    ix = e.index()
    ix.loads(e.s, e.t, e.demand)
    seen = 0
    for power in (1, 2, 3, 4):
        for load_div in (1, 3):
            # small weights (1..5) need a large a to move at all
            w = check_one_plane(ix, e, (7, 2), power, load_div, f"{name} p{power} d{load_div}")
            seen += int((w != e.g.w).sum())
    assert seen > 0
    w = check_one_plane(ix, e, (3, 20), 4, 1, f"{name} bpr")
    # a walk costs under the new weights ...
    cost, hops, fin, _ = ix.query(e.s, e.t)
    rc, rh, rf = e.walk(w)
    np.testing.assert_array_equal(cost, rc)
    np.testing.assert_array_equal(hops, rh)
    np.testing.assert_array_equal(fin, rf)
    # ... and both forms of the search see them (the incumbent tables are rebuilt)
    for form in ("tables", "walks"):
        ix.search(e.s, e.t, tables=form)  # tables of the weights before the update
        ix.loads(e.s, e.t, e.demand)
        w = check_one_plane(ix, e, (7, 2), 2, 1, f"{name} {form}")
        got = ix.search(e.s, e.t, tables=form)
        want = e.search(w)
        for a, b in zip(got[:3], want[:3]):
            np.testing.assert_array_equal(a, b, err_msg=f"{name} {form}")
        np.testing.assert_array_equal(got[3].astype(np.uint64), want[3], err_msg=f"{name} {form}")
    # after a search's loading
    ix.search_loads(e.s, e.t, e.demand)
    check_one_plane(ix, e, (7, 2), 3, 1, f"{name} search loads")
    # free flow comes back
    ix.set_weights(None)
    np.testing.assert_array_equal(ix.get_weights(), e.g.w)
    np.testing.assert_array_equal(ix.query(e.s, e.t)[0], e.walk(e.g.w)[0])


def check_planes(ix, e, K, a, power, load_div, msg):
    loads = ix.loads_fetch()
    assert loads.shape == (K, e.g.m)
    info = ix.weights_from_loads(e.capacity, a=a, power=power, load_div=load_div)
    sets = ix.get_weight_sets()
    assert sets.shape == (K, e.g.m), msg
    tstt = changed = 0
    for j in range(K):
        want, tj, cj = ref_weights_from_loads(e.g.w, loads[j], e.capacity, a[0], a[1], power,
                                              load_div)
        np.testing.assert_array_equal(sets[j], want, err_msg=f"{msg} plane {j}")
        tstt, changed = tstt + tj, changed + cj
    print(f"{msg}: tstt {info['tstt']} want {tstt}; changed {info['changed']} want {changed}")
    assert (info["tstt"], info["changed"], info["planes"]) == (tstt, changed, K), msg
    # the walks cost under them
    costs, hops, fin, _ = ix.costs(e.s, e.t)
    rc, rh, rf = costs_ref.ref_all(e.g, e.order, e.targets, e.off, e.runs, e.s, e.t, list(sets))
    np.testing.assert_array_equal(costs, rc, err_msg=msg)
    np.testing.assert_array_equal(hops, rh, err_msg=msg)
    np.testing.assert_array_equal(fin, rf, err_msg=msg)
    return sets


def test_k_planes(env):
    e = env
    wc = cpd.synth_congestion(e.g.w, frac=0.3, lo=1.0, hi=3.0, seed=4)
    ix = e.index()
    ix.set_weights(wc)
    ix.loads(e.s, e.t, e.demand, slices=3, slice_moves=5)
    sets = check_planes(ix, e, 3, (3, 20), 4, 1, "sliced")
    assert (sets != e.g.w).any() and (sets[0] != sets[2]).any()
    np.testing.assert_array_equal(ix.get_weights(), wc)  # the current weights stay
    for K in (2, 4, 5, 8):  # both record widths
        ix.set_weight_sets([None] + [wc] * (K - 1))
        ix.timed(e.s, e.t, period=20000, demand=e.demand, loads=True)
        sets = check_planes(ix, e, K, (1, 1), 2, 2, f"timed {K}")
        assert (sets != e.g.w).any()
        np.testing.assert_array_equal(ix.get_weights(), wc)
    # fewer sets after more: the record narrows again
    ix.loads(e.s, e.t, slices=2, slice_moves=9)
    check_planes(ix, e, 2, (3, 20), 4, 1, "after 8")


@pytest.mark.parametrize("name", ["synth", "lattice15"])
def test_weights_read_back_what_was_set(name):
    e = make_env(GRAPHS[name](), 10, 50, 3)
    ix = e.index()
    rng = np.random.default_rng(5)
    np.testing.assert_array_equal(ix.get_weights(), e.g.w)
    assert ix.get_weight_sets().shape == (0, e.g.m)
    wa = rng.integers(0, 1 << 32, e.g.m, dtype=np.uint64).astype(np.uint32)
    wb = rng.integers(0, 1 << 32, e.g.m, dtype=np.uint64).astype(np.uint32)
    ix.set_weights(wa)
    np.testing.assert_array_equal(ix.get_weights(), wa)
    for sets in ([None, wa, wb], [wb, None, wa, wa, wb], [wa] * 8):
        ix.set_weight_sets(sets)
        want = np.stack([e.g.w if w is None else w for w in sets])
        np.testing.assert_array_equal(ix.get_weight_sets(), want)
        np.testing.assert_array_equal(ix.get_weights(), wa)
    ix.set_weights(None)
    np.testing.assert_array_equal(ix.get_weights(), e.g.w)
    ix.set_weight_sets(None)
    assert ix.get_weight_sets().shape == (0, e.g.m)


def test_extremes():
    """tstt past 2^64 (both halves exact) and weights that saturate."""
    e = make_env(scaled_to_bound(GRAPHS["synth"](), 0xFFFFFFFD), 30, 600, 31)
    top = np.full(len(e.s), U32, np.uint32)
    ix = e.index()
    loads, _ = ix.loads(e.s, e.t, top)
    want, tstt, changed = ref_weights_from_loads(e.g.w, loads[0], e.capacity, 3, 20, 4, 1)
    assert tstt >= 1 << 64  # the inputs do pass 64 bits
    info = ix.weights_from_loads(e.capacity)
    print(f"extremes: tstt {info['tstt']} want {tstt}")
    assert info["tstt"] == tstt and info["tstt"] >> 64 == tstt >> 64 > 0
    assert info["tstt"] & (2 ** 64 - 1) == tstt & (2 ** 64 - 1) and info["changed"] == changed
    np.testing.assert_array_equal(ix.get_weights(), want)
    assert (want == U32).any()  # capacity 1 under 2^32 per query: saturated
    ones = np.ones(e.g.m, np.uint32)
    info = ix.weights_from_loads(ones, a=(65535, 1), power=4)
    want, tstt, changed = ref_weights_from_loads(e.g.w, loads[0], ones, 65535, 1, 4, 1)
    got = ix.get_weights()
    np.testing.assert_array_equal(got, want)
    assert (got[loads[0] > 0] == U32).all() and (got[loads[0] == 0] == e.g.w[loads[0] == 0]).all()
    assert info["tstt"] == tstt and info["changed"] == changed


def test_bad_arguments_change_nothing(env):
    e = env
    wc = cpd.synth_congestion(e.g.w, frac=0.3, lo=1.0, hi=3.0, seed=4)
    ix = e.index()
    with pytest.raises(cpd.CpdError) as err:  # no table yet
        ix.weights_from_loads(e.capacity)
    assert err.value.code == cpd.CPD_E_ARG and "no load table" in str(err.value)
    ix.set_weights(wc)
    ix.set_weight_sets([None, wc])
    ix.loads(e.s, e.t, e.demand)
    before = ix.loads_fetch()
    zero = e.capacity.copy()
    zero[7] = 0
    bad = [dict(capacity=zero), dict(a=(65536, 1)), dict(a=(1, 0)), dict(a=(1, 65536)),
           dict(power=0), dict(power=5), dict(load_div=0)]
    words = ["capacity 0 on edge 7", "a_num 65536", "a_den 0", "a_den 65536", "power 0",
             "power 5", "load_div 0"]
    for kw, word in zip(bad, words):
        with pytest.raises(cpd.CpdError) as err:
            ix.weights_from_loads(**dict(dict(capacity=e.capacity), **kw))
        assert err.value.code == cpd.CPD_E_ARG and word in str(err.value), kw
    f = cpd.Vdf(3, 20, 4, 1)
    assert cpd.lib.cpd_index_weights_from_loads(ix._h, None, C.byref(f), None) == cpd.CPD_E_ARG
    assert cpd.lib.cpd_index_weights_from_loads(ix._h, cpd._ptr(e.capacity, cpd.u32p), None,
                                                None) == cpd.CPD_E_ARG
    np.testing.assert_array_equal(ix.loads_fetch(), before)
    np.testing.assert_array_equal(ix.get_weights(), wc)
    np.testing.assert_array_equal(ix.get_weight_sets(), np.stack([e.g.w, wc]))
    # an incomplete index
    part = cpd.Index.streamed(e.dev, e.targets, int(e.off[-1]), mode="dense")
    with pytest.raises(cpd.CpdError) as err:
        part.weights_from_loads(e.capacity)
    assert err.value.code == cpd.CPD_E_ARG and "incomplete" in str(err.value)
    # the loop's own
    ix.prepare(e.s, e.t)
    for kw, word in ((dict(iters=0), "iterations"), (dict(iters=65536), "iterations"),
                     (dict(power=5), "power 5"), (dict(capacity=zero), "capacity 0 on edge 7")):
        args = dict(dict(capacity=e.capacity, iters=2), **kw)
        with pytest.raises(cpd.CpdError) as err:
            ix.assign_run(**args)
        assert err.value.code == cpd.CPD_E_ARG and word in str(err.value), kw
    np.testing.assert_array_equal(ix.loads_fetch(), before)
    np.testing.assert_array_equal(ix.get_weights(), wc)


# --- cpd_query_assign ------------------------------------------------------

@pytest.fixture(scope="module")
def loop():
    wd = loop_world()
    e = Env()
    e.g, e.order, e.targets, e.off, e.runs = wd["g"], wd["order"], wd["targets"], wd["off"], wd["runs"]
    e.s, e.t, e.demand, e.capacity = wd["s"], wd["t"], wd["demand"], wd["capacity"]
    e.plan = cpd.Plan(e.g)
    assert np.array_equal(e.plan.order(), e.order)
    e.dev = cpd.Graph(e.plan, batch=1024)
    return e


def check_assign(ix, recs, want, msg):
    wrecs, wloads, ww, (wcost, wplen, wfin, wstats) = want
    assert len(recs) == len(wrecs), msg
    for k, (r, w) in enumerate(zip(recs, wrecs)):
        print(f"{msg} k={k + 1}: got {({x: r[x] for x in w})} want {w}")
        assert {x: r[x] for x in w} == w, f"{msg} iteration {k + 1}"
        assert r["search_ms"] >= 0 and r["loads_ms"] >= 0 and r["vdf_ms"] >= 0
    np.testing.assert_array_equal(ix.loads_fetch()[0], wloads, err_msg=f"{msg} loads")
    np.testing.assert_array_equal(ix.get_weights(), ww, err_msg=f"{msg} weights")
    cost, plen, fin, cnt = ix.search_fetch()
    np.testing.assert_array_equal(cost, wcost, err_msg=f"{msg} cost")
    np.testing.assert_array_equal(plen, wplen, err_msg=f"{msg} plen")
    np.testing.assert_array_equal(fin, wfin, err_msg=f"{msg} finished")
    np.testing.assert_array_equal(cnt.astype(np.uint64), wstats, err_msg=f"{msg} counters")


@pytest.mark.parametrize("form", ["tables", "walks"])
@pytest.mark.parametrize("mode", ["dense", "rle"])
@pytest.mark.parametrize("fscale", [0.0, 0.1])
def test_assign_matches_reference(loop, fscale, mode, form):
    ix = loop.index(mode)
    recs = ix.assign(loop.s, loop.t, loop.capacity, LOOP_ITERS, loop.demand, a=BPR[:2],
                     power=BPR[2], fscale=fscale, tables=form)
    check_assign(ix, recs, loop_want(fscale=fscale), f"{mode} {form} fscale {fscale}")
    # set_weights(None) still restores free flow
    ix.set_weights(None)
    np.testing.assert_array_equal(ix.get_weights(), loop.g.w)


def test_assign_variants(loop):
    ix = loop.index()
    # no demand: 1 per query
    recs = ix.assign(loop.s, loop.t, loop.capacity, 2)
    check_assign(ix, recs, loop_want(demand=False, iters=2), "unit demand")
    # one iteration
    ix.set_weights(None)
    recs = ix.assign(loop.s, loop.t, loop.capacity, 1, loop.demand)
    check_assign(ix, recs, loop_want(iters=1), "one iteration")
    ix.flow_step(loop.capacity)  # a flow table: MSA keeps none and leaves this one alone
    flow = ix.flow_fetch()
    # a warm start: iteration 1 searches under the weights the index holds
    wc = cpd.synth_congestion(loop.g.w, frac=0.2, lo=1.0, hi=3.0, seed=4)
    ix.set_weights(wc)
    recs = ix.assign(loop.s, loop.t, loop.capacity, 3, loop.demand)
    want = loop_want(warm=wc, iters=3)
    check_assign(ix, recs, want, "warm start")
    np.testing.assert_array_equal(ix.flow_fetch(), flow)
    assert want[0][0]["sptt"] != loop_want(iters=1)[0][0]["sptt"]
    # the empty batch: all-zero records, a zeroed table, w0 on every edge
    none = np.zeros(0, np.uint32)
    recs = ix.assign(none, none, loop.capacity, 2)
    assert len(recs) == 2
    for r in recs:
        assert all(r[k] == 0 for k in ("finished", "sptt", "tstt", "moves", "changed"))
    assert ix.loads_fetch().shape == (1, loop.g.m) and not ix.loads_fetch().any()
    np.testing.assert_array_equal(ix.get_weights(), loop.g.w)


def test_assign_pool_overflow(loop):
    """test_search_loads_pool_overflow's pattern: CPD_E_OOM from iteration 1,
    the state as it was, a second call succeeds."""
    ix = loop.index()
    wc = cpd.synth_congestion(loop.g.w, frac=0.2, lo=1.0, hi=3.0, seed=4)
    ix.set_weights(wc)
    before, _ = ix.loads(loop.s, loop.t)
    with pytest.raises(cpd.CpdError) as e:
        ix.assign(loop.s, loop.t, loop.capacity, LOOP_ITERS, loop.demand, prefix_bytes=64)
    assert e.value.code == cpd.CPD_E_OOM
    need = int(re.search(r"need (\d+) bytes", str(e.value)).group(1))
    assert need > 64
    np.testing.assert_array_equal(ix.loads_fetch(), before)
    np.testing.assert_array_equal(ix.get_weights(), wc)
    ix.set_weights(None)
    recs = ix.assign(loop.s, loop.t, loop.capacity, LOOP_ITERS, loop.demand)
    check_assign(ix, recs, loop_want(), "retry")
