"""GPU: the flow step and the loop around it (cpd_index_flow_step, _flow_fetch,
_flow_clear, cpd_query_assign_line) against tests/flow_ref.py, which restates
the header in Python ints (pinned by test_flow_cpu.py).  Every value is
compared exactly: the flow table and the weights bit for bit, the signed and
unsigned 128-bit sums, the step, the evaluation count, the loop's records."""
import ctypes as C
import gc
import re

import numpy as np
import pytest

import cpd
import oracle
from assign_ref import BPR, LOOP_ITERS, loop_world
from flow_ref import LINE, ONE, REC_KEYS, FlowRange, loop_line_want, ref_assign_line, ref_flow_step
from graphs import deg8_graph, irregular_graph, lattice_wide, ring2_graph

pytestmark = pytest.mark.gpu
INFO_KEYS = ("lambda_q16", "evals", "g0", "xw0", "tstt", "changed")


class Env:
    def index(self, mode="dense"):
        ix = cpd.Index.streamed(self.dev, self.targets, int(self.off[-1]), mode=mode)
        ix.append(self.off, self.runs)
        return ix

    def walk(self, w, s, t):
        return oracle.table_search(self.g.row_ptr, self.g.dst, w, self.order, self.targets,
                                   self.off, self.runs, s, t)


def make_env(g, ntargets, nq, seed):
    """test_gpu_assign.make_env's world plus a second loading (other queries,
    other demand), so that a second step's D takes both signs."""
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
    e.s2 = rng.integers(0, g.n, nq).astype(np.uint32)
    e.t2 = e.targets[rng.integers(0, ntargets, nq)]
    e.demand2 = rng.integers(0, 90, nq).astype(np.uint32)
    return e


GRAPHS = {  # the five of test_gpu_assign.py: 4, 2, 8, 16 and 16 slots per column
    "synth": lambda: cpd.synth_road_graph(40, 30, seed=7),
    "ring2": ring2_graph,
    "deg8": deg8_graph,
    "irregular": irregular_graph,                            # padding, parallel, 0-weight
    "lattice15": lambda: lattice_wide(20, 15, 15, seed=15),
}


@pytest.fixture(scope="module", params=sorted(GRAPHS))
def wenv(request):
    return request.param, make_env(GRAPHS[request.param](), 30, 800, 23)


@pytest.fixture(scope="module")
def env():
    return make_env(GRAPHS["synth"](), 30, 800, 29)


def check_step(ix, e, X, lam, msg, a=BPR[:2], power=BPR[2]):
    """flow_step(lam) towards the resident table against the reference from
    the flow X (None: no table); returns the new X (a list of ints)."""
    Y = ix.loads_fetch()
    assert Y.shape == (1, e.g.m)
    info = ix.flow_step(e.capacity, lam="line" if lam == LINE else lam, a=a, power=power)
    Xn, w, want = ref_flow_step(e.g.w, Y[0], X, e.capacity, (a[0], a[1], power), lam)
    D = want.pop("D")
    print(f"{msg}: got {({k: info[k] for k in INFO_KEYS})} want {want}; "
          f"D < 0 on {sum(d < 0 for d in D)}, > 0 on {sum(d > 0 for d in D)} edges")
    assert {k: info[k] for k in INFO_KEYS} == want, msg
    assert info["line_ms"] >= 0 and info["apply_ms"] >= 0
    np.testing.assert_array_equal(ix.flow_fetch(), np.array(Xn, np.uint64), err_msg=msg)
    np.testing.assert_array_equal(ix.get_weights(), w, err_msg=msg)
    np.testing.assert_array_equal(ix.loads_fetch(), Y, err_msg=msg)  # the table is only read
    return Xn, D


def two_loadings(ix, e):
    """A first step from the first loading, then the second loading resident."""
    ix.flow_clear()
    ix.loads(e.s, e.t, e.demand)
    X, _ = check_step(ix, e, None, LINE, "init")
    ix.loads(e.s2, e.t2, e.demand2)
    return X


def test_steps_every_width(wenv):
    name, e = wenv
    ix = e.index()
    for lam in (LINE, 0, 1, 32768, ONE):
        X = two_loadings(ix, e)
        assert ix.flow_fetch().tolist() == X
        X2, D = check_step(ix, e, X, lam, f"{name} lambda {lam}")
        assert any(d < 0 for d in D) and any(d > 0 for d in D)
        if lam == 0:
            assert X2 == X
        if lam == ONE:
            assert X2 == [int(y) << 16 for y in ix.loads_fetch()[0]]
    # the last state again, the rule this time, then back towards the first loading
    X = two_loadings(ix, e)
    X, _ = check_step(ix, e, X, LINE, f"{name} line again")
    ix.loads(e.s, e.t, e.demand)
    X, _ = check_step(ix, e, X, LINE, f"{name} third step", a=(7, 2), power=2)
    # walks cost under the weights the step wrote: padding slots still stop a
    # walk, parallel and zero-weight edges cost what the reference says
    w = ix.get_weights()
    cost, hops, fin, _ = ix.query(e.s, e.t)
    rc, rh, rf = e.walk(w, e.s, e.t)
    np.testing.assert_array_equal(cost, rc)
    np.testing.assert_array_equal(hops, rh)
    np.testing.assert_array_equal(fin, rf)
    if name == "irregular":
        src = np.repeat(np.arange(e.g.n), np.diff(e.g.row_ptr.astype(np.int64)))
        pairs = {}
        for ed, key in enumerate(zip(src.tolist(), e.g.dst.tolist())):
            pairs.setdefault(key, []).append(ed)
        par = [v for v in pairs.values() if len(v) > 1]
        assert par and (e.g.w == 0).any()        # the graph has both kinds
        assert (w[e.g.w == 0] == 0).all()        # a zero weight stays zero    # both forms of the search see the new weights (the incumbent tables are rebuilt)
    for form in ("tables", "walks"):
        got = ix.search(e.s, e.t, tables=form)
        want = oracle.cpd_search(e.g.row_ptr, e.g.dst, e.g.w, w, e.order, e.targets, e.off,
                                 e.runs, e.s, e.t)
        for a, b in zip(got[:3], want[:3]):
            np.testing.assert_array_equal(a, b, err_msg=f"{name} {form}")


def test_state_rules(env):
    e = env
    ix = e.index()
    X = two_loadings(ix, e)
    X, _ = check_step(ix, e, X, LINE, "state")
    w = ix.get_weights()
    flow = ix.flow_fetch()
    assert (w != e.g.w).any()
    # the flow table survives cpd_query_loads_clear; a step then has no table to read
    ix.loads_clear()
    np.testing.assert_array_equal(ix.flow_fetch(), flow)
    with pytest.raises(cpd.CpdError) as err:
        ix.flow_step(e.capacity)
    assert err.value.code == cpd.CPD_E_ARG and "no load table" in str(err.value)
    # set_weights(None) restores free flow and leaves the flow table
    ix.set_weights(None)
    np.testing.assert_array_equal(ix.get_weights(), e.g.w)
    np.testing.assert_array_equal(ix.flow_fetch(), flow)
    # sliced and timed tables are refused, everything left as it was
    ix.set_weights(w)
    sliced, _ = ix.loads(e.s, e.t, e.demand, slices=3, slice_moves=5)
    with pytest.raises(cpd.CpdError) as err:
        ix.flow_step(e.capacity)
    assert err.value.code == cpd.CPD_E_ARG and "3 slices" in str(err.value)
    np.testing.assert_array_equal(ix.loads_fetch(), sliced)
    ix.set_weight_sets([None, w])
    ix.timed(e.s, e.t, period=20000, demand=e.demand, loads=True)
    timed = ix.loads_fetch()
    with pytest.raises(cpd.CpdError) as err:
        ix.flow_step(e.capacity, lam=5)
    assert err.value.code == cpd.CPD_E_ARG and "timed" in str(err.value)
    np.testing.assert_array_equal(ix.loads_fetch(), timed)
    np.testing.assert_array_equal(ix.flow_fetch(), flow)
    np.testing.assert_array_equal(ix.get_weights(), w)
    # the step goes on from the kept table once a one-plane loading is back
    ix.loads(e.s, e.t, e.demand)
    check_step(ix, e, X, LINE, "after refusals")
    # flow_clear, then a fetch has nothing to return; clearing twice is fine
    ix.flow_clear()
    ix.flow_clear()
    with pytest.raises(cpd.CpdError) as err:
        ix.flow_fetch()
    assert err.value.code == cpd.CPD_E_ARG and "no flow table" in str(err.value)
    check_step(ix, e, None, 0, "init after clear")  # initialises whatever lambda says


def test_bad_arguments_change_nothing(env):
    e = env
    ix = e.index()
    X = two_loadings(ix, e)
    w, flow, loads = ix.get_weights(), ix.flow_fetch(), ix.loads_fetch()
    zero = e.capacity.copy()
    zero[7] = 0
    bad = [dict(capacity=zero), dict(a=(65536, 1)), dict(a=(1, 0)), dict(a=(1, 65536)),
           dict(power=0), dict(power=5), dict(lam=65537), dict(lam=0xFFFFFFFE)]
    words = ["capacity 0 on edge 7", "a_num 65536", "a_den 0", "a_den 65536", "power 0",
             "power 5", "lambda_q16 65537", "lambda_q16 4294967294"]
    for kw, word in zip(bad, words):
        with pytest.raises(cpd.CpdError) as err:
            ix.flow_step(**dict(dict(capacity=e.capacity), **kw))
        assert err.value.code == cpd.CPD_E_ARG and word in str(err.value), kw
    f = cpd.Vdf(3, 20, 4, 0)  # load_div is ignored, 0 included
    assert cpd.lib.cpd_index_flow_step(ix._h, None, C.byref(f), C.c_uint32(0), None) == cpd.CPD_E_ARG
    assert cpd.lib.cpd_index_flow_step(ix._h, cpd._ptr(e.capacity, cpd.u32p), None,
                                       C.c_uint32(0), None) == cpd.CPD_E_ARG
    ix.prepare(e.s, e.t)
    for kw, word in ((dict(iters=0), "iterations"), (dict(iters=65536), "iterations"),
                     (dict(power=5), "power 5"), (dict(capacity=zero), "capacity 0 on edge 7")):
        with pytest.raises(cpd.CpdError) as err:
            ix.assign_line_run(**dict(dict(capacity=e.capacity, iters=2), **kw))
        assert err.value.code == cpd.CPD_E_ARG and word in str(err.value), kw
    np.testing.assert_array_equal(ix.get_weights(), w)
    np.testing.assert_array_equal(ix.flow_fetch(), flow)
    np.testing.assert_array_equal(ix.loads_fetch(), loads)
    # info may be NULL, load_div 0 is no error
    assert cpd.lib.cpd_index_flow_step(ix._h, cpd._ptr(e.capacity, cpd.u32p), C.byref(f),
                                       C.c_uint32(cpd.STEP_LINE), None) == cpd.CPD_OK
    want = ref_flow_step(e.g.w, loads[0], X, e.capacity, BPR, LINE)
    np.testing.assert_array_equal(ix.flow_fetch(), np.array(want[0], np.uint64))
    # an incomplete index
    part = cpd.Index.streamed(e.dev, e.targets, int(e.off[-1]), mode="dense")
    with pytest.raises(cpd.CpdError) as err:
        part.flow_step(e.capacity)
    assert err.value.code == cpd.CPD_E_ARG and "incomplete" in str(err.value)


def test_range_check_from_both_sides():
    """32769 one-move queries over one edge of ring2 carry 2^47 - 1 exactly
    (32768 x (2^32 - 1) + 32767): accepted; one unit more is CPD_E_RANGE."""
    g = ring2_graph()
    src = np.repeat(np.arange(g.n), np.diff(g.row_ptr.astype(np.int64)))
    edge = next(ed for ed in range(g.m) if g.dst[ed] == (src[ed] + 1) % g.n)
    a, b = int(src[edge]), int(g.dst[edge])
    e = make_env(g, 4, 10, 5)
    e.targets = np.array([b], np.uint32)
    e.off, e.runs = oracle.build_rows(g.row_ptr, g.dst, g.w, e.order, e.targets)
    nq = 32769
    s, t = np.full(nq, a, np.uint32), np.full(nq, b, np.uint32)
    demand = np.full(nq, 0xFFFFFFFF, np.uint32)
    demand[-1] = 32767
    ix = e.index()
    Y, st = ix.loads(s, t, demand)
    assert st["hops"] == nq and int(Y[0].max()) == (1 << 47) - 1 == int(Y[0, edge])
    X, _ = check_step(ix, e, None, LINE, "2^47 - 1")
    assert X[edge] == ((1 << 47) - 1) << 16
    # a second step from there: D = 0 everywhere, then towards an empty loading
    X, _ = check_step(ix, e, X, LINE, "2^47 - 1 again")
    ix.loads(s[:1], t[:1], np.zeros(1, np.uint32))
    X, D = check_step(ix, e, X, 40000, "down from 2^63")  # the product needs 79 bits
    assert D[edge] == -(((1 << 47) - 1) << 16)
    w, flow = ix.get_weights(), ix.flow_fetch()
    demand[-1] = 32768
    Y, _ = ix.loads(s, t, demand)
    assert int(Y[0, edge]) == 1 << 47
    with pytest.raises(FlowRange) as ref_err:
        ref_flow_step(g.w, Y[0], X, e.capacity, BPR)
    for lam in ("line", 0, ONE):
        with pytest.raises(cpd.CpdError) as err:
            ix.flow_step(e.capacity, lam=lam)
        assert err.value.code == cpd.CPD_E_RANGE and "below 2^47)" in str(err.value)
        assert f"on edge {ref_err.value.edge} " in str(err.value) and ref_err.value.edge == edge
    np.testing.assert_array_equal(ix.get_weights(), w)
    np.testing.assert_array_equal(ix.flow_fetch(), flow)
    np.testing.assert_array_equal(ix.loads_fetch(), Y)
    # ... and with no flow table none is made
    ix.flow_clear()
    with pytest.raises(cpd.CpdError) as err:
        ix.flow_step(e.capacity)
    assert err.value.code == cpd.CPD_E_RANGE
    with pytest.raises(cpd.CpdError) as err:
        ix.flow_fetch()
    assert err.value.code == cpd.CPD_E_ARG


def test_with_an_arena_committed():
    assert cpd.lib.cpd_device_arena(C.c_int(0), C.c_uint64(64 << 20), C.c_int(0)) == cpd.CPD_OK
    try:
        e = make_env(GRAPHS["deg8"](), 30, 800, 41)
        ix = e.index()
        for rep in range(2):  # the step works, and repeats after a clear
            X = two_loadings(ix, e)
            X, _ = check_step(ix, e, X, LINE, f"arena {rep}")
            ix.loads(e.s, e.t, e.demand)
            check_step(ix, e, X, 12345, f"arena {rep} explicit")
        del ix, e
        gc.collect()
    finally:
        rc = cpd.lib.cpd_device_arena_release(C.c_int(0))
    assert rc == cpd.CPD_OK, cpd.lib.cpd_last_error().decode()


# --- cpd_query_assign_line -------------------------------------------------

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


def check_loop(ix, recs, want, msg):
    wrecs, wX, ww, (wcost, wplen, wfin, wstats), wloads, _ = want
    for k, (r, w) in enumerate(zip(recs, wrecs)):
        print(f"{msg} k={k + 1}: got {({x: r[x] for x in REC_KEYS})} want {w}")
    assert len(recs) == len(wrecs), msg  # *done
    for k, (r, w) in enumerate(zip(recs, wrecs)):
        assert {x: r[x] for x in REC_KEYS} == {x: w[x] for x in REC_KEYS}, f"{msg} iteration {k + 1}"
        assert min(r["search_ms"], r["loads_ms"], r["vdf_ms"], r["line_ms"]) >= 0
    np.testing.assert_array_equal(ix.flow_fetch(), wX, err_msg=f"{msg} flow")
    np.testing.assert_array_equal(ix.get_weights(), ww, err_msg=f"{msg} weights")
    np.testing.assert_array_equal(ix.loads_fetch()[0], wloads, err_msg=f"{msg} last loading")
    cost, plen, fin, cnt = ix.search_fetch()
    np.testing.assert_array_equal(cost, wcost, err_msg=f"{msg} cost")
    np.testing.assert_array_equal(plen, wplen, err_msg=f"{msg} plen")
    np.testing.assert_array_equal(fin, wfin, err_msg=f"{msg} finished")
    np.testing.assert_array_equal(cnt.astype(np.uint64), wstats, err_msg=f"{msg} counters")


@pytest.mark.parametrize("form", ["tables", "walks"])
@pytest.mark.parametrize("mode", ["dense", "rle"])
def test_assign_line_matches_reference(loop, mode, form):
    ix = loop.index(mode)
    # a flow table left by earlier steps is cleared first
    ix.loads(loop.s, loop.t)
    ix.flow_step(loop.capacity)
    ix.set_weights(None)
    recs = ix.assign_line(loop.s, loop.t, loop.capacity, LOOP_ITERS, loop.demand, a=BPR[:2],
                          power=BPR[2], tables=form)
    check_loop(ix, recs, loop_line_want(), f"{mode} {form}")
    assert len(recs) == LOOP_ITERS
    ix.set_weights(None)
    np.testing.assert_array_equal(ix.get_weights(), loop.g.w)


def test_assign_line_variants(loop):
    ix = loop.index()
    wd = loop_world()
    # lambda = 0 ends the loop early: at these capacities w' = w0, the second
    # search finds the first's routes again and g(0) is 0
    huge = np.full(loop.g.m, 0xFFFFFFFF, np.uint32)
    recs = ix.assign_line(loop.s, loop.t, huge, LOOP_ITERS, loop.demand)
    want = loop_line_want(capacity=huge)
    assert len(want[0]) == 2 and want[0][1]["lambda_q16"] == 0 and want[0][1]["g0"] == 0
    check_loop(ix, recs, want, "early stop")
    assert recs[1]["evals"] == 1 and recs[1]["changed"] == 0
    # the raw call: *done and the records past it
    out = (cpd.AssignLineIter * LOOP_ITERS)()
    done = C.c_uint32(99)
    o = cpd.SearchOpts(1.0, 0.0, -1, -1, 0, 0, 0, 0, 0.0, 0)
    f = cpd.Vdf(3, 20, 4, 1)
    ix.set_weights(None)
    assert cpd.lib.cpd_query_assign_line(ix._h, C.byref(o), C.c_uint64(0),
                                         cpd._ptr(loop.demand, cpd.u32p), cpd._ptr(huge, cpd.u32p),
                                         C.byref(f), C.c_uint32(LOOP_ITERS), out,
                                         C.byref(done)) == cpd.CPD_OK
    assert done.value == 2 and out[1].lambda_q16 == 0 and out[0].lambda_q16 == ONE
    assert bytes(out[2]) == bytes(out[3]) == bytes(C.sizeof(cpd.AssignLineIter))
    # unit demand, a warm start, one iteration
    wc = cpd.synth_congestion(loop.g.w, frac=0.2, lo=1.0, hi=3.0, seed=4)
    ix.set_weights(wc)
    recs = ix.assign_line(loop.s, loop.t, loop.capacity, 2)
    want = ref_assign_line(wd["ref"], wc, wd["s"], wd["t"], None, wd["capacity"], BPR, 2)
    check_loop(ix, recs, want, "warm start, unit demand")
    ix.set_weights(None)
    recs = ix.assign_line(loop.s, loop.t, loop.capacity, 1, loop.demand)
    check_loop(ix, recs, loop_line_want(iters=1), "one iteration")
    # the empty batch: one record, zero apart from lambda, a zeroed flow table, w0
    none = np.zeros(0, np.uint32)
    recs = ix.assign_line(none, none, loop.capacity, 3)
    assert len(recs) == 1
    assert {k: recs[0][k] for k in REC_KEYS} == dict({k: 0 for k in REC_KEYS}, lambda_q16=ONE)
    assert not ix.flow_fetch().any() and not ix.loads_fetch().any()
    np.testing.assert_array_equal(ix.get_weights(), loop.g.w)


def test_assign_line_pool_overflow(loop):
    """cpd_query_assign's pattern: CPD_E_OOM from iteration 1, the state as it
    was (the flow table too), a second call succeeds."""
    ix = loop.index()
    wc = cpd.synth_congestion(loop.g.w, frac=0.2, lo=1.0, hi=3.0, seed=4)
    ix.loads(loop.s, loop.t)
    ix.flow_step(loop.capacity)
    flow = ix.flow_fetch()
    ix.set_weights(wc)
    before = ix.loads_fetch()
    with pytest.raises(cpd.CpdError) as e:
        ix.assign_line(loop.s, loop.t, loop.capacity, LOOP_ITERS, loop.demand, prefix_bytes=64)
    assert e.value.code == cpd.CPD_E_OOM
    assert int(re.search(r"need (\d+) bytes", str(e.value)).group(1)) > 64
    np.testing.assert_array_equal(ix.loads_fetch(), before)
    np.testing.assert_array_equal(ix.get_weights(), wc)
    np.testing.assert_array_equal(ix.flow_fetch(), flow)
    ix.set_weights(None)
    recs = ix.assign_line(loop.s, loop.t, loop.capacity, LOOP_ITERS, loop.demand)
    check_loop(ix, recs, loop_line_want(), "retry")
