"""GPU: the conjugate step and the loop around it (cpd_index_flow_step_conj,
cpd_index_target_fetch, cpd_query_assign_conj) against tests/conj_ref.py, which
restates the header in Python ints (pinned by test_conj_cpu.py).  Every value
is compared exactly: the flow and target tables and the weights bit for bit,
alpha, lambda, the evaluation count, the signed and unsigned 128-bit sums, the
loop's records."""
import ctypes as C
import gc
import re

import numpy as np
import pytest

import cpd
from assign_cases import world
from assign_ref import BPR, loop_world
from conj_ref import (ALPHA_MAX, CONJ, INFO_KEYS, LOOP_ITERS, REC_KEYS, ConjRange, alpha_rule,
                      loop_conj_want, ref_assign_conj, ref_conj_step, restart_capacity, slope)
from flow_ref import LINE, ONE, ref_flow_step
from test_gpu_flow import GRAPHS, Env, make_env

pytestmark = pytest.mark.gpu
U32 = 0xFFFFFFFF


@pytest.fixture(scope="module", params=sorted(GRAPHS))
def wenv(request):
    return request.param, make_env(GRAPHS[request.param](), 30, 800, 23)


@pytest.fixture(scope="module")
def env():
    return make_env(GRAPHS["synth"](), 30, 800, 29)


def check_conj(ix, w0, cap, X, S, alpha, lam, msg, vdf=BPR):
    """flow_step_conj(alpha, lam) towards the resident table against the
    reference from the flow X (None: no table) and the target S (None: none);
    returns (X', S', the reference's info with D)."""
    Y = ix.loads_fetch()
    assert Y.shape == (1, len(w0))
    info = ix.flow_step_conj(cap, alpha="conj" if alpha == CONJ else alpha,
                             lam="line" if lam == LINE else lam, a=vdf[:2], power=vdf[2])
    Xn, Sn, w, want = ref_conj_step(w0, Y[0], X, S, cap, vdf, alpha, lam)
    D = want.pop("D")
    print(f"{msg}: got {({k: info[k] for k in INFO_KEYS})} want {want}")
    assert {k: info[k] for k in INFO_KEYS} == want, msg
    assert min(info["conj_ms"], info["line_ms"], info["apply_ms"]) >= 0
    np.testing.assert_array_equal(ix.flow_fetch(), np.array(Xn, np.uint64), err_msg=msg)
    np.testing.assert_array_equal(ix.target_fetch(), np.array(Sn, np.uint64), err_msg=msg)
    np.testing.assert_array_equal(ix.get_weights(), w, err_msg=msg)
    np.testing.assert_array_equal(ix.loads_fetch(), Y, err_msg=msg)  # the table is only read
    want["D"] = D
    return Xn, Sn, want


def loading(ix, e, second):
    if second:
        ix.loads(e.s2, e.t2, e.demand2)
    else:
        ix.loads(e.s, e.t, e.demand)


def test_steps_every_width(wenv):
    name, e = wenv
    ix = e.index()
    w0, cap = e.g.w, e.capacity
    ix.flow_clear()
    loading(ix, e, False)
    X, S, info = check_conj(ix, w0, cap, None, None, 12345, 7, f"{name} init")
    assert X == S == [int(y) << 16 for y in ix.loads_fetch()[0]]
    second = True
    for alpha, lam in ((0, 32768), (40000, 16384), (ALPHA_MAX, 1), (12345, ONE)):
        loading(ix, e, second)
        second = not second
        X, S, info = check_conj(ix, w0, cap, X, S, alpha, lam, f"{name} alpha {alpha} lambda {lam}")
        D = info["D"]
        assert any(d < 0 for d in D) and any(d > 0 for d in D)
    assert X == S  # lambda = 65536 lands on the target
    # automatic steps; the first finds db = 0 everywhere: alpha 0
    seen = []
    for rep in range(4):
        loading(ix, e, second)
        second = not second
        vdf = BPR if rep != 2 else (7, 2, 2)
        X, S, info = check_conj(ix, w0, cap, X, S, CONJ, LINE, f"{name} automatic {rep}", vdf)
        seen.append(info)
    assert (seen[0]["alpha_q16"], seen[0]["n"], seen[0]["m"]) == (0, 0, 0)
    assert any(i["m"] > 0 and i["n"] != 0 for i in seen[1:])
    # both forms of the search see the weights the step wrote
    w = ix.get_weights()
    import oracle
    for form in ("tables", "walks"):
        got = ix.search(e.s, e.t, tables=form)
        want = oracle.cpd_search(e.g.row_ptr, e.g.dst, e.g.w, w, e.order, e.targets, e.off,
                                 e.runs, e.s, e.t)
        for a, b in zip(got[:3], want[:3]):
            np.testing.assert_array_equal(a, b, err_msg=f"{name} {form}")


def start(ix, e):
    """A flow and a target that differ: init from the first loading, a
    conjugate step half way to the second, the first loading resident again."""
    ix.flow_clear()
    loading(ix, e, False)
    X, S, _ = check_conj(ix, e.g.w, e.capacity, None, None, CONJ, LINE, "start init")
    loading(ix, e, True)
    X, S, _ = check_conj(ix, e.g.w, e.capacity, X, S, 30000, 32768, "start step")
    loading(ix, e, False)
    assert X != S
    return X, S


def test_alpha_zero_is_the_plain_step(env):
    e = env
    a, b = e.index(), e.index()
    for lam in (LINE, 0, 20000, ONE):
        for ix in (a, b):
            start(ix, e)
        ci = a.flow_step_conj(e.capacity, alpha=0, lam="line" if lam == LINE else lam)
        fi = b.flow_step(e.capacity, lam="line" if lam == LINE else lam)
        for k in ("lambda_q16", "evals", "xw0", "tstt", "changed", "g0"):
            assert ci[k] == fi[k], (lam, k)
        assert ci["gy"] == ci["g0"] and ci["alpha_q16"] == 0 and ci["m"] > 0
        np.testing.assert_array_equal(a.flow_fetch(), b.flow_fetch())
        np.testing.assert_array_equal(a.get_weights(), b.get_weights())
        np.testing.assert_array_equal(a.target_fetch(), a.loads_fetch()[0] << np.uint64(16))


def test_state_rules(env):
    e = env
    ix = e.index()
    w0, cap = e.g.w, e.capacity
    with pytest.raises(cpd.CpdError) as err:
        ix.target_fetch()
    assert err.value.code == cpd.CPD_E_ARG and "no target table" in str(err.value)
    X, S = start(ix, e)
    # the plain step drops the target; a conjugate step after it behaves as S = X
    Y = ix.loads_fetch()[0]
    ix.flow_step(cap, lam=1000)
    X = ref_flow_step(w0, Y, X, cap, BPR, 1000)[0]
    np.testing.assert_array_equal(ix.flow_fetch(), np.array(X, np.uint64))
    with pytest.raises(cpd.CpdError) as err:
        ix.target_fetch()
    assert err.value.code == cpd.CPD_E_ARG and "no target table" in str(err.value)
    loading(ix, e, True)
    X, S, info = check_conj(ix, w0, cap, X, None, CONJ, LINE, "after a plain step")
    assert (info["alpha_q16"], info["n"], info["m"]) == (0, 0, 0)
    # loads_clear and set_weights(None) leave both tables
    flow, target = ix.flow_fetch(), ix.target_fetch()
    ix.loads_clear()
    with pytest.raises(cpd.CpdError) as err:
        ix.flow_step_conj(cap)
    assert err.value.code == cpd.CPD_E_ARG and "no load table" in str(err.value)
    ix.set_weights(None)
    np.testing.assert_array_equal(ix.get_weights(), w0)
    np.testing.assert_array_equal(ix.flow_fetch(), flow)
    np.testing.assert_array_equal(ix.target_fetch(), target)
    loading(ix, e, False)
    X, S, info = check_conj(ix, w0, cap, X, S, CONJ, LINE, "after the clears")
    # flow_clear drops both; clearing twice is fine
    ix.flow_clear()
    ix.flow_clear()
    for fetch in (ix.flow_fetch, ix.target_fetch):
        with pytest.raises(cpd.CpdError) as err:
            fetch()
        assert err.value.code == cpd.CPD_E_ARG
    check_conj(ix, w0, cap, None, None, CONJ, 0, "init after clear")


def test_bad_arguments_change_nothing(env):
    e = env
    ix = e.index()
    X, S = start(ix, e)
    w, flow, target, loads = ix.get_weights(), ix.flow_fetch(), ix.target_fetch(), ix.loads_fetch()
    zero = e.capacity.copy()
    zero[7] = 0
    bad = [dict(alpha=ALPHA_MAX + 1), dict(alpha=65536), dict(alpha=0xFFFFFFFE),
           dict(capacity=zero), dict(a=(65536, 1)), dict(a=(1, 0)), dict(a=(1, 65536)),
           dict(power=0), dict(power=5), dict(lam=65537), dict(lam=0xFFFFFFFE)]
    words = ["alpha_q16 64882", "alpha_q16 65536", "alpha_q16 4294967294", "capacity 0 on edge 7",
             "a_num 65536", "a_den 0", "a_den 65536", "power 0", "power 5", "lambda_q16 65537",
             "lambda_q16 4294967294"]
    for kw, word in zip(bad, words):
        with pytest.raises(cpd.CpdError) as err:
            ix.flow_step_conj(**dict(dict(capacity=e.capacity), **kw))
        assert err.value.code == cpd.CPD_E_ARG and word in str(err.value), kw
    f = cpd.Vdf(3, 20, 4, 0)  # load_div is ignored, 0 included
    A, L = C.c_uint32(cpd.ALPHA_CONJ), C.c_uint32(cpd.STEP_LINE)
    assert cpd.lib.cpd_index_flow_step_conj(ix._h, None, C.byref(f), A, L, None) == cpd.CPD_E_ARG
    assert cpd.lib.cpd_index_flow_step_conj(ix._h, cpd._ptr(e.capacity, cpd.u32p), None, A, L,
                                            None) == cpd.CPD_E_ARG
    # sliced and timed tables are refused
    sliced, _ = ix.loads(e.s, e.t, e.demand, slices=3, slice_moves=5)
    with pytest.raises(cpd.CpdError) as err:
        ix.flow_step_conj(e.capacity)
    assert err.value.code == cpd.CPD_E_ARG and "3 slices" in str(err.value)
    ix.set_weight_sets([None, w])
    ix.timed(e.s, e.t, period=20000, demand=e.demand, loads=True)
    with pytest.raises(cpd.CpdError) as err:
        ix.flow_step_conj(e.capacity, alpha=5, lam=5)
    assert err.value.code == cpd.CPD_E_ARG and "timed" in str(err.value)
    loading(ix, e, False)
    ix.prepare(e.s, e.t)
    for kw, word in ((dict(iters=0), "iterations"), (dict(iters=65536), "iterations"),
                     (dict(power=5), "power 5"), (dict(capacity=zero), "capacity 0 on edge 7")):
        with pytest.raises(cpd.CpdError) as err:
            ix.assign_conj_run(**dict(dict(capacity=e.capacity, iters=2), **kw))
        assert err.value.code == cpd.CPD_E_ARG and word in str(err.value), kw
    np.testing.assert_array_equal(ix.get_weights(), w)
    np.testing.assert_array_equal(ix.flow_fetch(), flow)
    np.testing.assert_array_equal(ix.target_fetch(), target)
    np.testing.assert_array_equal(ix.loads_fetch(), loads)
    # info may be NULL, load_div 0 is no error
    assert cpd.lib.cpd_index_flow_step_conj(ix._h, cpd._ptr(e.capacity, cpd.u32p), C.byref(f), A, L,
                                            None) == cpd.CPD_OK
    want = ref_conj_step(e.g.w, loads[0], X, S, e.capacity, BPR)
    np.testing.assert_array_equal(ix.flow_fetch(), np.array(want[0], np.uint64))
    np.testing.assert_array_equal(ix.target_fetch(), np.array(want[1], np.uint64))
    part = cpd.Index.streamed(e.dev, e.targets, int(e.off[-1]), mode="dense")
    with pytest.raises(cpd.CpdError) as err:
        part.flow_step_conj(e.capacity)
    assert err.value.code == cpd.CPD_E_ARG and "incomplete" in str(err.value)


# --- arithmetic edges, tables placed through directed_loads -------------------

def table(m, entries):
    t = [0] * m
    for e, v in entries.items():
        t[int(e)] = int(v)
    return t


def place_state(w, ix, cap, X, Ys, Y):
    """The flow X, the target Ys << 16 and the loading Y resident on ix: the
    plain steps of place_flow, then a conjugate step with alpha = 0 (S = Yq)
    and lambda = 0 (X stays)."""
    w.place_flow(ix, X, cap)
    w.place(ix, Ys)
    ix.flow_step_conj(cap, alpha=0, lam=0)
    S = [y << 16 for y in Ys]
    assert ix.flow_fetch().tolist() == X and ix.target_fetch().tolist() == S
    w.place(ix, Y)
    return S


def edge_scenarios(m, ed):
    """name -> (X, Ys, Y, capacity of the named edges, vdf, what the reference's
    info must show for the scenario to test what its name says)."""
    e0, e1 = int(ed[0]), int(ed[1])
    sat = (65535, 1, 1)  # u = w0 * 65535 >= c << 16 at c = 1 for any w0 >= 2
    return {
        # S < X and Yq < X on one slot, neither difference a multiple of 2^16
        "both negative": (table(m, {e0: (100 << 16) + 1234}), table(m, {e0: 40}),
                          table(m, {e0: 10}), 30, BPR,
                          lambda i: i["n"] > 0 and i["m"] > 0 and i["n"] % 61 == 0
                          and i["n"] // 61 % 91 == 0 and i["alpha_q16"] == ALPHA_MAX),
        # db = 40, df = -30 on the only slot that counts: alpha = 30 / 70
        "mid alpha": (table(m, {e1: 50 << 16}), table(m, {e1: 90}), table(m, {e1: 20}), 30, BPR,
                      lambda i: i["n"] < 0 and i["n"] - i["m"] < 0
                      and i["alpha_q16"] == 30 * 65536 // 70),
        # N > 0 but below M: opposite signs, alpha 0
        "opposite signs": (table(m, {e1: 50 << 16}), table(m, {e1: 90}), table(m, {e1: 60}), 30,
                           BPR, lambda i: 0 < i["n"] < i["m"] and i["alpha_q16"] == 0),
        "h saturates": (table(m, {e0: 5 << 16}), table(m, {e0: 9}), table(m, {e0: 2}), 1, sat,
                        lambda i: i["n"] == -12 * U32 and i["m"] == 16 * U32),
        "past 2^64": (table(m, {e1: (1 << 29) << 16}), table(m, {e0: (1 << 30) - 1, e1: (1 << 30) - 1}),
                      table(m, {e0: 1 << 29}), 1, sat,
                      lambda i: abs(i["n"]) >= 1 << 64 and i["m"] >= 1 << 90),
    }


def test_arithmetic_edges():
    w = world("ring2")
    m, ed = w.g.m, w.loadable()
    assert len(ed) >= 2 and min(int(w.g.w[ed[0]]), int(w.g.w[ed[1]])) >= 2
    ix = w.index()
    for name, (X, Ys, Y, c, vdf, shows) in edge_scenarios(m, ed).items():
        cap = np.full(m, c, np.uint32)
        if name == "h saturates":
            assert slope(w.g.w[ed[0]], 5, 1, *vdf) == U32
        S = place_state(w, ix, cap, X, Ys, Y)
        Xn, Sn, info = check_conj(ix, w.g.w, cap, X, S, CONJ, LINE, name, vdf)
        assert shows(info), (name, info)
        assert info["alpha_q16"] == alpha_rule(info["n"], info["m"])


def test_range_check_from_both_sides():
    w = world("ring2")
    m, ed = w.g.m, w.loadable()
    e0 = int(ed[0])
    cap = np.full(m, 7, np.uint32)
    ix = w.index()
    X, Ys = table(m, {e0: (3 << 16) + 5}), table(m, {e0: 9})
    S = place_state(w, ix, cap, X, Ys, table(m, {e0: (1 << 30) - 1}))
    Xn, Sn, info = check_conj(ix, w.g.w, cap, X, S, CONJ, LINE, "2^30 - 1")
    wts, flow, target = ix.get_weights(), ix.flow_fetch(), ix.target_fetch()
    Y = table(m, {e0: 1 << 30})
    w.place(ix, Y)
    with pytest.raises(ConjRange) as ref_err:
        ref_conj_step(w.g.w, Y, Xn, Sn, cap, BPR)
    for alpha, lam in (("conj", "line"), (0, 0), (ALPHA_MAX, ONE)):
        with pytest.raises(cpd.CpdError) as err:
            ix.flow_step_conj(cap, alpha=alpha, lam=lam)
        assert err.value.code == cpd.CPD_E_RANGE and "below 2^30" in str(err.value)
        assert f"on edge {ref_err.value.edge} " in str(err.value) and ref_err.value.edge == e0
    np.testing.assert_array_equal(ix.get_weights(), wts)
    np.testing.assert_array_equal(ix.flow_fetch(), flow)
    np.testing.assert_array_equal(ix.target_fetch(), target)
    assert ix.loads_fetch()[0].tolist() == Y
    # the plain step still takes that counter (its bound is 2^47) ...
    ix.flow_step(cap, lam=0)
    # ... and with no flow table none is made, nor a target
    ix.flow_clear()
    with pytest.raises(cpd.CpdError) as err:
        ix.flow_step_conj(cap)
    assert err.value.code == cpd.CPD_E_RANGE
    for fetch in (ix.flow_fetch, ix.target_fetch):
        with pytest.raises(cpd.CpdError) as err:
            fetch()
        assert err.value.code == cpd.CPD_E_ARG
    w.place(ix, table(m, {e0: (1 << 30) - 1}))
    check_conj(ix, w.g.w, cap, None, None, CONJ, LINE, "init at 2^30 - 1")


def test_with_an_arena_committed():
    assert cpd.lib.cpd_device_arena(C.c_int(0), C.c_uint64(64 << 20), C.c_int(0)) == cpd.CPD_OK
    try:
        e = make_env(GRAPHS["deg8"](), 30, 800, 41)
        ix = e.index()
        for rep in range(2):  # the step works, and repeats after a clear
            X, S = start(ix, e)
            X, S, _ = check_conj(ix, e.g.w, e.capacity, X, S, CONJ, LINE, f"arena {rep}")
            loading(ix, e, True)
            check_conj(ix, e.g.w, e.capacity, X, S, 12345, 23456, f"arena {rep} explicit")
        del ix, e
        gc.collect()
    finally:
        rc = cpd.lib.cpd_device_arena_release(C.c_int(0))
    assert rc == cpd.CPD_OK, cpd.lib.cpd_last_error().decode()


# --- cpd_query_assign_conj -------------------------------------------------

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
    wrecs, wX, wS, ww, (wcost, wplen, wfin, wstats), wloads = want
    for k, (r, w) in enumerate(zip(recs, wrecs)):
        print(f"{msg} k={k + 1}: got {({x: r[x] for x in REC_KEYS})} want {w}")
    assert len(recs) == len(wrecs), msg  # *done
    for k, (r, w) in enumerate(zip(recs, wrecs)):
        assert {x: r[x] for x in REC_KEYS} == {x: w[x] for x in REC_KEYS}, f"{msg} iteration {k + 1}"
        assert min(r["search_ms"], r["loads_ms"], r["vdf_ms"], r["line_ms"]) >= 0
    np.testing.assert_array_equal(ix.flow_fetch(), wX, err_msg=f"{msg} flow")
    np.testing.assert_array_equal(ix.target_fetch(), wS, err_msg=f"{msg} target")
    np.testing.assert_array_equal(ix.get_weights(), ww, err_msg=f"{msg} weights")
    np.testing.assert_array_equal(ix.loads_fetch()[0], wloads, err_msg=f"{msg} last loading")
    cost, plen, fin, cnt = ix.search_fetch()
    np.testing.assert_array_equal(cost, wcost, err_msg=f"{msg} cost")
    np.testing.assert_array_equal(plen, wplen, err_msg=f"{msg} plen")
    np.testing.assert_array_equal(fin, wfin, err_msg=f"{msg} finished")
    np.testing.assert_array_equal(cnt.astype(np.uint64), wstats, err_msg=f"{msg} counters")


@pytest.mark.parametrize("form", ["tables", "walks"])
@pytest.mark.parametrize("mode", ["dense", "rle"])
def test_assign_conj_matches_reference(loop, mode, form):
    ix = loop.index(mode)
    # a flow and a target left by earlier steps are cleared first
    ix.loads(loop.s, loop.t)
    ix.flow_step_conj(loop.capacity)
    ix.set_weights(None)
    recs = ix.assign_conj(loop.s, loop.t, loop.capacity, LOOP_ITERS, loop.demand, a=BPR[:2],
                          power=BPR[2], tables=form)
    check_loop(ix, recs, loop_conj_want(), f"{mode} {form}")
    assert len(recs) == LOOP_ITERS
    ix.set_weights(None)
    np.testing.assert_array_equal(ix.get_weights(), loop.g.w)


def test_assign_conj_variants(loop):
    ix = loop.index()
    wd = loop_world()
    # the restart rule, then the early stop (test_conj_cpu.py asserts that the
    # reference shows both at these capacities)
    cap = restart_capacity()
    recs = ix.assign_conj(loop.s, loop.t, cap, 8, loop.demand)
    want = loop_conj_want(iters=8, capacity=cap)
    check_loop(ix, recs, want, "restart")
    assert len(recs) < 8
    assert any(r["lambda_q16"] == 0 and r["alpha_q16"] > 0 for r in recs)
    # the early stop at record 2: w' = w0 at these capacities
    huge = np.full(loop.g.m, U32, np.uint32)
    ix.set_weights(None)
    recs = ix.assign_conj(loop.s, loop.t, huge, LOOP_ITERS, loop.demand)
    check_loop(ix, recs, loop_conj_want(capacity=huge), "early stop")
    assert len(recs) == 2 and recs[1]["evals"] == 1 and recs[1]["changed"] == 0
    # the raw call: *done and the records past it
    out = (cpd.AssignConjIter * LOOP_ITERS)()
    done = C.c_uint32(99)
    o = cpd.SearchOpts(1.0, 0.0, -1, -1, 0, 0, 0, 0, 0.0, 0)
    f = cpd.Vdf(3, 20, 4, 1)
    ix.set_weights(None)
    assert cpd.lib.cpd_query_assign_conj(ix._h, C.byref(o), C.c_uint64(0),
                                         cpd._ptr(loop.demand, cpd.u32p), cpd._ptr(huge, cpd.u32p),
                                         C.byref(f), C.c_uint32(LOOP_ITERS), out,
                                         C.byref(done)) == cpd.CPD_OK
    assert done.value == 2 and out[1].lambda_q16 == 0 and out[0].lambda_q16 == ONE
    assert bytes(out[2]) == bytes(out[3]) == bytes(C.sizeof(cpd.AssignConjIter))
    # unit demand and a warm start
    wc = cpd.synth_congestion(loop.g.w, frac=0.2, lo=1.0, hi=3.0, seed=4)
    ix.set_weights(wc)
    recs = ix.assign_conj(loop.s, loop.t, loop.capacity, 3)
    want = ref_assign_conj(wd["ref"], wc, wd["s"], wd["t"], None, wd["capacity"], BPR, 3)
    check_loop(ix, recs, want, "warm start, unit demand")
    # the empty batch: one record, zero apart from lambda, zeroed tables, w0
    none = np.zeros(0, np.uint32)
    recs = ix.assign_conj(none, none, loop.capacity, 3)
    assert len(recs) == 1
    assert {k: recs[0][k] for k in REC_KEYS} == dict({k: 0 for k in REC_KEYS}, lambda_q16=ONE)
    assert not ix.flow_fetch().any() and not ix.target_fetch().any() and not ix.loads_fetch().any()
    np.testing.assert_array_equal(ix.get_weights(), loop.g.w)


def test_assign_conj_pool_overflow(loop):
    """cpd_query_assign_line's pattern: CPD_E_OOM from iteration 1, the state as
    it was (the flow and target tables too), a second call succeeds."""
    ix = loop.index()
    wc = cpd.synth_congestion(loop.g.w, frac=0.2, lo=1.0, hi=3.0, seed=4)
    ix.loads(loop.s, loop.t)
    ix.flow_step_conj(loop.capacity)
    flow, target = ix.flow_fetch(), ix.target_fetch()
    ix.set_weights(wc)
    before = ix.loads_fetch()
    with pytest.raises(cpd.CpdError) as e:
        ix.assign_conj(loop.s, loop.t, loop.capacity, LOOP_ITERS, loop.demand, prefix_bytes=64)
    assert e.value.code == cpd.CPD_E_OOM
    assert int(re.search(r"need (\d+) bytes", str(e.value)).group(1)) > 64
    np.testing.assert_array_equal(ix.loads_fetch(), before)
    np.testing.assert_array_equal(ix.get_weights(), wc)
    np.testing.assert_array_equal(ix.flow_fetch(), flow)
    np.testing.assert_array_equal(ix.target_fetch(), target)
    ix.set_weights(None)
    recs = ix.assign_conj(loop.s, loop.t, loop.capacity, LOOP_ITERS, loop.demand)
    check_loop(ix, recs, loop_conj_want(), "retry")
