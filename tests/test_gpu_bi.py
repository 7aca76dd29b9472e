"""GPU: the bi-conjugate step and the loop around it (cpd_index_flow_step_bi,
cpd_index_target2_fetch, cpd_query_assign_bi) against tests/bi_ref.py, which
restates the header in Python ints (pinned by test_bi_cpu.py).  Every value is
compared exactly: the flow table, both target tables and the weights bit for
bit, the branch, mu, nu, the betas, alpha, both lambdas, the evaluation count,
the signed and unsigned 128-bit sums, the loop's records."""
import ctypes as C

import numpy as np
import pytest

import cpd
from assign_cases import world
from assign_ref import BPR
from bi_ref import (AUTO, BI_MAX, INFO_KEYS, LOOP_ITERS, NO_STATE, REC_KEYS, betas, loop_bi_want,
                    loop_capacity, mu_rule, ref_bi_step)
from conj_ref import ConjRange, restart_capacity
from flow_ref import LINE, ONE
from test_gpu_conj import loading, loop, table  # noqa: F401  (loop: the loop world's fixture)
from test_gpu_flow import GRAPHS, make_env

pytestmark = pytest.mark.gpu
U32 = 0xFFFFFFFF


@pytest.fixture(scope="module", params=sorted(GRAPHS))
def wenv(request):
    return request.param, make_env(GRAPHS[request.param](), 30, 800, 23)


@pytest.fixture(scope="module")
def env():
    return make_env(GRAPHS["synth"](), 30, 800, 29)


def arr(T):
    return np.array(T, np.uint64)


def check_state(ix, state, w, msg):
    X, S1, S2, _ = state
    np.testing.assert_array_equal(ix.flow_fetch(), arr(X), err_msg=f"{msg} X")
    np.testing.assert_array_equal(ix.target_fetch(), arr(S1), err_msg=f"{msg} S1")
    if S2 is None:
        with pytest.raises(cpd.CpdError) as err:
            ix.target2_fetch()
        assert err.value.code == cpd.CPD_E_ARG and "no second target" in str(err.value), msg
    else:
        np.testing.assert_array_equal(ix.target2_fetch(), arr(S2), err_msg=f"{msg} S2")
    if w is not None:
        np.testing.assert_array_equal(ix.get_weights(), w, err_msg=f"{msg} weights")


def check_bi(ix, w0, cap, state, mu, nu, lam, msg, vdf=BPR):
    """flow_step_bi(mu, nu, lam) towards the resident table against the
    reference from state = (X, S1, S2, lambda_prev); returns (the new state,
    the reference's info)."""
    Y = ix.loads_fetch()
    assert Y.shape == (1, len(w0))
    info = ix.flow_step_bi(cap, mu="auto" if mu == AUTO else mu, nu="auto" if nu == AUTO else nu,
                           lam="line" if lam == LINE else lam, a=vdf[:2], power=vdf[2])
    new, w, want = ref_bi_step(w0, Y[0], state, cap, vdf, mu, nu, lam)
    want.pop("D")
    print(f"{msg}: got {({k: info[k] for k in INFO_KEYS})} want {want}")
    assert {k: info[k] for k in INFO_KEYS} == want, msg
    assert min(info["bi_ms"], info["line_ms"], info["apply_ms"]) >= 0
    check_state(ix, new, w, msg)
    np.testing.assert_array_equal(ix.loads_fetch(), Y, err_msg=msg)  # the table is only read
    return new, want


def start(ix, e, lams=(20000, 30000)):
    """Branch 0 from the first loading, branch 1 towards the second and branch 2
    towards the first again, with explicit lambdas: a state in which X, S1 and
    S2 all differ and lambda_prev is below 65536; the second loading is left
    resident."""
    w0, cap = e.g.w, e.capacity
    ix.flow_clear()
    loading(ix, e, False)
    st, info = check_bi(ix, w0, cap, NO_STATE, AUTO, AUTO, LINE, "start: branch 0")
    assert info["branch"] == 0 and st[2] is None and st[3] == ONE
    loading(ix, e, True)
    st, info = check_bi(ix, w0, cap, st, AUTO, AUTO, lams[0], "start: branch 1")
    assert info["branch"] == 1 and st[3] == lams[0]
    loading(ix, e, False)
    st, info = check_bi(ix, w0, cap, st, 20000, 30000, lams[1], "start: branch 2")
    assert info["branch"] == 2 and st[3] == lams[1]
    loading(ix, e, True)
    assert st[0] != st[1] and st[1] != st[2]
    return st


# automatic, explicit mu and nu, each alone (under another delay function too),
# a plain step, both at the cap, and the line rule
STEPS = ((AUTO, AUTO, 25000, BPR), (AUTO, AUTO, 18000, BPR), (40000, 50000, 12345, BPR),
         (70000, AUTO, 22222, BPR), (AUTO, 9999, 1, (7, 2, 2)), (0, 0, 30000, BPR),
         (BI_MAX, BI_MAX, 30000, BPR), (AUTO, AUTO, LINE, BPR))


def test_steps_every_width(wenv):
    name, e = wenv
    ix = e.index()
    w0, cap = e.g.w, e.capacity
    st = start(ix, e)
    seen = []
    second = False
    # a third loading: against it the sums give the rules a mu and a nu above 0
    ix.loads(e.s, e.t2, e.demand)
    for k, (mu, nu, lam, vdf) in enumerate(STEPS):
        st, info = check_bi(ix, w0, cap, st, mu, nu, lam, f"{name} step {k} mu {mu} nu {nu}", vdf)
        loading(ix, e, second)
        second = not second
        seen.append(info)
    assert all(i["branch"] == 2 for i in seen)
    assert seen[0]["mu_q16"] > 0 and seen[0]["nu_q16"] > 0       # the rules, both non-zero
    assert seen[3]["nu_q16"] > 70000 > 70000 * 12345 // (ONE - 12345)   # nu1 > 0 as well
    assert all(i["a2"] != 0 and i["b2"] != 0 and i["b1"] > 0 for i in seen)
    assert seen[5]["beta0_q16"] == ONE and seen[6]["beta0_q16"] == 255 and st[1] != st[2]


def test_branch_1_is_the_conjugate_step(env):
    """Both reasons for branch 1, automatic and with nu = 0, against
    flow_step_conj on a second index prepared identically."""
    e = env
    w0, cap = e.g.w, e.capacity
    a, b = e.index(), e.index()
    for reason in ("no S2", "lambda_prev 65536"):
        for nu, alpha, lam in ((AUTO, "conj", LINE), (0, 0, 20000)):
            for ix in (a, b):
                st = start(ix, e)
                if reason == "no S2":
                    ix.flow_step_conj(cap, alpha=30000, lam=30000)  # drops S2, moves X and S1
                else:
                    st, _ = check_bi(ix, w0, cap, st, 5000, 6000, ONE, "onto the target")
                    assert st[0] == st[1] and st[3] == ONE
                loading(ix, e, False)
            X, S1 = a.flow_fetch().tolist(), a.target_fetch().tolist()
            st = (X, S1, None if reason == "no S2" else st[2], ONE)
            msg = f"{reason} nu {nu} lambda {lam}"
            new, bi = check_bi(a, w0, cap, st, 77, nu, lam, msg)
            ci = b.flow_step_conj(cap, alpha=alpha, lam="line" if lam == LINE else lam)
            assert bi["branch"] == 1 and new[2] == S1
            for kb, kc in (("a1", "n"), ("b1", "m")) + tuple(
                    (k, k) for k in ("alpha_q16", "lambda_q16", "evals", "gy", "xw0", "g0",
                                     "tstt", "changed")):
                assert bi[kb] == ci[kc], (msg, kb)
            np.testing.assert_array_equal(a.flow_fetch(), b.flow_fetch(), err_msg=msg)
            np.testing.assert_array_equal(a.target_fetch(), b.target_fetch(), err_msg=msg)
            np.testing.assert_array_equal(a.get_weights(), b.get_weights(), err_msg=msg)
            with pytest.raises(cpd.CpdError):
                b.target2_fetch()
    # no target table at all: S2 takes X
    st = start(a, e)
    a.flow_step(cap, lam=0)
    st, info = check_bi(a, w0, cap, (st[0], None, None, ONE), AUTO, AUTO, 15000, "after a plain step")
    assert info["branch"] == 1 and info["alpha_q16"] == 0 and st[2] != st[1]
    # an explicit nu other than 0 is refused in this branch, nothing changed
    a.flow_step_conj(cap, alpha=0, lam=0)
    flow, target, wts = a.flow_fetch(), a.target_fetch(), a.get_weights()
    for nu in (1, BI_MAX):
        with pytest.raises(cpd.CpdError) as err:
            a.flow_step_bi(cap, nu=nu)
        assert err.value.code == cpd.CPD_E_ARG and f"nu_q16 {nu} " in str(err.value)
    np.testing.assert_array_equal(a.flow_fetch(), flow)
    np.testing.assert_array_equal(a.target_fetch(), target)
    np.testing.assert_array_equal(a.get_weights(), wts)


def test_other_steps_drop_s2_and_clears_leave_it(env):
    e = env
    w0, cap = e.g.w, e.capacity
    ix = e.index()
    with pytest.raises(cpd.CpdError) as err:
        ix.target2_fetch()
    assert err.value.code == cpd.CPD_E_ARG and "no second target" in str(err.value)
    for drop in (lambda: ix.flow_step(cap, lam=100), lambda: ix.flow_step_conj(cap, lam=100),
                 ix.flow_clear):
        st = start(ix, e)
        assert ix.target2_fetch().tolist() == st[2]
        drop()
        with pytest.raises(cpd.CpdError) as err:
            ix.target2_fetch()
        assert err.value.code == cpd.CPD_E_ARG and "no second target" in str(err.value)
    # loads_clear and set_weights(None) leave all three tables and lambda_prev
    st = start(ix, e)
    ix.loads_clear()
    with pytest.raises(cpd.CpdError) as err:
        ix.flow_step_bi(cap)
    assert err.value.code == cpd.CPD_E_ARG and "no load table" in str(err.value)
    ix.set_weights(None)
    np.testing.assert_array_equal(ix.get_weights(), w0)
    check_state(ix, st, None, "after the clears")
    loading(ix, e, True)
    st, info = check_bi(ix, w0, cap, st, AUTO, AUTO, LINE, "after the clears")
    assert info["branch"] == 2 and info["lambda_prev_q16"] == 30000


def test_bad_arguments_change_nothing(env):
    e = env
    ix = e.index()
    st = start(ix, e)
    w, loads = ix.get_weights(), ix.loads_fetch()
    zero = e.capacity.copy()
    zero[7] = 0
    bad = [dict(mu=BI_MAX + 1), dict(nu=BI_MAX + 1), dict(mu=0xFFFFFFFE), dict(nu=0xFFFFFFFE),
           dict(capacity=zero), dict(a=(65536, 1)), dict(a=(1, 0)), dict(power=0), dict(power=5),
           dict(lam=65537), dict(lam=0xFFFFFFFE)]
    words = ["mu_q16 8388608", "nu_q16 8388608", "mu_q16 4294967294", "nu_q16 4294967294",
             "capacity 0 on edge 7", "a_num 65536", "a_den 0", "power 0", "power 5",
             "lambda_q16 65537", "lambda_q16 4294967294"]
    for kw, word in zip(bad, words):
        with pytest.raises(cpd.CpdError) as err:
            ix.flow_step_bi(**dict(dict(capacity=e.capacity), **kw))
        assert err.value.code == cpd.CPD_E_ARG and word in str(err.value), kw
        assert "bi-conjugate step" in str(err.value)
    ix.prepare(e.s, e.t)
    for kw, word in ((dict(iters=0), "iterations"), (dict(iters=65536), "iterations"),
                     (dict(power=5), "power 5"), (dict(capacity=zero), "capacity 0 on edge 7")):
        with pytest.raises(cpd.CpdError) as err:
            ix.assign_bi_run(**dict(dict(capacity=e.capacity, iters=2), **kw))
        assert err.value.code == cpd.CPD_E_ARG and word in str(err.value), kw
        assert "assign bi" in str(err.value)
    check_state(ix, st, w, "after the refusals")
    np.testing.assert_array_equal(ix.loads_fetch(), loads)
    # info may be NULL; lambda_prev was left alone too: the next step reads it
    f = cpd.Vdf(3, 20, 4, 0)
    A = C.c_uint32(cpd.BI_AUTO)
    assert cpd.lib.cpd_index_flow_step_bi(ix._h, cpd._ptr(e.capacity, cpd.u32p), C.byref(f), A, A,
                                          C.c_uint32(cpd.STEP_LINE), None) == cpd.CPD_OK
    new, _, info = ref_bi_step(e.g.w, loads[0], st, e.capacity, BPR)
    assert info["branch"] == 2
    check_state(ix, new, None, "NULL info")


# --- arithmetic edges, tables placed through directed_loads -------------------

def place_bi(w, ix, cap, X, Ys1, Ys2, lp, Y):
    """X, S1 = Ys1 << 16, S2 = Ys2 << 16 and lambda_prev = lp resident with the
    loading Y: X0 is placed such that branch 1's explicit step lp from X0
    towards S1 lands on X — X0 = S1 - (S1 - X) * 65536 / (65536 - lp) must be
    exact, the caller sees to it — after an alpha = 0 conjugate step put Ys2 in
    S1."""
    S1, S2 = [y << 16 for y in Ys1], [y << 16 for y in Ys2]
    X0 = []
    for x, s in zip(X, S1):
        q, r = divmod((s - x) * ONE, ONE - lp)
        assert r == 0 and s - q >= 0
        X0.append(s - q)
    assert [x0 + ((lp * (s - x0)) >> 16) for x0, s in zip(X0, S1)] == X
    w.place_flow(ix, X0, cap)
    w.place(ix, Ys2)
    ix.flow_step_conj(cap, alpha=0, lam=0)     # S1 = Ys2 << 16, X0 stays, S2 dropped
    w.place(ix, Ys1)
    info = ix.flow_step_bi(cap, nu=0, lam=lp)  # branch 1, alpha 0: S2 <- S1, S1 <- Yq
    assert info["branch"] == 1 and info["lambda_q16"] == lp
    st = (X, S1, S2, lp)
    check_state(ix, st, None, "placed")
    w.place(ix, Y)
    return st


def edge_scenarios(m, ed):
    """name -> (X, Ys1, Ys2, lp, Y, capacity, vdf, what the reference's info
    must show for the scenario to test what its name says).  lp = 32768: X0 =
    2 X - S1."""
    e0, e1 = int(ed[0]), int(ed[1])
    sat = (65535, 1, 1)  # h saturates at c = 1 for any w0 >= 2
    half = 32768
    return {
        # d2 from a negative bracket that is no multiple of 2^32; A2 < 0 < B2
        "d2 floors": (table(m, {e0: (60 << 16) + 32768}), table(m, {e0: 80}), table(m, {e0: 90}),
                      half, table(m, {e0: 10}), 30, BPR,
                      lambda i: i["mu_q16"] > 0 and i["nu_q16"] > 0 and i["a2"] < 0 < i["b2"]),
        # |A2| >= 128 |B2|: mu saturates (d2 = 25, df = 5000, e21 = -1 on the one slot)
        "mu saturates": (table(m, {e1: 50 << 16}), table(m, {e1: 100}), table(m, {e1: 99}), half,
                         table(m, {e1: 5050}), 30, BPR,
                         lambda i: i["mu_q16"] == BI_MAX and i["a2"] > 0 > i["b2"]
                         and abs(i["a2"]) >= 128 * abs(i["b2"])),
        # A2 and B2 of one sign, A1 >= 0: a plain step
        "both zero": (table(m, {e1: 50 << 16}), table(m, {e1: 60}), table(m, {e1: 90}), half,
                      table(m, {e1: 70}), 30, BPR,
                      lambda i: (i["mu_q16"], i["nu_q16"], i["beta0_q16"]) == (0, 0, ONE)
                      and i["a2"] > 0 and i["b2"] > 0 and i["a1"] > 0),
        "h saturates": (table(m, {e0: 5 << 16}), table(m, {e0: 9}), table(m, {e0: 11}), half,
                        table(m, {e0: 2}), 1, sat,
                        lambda i: i["b1"] == 16 * U32 and i["a1"] == -12 * U32),
        "past 2^64": (table(m, {e1: (1 << 28) << 16}), table(m, {e1: (1 << 29)}),
                      table(m, {e0: (1 << 30) - 1, e1: (1 << 30) - 2}), half,
                      table(m, {e0: 1 << 29}), 1, sat,
                      lambda i: i["b1"] >= 1 << 64 and abs(i["a2"]) >= 1 << 64
                      and abs(i["b2"]) >= 1 << 64),
    }


def test_arithmetic_edges():
    w = world("ring2")
    m, ed = w.g.m, w.loadable()
    assert len(ed) >= 2 and min(int(w.g.w[ed[0]]), int(w.g.w[ed[1]])) >= 2
    ix = w.index()
    for name, (X, Ys1, Ys2, lp, Y, c, vdf, shows) in edge_scenarios(m, ed).items():
        cap = np.full(m, c, np.uint32)
        st = place_bi(w, ix, cap, X, Ys1, Ys2, lp, Y)
        new, info = check_bi(ix, w.g.w, cap, st, AUTO, AUTO, LINE, name, vdf)
        assert info["branch"] == 2 and shows(info), (name, info)
        assert info["mu_q16"] == mu_rule(info["a2"], info["b2"])
        assert (info["beta0_q16"], info["beta1_q16"], info["beta2_q16"]) == \
            betas(info["mu_q16"], info["nu_q16"])


def test_parallel_edges():
    """The irregular graph has parallel edges (and padding slots and 0-weight
    edges): each of a pair keeps its own X, S1 and S2."""
    e = make_env(GRAPHS["irregular"](), 30, 800, 37)
    src = np.repeat(np.arange(e.g.n), np.diff(e.g.row_ptr.astype(np.int64)))
    pairs = {}
    for ed, key in enumerate(zip(src.tolist(), e.g.dst.tolist())):
        pairs.setdefault(key, []).append(ed)
    par = [v for v in pairs.values() if len(v) > 1]
    assert par
    ix = e.index()
    st = start(ix, e)
    st, info = check_bi(ix, e.g.w, e.capacity, st, AUTO, AUTO, LINE, "parallel")
    assert info["branch"] == 2
    X, S1, S2, _ = st
    assert any(len({X[i] for i in v}) > 1 or len({S1[i] for i in v}) > 1 for v in par)


def test_range_check_from_both_sides():
    w = world("ring2")
    m, ed = w.g.m, w.loadable()
    e0 = int(ed[0])
    cap = np.full(m, 7, np.uint32)
    ix = w.index()
    st = place_bi(w, ix, cap, table(m, {e0: (6 << 16)}), table(m, {e0: 9}), table(m, {e0: 4}),
                  32768, table(m, {e0: (1 << 30) - 1}))
    st, info = check_bi(ix, w.g.w, cap, st, AUTO, AUTO, 1000, "2^30 - 1")
    assert info["branch"] == 2
    wts = ix.get_weights()
    Y = table(m, {e0: 1 << 30})
    w.place(ix, Y)
    with pytest.raises(ConjRange) as ref_err:
        ref_bi_step(w.g.w, Y, st, cap, BPR)
    for mu, nu, lam in (("auto", "auto", "line"), (0, 0, 0), (BI_MAX, BI_MAX, ONE)):
        with pytest.raises(cpd.CpdError) as err:
            ix.flow_step_bi(cap, mu=mu, nu=nu, lam=lam)
        assert err.value.code == cpd.CPD_E_RANGE and "below 2^30" in str(err.value)
        assert f"on edge {ref_err.value.edge} " in str(err.value) and ref_err.value.edge == e0
    # X, S1, S2 and the weights unchanged, and lambda_prev: the next step reads 1000
    check_state(ix, st, wts, "refused in branch 2")
    assert ix.loads_fetch()[0].tolist() == Y
    w.place(ix, table(m, {e0: 77}))
    st, info = check_bi(ix, w.g.w, cap, st, AUTO, AUTO, ONE, "after the refusal")
    assert info["branch"] == 2 and info["lambda_prev_q16"] == 1000
    # refused in branch 1 (lambda_prev = 65536 now): S2 keeps its values
    wts = ix.get_weights()
    w.place(ix, Y)
    with pytest.raises(cpd.CpdError) as err:
        ix.flow_step_bi(cap)
    assert err.value.code == cpd.CPD_E_RANGE
    check_state(ix, st, wts, "refused in branch 1")
    # and in branch 0 no table is made
    ix.flow_clear()
    with pytest.raises(cpd.CpdError) as err:
        ix.flow_step_bi(cap)
    assert err.value.code == cpd.CPD_E_RANGE
    for fetch in (ix.flow_fetch, ix.target_fetch, ix.target2_fetch):
        with pytest.raises(cpd.CpdError) as err:
            fetch()
        assert err.value.code == cpd.CPD_E_ARG


# --- cpd_query_assign_bi ------------------------------------------------------

def check_loop(ix, recs, want, msg):
    wrecs, wstate, ww, (wcost, wplen, wfin, wstats), wloads = want
    for k, (r, w) in enumerate(zip(recs, wrecs)):
        print(f"{msg} k={k + 1}: got {({x: r[x] for x in REC_KEYS})} want {w}")
    assert len(recs) == len(wrecs), msg  # *done
    for k, (r, w) in enumerate(zip(recs, wrecs)):
        assert {x: r[x] for x in REC_KEYS} == {x: w[x] for x in REC_KEYS}, f"{msg} iteration {k + 1}"
        assert min(r["search_ms"], r["loads_ms"], r["vdf_ms"], r["line_ms"]) >= 0
    check_state(ix, wstate, ww, msg)
    np.testing.assert_array_equal(ix.loads_fetch()[0], wloads, err_msg=f"{msg} last loading")
    cost, plen, fin, cnt = ix.search_fetch()
    np.testing.assert_array_equal(cost, wcost, err_msg=f"{msg} cost")
    np.testing.assert_array_equal(plen, wplen, err_msg=f"{msg} plen")
    np.testing.assert_array_equal(fin, wfin, err_msg=f"{msg} finished")
    np.testing.assert_array_equal(cnt.astype(np.uint64), wstats, err_msg=f"{msg} counters")


@pytest.mark.parametrize("form", ["tables", "walks"])
@pytest.mark.parametrize("mode", ["dense", "rle"])
def test_assign_bi_matches_reference(loop, mode, form):
    ix = loop.index(mode)
    # a flow and targets left by earlier steps are cleared first
    ix.loads(loop.s, loop.t)
    for lam in (ONE, 30000, 30000):
        ix.flow_step_bi(loop.capacity, lam=lam)
    ix.set_weights(None)
    recs = ix.assign_bi(loop.s, loop.t, loop_capacity(), LOOP_ITERS, loop.demand, a=BPR[:2],
                        power=BPR[2], tables=form)
    check_loop(ix, recs, loop_bi_want(), f"{mode} {form}")
    # test_bi_cpu.py asserts that the reference shows these
    assert len(recs) == LOOP_ITERS and [r["branch"] for r in recs[:3]] == [0, 1, 2]
    assert any(r["branch"] == 2 and r["mu_q16"] > 0 for r in recs)
    assert any(r["branch"] == 2 and r["nu_q16"] > 0 for r in recs)


def test_assign_bi_variants(loop):
    ix = loop.index()
    # the restart rule, then the early stop (test_bi_cpu.py asserts that the
    # reference shows both at these capacities)
    cap = restart_capacity()
    recs = ix.assign_bi(loop.s, loop.t, cap, 12, loop.demand)
    check_loop(ix, recs, loop_bi_want(iters=12, capacity=cap), "restart")
    assert len(recs) < 12
    assert any(r["lambda_q16"] == 0 and (r["mu_q16"] or r["nu_q16"]) for r in recs)
    # the early stop at record 2: w' = w0 at these capacities
    huge = np.full(loop.g.m, U32, np.uint32)
    ix.set_weights(None)
    recs = ix.assign_bi(loop.s, loop.t, huge, LOOP_ITERS, loop.demand)
    check_loop(ix, recs, loop_bi_want(capacity=huge), "early stop")
    assert len(recs) == 2 and recs[1]["evals"] == 1 and recs[1]["changed"] == 0
    # the raw call: *done and the records past it
    out = (cpd.AssignBiIter * LOOP_ITERS)()
    done = C.c_uint32(99)
    o = cpd.SearchOpts(1.0, 0.0, -1, -1, 0, 0, 0, 0, 0.0, 0)
    f = cpd.Vdf(3, 20, 4, 1)
    ix.set_weights(None)
    assert cpd.lib.cpd_query_assign_bi(ix._h, C.byref(o), C.c_uint64(0),
                                       cpd._ptr(loop.demand, cpd.u32p), cpd._ptr(huge, cpd.u32p),
                                       C.byref(f), C.c_uint32(LOOP_ITERS), out,
                                       C.byref(done)) == cpd.CPD_OK
    assert done.value == 2 and out[1].lambda_q16 == 0 and out[0].lambda_q16 == ONE
    assert (out[0].branch, out[1].branch, out[1].beta0_q16) == (0, 1, ONE)
    assert bytes(out[2]) == bytes(out[3]) == bytes(C.sizeof(cpd.AssignBiIter))
    # the empty batch: one record, zero apart from lambda, zeroed tables, w0
    none = np.zeros(0, np.uint32)
    recs = ix.assign_bi(none, none, loop.capacity, 3)
    assert len(recs) == 1
    assert {k: recs[0][k] for k in REC_KEYS} == dict({k: 0 for k in REC_KEYS}, lambda_q16=ONE)
    assert not ix.flow_fetch().any() and not ix.target_fetch().any() and not ix.loads_fetch().any()
    with pytest.raises(cpd.CpdError):
        ix.target2_fetch()
    np.testing.assert_array_equal(ix.get_weights(), loop.g.w)


def test_assign_bi_pool_overflow(loop):
    """cpd_query_assign_conj's pattern: CPD_E_OOM from iteration 1, the state as
    it was (all three tables and lambda_prev), a second call succeeds."""
    ix = loop.index()
    ix.loads(loop.s, loop.t)
    for lam in (ONE, 30000, 20000):
        ix.flow_step_bi(loop.capacity, lam=lam)
    state = (ix.flow_fetch().tolist(), ix.target_fetch().tolist(), ix.target2_fetch().tolist(),
             20000)
    wc = cpd.synth_congestion(loop.g.w, frac=0.2, lo=1.0, hi=3.0, seed=4)
    ix.set_weights(wc)
    before = ix.loads_fetch()
    with pytest.raises(cpd.CpdError) as e:
        ix.assign_bi(loop.s, loop.t, loop.capacity, LOOP_ITERS, loop.demand, prefix_bytes=64)
    assert e.value.code == cpd.CPD_E_OOM
    np.testing.assert_array_equal(ix.loads_fetch(), before)
    check_state(ix, state, wc, "after the overflow")
    info = ix.flow_step_bi(loop.capacity, lam=0)
    assert info["branch"] == 2 and info["lambda_prev_q16"] == 20000
    ix.set_weights(None)
    recs = ix.assign_bi(loop.s, loop.t, loop_capacity(), LOOP_ITERS, loop.demand)
    check_loop(ix, recs, loop_bi_want(), "retry")


def test_ledger_entry(env):
    """bi_sums_target: three launches a step and the stated byte model — 60,
    68 and 84 bytes a slot in branches 0, 1 and 2 — beside the line search's
    and the apply's entries."""
    e = env
    ix = e.index()
    cap = e.capacity
    nslots = e.g.n << 2  # synth: 4 slots a column
    e.dev.timing(True)
    try:
        ix.flow_clear()
        loading(ix, e, False)
        for k, (lam, per_slot) in enumerate(((LINE, 60.0), (20000, 68.0), (LINE, 84.0), (7, 84.0))):
            e.dev.timing_reset()
            info = ix.flow_step_bi(cap, lam="line" if lam == LINE else lam)
            assert info["branch"] == min(k, 2)
            led = e.dev.timing_get()
            assert "conj_sums_target" not in led
            t = led["bi_sums_target"]
            assert (t["launches"], t["bytes"]) == (3, nslots * per_slot), (k, t)
            assert t["ms"] >= 0
            # the initialising step makes one evaluation and reports none
            evals = info["evals"] if k else 1
            assert (led["flow_line_eval"]["launches"], led["flow_line_eval"]["bytes"]) == \
                (evals, nslots * 28.0 * evals)
            assert (led["flow_apply"]["launches"], led["flow_apply"]["bytes"]) == (1, nslots * 44.0)
            loading(ix, e, k % 2 == 0)
    finally:
        e.dev.timing(False)
