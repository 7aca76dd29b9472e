"""GPU: the CPD-heuristic search at every adjacency width.

tests/test_gpu_search.py searches one 4-slot lattice: cpd_search<2,*>.  The
kernel is instantiated for 2^0..2^4 slots per column, and from 8 slots on it
is other code (the expansion's edges are fetched inside the relaxation loop,
the room check reserves 8 or 16 entries); the jump tables and the memoised
walks read the same rows.  Here: ring2 (2 slots), deg8 (8), irregular (16:
zero-weight edges, a self loop, parallel edges, unreachable targets) and a
lattice with out-degrees up to 8 (8 slots, searches hundreds of expansions
deep) — per query cost, plen, finished and the five counters against
oracle.cpd_search, bit-exact, both forms, dense and RLE indexes, and the
overflow accounting with each graph's own margin.
"""
import numpy as np
import pytest

import cpd
import oracle
from graphs import deg8_graph, irregular_graph, lattice_wide, ring2_graph

pytestmark = pytest.mark.gpu

# name -> (graph, log2 of the adjacency slots per column)
CASES = {
    "ring2": (ring2_graph, 1),
    "deg8": (deg8_graph, 3),
    "irregular": (irregular_graph, 4),
    "lattice8": (lambda: lattice_wide(64, 48, 8, seed=8), 3),
}
NQ = 3000
CAP = 64


class Env:
    pass


_ENVS = {}


@pytest.fixture(scope="module", params=sorted(CASES))
def env(request):
    return make_env(request.param)


def make_env(name):
    """Graph, index rows, queries and the congested oracle reference of one
    case, made once."""
    if name not in _ENVS:
        _ENVS[name] = _make_env(name)
    return _ENVS[name]


def _make_env(name):
    e = Env()
    e.name = name
    make, e.shift = CASES[name]
    g = e.g = make()
    deg = int(np.diff(g.row_ptr.astype(np.int64)).max())
    assert (1 << e.shift) >= deg > (1 << e.shift) // 2
    e.plan = cpd.Plan(g)
    e.order = e.plan.order()
    e.dev = cpd.Graph(e.plan, batch=1024)
    e.wc = cpd.synth_congestion(g.w, frac=0.3, lo=1.0, hi=3.0, seed=4)
    for seed in range(31, 41):
        rng = np.random.default_rng(seed)
        e.targets = rng.choice(g.n, size=60, replace=False).astype(np.uint32)
        e.off, e.runs = oracle.build_rows(g.row_ptr, g.dst, g.w, e.order, e.targets)
        e.s = rng.integers(0, g.n, NQ).astype(np.uint32)
        e.t = e.targets[rng.integers(0, len(e.targets), NQ)]
        # the congested reference with the oracle's column count (6th stat)
        e.cong = ref(e, e.wc, columns=True)
        st = e.cong[3]
        # not vacuous: real searches, and some that outgrow a 64-column workspace
        if (st[:, 0] > 1).sum() >= 100 and st[:, 1].max() > CAP:
            break
    else:
        raise AssertionError(f"{e.name}: no seed gives searches past one expansion and {CAP} nodes")
    return e


def ref(e, w_sel, **kw):
    g = e.g
    return oracle.cpd_search(g.row_ptr, g.dst, g.w, w_sel, e.order, e.targets, e.off, e.runs,
                             e.s, e.t, **kw)


def index(e, mode="dense", congested=True):
    ix = cpd.Index.streamed(e.dev, e.targets, int(e.off[-1]), mode=mode)
    ix.append(e.off, e.runs)
    if congested:
        ix.set_weights(e.wc)
    return ix


def check_exact(got, want, msg):
    cost, plen, fin, cnt, st = got
    rc, rp, rf, rs = want
    rs = rs[:, :5]
    np.testing.assert_array_equal(cost, rc, err_msg=f"{msg} cost")
    np.testing.assert_array_equal(plen, rp, err_msg=f"{msg} plen")
    np.testing.assert_array_equal(fin, rf, err_msg=f"{msg} finished")
    np.testing.assert_array_equal(cnt.astype(np.uint64), rs, err_msg=f"{msg} counters")
    assert st["overflow"] == 0, msg
    for k, name in enumerate(("expanded", "inserted", "touched", "updated", "surplus")):
        assert st[name] == int(rs[:, k].sum()), f"{msg} {name}"
    assert st["finished"] == int(rf.sum()) and st["plen"] == int(rp[rf == 1].sum()), msg


@pytest.mark.parametrize("form", ["tables", "walks"])
@pytest.mark.parametrize("mode", ["dense", "rle"])
@pytest.mark.parametrize("opts", [dict(), dict(hscale=1.5), dict(fscale=0.25), dict(k_moves=40),
                                  dict(itrs=7)],
                         ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) or "default")
def test_search_matches_oracle(env, mode, opts, form):
    ix = index(env, mode, congested=False)
    for what, w_sel in (("congested", env.wc), ("free-flow", env.g.w)):
        ix.set_weights(None if w_sel is env.g.w else w_sel)
        got = ix.search(env.s, env.t, tables=form, **opts)
        assert got[4]["tables"] == cpd.SEARCH_FORMS[form]
        check_exact(got, ref(env, w_sel, **opts), f"{env.name} {form} {mode} {what}")


@pytest.mark.parametrize("form", ["tables", "walks"])
def test_search_overflow_margin(env, form):
    """A 64-column workspace.  pushes = inserted + updated bound a search's
    columns and heap entries, and a search stops before a pop whose expansion
    (up to 2^shift pushes: every slot of the column) might not fit; with walks
    the workspace also holds every column the walks met (the oracle's 6th
    stat).  Searches with that room are exact, those that insert more columns
    than there are report finished = 2, and the sums hold every query."""
    rc, rp, rf, rs = env.cong
    cost, plen, fin, cnt, st = index(env).search(env.s, env.t, capacity=CAP, tables=form)
    small = rs[:, 1] + rs[:, 3] + (1 << env.shift) <= CAP
    if form == "walks":
        small &= rs[:, 5] <= CAP
    assert small.sum() > 100
    np.testing.assert_array_equal(cost[small], rc[small])
    np.testing.assert_array_equal(plen[small], rp[small])
    np.testing.assert_array_equal(fin[small], rf[small])
    np.testing.assert_array_equal(cnt[small].astype(np.uint64), rs[small, :5])
    big = rs[:, 1] > CAP
    assert big.any() and (fin[big] == 2).all()
    assert int((fin == 2).sum()) == st["overflow"] >= int(big.sum())
    for k, name in enumerate(("expanded", "inserted", "touched", "updated", "surplus")):
        assert st[name] == int(cnt[:, k].astype(np.uint64).sum()), name


@pytest.mark.parametrize("form", ["tables", "walks"])
def test_search_capacity_escalation(env, form):
    """From 64 columns, resumed at 4x until nothing overflows: the oracle's
    results and counters, every query."""
    got = index(env).search(env.s, env.t, capacity=CAP, capacity_max=4096, tables=form)
    assert got[4]["passes"] >= 2 and got[4]["reruns"] > 0
    # the room check stops a search before the pop whose expansion might not
    # fit (2^shift entries): no expansion is done twice
    assert got[4]["wasted_expanded"] == 0
    check_exact(got, env.cong, f"{env.name} {form}")


@pytest.mark.parametrize("form", ["tables", "walks"])
def test_search_time_limit_virtual_clock(form):
    """One budget under the deterministic clock (a tick per expansion and per
    touched edge), at 8 slots per column."""
    env = make_env("deg8")
    got = index(env).search(env.s, env.t, time_ns=300, virtual_tick_ns=3, tables=form)
    want = ref(env, env.wc, time_ns=300, tick_ns=3)
    assert (want[3][:, 0] < env.cong[3][:, 0]).any()  # the budget cuts some search short
    check_exact(got, want, f"deg8 {form}")
