"""GPU: search paths (cpd_query_search_paths / Index.search_paths) against the
Python restatement ref_search_paths (tests/search_paths_ref.py, pinned to the
oracle by test_search_paths_cpu.py), node for node: the A* tree's chain from s
to the incumbent's node, then the CPD walk to t.  cost / plen / finished and
the counters stay the oracle's, as test_gpu_search.py checks them for
cpd_query_search."""
import re

import numpy as np
import pytest

import cpd
import oracle
from graphs import irregular_graph, lattice_wide, ring2_graph
from search_paths_ref import SearchPathsRef, flatten, ref_search_paths, reopened_graph

pytestmark = pytest.mark.gpu

OPTS = [dict(), dict(hscale=1.5), dict(fscale=0.25), dict(hscale=0.5, fscale=0.1),
        dict(k_moves=40), dict(itrs=7), dict(k_moves=0, itrs=200), dict(itrs=0)]
IDS = [",".join(f"{k}={v}" for k, v in o.items()) or "default" for o in OPTS]
NQ = 3000


class Env:
    def want(self, congested=True, **opts):
        """ref_search_paths of the env's queries, computed once per option set."""
        key = (congested, tuple(sorted(opts.items())))
        if key not in self.cache:
            w = self.wc if congested else self.g.w
            c, p, f, st, paths, _ = ref_search_paths(self.ref, w, self.s, self.t, **opts)
            self.cache[key] = (c, p, f, st) + flatten(paths)
        return self.cache[key]

    def index(self, mode="dense", congested=True):
        ix = cpd.Index.streamed(self.dev, self.targets, int(self.off[-1]), mode=mode)
        ix.append(self.off, self.runs)
        if congested:
            ix.set_weights(self.wc)
        return ix


def make_env(g, seed, frac):
    e = Env()
    e.g = g
    e.plan = cpd.Plan(g)
    e.order = e.plan.order()
    e.dev = cpd.Graph(e.plan, batch=1024)
    rng = np.random.default_rng(seed)
    e.targets = rng.choice(g.n, size=60, replace=False).astype(np.uint32)
    e.off, e.runs = oracle.build_rows(g.row_ptr, g.dst, g.w, e.order, e.targets)
    e.s = rng.integers(0, g.n, NQ).astype(np.uint32)
    e.t = e.targets[rng.integers(0, len(e.targets), NQ)]
    e.s[0] = e.t[0]  # a query with s == t
    e.wc = cpd.synth_congestion(g.w, frac=frac, lo=1.0, hi=3.0, seed=4)
    e.ref = SearchPathsRef(g, e.order, e.targets, e.off, e.runs)
    e.cache = {}
    return e


@pytest.fixture(scope="module")
def env():
    """The graph, targets and congestion of test_gpu_search.py."""
    return make_env(cpd.synth_road_graph(64, 48, seed=31), 31, 0.2)


def check(got, want, msg=""):
    """Offsets, nodes, results and counters exact; the sums as the search's."""
    off, nodes, cost, plen, fin, cnt, st = got
    rc, rp, rf, rs, roff, rnodes = want
    assert off.dtype == np.uint64 and off[0] == 0 and len(off) == len(rc) + 1
    np.testing.assert_array_equal(cost, rc, err_msg=f"{msg} cost")
    np.testing.assert_array_equal(plen, rp, err_msg=f"{msg} plen")
    np.testing.assert_array_equal(fin, rf, err_msg=f"{msg} finished")
    np.testing.assert_array_equal(cnt.astype(np.uint64), rs, err_msg=f"{msg} counters")
    np.testing.assert_array_equal(off, roff, err_msg=f"{msg} offsets")
    np.testing.assert_array_equal(nodes, rnodes, err_msg=f"{msg} nodes")
    assert st["overflow"] == 0 and st["expanded"] == int(rs[:, 0].sum()), msg
    assert st["finished"] == int(rf.sum()) and st["plen"] == int(rp[rf == 1].sum()), msg
    assert st["paths"]["nodes"] == int(roff[-1]), msg


@pytest.mark.parametrize("form", ["tables", "walks"])
@pytest.mark.parametrize("mode", ["dense", "rle"])
@pytest.mark.parametrize("opts", OPTS, ids=IDS)
def test_search_paths_match_restatement(env, mode, opts, form):
    ix = env.index(mode, congested=False)
    for congested in (True, False):
        ix.set_weights(env.wc if congested else None)
        got = ix.search_paths(env.s, env.t, tables=form, **opts)
        assert got[6]["tables"] == cpd.SEARCH_FORMS[form]
        want = env.want(congested, **opts)
        check(got, want, f"{form} {mode} {'congested' if congested else 'free-flow'}")
        off = got[0]
        if opts.get("itrs") == 0:
            assert off[-1] == 0  # no search expands: every path is empty
        else:
            assert got[1][off[0]:off[1]].tolist() == [int(env.s[0])]  # s == t
        if not congested and not opts:
            # free-flow: v* = s, a one-node prefix — the table-search walk
            assert got[6]["paths"]["prefix_nodes"] == NQ
            poff, pnodes, _, _, _, _ = ix.paths(env.s, env.t)
            np.testing.assert_array_equal(off, poff)
            np.testing.assert_array_equal(got[1], pnodes)


WIDTHS = {
    "ring2": ring2_graph,
    "lattice8": lambda: lattice_wide(64, 48, 8, seed=8),
    "lattice15": lambda: lattice_wide(64, 48, 15, seed=15),
    "irregular": irregular_graph,
}


@pytest.fixture(scope="module", params=sorted(WIDTHS))
def wenv(request):
    return request.param, make_env(WIDTHS[request.param](), 31, 0.3)


@pytest.mark.parametrize("form", ["tables", "walks"])
def test_search_paths_other_widths(wenv, form):
    """2, 8 and 16 adjacency slots per column; unreachable pairs."""
    name, e = wenv
    got = e.index().search_paths(e.s, e.t, tables=form)
    want = e.want()
    check(got, want, f"{name} {form}")
    if name == "irregular":
        off, fin = got[0], got[4]
        dead = np.nonzero(fin == 0)[0]
        assert len(dead) >= 1 and np.all(off[dead + 1] == off[dead])


@pytest.mark.parametrize("form", ["tables", "walks"])
def test_search_paths_escalation_and_resume(env, form, monkeypatch):
    """Searches that spill and resume (their parents and v* travel in the
    record), restart when the spill pool is full, or end on the workspace."""
    ix = env.index()
    want = env.want()
    got = ix.search_paths(env.s, env.t, capacity=64, capacity_max=4096, tables=form)
    assert got[6]["resumed"] > 0 and got[6]["passes"] >= 2
    check(got, want, f"{form} resumed")
    monkeypatch.setenv("CPD_SEARCH_POOL_WORDS", "60000")
    got = ix.search_paths(env.s, env.t, capacity=64, capacity_max=4096, tables=form)
    assert got[6]["restarted"] > 0 and got[6]["resumed"] > 0
    check(got, want, f"{form} restarted")
    monkeypatch.delenv("CPD_SEARCH_POOL_WORDS")
    off, nodes, cost, plen, fin, cnt, st = ix.search_paths(env.s, env.t, capacity=64,
                                                           capacity_max=256, tables=form)
    rc, rp, rf, rs, roff, rnodes = want
    big = fin == 2
    assert big.any() and int(big.sum()) == st["overflow"] and not (fin == 3).any()
    assert np.all(off[1:][big] == off[:-1][big])  # stopped on the workspace: 0 nodes
    ok = ~big
    np.testing.assert_array_equal(cost[ok], rc[ok])
    np.testing.assert_array_equal(fin[ok], rf[ok])
    np.testing.assert_array_equal(np.diff(off)[ok], np.diff(roff)[ok])
    for q in np.nonzero(ok)[0]:
        assert nodes[off[q]:off[q + 1]].tolist() == rnodes[roff[q]:roff[q + 1]].tolist(), q


@pytest.mark.parametrize("form", ["tables", "walks"])
def test_search_paths_lane_refill(env, form):
    """Fewer lanes than queries: a lane writes its prefix, then takes the next
    query into the same workspace."""
    got = env.index().search_paths(env.s, env.t, capacity=4096, workspace_frac=4e-4, tables=form)
    assert 64 <= got[6]["lanes"] < NQ
    check(got, env.want(), f"{form} refill")


def test_search_paths_pool_overflow(env):
    ix = env.index()
    want = env.want()
    with pytest.raises(cpd.CpdError) as e:
        ix.search_paths(env.s, env.t, prefix_bytes=64)
    assert e.value.code == cpd.CPD_E_OOM
    need = int(re.search(r"need (\d+) bytes", str(e.value)).group(1))
    assert need > 64 and str(need) in str(e.value)
    # the search itself is whole and fetchable, the queries still prepared
    cost, plen, fin, cnt = ix.search_fetch()
    np.testing.assert_array_equal(cost, want[0])
    np.testing.assert_array_equal(plen, want[1])
    np.testing.assert_array_equal(fin, want[2])
    np.testing.assert_array_equal(cnt.astype(np.uint64), want[3])
    with pytest.raises(cpd.CpdError):  # ... but there are no paths to fetch
        ix.paths_fetch(0, 1)
    c2, p2, f2, n2, _ = ix.search(env.s, env.t)
    np.testing.assert_array_equal(c2, want[0])
    got = ix.search_paths(env.s, env.t, prefix_bytes=need)
    check(got, want, "retry")
    assert got[6]["paths"]["prefix_nodes"] * 4 == need == got[6]["paths"]["prefix_bytes"]


def test_search_paths_fetch_ranges(env):
    ix = env.index()
    rc, rp, rf, rs, roff, rnodes = env.want()
    ix.prepare(env.s, env.t)
    off, st = ix.search_paths_run()
    np.testing.assert_array_equal(off, roff)
    for first, count in ((0, 1), (NQ // 2, 37), (NQ - 1, 1), (5, 0), (NQ, 0), (0, NQ)):
        got = ix.paths_fetch(first, count)
        np.testing.assert_array_equal(got, rnodes[int(roff[first]):int(roff[first + count])])
    # a following table-search paths call: the fetch returns its walks again
    poff, pnodes, _, _, _, _ = ix.paths(env.s, env.t)
    np.testing.assert_array_equal(ix.paths_fetch(0, NQ), pnodes)
    assert not np.array_equal(poff, roff)


@pytest.mark.parametrize("form", ["tables", "walks"])
def test_search_paths_reopened_chain(form):
    """hscale > 1 and an expansion limit that ends the search between the
    re-opening of the incumbent's node and its second expansion: the path is
    the chain read at the end, one move longer and 1 cheaper than the
    reported plen and cost, which stay the oracle's."""
    g, wc, s, t = reopened_graph()
    plan = cpd.Plan(g)
    dev = cpd.Graph(plan, batch=1024)
    targets = np.array([6], np.uint32)
    off, runs = oracle.build_rows(g.row_ptr, g.dst, g.w, plan.order(), targets)
    ref = SearchPathsRef(g, plan.order(), targets, off, runs)
    ix = cpd.Index.streamed(dev, targets, int(off[-1]), mode="dense")
    ix.append(off, runs)
    ix.set_weights(wc)
    for opts in (dict(hscale=1.5, itrs=3), dict(hscale=1.5)):
        rc, rp, rf, rs = oracle.cpd_search(g.row_ptr, g.dst, g.w, wc, plan.order(), targets, off,
                                           runs, s, t, **opts)
        c, p, f, st, paths, pcost = ref_search_paths(ref, wc, s, t, **opts)
        np.testing.assert_array_equal(c, rc)
        got = ix.search_paths(s, t, tables=form, **opts)
        check(got, (rc, rp, rf, rs) + flatten(paths), f"{form} {opts}")
    assert got[1][:5].tolist() == [0, 3, 2, 4, 6]


def test_search_paths_leave_no_scratch(env):
    """The prefix pool and the per-query records are scratch of one call:
    after it, and after the CPD_E_OOM return, the index holds no more HBM
    than a plain search leaves it with (plus the path nodes), so later
    searches are sized from the same memory."""
    ix = env.index()
    ix.search(env.s, env.t, capacity=1024)
    free0, _ = cpd.device_mem_info(0)
    pool = 1 << 30
    got = ix.search_paths(env.s, env.t, capacity=1024, prefix_bytes=pool)
    free1, _ = cpd.device_mem_info(0)
    # what may stay: the nodes (4 B each) and allocator rounding, far below the pool
    assert free0 - free1 < pool // 4 and 4 * int(got[0][-1]) < pool // 8
    with pytest.raises(cpd.CpdError):
        ix.search_paths(env.s, env.t, capacity=1024, prefix_bytes=64)
    free2, _ = cpd.device_mem_info(0)
    assert free0 - free2 < pool // 4
    st_a = ix.search(env.s, env.t)[4]
    st_b = env.index().search(env.s, env.t)[4]  # an index that never ran search_paths
    assert (st_a["lanes"], st_a["capacity"], st_a["passes"]) == \
           (st_b["lanes"], st_b["capacity"], st_b["passes"])
