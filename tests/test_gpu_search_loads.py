"""GPU: search loads (cpd_query_search_loads / Index.search_loads) against the
Python reference ref_search_loads (tests/search_loads_ref.py, pinned by
test_search_loads_cpu.py), counter for counter: the demand of every routed
query on each edge of the route search_paths() returns — on the A* tree's
chain the edge whose relaxation set g, on the CPD walk the edge the row's move
names.  cost / plen / finished and the counters stay cpd_query_search's.  Every
value is compared exactly."""
import ctypes as C
import re

import numpy as np
import pytest

import cpd
import loads_ref as L
import oracle
from graphs import irregular_graph, lattice_wide, ring2_graph
from search_loads_ref import (PARALLEL_FLIP_OPTS, parallel_flip_graph, ref_search_loads,
                              skip2_graph)
from search_paths_ref import SearchPathsRef

pytestmark = pytest.mark.gpu

OPTS = [dict(), dict(hscale=1.5), dict(fscale=0.25), dict(hscale=0.5, fscale=0.1),
        dict(k_moves=40), dict(itrs=7), dict(k_moves=0, itrs=200), dict(itrs=0)]
IDS = [",".join(f"{k}={v}" for k, v in o.items()) or "default" for o in OPTS]
NQ = 3000
FRAC = 0.2  # test_search_loads_cpu.py: the reference has >= NQ / 10 prefix moves at it


class Env:
    def want(self, congested=True, demand=False, **opts):
        """ref_search_loads of the env's queries (demand: the env's random one,
        else 1 each), computed once per option set: (cost, plen, fin, stats,
        loads, moves, prefix_moves)."""
        key = (congested, demand, tuple(sorted(opts.items())))
        if key not in self.cache:
            w = self.wc if congested else self.g.w
            r = ref_search_loads(self.ref, w, self.s, self.t, self.demand if demand else None,
                                 **opts)
            self.cache[key] = r[:4] + r[6:]
        return self.cache[key]

    def index(self, mode="dense", congested=True):
        ix = cpd.Index.streamed(self.dev, self.targets, int(self.off[-1]), mode=mode)
        ix.append(self.off, self.runs)
        if congested:
            ix.set_weights(self.wc)
        return ix


def make_env(g, seed, frac, flip=None):
    e = Env()
    e.g = g
    e.plan = cpd.Plan(g)
    e.order = e.plan.order()
    e.dev = cpd.Graph(e.plan, batch=1024)
    rng = np.random.default_rng(seed)
    if flip is None:
        e.targets = rng.choice(g.n, size=60, replace=False).astype(np.uint32)
        e.s = rng.integers(0, g.n, NQ).astype(np.uint32)
        e.t = e.targets[rng.integers(0, len(e.targets), NQ)]
        e.s[0] = e.t[0]  # a query with s == t
        e.wc = cpd.synth_congestion(g.w, frac=frac, lo=1.0, hi=3.0, seed=4)
    else:
        e.wc, e.s, e.t, e.targets = flip
    e.off, e.runs = oracle.build_rows(g.row_ptr, g.dst, g.w, e.order, e.targets)
    e.demand = rng.integers(0, 1 << 32, len(e.s), dtype=np.uint64).astype(np.uint32)
    e.ref = SearchPathsRef(g, e.order, e.targets, e.off, e.runs)
    e.cache = {}
    return e


@pytest.fixture(scope="module")
def env():
    """The graph, targets, queries and congestion of test_gpu_search_paths.py."""
    return make_env(cpd.synth_road_graph(64, 48, seed=31), 31, FRAC)


def check(got, want, msg=""):
    """Loads, results, counters and the move counts exact; the sums as the search's."""
    loads, cost, plen, fin, cnt, st = got
    rc, rp, rf, rs, rloads, rmoves, rprefix = want
    assert loads.dtype == np.uint64 and loads.shape == (1, len(rloads))
    np.testing.assert_array_equal(cost, rc, err_msg=f"{msg} cost")
    np.testing.assert_array_equal(plen, rp, err_msg=f"{msg} plen")
    np.testing.assert_array_equal(fin, rf, err_msg=f"{msg} finished")
    np.testing.assert_array_equal(cnt.astype(np.uint64), rs, err_msg=f"{msg} counters")
    np.testing.assert_array_equal(loads[0], rloads, err_msg=f"{msg} loads")
    assert st["overflow"] == 0 and st["expanded"] == int(rs[:, 0].sum()), msg
    assert st["finished"] == int(rf.sum()) and st["plen"] == int(rp[rf == 1].sum()), msg
    info = st["loads"]
    assert (info["moves"], info["prefix_moves"]) == (rmoves, rprefix), msg
    assert info["prefix_nodes"] == rprefix + int(rf.sum()), msg  # a prefix is s ... v*
    assert info["prefix_bytes"] >= 4 * info["prefix_nodes"] and info["loads_ms"] >= 0, msg


@pytest.mark.parametrize("form", ["tables", "walks"])
@pytest.mark.parametrize("mode", ["dense", "rle"])
@pytest.mark.parametrize("opts", OPTS, ids=IDS)
def test_search_loads_match_reference(env, mode, opts, form):
    ix = env.index(mode, congested=False)
    for congested in (True, False):
        msg = f"{form} {mode} {'congested' if congested else 'free-flow'}"
        ix.set_weights(env.wc if congested else None)
        got = ix.search_loads(env.s, env.t, tables=form, **opts)
        assert got[5]["tables"] == cpd.SEARCH_FORMS[form]
        want = env.want(congested, **opts)
        check(got, want, msg)
        # ... and what Index.search gives on the same queries
        c, p, f, n, _ = ix.search(env.s, env.t, tables=form, **opts)
        for a, b in zip(got[1:5], (c, p, f, n)):
            np.testing.assert_array_equal(a, b, err_msg=msg)
        np.testing.assert_array_equal(ix.loads_fetch(), got[0])  # a search leaves the table
        if opts.get("itrs") == 0:
            assert not got[0].any() and got[5]["loads"]["moves"] == 0  # no search expands
        if congested and not opts:
            assert want[6] >= NQ // 10  # real A* prefixes, not suffix-only routes
        if not congested and not opts:
            # free flow: v* = s, the route is the table-search walk
            assert got[5]["loads"]["prefix_moves"] == 0
            walk, _ = ix.loads(env.s, env.t)
            np.testing.assert_array_equal(got[0], walk)


WIDTHS = {
    "ring2": ring2_graph,
    "skip2": skip2_graph,
    "lattice8": lambda: lattice_wide(64, 48, 8, seed=8),
    "lattice15": lambda: lattice_wide(64, 48, 15, seed=15),
    "irregular": irregular_graph,
}


@pytest.fixture(scope="module", params=sorted(WIDTHS))
def wenv(request):
    return request.param, make_env(WIDTHS[request.param](), 31, 0.3)


@pytest.mark.parametrize("form", ["tables", "walks"])
def test_search_loads_other_widths(wenv, form):
    """2, 8 and 16 adjacency slots per column (the prefix kernel's row reads);
    unreachable pairs, a self loop, parallel and 0-weight edges.  ring2 has no
    alternative routes (search_loads_ref.skip2_graph): its 2-slot rows are
    read by the suffix walk alone, skip2's by the prefix kernel."""
    name, e = wenv
    want = e.want(demand=True)
    got = e.index().search_loads(e.s, e.t, e.demand, tables=form)
    check(got, want, f"{name} {form}")
    assert (want[6] > 0) == (name != "ring2")  # prefix moves at this width
    if name == "irregular":
        assert (got[3] == 0).any()


@pytest.mark.parametrize("form", ["tables", "walks"])
def test_search_loads_parallel_edges(form):
    """parallel_flip_graph: the cheaper of two parallel edges flips under
    congestion, two tie, and the CPD walk takes the dearer of two."""
    g, wc, s, t, targets = parallel_flip_graph()
    e = make_env(g, 31, 0.0, flip=(wc, s, t, targets))
    ix = e.index(congested=False)
    for opts in PARALLEL_FLIP_OPTS:
        for congested in (True, False):
            ix.set_weights(wc if congested else None)
            got = ix.search_loads(s, t, e.demand, tables=form, **opts)
            check(got, e.want(congested, demand=True, **opts), f"{form} {opts} {congested}")
    ix.set_weights(wc)
    one = ix.search_loads(s[:1], t[:1], tables=form, fscale=0.25)[0][0]
    assert np.nonzero(one)[0].tolist() == [1, 4, 7, 9, 11]
    one = ix.search_loads(s[:1], t[:1], tables=form)[0][0]
    assert np.nonzero(one)[0].tolist() == [1, 4, 7, 10, 11]


def test_search_loads_demand(env):
    ix = env.index()
    check(ix.search_loads(env.s, env.t, env.demand), env.want(demand=True), "random demand")
    ones = env.want()
    # 0xFFFFFFFF on every query: 64-bit counters do not wrap
    top = np.full(NQ, 0xFFFFFFFF, np.uint32)
    got = ix.search_loads(env.s, env.t, top)
    check(got, ones[:4] + (ones[4] * np.uint64(0xFFFFFFFF),) + ones[5:], "top demand")
    assert int(ones[4].max()) < 2 ** 32 and int(got[0].max()) > 2 ** 33
    # a demand of 0 loads nothing; the adds are still made and counted
    got = ix.search_loads(env.s, env.t, np.zeros(NQ, np.uint32))
    check(got, ones[:4] + (np.zeros_like(ones[4]),) + ones[5:], "zero demand")
    with pytest.raises(ValueError):
        ix.search_loads(env.s, env.t, top[:-1])


def test_search_loads_accumulate(env):
    """An all-or-nothing start (loads), then the batch as two halves of search
    iterations: the reference's sum."""
    ix = env.index()
    walk, hops, fin = L.walk_loads(env.g, env.order, env.targets, env.off, env.runs, env.s, env.t)
    want = env.want()
    start, _ = ix.loads(env.s, env.t)
    np.testing.assert_array_equal(start, walk)
    h = NQ // 2
    moves = prefix = 0
    for lo, hi in ((0, h), (h, NQ)):
        got = ix.search_loads(env.s[lo:hi], env.t[lo:hi], accumulate=True)
        for a, b in zip(got[1:4], want[:3]):
            np.testing.assert_array_equal(a, b[lo:hi])
        moves += got[5]["loads"]["moves"]
        prefix += got[5]["loads"]["prefix_moves"]
    np.testing.assert_array_equal(got[0][0], walk[0] + want[4])
    assert (moves, prefix) == (want[5], want[6])
    # accumulate with no table resident starts from zero; without it the table is made again
    ix.loads_clear()
    check(ix.search_loads(env.s, env.t, accumulate=True), want, "fresh")
    check(ix.search_loads(env.s, env.t), want, "again")


def test_search_loads_refuse_other_tables(env):
    """Onto a sliced or a timed table: CPD_E_ARG, the table unchanged."""
    ix = env.index()
    before, _ = ix.loads(env.s, env.t, slices=3, slice_moves=4)
    with pytest.raises(cpd.CpdError) as e:
        ix.search_loads(env.s, env.t, accumulate=True)
    assert e.value.code == cpd.CPD_E_ARG and "slices" in str(e.value)
    np.testing.assert_array_equal(ix.loads_fetch(), before)
    ix.set_weight_sets([None, env.wc])
    ix.timed(env.s, env.t, period=500, loads=True)
    before = ix.loads_fetch()
    assert before.shape[0] == 2 and before.any()
    with pytest.raises(cpd.CpdError) as e:
        ix.search_loads(env.s, env.t, accumulate=True)
    assert e.value.code == cpd.CPD_E_ARG and "timed" in str(e.value)
    np.testing.assert_array_equal(ix.loads_fetch(), before)
    # without accumulate the table is made again, one plane
    check(ix.search_loads(env.s, env.t), env.want(), "replaced")


def test_search_loads_pool_overflow(env):
    ix = env.index()
    want = env.want()
    before, _ = ix.loads(env.s, env.t)
    for accumulate in (False, True):
        with pytest.raises(cpd.CpdError) as e:
            ix.search_loads(env.s, env.t, accumulate=accumulate, prefix_bytes=64)
        assert e.value.code == cpd.CPD_E_OOM
        need = int(re.search(r"need (\d+) bytes", str(e.value)).group(1))
        assert need > 64 and str(need) in str(e.value)
        # the table is as it was, the search whole and fetchable, the queries still prepared
        np.testing.assert_array_equal(ix.loads_fetch(), before)
        cost, plen, fin, cnt = ix.search_fetch()
        np.testing.assert_array_equal(cost, want[0])
        np.testing.assert_array_equal(plen, want[1])
        np.testing.assert_array_equal(fin, want[2])
        np.testing.assert_array_equal(cnt.astype(np.uint64), want[3])
    got = ix.search_loads(env.s, env.t, prefix_bytes=need)
    check(got, want, "retry")
    assert got[5]["loads"]["prefix_nodes"] * 4 == need == got[5]["loads"]["prefix_bytes"]


@pytest.mark.parametrize("form", ["tables", "walks"])
def test_search_loads_escalation_and_resume(env, form):
    """Searches that spill and resume in later passes at a larger capacity:
    the prefix of each is the one of the pass it ended in."""
    got = env.index().search_loads(env.s, env.t, env.demand, capacity=64, capacity_max=4096,
                                   tables=form)
    assert got[5]["resumed"] > 0 and got[5]["passes"] >= 2
    check(got, env.want(demand=True), f"{form} resumed")


def test_search_loads_edge_cases(env):
    ix = env.index()
    m = env.g.m
    none = np.zeros(0, np.uint32)
    # the empty batch is answered: a zeroed table, info all 0 ...
    ix.prepare(none, none)
    st = ix.search_loads_run()
    assert all(v == 0 for v in st["loads"].values())
    assert ix.loads_fetch().shape == (1, m) and not ix.loads_fetch().any()
    # ... or the table kept
    want = env.want()
    check(ix.search_loads(env.s, env.t), want, "full")
    ix.prepare(none, none)
    st = ix.search_loads_run(accumulate=True)
    assert all(v == 0 for v in st["loads"].values())
    np.testing.assert_array_equal(ix.loads_fetch()[0], want[4])
    # unknown flag bits
    ix.prepare(env.s, env.t)
    for flags in (2, 4, 1 << 31):
        with pytest.raises(cpd.CpdError) as e:
            ix.search_loads_run(flags=flags)
        assert e.value.code == cpd.CPD_E_ARG and "flag" in str(e.value)
    np.testing.assert_array_equal(ix.loads_fetch()[0], want[4])
    # itrs = 0: no search expands, an all-zero table
    got = ix.search_loads(env.s, env.t, itrs=0)
    assert not got[0].any() and got[5]["loads"]["moves"] == 0 and not got[3].any()
    # like cpd_query_run, the call ends the validity of fetched paths
    ix.paths(env.s, env.t)
    ix.search_loads_run()
    with pytest.raises(cpd.CpdError):
        ix.paths_fetch(0, 1)
    node = np.zeros(4, np.uint32)  # ... in the library too, not only in the wrapper
    assert cpd.lib.cpd_query_paths_fetch(ix._h, C.c_uint32(0), C.c_uint32(1),
                                         node.ctypes.data_as(cpd.u32p)) == cpd.CPD_E_ARG
