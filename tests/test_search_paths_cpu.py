"""Search paths without a GPU: the Python restatement the GPU tests compare
against (tests/search_paths_ref.py ref_search_paths) pinned to the oracle —
cost, plen, finished and the five counters equal — its paths checked against
the definition (cpd_api.h at cpd_query_search_paths), and the new entry point
visible through ctypes."""
import ctypes as C

import numpy as np
import pytest

import cpd
import oracle
from search_paths_ref import SearchPathsRef, ref_search_paths, reopened_graph

OPTS = [dict(), dict(hscale=1.5), dict(fscale=0.25), dict(hscale=0.5, fscale=0.1),
        dict(k_moves=40), dict(itrs=7), dict(k_moves=0, itrs=200), dict(itrs=0)]
IDS = [",".join(f"{k}={v}" for k, v in o.items()) or "default" for o in OPTS]
NQ = 400


class Env:
    pass


@pytest.fixture(scope="module")
def env():
    """The graph of test_gpu_search.py: 64 x 48 synth, seed 31, 60 targets."""
    e = Env()
    g = e.g = cpd.synth_road_graph(64, 48, seed=31)
    e.order = cpd.Plan(g, hierarchy=False).order()
    rng = np.random.default_rng(31)
    e.targets = rng.choice(g.n, size=60, replace=False).astype(np.uint32)
    e.off, e.runs = oracle.build_rows(g.row_ptr, g.dst, g.w, e.order, e.targets)
    e.s = rng.integers(0, g.n, NQ).astype(np.uint32)
    e.t = e.targets[rng.integers(0, len(e.targets), NQ)]
    e.s[0] = e.t[0]  # s == t
    e.wc = cpd.synth_congestion(g.w, frac=0.2, lo=1.0, hi=3.0, seed=4)
    e.ref = SearchPathsRef(g, e.order, e.targets, e.off, e.runs)
    e.edges = {}
    for w in (g.w, e.wc):
        src = np.repeat(np.arange(g.n), np.diff(g.row_ptr.astype(np.int64)))
        d = {}
        for a, b, c in zip(src.tolist(), g.dst.tolist(), w.tolist()):
            d[(a, b)] = min(c, d.get((a, b), c))  # the cheapest of parallel edges
        e.edges[id(w)] = d
    return e


@pytest.mark.parametrize("congested", [True, False], ids=["congested", "free-flow"])
@pytest.mark.parametrize("opts", OPTS, ids=IDS)
def test_restatement_matches_oracle_and_definition(env, opts, congested):
    g = env.g
    w_sel = env.wc if congested else g.w
    rc, rp, rf, rs = oracle.cpd_search(g.row_ptr, g.dst, g.w, w_sel, env.order, env.targets,
                                       env.off, env.runs, env.s, env.t, **opts)
    cost, plen, fin, stats, paths, pcost = ref_search_paths(env.ref, w_sel, env.s, env.t, **opts)
    np.testing.assert_array_equal(cost, rc)
    np.testing.assert_array_equal(plen, rp)
    np.testing.assert_array_equal(fin, rf)
    np.testing.assert_array_equal(stats, rs)
    edges = env.edges[id(w_sel)]
    consistent = opts.get("hscale", 1.0) <= 1.0  # and w_sel >= g.w, both weight sets
    assert np.all(w_sel >= g.w)
    for q, p in enumerate(paths):
        if not rf[q]:
            assert p == [] and pcost[q] == 0
            continue
        assert p[0] == env.s[q] and p[-1] == env.t[q]
        assert all((a, b) in edges for a, b in zip(p, p[1:])), q
        # no route is cheaper than the cheapest parallel edges under its hops
        assert sum(edges[(a, b)] for a, b in zip(p, p[1:])) <= pcost[q] <= rc[q]
        if consistent:
            assert pcost[q] == rc[q] and len(p) - 1 == rp[q]
    if opts.get("itrs") == 0:
        assert not rf.any() and all(p == [] for p in paths)
    else:
        assert paths[0] == [int(env.s[0])] and rc[0] == 0 and rp[0] == 0  # s == t
    if not congested and "k_moves" not in opts and rf.all():
        # free-flow: v* = s, the path is the table-search walk
        tc, th, tf = oracle.table_search(g.row_ptr, g.dst, g.w, env.order, env.targets, env.off,
                                         env.runs, env.s, env.t)
        assert all(len(p) - 1 == h for p, h in zip(paths, th))


def test_hscale_above_one_has_a_path_that_differs(env):
    """The inequality branch of the definition is exercised: a query whose
    path undercuts `cost` and differs from `plen`, because a chain node's g
    improved after the incumbent was set.
    hscale = 1.5 alone does not reach it.  A path differs only if a chain
    node, re-opened with a smaller g, still waits in the heap when the search
    ends; a search that runs until its stop rule ends it was never seen to
    leave one (tools_scripts/search_paths_reopen_scan.py: 0 of 640,000
    searches on 400 random 40-node graphs, and 0 on this file's graph), and
    the expansion limit can cut a search off in between.  So the check is
    made on hscale = 1.5 with itrs = 3, on search_paths_ref.reopened_graph,
    whose docstring lists the three pops; the hscale = 1.5 set above still
    asserts path cost <= the oracle's cost per query."""
    g, wc, s, t = reopened_graph()
    order = cpd.Plan(g, hierarchy=False).order()
    targets = np.array([6], np.uint32)
    off, runs = oracle.build_rows(g.row_ptr, g.dst, g.w, order, targets)
    ref = SearchPathsRef(g, order, targets, off, runs)
    opts = dict(hscale=1.5, itrs=3)
    rc, rp, rf, rs = oracle.cpd_search(g.row_ptr, g.dst, g.w, wc, order, targets, off, runs, s, t,
                                       **opts)
    cost, plen, fin, stats, paths, pcost = ref_search_paths(ref, wc, s, t, **opts)
    np.testing.assert_array_equal(cost, rc)
    np.testing.assert_array_equal(plen, rp)
    np.testing.assert_array_equal(fin, rf)
    np.testing.assert_array_equal(stats, rs)
    differs = sum(1 for q, p in enumerate(paths)
                  if rf[q] and (pcost[q] < rc[q] or len(p) - 1 != rp[q]))
    print("hscale=1.5, itrs=3: paths that differ from plen or undercut cost:", differs)
    assert differs > 0
    assert paths[0] == [0, 3, 2, 4, 6] and (rc[0], rp[0], pcost[0]) == (40, 3, 39)
    assert all(pc <= c for pc, c in zip(pcost, rc))
    # the same search left to run re-expands node 2 and agrees with its path
    c2, p2, _, _, paths2, pcost2 = ref_search_paths(ref, wc, s, t, hscale=1.5)
    assert paths2[0] == paths[0] and (c2[0], p2[0], pcost2[0]) == (39, 4, 39)


def test_entry_point_visible_and_checks_arguments():
    """cpd_query_search_paths: exported, mirrored, its info struct of the
    header's size, and a null index is CPD_E_ARG (no device needed)."""
    assert "cpd_query_search_paths" in cpd.EXPORTED
    so = C.CDLL(cpd.LIB_PATH)
    fn = so.cpd_query_search_paths
    fn.restype = C.c_int
    assert C.sizeof(cpd.SearchPathsInfo) == 32
    assert [k for k, _ in cpd.SearchPathsInfo._fields_] == ["nodes", "prefix_nodes",
                                                            "prefix_bytes", "paths_ms"]
    off = (C.c_uint64 * 1)()
    info = cpd.SearchPathsInfo()
    rc = fn(None, None, C.c_uint64(0), off, None, C.byref(info))
    assert rc == cpd.CPD_E_ARG
    assert "null" in cpd.lib.cpd_last_error().decode()
    assert callable(cpd.Index.search_paths) and callable(cpd.Index.search_paths_run)
