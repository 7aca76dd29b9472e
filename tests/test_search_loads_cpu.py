"""Search loads without a GPU: the reference the GPU tests compare against
(tests/search_loads_ref.py ref_search_loads) pinned to ref_search_paths — cost,
plen, finished, counters and paths identical — its loads checked against the
definition (cpd_api.h at cpd_query_search_loads): the loaded edges cost what
the routes cost and number what the paths' moves number; the hand-made
parallel_flip_graph shown to exercise the three parallel-edge cases from the
reference alone; and the new entry point visible through ctypes."""
import ctypes as C

import numpy as np
import pytest

import cpd
import oracle
from graphs import irregular_graph, ring2_graph
from search_loads_ref import (PARALLEL_FLIP_EDGES, PARALLEL_FLIP_OPTS, parallel_flip_graph,
                              ref_search_loads, skip2_graph)
from search_paths_ref import SearchPathsRef, ref_search_paths

OPTS = [dict(), dict(hscale=1.5), dict(fscale=0.25), dict(hscale=0.5, fscale=0.1),
        dict(k_moves=40), dict(itrs=7), dict(k_moves=0, itrs=200), dict(itrs=0)]
IDS = [",".join(f"{k}={v}" for k, v in o.items()) or "default" for o in OPTS]
NQ = 3000
# the share of edges congested in the synth environment: the value of
# test_gpu_search_paths.py; test_congested_routes_have_prefix_moves shows it
# gives the reference well over NQ / 10 prefix moves, so it was not raised
FRAC = 0.2


class Env:
    pass


def make_env(g, seed, frac, nq=NQ, ntargets=60):
    e = Env()
    e.g = g
    e.order = cpd.Plan(g, hierarchy=False).order()
    rng = np.random.default_rng(seed)
    e.targets = rng.choice(g.n, size=ntargets, replace=False).astype(np.uint32)
    e.off, e.runs = oracle.build_rows(g.row_ptr, g.dst, g.w, e.order, e.targets)
    e.s = rng.integers(0, g.n, nq).astype(np.uint32)
    e.t = e.targets[rng.integers(0, len(e.targets), nq)]
    e.s[0] = e.t[0]  # s == t
    e.wc = cpd.synth_congestion(g.w, frac=frac, lo=1.0, hi=3.0, seed=4)
    e.demand = rng.integers(0, 1 << 32, nq, dtype=np.uint64).astype(np.uint32)
    e.ref = SearchPathsRef(g, e.order, e.targets, e.off, e.runs)
    return e


@pytest.fixture(scope="module")
def env():
    """The environment of test_gpu_search_paths.py."""
    return make_env(cpd.synth_road_graph(64, 48, seed=31), 31, FRAC)


def flip_env():
    g, wc, s, t, targets = parallel_flip_graph()
    e = Env()
    e.g, e.wc, e.s, e.t, e.targets = g, wc, s, t, targets
    e.order = cpd.Plan(g, hierarchy=False).order()
    e.off, e.runs = oracle.build_rows(g.row_ptr, g.dst, g.w, e.order, targets)
    e.demand = np.arange(1, len(s) + 1, dtype=np.uint32)
    e.ref = SearchPathsRef(g, e.order, targets, e.off, e.runs)
    return e


def check_against_paths(e, w_sel, opts):
    """ref_search_loads == ref_search_paths, and the loads are the routes'."""
    want = ref_search_paths(e.ref, w_sel, e.s, e.t, **opts)
    got = ref_search_loads(e.ref, w_sel, e.s, e.t, e.demand, **opts)
    for a, b in zip(got[:4], want[:4]):
        np.testing.assert_array_equal(a, b)
    assert got[4] == want[4] and got[5] == want[5]
    cost, plen, fin, stats, paths, pcost, loads, moves, prefix_moves = got
    dem = e.demand.astype(np.uint64).tolist()
    w = np.asarray(w_sel).astype(np.uint64).tolist()
    assert loads.dtype == np.uint64 and loads.shape == (e.g.m,)
    # exact in Python integers: no wrap of the sums themselves
    assert sum(int(l) * w[i] for i, l in enumerate(loads.tolist())) == \
        sum(d * int(c) for d, c in zip(dem, pcost))
    assert int(sum(loads.tolist())) == sum(dem[q] * (len(p) - 1) for q, p in enumerate(paths) if p)
    assert moves == sum(len(p) - 1 for p in paths if p) and 0 <= prefix_moves <= moves
    if not opts:  # demand None = 1 each: the table sums to the moves
        ones = ref_search_loads(e.ref, w_sel, e.s, e.t, None)
        assert int(ones[6].sum()) == moves == ones[7] and ones[8] == prefix_moves
    return got


@pytest.mark.parametrize("congested", [True, False], ids=["congested", "free-flow"])
@pytest.mark.parametrize("opts", OPTS, ids=IDS)
def test_reference_matches_paths_and_definition(env, opts, congested):
    got = check_against_paths(env, env.wc if congested else env.g.w, opts)
    if opts.get("itrs") == 0:
        assert not got[6].any() and got[7] == 0
    if not congested and not opts:
        # free flow: v* = s, the route is the table-search walk
        assert got[8] == 0


def test_congested_routes_have_prefix_moves(env):
    """What keeps the GPU test from passing on suffix-only routes."""
    got = ref_search_loads(env.ref, env.wc, env.s, env.t)
    print(f"synth_congestion(frac={FRAC}): prefix_moves {got[8]} of {got[7]} moves, {NQ} queries")
    assert got[8] >= NQ // 10


@pytest.mark.parametrize("congested", [True, False], ids=["congested", "free-flow"])
def test_reference_on_irregular_graph(congested):
    """Unreachable pairs, a self loop, parallel and 0-weight edges."""
    e = make_env(irregular_graph(), 31, 0.3)
    got = check_against_paths(e, e.wc if congested else e.g.w, {})
    assert (got[2] == 0).any()


def test_two_slot_graph_has_prefix_moves():
    """skip2_graph is what sends the prefix kernel over 2-slot rows: out-degree
    <= 2 and routes that leave the CPD path (ring2_graph has none)."""
    g = skip2_graph()
    assert int(np.diff(g.row_ptr.astype(np.int64)).max()) == 2
    e = make_env(g, 31, 0.3)
    got = check_against_paths(e, e.wc, {})
    assert got[8] >= NQ // 10
    r = make_env(ring2_graph(), 31, 0.3)
    assert ref_search_loads(r.ref, r.wc, r.s, r.t)[8] == 0


def test_parallel_flip_graph_exercises_the_three_cases():
    """(a), (b), (c) of search_loads_ref.parallel_flip_graph, from the
    reference alone: the graph cannot quietly stop exercising them."""
    e = flip_env()
    g, wc = e.g, e.wc
    assert g.n < 12 and np.all(wc >= g.w)
    tail = np.repeat(np.arange(g.n), np.diff(g.row_ptr.astype(np.int64)))
    assert [(int(a), int(b), int(f), int(c)) for a, b, f, c in zip(tail, g.dst, g.w, wc)] == \
        PARALLEL_FLIP_EDGES
    one = lambda q: (e.s[q:q + 1], e.t[q:q + 1])  # noqa: E731
    full = ref_search_loads(e.ref, wc, *one(0))
    early = ref_search_loads(e.ref, wc, *one(0), fscale=0.25)
    free = ref_search_loads(e.ref, g.w, *one(0))
    assert (full[0][0], early[0][0], free[0][0]) == (21, 25, 15)
    assert full[4][0] == early[4][0] == free[4][0] == [0, 1, 2, 4, 5, 8]  # one node route
    assert np.nonzero(free[6])[0].tolist() == [0, 3, 7, 9, 11] and free[8] == 0
    assert np.nonzero(full[6])[0].tolist() == [1, 4, 7, 10, 11] and (full[7], full[8]) == (5, 4)
    assert np.nonzero(early[6])[0].tolist() == [1, 4, 7, 9, 11] and (early[7], early[8]) == (5, 2)
    # (a) prefix move 0 -> 1: edges 0 and 1 are parallel, the cheaper flips
    assert (tail[0], g.dst[0]) == (tail[1], g.dst[1]) == (0, 1)
    assert g.w[0] < g.w[1] and wc[1] < wc[0] and full[6][1] == 1 and full[6][0] == 0
    # (b) prefix move 1 -> 2: edges 4 and 5 are parallel and equal, the first is taken
    assert (tail[4], g.dst[4]) == (tail[5], g.dst[5]) == (1, 2)
    assert wc[4] == wc[5] < wc[3] and full[6][4] == 1 and full[6][5] == 0
    # (c) suffix move 4 -> 5: the row names edge 9, the dearer of 9 and 10
    assert (tail[9], g.dst[9]) == (tail[10], g.dst[10]) == (4, 5)
    assert int(e.ref.move_edges(8)[4]) == 9 and wc[9] > wc[10]
    assert early[6][9] == 1 and early[6][10] == 0
    for opts in PARALLEL_FLIP_OPTS:
        for w in (wc, g.w):
            check_against_paths(e, w, opts)


def test_entry_point_visible_and_checks_arguments():
    """cpd_query_search_loads: exported, mirrored, its info struct of the
    header's size, and a null index is CPD_E_ARG (no device needed)."""
    assert "cpd_query_search_loads" in cpd.EXPORTED
    so = C.CDLL(cpd.LIB_PATH)
    fn = so.cpd_query_search_loads
    fn.restype = C.c_int
    assert C.sizeof(cpd.SearchLoadsInfo) == 40
    assert [k for k, _ in cpd.SearchLoadsInfo._fields_] == ["moves", "prefix_moves", "prefix_nodes",
                                                            "prefix_bytes", "loads_ms"]
    info = cpd.SearchLoadsInfo()
    rc = fn(None, None, C.c_uint64(0), None, C.c_uint32(0), None, C.byref(info))
    assert rc == cpd.CPD_E_ARG
    assert "null" in cpd.lib.cpd_last_error().decode()
    assert callable(cpd.Index.search_loads) and callable(cpd.Index.search_loads_run)
