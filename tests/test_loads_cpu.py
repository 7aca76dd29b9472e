"""Edge loads, without a GPU: the interface is there — the header declares it,
libcpd.so exports it, cpd.Index mirrors it, NULL arguments are refused — and
the reference of tests/loads_ref.py is pinned against the oracle independently
of its own walk: its move table is oracle.get_move's, the loads weighted by any
w sum to the oracle's demand-weighted costs under w, their total to the
demand-weighted hops, the planes of a sliced table to the unsliced one, and on
a one-way ring the loads have a closed form."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import cpd
import loads_ref as L
import oracle
from graphs import GRAPHS, graph_from_edges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cpd_query_loads", "cpd_query_loads_fetch", "cpd_query_loads_clear")


def test_header_declares_loads_entry_points():
    hdr = open(os.path.join(ROOT, "include", "cpd_api.h")).read()
    declared = set(re.findall(r"\b(cpd_[a-z_]+)\s*\(", hdr))
    assert set(NAMES) <= declared
    assert re.search(r"#define\s+CPD_MAX_LOAD_SLICES\s+8u", hdr)
    assert re.search(r"#define\s+CPD_LOADS_ACCUMULATE\s+1u", hdr)


def test_python_mirror_has_loads():
    for attr in ("loads", "loads_run", "loads_fetch", "loads_clear"):
        assert callable(getattr(cpd.Index, attr))
    for name in NAMES:
        assert name in cpd.EXPORTED and hasattr(cpd.lib, name)
    assert cpd.MAX_LOAD_SLICES == 8 and cpd.LOADS_ACCUMULATE == 1


def test_library_exports_loads_symbols():
    so = C.CDLL(cpd.LIB_PATH)  # dlsym on the shared library itself
    for name in NAMES:
        assert getattr(so, name, None) is not None, name


def test_null_index_is_refused():
    st = cpd.QueryStats()
    assert cpd.lib.cpd_query_loads(None, C.c_int32(-1), None, C.c_uint32(1), C.c_uint32(0),
                                   C.c_uint32(0), C.byref(st)) == cpd.CPD_E_ARG
    assert cpd.lib.cpd_query_loads(None, C.c_int32(-1), None, C.c_uint32(1), C.c_uint32(0),
                                   C.c_uint32(0), None) == cpd.CPD_E_ARG
    out = np.zeros(4, np.uint64)
    assert cpd.lib.cpd_query_loads_fetch(None, cpd._ptr(out, cpd.u64p)) == cpd.CPD_E_ARG
    assert cpd.lib.cpd_query_loads_fetch(None, None) == cpd.CPD_E_ARG
    assert cpd.lib.cpd_query_loads_clear(None) == cpd.CPD_E_ARG
    assert cpd.lib.cpd_last_error()


@functools.lru_cache(maxsize=None)
def world(name):
    g = GRAPHS[name]()
    order = oracle.dfs_preorder(g.row_ptr, g.dst)
    rng = np.random.default_rng(2)
    targets = rng.choice(g.n, size=30, replace=False).astype(np.uint32)
    off, runs = oracle.build_rows(g.row_ptr, g.dst, g.w, order, targets)
    s = rng.integers(0, g.n, 600).astype(np.uint32)
    t = targets[rng.integers(0, len(targets), 600)]
    demand = rng.integers(0, 1 << 32, 600, dtype=np.uint64).astype(np.uint32)
    return g, order, targets, off, runs, s, t, demand


def exact_sum(a):
    return int(np.asarray(a).astype(object).sum())


@pytest.mark.parametrize("graph", ["synth", "irregular", "deg8"])
def test_move_table_is_get_move(graph):
    g, order, targets, off, runs, s, t, demand = world(graph)
    table = L.move_table(off, runs, g.n)
    assert table.shape == (len(targets), g.n)
    rng = np.random.default_rng(4)
    for r in range(len(targets)):
        rr = runs[int(off[r]):int(off[r + 1])]
        for c in rng.integers(0, g.n, 40):
            assert table[r, c] == oracle.get_move(rr, int(c))


@pytest.mark.parametrize("graph", ["synth", "irregular", "deg8"])
def test_reference_is_pinned_by_the_oracle(graph):
    g, order, targets, off, runs, s, t, demand = world(graph)
    rng = np.random.default_rng(6)
    ws = [rng.integers(0, 1 << 20, g.m).astype(np.uint32) for _ in range(3)]
    d64 = demand.astype(object)
    for k in (-1, 0, 1, 10):
        loads, hops, fin = L.walk_loads(g, order, targets, off, runs, s, t, demand, k_moves=k)
        assert loads.shape == (1, g.m) and loads.dtype == np.uint64
        for w in ws:
            rc, rh, rf = oracle.table_search(g.row_ptr, g.dst, w, order, targets, off, runs, s, t,
                                             k_moves=k)
            np.testing.assert_array_equal(hops, rh)
            np.testing.assert_array_equal(fin, rf)
            # sum_e loads[e] w[e] == sum_q demand[q] cost_q under w
            assert exact_sum(loads[0].astype(object) * w.astype(object)) == \
                   exact_sum(d64 * rc.astype(object))
        assert exact_sum(loads) == exact_sum(d64 * hops.astype(object))
    if graph == "irregular":  # the unfinished walks are there
        assert 0 < int(fin.sum()) < len(s)
    # demand=None is a demand of 1
    ones, h1, _ = L.walk_loads(g, order, targets, off, runs, s, t)
    np.testing.assert_array_equal(
        ones, L.walk_loads(g, order, targets, off, runs, s, t, np.ones(len(s), np.uint32))[0])
    assert exact_sum(ones) == int(h1.astype(np.int64).sum())


@pytest.mark.parametrize("graph", ["synth", "irregular", "deg8"])
def test_sliced_planes(graph):
    g, order, targets, off, runs, s, t, demand = world(graph)
    for k in (-1, 10):
        full, hops, fin = L.walk_loads(g, order, targets, off, runs, s, t, demand, k_moves=k)
        longest = int(hops.max())
        for K in (2, 5, 8):
            for S in (1, 3, 7, g.n):
                pl, h2, f2 = L.walk_loads(g, order, targets, off, runs, s, t, demand, K=K, S=S,
                                          k_moves=k)
                assert pl.shape == (K, g.m)
                np.testing.assert_array_equal(h2, hops)
                np.testing.assert_array_equal(f2, fin)
                # the planes sum to the unsliced table
                np.testing.assert_array_equal(pl.sum(axis=0, dtype=np.uint64), full[0])
                for j in range(K):
                    # plane j (j < K - 1) holds moves j S .. (j + 1) S - 1, the last the rest:
                    # the demand-weighted count of those moves, and nothing where no walk
                    # reaches move j S
                    lo = j * S
                    moves = np.maximum(hops.astype(np.int64) - lo, 0)
                    if j < K - 1:
                        moves = np.minimum(moves, S)
                    assert exact_sum(pl[j]) == exact_sum(demand.astype(object) * moves.astype(object))
                    if longest <= lo:
                        assert not pl[j].any()
                if S >= longest:
                    np.testing.assert_array_equal(pl[0], full[0])


def test_one_way_ring_closed_form():
    n = 257
    g = graph_from_edges(n, [(a, (a + 1) % n, 1 + a % 3) for a in range(n)])
    order = oracle.dfs_preorder(g.row_ptr, g.dst)
    rng = np.random.default_rng(9)
    targets = rng.choice(n, size=20, replace=False).astype(np.uint32)
    off, runs = oracle.build_rows(g.row_ptr, g.dst, g.w, order, targets)
    s = rng.integers(0, n, 500).astype(np.uint32)
    t = targets[rng.integers(0, len(targets), 500)]
    demand = rng.integers(0, 1 << 32, 500, dtype=np.uint64).astype(np.uint32)
    # edge i is i -> i + 1: it carries query q iff i lies on the arc s .. t - 1
    i = np.arange(n, dtype=np.int64)[None, :]
    on = ((i - s.astype(np.int64)[:, None]) % n) < ((t.astype(np.int64) - s.astype(np.int64)) % n)[:, None]
    loads, hops, fin = L.walk_loads(g, order, targets, off, runs, s, t)
    assert fin.all()
    np.testing.assert_array_equal(loads[0], on.sum(axis=0).astype(np.uint64))
    loads, _, _ = L.walk_loads(g, order, targets, off, runs, s, t, demand)
    want = (on.astype(np.uint64) * demand.astype(np.uint64)[:, None]).sum(axis=0, dtype=np.uint64)
    np.testing.assert_array_equal(loads[0], want)
    assert int(loads[0].max()) > 1 << 32
