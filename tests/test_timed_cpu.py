"""Timed walks, without a GPU: the reference of tests/timed_ref.py is pinned —
the lock-step walk against a plain per-query loop, and both against the oracle
wherever the clock cannot matter (one set, equal sets, a period beyond every
arrival, departures in the last set), the loads summed over planes against
loads_ref — a hand-worked case states its numbers, and the interface is there:
the header declares it, libcpd.so exports it, cpd.Index mirrors it."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import cpd
import loads_ref as L
import oracle
import timed_ref as T
from graphs import GRAPHS, graph_from_edges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cpd_query_timed", "cpd_query_timed_fetch")
NQ = 500


@functools.lru_cache(maxsize=None)
def world(name):
    g = GRAPHS[name]()
    order = oracle.dfs_preorder(g.row_ptr, g.dst)
    rng = np.random.default_rng(2)
    targets = rng.choice(g.n, size=30, replace=False).astype(np.uint32)
    off, runs = oracle.build_rows(g.row_ptr, g.dst, g.w, order, targets)
    s = rng.integers(0, g.n, NQ).astype(np.uint32)
    t = targets[rng.integers(0, len(targets), NQ)]
    sets = [None] + [cpd.synth_congestion(g.w, frac=0.3, lo=1.0, hi=3.0, seed=k)
                     for k in (3, 4, 5, 6)]
    demand = rng.integers(0, 1 << 32, NQ, dtype=np.uint64).astype(np.uint32)
    plain = oracle.table_search(g.row_ptr, g.dst, g.w, order, targets, off, runs, s, t)
    P = max(1, int(np.median(plain[0])) // 3)
    return g, order, targets, off, runs, s, t, sets, demand, P


def orc(w, g, order, targets, off, runs, s, t, k=-1):
    w = g.w if w is None else w
    return oracle.table_search(g.row_ptr, g.dst, w, order, targets, off, runs, s, t, k_moves=k)


def same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("graph", ["synth", "irregular", "deg8"])
def test_lock_step_is_the_scalar_loop(graph):
    g, order, targets, off, runs, s, t, sets, demand, P = world(graph)
    rng = np.random.default_rng(7)
    for K in (1, 3, 5):
        dep = rng.integers(0, K * P, NQ).astype(np.uint64)
        for k in (-1, 0, 1, 10):
            a = T.walk_timed(g, order, targets, off, runs, s, t, sets[:K], dep, P, demand, k)
            b = T.walk_timed_scalar(g, order, targets, off, runs, s, t, sets[:K], dep, P, demand, k)
            same(a, b)
            oc = orc(None, g, order, targets, off, runs, s, t, k)
            np.testing.assert_array_equal(a[1], oc[1])
            np.testing.assert_array_equal(a[2], oc[2])
    # the clock shows: three sets are not one of them
    w3 = T.walk_timed(g, order, targets, off, runs, s, t, sets[:3], dep % np.uint64(3 * P), P)
    assert np.any(w3[0] != orc(sets[0], g, order, targets, off, runs, s, t)[0])
    assert w3[3][1:].any()
    if graph == "irregular":  # the unfinished walks are there
        assert 0 < int(w3[2].sum()) < NQ


@pytest.mark.parametrize("graph", ["synth", "irregular", "deg8"])
def test_reference_is_pinned_by_the_oracle(graph):
    g, order, targets, off, runs, s, t, sets, demand, P = world(graph)
    rng = np.random.default_rng(8)
    dep = rng.integers(0, 1 << 40, NQ).astype(np.uint64)
    for k in (-1, 10):
        o = [orc(w, g, order, targets, off, runs, s, t, k) for w in sets]
        # one set: its cost, whatever the departure and the period
        for Pk in (1, P, 1 << 60):
            same(T.walk_timed(g, order, targets, off, runs, s, t, [sets[1]], dep, Pk, k_moves=k)[:3],
                 o[1])
        # equal sets: the same
        same(T.walk_timed(g, order, targets, off, runs, s, t, [sets[2]] * 4, dep, P, k_moves=k)[:3],
             o[2])
        # a period beyond every arrival: everything in set 0
        big = int(dep.max()) + int(o[0][0].max()) + 1
        out = T.walk_timed(g, order, targets, off, runs, s, t, sets, dep, big, demand, k)
        same(out[:3], o[0])
        assert not out[3][1:].any()
        # departures in the last set: W_{K-1}
        late = (dep + np.uint64(4 * P)).astype(np.uint64)
        out = T.walk_timed(g, order, targets, off, runs, s, t, sets, late, P, demand, k)
        same(out[:3], o[4])
        assert not out[3][:4].any()
        # the planes sum to the unsliced table
        mid = T.walk_timed(g, order, targets, off, runs, s, t, sets, dep % np.uint64(5 * P), P,
                           demand, k)
        full = L.walk_loads(g, order, targets, off, runs, s, t, demand, k_moves=k)
        np.testing.assert_array_equal(mid[3].sum(axis=0, dtype=np.uint64), full[0][0])
        np.testing.assert_array_equal(mid[1], o[0][1])
        np.testing.assert_array_equal(mid[2], o[0][2])


def test_hand_worked_path():
    # 0 -> 1 -> 2 -> 3, weights 5, 7, 2 (set 0) and 50, 70, 20 (set 1), P = 10
    g = graph_from_edges(4, [(0, 1, 5), (1, 2, 7), (2, 3, 2)])
    order = oracle.dfs_preorder(g.row_ptr, g.dst)
    targets = np.array([3], np.uint32)
    off, runs = oracle.build_rows(g.row_ptr, g.dst, g.w, order, targets)
    np.testing.assert_array_equal(g.w, [5, 7, 2])
    sets = [None, np.array([50, 70, 20], np.uint32)]
    s = np.array([0, 0, 0, 1], np.uint32)
    t = np.full(4, 3, np.uint32)
    dep = np.array([0, 9, 10, 3], np.uint64)   # P - 1 and exactly P among them
    dem = np.array([1, 10, 100, 1000], np.uint32)
    # q0: 0 @0 set 0 (5), 1 @5 set 0 (7), 2 @12 set 1 (20)            -> 32
    # q1: 0 @9 set 0 (5), 1 @14 set 1 (70), 2 @84 set 1 (20)          -> 95
    # q2: 0 @10 set 1 (50), 1 @60 set 1 (70), 2 @130 set 1 (20)       -> 140
    # q3: 1 @3 set 0 (7), 2 @10 set 1 (20)                            -> 27
    for walk in (T.walk_timed, T.walk_timed_scalar):
        cost, hops, fin, loads = walk(g, order, targets, off, runs, s, t, sets, dep, 10, dem)
        assert cost.tolist() == [32, 95, 140, 27]
        assert hops.tolist() == [3, 3, 3, 2] and fin.tolist() == [1, 1, 1, 1]
        assert loads.tolist() == [[11, 1001, 0], [100, 110, 1111]]


def test_header_declares_timed_entry_points():
    hdr = open(os.path.join(ROOT, "include", "cpd_api.h")).read()
    declared = set(re.findall(r"\b(cpd_[a-z_]+)\s*\(", hdr))
    assert set(NAMES) <= declared
    timed = re.search(r"#define\s+CPD_TIMED_LOADS\s+(\d+)u", hdr)
    acc = re.search(r"#define\s+CPD_LOADS_ACCUMULATE\s+(\d+)u", hdr)
    assert timed and acc and int(timed.group(1)) == 2
    assert int(timed.group(1)) & int(acc.group(1)) == 0


def test_python_mirror_has_timed():
    for attr in ("timed", "timed_run", "timed_fetch"):
        assert callable(getattr(cpd.Index, attr))
    for name in NAMES:
        assert name in cpd.EXPORTED and hasattr(cpd.lib, name)
    assert cpd.TIMED_LOADS == 2 and cpd.TIMED_LOADS != cpd.LOADS_ACCUMULATE


def test_library_exports_timed_symbols():
    so = C.CDLL(cpd.LIB_PATH)  # dlsym on the shared library itself
    for name in NAMES:
        assert getattr(so, name, None) is not None, name


def test_null_index_is_refused():
    st = cpd.QueryStats()
    assert cpd.lib.cpd_query_timed(None, C.c_int32(-1), None, C.c_uint64(1), None, C.c_uint32(0),
                                   C.byref(st)) == cpd.CPD_E_ARG
    assert cpd.lib.cpd_query_timed_fetch(None, None, None, None) == cpd.CPD_E_ARG
    assert cpd.lib.cpd_last_error()
