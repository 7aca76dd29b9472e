"""Costs under several weight sets, without a GPU: the references of
tests/costs_ref.py agree with each other — the oracle identity for the sliced
mode against a lock-step numpy walk that costs hop h under set min(h // S, K -
1), the all-sets columns against the same walk — and the interface is there:
the header declares it, libcpd.so exports it, cpd.Index mirrors it."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import costs_ref as R
import cpd
import oracle
from graphs import GRAPHS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cpd_index_set_weight_sets", "cpd_query_costs", "cpd_query_costs_fetch")


@functools.lru_cache(maxsize=None)
def world(name):
    g = GRAPHS[name]()
    order = oracle.dfs_preorder(g.row_ptr, g.dst)
    rng = np.random.default_rng(2)
    targets = rng.choice(g.n, size=30, replace=False).astype(np.uint32)
    off, runs = oracle.build_rows(g.row_ptr, g.dst, g.w, order, targets)
    s = rng.integers(0, g.n, 600).astype(np.uint32)
    t = targets[rng.integers(0, len(targets), 600)]
    sets = [None] + [cpd.synth_congestion(g.w, frac=0.3, lo=1.0, hi=3.0, seed=k)
                     for k in (3, 4, 5, 6)]
    return g, order, targets, off, runs, s, t, sets


@pytest.mark.parametrize("graph", ["synth", "irregular", "deg8"])
def test_all_sets_reference_is_the_walk(graph):
    g, order, targets, off, runs, s, t, sets = world(graph)
    for k in (-1, 0, 1, 10):
        ref = R.ref_all(g, order, targets, off, runs, s, t, sets, k_moves=k)
        wlk = R.walk_costs(g, order, targets, off, runs, s, t, sets, k_moves=k)
        for a, b in zip(ref, wlk):
            np.testing.assert_array_equal(a, b)
    assert np.any(ref[0][:, 0] != ref[0][:, 1])  # the sets differ where it shows


@pytest.mark.parametrize("graph", ["synth", "irregular", "deg8"])
def test_sliced_identity_is_the_walk(graph):
    g, order, targets, off, runs, s, t, sets = world(graph)
    for K in (1, 2, 5):
        for S in (1, 3, 7, g.n):
            for k in (-1, 0, 1, 10):
                ref = R.ref_sliced(g, order, targets, off, runs, s, t, sets[:K], S, k_moves=k)
                wlk = R.walk_costs(g, order, targets, off, runs, s, t, sets[:K], S=S, k_moves=k)
                for a, b in zip(ref, wlk):
                    np.testing.assert_array_equal(a, b, err_msg=f"K={K} S={S} k={k}")
    # one slice holding every walk is set 0's column; equal sets the plain cost
    full = R.ref_all(g, order, targets, off, runs, s, t, sets)
    one = R.ref_sliced(g, order, targets, off, runs, s, t, sets, g.n)
    np.testing.assert_array_equal(one[0][:, 0], full[0][:, 0])
    same = R.ref_sliced(g, order, targets, off, runs, s, t, [sets[1]] * 3, 2)
    np.testing.assert_array_equal(same[0][:, 0], full[0][:, 1])


def test_header_declares_costs_entry_points():
    hdr = open(os.path.join(ROOT, "include", "cpd_api.h")).read()
    declared = set(re.findall(r"\b(cpd_[a-z_]+)\s*\(", hdr))
    assert set(NAMES) <= declared
    assert re.search(r"#define\s+CPD_MAX_WEIGHT_SETS\s+8u", hdr)


def test_python_mirror_has_costs():
    for attr in ("set_weight_sets", "costs", "costs_run", "costs_fetch"):
        assert callable(getattr(cpd.Index, attr))
    for name in NAMES:
        assert name in cpd.EXPORTED and hasattr(cpd.lib, name)


def test_library_exports_costs_symbols():
    so = C.CDLL(cpd.LIB_PATH)  # dlsym on the shared library itself
    for name in NAMES:
        assert getattr(so, name, None) is not None, name
