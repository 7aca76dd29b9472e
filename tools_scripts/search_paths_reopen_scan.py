#!/usr/bin/env python3
"""Counts, with the tests' restatement of the search (tests/search_paths_ref.py),
the searches at --hscale whose path read at the end differs from the reported
plen or undercuts the reported cost: all pairs of --graphs random --nodes-node
graphs (a ring plus 1-3 random out-edges a node, weights 1..19, half of the
edges congested by 1-3x), then the graph of tests/test_search_paths_cpu.py.
No GPU.  With --itrs N the expansion limit is set, which is what lets a search
end with a re-opened chain node still waiting (default: no limit)."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "distributed-oracle-search_amd", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np
import cpd
import oracle
from graphs import graph_from_edges
from search_paths_ref import SearchPathsRef, ref_search_paths

ap = argparse.ArgumentParser()
ap.add_argument("--graphs", type=int, default=400)
ap.add_argument("--nodes", type=int, default=40)
ap.add_argument("--hscale", type=float, default=1.5)
ap.add_argument("--itrs", type=int, default=-1)
a = ap.parse_args()


def count(g, wc, targets, s, t):
    order = cpd.Plan(g, hierarchy=False).order()
    off, runs = oracle.build_rows(g.row_ptr, g.dst, g.w, order, targets)
    ref = SearchPathsRef(g, order, targets, off, runs)
    c, p, f, _, paths, pc = ref_search_paths(ref, wc, s, t, hscale=a.hscale, itrs=a.itrs)
    return sum(1 for q in range(len(s)) if f[q] and (pc[q] < c[q] or len(paths[q]) - 1 != p[q]))


total = differ = 0
n = a.nodes
for seed in range(a.graphs):
    rng = np.random.default_rng(seed)
    edges = []
    for v in range(n):
        edges.append((v, (v + 1) % n, int(rng.integers(1, 20))))
        for _ in range(int(rng.integers(1, 4))):
            edges.append((v, int(rng.integers(0, n)), int(rng.integers(1, 20))))
    g = graph_from_edges(n, edges)
    wc = cpd.synth_congestion(g.w, frac=0.5, lo=1.0, hi=3.0, seed=4)
    s = np.repeat(np.arange(n), n).astype(np.uint32)
    t = np.tile(np.arange(n), n).astype(np.uint32)
    differ += count(g, wc, np.arange(n, dtype=np.uint32), s, t)
    total += len(s)
print(f"random graphs: {differ} of {total} searches differ")
g = cpd.synth_road_graph(64, 48, seed=31)
rng = np.random.default_rng(31)
targets = rng.choice(g.n, size=60, replace=False).astype(np.uint32)
s = rng.integers(0, g.n, 3000).astype(np.uint32)
t = targets[rng.integers(0, 60, 3000)]
wc = cpd.synth_congestion(g.w, frac=0.2, lo=1.0, hi=3.0, seed=4)
print(f"64 x 48 synth, seed 31: {count(g, wc, targets, s, t)} of 3000 searches differ")
