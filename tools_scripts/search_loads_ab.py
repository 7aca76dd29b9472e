#!/usr/bin/env python3
"""What search loads cost, on the bench's search workload (search_paths_ab.py's:
the 1M-node synthetic graph, a 256-row dense index, the .diff stand-in
weights, 65536 queries) at fscale 0.1: cpd_query_search_loads warm, --repeats
times — the search passes (kernel_ms), loads_ms of the two load launches,
moves and prefix_moves — and beside it cpd_query_search_paths on the same
batch, whose paths_ms is the yardstick (the same prefixes and suffix walks,
stored as nodes instead of counted).  One JSON line per form; every repeat's
table is checked against the first (integer adds commute)."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--fscale", type=float, default=0.1)
ap.add_argument("--forms", default="tables,walks")
ap.add_argument("--queries", type=int, default=65536)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--cache", default="/tmp/cpd-bench-cache")
a = ap.parse_args()
sys.path.insert(0, os.path.join(ROOT, "distributed-oracle-search_amd"))
sys.path.insert(0, ROOT)
import numpy as np
import cpd
import bench

args = bench.parse(["--cache", a.cache])
os.makedirs(a.cache, exist_ok=True)
g = cpd.synth_road_graph(args.width, args.width, seed=args.seed, style=args.style)
pp = bench.plan_path(args)
if not os.path.exists(pp):
    cpd.Plan(g, gpu=0).save(pp)
plan = cpd.Plan.load(pp)
dev = cpd.Graph(plan, device=0, batch=1024)
dev.set_coords(g.x, g.y)
srows = bench.rank_targets(args, g.n, 1, 0)[:256]
rows = dev.build_rows(srows)
ix = cpd.Index.streamed(dev, srows, rows.count()[1], mode="dense")
ix.append_rows(rows)
del rows
ix.set_weights(cpd.synth_congestion(g.w, frac=0.1, lo=1.0, hi=3.0, seed=3))
rng = np.random.default_rng(5)
s = rng.integers(0, g.n, a.queries).astype(np.uint32)
t = srows[rng.integers(0, len(srows), a.queries)]


def mmm(v):
    v = sorted(v)
    return [round(v[0], 4), round(v[len(v) // 2], 4), round(v[-1], 4)]


for form in a.forms.split(","):
    ix.search(s[:64], t[:64], fscale=a.fscale, tables=form)  # warm (tables built)
    out = {"n": g.n, "m": g.m, "fscale": a.fscale, "form": form, "queries": a.queries,
           "repeats": a.repeats}
    ix.prepare(s, t)
    loads_ms, kernel_ms, paths_ms, paths_kernel_ms, first = [], [], [], [], None
    for _ in range(a.repeats):
        st = ix.search_loads_run(fscale=a.fscale, tables=form)
        tab = ix.loads_fetch()
        first = tab if first is None else first
        assert np.array_equal(tab, first) and int(tab.sum()) == st["loads"]["moves"]
        loads_ms.append(st["loads"]["loads_ms"])
        kernel_ms.append(st["kernel_ms"])
        out.update(moves=st["loads"]["moves"], prefix_moves=st["loads"]["prefix_moves"],
                   prefix_nodes=st["loads"]["prefix_nodes"], finished=int(st["finished"]),
                   expanded=int(st["expanded"]), passes=st["passes"], lanes=st["lanes"])
    for _ in range(a.repeats):
        off, st = ix.search_paths_run(fscale=a.fscale, tables=form)
        assert int(off[-1]) == out["moves"] + out["finished"]  # nodes = moves + 1 per route
        paths_ms.append(st["paths"]["paths_ms"])
        paths_kernel_ms.append(st["kernel_ms"])
    out["loads_ms_min_med_max"] = mmm(loads_ms)
    out["kernel_ms_min_med_max"] = mmm(kernel_ms)
    out["paths_ms_min_med_max"] = mmm(paths_ms)
    out["paths_kernel_ms_min_med_max"] = mmm(paths_kernel_ms)
    out["moves_per_s_med"] = round(out["moves"] / (mmm(loads_ms)[1] * 1e-3))
    out["loaded_edges"] = int(np.count_nonzero(first))
    print(json.dumps(out), flush=True)
