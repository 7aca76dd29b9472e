#!/usr/bin/env python3
"""What search paths cost, on the bench's search workload (search_ab.py's:
the 1M-node synthetic graph, a 256-row dense index, the .diff stand-in
weights, 65536 queries): cpd_query_search_paths against cpd_query_search of
the same build, warm, --repeats times each, the plain searches first and
one more after the paths calls (search_after: the index is left as it was).  One JSON line per
(leg, form): per repeat the search passes (kernel_ms), paths_ms and the D2H
of the nodes; lanes, reruns, prefix_nodes against nodes.

--mode search runs cpd_query_search alone, and --pkg names the directory of
the cpd.py (and libcpd.so) to load: the parent commit's build for the
"existing search must not get slower" comparison — one process per build, in
the order parent / new / parent / new.  (ab_libs.sh's CPD_LIB cannot load a
parent build here: this tree's cpd.py binds cpd_query_search_paths, which the
parent's library does not export.)  --tag labels the records; in each
process all the plain searches run before the first paths call."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=["both", "search"], default="both")
ap.add_argument("--pkg", default=os.path.join(ROOT, "distributed-oracle-search_amd"))
ap.add_argument("--legs", default="0.1,0")       # fscale of each leg
ap.add_argument("--forms", default="tables,walks")
ap.add_argument("--queries", type=int, default=65536)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--tag", default="")
ap.add_argument("--cache", default="/tmp/cpd-bench-cache")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.pkg))
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
KEEP = ("kernel_ms", "lanes", "passes", "reruns", "resumed", "restarted", "capacity",
        "capacity_last", "overflow")

for fs in [float(x) for x in a.legs.split(",")]:
    for form in a.forms.split(","):
        ix.search(s[:64], t[:64], fscale=fs, tables=form)  # warm (tables built)
        out = {"tag": a.tag, "fscale": fs, "form": form,
               "queries": a.queries, "search": [], "paths": []}
        for _ in range(a.repeats):
            _, _, fin, _, st = ix.search(s, t, fscale=fs, tables=form)
            out["search"].append({k: st[k] for k in KEEP})
            out["expanded"], out["finished"] = int(st["expanded"]), int(fin.sum())
        for _ in range(a.repeats if a.mode == "both" else 0):
            ix.prepare(s, t)
            off, st = ix.search_paths_run(fscale=fs, tables=form)
            t0 = time.perf_counter()
            nodes = ix.paths_fetch(0, a.queries)
            d2h = time.perf_counter() - t0
            assert int(st["expanded"]) == out["expanded"] and len(nodes) == int(off[-1])
            out["paths"].append({**{k: st[k] for k in KEEP}, **st["paths"],
                                 "d2h_ms": round(d2h * 1e3, 3)})
        if out["paths"]:
            _, _, _, _, st = ix.search(s, t, fscale=fs, tables=form)
            out["search_after"] = {k: st[k] for k in KEEP}
        ms = sorted(r["kernel_ms"] for r in out["search"])
        out["search_ms_min_med_max"] = [round(ms[0], 3), round(ms[len(ms) // 2], 3), round(ms[-1], 3)]
        if out["paths"]:
            pm = sorted(r["kernel_ms"] for r in out["paths"])
            out["paths_search_ms_min_med_max"] = [round(pm[0], 3), round(pm[len(pm) // 2], 3),
                                                  round(pm[-1], 3)]
        print(json.dumps(out), flush=True)
