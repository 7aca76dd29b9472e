#!/usr/bin/env python3
"""Costs under several weight sets against what they replace, on the bench
workload (1M-node synthetic graph, one 16384-row batch, the bench's 1M-query
mix), both index forms, warm, --reps repeats, min / median / max.  One JSON
line per (what, form[, K]) appended to --out:

  --what plain    cpd_query_run alone (kernel_ms): the existing walk.  Run once
                  per build, processes alternating parent / new / parent / new.
  --what kwalks   K x (cpd_index_set_weights + cpd_query_run) for K in --ks:
                  host clock end to end (e2e_ms) and the K kernels (kernel_ms).
                  What costing a scenario under K diffs takes without the feature.
  --what costs    one cpd_index_set_weight_sets + cpd_query_costs at the same
                  K, all sets and sliced (--slice moves per set): e2e_ms and
                  kernel_ms; K = 1 is the case against the plain walk.

--pkg names the directory of the cpd.py (and libcpd.so) to load — the parent
commit's build for plain / kwalks (its library has no costs entry points, so
this tree's cpd.py cannot bind it) — and --tag labels the records.  The plan
is cached in --cache (built on first use).

  python tools_scripts/costs_ab.py --what plain  --pkg PARENT/distributed-oracle-search_amd --tag parent
  python tools_scripts/costs_ab.py --what plain  --tag new
  python tools_scripts/costs_ab.py --what kwalks --pkg PARENT/distributed-oracle-search_amd --tag parent
  python tools_scripts/costs_ab.py --what costs  --tag new"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--what", choices=["plain", "kwalks", "costs"], required=True)
ap.add_argument("--pkg", default=os.path.join(ROOT, "distributed-oracle-search_amd"))
ap.add_argument("--tag", default="")
ap.add_argument("--width", type=int, default=1000)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--queries", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--modes", default="dense,rle")
ap.add_argument("--ks", default="1,2,4,8")
ap.add_argument("--slice", type=int, default=64)
ap.add_argument("--cache", default="/tmp/cpd-bench-cache")
ap.add_argument("--out")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.pkg))
import numpy as np
import cpd


def spread(v):
    v = sorted(v)
    return {"min": round(v[0], 3), "med": round(v[len(v) // 2], 3), "max": round(v[-1], 3)}


def emit(rec):
    rec = {"tag": a.tag, "what": a.what, "queries": a.queries, "reps": a.reps,
           "lib": cpd.version(), **rec}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


os.makedirs(a.cache, exist_ok=True)
g = cpd.synth_road_graph(a.width, a.width, seed=a.seed)
plan, _ = cpd.Plan.cache(os.path.join(a.cache, f"synth{a.width}-s{a.seed}-ch823.plan"), g, gpu=0)
dev = cpd.Graph(plan, device=0)
targets = cpd.owned_nodes(g.n, 1, "div", 8, 0)[: dev.batch]
rows = dev.build_rows(targets)
rng = np.random.default_rng(100)
s = rng.integers(0, g.n, a.queries).astype(np.uint32)
t = targets[rng.integers(0, len(targets), a.queries)]
ks = [int(k) for k in a.ks.split(",")]
sets = [None] + [cpd.synth_congestion(g.w, frac=0.1, lo=1.0, hi=3.0, seed=2 + j)
                 for j in range(1, max(ks))]

for mode in a.modes.split(","):
    ix = cpd.Index(dev, rows=rows)
    ix.set_mode(mode)
    ix.prepare(s, t)
    st = ix.run()  # warm (dense: the tables are expanded)
    hops = int(st["hops"])
    if a.what == "plain":
        emit({"form": mode, "hops": hops,
              "kernel_ms": spread([ix.run()["kernel_ms"] for _ in range(a.reps)])})
    elif a.what == "kwalks":
        for K in ks:
            e2e, ker = [], []
            for _ in range(a.reps + 1):  # the first repeat warms the buffers
                t0 = time.perf_counter()
                k_ms = 0.0
                for w in sets[:K]:
                    ix.set_weights(w)
                    k_ms += ix.run()["kernel_ms"]
                e2e.append((time.perf_counter() - t0) * 1e3)
                ker.append(k_ms)
            emit({"form": mode, "K": K, "hops": hops, "e2e_ms": spread(e2e[1:]),
                  "kernel_ms": spread(ker[1:])})
        ix.set_weights(None)
    else:
        for K in ks:
            for S in (0, a.slice):
                e2e, ker = [], []
                for _ in range(a.reps + 1):
                    t0 = time.perf_counter()
                    ix.set_weight_sets(sets[:K])
                    c = ix.costs_run(slice_moves=S)
                    e2e.append((time.perf_counter() - t0) * 1e3)
                    ker.append(c["kernel_ms"])
                    assert c["hops"] == hops
                emit({"form": mode, "K": K, "slice": S, "hops": hops, "e2e_ms": spread(e2e[1:]),
                      "kernel_ms": spread(ker[1:])})
        plain = [ix.run()["kernel_ms"] for _ in range(a.reps)]
        emit({"form": mode, "K": 0, "note": "plain walk, same process", "hops": hops,
              "kernel_ms": spread(plain)})
    del ix
