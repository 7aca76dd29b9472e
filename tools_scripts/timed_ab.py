#!/usr/bin/env python3
"""Timed walks against the two kernels they combine, on the bench workload
(1M-node synthetic graph, one 16384-row batch, the bench's 1M-query mix), both
index forms, warm, --reps repeats, min / median / max of kernel_ms.  One JSON
line per (what, form, K) appended to --out:

  --what costs   cpd_query_costs, all sets, at K in --ks: the same record loads
                 as a timed walk makes — the yardstick.  Parent commit's build.
  --what loads   cpd_query_loads at K planes (K = 1: unsliced; else sliced at
                 mean hops / K moves per plane).  Parent commit's build.
  --what timed   cpd_query_timed at the same K without and with
                 CPD_TIMED_LOADS.  The period comes from the run itself: the
                 mean plain cost per query / K, so the walks span all K sets;
                 departures uniform in [0, K * period).

--pkg names the directory of the cpd.py (and libcpd.so) to load — the parent
commit's build for costs / loads (this tree's cpd.py cannot bind a library
without the timed entry points) — and --tag labels the records.  The plan is
cached in --cache (built on first use).

  python tools_scripts/timed_ab.py --what costs --pkg PARENT/distributed-oracle-search_amd --tag parent
  python tools_scripts/timed_ab.py --what loads --pkg PARENT/distributed-oracle-search_amd --tag parent
  python tools_scripts/timed_ab.py --what timed --tag new"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--what", choices=["costs", "loads", "timed"], required=True)
ap.add_argument("--pkg", default=os.path.join(ROOT, "distributed-oracle-search_amd"))
ap.add_argument("--tag", default="")
ap.add_argument("--width", type=int, default=1000)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--queries", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--modes", default="dense,rle")
ap.add_argument("--ks", default="1,4,8")
ap.add_argument("--cache", default="/tmp/cpd-bench-cache")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timed", "timed_ab.jsonl"))
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
    hops, mean_cost = int(st["hops"]), st["cost"] / a.queries
    plain = spread([ix.run()["kernel_ms"] for _ in range(a.reps)])
    for K in ks:
        base = {"form": mode, "K": K, "hops": hops, "plain_ms": plain}
        if a.what == "costs":
            ix.set_weight_sets(sets[:K])
            ms = [ix.costs_run()["kernel_ms"] for _ in range(a.reps + 1)][1:]
            emit({**base, "kernel_ms": spread(ms)})
        elif a.what == "loads":
            S = 0 if K == 1 else max(1, hops // a.queries // K)
            ms = [ix.loads_run(slices=K, slice_moves=S)["kernel_ms"] for _ in range(a.reps + 1)][1:]
            emit({**base, "slice_moves": S, "kernel_ms": spread(ms)})
        else:
            ix.set_weight_sets(sets[:K])
            P = max(1, int(mean_cost / K))
            dep = np.random.default_rng(101).integers(0, K * P, a.queries).astype(np.uint64)
            for loads in (False, True):
                runs = [ix.timed_run(dep, P, loads=loads) for _ in range(a.reps + 1)][1:]
                assert all(r["hops"] == hops for r in runs)
                rec = {**base, "period": P, "loads": loads,
                       "kernel_ms": spread([r["kernel_ms"] for r in runs])}
                if loads:  # how the moves spread over the K sets
                    rec["plane_share"] = [round(float(x), 4) for x in
                                          ix.loads_fetch().sum(axis=1, dtype=np.uint64) / hops]
                emit(rec)
    del ix
