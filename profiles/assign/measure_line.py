"""The flow step on the 1M-node bench graph (the setting of measure.py:
synth_road_graph(1000, 1000, seed=1), 1024 index rows, 65536 queries, BPR,
fscale 0.1), but with capacities in proportion to the demand — capacity[e] =
max(4, the free-flow loading of e) — so that the searches stay short.  One
JSON object on stdout:

  --rule line   cpd_query_assign_line, ITERS iterations: per iteration lambda,
                evals, line_ms, apply_ms (vdf_ms), search_ms, loads_ms and the
                gap -g0 / xw0; then vdf_ms of cpd_index_weights_from_loads on
                the same resident table, the yardstick for line_ms / evals;
  --rule msa    the same loop with MSA's step: cpd_query_search_loads and
                cpd_index_flow_step(65536 // k) per iteration, the gap from the
                same record.

    python profiles/assign/measure_line.py --rule line > line.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "distributed-oracle-search_amd"))
import cpd  # noqa: E402

ITERS = 4
KEYS = ("lambda_q16", "evals", "line_ms", "search_ms", "loads_ms", "changed", "finished")


def gap(r):
    return -r["g0"] / r["xw0"] if r["xw0"] else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rule", choices=("line", "msa"), default="line")
    rule = ap.parse_args().rule
    g = cpd.synth_road_graph(1000, 1000, seed=1)
    t0 = time.perf_counter()
    plan = cpd.Plan(g, gpu=0)
    dev = cpd.Graph(plan, batch=1024)
    rng = np.random.default_rng(7)
    targets = rng.choice(g.n, 1024, replace=False).astype(np.uint32)
    ix = cpd.Index(dev, rows=dev.build_rows(targets))
    setup_s = time.perf_counter() - t0
    nq = 65536
    s = rng.integers(0, g.n, nq).astype(np.uint32)
    t = targets[rng.integers(0, len(targets), nq)]
    first = ix.search_loads(s, t, fscale=0.1)[0][0]  # also the warm-up
    cap = np.maximum(first, 4).astype(np.uint32)
    out = {"graph": {"n": g.n, "m": g.m, "adjacency_slots": g.n * 4}, "queries": nq,
           "rows": len(targets), "setup_s": setup_s, "version": cpd.version(), "rule": rule,
           "loaded_edges": int((first > 0).sum())}
    if rule == "line":
        ix.assign_line(s, t, cap, 1, fscale=0.1)  # warm-up of the step's code objects
        ix.set_weights(None)
        recs = ix.assign_line(s, t, cap, ITERS, fscale=0.1)
        out["iterations"] = [{k: r[k] for k in KEYS} | {"apply_ms": r["vdf_ms"], "gap": gap(r),
                                                        "sptt": str(r["sptt"]), "tstt": str(r["tstt"])}
                             for r in recs]
        # the existing one-evaluation pass over the same resident table
        out["weights_from_loads_vdf_ms"] = [ix.weights_from_loads(cap)["vdf_ms"] for _ in range(5)]
    else:
        ix.flow_clear()
        ix.prepare(s, t)
        its = []
        for k in range(1, ITERS + 1):
            st = ix.search_loads_run(fscale=0.1)
            r = ix.flow_step(cap, lam=65536 // k)
            its.append({"lambda_q16": r["lambda_q16"], "evals": r["evals"], "line_ms": r["line_ms"],
                        "apply_ms": r["apply_ms"], "gap": gap(r), "changed": r["changed"],
                        "search_ms": st["kernel_ms"] + st["tables_ms"], "tstt": str(r["tstt"])})
        out["iterations"] = its
    print(json.dumps(out))


if __name__ == "__main__":
    main()
