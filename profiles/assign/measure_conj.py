"""The conjugate step beside the line step and MSA on the 1M-node bench graph
(the setting of measure_line.py: synth_road_graph(1000, 1000, seed=1), 1024
index rows, 65536 queries, BPR, fscale 0.1, capacity[e] = max(4, the free-flow
loading of e)).  The three rules run in one process from the same start (free
flow, an empty flow table), ITERS iterations each, every iteration written out
by hand — cpd_query_search_loads, then one step — so that the step's three
device times come out apart:

  conj   cpd_index_flow_step_conj(CPD_ALPHA_CONJ, CPD_STEP_LINE), with the
         restart rule of cpd_query_assign_conj;
  line   cpd_index_flow_step(CPD_STEP_LINE);
  msa    cpd_index_flow_step(65536 // k).

The gap of a record is the exact relative gap before its step: -gy / xw0
(conj), -g0 / xw0 (line, msa).  One JSON object on stdout.

    python profiles/assign/measure_conj.py > conjugate.json
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "distributed-oracle-search_amd"))
import cpd  # noqa: E402

ITERS = 10


def run(ix, cap, rule):
    ix.set_weights(None)
    ix.flow_clear()
    its, restart = [], False
    for k in range(1, ITERS + 1):
        st = ix.search_loads_run(fscale=0.1)
        if rule == "conj":
            r = ix.flow_step_conj(cap, alpha=0 if restart else "conj")
            restart = r["lambda_q16"] == 0 and r["alpha_q16"] > 0
            num = r["gy"]
        else:
            r = ix.flow_step(cap, lam="line" if rule == "line" else 65536 // k)
            num = r["g0"]
        its.append({"k": k, "alpha_q16": r.get("alpha_q16"), "lambda_q16": r["lambda_q16"],
                    "evals": r["evals"], "gap": -num / r["xw0"] if r["xw0"] else None,
                    "conj_ms": r.get("conj_ms", 0.0), "line_ms": r["line_ms"],
                    "apply_ms": r["apply_ms"], "search_ms": st["kernel_ms"] + st["tables_ms"],
                    "changed": r["changed"], "tstt": str(r["tstt"])})
        if rule == "conj" and k >= 2 and r["lambda_q16"] == 0 and r["alpha_q16"] == 0:
            break
        if rule == "line" and k >= 2 and r["lambda_q16"] == 0:
            break
    return its


def step_ms(its):
    """Median and least device time of a whole step over the records that made
    all 18 evaluations."""
    full = [i["conj_ms"] + i["line_ms"] + i["apply_ms"] for i in its if i["evals"] == 18]
    parts = {k: statistics.median(i[k] for i in its if i["evals"] == 18)
             for k in ("conj_ms", "line_ms", "apply_ms")} if full else {}
    return {"records": len(full), "median_ms": statistics.median(full) if full else None,
            "min_ms": min(full) if full else None, "median_parts": parts}


def main():
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
    first = ix.search_loads(s, t, fscale=0.1)[0][0]  # also the warm-up of the search
    cap = np.maximum(first, 4).astype(np.uint32)
    out = {"graph": {"n": g.n, "m": g.m, "adjacency_slots": g.n * 4}, "queries": nq,
           "rows": len(targets), "setup_s": setup_s, "version": cpd.version(), "iters": ITERS,
           "loaded_edges": int((first > 0).sum())}
    # warm-up of both steps' code objects: two steps each, not recorded
    for warm in (lambda: ix.flow_step(cap), lambda: ix.flow_step_conj(cap)):
        ix.flow_clear()
        warm()
        warm()
    ix.prepare(s, t)
    for rule in ("conj", "line", "msa"):
        its = run(ix, cap, rule)
        out[rule] = {"iterations": its, "step": step_ms(its)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
