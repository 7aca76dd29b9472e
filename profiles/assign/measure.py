"""Timings of the assignment loop on the 1M-node bench graph (bench.py's
synth1m: synth_road_graph(1000, 1000, seed=1)), one JSON object on stdout:

  - cpd_query_assign, 3 iterations at fscale 0.1 on 65536 queries (the query
    count of the bench's cpd-search leg) over 1024 index rows: search_ms,
    loads_ms and vdf_ms of every iteration;
  - the wall time of one update through cpd_index_weights_from_loads (host
    clock around the call, which ends in a device synchronise), 20 calls;
  - the wall time of the same update done the old way — cpd_query_loads_fetch,
    the delay function in numpy (u64), cpd_index_set_weights — 5 calls, and
    that both ways leave the same weights.

    python profiles/assign/measure.py > assign.json
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "distributed-oracle-search_amd"))
import cpd  # noqa: E402

A_NUM, A_DEN, POWER = 3, 20, 4


def vdf_numpy(w0, loads, cap, load_div):
    x = loads // np.uint64(load_div)
    c = cap.astype(np.uint64)
    r = np.where(x >= (c << np.uint64(4)), np.uint64(1 << 20),
                 (np.minimum(x, c << np.uint64(4)) << np.uint64(16)) // c)
    p = r.copy()
    for _ in range(POWER - 1):
        p = (p * r) >> np.uint64(16)
    t = (w0.astype(np.uint64) * p) >> np.uint64(16)
    add = t * np.uint64(A_NUM) // np.uint64(A_DEN)
    return np.minimum(w0.astype(np.uint64) + add, np.uint64(0xFFFFFFFF)).astype(np.uint32)


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
    cap = rng.integers(1, 64, g.m).astype(np.uint32)
    ix.assign(s, t, cap, 1, fscale=0.1)  # warm-up: code objects, buffers, tables
    ix.set_weights(None)
    recs = ix.assign(s, t, cap, 3, fscale=0.1)
    loads = ix.loads_fetch()
    new_ms, old_ms = [], []
    for _ in range(20):
        t0 = time.perf_counter()
        info = ix.weights_from_loads(cap, a=(A_NUM, A_DEN), power=POWER, load_div=3)
        new_ms.append((time.perf_counter() - t0) * 1e3)
    w_new = ix.get_weights()
    for _ in range(5):
        t0 = time.perf_counter()
        w_old = vdf_numpy(g.w, ix.loads_fetch()[0], cap, 3)
        ix.set_weights(w_old)
        old_ms.append((time.perf_counter() - t0) * 1e3)
    slots = g.n * 4
    print(json.dumps({
        "graph": {"n": g.n, "m": g.m, "adjacency_slots": slots}, "queries": nq, "rows": len(targets),
        "setup_s": setup_s, "version": cpd.version(),
        "iterations": [{k: r[k] for k in ("finished", "moves", "changed", "search_ms", "loads_ms",
                                          "vdf_ms")} | {"sptt": str(r["sptt"]), "tstt": str(r["tstt"])}
                       for r in recs],
        "loaded_edges": int((loads[0] > 0).sum()),
        "update_device_path_wall_ms": new_ms, "update_kernel_ms_last": info["vdf_ms"],
        "update_host_round_trip_wall_ms": old_ms,
        "same_weights": bool(np.array_equal(w_new, ix.get_weights())),
    }))


if __name__ == "__main__":
    main()
