#!/usr/bin/env python3
"""Path extraction against the plain walk on the bench workload (1M-node
synthetic graph, one 16384-row batch, the bench's 1M-query mix), both index
forms.  Per form, warm, --reps repeats, min / median / max:

  walk_ms      cpd_query_run: the unchanged table_walk (the baseline)
  count_ms     the same walk as cpd_query_paths' count pass
  offsets_ms   scatter + widen + exclusive sum
  fill_ms      table_walk_paths; fill_gbs = 4 * nodes / fill_ms (its stores)
  paths_ms     cpd_query_paths end to end (host clock, the offsets copy
               included); fetch_ms: all nodes to the host
The steps are the library's own HIP-event times (cpd_timing_get).

  python tools_scripts/paths_ab.py [--out FILE.json]
  python tools_scripts/paths_ab.py --pmc OUT.json   fill kernel's L2 -> fabric
      write traffic against 4 * nodes (rocprofv3, counters only, a run of its
      own per counter group; the child does one paths call per form)
The plan is cached in --cache (built on first use)."""
import argparse, csv, glob, json, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-oracle-search_amd"))

PASSES = [
    ["TCC_EA0_WRREQ_sum", "TCC_EA0_WRREQ_64B_sum", "TCC_REQ_sum", "TCC_WRITE_sum"],
    ["TCC_HIT_sum", "TCC_MISS_sum", "TCC_EA0_RDREQ_sum", "TCC_EA0_RDREQ_32B_sum"],
]

ap = argparse.ArgumentParser()
ap.add_argument("--width", type=int, default=1000)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--queries", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--modes", default="dense,rle")
ap.add_argument("--cache", default="/tmp/cpd-bench-cache")
ap.add_argument("--out")
ap.add_argument("--pmc", metavar="OUT.json")
ap.add_argument("--pmc-child", action="store_true")
a = ap.parse_args()


def spread(v):
    v = sorted(v)
    return {"min": round(v[0], 3), "med": round(v[len(v) // 2], 3), "max": round(v[-1], 3)}


def workload():
    import numpy as np
    import cpd
    os.makedirs(a.cache, exist_ok=True)
    g = cpd.synth_road_graph(a.width, a.width, seed=a.seed)
    plan, _ = cpd.Plan.cache(os.path.join(a.cache, f"synth{a.width}-s{a.seed}-ch823.plan"), g,
                             gpu=0)
    dev = cpd.Graph(plan, device=0)
    targets = cpd.owned_nodes(g.n, 1, "div", 8, 0)[: dev.batch]
    rows = dev.build_rows(targets)
    rng = np.random.default_rng(100)
    s = rng.integers(0, g.n, a.queries).astype(np.uint32)
    t = targets[rng.integers(0, len(targets), a.queries)]
    return cpd, dev, rows, s, t


def measure():
    import numpy as np
    cpd, dev, rows, s, t = workload()
    out = {"queries": a.queries, "reps": a.reps, "lib": os.environ.get("CPD_LIB", "tree")}
    for mode in a.modes.split(","):
        ix = cpd.Index(dev, rows=rows)
        ix.set_mode(mode)
        ix.prepare(s, t)
        ix.run()
        walk = [ix.run()["kernel_ms"] for _ in range(a.reps)]
        if a.pmc_child:
            reps = 1
        else:
            reps = a.reps
        res = {}

        def paths():
            res["off"], res["st"] = ix.paths_run()
        if not a.pmc_child:
            paths()  # warm: the node buffer is allocated, node_of_col uploaded
        steps = {"count_ms": [], "offsets_ms": [], "fill_ms": [], "paths_ms": []}
        sfx = "_dense" if mode == "dense" else ""
        for _ in range(reps):
            dev.timing(True)
            dev.timing_reset()
            t0 = time.perf_counter()
            paths()
            steps["paths_ms"].append((time.perf_counter() - t0) * 1e3)
            tm = dev.timing_get()
            dev.timing(False)
            steps["count_ms"].append(tm["table_search" + sfx]["ms"])
            steps["offsets_ms"].append(tm["table_paths_offsets"]["ms"])
            steps["fill_ms"].append(tm["table_paths" + sfx]["ms"])
        off, st = res["off"], res["st"]
        nodes = int(off[-1])
        fetch = []
        for _ in range(0 if a.pmc_child else min(reps, 2)):
            t0 = time.perf_counter()
            v = ix.paths_fetch(0, a.queries)
            fetch.append((time.perf_counter() - t0) * 1e3)
            assert len(v) == nodes and np.array_equal(v[off[:-1].astype(np.int64)], s)
            del v
        r = {"nodes": nodes, "hops": int(st["hops"]), "walk_ms": spread(walk)}
        r.update({k: spread(v) for k, v in steps.items()})
        if fetch:
            r["fetch_ms"] = spread(fetch)
        f = sorted(steps["fill_ms"])[len(steps["fill_ms"]) // 2]
        w = sorted(walk)[len(walk) // 2]
        r["fill_gbs"] = round(4.0 * nodes / f / 1e6, 2)
        r["fill_over_walk"] = round(f / w, 3)
        out[mode] = r
        del ix
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return out


def pmc():
    base = tempfile.mkdtemp(prefix="pathspmc-")
    res = {}
    nodes = None
    for i, counters in enumerate(PASSES):
        d = os.path.join(base, f"p{i}")
        cmd = ["timeout", "-s", "KILL", "400", "rocprofv3", "--pmc", *counters, "-d", d,
               "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
               "--pmc-child", "--reps", "1", "--width", str(a.width), "--seed", str(a.seed),
               "--queries", str(a.queries), "--modes", a.modes, "--cache", a.cache]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=base)
        files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
        if p.returncode or not files:
            print(f"pass {i} failed rc={p.returncode}: {p.stderr[-500:]}", file=sys.stderr)
            sys.exit(1)
        for line in p.stdout.splitlines():
            if line.startswith("{") and nodes is None:
                nodes = {m: json.loads(line)[m]["nodes"] for m in a.modes.split(",")}
        for row in csv.DictReader(open(files[0])):
            kn = row["Kernel_Name"]
            if "table_walk_paths" not in kn:
                continue
            k = "dense" if "DenseRows" in kn else "rle"
            e = res.setdefault(k, {})
            e[row["Counter_Name"]] = e.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
    for k, e in res.items():
        # a write request carries 64 B when counted in _64B, else 32 B
        w64 = e.get("TCC_EA0_WRREQ_64B_sum", 0.0)
        w32 = e.get("TCC_EA0_WRREQ_sum", 0.0) - w64
        e["write_bytes"] = 64.0 * w64 + 32.0 * w32
        e["nodes"] = (nodes or {}).get(k)
        if e["nodes"]:
            e["write_amplification"] = round(e["write_bytes"] / (4.0 * e["nodes"]), 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.pmc)), exist_ok=True)
    json.dump(res, open(a.pmc, "w"), indent=1)
    print(json.dumps(res))
    shutil.rmtree(base, ignore_errors=True)


if __name__ == "__main__":
    if a.pmc:
        pmc()
    else:
        measure()
