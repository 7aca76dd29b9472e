#!/usr/bin/env python3
"""Edge loads against the plain walk on the bench workload (1M-node synthetic
graph, one 16384-row batch, the bench's 1M-query mix), both index forms.  Per
form, warm, --reps repeats, min / median / max of the library's HIP-event
kernel times:

  walk_ms            cpd_query_run: the unchanged table_walk (the baseline)
  loads_k1_ms        cpd_query_loads, one slice
  loads_k8_ms        cpd_query_loads, 8 slices of 100 moves
  loads_fetch_ms     cpd_query_loads + cpd_query_loads_fetch end to end (host clock)
  paths_fetch_ms     the route it replaces: cpd_query_paths + the fetch of all
                     nodes (host clock; --paths-reps repeats)

  python tools_scripts/loads_ab.py [--out FILE.json] [--rounds N]
      --rounds N repeats the whole set N times in one process (alternating
      runs).  --baseline measures walk_ms alone: with CPD_PKG naming a
      directory that holds another build's cpd.py and libcpd.so (the parent
      commit's), the plain walk of that build.
  python tools_scripts/loads_ab.py --pmc OUT.json
      the loads kernel's L2 atomic and fabric write requests against its
      moves (rocprofv3, counters only, a run of its own per counter group;
      the child does one loads call per form and slice count)
The plan is cached in --cache (built on first use)."""
import argparse, csv, glob, json, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("CPD_PKG") or os.path.join(ROOT, "distributed-oracle-search_amd"))

PASSES = [
    ["TCC_EA0_ATOMIC_sum", "TCC_ATOMIC_sum", "TCC_EA0_WRREQ_sum", "TCC_EA0_WRREQ_64B_sum"],
    ["TCC_REQ_sum", "TCC_HIT_sum", "TCC_MISS_sum", "TCC_EA0_RDREQ_sum"],
]

ap = argparse.ArgumentParser()
ap.add_argument("--width", type=int, default=1000)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--queries", type=int, default=1_000_000)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--paths-reps", type=int, default=2)
ap.add_argument("--rounds", type=int, default=1)
ap.add_argument("--modes", default="dense,rle")
ap.add_argument("--cache", default="/tmp/cpd-bench-cache")
ap.add_argument("--out")
ap.add_argument("--baseline", action="store_true")
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
    dev = cpd.Graph(plan, device=0, batch=a.batch)
    targets = cpd.owned_nodes(g.n, 1, "div", 8, 0)[: dev.batch]
    rows = dev.build_rows(targets)
    rng = np.random.default_rng(100)
    s = rng.integers(0, g.n, a.queries).astype(np.uint32)
    t = targets[rng.integers(0, len(targets), a.queries)]
    return cpd, g, dev, rows, s, t


def measure():
    cpd, g, dev, rows, s, t = workload()
    out = {"queries": a.queries, "reps": a.reps, "lib": cpd.version(), "rounds": []}
    for rnd in range(a.rounds):
        res = {}
        for mode in a.modes.split(","):
            ix = cpd.Index(dev, rows=rows)
            ix.set_mode(mode)
            ix.prepare(s, t)
            st = ix.run()
            r = {"hops": int(st["hops"]),
                 "walk_ms": spread([ix.run()["kernel_ms"] for _ in range(a.reps)])}
            if a.baseline:
                res[mode] = r
                continue
            w = r["walk_ms"]["med"]
            if a.pmc_child:
                ix.loads_run()
                ix.loads_run(slices=8, slice_moves=100)
                res[mode] = r
                continue
            for key, kw in (("loads_k1_ms", {}), ("loads_k8_ms", {"slices": 8, "slice_moves": 100})):
                ix.loads_run(**kw)  # warm: the table is allocated, slot_of_edge uploaded
                r[key] = spread([ix.loads_run(**kw)["kernel_ms"] for _ in range(a.reps)])
                r[key.replace("_ms", "_over_walk")] = round(r[key]["med"] / w, 3)
            e2e = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                ix.loads_run()
                tab = ix.loads_fetch()
                e2e.append((time.perf_counter() - t0) * 1e3)
            assert int(tab.sum()) == r["hops"]
            r["loads_fetch_ms"] = spread(e2e)
            r["loads_bytes"] = int(tab.nbytes)
            ix.loads_clear()
            pf = []
            for _ in range(a.paths_reps + 1):  # the first one warms the node buffer
                t0 = time.perf_counter()
                off, _ = ix.paths_run()
                nodes = ix.paths_fetch(0, a.queries)
                pf.append((time.perf_counter() - t0) * 1e3)
                r["paths_bytes"] = int(nodes.nbytes)
                del nodes
            if len(pf) > 1:
                r["paths_fetch_ms"] = spread(pf[1:])
            res[mode] = r
            del ix
        out["rounds"].append(res)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return out


def pmc():
    base = tempfile.mkdtemp(prefix="loadspmc-")
    res = {}
    hops = None
    for i, counters in enumerate(PASSES):
        d = os.path.join(base, f"p{i}")
        cmd = ["timeout", "-s", "KILL", "400", "rocprofv3", "--pmc", *counters, "-d", d,
               "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
               "--pmc-child", "--reps", "1", "--width", str(a.width), "--seed", str(a.seed),
               "--queries", str(a.queries), "--modes", a.modes, "--cache", a.cache,
               "--batch", str(a.batch)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=base)
        files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
        if p.returncode or not files:
            print(f"pass {i} failed rc={p.returncode}: {p.stderr[-500:]}", file=sys.stderr)
            sys.exit(1)
        for line in p.stdout.splitlines():
            if line.startswith("{") and hops is None:
                hops = {m: v["hops"] for m, v in json.loads(line)["rounds"][0].items()}
        for row in csv.DictReader(open(files[0])):
            kn = row["Kernel_Name"]
            if "table_walk_loads" not in kn:
                continue
            mode = "dense" if "DenseRows" in kn else "rle"
            e = res.setdefault(mode, {}).setdefault(kn, {})
            e[row["Counter_Name"]] = e.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
    out = {"hops": hops, "kernels": res}
    os.makedirs(os.path.dirname(os.path.abspath(a.pmc)), exist_ok=True)
    json.dump(out, open(a.pmc, "w"), indent=1)
    print(json.dumps(out))
    shutil.rmtree(base, ignore_errors=True)


if __name__ == "__main__":
    if a.pmc:
        pmc()
    else:
        measure()
