"""fifo_auto --loads driven as the reference head node drives a worker
(tests/driver_harness.py, as test_gpu_costs_driver.py does): every request is
answered through cpd_query_loads at a demand of 1 per query line, <query
file>.loads holds every loaded edge's load (or, with --load-slices /
--load-slice-moves, its load per time slice) equal to the reference's, and the
answer line is the one a run without the flag gives."""
import os

import numpy as np
import pytest

import cpd
import driver_harness as H
import loads_ref as L
import oracle

pytestmark = pytest.mark.gpu
BIN = H.BIN
W, METHOD, KEY = 2, "mod", 3


def test_fifo_auto_loads(tmp_path):
    xy, diff, scen, outdir = H.build_index(tmp_path, W, METHOD, KEY)
    g = cpd.synth_road_graph(30, 24, seed=2)
    order = oracle.dfs_preorder(g.row_ptr, g.dst)
    src = np.repeat(np.arange(g.n), np.diff(g.row_ptr.astype(np.int64)))

    # --loads is table-search's, and not --paths' or --costs': refused at start, with one line
    for extra in (["--alg", "cpd-search", "--loads"], ["--alg", "table-search", "--paths", "--loads"],
                  ["--alg", "table-search", "--costs", "--loads"]):
        p = H.refused(xy, diff, outdir, extra, tmp_path, W, METHOD, KEY)
        assert p.returncode != 0
        assert len(p.stderr.strip().splitlines()) == 1
        assert ("--loads" in p.stderr) and not os.path.exists(tmp_path / "never.fifo")

    answers = {}
    for name, extra, K, S in (("plain", [], None, 0), ("loads", ["--loads"], 1, 0),
                              ("sliced", ["--loads", "--load-slices", "3", "--load-slice-moves",
                                          "4"], 3, 4)):
        nfs = str(tmp_path / f"nfs_{name}")
        os.makedirs(nfs)
        procs = H.serve(xy, diff, outdir, "table-search", extra, W, METHOD, KEY)
        try:
            for pr in procs:
                H.wait_ready(pr, timeout=60)
            conf = {"workers": ["localhost"] * W, "nfs": nfs, "partmethod": METHOD, "partkey": KEY,
                    "xy_file": xy, "scenfile": scen, "diffs": ["-"]}
            parts, stats = H.run(conf, dict(H.DEFAULT_CONFIG))
        finally:
            H.quit(procs)
        answers[name] = stats[0]
        side = sorted(os.listdir(nfs))
        if K is None:
            assert side == []  # nothing changes without the flag
            continue
        assert side == [f"query.localhost{wid}.loads" for wid in range(W)]  # no .res, no .tmp
        for wid, part in enumerate(parts):
            s = np.array([q[0] for q in part], np.uint32)
            t = np.array([q[1] for q in part], np.uint32)
            targets = np.unique(t)
            off, runs = oracle.build_rows(g.row_ptr, g.dst, g.w, order, targets)
            rl, rh, rf = L.walk_loads(g, order, targets, off, runs, s, t, K=K, S=S)
            if K > 1:
                assert all(rl[j].any() for j in range(K))
            edges = np.nonzero(rl.any(axis=0))[0]
            want = [[int(e), int(src[e]), int(g.dst[e])] + [int(rl[j, e]) for j in range(K)]
                    for e in edges]
            lines = open(os.path.join(nfs, side[wid])).read().splitlines()
            assert [[int(x) for x in line.split()] for line in lines] == want, (name, wid)
            row = answers[name][wid]
            assert int(row[0]) == int(rh.sum()) == int(row[5]) and int(row[6]) == int(rf.sum())
    # the answer line: 10 fields, the seven non-time ones those of a plain run
    for name in ("loads", "sliced"):
        for a, b in zip(answers["plain"], answers[name]):
            assert len(a) == len(b) == 13  # 10 fields + the harness's two times and size
            assert list(a[:7]) == list(b[:7]) and a[-1] == b[-1]
