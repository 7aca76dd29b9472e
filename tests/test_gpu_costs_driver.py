"""fifo_auto --costs driven as the reference head node drives a worker
(tests/driver_harness.py, as test_gpu_paths_driver.py does): one request names
a list of diffs, the walk runs once, <query file>.res holds every query's cost
under each diff (or, with --slice-moves, the one sliced cost) equal to the
oracle's, and the answer line is the one a run without the flag gives."""
import os

import numpy as np
import pytest

import costs_ref as R
import cpd
import driver_harness as H
import oracle

pytestmark = pytest.mark.gpu
BIN = H.BIN
W, METHOD, KEY = 2, "mod", 3


def write_diff(path, g, wc):
    """A .diff as gen_synth writes it, and the weights fifo_auto reads from it
    (a line sets the first edge a -> b of the file)."""
    w = g.w.copy()
    rp = g.row_ptr.astype(np.int64)
    with open(path, "w") as f:
        f.write("c congestion diff: e from to new_cost\n")
        for a in range(g.n):
            for e in range(rp[a], rp[a + 1]):
                if wc[e] != g.w[e]:
                    f.write(f"e {a} {g.dst[e]} {wc[e]}\n")
                    first = rp[a] + int(np.nonzero(g.dst[rp[a]:rp[a + 1]] == g.dst[e])[0][0])
                    w[first] = wc[e]
    return w


def test_fifo_auto_costs(tmp_path):
    xy, diff, scen, outdir = H.build_index(tmp_path, W, METHOD, KEY)
    g = cpd.synth_road_graph(30, 24, seed=2)
    order = oracle.dfs_preorder(g.row_ptr, g.dst)
    da, db = str(tmp_path / "a.diff"), str(tmp_path / "b.diff")
    sets = [None,
            write_diff(da, g, cpd.synth_congestion(g.w, frac=0.3, lo=1.0, hi=3.0, seed=3)),
            write_diff(db, g, cpd.synth_congestion(g.w, frac=0.3, lo=1.0, hi=3.0, seed=4))]
    assert np.any(sets[1] != g.w) and np.any(sets[2] != sets[1])

    # --costs is table-search's, and not --paths': refused at start, with one line
    for extra in (["--alg", "cpd-search", "--costs"], ["--alg", "table-search", "--paths", "--costs"],
                  ["--alg", "table-search", "--slice-moves", "4"]):
        p = H.refused(xy, diff, outdir, extra, tmp_path, W, METHOD, KEY)
        assert p.returncode != 0
        assert len(p.stderr.strip().splitlines()) == 1
        assert ("--costs" in p.stderr) and not os.path.exists(tmp_path / "never.fifo")

    answers = {}
    for name, extra, S in (("plain", [], None), ("costs", ["--costs"], 0),
                           ("sliced", ["--costs", "--slice-moves", "4"], 4)):
        nfs = str(tmp_path / f"nfs_{name}")
        os.makedirs(nfs)
        procs = H.serve(xy, diff, outdir, "table-search", extra, W, METHOD, KEY)
        try:
            for pr in procs:
                H.wait_ready(pr, timeout=60)
            conf = {"workers": ["localhost"] * W, "nfs": nfs, "partmethod": METHOD, "partkey": KEY,
                    "xy_file": xy, "scenfile": scen,
                    "diffs": ["-" if S is None else f"-,{da},{db}"]}
            parts, stats = H.run(conf, dict(H.DEFAULT_CONFIG))
        finally:
            H.quit(procs)
        answers[name] = stats[0]
        side = sorted(f for f in os.listdir(nfs) if f.endswith(".res"))
        if S is None:
            assert side == []  # nothing changes without the flag
            continue
        assert side == [f"query.localhost{wid}.res" for wid in range(W)]
        for wid, part in enumerate(parts):
            s = np.array([q[0] for q in part], np.uint32)
            t = np.array([q[1] for q in part], np.uint32)
            targets = np.unique(t)
            off, runs = oracle.build_rows(g.row_ptr, g.dst, g.w, order, targets)
            if S:
                rc, rh, rf = R.ref_sliced(g, order, targets, off, runs, s, t, sets, S)
            else:
                rc, rh, rf = R.ref_all(g, order, targets, off, runs, s, t, sets)
                assert np.any(rc[:, 0] != rc[:, 1]) and np.any(rc[:, 1] != rc[:, 2])
            lines = open(os.path.join(nfs, side[wid])).read().splitlines()
            assert len(lines) == len(part)           # one line per query, in file order
            for q, line in enumerate(lines):
                v = [int(x) for x in line.split()]
                assert v == [s[q], t[q], rh[q], rf[q]] + rc[q].tolist(), (name, wid, q)
            row = answers[name][wid]
            assert int(row[0]) == int(rh.sum()) == int(row[5]) and int(row[6]) == int(rf.sum())
    # the answer line: 10 fields, the seven non-time ones those of a plain run
    for name in ("costs", "sliced"):
        for a, b in zip(answers["plain"], answers[name]):
            assert len(a) == len(b) == 13  # 10 fields + the harness's two times and size
            assert list(a[:7]) == list(b[:7]) and a[-1] == b[-1]
