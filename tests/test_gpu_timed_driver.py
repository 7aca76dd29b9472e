"""fifo_auto --timed driven as the reference head node drives a worker
(tests/driver_harness.py, as test_gpu_costs_driver.py does): a request names a
list of diffs, <query file>.dep the departures, the walk runs once on the clock
and <query file>.res holds every query's hops, finished, departure and cost
equal to tests/timed_ref.py's; with --loads <query file>.loads holds every
loaded edge's load per diff.  A .dep that does not fit the query file fails the
request, and the flag combinations that make no sense are refused at start."""
import os

import numpy as np
import pytest

import cpd
import driver_harness as H
import oracle
import timed_ref as T
from test_gpu_costs_driver import write_diff

pytestmark = pytest.mark.gpu
BIN = H.BIN
W, METHOD, KEY = 2, "mod", 3


def test_fifo_auto_timed(tmp_path):
    xy, diff, scen, outdir = H.build_index(tmp_path, W, METHOD, KEY)
    g = cpd.synth_road_graph(30, 24, seed=2)
    order = oracle.dfs_preorder(g.row_ptr, g.dst)
    src = np.repeat(np.arange(g.n), np.diff(g.row_ptr.astype(np.int64)))
    da = str(tmp_path / "a.diff")
    sets = [None, write_diff(da, g, cpd.synth_congestion(g.w, frac=0.3, lo=1.0, hi=3.0, seed=3))]
    assert np.any(sets[1] != g.w)

    # --timed is table-search's alone: refused at start, with one line
    for extra in (["--alg", "cpd-search", "--timed", "100"],
                  ["--alg", "table-search", "--paths", "--timed", "100"],
                  ["--alg", "table-search", "--costs", "--timed", "100"],
                  ["--alg", "table-search", "--timed", "100", "--loads", "--load-slices", "2",
                   "--load-slice-moves", "3"],
                  ["--alg", "table-search", "--timed", "100", "--load-slice-moves", "3"],
                  ["--alg", "table-search", "--timed", "0"],
                  ["--alg", "table-search", "--timed", str((1 << 60) + 1)]):
        p = H.refused(xy, diff, outdir, extra, tmp_path, W, METHOD, KEY)
        assert p.returncode != 0
        assert len(p.stderr.strip().splitlines()) == 1
        assert ("--timed" in p.stderr) and not os.path.exists(tmp_path / "never.fifo")

    # the head node's partition of the scenario, and each part's reference
    reqs = H.read_p2p(scen)
    code, parts = H.make_parts(reqs, H.get_node_num(xy), W, METHOD, KEY)
    assert code == 0 and len(parts) == W and all(parts)
    world = []
    for part in parts:
        s = np.array([q[0] for q in part], np.uint32)
        t = np.array([q[1] for q in part], np.uint32)
        targets = np.unique(t)
        off, runs = oracle.build_rows(g.row_ptr, g.dst, g.w, order, targets)
        world.append((s, t, (g, order, targets, off, runs)))
    plain = np.concatenate([oracle.table_search(g.row_ptr, g.dst, g.w, *wd[1:], s, t)[0]
                            for s, t, wd in world])
    P = max(1, int(np.median(plain)) // 2)
    rng = np.random.default_rng(70)
    deps = [rng.integers(0, 2 * P, len(part)).astype(np.uint64) for part in parts]
    deps[0][0] = (1 << 63) - 1  # the largest departure there is

    def run(nfs, dep_text):
        """One scenario through the resident workers; dep_text[wid]: the
        worker's .dep file (None: none)."""
        os.makedirs(nfs)
        for wid, text in enumerate(dep_text):
            if text is not None:
                with open(os.path.join(nfs, f"query.localhost{wid}.dep"), "w") as f:
                    f.write(text)
        conf = {"workers": ["localhost"] * W, "nfs": nfs, "partmethod": METHOD, "partkey": KEY,
                "xy_file": xy, "scenfile": scen, "diffs": [f"-,{da}"]}
        got, stats = H.run(conf, dict(H.DEFAULT_CONFIG))
        assert got == parts
        return stats[0], sorted(f for f in os.listdir(nfs) if not f.endswith(".dep"))

    good = ["".join(f"{int(d)}\n" for d in dep) for dep in deps]
    for name, extra in (("timed", ["--timed", str(P)]), ("loads", ["--timed", str(P), "--loads"])):
        procs = H.serve(xy, diff, outdir, "table-search", extra, W, METHOD, KEY)
        try:
            for pr in procs:
                H.wait_ready(pr, timeout=60)
            rows, side = run(str(tmp_path / f"nfs_{name}"), good)
            rows0, side0 = run(str(tmp_path / f"nfs_{name}_nodep"), [None] * W)
            if name == "timed":
                # worker 0's file a line short, worker 1's whole
                bad = [good[0].rsplit("\n", 2)[0] + "\n"] + good[1:]
                rows_bad, side_bad = run(str(tmp_path / "nfs_count"), bad)
                # a number that is none; a line too many
                mal = [good[0].replace("\n", "x\n", 1)] + [text + "7\n" for text in good[1:]]
                rows_mal, side_mal = run(str(tmp_path / "nfs_malformed"), mal)
        finally:
            H.quit(procs)
        want_side = [f"query.localhost{wid}{ext}" for wid in range(W)
                     for ext in ((".loads", ".res") if name == "loads" else (".res",))]
        assert side == want_side and side0 == want_side  # no .tmp left
        for nfs, dd, rr in ((f"nfs_{name}", deps, rows), (f"nfs_{name}_nodep", [None] * W, rows0)):
            for wid, (s, t, wd) in enumerate(world):
                rc, rh, rf, rl = T.walk_timed(*wd, s, t, sets, dd[wid], P)
                if dd[wid] is not None:
                    assert rl[0].any() and rl[1].any()
                d = np.zeros(len(s), np.uint64) if dd[wid] is None else dd[wid]
                lines = open(tmp_path / nfs / f"query.localhost{wid}.res").read().splitlines()
                assert len(lines) == len(s)          # one line per query, in file order
                for q, line in enumerate(lines):
                    assert [int(x) for x in line.split()] == \
                           [s[q], t[q], rh[q], rf[q], int(d[q]), int(rc[q])], (nfs, wid, q)
                if name == "loads":
                    edges = np.nonzero(rl.any(axis=0))[0]
                    want = [[int(e), int(src[e]), int(g.dst[e]), int(rl[0, e]), int(rl[1, e])]
                            for e in edges]
                    lines = open(tmp_path / nfs / f"query.localhost{wid}.loads").read().splitlines()
                    assert [[int(x) for x in line.split()] for line in lines] == want, (nfs, wid)
                row = rr[wid]
                assert len(row) == 13  # 10 fields + the harness's two times and size
                assert int(row[0]) == int(rh.sum()) == int(row[5]) and int(row[6]) == int(rf.sum())
    # the failed requests: the all-zero answer, nothing written; the worker whose .dep
    # was left whole answered as before
    for wid in range(W):
        assert [int(x) for x in rows_mal[wid][:7]] == [0] * 7
    assert [int(x) for x in rows_bad[0][:7]] == [0] * 7
    assert list(rows_bad[1][:7]) == list(rows[1][:7])
    assert side_mal == []
    assert side_bad == [f"query.localhost{wid}.res" for wid in range(1, W)]
