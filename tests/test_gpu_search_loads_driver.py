"""fifo_auto --alg cpd-search --search-loads driven as the reference head node
drives a worker (tests/driver_harness.py, as test_gpu_loads_driver.py and
test_gpu_search_paths_driver.py do): every request is answered through
cpd_query_search_loads at a demand of 1 per query line, <query file>.loads
holds every loaded edge of the routes found under the request's diff, equal to
ref_search_loads (tests/search_loads_ref.py) line for line, and the answer line
and <query file>.res are those of a run without the flag."""
import os

import numpy as np
import pytest

import cpd
import driver_harness as H
import oracle
from search_loads_ref import ref_search_loads
from search_paths_ref import SearchPathsRef
from test_gpu_drivers import _read_diff

pytestmark = pytest.mark.gpu
BIN = H.BIN
W, METHOD, KEY = 2, "mod", 3


def test_fifo_auto_search_loads(tmp_path):
    xy, diff, scen, outdir = H.build_index(tmp_path, W, METHOD, KEY)
    g = cpd.synth_road_graph(30, 24, seed=2)
    order = oracle.dfs_preorder(g.row_ptr, g.dst)
    wc = _read_diff(diff, g)
    src = np.repeat(np.arange(g.n), np.diff(g.row_ptr.astype(np.int64)))

    # --search-loads is cpd-search's, and not --search-paths' or the slices': refused at
    # start with exit 2 and one line
    for extra in (["--alg", "table-search", "--search-loads"],
                  ["--alg", "cpd-search", "--search-paths", "--search-loads"],
                  ["--alg", "cpd-search", "--search-loads", "--load-slices", "3",
                   "--load-slice-moves", "4"]):
        p = H.refused(xy, diff, outdir, extra, tmp_path, W, METHOD, KEY)
        assert p.returncode == 2, (extra, p.stderr)
        assert len(p.stderr.strip().splitlines()) == 1 and "--search-loads" in p.stderr
        assert not os.path.exists(tmp_path / "never.fifo")

    answers, res = {}, {}
    config = dict(H.DEFAULT_CONFIG, debug=True)  # per-query results into <query file>.res
    for flag in (False, True):
        nfs = str(tmp_path / ("nfs_loads" if flag else "nfs_plain"))
        os.makedirs(nfs)
        procs = H.serve(xy, diff, outdir, "cpd-search", ["--search-loads"] if flag else [], W,
                        METHOD, KEY)
        try:
            for pr in procs:
                H.wait_ready(pr, timeout=60)
            conf = {"workers": ["localhost"] * W, "nfs": nfs, "partmethod": METHOD, "partkey": KEY,
                    "xy_file": xy, "scenfile": scen, "diffs": [diff]}
            parts, stats = H.run(conf, dict(config))
        finally:
            H.quit(procs)
        answers[flag] = stats[0]
        res[flag] = [open(os.path.join(nfs, f"query.localhost{wid}.res")).read()
                     for wid in range(W)]
        side = sorted(f for f in os.listdir(nfs) if ".loads" in f)
        if not flag:
            assert side == []  # nothing changes without the flag
            continue
        assert side == [f"query.localhost{wid}.loads" for wid in range(W)]  # no .tmp left
        for wid, part in enumerate(parts):
            s = np.array([q[0] for q in part], np.uint32)
            t = np.array([q[1] for q in part], np.uint32)
            targets = np.unique(t)
            off, runs = oracle.build_rows(g.row_ptr, g.dst, g.w, order, targets)
            ref = SearchPathsRef(g, order, targets, off, runs)
            rc, rp, rf, rs, _, _, rl, moves, prefix_moves = ref_search_loads(ref, wc, s, t)
            assert prefix_moves > 50  # real searches under the diff
            edges = np.nonzero(rl)[0]
            want = [[int(e), int(src[e]), int(g.dst[e]), int(rl[e])] for e in edges]
            lines = open(os.path.join(nfs, side[wid])).read().splitlines()
            assert [[int(x) for x in line.split()] for line in lines] == want, wid
            row = answers[True][wid]
            assert int(row[0]) == int(rs[:, 0].sum()) and int(row[5]) == int(rp[rf == 1].sum())
            assert int(row[6]) == int(rf.sum())
            want_res = "".join(f"{a} {b} {c} {h} {f}\n" for a, b, c, h, f in
                               zip(s.tolist(), t.tolist(), rc.tolist(), rp.tolist(), rf.tolist()))
            assert res[True][wid] == want_res
    # .res and the seven non-time fields of the answer line are those of a plain run
    assert res[False] == res[True]
    for a, b in zip(answers[False], answers[True]):
        assert list(a[:7]) == list(b[:7]) and a[-1] == b[-1]
