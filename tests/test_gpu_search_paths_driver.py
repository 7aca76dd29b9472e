"""fifo_auto --alg cpd-search --search-paths driven as the reference head node
drives a worker (tests/driver_harness.py, as test_gpu_paths_driver.py does):
the answer line is the one a run without the flag gives, and <query
file>.paths holds every route's nodes, equal to ref_search_paths
(tests/search_paths_ref.py) under the request's diff weights."""
import os

import numpy as np
import pytest

import cpd
import driver_harness as H
import oracle
from search_paths_ref import SearchPathsRef, ref_search_paths
from test_gpu_drivers import _read_diff

pytestmark = pytest.mark.gpu
BIN = H.BIN
W, METHOD, KEY = 2, "mod", 3



def test_fifo_auto_search_paths(tmp_path):
    xy, diff, scen, outdir = H.build_index(tmp_path, W, METHOD, KEY)
    g = cpd.synth_road_graph(30, 24, seed=2)
    order = oracle.dfs_preorder(g.row_ptr, g.dst)
    wc = _read_diff(diff, g)

    # table-search has no search paths: refused at start, with one line
    p = H.refused(xy, diff, outdir, ["--alg", "table-search", "--search-paths"], tmp_path, W,
                  METHOD, KEY)
    assert p.returncode != 0
    assert len(p.stderr.strip().splitlines()) == 1 and "--search-paths" in p.stderr
    assert not os.path.exists(tmp_path / "never.fifo")

    answers = {}
    for flag in (False, True):
        nfs = str(tmp_path / ("nfs_paths" if flag else "nfs_plain"))
        os.makedirs(nfs)
        procs = H.serve(xy, diff, outdir, "cpd-search", ["--search-paths"] if flag else [], W,
                        METHOD, KEY)
        try:
            for pr in procs:
                H.wait_ready(pr, timeout=60)
            conf = {"workers": ["localhost"] * W, "nfs": nfs, "partmethod": METHOD, "partkey": KEY,
                    "xy_file": xy, "scenfile": scen, "diffs": [diff]}
            parts, stats = H.run(conf, dict(H.DEFAULT_CONFIG))
        finally:
            H.quit(procs)
        answers[flag] = stats[0]
        side = sorted(f for f in os.listdir(nfs) if ".paths" in f)
        if not flag:
            assert side == []  # nothing changes without the flag
            continue
        assert side == [f"query.localhost{wid}.paths" for wid in range(W)]
        for wid, part in enumerate(parts):
            s = np.array([q[0] for q in part], np.uint32)
            t = np.array([q[1] for q in part], np.uint32)
            targets = np.unique(t)
            off, runs = oracle.build_rows(g.row_ptr, g.dst, g.w, order, targets)
            ref = SearchPathsRef(g, order, targets, off, runs)
            rc, rp, rf, rs, paths, _ = ref_search_paths(ref, wc, s, t)
            assert (rs[:, 0] > 1).sum() > 50  # real searches under the diff
            lines = open(os.path.join(nfs, side[wid])).read().splitlines()
            assert len(lines) == len(part)           # one line per query, in file order
            for q, line in enumerate(lines):
                v = [int(x) for x in line.split()]
                assert v[:4] == [s[q], t[q], rf[q], len(paths[q])], (wid, q)
                assert v[4:] == paths[q], (wid, q)
            row = answers[True][wid]
            assert int(row[0]) == int(rs[:, 0].sum()) and int(row[5]) == int(rp[rf == 1].sum())
            assert int(row[6]) == int(rf.sum())
    # the seven non-time fields of the answer line are those of a plain run
    for a, b in zip(answers[False], answers[True]):
        assert list(a[:7]) == list(b[:7]) and a[-1] == b[-1]
