"""fifo_auto --paths driven as the reference head node drives a worker
(tests/driver_harness.py, as test_gpu_drivers.py does): the answer line is the
one a run without the flag gives, and <query file>.paths holds every walk's
nodes, equal to the numpy walk of test_gpu_paths.py over the oracle's rows."""
import os

import numpy as np
import pytest

import cpd
import driver_harness as H
import oracle
from test_gpu_paths import pinned, ref_paths

pytestmark = pytest.mark.gpu
BIN = H.BIN
W, METHOD, KEY = 2, "mod", 3



def test_fifo_auto_paths(tmp_path):
    xy, diff, scen, outdir = H.build_index(tmp_path, W, METHOD, KEY)
    g = cpd.synth_road_graph(30, 24, seed=2)
    order = oracle.dfs_preorder(g.row_ptr, g.dst)

    # cpd-search has no paths: refused at start, with one line
    p = H.refused(xy, diff, outdir, ["--alg", "cpd-search", "--paths"], tmp_path, W, METHOD, KEY)
    assert p.returncode != 0
    assert len(p.stderr.strip().splitlines()) == 1 and "--paths" in p.stderr
    assert not os.path.exists(tmp_path / "never.fifo")

    answers = {}
    for flag in (False, True):
        nfs = str(tmp_path / ("nfs_paths" if flag else "nfs_plain"))
        os.makedirs(nfs)
        procs = H.serve(xy, diff, outdir, "table-search", ["--paths"] if flag else [], W, METHOD,
                        KEY)
        try:
            for pr in procs:
                H.wait_ready(pr, timeout=60)
            conf = {"workers": ["localhost"] * W, "nfs": nfs, "partmethod": METHOD, "partkey": KEY,
                    "xy_file": xy, "scenfile": scen, "diffs": ["-"]}
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
            ref = ref_paths(g, order, targets, off, runs, s, t)
            rc, rh, rf = pinned(ref, g, order, targets, off, runs, s, t)
            lines = open(os.path.join(nfs, side[wid])).read().splitlines()
            assert len(lines) == len(part)           # one line per query, in file order
            o = ref[0].astype(np.int64)
            for q, line in enumerate(lines):
                v = [int(x) for x in line.split()]
                assert v[:4] == [s[q], t[q], rf[q], rh[q] + 1], (wid, q)
                assert v[4:] == ref[1][o[q]:o[q + 1]].tolist(), (wid, q)
            row = answers[True][wid]
            assert int(row[0]) == int(rh.sum()) == int(row[5]) and int(row[6]) == int(rf.sum())
    # the seven non-time fields of the answer line are those of a plain run
    for a, b in zip(answers[False], answers[True]):
        assert list(a[:7]) == list(b[:7]) and a[-1] == b[-1]
