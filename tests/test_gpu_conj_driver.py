"""fifo_auto --alg cpd-search --assign K --capacity C --step conj driven as the
reference head node drives a worker (tests/driver_harness.py, as
test_gpu_flow_driver.py does): every request is answered through
cpd_query_assign_conj; <query file>.assign, .loads and .diff equal what
tests/conj_ref.py computes under the request's diff."""
import os

import numpy as np

import pytest

import cpd
import driver_harness as H
import oracle
from assign_ref import BPR
from conj_ref import ref_assign_conj
from search_paths_ref import SearchPathsRef
from test_gpu_drivers import _read_diff
from test_gpu_flow_driver import BIN, CAP, _round

pytestmark = pytest.mark.gpu
W, METHOD, KEY = 2, "mod", 3
ITERS = 4


def test_fifo_auto_assign_conj(tmp_path):
    xy, diff, scen, outdir = H.build_index(tmp_path, W, METHOD, KEY, queries=600)
    g = cpd.synth_road_graph(30, 24, seed=2)
    wc = _read_diff(diff, g)
    src = np.repeat(np.arange(g.n), np.diff(g.row_ptr.astype(np.int64)))
    order = oracle.dfs_preorder(g.row_ptr, g.dst)

    # --step conj without --assign is refused as the other words are
    p = H.refused(xy, diff, outdir, ["--alg", "cpd-search", "--step", "conj"], tmp_path, W, METHOD,
                  KEY)
    assert p.returncode == 2 and p.stderr.startswith("fifo_auto: --step")
    assert len(p.stderr.strip().splitlines()) == 1 and not os.path.exists(tmp_path / "never.fifo")

    loop = ["--assign", str(ITERS), "--capacity", str(CAP)]
    nfs, parts = _round(tmp_path, "conj", xy, diff, scen, outdir, loop + ["--step", "conj"])
    cap = np.full(g.m, CAP, np.uint32)
    for wid, part in enumerate(parts):
        s = np.array([q[0] for q in part], np.uint32)
        t = np.array([q[1] for q in part], np.uint32)
        targets = np.unique(t)
        off, runs = oracle.build_rows(g.row_ptr, g.dst, g.w, order, targets)
        ref = SearchPathsRef(g, order, targets, off, runs)
        recs, X, S, w, (cost, plen, fin, _), _ = ref_assign_conj(ref, wc, s, t, None, cap, BPR,
                                                                 ITERS)
        assert len(recs) >= 3 and recs[1]["gy"] < 0 and recs[0]["changed"] > 50  # a real loop
        name = os.path.join(nfs, f"query.localhost{wid}")
        want = "".join(f"{k + 1} {r['finished']} {r['sptt']} {r['tstt']} {r['moves']} "
                       f"{r['changed']} {r['lambda_q16']} {r['gy']} {r['xw0']} {r['alpha_q16']}\n"
                       for k, r in enumerate(recs))
        assert open(name + ".assign").read() == want
        vol = [int(x) >> 16 for x in X.tolist()]
        want = [[e, int(src[e]), int(g.dst[e]), v] for e, v in enumerate(vol) if v]
        got = [[int(x) for x in line.split()] for line in open(name + ".loads")]
        assert got == want, wid
        np.testing.assert_array_equal(_read_diff(name + ".diff", g), w)
        want = "".join(f"{a} {b} {c} {h} {1 if f == 1 else 0}\n" for a, b, c, h, f in
                       zip(s.tolist(), t.tolist(), cost.tolist(), plen.tolist(), fin.tolist()))
        assert open(name + ".res").read() == want
