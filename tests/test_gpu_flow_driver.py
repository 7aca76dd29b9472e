"""fifo_auto --alg cpd-search --assign K --capacity C --step line driven as the
reference head node drives a worker (tests/driver_harness.py, as
test_gpu_assign_driver.py does): every request is answered through
cpd_query_assign_line; <query file>.assign, .loads and .diff equal what
tests/flow_ref.py computes under the request's diff, and --step msa writes
byte for byte what a run without --step writes."""
import os

import numpy as np

import pytest

import cpd
import driver_harness as H
import oracle
from assign_ref import BPR
from flow_ref import ref_assign_line
from search_paths_ref import SearchPathsRef
from test_gpu_drivers import _read_diff

pytestmark = pytest.mark.gpu
BIN = H.BIN
W, METHOD, KEY = 2, "mod", 3
ITERS, CAP = 3, 2
EXTS = ("assign", "diff", "loads", "res")


def _round(tmp_path, name, xy, diff, scen, outdir, extra):
    """One serving session answering one request; returns (nfs dir, parts)."""
    nfs = str(tmp_path / name)
    os.makedirs(nfs)
    procs = H.serve(xy, diff, outdir, "cpd-search", extra, W, METHOD, KEY)
    try:
        for pr in procs:
            H.wait_ready(pr, timeout=60)
        conf = {"workers": ["localhost"] * W, "nfs": nfs, "partmethod": METHOD, "partkey": KEY,
                "xy_file": xy, "scenfile": scen, "diffs": [diff]}
        parts, _ = H.run(conf, dict(H.DEFAULT_CONFIG, debug=True))
    finally:
        H.quit(procs)
    side = sorted(f for f in os.listdir(nfs) if f.startswith("query."))
    assert side == sorted(f"query.localhost{wid}.{ext}" for wid in range(W) for ext in EXTS)
    return nfs, parts


def test_fifo_auto_assign_line(tmp_path):
    xy, diff, scen, outdir = H.build_index(tmp_path, W, METHOD, KEY, queries=600)
    g = cpd.synth_road_graph(30, 24, seed=2)
    wc = _read_diff(diff, g)
    src = np.repeat(np.arange(g.n), np.diff(g.row_ptr.astype(np.int64)))
    order = oracle.dfs_preorder(g.row_ptr, g.dst)

    # refused at start, exit 2 and one line, no FIFO made
    loop = ["--assign", str(ITERS), "--capacity", str(CAP)]
    for extra in (["--alg", "cpd-search", "--step", "line"],                  # no --assign
                  ["--alg", "cpd-search", "--step", "msa"],
                  ["--alg", "cpd-search", "--step", "fw"] + loop):
        p = H.refused(xy, diff, outdir, extra, tmp_path, W, METHOD, KEY)
        assert p.returncode == 2, (extra, p.stderr)
        assert len(p.stderr.strip().splitlines()) == 1 and "fifo_auto: --step" in p.stderr, extra
        assert not os.path.exists(tmp_path / "never.fifo")

    nfs, parts = _round(tmp_path, "line", xy, diff, scen, outdir, loop + ["--step", "line"])
    cap = np.full(g.m, CAP, np.uint32)
    for wid, part in enumerate(parts):
        s = np.array([q[0] for q in part], np.uint32)
        t = np.array([q[1] for q in part], np.uint32)
        targets = np.unique(t)
        off, runs = oracle.build_rows(g.row_ptr, g.dst, g.w, order, targets)
        ref = SearchPathsRef(g, order, targets, off, runs)
        recs, X, w, (cost, plen, fin, _), _, _ = ref_assign_line(ref, wc, s, t, None, cap, BPR, ITERS)
        assert len(recs) >= 2 and recs[1]["g0"] < 0 and recs[0]["changed"] > 50  # a real loop
        name = os.path.join(nfs, f"query.localhost{wid}")
        want = "".join(f"{k + 1} {r['finished']} {r['sptt']} {r['tstt']} {r['moves']} "
                       f"{r['changed']} {r['lambda_q16']} {r['g0']} {r['xw0']}\n"
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

    # --step msa is the run without --step, byte for byte
    msa, _ = _round(tmp_path, "msa", xy, diff, scen, outdir, loop + ["--step", "msa"])
    plain, _ = _round(tmp_path, "plain", xy, diff, scen, outdir, loop)
    for wid in range(W):
        for ext in EXTS:
            a = open(os.path.join(msa, f"query.localhost{wid}.{ext}"), "rb").read()
            b = open(os.path.join(plain, f"query.localhost{wid}.{ext}"), "rb").read()
            assert a == b and a, (wid, ext)
        lines = open(os.path.join(msa, f"query.localhost{wid}.assign")).read().splitlines()
        assert len(lines) == ITERS and all(len(ln.split()) == 6 for ln in lines)
