"""fifo_auto --alg cpd-search --assign K --capacity C driven as the reference
head node drives a worker (tests/driver_harness.py, as
test_gpu_search_loads_driver.py does): every request is answered through
cpd_query_assign at a demand of 1 per query line and a uniform capacity;
<query file>.assign, .loads and .res equal what the library returns in
process, <query file>.diff reads back to its final weights, and the flag
combinations the loop cannot serve are refused at start."""
import os

import numpy as np
import pytest

import cpd
import driver_harness as H
import oracle
from test_gpu_drivers import _read_diff

pytestmark = pytest.mark.gpu
BIN = H.BIN
W, METHOD, KEY = 2, "mod", 3
ITERS, CAP = 3, 2


def test_fifo_auto_assign(tmp_path):
    xy, diff, scen, outdir = H.build_index(tmp_path, W, METHOD, KEY)
    g = cpd.synth_road_graph(30, 24, seed=2)
    wc = _read_diff(diff, g)
    src = np.repeat(np.arange(g.n), np.diff(g.row_ptr.astype(np.int64)))

    # refused at start, exit 2 and one line, no FIFO made
    loop = ["--assign", str(ITERS), "--capacity", str(CAP)]
    for extra in (["--alg", "table-search"] + loop,
                  ["--alg", "cpd-search", "--search-paths"] + loop,
                  ["--alg", "cpd-search", "--search-loads"] + loop,
                  ["--alg", "cpd-search", "--loads"] + loop,
                  ["--alg", "cpd-search", "--timed", "100"] + loop,
                  ["--alg", "cpd-search", "--assign", str(ITERS)],            # no capacity
                  ["--alg", "cpd-search", "--assign", "0", "--capacity", "2"],
                  ["--alg", "cpd-search", "--capacity", "2"],                 # no --assign
                  ["--alg", "cpd-search", "--vdf", "3/20^5"] + loop):
        p = H.refused(xy, diff, outdir, extra, tmp_path, W, METHOD, KEY)
        assert p.returncode == 2, (extra, p.stderr)
        assert len(p.stderr.strip().splitlines()) == 1 and "fifo_auto: --" in p.stderr, extra
        assert not os.path.exists(tmp_path / "never.fifo")

    nfs = str(tmp_path / "nfs")
    os.makedirs(nfs)
    procs = H.serve(xy, diff, outdir, "cpd-search", loop, W, METHOD, KEY)
    try:
        for pr in procs:
            H.wait_ready(pr, timeout=60)
        conf = {"workers": ["localhost"] * W, "nfs": nfs, "partmethod": METHOD, "partkey": KEY,
                "xy_file": xy, "scenfile": scen, "diffs": [diff, diff]}  # the request twice
        parts, stats = H.run(conf, dict(H.DEFAULT_CONFIG, debug=True))
    finally:
        H.quit(procs)
    side = sorted(f for f in os.listdir(nfs) if f.startswith("query."))
    assert side == sorted(f"query.localhost{wid}.{ext}" for wid in range(W)
                          for ext in ("assign", "diff", "loads", "res"))  # no .tmp left
    # every request starts again from its diff: the second answer is the first's
    for a, b in zip(*stats):
        assert list(a[:7]) == list(b[:7])

    plan = cpd.Plan(g)
    dev = cpd.Graph(plan, batch=1024)
    order = plan.order()
    for wid, part in enumerate(parts):
        s = np.array([q[0] for q in part], np.uint32)
        t = np.array([q[1] for q in part], np.uint32)
        targets = np.unique(t)
        off, runs = oracle.build_rows(g.row_ptr, g.dst, g.w, order, targets)
        ix = cpd.Index(dev, row_targets=targets, offsets=off, runs=runs)
        ix.set_weights(wc)
        recs = ix.assign(s, t, np.full(g.m, CAP, np.uint32), ITERS)
        assert recs[1]["sptt"] != recs[0]["sptt"] and recs[0]["changed"] > 50  # a real loop
        name = os.path.join(nfs, f"query.localhost{wid}")
        want = "".join(f"{k + 1} {r['finished']} {r['sptt']} {r['tstt']} {r['moves']} "
                       f"{r['changed']}\n" for k, r in enumerate(recs))
        assert open(name + ".assign").read() == want
        loads = ix.loads_fetch()[0]
        want = [[int(e), int(src[e]), int(g.dst[e]), int(loads[e])] for e in np.nonzero(loads)[0]]
        got = [[int(x) for x in line.split()] for line in open(name + ".loads")]
        assert got == want, wid
        cost, plen, fin, cnt = ix.search_fetch()
        want = "".join(f"{a} {b} {c} {h} {1 if f == 1 else 0}\n" for a, b, c, h, f in
                       zip(s.tolist(), t.tolist(), cost.tolist(), plen.tolist(), fin.tolist()))
        assert open(name + ".res").read() == want
        np.testing.assert_array_equal(_read_diff(name + ".diff", g), ix.get_weights())
        row = stats[0][wid]
        assert [int(x) for x in row[:5]] == cnt.astype(np.uint64).sum(0).tolist()
        assert int(row[5]) == int(plen[fin == 1].sum()) and int(row[6]) == int((fin == 1).sum())
