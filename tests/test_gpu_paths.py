"""Path extraction (cpd_query_paths / Index.paths): the node sequence of every
table-search walk, bit-exact against a lock-step numpy walk over the oracle's
rows.  The numpy walk (ref_paths) restates the oracle's ora_table_search and is
itself pinned against it in every test (pinned): path length, end node and the
cost along the path's edges."""
import functools

import numpy as np
import pytest

import cpd
import oracle
from graphs import GRAPHS, graph_from_edges

pytestmark = pytest.mark.gpu


def ref_paths(g, order, targets, off, runs, s, t, w_sel=None, k_moves=-1):
    """All walks at once: (offsets, nodes, cost, hops, fin).  mv = the row's
    move at the current node's column; a walk stops at t, after `limit` moves
    or at a move naming no out-edge."""
    n = g.n
    w_sel = g.w if w_sel is None else w_sel
    mv4 = oracle.moves_from_runs(off, runs, n, 4)
    table = ((mv4[:, :, None] >> (4 * np.arange(8, dtype=np.uint32))) & 0xF)
    table = table.reshape(len(targets), -1)[:, :n].astype(np.int64)
    row_of = np.full(n, -1, np.int64)
    row_of[targets] = np.arange(len(targets))
    s, t = np.asarray(s, np.int64), np.asarray(t, np.int64)
    row = row_of[t]
    assert (row >= 0).all()
    rp, dst = g.row_ptr.astype(np.int64), g.dst.astype(np.int64)
    outdeg = np.diff(rp)
    order = order.astype(np.int64)
    limit = n if k_moves < 0 else min(k_moves, n)
    nq = len(s)
    cur = s.copy()
    hops = np.zeros(nq, np.int64)
    cost = np.zeros(nq, np.uint64)
    idx = np.arange(nq)
    steps = []
    h = 0
    while len(idx):
        c = cur[idx]
        mv = table[row[idx], order[c]]
        go = (c != t[idx]) & (h < limit) & (mv < outdeg[c])
        idx, c, mv = idx[go], c[go], mv[go]
        e = rp[c] + mv
        cur[idx] = dst[e]
        cost[idx] += w_sel[e].astype(np.uint64)
        h += 1
        hops[idx] = h
        steps.append((idx, dst[e]))
    offsets = np.concatenate(([0], np.cumsum(hops + 1))).astype(np.uint64)
    nodes = np.empty(int(offsets[-1]), np.uint32)
    base = offsets[:-1].astype(np.int64)
    nodes[base] = s
    for k, (ix, v) in enumerate(steps):
        nodes[base[ix] + k + 1] = v
    return offsets, nodes, cost, hops.astype(np.uint32), (cur == t).astype(np.uint8)


def pinned(ref, g, order, targets, off, runs, s, t, w_sel=None, k_moves=-1):
    """ref_paths' result against oracle.table_search; returns the oracle's
    (cost, hops, fin)."""
    offsets, nodes, cost, hops, fin = ref
    w_sel = g.w if w_sel is None else w_sel
    rc, rh, rf = oracle.table_search(g.row_ptr, g.dst, w_sel, order, targets, off, runs, s, t,
                                     k_moves=k_moves)
    np.testing.assert_array_equal(np.diff(offsets.astype(np.int64)) - 1, rh)   # len - 1 == hops
    last = nodes[offsets[1:].astype(np.int64) - 1]
    np.testing.assert_array_equal(last == t, rf == 1)                   # ends at t iff finished
    np.testing.assert_array_equal(cost, rc)                             # w_sel along the path
    np.testing.assert_array_equal(hops, rh)
    np.testing.assert_array_equal(fin, rf)
    return rc, rh, rf


def check_paths(out, ref, s, orc):
    offsets, nodes, cost, hops, fin, st = out
    rc, rh, rf = orc
    assert offsets.dtype == np.uint64 and nodes.dtype == np.uint32
    np.testing.assert_array_equal(
        offsets, np.concatenate(([0], np.cumsum(rh.astype(np.uint64) + 1))).astype(np.uint64))
    np.testing.assert_array_equal(offsets, ref[0])
    np.testing.assert_array_equal(nodes, ref[1])
    np.testing.assert_array_equal(nodes[offsets[:-1].astype(np.int64)], s)
    np.testing.assert_array_equal(cost, rc)
    np.testing.assert_array_equal(hops, rh)
    np.testing.assert_array_equal(fin, rf)
    assert st["queries"] == len(s)
    assert st["hops"] == int(rh.sum()) and st["finished"] == int(rf.sum())
    assert st["cost"] == int(rc.sum())


@functools.lru_cache(maxsize=None)
def world(name, ntargets=50):
    """Graph, plan, device graph, ntargets target rows built on the GPU and the
    oracle's rows for them (shared by the tests; never changed)."""
    g = GRAPHS[name]()
    plan = cpd.Plan(g)
    dev = cpd.Graph(plan, batch=1024)
    rng = np.random.default_rng(2)
    targets = rng.choice(g.n, size=min(g.n, ntargets), replace=False).astype(np.uint32)
    rows = dev.build_rows(targets)
    order = plan.order()
    off, runs = oracle.build_rows(g.row_ptr, g.dst, g.w, order, targets)
    return g, plan, dev, targets, rows, order, off, runs


def draw(g, targets, nq, seed):
    rng = np.random.default_rng(seed)
    if g.n == 1:  # single: the one pair there is
        return np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    s = rng.integers(0, g.n, nq).astype(np.uint32)
    return s, targets[rng.integers(0, len(targets), nq)]


@pytest.mark.parametrize("mode", ["rle", "dense"])
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_paths_bit_exact(graph, mode):
    g, plan, dev, targets, rows, order, off, runs = world(graph)
    ix = cpd.Index(dev, rows=rows)
    ix.set_mode(mode)
    assert ix.mode == mode
    s, t = draw(g, targets, 4000, seed=3)
    ref = ref_paths(g, order, targets, off, runs, s, t)
    orc = pinned(ref, g, order, targets, off, runs, s, t)
    out = ix.paths(s, t)
    check_paths(out, ref, s, orc)
    if graph == "irregular":  # the unfinished walks are there
        assert 0 < int(orc[2].sum()) < len(s)
    if graph == "single":
        assert out[0].tolist() == [0, 1] and out[1].tolist() == [0]
    # the empty batch
    e = ix.paths(np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    assert e[0].tolist() == [0] and len(e[1]) == 0 and e[5]["queries"] == 0


@pytest.mark.parametrize("mode", ["rle", "dense"])
def test_paths_k_moves(mode):
    g, plan, dev, targets, rows, order, off, runs = world("synth")
    ix = cpd.Index(dev, rows=rows)
    ix.set_mode(mode)
    s, t = draw(g, targets, 4000, seed=4)
    full = ix.paths(s, t)
    fo, fn = full[0].astype(np.int64), full[1]
    flen = np.diff(fo)
    for k in (0, 1, 3):
        ref = ref_paths(g, order, targets, off, runs, s, t, k_moves=k)
        orc = pinned(ref, g, order, targets, off, runs, s, t, k_moves=k)
        out = ix.paths(s, t, k_moves=k)
        check_paths(out, ref, s, orc)
        ko, kn = out[0].astype(np.int64), out[1]
        klen = np.diff(ko)
        np.testing.assert_array_equal(klen, np.minimum(k, flen - 1) + 1)
        # each a prefix of the whole path
        src = np.repeat(fo[:-1] - ko[:-1], klen) + np.arange(len(kn))
        np.testing.assert_array_equal(kn, fn[src])
        if k == 0:
            np.testing.assert_array_equal(kn, s)


def one_way_ring(n=300):
    """Every out-degree is 1: a 1-slot adjacency (shift 0) and 1-bit tables."""
    rng = np.random.default_rng(13)
    return graph_from_edges(n, [(a, (a + 1) % n, int(rng.integers(1, 6))) for a in range(n)])


def test_paths_out_degree_one():
    g = one_way_ring()
    plan = cpd.Plan(g, hierarchy=False)
    dev = cpd.Graph(plan)
    assert dev.move_bits() == 1
    order = plan.order()
    rng = np.random.default_rng(5)
    targets = rng.choice(g.n, size=40, replace=False).astype(np.uint32)
    off, runs = oracle.build_rows(g.row_ptr, g.dst, g.w, order, targets)
    s, t = draw(g, targets, 3000, seed=6)
    ref = ref_paths(g, order, targets, off, runs, s, t)
    orc = pinned(ref, g, order, targets, off, runs, s, t)
    assert int(orc[2].sum()) == len(s) and int(orc[1].max()) > 250
    for mode in ("rle", "dense"):
        ix = cpd.Index(dev, row_targets=targets, offsets=off, runs=runs)
        ix.set_mode(mode)
        # the precondition: the existing walk at this width equals the oracle
        cost, hops, fin, _ = ix.query(s, t)
        np.testing.assert_array_equal(cost, orc[0])
        np.testing.assert_array_equal(hops, orc[1])
        np.testing.assert_array_equal(fin, orc[2])
        check_paths(ix.paths(s, t), ref, s, orc)


# the walk's launch constants (kDenseWaves, kRleWaves in cpd_kernels.hip), which
# the fill kernel shares: past 64 queries per wave a wave's lanes are refilled
@pytest.mark.parametrize("mode,nq", [("dense", 64 * 1024 + 4096), ("rle", 64 * 8192 + 4096)])
def test_paths_lane_refill(mode, nq):
    g, plan, dev, targets, rows, order, off, runs = world("synth", 1200)
    assert len(targets) == g.n == 1200
    ix = cpd.Index(dev, rows=rows)
    ix.set_mode(mode)
    s, t = draw(g, targets, nq, seed=7)
    ref = ref_paths(g, order, targets, off, runs, s, t)
    orc = pinned(ref, g, order, targets, off, runs, s, t)
    check_paths(ix.paths(s, t), ref, s, orc)


def test_paths_weights_and_forms():
    g, plan, dev, targets, rows, order, off, runs = world("synth")
    s, t = draw(g, targets, 4000, seed=8)
    ref = ref_paths(g, order, targets, off, runs, s, t)
    orc = pinned(ref, g, order, targets, off, runs, s, t)
    wc = cpd.synth_congestion(g.w, frac=0.3, lo=1.0, hi=3.0, seed=3)
    refc = ref_paths(g, order, targets, off, runs, s, t, w_sel=wc)
    orcc = pinned(refc, g, order, targets, off, runs, s, t, w_sel=wc)
    np.testing.assert_array_equal(refc[1], ref[1])
    assert np.any(orcc[0] != orc[0])
    bits = dev.move_bits()
    forms = []
    for mode in ("rle", "dense"):
        forms.append((f"rows-{mode}", cpd.Index(dev, rows=rows), mode))
        forms.append((f"host-{mode}", cpd.Index(dev, row_targets=targets, offsets=off, runs=runs),
                      mode))
        for b in (bits, 4):  # streamed at the packed width and at 4 bits
            ix = cpd.Index.streamed(dev, targets, int(off[-1]), mode=mode)
            ix.append_moves(oracle.moves_from_runs(off, runs, g.n, b), b)
            forms.append((f"moves{b}-{mode}", ix, None))
    for name, ix, mode in forms:
        if mode:
            ix.set_mode(mode)
        check_paths(ix.paths(s, t), ref, s, orc)
        ix.set_weights(wc)   # the nodes stay, the cost follows the weights
        check_paths(ix.paths(s, t), refc, s, orcc)
        ix.set_weights(None)
        check_paths(ix.paths(s, t), ref, s, orc)


def test_paths_fetch_ranges_and_errors():
    g, plan, dev, targets, rows, order, off, runs = world("synth")
    ix = cpd.Index(dev, rows=rows)
    s, t = draw(g, targets, 1000, seed=9)
    ref = ref_paths(g, order, targets, off, runs, s, t)
    orc = pinned(ref, g, order, targets, off, runs, s, t)
    check_paths(ix.paths(s, t), ref, s, orc)
    # an uneven partition of the batch, empty pieces included
    cuts = [0, 0, 1, 7, 7, 300, 301, 999, 1000, 1000]
    pieces = [ix.paths_fetch(a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    assert [len(p) for p in pieces] == [int(ref[0][b] - ref[0][a])
                                        for a, b in zip(cuts[:-1], cuts[1:])]
    np.testing.assert_array_equal(np.concatenate(pieces), ref[1])

    def again():
        check_paths(ix.paths(s, t), ref, s, orc)

    for first, count in [(1000, 1), (990, 11), (0xFFFFFFFF, 2)]:  # past nq
        with pytest.raises(cpd.CpdError) as ei:
            ix.paths_fetch(first, count)
        assert ei.value.code == cpd.CPD_E_ARG
    again()
    ix.prepare(s, t)  # a fresh batch: its paths have not been walked
    with pytest.raises(cpd.CpdError) as ei:
        ix.paths_fetch(0, 1)
    assert ei.value.code == cpd.CPD_E_ARG
    ix.run()
    with pytest.raises(cpd.CpdError) as ei:
        ix.paths_fetch(0, 0)
    assert ei.value.code == cpd.CPD_E_ARG
    again()
    norow = np.setdiff1d(np.arange(g.n, dtype=np.uint32), targets)[:1]
    with pytest.raises(cpd.CpdError) as ei:
        ix.paths(s[:1], norow)
    assert ei.value.code == cpd.CPD_E_NOROW
    with pytest.raises(cpd.CpdError) as ei:  # the failed prepare left no batch
        ix.paths_fetch(0, 1)
    assert ei.value.code == cpd.CPD_E_ARG
    again()


@pytest.mark.parametrize("mode", ["rle", "dense"])
def test_paths_does_not_disturb_query(mode):
    g, plan, dev, targets, rows, order, off, runs = world("synth")
    ix = cpd.Index(dev, rows=rows)
    ix.set_mode(mode)
    s, t = draw(g, targets, 2000, seed=10)
    ref = ref_paths(g, order, targets, off, runs, s, t)
    orc = pinned(ref, g, order, targets, off, runs, s, t)
    before = ix.query(s, t)
    check_paths(ix.paths(s, t), ref, s, orc)
    after = ix.query(s, t)
    for a, b, c in zip(before[:3], after[:3], orc):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)
    assert {k: v for k, v in before[3].items() if k != "kernel_ms"} == \
           {k: v for k, v in after[3].items() if k != "kernel_ms"}
    # after a search on other weights, paths() is still the table-search walk
    wc = cpd.synth_congestion(g.w, frac=0.3, lo=1.0, hi=3.0, seed=3)
    ix.set_weights(wc)
    ix.search(s[:200], t[:200])
    off2, _ = ix.paths_run()  # on the very batch the search prepared
    np.testing.assert_array_equal(off2, ref[0][:201])
    np.testing.assert_array_equal(ix.paths_fetch(0, 200), ref[1][:int(ref[0][200])])
    ix.set_weights(None)
    check_paths(ix.paths(s, t), ref, s, orc)
