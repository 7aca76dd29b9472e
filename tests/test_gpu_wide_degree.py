"""GPU parity off the out-degree <= 4 path, past one tile and one slab.

A graph with one node of out-degree 5 leaves the 4-bit first-move kernels:
its rows go through rle_scan<8|16> (the only count pass for wide sets),
rle_moves<8|16>, the generic first_moves<8|16,1,*> and the 4-bit move width
of the tables.  The graphs of tests/graphs.py GRAPHS reach those at n <= 400:
one 2048-column tile, one 1024-target slab.  The graphs here (graphs.WIDE,
their shape pinned by test_oracle_cpu.py) have 4, 5 and 17 tiles, batches of
two slabs, rows of a handful of runs (every run crosses tiles and the 16-tile
chunk seam of rle_moves) and rows of ~17-column runs (past rle_scan's
16-column look-back guess).  Every comparison is exact equality with the
oracle.
"""
import numpy as np
import pytest

import cpd
import oracle
from graphs import WIDE, lattice_wide, wide_targets
from test_gpu_parity import make_graph

pytestmark = pytest.mark.gpu

_REF = {}


def ref(name):
    """(graph, plan, targets, oracle offsets, oracle runs, oracle 4-bit moves)
    of WIDE[name], computed once and never written to."""
    if name not in _REF:
        g = WIDE[name][0]()
        plan = cpd.Plan(g)
        targets = wide_targets(name, g)
        off, runs = oracle.build_rows(g.row_ptr, g.dst, g.w, plan.order(), targets)
        mv = oracle.moves_from_runs(off, runs, g.n, 4)
        for a in (targets, off, runs, mv):
            a.setflags(write=False)
        _REF[name] = (g, plan, targets, off, runs, mv)
    return _REF[name]


def check_rows(rows, off, runs, mv, msg):
    o, r = rows.export()
    np.testing.assert_array_equal(o, off, err_msg=msg)
    np.testing.assert_array_equal(r, runs, err_msg=msg)
    assert rows.move_bits() == 4
    np.testing.assert_array_equal(rows.export_moves(), mv, err_msg=msg)


@pytest.mark.parametrize("xy", [False, True], ids=["cols", "xy"])
@pytest.mark.parametrize("narrow", [True, False], ids=["narrow", "wide"])
@pytest.mark.parametrize("name", ["lattice8", "lattice15"])
def test_rows_many_tiles_two_slabs(name, narrow, xy):
    """4 tiles, batch 2048: a full two-slab batch, then a partial one (452
    targets).  rle_scan / rle_moves<8|16> at t > 0, first_moves<8|16,1,*> at
    slab 1."""
    g, plan, targets, off, runs, mv = ref(name)
    dev = make_graph(plan, 2048, narrow)
    if xy:
        cell = np.arange(g.n, dtype=np.int32)
        dev.set_coords(cell % 80, cell // 80)
    assert dev.move_bits() == 4
    check_rows(dev.build_rows(targets), off, runs, mv, name)
    # one full batch's distances and first-move sets: five targets from each
    # half of the column order (the lanes are sorted by column without
    # coordinates: one half per slab)
    tg = targets[:2048]
    dist, fm = dev.debug_rows(tg)
    by_col = np.argsort(plan.order()[tg], kind="stable")
    for i in np.concatenate([by_col[5:1024:220], by_col[1030::220]]):
        np.testing.assert_array_equal(
            dist[:, i], oracle.reverse_dijkstra(g.row_ptr, g.dst, g.w, tg[i]),
            err_msg=f"{name} dist t={tg[i]}")
        np.testing.assert_array_equal(fm[i], oracle.first_moves(g.row_ptr, g.dst, g.w, tg[i]),
                                      err_msg=f"{name} fm t={tg[i]}")


@pytest.mark.parametrize("name", ["hub8", "hub12", "comb8", "comb15"])
def test_long_and_mixed_runs(name):
    """hub: 17 tiles = two 16-tile chunks of rle_moves; <= 7 runs per row, so
    every run crosses tiles, the chunk to the left looks for its carry right
    of itself and most rows end in a final run that starts before the seam.
    comb: runs of ~17 columns, so rle_scan's 16-column guess is often wrong
    and segments with and without breaks alternate inside a tile."""
    g, plan, targets, off, runs, mv = ref(name)
    dev = cpd.Graph(plan, batch=1024)
    rows = dev.build_rows(targets)
    check_rows(rows, off, runs, mv, name)
    if name.startswith("hub"):
        assert int(rows.export()[0][-1]) < 16 * len(targets)


def test_wide_pool_rows_with_wide_sets():
    """Weights x700 on an 8-bit-set graph: most 256-target group rows spread
    past 0xFFFF and are kept 32-bit in the pool (kWideRow), read by
    first_moves<8,1,true>; the first full batch's probe then switches narrow
    rows off, and the second build runs first_moves<8,1,false>."""
    g0 = lattice_wide(40, 40, 8, seed=8)
    g = cpd.RoadGraph(g0.row_ptr, g0.dst, (g0.w * 700).astype(np.uint32))
    plan = cpd.Plan(g)
    dev = make_graph(plan, 1024, True)
    dev.timing(True)
    targets = np.random.default_rng(12).permutation(g.n).astype(np.uint32)[:1500]
    off, runs = oracle.build_rows(g.row_ptr, g.dst, g.w, plan.order(), targets)
    for rep in range(2):
        dev.timing_reset()
        o, r = dev.build_rows(targets).export()
        np.testing.assert_array_equal(o, off, err_msg=f"build {rep}")
        np.testing.assert_array_equal(r, runs, err_msg=f"build {rep}")
        assert ("group_rows" in dev.timing_get()) == (rep == 0)  # narrow, then switched off
    dev2 = make_graph(plan, 1024, True)
    dist, fm = dev2.debug_rows(targets[:300])
    for i in range(0, 300, 37):
        np.testing.assert_array_equal(
            dist[:, i], oracle.reverse_dijkstra(g.row_ptr, g.dst, g.w, targets[i]))
        np.testing.assert_array_equal(fm[i], oracle.first_moves(g.row_ptr, g.dst, g.w, targets[i]))


def test_wide_rows_several_slabs_four_slot_graph():
    """test_multi_slab_batches runs narrow rows (first_moves_n4); with narrow
    rows off a 4-slot graph takes first_moves<4,2,false>, here over the four
    slabs of a 4096-target batch and a partial second batch."""
    g = cpd.synth_road_graph(90, 90, seed=90)
    plan = cpd.Plan(g)
    dev = make_graph(plan, 4096, False)
    rng = np.random.default_rng(90)
    targets = rng.permutation(g.n).astype(np.uint32)[:4096 + 1500]
    off, runs = dev.build_rows(targets).export()
    ref_off, ref_runs = oracle.build_rows(g.row_ptr, g.dst, g.w, plan.order(), targets)
    np.testing.assert_array_equal(off, ref_off)
    np.testing.assert_array_equal(runs, ref_runs)
    dist, _ = dev.debug_rows(targets[:4096], want_fm=False)
    by_col = np.argsort(plan.order()[targets[:4096]], kind="stable")
    for i in by_col[[3, 1500, 2100, 3100, 4090]]:  # slabs 0, 1, 2, 3, 3
        np.testing.assert_array_equal(
            dist[:, i], oracle.reverse_dijkstra(g.row_ptr, g.dst, g.w, targets[i]))


# ---------------------------------------------------------------------------
# Indexes and walks at the 4-bit move width over many tiles

NQ = 4000
_WALK = {}
_BUILT = {}


def walk_ref(name):
    """Queries over ref(name)'s rows and the oracle's walks: free-flow,
    congested, k_moves = 3."""
    if name not in _WALK:
        g, plan, targets, off, runs, _ = ref(name)
        rng = np.random.default_rng(2)
        s = rng.integers(0, g.n, NQ).astype(np.uint32)
        t = targets[rng.integers(0, len(targets), NQ)]
        wc = cpd.synth_congestion(g.w, frac=0.3, lo=1.0, hi=3.0, seed=3)
        args = (plan.order(), targets, off, runs, s, t)
        _WALK[name] = (s, t, wc,
                       oracle.table_search(g.row_ptr, g.dst, g.w, *args),
                       oracle.table_search(g.row_ptr, g.dst, wc, *args),
                       oracle.table_search(g.row_ptr, g.dst, g.w, *args, k_moves=3))
    return _WALK[name]


def built(name):
    """One device graph per case and its rows (checked by the tests above)."""
    if name not in _BUILT:
        g, plan, targets = ref(name)[:3]
        dev = cpd.Graph(plan, batch=2048 if name.startswith("lattice") else 1024)
        _BUILT[name] = (dev, dev.build_rows(targets))
    return _BUILT[name]


def check_walks(ix, name, msg):
    s, t, wc, free, cong, k3 = walk_ref(name)

    def same(got, want, what):
        cost, hops, fin, st = got
        np.testing.assert_array_equal(cost, want[0], err_msg=f"{msg} {what} cost")
        np.testing.assert_array_equal(hops, want[1], err_msg=f"{msg} {what} hops")
        np.testing.assert_array_equal(fin, want[2], err_msg=f"{msg} {what} finished")
        assert st["cost"] == int(want[0].sum()) and st["hops"] == int(want[1].sum()), what
        assert st["finished"] == int(want[2].sum()) and st["queries"] == NQ, what

    same(ix.query(s, t), free, "free-flow")
    ix.set_weights(wc)
    same(ix.query(s, t), cong, "congested")
    ix.set_weights(None)
    same(ix.query(s, t, k_moves=3), k3, "k_moves=3")


@pytest.mark.parametrize("mode", ["rle", "dense", "auto"])
@pytest.mark.parametrize("name", ["lattice15", "hub12"])
def test_index_from_built_rows(name, mode):
    dev, rows = built(name)
    ix = cpd.Index(dev, rows=rows)
    ix.set_mode(mode)
    assert mode == "auto" or ix.mode == mode
    check_walks(ix, name, f"{name} {mode}")


@pytest.mark.parametrize("name", ["lattice15", "hub12"])
def test_index_from_host_arrays(name):
    g, plan, targets, off, runs, _ = ref(name)
    dev, _ = built(name)
    ix = cpd.Index(dev, row_targets=targets, offsets=off, runs=runs)
    check_walks(ix, name, name)


@pytest.mark.parametrize("mode", ["dense", "rle"])
@pytest.mark.parametrize("name", ["lattice15", "hub12"])
def test_index_streamed_moves_then_runs(name, mode):
    """Half the rows as 4-bit compact rows (validated, and for an RLE index
    turned back into runs by moves_runs), half as runs (validate_rows, and
    for a dense index expand_rows), each across every tile of the row."""
    g, plan, targets, off, runs, mv = ref(name)
    dev, _ = built(name)
    ix = cpd.Index.streamed(dev, targets, int(off[-1]), mode=mode)
    half = len(targets) // 2
    q = half // 2
    ix.append_moves(mv[:q], 4)
    ix.append_moves(mv[q:half], 4)
    three = half + (len(targets) - half) // 2
    for a, b in ((half, three), (three, len(targets))):
        ix.append(off[a:b + 1] - off[a], runs[int(off[a]):int(off[b])])
    info = ix.info()
    assert ix.mode == mode and info["added"] == len(targets)
    if mode == "rle":
        assert info["runs_resident"] == int(off[-1])
    check_walks(ix, name, f"{name} streamed {mode}")
