"""GPU: foreign rows (tests/foreign_rows.py — perturbed moves, inserted runs, a
random row, a single-run row; pinned by test_foreign_rows_cpu.py) through every
walk family, each compared exactly with the reference its own test file uses:
walks that finish by a longer route, stop at a move naming no edge, run into
the n-move guard on a cycle they start on or reach from a tail, and searches
whose heuristic is inexact or INF.  Rows built from exact shortest paths reach
almost none of that."""
import functools

import numpy as np
import pytest

import costs_ref
import cpd
import foreign_rows as F
import loads_ref
import oracle
import timed_ref
from graphs import graph_from_edges
from search_loads_ref import ref_search_loads
from search_paths_ref import flatten
from test_gpu_loads import fetch
from test_gpu_paths import check_paths, ref_paths

pytestmark = pytest.mark.gpu

MODES = ["dense", "rle"]
K = F.K_MOVES


@functools.lru_cache(maxsize=None)
def env(name, mode, wide=True):
    """(world, device graph): a dense index takes the moves its tables hold; an
    RLE index moves up to WIDE_MOVE on the graphs whose tables are narrower —
    for the table-search walks (wide), which read the runs (deg8 and irregular
    have 4-bit tables: both modes get moves up to 15, which names no edge).  The searches read
    the dense tables whatever the mode: they get the moves those hold."""
    w = F.world(name)
    if mode == "rle" and wide and w.max_move < F.WIDE_MOVE:
        w = F.world(name, F.WIDE_MOVE)
    return w, cpd.Graph(w.plan, batch=1024)


def index(name, mode, wide=True):
    w, dev = env(name, mode, wide)
    if mode == "dense" or not wide:
        assert w.max_move == (1 << dev.move_bits()) - 1
    ix = cpd.Index.streamed(dev, w.targets, int(w.off[-1]), mode=mode)
    half = len(w.targets) // 2          # two appends
    ix.append(w.off[:half + 1], w.runs[:int(w.off[half])])
    ix.append(w.off[half:] - w.off[half], w.runs[int(w.off[half]):])
    assert ix.mode == mode
    return w, ix


def rows_of(w):
    return w.g, w.order, w.targets, w.off, w.runs


def same(got, want, msg=""):
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b, err_msg=msg)


@functools.lru_cache(maxsize=None)
def search_ref(name, max_move, weights, key):
    """ref_search_loads of the world's queries, unit demand: (cost, plen, fin,
    counters, path offsets, path nodes, loads, moves, prefix moves)."""
    w = F.world(name, max_move)
    r = ref_search_loads(w.ref, w.wc if weights == "congested" else w.wl, w.s, w.t, **dict(key))
    return r[:4] + flatten(r[4]) + r[6:]


def opt_key(opts):
    return tuple(sorted(opts.items()))


world_mode = pytest.mark.parametrize("mode", MODES)
world_name = pytest.mark.parametrize("name", list(F.WORLDS))


@world_mode
@world_name
def test_query(name, mode):
    """No cut-off, k_moves = 0, and the k_moves that cuts the walks of K + 1."""
    w, ix = index(name, mode)
    for w_sel in (None, w.wc):
        ix.set_weights(w_sel)
        for k in (-1, 0, K):
            rc, rh, rf = F.table_search(w, w_sel, k_moves=k)
            c, h, f, st = ix.query(w.s, w.t, k_moves=k)
            same((c, h, f), (rc, rh, rf), f"k_moves={k}")
            assert st["hops"] == int(rh.sum()) and st["finished"] == int(rf.sum())
    qc = F.query_classes(w)
    _, h, f, _ = ix.query(w.s, w.t, k_moves=K)
    assert np.all(h[qc["k_plus_1"]] == K) and not f[qc["k_plus_1"]].any()
    assert np.all(h[qc["k_exact"]] == K) and f[qc["k_exact"]].all()


@world_name
@world_mode
def test_append_moves(name, mode):
    """The same rows loaded in the compact form (oracle.moves_from_runs), at
    the tables' width and as nibbles (one and the same on deg8 and irregular),
    on every adjacency width."""
    w, dev = env(name, "dense")
    rc, rh, rf = F.table_search(w)
    sc = F.cpd_search(w, w.wc)
    for bits in sorted({dev.move_bits(), 4}):
        ix = cpd.Index.streamed(dev, w.targets, int(w.off[-1]), mode=mode)
        ix.append_moves(oracle.moves_from_runs(w.off, w.runs, w.g.n, bits), bits)
        same(ix.query(w.s, w.t)[:3], (rc, rh, rf), f"{bits}-bit moves")
        ix.set_weights(w.wc)
        c, p, f, cnt, _ = ix.search(w.s, w.t)
        same((c, p, f, cnt.astype(np.uint64)), sc, f"{bits}-bit moves, search")


@world_mode
@world_name
def test_paths(name, mode):
    """Node sequences, full and k_moves-limited: an unfinished walk's path is
    its hops + 1 nodes from s to where it stopped (cpd_api.h)."""
    w, ix = index(name, mode)
    g = w.g
    for k in (-1, K):
        ref = ref_paths(*rows_of(w), w.s, w.t, k_moves=k)
        orc = F.table_search(w, k_moves=k)
        same(ref[2:], orc)
        out = ix.paths(w.s, w.t, k_moves=k)
        check_paths(out, ref, w.s, orc)
        off, nodes, fin = out[0].astype(np.int64), out[1], out[4]
        last = nodes[off[1:] - 1]
        assert np.all((last == w.t) == (fin == 1))
        # every step of every path, finished or not, is an edge of the graph
        inner = np.ones(len(nodes), bool)
        inner[off[1:] - 1] = False
        a, b = nodes[inner], nodes[1:][inner[:-1]]
        edges = set(zip(np.repeat(np.arange(g.n), np.diff(g.row_ptr.astype(np.int64))).tolist(),
                        g.dst.tolist()))
        assert all(e in edges for e in set(zip(a.tolist(), b.tolist())))
    qc = F.query_classes(w)
    full = ix.paths(w.s, w.t)
    n1 = np.diff(full[0].astype(np.int64))
    assert np.all(n1[qc["cycle_on"] | qc["cycle_tail"]] == g.n + 1)   # the guard: n moves


@world_mode
@world_name
def test_costs(name, mode):
    """All sets at once with 1, 4, 5 and 8 sets and the sliced mode; one set
    is all zeros, so cycles of no cost are met."""
    w, ix = index(name, mode)
    g = w.g
    rng = np.random.default_rng(3)
    zero = np.zeros(g.m, np.uint32)
    sets = [w.wc, zero, None, w.wl] + [rng.integers(0, 1 << 20, g.m).astype(np.uint32)
                                       for _ in range(4)]
    for n_sets in (1, 4, 5, 8):
        ix.set_weight_sets(sets[:n_sets])
        for k in (-1, K):
            want = costs_ref.ref_all(*rows_of(w), w.s, w.t, sets[:n_sets], k_moves=k)
            got = ix.costs(w.s, w.t, k_moves=k)
            same(got[:3], want, f"{n_sets} sets, k_moves={k}")
    qc = F.query_classes(w)
    ix.set_weight_sets(sets[:5])
    full = ix.costs(w.s, w.t)[0]
    assert not full[qc["cycle_on"] | qc["cycle_tail"], 1].any()   # the zero set over a cycle
    for S in (2, 5):
        for k in (-1, K):
            want = costs_ref.ref_sliced(*rows_of(w), w.s, w.t, sets[:5], S, k_moves=k)
            got = ix.costs(w.s, w.t, k_moves=k, slice_moves=S)
            same(got[:3], want, f"slice_moves={S}, k_moves={k}")


@world_mode
@world_name
def test_loads(name, mode):
    """Unit demand and a demand array, 1 and 3 slices, a second batch added to
    the first; the walk's finished and hop results beside the table."""
    w, ix = index(name, mode)
    ix.set_weights(w.wc)
    nq = len(w.s)
    dem = np.random.default_rng(4).integers(0, 1 << 32, nq, dtype=np.uint64).astype(np.uint32)
    cut = nq // 3
    for slices, S in ((1, 0), (3, 4)):
        for demand in (None, dem):
            for k in (-1, K):
                msg = f"slices={slices} demand={demand is not None} k_moves={k}"
                want, rh, rf = loads_ref.walk_loads(*rows_of(w), w.s, w.t, demand, K=slices, S=S,
                                                    k_moves=k)
                rc = F.table_search(w, w.wc, k_moves=k)[0]
                got, st = ix.loads(w.s, w.t, demand, k_moves=k, slices=slices, slice_moves=S)
                np.testing.assert_array_equal(got, want, err_msg=msg)
                same(fetch(ix, nq), (rc, rh, rf), msg)
                assert st["hops"] == int(rh.sum()) and st["finished"] == int(rf.sum())
        first = loads_ref.walk_loads(*rows_of(w), w.s[:cut], w.t[:cut], dem[:cut], K=slices, S=S)[0]
        ix.loads_clear()
        a, _ = ix.loads(w.s[:cut], w.t[:cut], dem[:cut], slices=slices, slice_moves=S,
                        accumulate=True)
        np.testing.assert_array_equal(a, first)
        b, _ = ix.loads(w.s[cut:], w.t[cut:], dem[cut:], slices=slices, slice_moves=S,
                        accumulate=True)
        whole = loads_ref.walk_loads(*rows_of(w), w.s, w.t, dem, K=slices, S=S)[0]
        np.testing.assert_array_equal(b, whole)


@world_mode
@world_name
def test_timed(name, mode):
    """The shortest period there is (1: every move of positive weight crosses a
    period edge) and one longer than any walk, with and without the load
    table, departures on both sides of a period edge."""
    w, ix = index(name, mode)
    g = w.g
    rng = np.random.default_rng(5)
    sets = [w.wc, w.wl, None]
    ix.set_weight_sets(sets)
    nq = len(w.s)
    dem = rng.integers(0, 1 << 32, nq, dtype=np.uint64).astype(np.uint32)
    longest = int(np.stack(costs_ref.weights_of(g, sets)).max()) * (g.n + 1)
    for P in (1, longest + 1):
        assert P == 1 or P > longest
        dep = (P - 1 + rng.integers(-min(P - 1, 3), 4, nq)).astype(np.uint64)   # around t = P
        assert np.any(dep < P) and np.any(dep >= P)
        for k in (-1, K):
            msg = f"period {P} k_moves={k}"
            want = timed_ref.walk_timed(*rows_of(w), w.s, w.t, sets, dep, P, dem, k_moves=k)
            same(ix.timed(w.s, w.t, dep, P, k_moves=k)[:3], want[:3], msg)
            ix.loads_clear()
            same(ix.timed(w.s, w.t, dep, P, dem, k_moves=k, loads=True)[:3], want[:3], msg)
            np.testing.assert_array_equal(ix.loads_fetch(), want[3], err_msg=msg)


def check_search(got, want, msg):
    cost, plen, fin, cnt, st = got
    same((cost, plen, fin, cnt.astype(np.uint64)), want[:4], msg)
    assert st["overflow"] == 0 and st["expanded"] == int(want[3][:, 0].sum()), msg
    assert st["finished"] == int(want[2].sum()), msg


@pytest.mark.parametrize("weights", ["congested", "below"])
@world_mode
@world_name
def test_search(name, mode, weights):
    """Both forms of the CPD path values over the option sets of the CPU test:
    the oracle's cost, plen, finished and five counters, and each other's."""
    w, ix = index(name, mode, wide=False)
    w_sel = w.wc if weights == "congested" else w.wl
    ix.set_weights(w_sel)
    for opts, oid in zip(F.SEARCH_OPTS, F.SEARCH_IDS):
        want = F.cpd_search(w, w_sel, **opts)
        got = {}
        for form in ("tables", "walks"):
            got[form] = ix.search(w.s, w.t, tables=form, **opts)
            assert got[form][4]["tables"] == cpd.SEARCH_FORMS[form]
            check_search(got[form], want, f"{form} {oid}")
        same(got["tables"][:4], got["walks"][:4], oid)
    # a source whose own walk is INF is never inserted: nothing expands
    qc = F.query_classes(w)
    m = qc["no_edge"] | qc["cycle_on"] | qc["cycle_tail"]
    for form in ("tables", "walks"):
        _, _, fin, cnt, _ = ix.search(w.s, w.t, tables=form)
        assert not fin[m].any() and not cnt[m].any(), form


@pytest.mark.parametrize("name", ["ring2", "synth"])
def test_search_refuses_moves_wider_than_tables(name):
    """An RLE index holds moves the graph's dense tables cannot; the searches
    read those tables and refuse such rows (never truncate them) — and the
    table-search walks over the runs still answer."""
    w, ix = index(name, "rle")
    assert int((w.runs & 0xF).max()) > (1 << env(name, "rle")[1].move_bits()) - 1
    for form in ("tables", "walks"):
        with pytest.raises(cpd.CpdError) as ei:
            ix.search(w.s, w.t, tables=form)
        assert ei.value.code == cpd.CPD_E_ARG and "moves <" in str(ei.value)
    same(ix.query(w.s, w.t)[:3], F.table_search(w))


@pytest.mark.parametrize("form", ["tables", "walks"])
@world_mode
@world_name
def test_search_spilled(name, mode, form):
    """capacity 64 growing to 4096: searches over rows full of INF values are
    spilled and resumed, with the oracle's results."""
    w, ix = index(name, mode, wide=False)
    ix.set_weights(w.wc)
    opts = dict(hscale=0.5, fscale=0.1)         # the widest searches of the option sets
    want = F.cpd_search(w, w.wc, **opts)
    got = ix.search(w.s, w.t, tables=form, capacity=64, capacity_max=4096, **opts)
    check_search(got, want, form)
    assert want[3][:, 1].max() > 64         # some search inserts more than the first capacity
    assert got[4]["reruns"] > 0


@world_mode
@world_name
def test_search_paths_and_loads(name, mode):
    """search_paths node for node and search_loads table for table (unit demand
    and a demand array) on the option sets, both forms, both weightings."""
    w, ix = index(name, mode, wide=False)
    nq = len(w.s)
    dem = np.random.default_rng(6).integers(0, 1 << 32, nq, dtype=np.uint64).astype(np.uint32)
    for weights, w_sel in (("congested", w.wc), ("below", w.wl)):
        ix.set_weights(w_sel)
        for opts, oid in zip(F.SEARCH_OPTS, F.SEARCH_IDS):
            rc, rp, rf, rs, roff, rnodes, rloads, rmoves, rprefix = search_ref(
                name, w.max_move, weights, opt_key(opts))
            for form in ("tables", "walks"):
                msg = f"{weights} {oid} {form}"
                off, nodes, c, p, f, cnt, st = ix.search_paths(w.s, w.t, tables=form, **opts)
                same((c, p, f, cnt.astype(np.uint64), off, nodes), (rc, rp, rf, rs, roff, rnodes),
                     msg)
                assert st["paths"]["nodes"] == int(roff[-1]), msg
                loads, c, p, f, cnt, st = ix.search_loads(w.s, w.t, tables=form, **opts)
                same((c, p, f, cnt.astype(np.uint64), loads[0]), (rc, rp, rf, rs, rloads), msg)
                assert (st["loads"]["moves"], st["loads"]["prefix_moves"]) == (rmoves, rprefix), msg
            # a demand array: the route of query q carries dem[q]
            r = ref_search_loads(w.ref, w_sel, w.s, w.t, dem, **opts)
            for form in ("tables", "walks"):
                loads = ix.search_loads(w.s, w.t, dem, tables=form, **opts)[0]
                np.testing.assert_array_equal(loads[0], r[6],
                                              err_msg=f"{weights} {oid} {form} demand")


@pytest.mark.parametrize("n", [1023, 1024, 1025, 1026])
def test_jump_table_depth(n):
    """A one-way path of n nodes and the row of its far end: the tables of the
    `tables` form are built in log2(n) + 1 doubling rounds, and the walk of
    n - 1 moves from the near end must come out finite."""
    rng = np.random.default_rng(n)
    g = graph_from_edges(n, [(v, v + 1, int(rng.integers(1, 4))) for v in range(n - 1)])
    plan = cpd.Plan(g)
    order = plan.order()
    dev = cpd.Graph(plan, batch=1024)
    targets = np.array([n - 1], np.uint32)
    off, runs = oracle.build_rows(g.row_ptr, g.dst, g.w, order, targets)
    wc = (g.w * rng.integers(1, 4, g.m)).astype(np.uint32)
    s = np.array([0, 1, 2, n - 2, n - 1], np.uint32)
    t = np.full(len(s), n - 1, np.uint32)
    for mode in MODES:
        ix = cpd.Index.streamed(dev, targets, int(off[-1]), mode=mode)
        ix.append(off, runs)
        ix.set_weights(wc)
        want = oracle.cpd_search(g.row_ptr, g.dst, g.w, wc, order, targets, off, runs, s, t)
        assert want[2].all() and want[1].tolist() == [n - 1, n - 2, n - 3, 1, 0]
        assert int(want[0][0]) == int(wc.sum())
        for form in ("tables", "walks"):
            got = ix.search(s, t, tables=form)
            check_search(got, want, f"{mode} {form}")
        same(ix.query(s, t)[:3], oracle.table_search(g.row_ptr, g.dst, wc, order, targets, off,
                                                     runs, s, t))
