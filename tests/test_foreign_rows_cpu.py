"""CPU: the foreign rows of tests/foreign_rows.py and the references that
tests/test_gpu_foreign_rows.py compares the kernels with, pinned on those rows
before any kernel is looked at: every walk class has members on every world,
the two search references agree, and the lock-step walk references agree with
the oracle's walk."""
import numpy as np
import pytest

import costs_ref
import foreign_rows as F
import loads_ref
import timed_ref
from search_loads_ref import ref_search_loads
from search_paths_ref import ref_search_paths

# (world, max_move): the tables' own field, and for the narrow tables also the
# moves only an RLE index can hold
CASES = [(n, None) for n in F.WORLDS] + [("ring2", F.WIDE_MOVE), ("synth", F.WIDE_MOVE)]
IDS = [f"{n}-{'table' if m is None else 'wide'}" for n, m in CASES]


@pytest.mark.parametrize("name,max_move", CASES, ids=IDS)
def test_class_coverage(name, max_move):
    """Every class of foreign_rows.classify has members among the pairs and the
    queries; the references alone finish >= 60 % of the queries, leave >= 5 %
    unfinished, and >= 5 % finish on a longer path than the shortest.

    The shares started at 0.02 .. 0.05 of the runs.  synth and irregular went
    down to 0.01 (at 0.02 fewer than 60 % of the queries finished: on synth
    0.598, on irregular two of three pairs finish before any perturbation);
    ring2's rows hold two or three runs each, so most of its inserted runs
    repeat the run's move (0.9) and its seed is 3 (seed 2: 0.509 finished).
    Queries finished / unfinished / on a longer path, of 3000, with the pairs
    per class (shortest, longer, no_edge, cycle_on, cycle_tail, k_exact,
    k_plus_1) over all 16 rows x n sources:

      ring2      share 0.05  1932 / 1068 / 182   5122    8 1602   82 1170  13  13
      ring2 wide             2093 /  907 / 183   5613    9 1730    8  624  14  14
      synth      share 0.01  2091 /  909 / 295  12549  956 2784  682 2213 159 194
      synth wide             1927 / 1073 / 515   9551 2783 3869  676 2305 160 191
      deg8       share 0.03  2579 /  421 / 588   4753  936  667   18   10 479 150
      irregular  share 0.01  2047 /  953 / 456   1985  366 2193   31  209 201 228

    ring2 has few pairs that finish by a longer route (a node just behind the
    target sent forward round the whole ring): the class's quota of the
    queries draws them repeatedly.
    """
    w = F.world(name, max_move)
    g = w.g
    F.check_format(w.off, w.runs, g.n)
    assert len(w.targets) <= 16 and len(w.s) <= 3000
    moves = w.runs & 0xF
    assert int(moves.max()) <= w.max_move
    if max_move is None:
        assert w.max_move == (1 << F.table_bits(g)) - 1
    cost, hops, fin = F.table_search(w)
    qc = F.query_classes(w)
    pairs = {c: int(m.sum()) for c, m in w.classes.items()}
    nq = len(w.s)
    print(f"\n{name} max_move {w.max_move} share {w.share}: {int(fin.sum())} / "
          f"{nq - int(fin.sum())} / {int(qc['longer'].sum())} of {nq} queries finished / "
          f"unfinished / longer; pairs {pairs}; queries "
          f"{ {c: int(m.sum()) for c, m in qc.items()} }")
    for c in F.CLASSES:
        assert pairs[c] > 0 and qc[c].any(), c
    assert fin.sum() >= 0.60 * nq
    assert (fin == 0).sum() >= 0.05 * nq
    assert qc["longer"].sum() >= 0.05 * nq
    # what the classes say is what the oracle's walk does
    assert np.all(fin[qc["shortest"] | qc["longer"] | qc["k_exact"] | qc["k_plus_1"]] == 1)
    assert np.all(fin[qc["no_edge"] | qc["cycle_on"] | qc["cycle_tail"]] == 0)
    assert np.all(hops[qc["cycle_on"] | qc["cycle_tail"]] == g.n)
    assert np.all(hops[qc["no_edge"]] < g.n)
    assert np.all(hops[qc["k_exact"]] == F.K_MOVES) and np.all(hops[qc["k_plus_1"]] == F.K_MOVES + 1)
    # ... and the cutting k_moves cuts k_plus_1 and leaves k_exact
    _, hk, fk = F.table_search(w, k_moves=F.K_MOVES)
    assert np.all(fk[qc["k_exact"]] == 1) and np.all(fk[qc["k_plus_1"]] == 0)
    assert np.all(hk[qc["k_plus_1"]] == F.K_MOVES)
    # a move naming no edge is there on columns that have edges (not only at degree 0)
    deg = np.diff(g.row_ptr.astype(np.int64))
    stuck = w.s[qc["no_edge"] & (hops == 0)]
    assert np.any(deg[stuck] > 0)
    # the target's own column carries a run whose move names no edge there (or
    # another edge): the walks that finish never read it
    col_t = w.order[w.targets[:-2]].astype(np.int64)
    for r, c in enumerate(col_t):
        rr = w.runs[int(w.off[r]):int(w.off[r + 1])]
        assert c in (rr >> 4).astype(np.int64)


@pytest.mark.parametrize("weights", ["congested", "below"])
@pytest.mark.parametrize("opts", F.SEARCH_OPTS, ids=F.SEARCH_IDS)
@pytest.mark.parametrize("name,max_move", CASES, ids=IDS)
def test_search_references_agree(name, max_move, opts, weights):
    """oracle.cpd_search == ref_search_paths == ref_search_loads on cost, plen,
    finished and the five counters over the foreign rows: inexact heuristics
    (re-opened nodes, stale heap entries), INF heuristics from bad moves and
    cycles, walks cut by k_moves."""
    w = F.world(name, max_move)
    w_sel = w.wc if weights == "congested" else w.wl
    if weights == "below":
        assert np.all(w_sel <= w.g.w) and np.any(w_sel < w.g.w)
    want = F.cpd_search(w, w_sel, **opts)
    got = ref_search_paths(w.ref, w_sel, w.s, w.t, **opts)
    got2 = ref_search_loads(w.ref, w_sel, w.s, w.t, **opts)
    for a, b, c, what in zip(want, got, got2, ("cost", "plen", "finished", "counters")):
        np.testing.assert_array_equal(b, a, err_msg=what)
        np.testing.assert_array_equal(c, a, err_msg=what)
    assert got[4] == got2[4]                                   # the same paths
    np.testing.assert_array_equal(np.array(got[5], np.uint64), want[0])   # costed along their edges
    if weights == "congested" and not opts and name != "ring2":
        assert want[3][:, 3].sum() > 0     # nodes are re-opened: the heuristic is inexact
    if "k_moves" in opts:
        full = F.cpd_search(w, w_sel)
        assert np.any(full[3] != want[3])   # it cuts: searches go on to a node near enough


@pytest.mark.parametrize("name,max_move", CASES, ids=IDS)
def test_walk_references_agree(name, max_move):
    """The hops and finished flags of costs_ref, loads_ref and timed_ref are
    oracle.table_search's on the foreign rows, with and without the cutting
    k_moves; the weights of a walk's loaded edges sum to its cost."""
    w = F.world(name, max_move)
    g = w.g
    args = (g, w.order, w.targets, w.off, w.runs, w.s, w.t)
    dem = np.random.default_rng(1).integers(1, 1000, len(w.s)).astype(np.uint32)
    for k in (-1, F.K_MOVES):
        rc, rh, rf = F.table_search(w, w.wc, k_moves=k)
        c, h, f = costs_ref.walk_costs(*args, [None, w.wc], k_moves=k)
        np.testing.assert_array_equal(c[:, 1], rc)
        np.testing.assert_array_equal(h, rh)
        np.testing.assert_array_equal(f, rf)
        a, h2, f2 = costs_ref.ref_all(*args, [None, w.wc], k_moves=k)
        np.testing.assert_array_equal(a, c)
        ld, h, f = loads_ref.walk_loads(*args, demand=dem, k_moves=k)
        np.testing.assert_array_equal(h, rh)
        np.testing.assert_array_equal(f, rf)
        assert int((ld[0] * w.wc.astype(np.uint64)).sum()) == int((rc * dem).sum())
        assert int(ld.sum()) == int((rh.astype(np.uint64) * dem).sum())
        tc, h, f, tl = timed_ref.walk_timed(*args, [w.wc, w.wc], None, 7, demand=dem, k_moves=k)
        np.testing.assert_array_equal(tc, rc)      # both sets the same: the clock does not matter
        np.testing.assert_array_equal(h, rh)
        np.testing.assert_array_equal(f, rf)
        np.testing.assert_array_equal(tl.sum(axis=0), ld[0])
    # one walk of every class on its own: its loaded edges' weights are its cost
    rc, rh, rf = F.table_search(w, w.wc)
    for cls, m in F.query_classes(w).items():
        q = int(np.flatnonzero(m)[0])
        one = (g, w.order, w.targets, w.off, w.runs, w.s[q:q + 1], w.t[q:q + 1])
        ld, h, f = loads_ref.walk_loads(*one)
        assert int((ld[0] * w.wc.astype(np.uint64)).sum()) == int(rc[q]), cls
        assert int(ld.sum()) == int(rh[q]) == int(h[0]) and int(f[0]) == int(rf[q]), cls
