"""Foreign rows: well-formed index rows that no shortest-path build made — what
`fifo_auto` serves from an index directory and `cpd_index_append` /
`append_moves` take from any producer.  validate_rows checks the format only
(first column 0, strictly increasing columns, every column < n, moves that fit
the table's field); what the moves say is left to the walks.  A helper, not a
test: a fixed seed turns the oracle's rows for a graph into

  perturbed rows   a share of the runs get another move from 0 .. max_move —
                   some a real other edge, some no edge of the column;
  inserted runs    run starts added inside existing runs (columns stay strictly
                   increasing): a stretch of 1 .. 6 columns with another move,
                   or with the same move (two neighbouring runs of one move, a
                   thing the RLE of a build never writes);
  target columns   a run on the target's own column, whose move (max_move, or
                   one past the column's degree) must never be read;
  traps, detours   a cycle of the graph written into a row (entered from its
                   own nodes and from tails), and columns moved to an edge from
                   which the walk still finishes, by a longer route;
  a random row     random starts, random moves;
  a single-run row one run at column 0.

classify() sorts every (source, row) pair by what its walk does, from
oracle.table_search, oracle.reverse_dijkstra and the move edges of
search_paths_ref.SearchPathsRef alone.  tests/test_foreign_rows_cpu.py pins the
classes and the references on these rows; tests/test_gpu_foreign_rows.py puts
them through every walk family."""
import functools

import numpy as np

import cpd
import oracle
from graphs import GRAPHS
from search_paths_ref import SearchPathsRef

CLASSES = ("shortest", "longer", "no_edge", "cycle_on", "cycle_tail", "k_exact", "k_plus_1")
K_MOVES = 6      # the cutting k_moves of the tests: walks of K_MOVES and K_MOVES + 1 moves exist
NROWS = 16
NQ = 3000
# the largest move an RLE index is given where the dense tables are narrower
# than 4 bits (4-bit tables hold moves up to 15 in both modes: no edge is 15)
WIDE_MOVE = 14
DETOURS = 4      # detour columns per perturbed row

# world -> (graph, share of the runs perturbed, inserted runs per row, the share
# of those that repeat the run's move, seed), chosen so that
# test_foreign_rows_cpu.py's cap conditions hold (its docstring has the counts
# and what was tried first)
WORLDS = {
    "ring2": (GRAPHS["ring2"], 0.05, 4, 0.9, 3),
    "synth": (GRAPHS["synth"], 0.01, 4, 0.5, 7),
    "deg8": (GRAPHS["deg8"], 0.03, 4, 0.3, 8),
    "irregular": (GRAPHS["irregular"], 0.01, 2, 0.5, 5),
}
# the share of the queries drawn from each class; the rest are uniform pairs
QUOTA = {"shortest": 0.02, "longer": 0.06, "no_edge": 0.02, "cycle_on": 0.02,
         "cycle_tail": 0.02, "k_exact": 0.02, "k_plus_1": 0.02}


def table_bits(g):
    """Bits per move of the graph's dense tables (cpd.Graph.move_bits)."""
    maxdeg = int(np.diff(g.row_ptr.astype(np.int64)).max()) if g.n else 0
    return 1 if maxdeg <= 2 else 2 if maxdeg <= 4 else 4


def check_format(off, runs, n):
    """What validate_rows accepts: per row, first column 0, strictly
    increasing columns, every column < n."""
    off = np.asarray(off, np.uint64)
    assert off[0] == 0 and int(off[-1]) == len(runs)
    for r in range(len(off) - 1):
        cols = (runs[int(off[r]):int(off[r + 1])] >> 4).astype(np.int64)
        assert len(cols) >= 1 and cols[0] == 0, f"row {r}: first column"
        assert np.all(np.diff(cols) > 0), f"row {r}: column order"
        assert cols[-1] < n, f"row {r}: column >= n"


def _row_moves(rr, n):
    """The move at every column of one RLE row."""
    starts = (rr >> 4).astype(np.int64)
    return (rr[np.searchsorted(starts, np.arange(n), side="right") - 1] & 0xF).astype(np.int64)


def _rle(mv, breaks):
    """Runs of a per-column move array: a run starts at column 0, where the
    move changes, and at every column of `breaks` besides."""
    cut = np.concatenate(([True], mv[1:] != mv[:-1]))
    cut[np.asarray(sorted(breaks), np.int64)] = True
    starts = np.flatnonzero(cut)
    return ((starts.astype(np.uint32) << 4) | mv[starts].astype(np.uint32)).astype(np.uint32)


def _other_move(rng, old, deg, max_move, missing):
    """A move != old from 0 .. max_move: one naming no edge of a column of
    out-degree deg when `missing` (and the field can hold one), else a real
    other edge when there is one."""
    if missing and deg <= max_move:
        return int(rng.integers(deg, max_move + 1))
    real = [m for m in range(min(deg, max_move + 1)) if m != old]
    if real:
        return int(rng.choice(real))
    return int(rng.choice([m for m in range(max_move + 1) if m != old] or [old]))


def _detours(rng, g, order, t, mv, max_move, count):
    """Up to `count` columns of mv moved to a real other edge from whose head
    the row's walk still reaches t without coming back: the column's walk now
    finishes by another route (longer, or as short).  Returns the columns."""
    n = g.n
    rp, dst = g.row_ptr.astype(np.int64), g.dst.astype(np.int64)
    deg = np.diff(rp)
    done = []
    for v in rng.permutation(n):
        v = int(v)
        if len(done) == count:
            break
        if v == t:
            continue
        for m in rng.permutation(min(int(deg[v]), max_move + 1)):
            m = int(m)
            if m == mv[order[v]]:
                continue
            u, steps = int(dst[rp[v] + m]), 0
            while u != t and u != v and steps < n and mv[order[u]] < deg[u]:
                u, steps = int(dst[rp[u] + mv[order[u]]]), steps + 1
            if u == t:
                mv[order[v]] = m
                done.append(int(order[v]))
                break
    return done


def _trap(rng, g, order, t, mv, max_move):
    """A shortest cycle of the graph through a random node, avoiding t, written
    into mv: its nodes walk the cycle for ever, whatever led to them reaches it
    from a tail.  Returns the columns changed ([] when no node has one)."""
    n = g.n
    rp, dst = g.row_ptr.astype(np.int64), g.dst.astype(np.int64)
    for v in rng.permutation(n)[:32]:
        v = int(v)
        if v == t:
            continue
        par, queue = {v: None}, [v]     # breadth first from v back to v
        for x in queue:
            for m in range(min(int(rp[x + 1] - rp[x]), max_move + 1)):
                u = int(dst[rp[x] + m])
                if u == v:
                    cols = []
                    while x is not None:
                        mv[order[x]] = m
                        cols.append(int(order[x]))
                        x, m = par[x] if par[x] is not None else (None, None)
                    return cols
                if u != t and u not in par and len(par) < 64:
                    par[u] = (x, m)
                    queue.append(u)
    return []


def make_rows(g, order, targets, off, runs, share, inserts, p_same, max_move, seed):
    """(offsets, runs) of len(targets) foreign rows from the oracle's rows:
    all but the last two perturbed, with inserted runs and a target-column
    run; then the random row and the single-run row."""
    rng = np.random.default_rng(seed)
    n = g.n
    deg = np.diff(g.row_ptr.astype(np.int64))
    node_at = np.empty(n, np.int64)         # column -> node
    node_at[order.astype(np.int64)] = np.arange(n)
    out = []
    for r, t in enumerate(targets):
        rr = runs[int(off[r]):int(off[r + 1])]
        if r == len(targets) - 2:            # the random row
            k = max(2, n // 3)
            cols = np.concatenate(([0], np.sort(rng.choice(np.arange(1, n), k - 1, replace=False))))
            out.append(((cols.astype(np.uint32) << 4)
                        | rng.integers(0, max_move + 1, k).astype(np.uint32)).astype(np.uint32))
            continue
        if r == len(targets) - 1:            # the single-run row
            out.append(np.array([int(rng.integers(0, min(2, max_move + 1)))], np.uint32))
            continue
        starts = (rr >> 4).astype(np.int64)
        mv = _row_moves(rr, n)
        breaks = set()
        # perturbed runs: the whole run takes another move
        ends = np.concatenate((starts[1:], [n]))
        for i in np.flatnonzero(rng.random(len(rr)) < share):
            d = int(deg[node_at[starts[i]]])
            mv[starts[i]:ends[i]] = _other_move(rng, int(mv[starts[i]]), d, max_move,
                                                rng.random() < 0.4)
        # inserted runs: a short stretch inside a run
        for c in rng.choice(np.arange(1, n), size=inserts, replace=False):
            c = int(c)
            if rng.random() < p_same:        # the same move again: format only
                breaks.add(c)
                continue
            e = min(n, c + int(rng.integers(1, 7)))
            d = int(deg[node_at[c]])
            mv[c:e] = _other_move(rng, int(mv[c]), d, max_move, rng.random() < 0.4)
            breaks.add(c)
        # the target's own column: a move that names no edge where one exists
        ct = int(order[t])
        d = int(deg[t])
        mv[ct] = max_move if d <= max_move else (int(mv[ct]) + 1) % (max_move + 1)
        breaks.add(ct)
        if r % 4 == 0:
            breaks.update(_trap(rng, g, order, int(t), mv, max_move))
        breaks.update(_detours(rng, g, order, int(t), mv, max_move, DETOURS))
        out.append(_rle(mv, breaks))
    new_off = np.concatenate(([0], np.cumsum([len(x) for x in out]))).astype(np.uint64)
    new_runs = np.concatenate(out).astype(np.uint32)
    check_format(new_off, new_runs, n)
    assert int((new_runs & 0xF).max()) <= max_move
    return new_off, new_runs


def classify(g, order, targets, off, runs, dist, k_moves=K_MOVES):
    """{class: bool[nrows, n]} over every (row, source) pair, source != the
    row's target.  A walk without a cut-off ends at t (on a shortest path or a
    longer one), at a move naming no edge (fewer than n moves, unfinished), or
    at the n-move guard — on a cycle, which the source is on or reaches from a
    tail; k_exact / k_plus_1: finished walks of k_moves and k_moves + 1 moves."""
    n, nr = g.n, len(targets)
    s = np.tile(np.arange(n, dtype=np.uint32), nr)
    t = np.repeat(np.asarray(targets, np.uint32), n)
    cost, hops, fin = oracle.table_search(g.row_ptr, g.dst, g.w, order, targets, off, runs, s, t)
    cost, hops, fin = (a.reshape(nr, n) for a in (cost, hops, fin.astype(bool)))
    ref = SearchPathsRef(g, order, targets, off, runs)
    on_cycle = np.zeros((nr, n), bool)
    for r, x in enumerate(targets):
        e = ref.move_edges(int(x))
        nxt = np.where(e >= 0, ref.dst[np.maximum(e, 0)], -1)
        nxt[int(x)] = -1                     # the walk stops at the target
        for v in np.flatnonzero(hops[r] == n):
            u, seen = int(nxt[v]), 0
            while u != v and seen < n:       # does the walk from v come back to v?
                u, seen = int(nxt[u]), seen + 1
            on_cycle[r, v] = u == v
    other = np.ones((nr, n), bool)
    other[np.arange(nr), np.asarray(targets, np.int64)] = False
    guard = ~fin & (hops == n)
    assert not np.any(fin & (cost < dist)), "a walk beat the shortest path"
    return {
        "shortest": other & fin & (cost == dist),
        "longer": other & fin & (cost > dist),
        "no_edge": other & ~fin & (hops < n),
        "cycle_on": other & guard & on_cycle,
        "cycle_tail": other & guard & ~on_cycle,
        "k_exact": other & fin & (hops == k_moves),
        "k_plus_1": other & fin & (hops == k_moves + 1),
    }


# the option sets of the search tests; K_MOVES cuts some walks
SEARCH_OPTS = [dict(), dict(fscale=0.25), dict(hscale=1.5), dict(hscale=0.5, fscale=0.1),
               dict(k_moves=K_MOVES), dict(itrs=7)]
SEARCH_IDS = [",".join(f"{k}={v}" for k, v in o.items()) or "default" for o in SEARCH_OPTS]


def table_search(w, w_sel=None, k_moves=-1):
    """oracle.table_search of the world's queries over its foreign rows."""
    g = w.g
    return oracle.table_search(g.row_ptr, g.dst, g.w if w_sel is None else w_sel, w.order,
                               w.targets, w.off, w.runs, w.s, w.t, k_moves=k_moves)


def cpd_search(w, w_sel, **opts):
    """oracle.cpd_search of the world's queries over its foreign rows."""
    g = w.g
    return oracle.cpd_search(g.row_ptr, g.dst, g.w, w_sel, w.order, w.targets, w.off, w.runs,
                             w.s, w.t, **opts)


class World:
    """One graph with its foreign rows, queries and weights (never changed)."""


@functools.lru_cache(maxsize=None)
def world(name, max_move=None):
    """The world `name` with moves up to max_move (None: what the graph's
    dense tables hold).  QUOTA of the queries are drawn class by class, so that
    every class is walked; the rest are uniform (source, row) pairs."""
    graph, share, inserts, p_same, seed = WORLDS[name]
    w = World()
    w.name, w.share, w.inserts, w.seed = name, share, inserts, seed
    w.g = g = graph()
    w.max_move = (1 << table_bits(g)) - 1 if max_move is None else max_move
    w.plan = cpd.Plan(g)
    w.order = w.plan.order()
    rng = np.random.default_rng(seed)
    deg = np.diff(g.row_ptr.astype(np.int64))
    indeg = np.bincount(g.dst, minlength=g.n)
    live = np.flatnonzero((deg > 0) & (indeg > 0))   # a target that can be reached and left
    w.targets = rng.choice(live, size=NROWS, replace=False).astype(np.uint32)
    w.off0, w.runs0 = oracle.build_rows(g.row_ptr, g.dst, g.w, w.order, w.targets)
    w.off, w.runs = make_rows(g, w.order, w.targets, w.off0, w.runs0, share, inserts, p_same, w.max_move, seed)
    w.dist = np.stack([oracle.reverse_dijkstra(g.row_ptr, g.dst, g.w, int(x)) for x in w.targets])
    w.classes = classify(g, w.order, w.targets, w.off, w.runs, w.dist)
    w.uniform = NQ - sum(int(NQ * q) for q in QUOTA.values())
    rows = [rng.integers(0, NROWS, w.uniform)]
    srcs = [rng.integers(0, g.n, w.uniform)]
    # most of the pairs the graph itself does not join are drawn again
    for i in np.flatnonzero((w.dist[rows[0], srcs[0]] == oracle.INF)
                            & (rng.random(w.uniform) < 0.8)):
        srcs[0][i] = rng.choice(np.flatnonzero(w.dist[rows[0][i]] != oracle.INF))
    for c in CLASSES:
        r, v = np.nonzero(w.classes[c])
        if len(r):
            pick = rng.integers(0, len(r), int(NQ * QUOTA[c]))
            rows.append(r[pick])
            srcs.append(v[pick])
    w.s = np.concatenate(srcs).astype(np.uint32)
    w.t = w.targets[np.concatenate(rows)]
    w.s[0] = w.t[0]                                   # a query with s == t
    # congested weights (>= free flow) and weights below free flow (>= 0)
    w.wc = cpd.synth_congestion(g.w, frac=0.3, lo=1.0, hi=3.0, seed=4)
    w.wl = (g.w - (g.w * rng.random(g.m) * 0.6).astype(np.uint32)).astype(np.uint32)
    w.ref = SearchPathsRef(g, w.order, w.targets, w.off, w.runs)
    return w


def query_classes(w):
    """{class: bool[nq]} of the world's queries (s == t is in none)."""
    row_of = {int(t): i for i, t in enumerate(w.targets)}
    r = np.array([row_of[int(x)] for x in w.t])
    return {c: m[r, w.s.astype(np.int64)] for c, m in w.classes.items()}
