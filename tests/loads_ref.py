"""Reference for edge loads (cpd_query_loads / Index.loads): a lock-step numpy
walk over the oracle's rows, in the manner of tests/costs_ref.py.  Every hop
takes the row's move at the current node's column — oracle.get_move's answer,
the move of the last run starting at or before the column, read for all walks
at once from oracle.moves_from_runs (tests/test_loads_cpu.py pins that table
against oracle.get_move itself) — the edge taken is e = row_ptr[cur] + move,
an index in original edge order, and the query's demand is added to
loads[j, e], j = min(h // S, K - 1) for hop number h.  The stop rules are
oracle.table_search's: at t, after `limit` moves, or at a move naming no
out-edge (which adds nothing)."""
import numpy as np

import oracle


def move_table(off, runs, n):
    """table[row, column] = the row's move at the column."""
    mv4 = oracle.moves_from_runs(off, runs, n, 4)
    table = ((mv4[:, :, None] >> (4 * np.arange(8, dtype=np.uint32))) & 0xF)
    return table.reshape(len(off) - 1, -1)[:, :n].astype(np.int64)


def walk_loads(g, order, targets, off, runs, s, t, demand=None, K=1, S=0, k_moves=-1):
    """(loads u64[K, m], hops, fin).  K == 1: S must be 0, one plane; K > 1:
    hop h of a walk counts in plane min(h // S, K - 1)."""
    assert (K == 1) == (S == 0)
    n = g.n
    table = move_table(off, runs, n)
    row_of = np.full(n, -1, np.int64)
    row_of[targets] = np.arange(len(targets))
    s, t = np.asarray(s, np.int64), np.asarray(t, np.int64)
    nq = len(s)
    dem = np.ones(nq, np.uint64) if demand is None else np.asarray(demand).astype(np.uint64)
    assert dem.shape == (nq,)
    row = row_of[t]
    assert (row >= 0).all()
    rp, dst = g.row_ptr.astype(np.int64), g.dst.astype(np.int64)
    outdeg = np.diff(rp)
    order = order.astype(np.int64)
    limit = n if k_moves < 0 else min(k_moves, n)
    cur = s.copy()
    hops = np.zeros(nq, np.int64)
    loads = np.zeros((K, len(dst)), np.uint64)
    idx = np.arange(nq)
    h = 0
    while len(idx):
        c = cur[idx]
        mv = table[row[idx], order[c]]
        go = (c != t[idx]) & (h < limit) & (mv < outdeg[c])
        idx, c, mv = idx[go], c[go], mv[go]
        e = rp[c] + mv
        np.add.at(loads[min(h // S, K - 1) if S else 0], e, dem[idx])
        cur[idx] = dst[e]
        h += 1
        hops[idx] = h
    return loads, hops.astype(np.uint32), (cur == t).astype(np.uint8)
