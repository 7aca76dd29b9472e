"""References for costs under several weight sets (cpd_query_costs /
Index.costs).  Both modes are referred to the oracle itself:

  all sets   column j = oracle.table_search(..., w_sel = w_j, k_moves)
  sliced     at S moves per set over K sets, with the walk's limit L (n when
             k_moves < 0) and P_j(x) = the oracle's cost under set j with
             k_moves = x:
               sum_{j < K-1} [P_j(min(L, (j+1) S)) - P_j(min(L, j S))]
               + P_{K-1}(L) - P_{K-1}(min(L, (K-1) S))
             (the route never depends on the weights, so P_j(b) - P_j(a) is
             the cost of moves a .. b-1 under set j).

walk_costs is a lock-step numpy walk — the one of tests/test_gpu_paths.py
(ref_paths) restated, costing hop h under set min(h // S, K - 1) — against
which tests/test_costs_cpu.py pins the sliced identity."""
import numpy as np

import oracle


def weights_of(g, sets):
    """The weight arrays of a set list (None = the free-flow weights)."""
    return [g.w if w is None else np.ascontiguousarray(w, np.uint32) for w in sets]


def ref_all(g, order, targets, off, runs, s, t, sets, k_moves=-1):
    """(costs[nq, K], hops, fin): one oracle walk per set."""
    cols, hops, fin = [], None, None
    for w in weights_of(g, sets):
        c, h, f = oracle.table_search(g.row_ptr, g.dst, w, order, targets, off, runs, s, t,
                                      k_moves=k_moves)
        if hops is not None:  # the route does not depend on the weights
            np.testing.assert_array_equal(h, hops)
            np.testing.assert_array_equal(f, fin)
        cols.append(c.astype(np.uint64))
        hops, fin = h, f
    return np.stack(cols, axis=1), hops, fin


def ref_sliced(g, order, targets, off, runs, s, t, sets, S, k_moves=-1):
    """(costs[nq, 1], hops, fin) by the identity above."""
    assert S > 0
    ws = weights_of(g, sets)
    K, n = len(ws), g.n
    L = n if k_moves < 0 else min(k_moves, n)
    memo = {}

    def P(j, x):
        if (j, x) not in memo:
            km = k_moves if x == L else x  # x == L: the walk as asked for
            memo[(j, x)] = oracle.table_search(g.row_ptr, g.dst, ws[j], order, targets, off, runs,
                                               s, t, k_moves=km)
        return memo[(j, x)][0].astype(np.uint64)

    total = np.zeros(len(s), np.uint64)
    for j in range(K - 1):
        total += P(j, min(L, (j + 1) * S)) - P(j, min(L, j * S))
    total += P(K - 1, L) - P(K - 1, min(L, (K - 1) * S))
    _, hops, fin = memo[(K - 1, L)]
    return total.reshape(-1, 1), hops, fin


def walk_costs(g, order, targets, off, runs, s, t, sets, S=0, k_moves=-1):
    """All walks at once, in lock step: (costs[nq, C], hops, fin).  mv = the
    row's move at the current node's column; a walk stops at t, after `limit`
    moves or at a move naming no out-edge.  S == 0: C = K, every hop costed
    under every set; S > 0: C = 1, hop h costed under set min(h // S, K - 1)."""
    n = g.n
    ws = np.stack(weights_of(g, sets)).astype(np.uint64)  # [K, m]
    K = len(ws)
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
    costs = np.zeros((nq, 1 if S else K), np.uint64)
    idx = np.arange(nq)
    h = 0
    while len(idx):
        c = cur[idx]
        mv = table[row[idx], order[c]]
        go = (c != t[idx]) & (h < limit) & (mv < outdeg[c])
        idx, c, mv = idx[go], c[go], mv[go]
        e = rp[c] + mv
        cur[idx] = dst[e]
        if S:
            costs[idx, 0] += ws[min(h // S, K - 1), e]
        else:
            costs[idx] += ws[:, e].T
        h += 1
        hops[idx] = h
    return costs, hops.astype(np.uint32), (cur == t).astype(np.uint8)
