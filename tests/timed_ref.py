"""Reference for timed walks (cpd_query_timed / Index.timed): the table-search
walk with a u64 clock per query.  The clock starts at depart[q]; move number h
on original edge e_h (e = row_ptr[cur] + move, as tests/loads_ref.py) does

    j_h       = min(tau_h // P, K - 1)
    c_h       = W_{j_h}[e_h]
    tau_{h+1} = tau_h + c_h

and adds demand[q] to loads[j_h, e_h]; cost = tau_end - depart[q].  The stop
rules are oracle.table_search's: at t, after `limit` moves, or at a move naming
no out-edge (which costs and adds nothing).

walk_timed is the lock-step numpy walk in the manner of costs_ref.walk_costs /
loads_ref.walk_loads; walk_timed_scalar is a deliberately plain per-query loop
in Python integers over the same move table, and walk_timed_sets also returns
the set of every move (tests read "one move crosses several periods" off it)."""
import numpy as np

import oracle
from costs_ref import weights_of
from loads_ref import move_table


def _setup(g, order, targets, off, runs, s, t, sets, depart, demand, k_moves):
    n = g.n
    table = move_table(off, runs, n)
    row_of = np.full(n, -1, np.int64)
    row_of[targets] = np.arange(len(targets))
    s, t = np.asarray(s, np.int64), np.asarray(t, np.int64)
    nq = len(s)
    row = row_of[t]
    assert (row >= 0).all()
    ws = np.stack(weights_of(g, sets)).astype(np.uint64)  # [K, m]
    dep = np.zeros(nq, np.uint64) if depart is None else np.asarray(depart).astype(np.uint64)
    dem = np.ones(nq, np.uint64) if demand is None else np.asarray(demand).astype(np.uint64)
    assert dep.shape == (nq,) and dem.shape == (nq,)
    limit = n if k_moves < 0 else min(k_moves, n)
    return table, row, s, t, ws, dep, dem, limit


def walk_timed_sets(g, order, targets, off, runs, s, t, sets, depart, P, demand=None, k_moves=-1):
    """(cost u64[nq], hops, fin, loads u64[K, m], jumps): jumps[q] = the largest
    rise of the set index from one move of walk q to its next."""
    table, row, s, t, ws, dep, dem, limit = _setup(g, order, targets, off, runs, s, t, sets,
                                                   depart, demand, k_moves)
    assert 1 <= int(P) <= 1 << 60 and (len(dep) == 0 or int(dep.max()) < 1 << 63)
    K, P = len(ws), np.uint64(P)
    rp, dst = g.row_ptr.astype(np.int64), g.dst.astype(np.int64)
    outdeg = np.diff(rp)
    order = order.astype(np.int64)
    nq = len(s)
    cur = s.copy()
    hops = np.zeros(nq, np.int64)
    tau = dep.copy()
    last_j = np.full(nq, -1, np.int64)
    jumps = np.zeros(nq, np.int64)
    loads = np.zeros((K, len(dst)), np.uint64)
    idx = np.arange(nq)
    h = 0
    while len(idx):
        c = cur[idx]
        mv = table[row[idx], order[c]]
        go = (c != t[idx]) & (h < limit) & (mv < outdeg[c])
        idx, c, mv = idx[go], c[go], mv[go]
        e = rp[c] + mv
        j = np.minimum(tau[idx] // P, np.uint64(K - 1)).astype(np.int64)
        np.add.at(loads, (j, e), dem[idx])
        seen = last_j[idx] >= 0
        jumps[idx] = np.maximum(jumps[idx], np.where(seen, j - last_j[idx], 0))
        last_j[idx] = j
        tau[idx] += ws[j, e]
        cur[idx] = dst[e]
        h += 1
        hops[idx] = h
    return tau - dep, hops.astype(np.uint32), (cur == t).astype(np.uint8), loads, jumps


def walk_timed(g, order, targets, off, runs, s, t, sets, depart, P, demand=None, k_moves=-1):
    """(cost u64[nq], hops, fin, loads u64[K, m])."""
    return walk_timed_sets(g, order, targets, off, runs, s, t, sets, depart, P, demand,
                           k_moves)[:4]


def walk_timed_scalar(g, order, targets, off, runs, s, t, sets, depart, P, demand=None,
                      k_moves=-1):
    """The same, one query at a time, in Python integers."""
    table, row, s, t, ws, dep, dem, limit = _setup(g, order, targets, off, runs, s, t, sets,
                                                   depart, demand, k_moves)
    K, P = len(ws), int(P)
    nq = len(s)
    cost = np.zeros(nq, np.uint64)
    hops = np.zeros(nq, np.uint32)
    fin = np.zeros(nq, np.uint8)
    loads = [[0] * g.m for _ in range(K)]
    for q in range(nq):
        cur, tt, tau, h = int(s[q]), int(t[q]), int(dep[q]), 0
        while cur != tt and h < limit:
            mv = int(table[row[q], order[cur]])
            if mv >= int(g.row_ptr[cur + 1]) - int(g.row_ptr[cur]):
                break
            e = int(g.row_ptr[cur]) + mv
            j = min(tau // P, K - 1)
            loads[j][e] += int(dem[q])
            tau += int(ws[j, e])
            cur = int(g.dst[e])
            h += 1
        cost[q], hops[q], fin[q] = tau - int(dep[q]), h, cur == tt
    return cost, hops, fin, np.array(loads, dtype=object).astype(np.uint64).reshape(K, g.m)
