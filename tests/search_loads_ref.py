"""ref_search_loads: ref_search_paths (tests/search_paths_ref.py) that also
keeps, per node, the EDGE that set g — and returns the edge loads of the
routes as cpd_api.h defines them at cpd_query_search_loads:

  prefix move p -> u  the edge whose relaxation set g(u): the expansion of p
          scans p's out-list in file order and replaces g(u) only by a
          strictly smaller value, so among the parallel edges p -> u it is the
          first of least weight under the selected weights;
  suffix move         the edge the row's move names (ref.move_edges(t)), what
          cpd_query_loads counts.

demand[q] is added to loads[e] for every edge e of the route of a query with
finished == 1.  The search loop is ref_search_paths' line for line (the heap,
the floats, the counters); tests/test_search_loads_cpu.py pins both against
each other and against the oracle's sums.
"""
import heapq

import numpy as np

from graphs import graph_from_edges
from search_paths_ref import INF


def ref_search_loads(ref, w_sel, s, t, demand=None, hscale=1.0, fscale=0.0, k_moves=-1, itrs=-1):
    """(cost, plen, fin, stats, paths, pcost, loads u64[m], moves,
    prefix_moves): the first six as ref_search_paths returns them; moves = the
    counter adds made over all routes, prefix_moves those on A*-tree edges."""
    nq = len(s)
    cost = np.zeros(nq, np.uint64)
    plen = np.zeros(nq, np.uint32)
    fin = np.zeros(nq, np.uint8)
    stats = np.zeros((nq, 5), np.uint64)
    paths, pcost = [], []
    order = ref.order.tolist()
    dst = ref.dst.tolist()
    rp = ref.rp.tolist()
    ws = np.asarray(w_sel).tolist()
    dem = [1] * nq if demand is None else [int(d) for d in demand]
    loads = [0] * len(dst)
    moves = prefix_moves = 0
    f1 = 1.0 + fscale
    for q in range(nq):
        sq, tq = int(s[q]), int(t[q])
        hf, cw, lw = ref.walks(tq, w_sel)
        expanded = inserted = touched = updated = surplus = 0
        ub, best_len, vstar = INF, 0, -1
        g, depth, par, pare, heap = {}, {}, {}, {}, []
        if hf[sq] != INF:
            g[sq], depth[sq], par[sq] = 0, 0, -1
            inserted = 1
            heap.append((int(hscale * float(hf[sq])), order[sq], 0, sq))
        while heap:
            f, _, kg, v = heapq.heappop(heap)
            if kg > g[v]:
                surplus += 1
                continue
            if float(f) * f1 >= float(ub):
                break
            if 0 <= itrs <= expanded:
                break
            expanded += 1
            if cw[v] != INF and (k_moves < 0 or lw[v] <= k_moves):
                cand = kg + cw[v]
                if cand < ub:
                    ub, best_len, vstar = cand, depth[v] + lw[v], v
            dv = depth[v] + 1
            for e in range(rp[v], rp[v + 1]):   # the out-list, in file order
                u, we = dst[e], ws[e]
                touched += 1
                ng = kg + we
                if u not in g:
                    if hf[u] == INF:
                        continue
                    inserted += 1
                elif ng < g[u]:
                    updated += 1
                else:
                    continue
                g[u], depth[u], par[u], pare[u] = ng, dv, v, e   # e set g(u)
                heapq.heappush(heap, (ng + int(hscale * float(hf[u])), order[u], ng, u))
        stats[q] = (expanded, inserted, touched, updated, surplus)
        if ub == INF:
            paths.append([])
            pcost.append(0)
            continue
        cost[q], plen[q], fin[q] = ub, best_len, 1
        chain, c = [], 0
        v = vstar
        while v != -1:
            chain.append(v)
            if v in pare:
                e = pare[v]
                c += ws[e]
                loads[e] += dem[q]
                prefix_moves += 1
                moves += 1
            v = par[v]
        chain.reverse()
        e_of = ref.move_edges(tq)
        v = vstar
        for _ in range(lw[vstar]):
            e = int(e_of[v])
            loads[e] += dem[q]
            moves += 1
            v = dst[e]
            chain.append(v)
        assert v == tq
        paths.append(chain)
        pcost.append(c + cw[vstar])
    return (cost, plen, fin, stats, paths, pcost, np.array(loads, np.uint64), moves,
            prefix_moves)


def skip2_graph():
    """Out-degree 2 (2-slot adjacency, the shift-1 kernels) WITH alternative
    routes: a -> a + 1 (weights 1..5) and a -> a + 2 (1..9) around a ring of
    500.  graphs.ring2_graph is all but one-way (every 7th node lacks its back
    edge), so no search on it ever leaves the CPD path: its prefixes are [s]."""
    rng = np.random.default_rng(22)
    n = 500
    edges = []
    for a in range(n):
        edges.append((a, (a + 1) % n, int(rng.integers(1, 6))))
        edges.append((a, (a + 2) % n, int(rng.integers(1, 10))))
    return graph_from_edges(n, edges)


# parallel_flip_graph: 9 nodes, target 8.  Edges in file order (index: tail ->
# head, free-flow / congested weight), listed by tail so that the index below
# is the edge's index in the graph:
#    0: 0->1  2/9     1: 0->1  3/4     the cheaper of the pair flips       (a)
#    2: 0->6  9/9                      a detour 0 6 7 8 (27), never taken
#    3: 1->2  2/7     4: 1->2  4/5     5: 1->2  4/5   equal congested: 4   (b)
#    6: 2->3 11/30    7: 2->4  5/5
#    8: 3->8  1/1
#    9: 4->5  1/6    10: 4->5  2/2     the row names 9, the dearer         (c)
#   11: 5->8  5/5    12: 6->7  9/9    13: 7->8  9/9
# Free flow, the CPD path from 0 is 0 1 2 4 5 8 over edges 0, 3, 7, 9, 11 (15).
# Congested, that walk costs 9 + 7 + 5 + 6 + 5 = 32.  The search from 0 pops 0
# (incumbent 32), 1 at g = 4 over edge 1 (27, v* = 1), 2 at g = 9 over edge 4
# — edge 3 gave 11, edge 5 ties with 4 and does not replace it — (25, v* = 2):
#   fscale = 0.25 stops here (f_min = 20, 20 x 1.25 >= 25): prefix edges 1, 4,
#       then the walk 2 4 5 8 over edges 7, 9, 11 — edge 9 (6) although edge
#       10 (2) joins the same nodes;
#   fscale = 0 goes on: 4 at 14, 5 at 16 over edge 10 (21, v* = 5), and stops
#       at t: prefix edges 1, 4, 7, 10, then edge 11.  A search left to run
#       under a consistent heuristic never keeps a dearer parallel edge (the
#       cheaper one gives a cheaper route, which it finds): (c) needs the
#       bounded-suboptimal stop.
PARALLEL_FLIP_EDGES = [
    (0, 1, 2, 9), (0, 1, 3, 4), (0, 6, 9, 9), (1, 2, 2, 7), (1, 2, 4, 5), (1, 2, 4, 5),
    (2, 3, 11, 30), (2, 4, 5, 5), (3, 8, 1, 1), (4, 5, 1, 6), (4, 5, 2, 2), (5, 8, 5, 5),
    (6, 7, 9, 9), (7, 8, 9, 9)]
PARALLEL_FLIP_OPTS = [dict(), dict(fscale=0.25)]


def parallel_flip_graph():
    """(graph, congested weights, s, t, targets): a hand-made graph with (a) a
    prefix move over two parallel edges whose cheaper one differs between the
    free-flow and the congested weights, (b) a prefix move over two parallel
    edges of equal congested weight, (c) a suffix move whose CPD edge is the
    dearer of two parallel edges under congestion (with fscale = 0.25: see
    above).  Every congested weight is >= its free-flow weight."""
    e = PARALLEL_FLIP_EDGES
    assert all(a[0] <= b[0] for a, b in zip(e, e[1:])), "listed by tail: list index = edge index"
    g = graph_from_edges(9, [(a, b, f) for a, b, f, _ in e])
    wc = np.array([c for _, _, _, c in e], np.uint32)
    s = np.array([0, 1, 2, 4, 8, 6, 3], np.uint32)
    t = np.full(len(s), 8, np.uint32)
    return g, wc, s, t, np.array([8], np.uint32)
