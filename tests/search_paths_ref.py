"""ref_search_paths: a Python restatement of the oracle's CPD-heuristic search
(oracle/cpd_oracle.c ora_cpd_search) that also keeps what names the route —
the parent of every node and the incumbent's node v* — and returns the search
path as cpd_api.h defines it at cpd_query_search_paths:

  prefix  the parent chain v* -> par(v*) -> ... -> s read when the search has
          ended, reversed; par(u) = the node whose relaxation last set g(u);
  suffix  the row's table-search walk from v* to t, without v*.

Python floats are the oracle's doubles: int(hscale * float(hf)) and
float(f) * (1 + fscale) >= float(ub), as the C does.  The heap is heapq over
(f, column, g, node): the oracle's key order is total over the entries a
search holds, so the pops are those of its binary heap.
tests/test_search_paths_cpu.py pins cost / plen / finished and the five
counters of this restatement against oracle.cpd_search.
"""
import heapq

import numpy as np

INF = (1 << 64) - 1


class SearchPathsRef:
    """The CPD walks of one (graph, column order, index rows), per target."""

    def __init__(self, g, order, targets, off, runs):
        self.rp = g.row_ptr.astype(np.int64)
        self.dst = g.dst.astype(np.int64)
        self.w_free = g.w
        self.order = np.asarray(order, np.int64)
        self.n = len(self.rp) - 1
        self.deg = np.diff(self.rp)
        self.targets = np.asarray(targets)
        self.row_of = {int(t): i for i, t in enumerate(self.targets)}
        self.off = np.asarray(off, np.uint64)
        self.runs = np.asarray(runs, np.uint32)
        self._edge = {}    # target -> the edge each node's move names (-1: none)
        self._memo = {}    # (target, id of the weights) -> hf, cw, lw
        self._adj = {}     # id of the weights -> per node [(head, weight), ...]
        self._keep = []    # the weight arrays behind those ids

    def move_edges(self, t):
        """e[v] = the out-edge the row of t names at v (ora_get_move: the last
        run starting at or before v's column), -1 when v has no such edge."""
        if t not in self._edge:
            r = self.row_of[t]
            rr = self.runs[int(self.off[r]):int(self.off[r + 1])]
            starts = (rr >> 4).astype(np.int64)
            mv = (rr[np.searchsorted(starts, self.order, side="right") - 1] & 0xF).astype(np.int64)
            self._edge[t] = np.where(mv < self.deg, self.rp[:-1] + mv, -1)
        return self._edge[t]

    def walks(self, t, w_sel):
        """hf, cw, lw of every node for target t (ora_walk from every node):
        the free-flow cost, the cost under w_sel and the moves of its CPD walk
        to t; INF, INF, 0 when the walk meets a missing edge or a cycle."""
        key = (t, id(w_sel))
        if key in self._memo:
            return self._memo[key]
        self._keep.append(w_sel)
        e_of = self.move_edges(t).tolist()
        dst, wf, ws = self.dst.tolist(), self.w_free.tolist(), np.asarray(w_sel).tolist()
        n = self.n
        hf, cw, lw, known = [INF] * n, [INF] * n, [0] * n, [0] * n
        hf[t] = cw[t] = 0
        known[t] = 1
        for v in range(n):
            stack, x, bad = [], v, False
            while known[x] != 1:
                if known[x] == 2:
                    bad = True
                    break
                known[x] = 2
                stack.append(x)
                e = e_of[x]
                if e < 0:
                    bad = True
                    break
                x = dst[e]
            a, b, c = (INF, INF, 0) if bad else (hf[x], cw[x], lw[x])
            while stack:
                y = stack.pop()
                if a != INF:
                    a, b, c = a + wf[e_of[y]], b + ws[e_of[y]], c + 1
                known[y] = 1
                hf[y], cw[y], lw[y] = a, b, (0 if a == INF else c)
        self._memo[key] = (hf, cw, lw)
        return self._memo[key]

    def adjacency(self, w_sel):
        key = id(w_sel)
        if key not in self._adj:
            self._keep.append(w_sel)
            dst, ws, rp = self.dst.tolist(), np.asarray(w_sel).tolist(), self.rp.tolist()
            self._adj[key] = [list(zip(dst[rp[v]:rp[v + 1]], ws[rp[v]:rp[v + 1]]))
                              for v in range(self.n)]
        return self._adj[key]


def ref_search_paths(ref, w_sel, s, t, hscale=1.0, fscale=0.0, k_moves=-1, itrs=-1):
    """Per query: cost, plen, finished, stats[nq, 5] as oracle.cpd_search, and
    paths (a list of node lists; [] without an incumbent) with pcost, each
    path's cost along the edges this restatement took (0 for [])."""
    nq = len(s)
    cost = np.zeros(nq, np.uint64)
    plen = np.zeros(nq, np.uint32)
    fin = np.zeros(nq, np.uint8)
    stats = np.zeros((nq, 5), np.uint64)
    paths, pcost = [], []
    order = ref.order.tolist()
    adj = ref.adjacency(w_sel)
    dst = ref.dst.tolist()
    f1 = 1.0 + fscale
    for q in range(nq):
        sq, tq = int(s[q]), int(t[q])
        hf, cw, lw = ref.walks(tq, w_sel)
        expanded = inserted = touched = updated = surplus = 0
        ub, best_len, vstar = INF, 0, -1
        g, depth, par, parw, heap = {}, {}, {}, {}, []
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
            for u, we in adj[v]:
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
                g[u], depth[u], par[u], parw[u] = ng, dv, v, we
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
            c += parw.get(v, 0)
            v = par[v]
        chain.reverse()
        e_of = ref.move_edges(tq)
        v = vstar
        for _ in range(lw[vstar]):
            v = dst[int(e_of[v])]
            chain.append(v)
        assert v == tq
        paths.append(chain)
        pcost.append(c + cw[vstar])
    return cost, plen, fin, stats, paths, pcost


def flatten(paths):
    """(offsets u64[nq + 1], nodes u32[]) of a list of node lists."""
    off = np.zeros(len(paths) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in paths], dtype=np.uint64)
    nodes = np.fromiter((v for p in paths for v in p), np.uint32, count=int(off[-1]))
    return off, nodes


def reopened_graph():
    """A 7-node graph on which hscale = 1.5 with itrs = 3 ends the search of
    (s, t) = (0, 6) between the re-opening of the incumbent's node and its
    second expansion: (graph, congested weights, s, t).  Free-flow / congested
    weights: 0->1 1/100, 0->2 10/10, 0->3 2/2, 1->6 1/1, 2->4 4/20, 3->2 7/7,
    3->5 1/200, 4->6 10/10, 5->6 19/19.  Pops: 0 (incumbent 101 over 1), 2
    (g = 10: incumbent 40, v* = 2, plen 3), 3 (g(2) improves to 9, parent 3),
    then the expansion limit.  The path read at the end is 0 3 2 4 6: 4 moves
    and cost 39, against the reported plen 3 and cost 40."""
    from graphs import graph_from_edges
    e = [(0, 1, 1, 100), (0, 2, 10, 10), (0, 3, 2, 2), (1, 6, 1, 1), (2, 4, 4, 20),
         (3, 2, 7, 7), (3, 5, 1, 200), (4, 6, 10, 10), (5, 6, 19, 19)]
    g = graph_from_edges(7, [(a, b, f) for a, b, f, _ in e])
    wc = np.array([w for _, _, _, w in e], np.uint32)  # edges are listed in node order
    return g, wc, np.array([0, 3, 6], np.uint32), np.array([6, 6, 6], np.uint32)
