"""Placing a chosen load table and flow table through the public API, so that
hand-picked boundary values reach the assignment kernels.

Y, one edge at a time: a walk limited to one move (Index.loads(.., k_moves=1))
adds its query's demand to the edge row_ptr[u] + move, move = the row of the
target at the column of u (loads_ref.move_table).  An edge is LOADABLE on a
world when some target of the world has it as the first move from its tail; a
counter above 2^32 - 1 takes several queries on that edge, a table of more than
BATCH queries takes accumulating calls.  K planes: the timed walk with
k_moves=1 and loads=True; cpd_api.h "Timed walks" puts a move entered at clock
time tau into plane min(tau / P, K - 1), and the clock of the first move is the
query's departure, so depart = j P lands in plane j.  X: two steps with an
explicit lambda — the initialising step from Y1 leaves X = Y1 << 16, a step of
lambda = 1 towards Y2 adds floor(((Y2 - Y1) << 16) / 2^16) = Y2 - Y1 — give X =
(Y1 << 16) + (Y2 - Y1) exactly; with Y1 = X >> 16 and Y2 = Y1 + (X & 0xFFFF)
that is any X below 2^63.

Every placement asserts what it placed (loads_fetch / flow_fetch against the
wanted table): a misplacement fails there, not later in a comparison of
weights.  World.check_* do the same without a device, against
loads_ref.walk_loads and timed_ref.walk_timed."""
import numpy as np

import oracle
from graphs import graph_from_edges
from loads_ref import move_table, walk_loads
from timed_ref import walk_timed

U32 = 0xFFFFFFFF
BATCH = 32768      # queries per call
PERIOD = 1000      # of the timed placements: plane j departs at j * PERIOD


def made_graph(w0s, fan):
    """The purpose-made graph: a one-way ring of R nodes (weight 1); ring node
    i also has `fan` out-edges (weight 1) to feeder nodes, and a feeder's
    single out-edge leads straight back to its ring node with the chosen
    weight w0s[k].  A feeder's first move is forced whatever the weights; the
    adjacency has fan + 1 slots per column (feeders: 1 edge and fan padding
    slots).  Strongly connected, and no path takes two feeder edges, so the
    distance bound is about max(w0s) + 2 R.  Returns (graph, the edge index of
    every feeder's out-edge)."""
    nf = len(w0s)
    R = max(3, -(-nf // fan))
    edges = []
    for i in range(R):
        edges.append((i, (i + 1) % R, 1))
        for k in range(i * fan, min(nf, (i + 1) * fan)):
            edges.append((i, R + k, 1))
    for k, w in enumerate(w0s):
        edges.append((R + k, k // fan, int(w)))
    g = graph_from_edges(R + nf, edges)
    return g, g.row_ptr[R:R + nf].astype(np.int64)


class World:
    """A graph, its column order, a set of targets with their rows, and for
    every edge a target that loads it in one move (target_of[e], -1: none)."""

    def __init__(self, g, targets, order=None):
        self.g = g
        self.order = oracle.dfs_preorder(g.row_ptr, g.dst) if order is None else order
        self.targets = np.asarray(targets, np.uint32)
        self.off, self.runs = oracle.build_rows(g.row_ptr, g.dst, g.w, self.order, self.targets)
        rp = g.row_ptr.astype(np.int64)
        self.src = np.repeat(np.arange(g.n), np.diff(rp))
        table = move_table(self.off, self.runs, g.n)
        col = self.order.astype(np.int64)
        outdeg, nodes = np.diff(rp), np.arange(g.n)
        self.target_of = np.full(g.m, -1, np.int64)
        for r, t in enumerate(self.targets.tolist()):
            mv = table[r, col]
            ok = (mv < outdeg) & (nodes != t)
            e = rp[:-1][ok] + mv[ok]
            e = e[self.target_of[e] < 0]
            self.target_of[e] = t
        self._dev = None

    def loadable(self):
        return np.nonzero(self.target_of >= 0)[0]

    def _queries(self, Y):
        """(s, t, demand) of the one-move queries that place Y (m ints)."""
        Y = [int(v) for v in Y]
        assert len(Y) == self.g.m and all(0 <= v < 1 << 47 for v in Y)
        s, t, d = [], [], []
        for e, y in enumerate(Y):
            if not y:
                continue
            assert self.target_of[e] >= 0, f"edge {e} is not loadable"
            parts = [U32] * (y // U32) + ([y % U32] if y % U32 else [])
            s += [int(self.src[e])] * len(parts)
            t += [int(self.target_of[e])] * len(parts)
            d += parts
        if not s:  # an all-zero table still takes a call: one query of demand 0
            e = int(self.loadable()[0])
            s, t, d = [int(self.src[e])], [int(self.target_of[e])], [0]
        return np.array(s, np.uint32), np.array(t, np.uint32), np.array(d, np.uint32)

    def batches(self, planes):
        """The calls that place the planes (K tables of m ints): a list of (s,
        t, demand, depart), depart = j * PERIOD for plane j."""
        parts = [self._queries(Y) + (j,) for j, Y in enumerate(planes)]
        s, t, d = (np.concatenate([p[i] for p in parts]) for i in range(3))
        dep = np.concatenate([np.full(len(p[0]), p[3] * PERIOD, np.uint64) for p in parts])
        return [(s[i:i + BATCH], t[i:i + BATCH], d[i:i + BATCH], dep[i:i + BATCH])
                for i in range(0, len(s), BATCH)]

    # --- without a device -----------------------------------------------------
    def check_place(self, Y):
        got = np.zeros(self.g.m, np.uint64)
        for s, t, d, _ in self.batches([Y]):
            got += walk_loads(self.g, self.order, self.targets, self.off, self.runs, s, t, d,
                              k_moves=1)[0][0]
        assert got.tolist() == [int(v) for v in Y]

    def check_place_planes(self, planes):
        K = len(planes)
        got = np.zeros((K, self.g.m), np.uint64)
        for s, t, d, dep in self.batches(planes):
            got += walk_timed(self.g, self.order, self.targets, self.off, self.runs, s, t,
                              [None] * K, dep, PERIOD, d, k_moves=1)[3]
        assert got.tolist() == [[int(v) for v in Y] for Y in planes]

    # --- on the device --------------------------------------------------------
    def index(self):
        import cpd
        if self._dev is None:
            plan = cpd.Plan(self.g)
            assert np.array_equal(plan.order(), self.order)
            self._dev = cpd.Graph(plan, batch=1024)
        ix = cpd.Index.streamed(self._dev, self.targets, int(self.off[-1]), mode="dense")
        ix.append(self.off, self.runs)
        return ix

    def place(self, ix, Y):
        """The one-plane load table Y resident on ix."""
        for k, (s, t, d, _) in enumerate(self.batches([Y])):
            ix.loads(s, t, d, k_moves=1, accumulate=k > 0)
        got = ix.loads_fetch()
        assert got.shape == (1, self.g.m) and got[0].tolist() == [int(v) for v in Y]

    def place_planes(self, ix, planes):
        """A timed table of len(planes) planes resident on ix (which then
        holds that many free-flow weight sets)."""
        K = len(planes)
        ix.set_weight_sets([None] * K)
        for k, (s, t, d, dep) in enumerate(self.batches(planes)):
            ix.timed(s, t, depart=dep, period=PERIOD, demand=d, k_moves=1, loads=True,
                     accumulate=k > 0)
        got = ix.loads_fetch()
        assert got.shape == (K, self.g.m)
        assert got.tolist() == [[int(v) for v in Y] for Y in planes]

    def place_flow(self, ix, X, capacity):
        """The flow table X (m ints below 2^63) resident on ix; the load table
        is left holding the second loading."""
        X = [int(v) for v in X]
        Y1, Y2 = flow_loadings(X)
        ix.flow_clear()
        self.place(ix, Y1)
        ix.flow_step(capacity, lam=0)  # no table: initialises X = Y1 << 16
        self.place(ix, Y2)
        ix.flow_step(capacity, lam=1)
        assert ix.flow_fetch().tolist() == X


def flow_loadings(X):
    """(Y1, Y2) with (Y1 << 16) + (Y2 - Y1) == X."""
    Y1 = [x >> 16 for x in X]
    return Y1, [y + (x & 0xFFFF) for y, x in zip(Y1, X)]
