"""Seeded test graphs shared by the CPU and GPU suites."""
import numpy as np

import cpd


def graph_from_edges(n, edges):
    """edges: list of (a, b, w) in file order."""
    rp = np.zeros(n + 1, np.uint32)
    for a, _, _ in edges:
        rp[a + 1] += 1
    rp = np.cumsum(rp).astype(np.uint32)
    pos = rp[:-1].copy()
    dst = np.zeros(len(edges), np.uint32)
    w = np.zeros(len(edges), np.uint32)
    for a, b, c in edges:
        dst[pos[a]] = b
        w[pos[a]] = c
        pos[a] += 1
    return cpd.RoadGraph(rp, dst, w)


def irregular_graph():
    """Unreachable pairs, a degree-15 node, a self loop, parallel and 0-weight edges."""
    rng = np.random.default_rng(5)
    n = 300
    edges = []
    for a in range(n):
        k = 15 if a == 17 else int(rng.integers(0, 5))
        for _ in range(k):
            b = int(rng.integers(0, n))
            edges.append((a, b, int(rng.integers(0, 4))))
    edges.append((3, 3, 1))        # self loop
    edges.append((5, 9, 2))        # parallel edge pair
    edges.append((5, 9, 1))
    edges = [e for e in edges if not (e[1] >= 290)]   # nodes 290.. are never entered
    return graph_from_edges(n, edges)


def deg8_graph():
    """Out-degrees 5..8 on a ring (8-bit first-move sets), weights 1..3 (ties)."""
    rng = np.random.default_rng(8)
    n = 400
    edges = []
    for a in range(n):
        edges.append((a, (a + 1) % n, int(rng.integers(1, 4))))   # strongly connected ring
        for _ in range(int(rng.integers(4, 8))):
            edges.append((a, int(rng.integers(0, n)), int(rng.integers(1, 4))))
    return graph_from_edges(n, edges)


def ring2_graph():
    """Out-degree <= 2 (a two-way ring with a few chords removed: 2-slot
    adjacency, the shift-1 kernels), weights 1..5."""
    rng = np.random.default_rng(2)
    n = 500
    edges = []
    for a in range(n):
        edges.append((a, (a + 1) % n, int(rng.integers(1, 6))))
        if a % 7:
            edges.append((a, (a - 1) % n, int(rng.integers(1, 6))))
    return graph_from_edges(n, edges)


def tie_graph():
    """Tiny weights -> many equal-cost paths (multi-bit first-move sets)."""
    g = cpd.synth_road_graph(24, 24, seed=11)
    return cpd.RoadGraph(g.row_ptr, g.dst, (g.w % 3 + 1).astype(np.uint32), g.x, g.y)


def _path_edges(n, rng, wmax):
    """A bidirectional path 0-1-...-(n-1), weights 1..wmax, in node order."""
    edges = []
    for v in range(n):
        if v > 0:
            edges.append((v, v - 1, int(rng.integers(1, wmax + 1))))
        if v + 1 < n:
            edges.append((v, v + 1, int(rng.integers(1, wmax + 1))))
    return edges


def chain_graph(n, seed):
    """A bidirectional path 0-1-...-(n-1), weights 1..3: every row has a
    handful of runs, each spanning thousands of columns — far past the
    chunked RLE count's 16-column look-back guess."""
    return graph_from_edges(n, _path_edges(n, np.random.default_rng(seed), 3))


# The graphs below leave the out-degree <= 4 path (8- and 16-bit first-move
# sets, 4-bit moves) at sizes of several 2048-column tiles.  They are not in
# GRAPHS: that would multiply the whole parametrised suite and the pure-Python
# CPU checks.  Tests name them directly; test_oracle_cpu.py pins what the GPU
# tests rely on (degree band, tile count, runs per row).

def lattice_wide(w, h, dmax, seed):
    """A 4-neighbour w x h lattice (strongly connected); about 30% of the
    nodes get extra out-edges, up to out-degree dmax, to nodes within +-3
    cells.  Weights 1..29: many runs per row (no long stretch shares a move)."""
    rng = np.random.default_rng(seed)
    edges = []
    for y in range(h):
        for x in range(w):
            a = y * w + x
            nb = [(x + dx, y + dy) for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1))
                  if 0 <= x + dx < w and 0 <= y + dy < h]
            for bx, by in nb:
                edges.append((a, by * w + bx, int(rng.integers(1, 30))))
            if rng.random() < 0.3:
                near = [(bx, by) for bx in range(max(0, x - 3), min(w, x + 4))
                        for by in range(max(0, y - 3), min(h, y + 4)) if (bx, by) != (x, y)]
                extra = int(rng.integers(1, dmax - len(nb) + 1))
                for i in rng.choice(len(near), size=extra, replace=False):
                    edges.append((a, near[i][1] * w + near[i][0], int(rng.integers(1, 30))))
    return graph_from_edges(w * h, edges)


def chain_hub(n, hub_deg, seed):
    """chain_graph plus one node (n // 2) of out-degree hub_deg, its extra
    edges to random far endpoints: the hub sets the whole graph's first-move
    set width, the rows stay a handful of runs spanning thousands of columns."""
    rng = np.random.default_rng(seed)
    edges = _path_edges(n, rng, 3)
    hub = n // 2
    for b in rng.choice(n, size=hub_deg - 2, replace=False):
        edges.append((hub, int(b), int(rng.integers(1, 4))))
    return graph_from_edges(n, edges)


def comb(n, every, dmax, reach, seed):
    """chain_graph's path with every `every`-th node given 3..dmax-2 extra
    out-edges within +-reach, weights 1..199: runs of a few to a few dozen
    columns, stretches with and without breaks alternating inside one tile."""
    rng = np.random.default_rng(seed)
    edges = _path_edges(n, rng, 3)
    for a in range(every // 2, n, every):
        for _ in range(int(rng.integers(3, dmax - 1))):
            b = a
            while b == a:
                b = int(rng.integers(max(0, a - reach), min(n, a + reach + 1)))
            edges.append((a, b, int(rng.integers(1, 200))))
    return graph_from_edges(n, edges)


# dmax -> (lowest out-degree, first-move set bits, bits per move)
BAND = {2: (2, 4, 1), 4: (3, 4, 2), 8: (5, 8, 4), 15: (9, 16, 4)}
BAND_REACH = 40
BAND_TAIL = 80


def band(n, dmax, seed):
    """A one-way ring a -> (a + 1) % n (strongly connected at any n >= 2) with
    every node's out-degree in the band of one adjacency width: exactly 2 for
    dmax = 2, 3..4, 5..8 and 9..15 for dmax = 4, 8 and 15.  The extra edges go
    to distinct nodes within +-BAND_REACH positions; weights 1..29, so rows
    hold many short runs (lattice_wide's reasoning).  A graph of any n at any
    width: what the size-edge tests need (tests/test_gpu_size_edges.py).

    The ring edge is every node's last edge, the one the DFS preorder follows
    first: column == node id.  One node among the first 32 and one among the
    last 32 get out-degree dmax itself.  From 2 * BAND_TAIL nodes on, the last
    BAND_TAIL nodes all have out-degree dmax, a ring edge of weight 1 and
    extra edges that go backwards only.  No edge from before the tail lands
    in its last BAND_TAIL - BAND_REACH nodes, so towards a target just past
    the wrap those take the ring edge, move dmax - 1 in every one of them: such
    rows end in a single run over the whole last 32-column segment — while
    towards the targets behind them the same nodes pick among their extra
    edges, and rows end in a run that starts at column n - 1."""
    lo = BAND[dmax][0]
    assert n >= 2 and min(n - 1, BAND_REACH) >= dmax - 1
    rng = np.random.default_rng(seed)
    tail = n - BAND_TAIL if n >= 2 * BAND_TAIL else n
    deg = rng.integers(lo, dmax + 1, n)
    deg[int(rng.integers(0, min(32, n)))] = dmax
    deg[n - 1 - int(rng.integers(0, min(32, n)))] = dmax
    deg[tail:] = dmax
    edges = []
    for a in range(n):
        near = sorted({(a + d) % n for d in range(-BAND_REACH, 0 if a >= tail else BAND_REACH + 1)}
                      - {a})
        for i in rng.choice(len(near), size=int(deg[a]) - 1, replace=False):
            edges.append((a, near[i], int(rng.integers(1, 30))))
        edges.append((a, (a + 1) % n, 1 if a >= tail else int(rng.integers(1, 30))))
    return graph_from_edges(n, edges)


# The size-edge cases of tests/test_gpu_size_edges.py: column counts on and
# one off the 32-column segment and the 2048-column tile, at every adjacency
# width.  test_oracle_cpu.py pins, from the oracle alone, what the GPU tests
# rely on.  Not in GRAPHS, for the reason above.
EDGE_N = (31, 32, 33, 2047, 2048, 2049, 4095, 4096, 4097)
EDGE_DMAX = (2, 4, 8, 15)
EDGE_TARGETS = 1100


def edge_graph(n, dmax):
    return band(n, dmax, seed=100 * n + dmax)


def edge_targets(order, k=EDGE_TARGETS):
    """min(n, k) shuffled nodes that always hold the nodes at columns 0, 1,
    n - 2 and n - 1 (order[node] = column)."""
    n = len(order)
    col_node = np.argsort(order)
    forced = np.unique(col_node[[0, 1, n - 2, n - 1]])
    rng = np.random.default_rng(n)
    rest = rng.permutation(n)
    rest = rest[~np.isin(rest, forced)][:max(0, min(n, k) - len(forced))]
    t = np.concatenate([forced, rest]).astype(np.uint32)
    rng.shuffle(t)
    return t


def edge_queries(order, targets, nq):
    """nq seeded (source, target) pairs over `targets`; the first six have the
    nodes at columns 0 and n - 1 as source and as target, in every pairing."""
    n = len(order)
    col_node = np.argsort(order)
    rng = np.random.default_rng(2)
    s = rng.integers(0, n, nq).astype(np.uint32)
    t = targets[rng.integers(0, len(targets), nq)].copy()
    first, last = col_node[0], col_node[n - 1]
    s[:6] = [first, last, first, last, first, last]
    t[:4] = [last, first, first, last]
    return s, t


# name -> (graph, first-move set bits, 2048-column tiles, targets the GPU test builds)
WIDE = {
    "lattice8": (lambda: lattice_wide(80, 80, 8, seed=8), 8, 4, 2500),
    "lattice15": (lambda: lattice_wide(80, 80, 15, seed=15), 16, 4, 2500),
    "hub8": (lambda: chain_hub(34000, 8, seed=8), 8, 17, 300),
    "hub12": (lambda: chain_hub(34000, 12, seed=12), 16, 17, 300),
    "comb8": (lambda: comb(10000, 53, 8, 300, seed=8), 8, 5, 400),
    "comb15": (lambda: comb(10000, 53, 15, 300, seed=15), 16, 5, 400),
}


def wide_targets(name, g):
    """The shuffled targets the GPU tests build for WIDE[name]."""
    return np.random.default_rng(1).permutation(g.n).astype(np.uint32)[:WIDE[name][3]]


# Range and level-1 edge graphs (test_host_cpu.py pins what the GPU tests of
# test_gpu_range_edges.py rely on).  Not in GRAPHS, for the reason above.

def scaled_to_bound(g0, limit):
    """g0 with every weight x floor(limit / dist_bound of g0): the plan's
    distance bound lands just under `limit` (the factor is applied in u64)."""
    bound1 = cpd.Plan(g0, hierarchy=False).info()["dist_bound"]
    scale = int(limit) // int(bound1)
    w = g0.w.astype(np.uint64) * np.uint64(scale)
    assert scale >= 1 and int(w.max()) <= 0xFFFFFFFF
    return cpd.RoadGraph(g0.row_ptr, g0.dst, w.astype(np.uint32), g0.x, g0.y)


TOP_LIMIT = 0xFFFFFFFD  # the largest bound at which narrow rows stay on

# strongly connected graphs whose distance bound is just under TOP_LIMIT
TOP = {
    "synth": lambda: scaled_to_bound(cpd.synth_road_graph(40, 40, seed=12), TOP_LIMIT),
    "deg8": lambda: scaled_to_bound(deg8_graph(), TOP_LIMIT),
    # ... and edges whose w + d(head) wraps past 2^32 (deg8_heavy_graph)
    "deg8heavy": lambda: scaled_to_bound(deg8_heavy_graph(), TOP_LIMIT),
}


def deg8_heavy_graph():
    """deg8_graph's construction, the last chord of every node made heavy: its
    weight is the distance bound of the graph without these chords, less 1.
    No shortest path takes one, so distances and bound stay what they were —
    but w + d(head) passes the bound for most (heavy edge, target) pairs:
    scaled to the top of the range, those adds wrap past 2^32 (on the scaled
    deg8_graph and synth graph no edge's add can: the largest w + d(head)
    over all targets is 0xD2D2D2C4 and 0xA15A8628)."""
    rng = np.random.default_rng(8)
    n = 400
    light, heavy = [], []
    for a in range(n):
        light.append((a, (a + 1) % n, int(rng.integers(1, 4))))
        k = int(rng.integers(4, 8))
        for i in range(k):
            e = (a, int(rng.integers(0, n)), int(rng.integers(1, 4)))
            (heavy if i == k - 1 else light).append(e)
    bound = cpd.Plan(graph_from_edges(n, light), hierarchy=False).info()["dist_bound"]
    return graph_from_edges(n, light + [(a, b, bound - 1) for a, b, _ in heavy])


def two_cycle(a):
    """0 -> 1 of weight a, 1 -> 0 of weight 1: the distance bound is a."""
    return graph_from_edges(2, [(0, 1, a), (1, 0, 1)])


def stars(nh, seed):
    """A one-way ring of nh hubs (nodes 0..nh-1, weights 1..8), each hub with
    0..6 pendant nodes joined to it both ways (weights 1..8).  Ring edges
    first, then the pendants in hub order.  The pendants are contracted first
    (level 0), so a hub with many of them is a level-1 node whose leaf arcs
    are its out-arcs to them — up to 6, and a 7th when the next hub of the
    ring is a leaf of the hierarchy too."""
    rng = np.random.default_rng(seed)
    edges = [(h, (h + 1) % nh, int(rng.integers(1, 9))) for h in range(nh)]
    n = nh
    for h in range(nh):
        for _ in range(int(rng.integers(0, 7))):
            edges.append((h, n, int(rng.integers(1, 9))))
            edges.append((n, h, int(rng.integers(1, 9))))
            n += 1
    return graph_from_edges(n, edges)


def wide_level1(ch):
    """Nodes of an exported hierarchy at sweep level 1 with more than 4
    down-arcs, and each one's down-arc count."""
    cnt = np.diff(ch["dn_off"].astype(np.int64))
    v = np.nonzero((ch["level_up"] == 1) & (cnt > 4))[0]
    return v, cnt[v]


# Contraction gadgets: witness searches with many targets on graphs that
# contract in a fraction of a second (tests/test_gpu_ch_edges.py;
# test_ch_edges_cpu.py pins, from the host plan alone, what the GPU tests rely
# on).  Not in GRAPHS, for the reason above.

def ch_hub(n0, D, Din, seed, wmax=3):
    """chain_graph's path (weights 1..wmax) whose middle node, the hub, has
    out-degree exactly D (D - 2 extra arcs to distinct chain nodes) and Din
    extra in-arcs from chain nodes outside its out-list.  The hub is contracted
    last, so its searches are simulations: one per in-neighbour, with D targets
    from an extra in-neighbour (D - 1 from a path neighbour).  wmax = 2: most
    targets tie on their via weight.  Returns (graph, hub)."""
    rng = np.random.default_rng(seed)
    edges = _path_edges(n0, rng, wmax)
    hub = n0 // 2
    far = np.array([x for x in range(n0) if abs(x - hub) > 1])
    pick = rng.choice(far, size=D - 2 + Din, replace=False)
    for b in pick[:D - 2]:
        edges.append((hub, int(b), int(rng.integers(1, wmax + 1))))
    for a in pick[D - 2:]:
        edges.append((int(a), hub, int(rng.integers(1, wmax + 1))))
    return graph_from_edges(n0, edges), hub


def ch_fan(n0, D, F, seed, wmax=3):
    """chain_graph's path (weights 1..wmax) and F fan nodes n0 .. n0 + F - 1.
    Fan f has one in-arc, from chain node u_f with weight 1, and D out-arcs of
    weight 10 to distinct chain nodes x more than one position from u_f; a
    direct arc u_f -> x of weight 1..wmax witnesses every one of them.  A fan
    needs no shortcut (edge difference -(D + 1)): it is contracted early, all
    D out-neighbours still there — one contraction search of exactly D
    targets, all tied on via = 11 — and u_f keeps out-degree D + 3.  Returns
    (graph, fan node ids)."""
    rng = np.random.default_rng(seed)
    edges = _path_edges(n0, rng, wmax)
    fans = np.arange(n0, n0 + F)
    for f in range(F):
        u = (f + 1) * n0 // (F + 1)
        far = np.array([x for x in range(n0) if abs(x - u) > 1])
        edges.append((u, n0 + f, 1))
        for x in rng.choice(far, size=D, replace=False):
            edges.append((n0 + f, int(x), 10))
            edges.append((u, int(x), int(rng.integers(1, wmax + 1))))
    return graph_from_edges(n0 + F, edges), fans


# the degrees test_gpu_ch_edges.py runs: one below, on and one past the lane
# workspace's 32 targets and the wave kernel's 64 and 128, and far past them
CH_FAN_D = (31, 32, 33, 64, 65, 128, 129, 300)
CH_HUB_D = (33, 65, 129, 300)
CH_TIE_D = (65, 300)
CH_LANE_EDGE_D = (32, 33)   # hubs, with every search started in the lane kernel


def ch_fan_case(D, wmax=3):
    return ch_fan(1000, D, 3, seed=D, wmax=wmax)


def ch_hub_case(D, wmax=3):
    return ch_hub(1000, D, 1, seed=D, wmax=wmax)


def ch_hub_two_way():
    return ch_hub(2000, 300, 300, seed=7)


GRAPHS = {
    "synth": lambda: cpd.synth_road_graph(40, 30, seed=7),
    "ties": tie_graph,
    "irregular": irregular_graph,
    "deg8": deg8_graph,
    "ring2": ring2_graph,
    "single": lambda: graph_from_edges(1, []),
}
