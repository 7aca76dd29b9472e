"""Pure-Python reference of the assignment loop (cpd_api.h "The delay
function", cpd_index_weights_from_loads, cpd_query_assign): Python ints only,
so nothing here can wrap.  tests/test_assign_cpu.py pins the definition by
hand-worked values; the GPU tests compare the library with it bit for bit."""
import numpy as np

from search_loads_ref import ref_search_loads

U32 = 0xFFFFFFFF
BPR = (3, 20, 4)


def vdf_steps(w0, L, c, a_num, a_den, power, load_div):
    """(w', x, every intermediate value) of the delay function, as the header
    states it line for line."""
    w0, L, c = int(w0), int(L), int(c)
    x = L // load_div
    r = (1 << 20) if x >= (c << 4) else (x << 16) // c
    mids = [x, c << 4, x << 16 if x < (c << 4) else 0, r]
    p = r
    for _ in range(power - 1):
        mids.append(p * r)
        p = (p * r) >> 16
    mids.append(w0 * p)
    t = (w0 * p) >> 16
    mids.append(t * a_num)
    add = (t * a_num) // a_den
    mids += [p, t, add]
    return min(w0 + add, U32), x, mids


def vdf_ref(w0, L, c, a_num, a_den, power, load_div):
    return vdf_steps(w0, L, c, a_num, a_den, power, load_div)[0]


def ref_weights_from_loads(w0, loads, capacity, a_num, a_den, power, load_div):
    """One plane: (w' u32[m], tstt, changed) with tstt = sum of x * w' over the
    edges, a Python int, and changed = the edges with w' != w0."""
    out = np.empty(len(w0), np.uint32)
    tstt = changed = 0
    for e, (w, L, c) in enumerate(zip(np.asarray(w0).tolist(), np.asarray(loads).tolist(),
                                      np.asarray(capacity).tolist())):
        wn, x, _ = vdf_steps(w, L, c, a_num, a_den, power, load_div)
        out[e] = wn
        tstt += x * wn
        changed += wn != w
    return out, tstt, changed


def ref_assign(ref, w_start, s, t, demand, capacity, vdf, iters, **opts):
    """cpd_query_assign over ref_search_loads: (records, summed loads u64[m],
    final weights u32[m], the last search's (cost, plen, fin, stats)).  vdf =
    (a_num, a_den, power); records hold finished, sptt, tstt, moves, changed."""
    a_num, a_den, power = vdf
    w = np.asarray(w_start, np.uint32)
    total = np.zeros(len(ref.dst), np.uint64)
    dem = [1] * len(s) if demand is None else [int(d) for d in demand]
    recs, last = [], None
    for k in range(1, iters + 1):
        cost, plen, fin, stats, _, _, loads, moves, _ = ref_search_loads(ref, w, s, t, demand,
                                                                         **opts)
        total = total + loads
        sptt = sum(d * int(c) for d, c, f in zip(dem, cost.tolist(), fin.tolist()) if f == 1)
        w, tstt, changed = ref_weights_from_loads(ref.w_free, total, capacity, a_num, a_den,
                                                  power, k)
        recs.append({"finished": int((fin == 1).sum()), "sptt": sptt, "tstt": tstt,
                     "moves": moves, "changed": changed})
        last = (cost, plen, fin, stats)
    return recs, total, w, last


# The loop test's world, shared by test_assign_cpu.py (which checks, without a
# GPU, that the second iteration's loading differs from the first's: without
# that the loop test shows nothing about feedback) and test_gpu_assign.py.
LOOP_NQ = 300
LOOP_ITERS = 4
_LOOP = {}


def loop_world():
    """graphs.GRAPHS["synth"] (synth_road_graph(40, 30)), 40 targets, LOOP_NQ
    queries, a random demand of 1..9 and per-edge capacities of 1..60 (some of
    them 1): a dict, built once."""
    if _LOOP:
        return _LOOP
    import cpd
    import oracle
    from search_paths_ref import SearchPathsRef
    g = cpd.synth_road_graph(40, 30, seed=7)
    order = oracle.dfs_preorder(g.row_ptr, g.dst)
    rng = np.random.default_rng(17)
    targets = rng.choice(g.n, size=40, replace=False).astype(np.uint32)
    s = rng.integers(0, g.n, LOOP_NQ).astype(np.uint32)
    t = targets[rng.integers(0, len(targets), LOOP_NQ)]
    s[0] = t[0]  # a query with s == t
    off, runs = oracle.build_rows(g.row_ptr, g.dst, g.w, order, targets)
    capacity = rng.integers(1, 61, g.m).astype(np.uint32)
    capacity[:8] = 1
    _LOOP.update(g=g, order=order, targets=targets, s=s, t=t, off=off, runs=runs,
                 demand=rng.integers(1, 10, LOOP_NQ).astype(np.uint32), capacity=capacity,
                 ref=SearchPathsRef(g, order, targets, off, runs), cache={})
    return _LOOP


def loop_want(demand=True, warm=None, iters=LOOP_ITERS, **opts):
    """ref_assign on loop_world(), computed once per variant.  warm: the
    starting weights (None: free flow)."""
    wd = loop_world()
    key = (demand, None if warm is None else warm.tobytes(), iters, tuple(sorted(opts.items())))
    if key not in wd["cache"]:
        wd["cache"][key] = ref_assign(wd["ref"], wd["g"].w if warm is None else warm, wd["s"],
                                      wd["t"], wd["demand"] if demand else None, wd["capacity"],
                                      BPR, iters, **opts)
    return wd["cache"][key]
