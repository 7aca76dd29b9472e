"""Pure-Python reference of the flow step and the loop around it (cpd_api.h
"The flow step", cpd_index_flow_step, cpd_query_assign_line): Python ints only,
so nothing here can wrap or round.  tests/test_flow_cpu.py pins the definition
by hand-worked values; the GPU tests compare the library with it bit for bit."""
import numpy as np

from assign_ref import BPR, LOOP_ITERS, loop_world, vdf_steps
from search_loads_ref import ref_search_loads

LINE = "line"
ONE = 1 << 16


class FlowRange(Exception):
    """A counter of Y at or above 2^47; .edge is the first such edge."""

    def __init__(self, edge):
        super().__init__(f"edge {edge}")
        self.edge = edge


def flow_at(X, D, lam):
    """X(lambda) = X + floor(lambda * D / 2^16); >> on a Python int floors."""
    return X + ((lam * D) >> 16)


def g_of(w0, D, X, capacity, vdf, lam):
    """g(lambda) = the sum of D * w(lambda) over the edges."""
    a_num, a_den, power = vdf
    return sum(d * vdf_steps(w, flow_at(x, d, lam) >> 16, c, a_num, a_den, power, 1)[0]
               for w, d, x, c in zip(w0, D, X, capacity) if d)


def line_rule(g):
    """(lambda, evaluations) of the header's procedure over a callable g."""
    if g(0) >= 0:
        return 0, 1
    if g(ONE) < 0:
        return ONE, 2
    lo, hi, evals = 0, ONE, 2
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        evals += 1
        if g(mid) < 0:
            lo = mid
        else:
            hi = mid
    return hi, evals


def ref_flow_step(w0, Y, X, capacity, vdf, lam=LINE):
    """One step: (X' as a list of ints, w' u32[m], info).  X None = no flow
    table resident.  info: lambda_q16, evals, g0, xw0, tstt, changed, and D (the
    list the step moved along).  Raises FlowRange for a counter >= 2^47."""
    a_num, a_den, power = vdf
    w0 = [int(v) for v in np.asarray(w0).tolist()]
    Y = [int(v) for v in np.asarray(Y).tolist()]
    cap = [int(v) for v in np.asarray(capacity).tolist()]
    for e, y in enumerate(Y):
        if y >= 1 << 47:
            raise FlowRange(e)
    init = X is None
    X = [0] * len(Y) if init else [int(v) for v in X]
    D = [(y << 16) - x for y, x in zip(Y, X)]
    if init:
        lam_q, evals, g0, xw0 = ONE, 0, 0, 0
    else:
        g0 = g_of(w0, D, X, cap, vdf, 0)
        xw0 = sum(x * vdf_steps(w, x >> 16, c, a_num, a_den, power, 1)[0]
                  for w, x, c in zip(w0, X, cap))
        if lam == LINE:
            lam_q, evals = line_rule(lambda l: g0 if l == 0 else g_of(w0, D, X, cap, vdf, l))
        else:
            lam_q, evals = int(lam), 1
    Xn = [flow_at(x, d, lam_q) for x, d in zip(X, D)]
    wn = np.array([vdf_steps(w, x >> 16, c, a_num, a_den, power, 1)[0]
                   for w, x, c in zip(w0, Xn, cap)], np.uint32).reshape(len(Y))
    info = {"lambda_q16": lam_q, "evals": evals, "g0": g0, "xw0": xw0,
            "tstt": sum((x >> 16) * int(w) for x, w in zip(Xn, wn.tolist())),
            "changed": sum(int(w) != v for w, v in zip(wn.tolist(), w0)), "D": D}
    return Xn, wn, info


REC_KEYS = ("finished", "sptt", "tstt", "moves", "changed", "lambda_q16", "evals", "g0", "xw0")


def ref_assign_line(ref, w_start, s, t, demand, capacity, vdf, iters, rule=LINE, **opts):
    """cpd_query_assign_line over ref_search_loads: (records, X u64[m], final
    weights u32[m], the last search's (cost, plen, fin, stats), the last
    loading u64[m], the D of every step).  rule = "msa" takes the explicit step
    65536 // k instead of the line rule (MSA restated on the flow table, for the
    gap comparison) and never stops early."""
    w = np.asarray(w_start, np.uint32)
    dem = [1] * len(s) if demand is None else [int(d) for d in demand]
    X, recs, last, loads, Ds = None, [], None, None, []
    for k in range(1, iters + 1):
        cost, plen, fin, stats, _, _, loads, moves, _ = ref_search_loads(ref, w, s, t, demand,
                                                                         **opts)
        sptt = sum(d * int(c) for d, c, f in zip(dem, cost.tolist(), fin.tolist()) if f == 1)
        X, w, info = ref_flow_step(ref.w_free, loads, X, capacity, vdf,
                                   LINE if rule == LINE else ONE // k)
        Ds.append(info.pop("D"))
        recs.append(dict(info, finished=int((fin == 1).sum()), sptt=sptt, moves=moves))
        last = (cost, plen, fin, stats)
        if (rule == LINE and k >= 2 and info["lambda_q16"] == 0) or len(s) == 0:
            break
    return recs, np.array(X, np.uint64), w, last, loads, Ds


def gaps(recs):
    """-g0 / xw0 per record (None where xw0 is 0: the initialising step)."""
    return [(-r["g0"] / r["xw0"]) if r["xw0"] else None for r in recs]


_CACHE = {}


def loop_line_want(iters=LOOP_ITERS, rule=LINE, capacity=None, **opts):
    """ref_assign_line on assign_ref.loop_world() with its demand, computed
    once per variant.  capacity: other capacities than the world's."""
    wd = loop_world()
    key = (iters, rule, None if capacity is None else np.asarray(capacity).tobytes(),
           tuple(sorted(opts.items())))
    if key not in _CACHE:
        cap = wd["capacity"] if capacity is None else capacity
        _CACHE[key] = ref_assign_line(wd["ref"], wd["g"].w, wd["s"], wd["t"], wd["demand"], cap,
                                      BPR, iters, rule, **opts)
    return _CACHE[key]
