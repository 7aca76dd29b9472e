"""Pure-Python reference of the conjugate step and the loop around it (cpd_api.h
"The conjugate step", cpd_index_flow_step_conj, cpd_query_assign_conj): Python
ints only, so nothing here can wrap or round.  tests/test_conj_cpu.py pins the
definition by hand-worked values; the GPU tests compare the library with it bit
for bit."""
import numpy as np

from assign_ref import BPR, loop_world, vdf_steps
from flow_ref import LINE, ONE, flow_at, line_rule
from search_loads_ref import ref_search_loads

CONJ = "conj"
ALPHA_MAX = 64881
U32 = 0xFFFFFFFF
LOOP_ITERS = 6


class ConjRange(Exception):
    """A counter of Y at or above 2^30; .edge is the first such edge."""

    def __init__(self, edge):
        super().__init__(f"edge {edge}")
        self.edge = edge


def slope(w0, x, c, a_num, a_den, power):
    """h: the slope of the delay function at volume x, Q16 per unit volume,
    saturating; the header's lines one for one."""
    w0, x, c = int(w0), int(x), int(c)
    r = (1 << 20) if x >= (c << 4) else (x << 16) // c
    q = ONE if power == 1 else r
    for _ in range(power - 2):
        q = (q * r) >> 16
    t = (w0 * q) >> 16
    u = (t * a_num * power) // a_den
    return U32 if u >= (c << 16) else (u << 16) // c


def alpha_rule(N, M):
    """alpha (Q16) of the header's rule from the sums N (signed) and M."""
    Dn = N - M
    if Dn == 0 or N == 0 or (N < 0) != (Dn < 0):
        return 0
    a = ALPHA_MAX if abs(N) >= abs(Dn) else (abs(N) * 65536) // abs(Dn)
    return min(a, ALPHA_MAX)


def ref_conj_step(w0, Y, X, S, capacity, vdf, alpha=CONJ, lam=LINE):
    """One step: (X' and S' as lists of ints, w' u32[m], info).  X None = no
    flow table resident (S is then ignored); S None = no target table: S = X.
    info: alpha_q16, lambda_q16, evals, n, m, gy, xw0, g0, tstt, changed, and D
    (the list the step moved along).  Raises ConjRange for a counter >= 2^30."""
    a_num, a_den, power = vdf
    w0 = [int(v) for v in np.asarray(w0).tolist()]
    Y = [int(v) for v in np.asarray(Y).tolist()]
    cap = [int(v) for v in np.asarray(capacity).tolist()]
    for e, y in enumerate(Y):
        if y >= 1 << 30:
            raise ConjRange(e)
    Yq = [y << 16 for y in Y]

    def w_at(w, x, c):
        return vdf_steps(w, x >> 16, c, a_num, a_den, power, 1)[0]

    init = X is None
    if init:
        X = S = list(Yq)
        al, lam_q, evals, N, M, gy, xw0, g0 = 0, ONE, 0, 0, 0, 0, 0, 0
        D = [0] * len(Y)
    else:
        X = [int(v) for v in X]
        S = list(X) if S is None else [int(v) for v in S]
        N = M = gy = xw0 = 0
        for w, yq, x, s, c in zip(w0, Yq, X, S, cap):
            db, df = (s - x) >> 16, (yq - x) >> 16   # >> on a Python int floors
            if db:
                h = slope(w, x >> 16, c, a_num, a_den, power)
                N += db * df * h
                M += db * db * h
            wx = w_at(w, x, c)
            gy += (yq - x) * wx
            xw0 += x * wx
        al = alpha_rule(N, M) if alpha == CONJ else int(alpha)
        S = [flow_at(yq, s - yq, al) for yq, s in zip(Yq, S)]
        D = [s - x for s, x in zip(S, X)]

        def g(l):
            return sum(d * w_at(w, flow_at(x, d, l), c)
                       for w, d, x, c in zip(w0, D, X, cap) if d)
        g0 = g(0)
        if lam == LINE:
            lam_q, evals = line_rule(lambda l: g0 if l == 0 else g(l))
        else:
            lam_q, evals = int(lam), 1
    Xn = [flow_at(x, d, lam_q) for x, d in zip(X, D)]
    wn = np.array([w_at(w, x, c) for w, x, c in zip(w0, Xn, cap)], np.uint32).reshape(len(Y))
    info = {"alpha_q16": al, "lambda_q16": lam_q, "evals": evals, "n": N, "m": M, "gy": gy,
            "xw0": xw0, "g0": g0,
            "tstt": sum((x >> 16) * int(w) for x, w in zip(Xn, wn.tolist())),
            "changed": sum(int(w) != v for w, v in zip(wn.tolist(), w0)), "D": D}
    return Xn, S, wn, info


INFO_KEYS = ("alpha_q16", "lambda_q16", "evals", "n", "m", "gy", "xw0", "g0", "tstt", "changed")
REC_KEYS = ("finished", "sptt", "moves") + INFO_KEYS


def ref_assign_conj(ref, w_start, s, t, demand, capacity, vdf, iters, **opts):
    """cpd_query_assign_conj over ref_search_loads: (records, X u64[m], S
    u64[m], final weights u32[m], the last search's (cost, plen, fin, stats),
    the last loading u64[m])."""
    w = np.asarray(w_start, np.uint32)
    dem = [1] * len(s) if demand is None else [int(d) for d in demand]
    X = S = None
    recs, last, loads, restart = [], None, None, False
    for k in range(1, iters + 1):
        cost, plen, fin, stats, _, _, loads, moves, _ = ref_search_loads(ref, w, s, t, demand,
                                                                         **opts)
        sptt = sum(d * int(c) for d, c, f in zip(dem, cost.tolist(), fin.tolist()) if f == 1)
        X, S, w, info = ref_conj_step(ref.w_free, loads, X, S, capacity, vdf,
                                      0 if restart else CONJ, LINE)
        info.pop("D")
        recs.append(dict(info, finished=int((fin == 1).sum()), sptt=sptt, moves=moves))
        last = (cost, plen, fin, stats)
        # the conjugate direction went nowhere: a plain step next
        restart = info["lambda_q16"] == 0 and info["alpha_q16"] > 0
        if (k >= 2 and info["lambda_q16"] == 0 and info["alpha_q16"] == 0) or len(s) == 0:
            break
    return recs, np.array(X, np.uint64), np.array(S, np.uint64), w, last, loads


def gaps(recs):
    """-gy / xw0 per record (None where xw0 is 0: the initialising step)."""
    return [(-r["gy"] / r["xw0"]) if r["xw0"] else None for r in recs]


def restart_capacity():
    """loop_world()'s capacities times 50: mild congestion, on which the
    reference loop shows the restart rule and then the early stop
    (test_conj_cpu.py asserts both)."""
    return (loop_world()["capacity"].astype(np.uint64) * 50).astype(np.uint32)


_CACHE = {}


def loop_conj_want(iters=LOOP_ITERS, capacity=None, **opts):
    """ref_assign_conj on assign_ref.loop_world() with its demand, computed
    once per variant.  capacity: other capacities than the world's."""
    wd = loop_world()
    key = (iters, None if capacity is None else np.asarray(capacity).tobytes(),
           tuple(sorted(opts.items())))
    if key not in _CACHE:
        cap = wd["capacity"] if capacity is None else capacity
        _CACHE[key] = ref_assign_conj(wd["ref"], wd["g"].w, wd["s"], wd["t"], wd["demand"], cap,
                                      BPR, iters, **opts)
    return _CACHE[key]
