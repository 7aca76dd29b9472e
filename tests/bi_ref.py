"""Pure-Python reference of the bi-conjugate step and the loop around it
(cpd_api.h "The bi-conjugate step", cpd_index_flow_step_bi,
cpd_query_assign_bi): Python ints only, so nothing here can wrap or round.
Built on conj_ref.py, flow_ref.py and assign_ref.py; branch 1 calls
ref_conj_step.  tests/test_bi_cpu.py pins the definition by hand-worked values;
the GPU tests compare the library with it bit for bit."""
import numpy as np

from assign_ref import BPR, loop_world, vdf_steps
from conj_ref import CONJ, ConjRange, ref_conj_step, slope
from flow_ref import LINE, ONE, flow_at, line_rule
from search_loads_ref import ref_search_loads

AUTO = "auto"
BI_MAX = (1 << 23) - 1
LOOP_ITERS = 8


def quot(a, b):
    """min(floor(a * 65536 / b), BI_MAX) for magnitudes a >= 0, b > 0."""
    return min((a << 16) // b, BI_MAX)


def mu_rule(A2, B2):
    if A2 == 0 or B2 == 0 or (A2 < 0) == (B2 < 0):
        return 0
    return quot(abs(A2), abs(B2))


def nu1_rule(A1, B1):
    return 0 if B1 == 0 or A1 >= 0 else quot(-A1, B1)


def nu_rule(A1, B1, mu, lp):
    return min(nu1_rule(A1, B1) + (mu * lp) // (ONE - lp), BI_MAX)


def betas(mu, nu):
    """(beta0, beta1, beta2): the weights of Yq, S1 and S2, Q16."""
    b0 = (1 << 32) // (ONE + mu + nu)
    b2 = (mu * b0) >> 16
    return b0, ONE - b0 - b2, b2


def d2_of(s1, s2, x, lp):
    return (lp * s1 + (ONE - lp) * s2 - ONE * x) >> 32   # >> on a Python int floors


def new_target(yq, s1, s2, b):
    return (b[0] * yq + b[1] * s1 + b[2] * s2) >> 16


class BiArg(Exception):
    """An explicit nu other than 0 in branch 1."""


INFO_KEYS = ("branch", "mu_q16", "nu_q16", "beta0_q16", "beta1_q16", "beta2_q16", "alpha_q16",
             "lambda_prev_q16", "lambda_q16", "evals", "a1", "b1", "a2", "b2", "gy", "xw0", "g0",
             "tstt", "changed")


def ref_bi_step(w0, Y, state, capacity, vdf, mu=AUTO, nu=AUTO, lam=LINE):
    """One step from state = (X, S1, S2, lambda_prev) — X None: no flow table,
    S1 / S2 None: that table not resident; the lists are ints — to (the new
    state, w' u32[m], info).  Raises ConjRange for a counter >= 2^30 and BiArg
    for an explicit nu > 0 in branch 1."""
    X, S1, S2, lp = state
    a_num, a_den, power = vdf
    branch = 2
    if X is None:
        Xn, Sn, wn, ci = ref_conj_step(w0, Y, None, None, capacity, vdf, 0, lam)
        branch, S2n = 0, None
    elif S1 is None or S2 is None or lp == ONE:
        for e, y in enumerate(np.asarray(Y).tolist()):
            if int(y) >= 1 << 30:
                raise ConjRange(e)
        if nu not in (AUTO, 0):
            raise BiArg(nu)
        Xn, Sn, wn, ci = ref_conj_step(w0, Y, X, S1, capacity, vdf, CONJ if nu == AUTO else 0, lam)
        branch = 1
        S2n = [int(v) for v in (X if S1 is None else S1)]
    if X is None or branch == 1:
        al = ci["alpha_q16"]
        info = dict(branch=branch, mu_q16=0, nu_q16=0, alpha_q16=al, lambda_prev_q16=lp,
                    beta0_q16=ONE - al if branch else 0, beta1_q16=al, beta2_q16=0,
                    a1=ci["n"], b1=ci["m"], a2=0, b2=0)
        for k in ("lambda_q16", "evals", "gy", "xw0", "g0", "tstt", "changed", "D"):
            info[k] = ci[k]
        return (Xn, Sn, S2n, info["lambda_q16"]), wn, info

    w0 = [int(v) for v in np.asarray(w0).tolist()]
    Y = [int(v) for v in np.asarray(Y).tolist()]
    cap = [int(v) for v in np.asarray(capacity).tolist()]
    for e, y in enumerate(Y):
        if y >= 1 << 30:
            raise ConjRange(e)
    Yq = [y << 16 for y in Y]
    X, S1, S2 = ([int(v) for v in T] for T in (X, S1, S2))

    def w_at(w, x, c):
        return vdf_steps(w, x >> 16, c, a_num, a_den, power, 1)[0]

    A1 = B1 = A2 = B2 = gy = xw0 = 0
    for w, yq, x, s1, s2, c in zip(w0, Yq, X, S1, S2, cap):
        d1, df, e21 = (s1 - x) >> 16, (yq - x) >> 16, (s2 - s1) >> 16
        d2 = d2_of(s1, s2, x, lp)
        # the header's range: outside it the library works mod 2^64
        assert max(abs(d1), abs(df), abs(e21), abs(d2)) <= 1 << 30
        if d1 or d2:
            h = slope(w, x >> 16, c, a_num, a_den, power)
            A1 += d1 * df * h
            B1 += d1 * d1 * h
            A2 += d2 * df * h
            B2 += d2 * e21 * h
        wx = w_at(w, x, c)
        gy += (yq - x) * wx
        xw0 += x * wx
    m = mu_rule(A2, B2) if mu == AUTO else int(mu)
    n = nu_rule(A1, B1, m, lp) if nu == AUTO else int(nu)
    b = betas(m, n)
    T = [new_target(yq, s1, s2, b) for yq, s1, s2 in zip(Yq, S1, S2)]
    D = [t - x for t, x in zip(T, X)]

    def g(l):
        return sum(d * w_at(w, flow_at(x, d, l), c) for w, d, x, c in zip(w0, D, X, cap) if d)
    g0 = g(0)
    if lam == LINE:
        lam_q, evals = line_rule(lambda l: g0 if l == 0 else g(l))
    else:
        lam_q, evals = int(lam), 1
    Xn = [flow_at(x, d, lam_q) for x, d in zip(X, D)]
    wn = np.array([w_at(w, x, c) for w, x, c in zip(w0, Xn, cap)], np.uint32).reshape(len(Y))
    info = dict(branch=2, mu_q16=m, nu_q16=n, beta0_q16=b[0], beta1_q16=b[1], beta2_q16=b[2],
                alpha_q16=0, lambda_prev_q16=lp, lambda_q16=lam_q, evals=evals, a1=A1, b1=B1,
                a2=A2, b2=B2, gy=gy, xw0=xw0, g0=g0,
                tstt=sum((x >> 16) * int(w) for x, w in zip(Xn, wn.tolist())),
                changed=sum(int(w) != v for w, v in zip(wn.tolist(), w0)), D=D)
    return (Xn, T, S1, lam_q), wn, info


NO_STATE = (None, None, None, ONE)
REC_KEYS = ("finished", "sptt", "moves") + tuple(k for k in INFO_KEYS if k != "lambda_prev_q16")


def ref_assign_bi(ref, w_start, s, t, demand, capacity, vdf, iters, **opts):
    """cpd_query_assign_bi over ref_search_loads: (records, the final state (X,
    S1, S2, lambda_prev), final weights u32[m], the last search's (cost, plen,
    fin, stats), the last loading u64[m])."""
    w = np.asarray(w_start, np.uint32)
    dem = [1] * len(s) if demand is None else [int(d) for d in demand]
    state, recs, last, loads, restart = NO_STATE, [], None, None, False
    for k in range(1, iters + 1):
        cost, plen, fin, stats, _, _, loads, moves, _ = ref_search_loads(ref, w, s, t, demand,
                                                                         **opts)
        sptt = sum(d * int(c) for d, c, f in zip(dem, cost.tolist(), fin.tolist()) if f == 1)
        state, w, info = ref_bi_step(ref.w_free, loads, state, capacity, vdf,
                                     0 if restart else AUTO, 0 if restart else AUTO, LINE)
        info.pop("D")
        recs.append(dict(info, finished=int((fin == 1).sum()), sptt=sptt, moves=moves))
        last = (cost, plen, fin, stats)
        aimed = info["mu_q16"] > 0 or info["nu_q16"] > 0 or info["alpha_q16"] > 0
        restart = info["lambda_q16"] == 0 and aimed   # the direction went nowhere
        if (k >= 2 and info["lambda_q16"] == 0 and not aimed) or len(s) == 0:
            break
    return recs, state, w, last, loads


def gaps(recs):
    """-gy / xw0 per record (None where xw0 is 0: the initialising step)."""
    return [(-r["gy"] / r["xw0"]) if r["xw0"] else None for r in recs]


def loop_capacity():
    """The capacities of the GPU loop test: loop_world()'s own, on which the
    reference loop shows branch-2 records with mu > 0 and with nu > 0 within
    LOOP_ITERS iterations (test_bi_cpu.py asserts it)."""
    return loop_world()["capacity"]


_CACHE = {}


def loop_bi_want(iters=LOOP_ITERS, capacity=None, **opts):
    """ref_assign_bi on assign_ref.loop_world() with its demand, computed once
    per variant.  capacity: other capacities than loop_capacity()."""
    wd = loop_world()
    key = (iters, None if capacity is None else np.asarray(capacity).tobytes(),
           tuple(sorted(opts.items())))
    if key not in _CACHE:
        cap = loop_capacity() if capacity is None else capacity
        _CACHE[key] = ref_assign_bi(wd["ref"], wd["g"].w, wd["s"], wd["t"], wd["demand"], cap,
                                    BPR, iters, **opts)
    return _CACHE[key]
