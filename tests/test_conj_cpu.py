"""CPU: the conjugate step's definition (tests/conj_ref.py restates cpd_api.h
"The conjugate step", cpd_index_flow_step_conj and cpd_query_assign_conj in
Python ints) pinned by hand-worked values, the conditions on the GPU loop
tests' inputs, and what the new entry points refuse before they touch a
device."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import cpd
from assign_ref import loop_world
from conj_ref import (ALPHA_MAX, CONJ, LOOP_ITERS, ConjRange, alpha_rule, gaps, loop_conj_want,
                      ref_conj_step, restart_capacity, slope)
from flow_ref import LINE, ONE, ref_flow_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cpd_index_flow_step_conj", "cpd_index_target_fetch", "cpd_query_assign_conj")
BPR = (3, 20, 4)


def test_header_and_mirror_declare_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "cpd_api.h")).read()
    declared = set(re.findall(r"\b(cpd_[a-z_]+)\s*\(", hdr))
    assert set(NAMES) <= declared
    for word in ("The conjugate step", "#define CPD_ALPHA_CONJ 0xFFFFFFFFu",
                 "#define CPD_ALPHA_MAX  64881u", "} cpd_conj_info;", "} cpd_assign_conj_iter;",
                 "-gy / xw0", "Out of scope", "bi-conjugate Frank-Wolfe"):
        assert word in hdr, word
    assert "conjugate and bi-conjugate" not in hdr
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "conjugate and bi-conjugate" not in readme and "bi-conjugate" in readme
    so = C.CDLL(cpd.LIB_PATH)
    for name in NAMES:
        assert name in cpd.EXPORTED and getattr(so, name, None) is not None
    for attr in ("flow_step_conj", "target_fetch", "assign_conj", "assign_conj_run"):
        assert callable(getattr(cpd.Index, attr))
    assert cpd.ALPHA_CONJ == 0xFFFFFFFF and cpd.ALPHA_MAX == ALPHA_MAX == 64881
    assert ALPHA_MAX == round(0.99 * 65536)
    # the header's layouts: 3 u32 (+ 4 of padding) + 13 u64 + 3 double;
    # cpd_assign_line_iter's 128 B + u32 (+ 4) + 6 u64
    assert C.sizeof(cpd.ConjInfo) == 144 and cpd.ConjInfo.n_lo.offset == 16
    assert C.sizeof(cpd.AssignConjIter) == 184
    assert cpd.AssignConjIter.alpha_q16.offset == C.sizeof(cpd.AssignLineIter) == 128
    assert cpd.AssignConjIter.n_lo.offset == 136


def test_slope_hand_worked():
    # w0 1000, c 50, a = 3/20: the slope of w0 (1 + a (x / c)^p) is w0 a p (x / c)^(p - 1) / c
    assert slope(1000, 7, 50, 3, 20, 1) == 3 << 16           # u = 150, 150 / 50
    assert slope(1000, 50, 50, 3, 20, 2) == 6 << 16          # r = 1.0: u = 300
    assert slope(1000, 100, 50, 3, 20, 3) == 36 << 16        # r = 2.0, q = 4.0, t = 4000, u = 1800
    assert slope(1000, 100, 50, 3, 20, 4) == 96 << 16        # q = 8.0, t = 8000, u = 4800
    # truncation on the way: x = 75, r = 1.5 = 98304; q = (r * r) >> 16 = 147456; t = 2250;
    # u = 2250 * 9 // 20 = 1012; h = (1012 << 16) // 50
    assert slope(1000, 75, 50, 3, 20, 3) == (1012 << 16) // 50 == 1326448
    # x = 0: power 1 is a constant slope, every other power starts flat
    assert slope(1000, 0, 50, 3, 20, 1) == 3 << 16
    assert [slope(1000, 0, 50, 3, 20, p) for p in (2, 3, 4)] == [0, 0, 0]
    # the clamp of r at 16.0 (x >= 16 c): q = 4096.0, t = 4096000, u = 2457600 < c << 16
    assert slope(1000, 800, 50, 3, 20, 4) == (2457600 << 16) // 50 == 3221225472
    assert slope(1000, 799, 50, 3, 20, 4) < slope(1000, 800, 50, 3, 20, 4)
    assert slope(1000, 10 ** 9, 50, 3, 20, 4) == slope(1000, 800, 50, 3, 20, 4)  # not 0
    # both sides of u == c << 16 (c = 1, a = 1/1, power 1: u = w0)
    assert slope(65535, 3, 1, 1, 1, 1) == 65535 << 16 == 0xFFFF0000
    assert slope(65536, 3, 1, 1, 1, 1) == 0xFFFFFFFF
    assert slope(65537, 3, 1, 1, 1, 1) == 0xFFFFFFFF
    assert slope(0xFFFFFFFF, 1 << 40, 1, 65535, 1, 4) == 0xFFFFFFFF


def test_db_floors_a_negative_difference():
    """One edge, power 1 (h = 3 << 16 whatever x): S - X = -65537 floors to -2,
    Yq - X = -(5 << 16) - 65537 to -7."""
    X = [(10 << 16) + 65537]
    S = [10 << 16]
    Xn, Sn, w, info = ref_conj_step([1000], [5], X, S, [50], (3, 20, 1), CONJ, 0)
    h = 3 << 16
    assert (info["n"], info["m"]) == (14 * h, 4 * h)
    # N > 0 and Dn = 10 h > 0: |N| >= |Dn|, the cap
    assert info["alpha_q16"] == ALPHA_MAX
    assert Sn == [(5 << 16) + ((ALPHA_MAX * (5 << 16)) >> 16)]
    # gy and xw0 under w(0): x = 11, r = 11 * 65536 // 50 = 14417, t = 219, add = 32
    assert info["gy"] == (-(5 << 16) - 65537) * 1032 and info["xw0"] == X[0] * 1032
    assert info["g0"] == (Sn[0] - X[0]) * 1032 and Xn == X and info["lambda_q16"] == 0
    # one unit less and the difference is a multiple of 2^16: db = -1, df = -6
    _, _, _, info = ref_conj_step([1000], [5], [(10 << 16) + 65536], S, [50], (3, 20, 1), 0, 0)
    assert (info["n"], info["m"]) == (6 * h, h)


def test_alpha_rule_branches():
    assert alpha_rule(5, 5) == 0                       # Dn == 0
    assert alpha_rule(0, 7) == 0 and alpha_rule(0, 0) == 0   # N == 0
    assert alpha_rule(5, 9) == 0                       # N > 0 > Dn
    assert alpha_rule(10, 3) == ALPHA_MAX              # |N| >= |Dn|, both positive
    assert alpha_rule(-5, 0) == ALPHA_MAX              # |N| == |Dn|
    # N < 0: alpha = floor(|N| 65536 / (|N| + M)); the cap from below
    assert alpha_rule(-64880, 656) == 64880
    assert alpha_rule(-64881, 655) == 64881
    assert alpha_rule(-64882, 654) == 64881
    assert alpha_rule(-1, 65535) == 1 and alpha_rule(-1, 65536) == 0
    assert alpha_rule(-(1 << 20), 1 << 20) == 32768
    N, M = -((3 << 70) + 12345), (5 << 69) + 99         # past 64 bits
    want = math.floor(Fraction(-N * 65536, M - N))
    assert alpha_rule(N, M) == want == 35746 and 0 < want < ALPHA_MAX
    rng = np.random.default_rng(5)
    for _ in range(500):
        N = -int(rng.integers(1, 1 << 62)) * int(rng.integers(1, 1 << 50))
        M = int(rng.integers(1, 1 << 62)) * int(rng.integers(1, 1 << 50))
        assert alpha_rule(N, M) == min(ALPHA_MAX, math.floor(Fraction(-N * 65536, M - N)))


def test_one_step_hand_worked():
    """Two edges of w0 1000, c 50, power 1 (h = 3 << 16): the flow sits between
    the old target (all on edge 0) and the new loading (all on edge 1)."""
    w0, cap, vdf = [1000, 1000], [50, 50], (3, 20, 1)
    X = [60 << 16, 40 << 16]
    S = [100 << 16, 0]
    Y = [0, 100]
    h = 3 << 16
    Xn, Sn, w, info = ref_conj_step(w0, Y, X, S, cap, vdf, CONJ, 32768)
    # db = (40, -40), df = (-60, 60): N = -4800 h, M = 3200 h, alpha = 0.6 floored
    assert (info["n"], info["m"]) == (-4800 * h, 3200 * h)
    assert info["alpha_q16"] == 4800 * 65536 // 8000 == 39321
    a = 39321
    assert Sn == [(a * (100 << 16)) >> 16, (100 << 16) + ((-a * (100 << 16)) >> 16)]
    assert Sn == [3932100, 2621500]
    # w(0): x = 60: r = 78643, t = 1199, add = 179; x = 40: r = 52428, t = 799, add = 119
    assert info["gy"] == -(60 << 16) * 1179 + (60 << 16) * 1119
    assert info["xw0"] == (60 << 16) * 1179 + (40 << 16) * 1119
    assert info["g0"] == (Sn[0] - X[0]) * 1179 + (Sn[1] - X[1]) * 1119
    assert Xn == [X[0] + ((Sn[0] - X[0]) >> 1), X[1] + ((Sn[1] - X[1]) >> 1)]
    assert (info["lambda_q16"], info["evals"]) == (32768, 1)
    # no target table: S = X, db = 0, alpha 0, the plain step
    Xn, Sn, w, info = ref_conj_step(w0, Y, X, None, cap, vdf, CONJ, 32768)
    assert (info["n"], info["m"], info["alpha_q16"]) == (0, 0, 0)
    assert Sn == [0, 100 << 16] and Xn == [30 << 16, 70 << 16]
    # an explicit alpha skips the rule, the sums are still made
    Xn, Sn, w, info = ref_conj_step(w0, Y, X, S, cap, vdf, ALPHA_MAX, ONE)
    assert (info["n"], info["m"], info["alpha_q16"]) == (-4800 * h, 3200 * h, ALPHA_MAX)
    assert Xn == Sn == [(ALPHA_MAX * (100 << 16)) >> 16,
                        (100 << 16) + ((-ALPHA_MAX * (100 << 16)) >> 16)]


def test_alpha_zero_is_the_flow_step():
    rng = np.random.default_rng(11)
    for trial in range(30):
        m = int(rng.integers(1, 40))
        vdf = (int(rng.integers(0, 50)), int(rng.integers(1, 50)), int(rng.integers(1, 5)))
        w0 = rng.integers(0, 5000, m)
        cap = rng.integers(1, 30, m)
        Y = rng.integers(0, 200, m)
        X = [int(v) for v in rng.integers(0, 200 << 16, m)]
        S = [int(v) for v in rng.integers(0, 200 << 16, m)]
        lam = [LINE, 0, 1, 30000, ONE][trial % 5]
        Xf, wf, fi = ref_flow_step(w0, Y, X, cap, vdf, lam)
        Xc, Sc, wc, ci = ref_conj_step(w0, Y, X, S, cap, vdf, 0, lam)
        assert Xc == Xf and Sc == [int(y) << 16 for y in Y]
        np.testing.assert_array_equal(wc, wf)
        for k in ("lambda_q16", "evals", "g0", "xw0", "tstt", "changed", "D"):
            assert ci[k] == fi[k], (trial, k)
        assert ci["gy"] == ci["g0"] and ci["alpha_q16"] == 0


def test_no_table_initialises_and_the_range():
    w0, Y, cap = [1000, 20, 0], [100, 0, 7], [50, 1, 1]
    for alpha, lam in ((CONJ, LINE), (0, 0), (ALPHA_MAX, 1)):
        Xn, Sn, w, info = ref_conj_step(w0, Y, None, [5, 5, 5], cap, BPR, alpha, lam)
        assert Xn == Sn == [100 << 16, 0, 7 << 16] and w.tolist() == [3400, 20, 0]
        assert [info[k] for k in ("alpha_q16", "lambda_q16", "evals", "n", "m", "gy", "xw0",
                                  "g0")] == [0, ONE, 0, 0, 0, 0, 0, 0]
        assert info["tstt"] == 100 * 3400 and info["changed"] == 1
    ref_conj_step(w0, [0, (1 << 30) - 1, 0], None, None, cap, BPR)
    with pytest.raises(ConjRange) as err:
        ref_conj_step(w0, [0, 1 << 30, 1 << 40], [0, 0, 0], None, cap, BPR)
    assert err.value.edge == 1


def test_loop_inputs_exercise_the_alpha_rule():
    """The condition on the GPU loop test's inputs (assign_ref.loop_world(), BPR,
    LOOP_ITERS = 6 iterations): at least two records with alpha > 0, and at
    least one record k >= 3 with alpha = 0 because N > 0.  Prints the records
    and the gaps -gy / xw0; nothing is asserted about their size."""
    wd = loop_world()
    recs, X, S, w, last, loads = loop_conj_want()
    for k, (r, gap) in enumerate(zip(recs, gaps(recs))):
        print(f"k={k + 1}: alpha {r['alpha_q16']} lambda {r['lambda_q16']} evals {r['evals']} "
              f"n {r['n']} m {r['m']} gap {gap}")
    assert LOOP_ITERS == 6 and len(recs) == LOOP_ITERS
    assert [recs[0][k] for k in ("alpha_q16", "lambda_q16", "evals", "n", "m", "gy", "xw0")] == \
        [0, ONE, 0, 0, 0, 0, 0]
    assert sum(r["alpha_q16"] > 0 for r in recs) >= 2
    assert any(r["alpha_q16"] == 0 and r["n"] > 0 for r in recs[2:])
    assert all(0 < r["alpha_q16"] < ALPHA_MAX for r in recs if r["alpha_q16"])  # mid-range
    assert all(r["finished"] == len(wd["s"]) for r in recs)
    assert all(r["gy"] < 0 and 0 < -r["gy"] <= r["xw0"] for r in recs[1:])
    assert (S != X).any()


def test_loop_early_stop_inputs():
    """At capacities no volume comes near, w' = w0: the second search repeats
    the first, db = 0 and D = 0 everywhere, and the loop stops after record 2
    with lambda = 0 and alpha = 0."""
    huge = np.full(loop_world()["g"].m, 0xFFFFFFFF, np.uint32)
    recs = loop_conj_want(capacity=huge)[0]
    assert len(recs) == 2
    assert [recs[1][k] for k in ("alpha_q16", "lambda_q16", "evals", "n", "m", "gy", "g0")] == \
        [0, 0, 1, 0, 0, 0, 0]


def test_loop_restart_inputs():
    """At 50 times the world's capacities some record k has lambda = 0 with
    alpha > 0 (here the cap, |N| >= |Dn|); record k + 1 is then a plain step
    (alpha = 0, N and M still summed against the kept target), and as its
    lambda is 0 too the loop stops there, short of the 8 iterations asked."""
    recs = loop_conj_want(iters=8, capacity=restart_capacity())[0]
    for k, r in enumerate(recs):
        print(f"k={k + 1}: alpha {r['alpha_q16']} lambda {r['lambda_q16']} n {r['n']} m {r['m']}")
    hits = [k for k, r in enumerate(recs) if r["lambda_q16"] == 0 and r["alpha_q16"] > 0]
    assert hits and hits[0] >= 2 and hits[0] + 1 < len(recs)
    nxt = recs[hits[0] + 1]
    assert nxt["alpha_q16"] == 0 and nxt["m"] > 0 and nxt["n"] != 0
    assert alpha_rule(nxt["n"], nxt["m"]) > 0        # the rule would not have said 0
    assert any(r["alpha_q16"] == ALPHA_MAX for r in recs)
    assert len(recs) < 8 and recs[-1]["lambda_q16"] == 0 and recs[-1]["alpha_q16"] == 0


def test_entry_points_refuse_before_touching_a_device():
    f = cpd.Vdf(3, 20, 4, 1)
    info = cpd.ConjInfo()
    cap = np.ones(4, np.uint32)
    x = np.zeros(4, np.uint64)
    out = (cpd.AssignConjIter * 2)()
    done = C.c_uint32(7)
    L = cpd.lib
    assert L.cpd_index_flow_step_conj(None, cpd._ptr(cap, cpd.u32p), C.byref(f),
                                      C.c_uint32(cpd.ALPHA_CONJ), C.c_uint32(cpd.STEP_LINE),
                                      C.byref(info)) == cpd.CPD_E_ARG
    assert "null index" in L.cpd_last_error().decode()
    assert L.cpd_index_target_fetch(None, cpd._ptr(x, cpd.u64p)) == cpd.CPD_E_ARG
    assert "null index" in L.cpd_last_error().decode()
    assert L.cpd_query_assign_conj(None, None, C.c_uint64(0), None, cpd._ptr(cap, cpd.u32p),
                                   C.byref(f), C.c_uint32(2), out, C.byref(done)) == cpd.CPD_E_ARG
    assert "null argument" in L.cpd_last_error().decode() and done.value == 7
