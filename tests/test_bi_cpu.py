"""CPU: the bi-conjugate step's definition (tests/bi_ref.py restates cpd_api.h
"The bi-conjugate step", cpd_index_flow_step_bi and cpd_query_assign_bi in
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
from bi_ref import (AUTO, BI_MAX, LOOP_ITERS, NO_STATE, BiArg, betas, d2_of, gaps, loop_bi_want,
                    loop_capacity, mu_rule, new_target, nu1_rule, nu_rule, quot, ref_bi_step)
from conj_ref import CONJ, ConjRange, ref_conj_step, restart_capacity
from flow_ref import LINE, ONE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cpd_index_flow_step_bi", "cpd_index_target2_fetch", "cpd_query_assign_bi")
BPR = (3, 20, 4)
P1 = (3, 20, 1)   # power 1: h = 3 << 16 at w0 1000, c 50, whatever x
H = 3 << 16


def test_header_and_mirror_declare_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "cpd_api.h")).read()
    declared = set(re.findall(r"\b(cpd_[a-z0-9_]+)\s*\(", hdr))
    assert set(NAMES) <= declared
    for word in ("The bi-conjugate step", "#define CPD_BI_AUTO 0xFFFFFFFFu",
                 "#define CPD_BI_MAX  8388607u", "} cpd_bi_info;", "} cpd_assign_bi_iter;",
                 "Branch 0", "Branch 1", "Branch 2", "beta1 is\n * never negative"):
        assert word in hdr, word
    # no longer out of scope, in the header or the README
    scope = hdr[hdr.index("Out of scope"):hdr.index("typedef struct cpd_assign_iter")]
    assert "bi-conjugate Frank-Wolfe" not in scope
    readme = open(os.path.join(ROOT, "README.md")).read()
    scope = readme[readme.index("Out of scope"):readme.index("**the line-search step**")]
    assert "bi-conjugate" not in scope and "cpd_index_flow_step_bi" in readme
    so = C.CDLL(cpd.LIB_PATH)
    for name in NAMES:
        assert name in cpd.EXPORTED + cpd.EXPORTED_MORE and getattr(so, name, None) is not None
    for attr in ("flow_step_bi", "target2_fetch", "assign_bi", "assign_bi_run"):
        assert callable(getattr(cpd.Index, attr))
    assert cpd.BI_AUTO == 0xFFFFFFFF and cpd.BI_MAX == BI_MAX == 8388607 == (1 << 23) - 1
    # the header's layouts: 10 u32 + 17 u64 + 3 double; cpd_assign_line_iter's
    # 128 B + 7 u32 (+ 4 of padding) + 10 u64
    assert C.sizeof(cpd.BiInfo) == 40 + 136 + 24 and cpd.BiInfo.a1_lo.offset == 40
    assert cpd.AssignBiIter.branch.offset == C.sizeof(cpd.AssignLineIter) == 128
    assert cpd.AssignBiIter.a1_lo.offset == 160 and C.sizeof(cpd.AssignBiIter) == 240


def test_d2_floors_a_negative_bracket():
    # lp = 0.25: the bracket is 16384 S1 + 49152 S2 - 65536 X
    assert d2_of(8 << 16, 4 << 16, 5 << 16, 16384) == 0       # exactly 0
    assert d2_of(8 << 16, 4 << 16, (5 << 16) + 1, 16384) == -1  # bracket -65536: floor(-2^-16)
    assert d2_of(8 << 16, 4 << 16, 6 << 16, 16384) == -1      # bracket -(1 << 32) exactly
    assert d2_of(8 << 16, 4 << 16, (6 << 16) + 1, 16384) == -2
    assert d2_of(8 << 16, 4 << 16, 4 << 16, 16384) == 1
    assert d2_of(8 << 16, 4 << 16, (4 << 16) - 1, 16384) == 1
    # lp = 1: the bracket is S1 + 65535 S2 - 65536 X, just short of S2 - X
    assert d2_of(0, 10 << 16, 3 << 16, 1) == 6 and d2_of(0, 3 << 16, 10 << 16, 1) == -8
    # magnitudes at the top of the header's range stay below 2^63
    top = (1 << 46) - 1
    assert abs(ONE * top) < 1 << 63 and d2_of(0, 0, top, 65535) == -(1 << 30)
    assert d2_of(top, top, 0, 30000) == (ONE * top) >> 32 == (1 << 30) - 1


def test_mu_and_nu1_zero_and_sign_cases():
    assert mu_rule(0, 5) == 0 and mu_rule(5, 0) == 0 and mu_rule(0, 0) == 0
    assert mu_rule(5, 7) == 0 and mu_rule(-5, -7) == 0               # the same sign
    assert mu_rule(-5, 10) == 32768 and mu_rule(5, -10) == 32768     # 0.5
    assert mu_rule(-10, 5) == 2 << 16 and mu_rule(-1, 3) == 21845    # an integer part; a floor
    assert nu1_rule(-5, 0) == 0 and nu1_rule(0, 9) == 0 and nu1_rule(4, 9) == 0
    assert nu1_rule(-3, 4) == 49152 and nu1_rule(-9, 4) == (2 << 16) + 16384
    # past 64 bits
    A, B = -((3 << 90) + 12345), (5 << 83) + 99
    want = math.floor(Fraction(-A * 65536, B))
    assert nu1_rule(A, B) == mu_rule(A, B) == mu_rule(-A, -B) == want and 76 << 16 < want < 77 << 16


def test_nu_takes_the_lp_term():
    # nu = nu1 + floor(mu lp / (65536 - lp))
    assert nu_rule(-3, 4, 0, 40000) == 49152
    assert nu_rule(5, 4, 65536, 32768) == 65536                      # lp = 0.5: mu itself
    assert nu_rule(-3, 4, 65536, 16384) == 49152 + 21845             # lp = 0.25: mu / 3, floored
    assert nu_rule(0, 0, 100, 65535) == 6553500                      # lp one short of 1 ...
    assert nu_rule(0, 0, 100, 0) == 0                                # ... and lp = 0
    assert nu_rule(0, 0, 129, 65535) == BI_MAX                       # 8454015 saturates
    assert nu_rule(0, 0, 128, 65535) == 128 * 65535 == 8388480


def test_saturation_at_bi_max():
    assert quot(127, 1) == 127 << 16 and quot(128, 1) == BI_MAX and quot(1 << 100, 3) == BI_MAX
    # the last quotient below 2^23 and the first at it: a = 128 b - 1, 128 b
    b = (1 << 70) + 7
    assert quot(128 * b - 1, b) == BI_MAX == (1 << 23) - 1   # 127.99..: floor is 2^23 - 1 unsaturated
    assert ((128 * b - 1) << 16) // b == BI_MAX and ((128 * b) << 16) // b == BI_MAX + 1
    assert quot(128 * b, b) == BI_MAX
    assert mu_rule(-(1 << 123), 1) == BI_MAX and nu1_rule(-(1 << 123), 1) == BI_MAX
    assert nu_rule(-(1 << 123), 1, BI_MAX, 65535) == BI_MAX
    # 2^32 // (65536 + 2 (2^23 - 1)) = 255; (8388607 * 255) >> 16 = 32639
    assert betas(BI_MAX, BI_MAX) == (255, 32642, 32639)


def test_betas_sum_to_one_and_beta1_is_never_negative():
    assert betas(0, 0) == (ONE, 0, 0)
    assert betas(0, ONE) == (32768, 32768, 0) and betas(ONE, 0) == (32768, 0, 32768)
    assert betas(ONE, ONE) == (21845, 21846, 21845)
    for mu in range(0, 300):
        for nu in range(0, 300):
            b0, b1, b2 = betas(mu, nu)
            assert b0 + b1 + b2 == ONE and min(b0, b1, b2) >= 0, (mu, nu)
    rng = np.random.default_rng(9)
    draws = [(int(m), int(n)) for m, n in rng.integers(0, BI_MAX + 1, (20000, 2))]
    draws += [(BI_MAX, 0), (0, BI_MAX), (BI_MAX, 1), (1, BI_MAX), (BI_MAX - 1, BI_MAX)]
    for mu, nu in draws:
        b0, b1, b2 = betas(mu, nu)
        assert b0 + b1 + b2 == ONE and min(b0, b1, b2) >= 0, (mu, nu)
        assert b0 == (1 << 32) // (ONE + mu + nu) and b2 == (mu * b0) >> 16


def test_target_is_the_loading_at_mu_nu_zero():
    for yq, s1, s2 in ((5 << 16, 123456789, 987654321), (0, (1 << 46) - 1, 1), (7, 0, 0)):
        assert new_target(yq, s1, s2, betas(0, 0)) == yq
    # and the sum is formed exactly before the one shift: three remainders of 2/3 make 2
    b = betas(ONE, ONE)
    assert b == (21845, 21846, 21845)
    assert new_target(3, 3, 3, b) == 3 and new_target(1, 2, 4, b) == (21845 + 43692 + 87380) >> 16 == 2


def two_edges(lp=16384):
    """Two edges of w0 1000, c 50, power 1: the flow between two old targets
    and the new loading."""
    w0, cap = [1000, 1000], [50, 50]
    X = [60 << 16, 40 << 16]
    S1 = [100 << 16, 0]
    S2 = [20 << 16, 80 << 16]
    Y = [0, 100]
    return w0, cap, Y, (X, S1, S2, lp)


def test_one_step_hand_worked():
    w0, cap, Y, st = two_edges()
    (Xn, T, S2n, lpn), w, info = ref_bi_step(w0, Y, st, cap, P1, AUTO, AUTO, 32768)
    # d1 = (40, -40), df = (-60, 60), e21 = (-80, 80)
    # d2 = 0.25 S1 + 0.75 S2 - X = (25 + 15 - 60, 0 + 60 - 40) = (-20, 20)
    assert info["branch"] == 2 and info["lambda_prev_q16"] == 16384 and info["alpha_q16"] == 0
    assert (info["a1"], info["b1"]) == (-4800 * H, 3200 * H)
    assert (info["a2"], info["b2"]) == (2400 * H, 3200 * H)
    # A2 and B2 of the same sign: mu = 0; nu1 = 4800 / 3200 = 1.5; the lp term is 0
    assert (info["mu_q16"], info["nu_q16"]) == (0, 98304)
    # beta0 = 2^32 // 163840 = 26214 (0.4), beta2 = 0, beta1 = 39322
    assert [info[k] for k in ("beta0_q16", "beta1_q16", "beta2_q16")] == [26214, 39322, 0]
    assert T == [(39322 * (100 << 16)) >> 16, (26214 * (100 << 16)) >> 16] == [3932200, 2621400]
    assert S2n == st[1] and lpn == 32768 == info["lambda_q16"] and info["evals"] == 1
    assert Xn == [st[0][0] + ((T[0] - st[0][0]) >> 1), st[0][1] + ((T[1] - st[0][1]) >> 1)]
    # w(0) as in the conjugate step's hand-worked case: 1179 and 1119
    assert info["gy"] == -(60 << 16) * 1179 + (60 << 16) * 1119
    assert info["xw0"] == (60 << 16) * 1179 + (40 << 16) * 1119
    assert info["g0"] == (T[0] - st[0][0]) * 1179 + (T[1] - st[0][1]) * 1119
    # S2 beyond S1 on edge 0: A2 < 0 < B2
    w0, cap, Y, (X, S1, S2, lp) = two_edges()
    S2 = [180 << 16, 0]
    # d2 = (25 + 135 - 60, 0 + 0 - 40) = (100, -40); e21 = (80, 0); df = (-60, 60)
    _, _, info = ref_bi_step(w0, Y, (X, S1, S2, lp), cap, P1, AUTO, AUTO, 0)
    assert (info["a2"], info["b2"]) == ((-6000 - 2400) * H, 8000 * H)
    assert info["mu_q16"] == 8400 * 65536 // 8000 == 68812                  # 1.05
    assert info["nu_q16"] == 98304 + 68812 * 16384 // 49152 == 98304 + 22937
    b0 = (1 << 32) // (ONE + 68812 + 121241)
    assert [info[k] for k in ("beta0_q16", "beta2_q16")] == [b0, (68812 * b0) >> 16] == [16804, 17643]
    assert info["beta1_q16"] == ONE - 16804 - 17643
    # explicit mu, explicit nu, each alone: the rule fills in the other from it
    for mu, nu, want in ((1000, AUTO, (1000, 98304 + 333)), (AUTO, 777, (68812, 777)),
                         (5, 6, (5, 6)), (0, 0, (0, 0)),
                         (BI_MAX, AUTO, (BI_MAX, 98304 + 2796202))):
        _, _, info = ref_bi_step(w0, Y, (X, S1, S2, lp), cap, P1, mu, nu, 0)
        assert (info["mu_q16"], info["nu_q16"]) == want, (mu, nu)
        assert (info["a2"], info["b2"]) == (-8400 * H, 8000 * H)              # still made


def test_branches_0_and_1():
    w0, cap, Y, (X, S1, S2, lp) = two_edges()
    # branch 0: no flow table, whatever else is passed
    for mu, nu, lam in ((AUTO, AUTO, LINE), (7, 9, 0)):
        (Xn, Sn, S2n, lpn), w, info = ref_bi_step(w0, Y, (None, S1, S2, 5), cap, P1, mu, nu, lam)
        assert Xn == Sn == [0, 100 << 16] and S2n is None and lpn == ONE
        assert {k: info[k] for k in ("branch", "mu_q16", "nu_q16", "beta0_q16", "beta1_q16",
                                     "beta2_q16", "alpha_q16", "evals", "a1", "b1", "a2", "b2",
                                     "gy", "xw0", "g0")} == \
            dict(branch=0, mu_q16=0, nu_q16=0, beta0_q16=0, beta1_q16=0, beta2_q16=0, alpha_q16=0,
                 evals=0, a1=0, b1=0, a2=0, b2=0, gy=0, xw0=0, g0=0)
        assert info["lambda_q16"] == ONE
    # branch 1 for each reason: the conjugate step, and S2 takes the S it read
    for state, s_read in (((X, S1, None, 16384), S1), ((X, S1, S2, ONE), S1),
                          ((X, None, None, ONE), X)):
        (Xn, Sn, S2n, lpn), w, info = ref_bi_step(w0, Y, state, cap, P1, 12345, AUTO, LINE)
        Xc, Sc, wc, ci = ref_conj_step(w0, Y, X, state[1], cap, P1, CONJ, LINE)
        assert (Xn, Sn) == (Xc, Sc) and S2n == s_read and lpn == ci["lambda_q16"]
        np.testing.assert_array_equal(w, wc)
        al = ci["alpha_q16"]
        assert info["branch"] == 1 and info["alpha_q16"] == al and info["mu_q16"] == info["nu_q16"] == 0
        assert (info["a1"], info["b1"], info["a2"], info["b2"]) == (ci["n"], ci["m"], 0, 0)
        assert [info[k] for k in ("beta0_q16", "beta1_q16", "beta2_q16")] == [ONE - al, al, 0]
        for k in ("lambda_q16", "evals", "gy", "xw0", "g0", "tstt", "changed"):
            assert info[k] == ci[k]
    assert al == 0 and ref_conj_step(w0, Y, X, S1, cap, P1)[3]["alpha_q16"] == 39321
    # an explicit nu of 0 is alpha 0; any other is refused
    (_, Sn, _, _), _, info = ref_bi_step(w0, Y, (X, S1, None, 7), cap, P1, AUTO, 0, LINE)
    assert info["alpha_q16"] == 0 and Sn == [0, 100 << 16] and info["b1"] == 3200 * H
    with pytest.raises(BiArg):
        ref_bi_step(w0, Y, (X, S1, None, 7), cap, P1, AUTO, 1, LINE)
    # the range, in every branch
    for state in (NO_STATE, (X, S1, None, 7), (X, S1, S2, 7)):
        with pytest.raises(ConjRange) as err:
            ref_bi_step(w0, [5, 1 << 30], state, cap, P1)
        assert err.value.edge == 1
        ref_bi_step(w0, [5, (1 << 30) - 1], state, cap, P1, AUTO, AUTO, 0)


def test_loop_inputs_reach_branch_2_with_mu_and_nu():
    """The condition the GPU loop test relies on: on loop_world() with
    loop_capacity() the reference loop has, within LOOP_ITERS = 8 iterations, at
    least one branch-2 record with mu > 0 and one with nu > 0.  Prints the
    records and the gaps -gy / xw0; nothing is asserted about their size."""
    wd = loop_world()
    assert LOOP_ITERS == 8 and np.array_equal(loop_capacity(), wd["capacity"])
    recs, state, w, last, loads = loop_bi_want()
    for k, (r, gap) in enumerate(zip(recs, gaps(recs))):
        print(f"k={k + 1}: branch {r['branch']} mu {r['mu_q16']} nu {r['nu_q16']} alpha "
              f"{r['alpha_q16']} lambda {r['lambda_q16']} evals {r['evals']} gap {gap}")
    assert len(recs) == LOOP_ITERS and [r["branch"] for r in recs[:3]] == [0, 1, 2]
    assert any(r["branch"] == 2 and r["mu_q16"] > 0 for r in recs)
    assert any(r["branch"] == 2 and r["nu_q16"] > 0 for r in recs)
    assert any(r["branch"] == 2 and r["mu_q16"] > 0 and r["nu_q16"] > 0 for r in recs)
    assert all(r["beta0_q16"] + r["beta1_q16"] + r["beta2_q16"] == ONE for r in recs[1:])
    assert all(r["finished"] == len(wd["s"]) for r in recs)
    assert all(r["gy"] < 0 and 0 < -r["gy"] <= r["xw0"] for r in recs[1:])
    X, S1, S2, lp = state
    assert S2 is not None and X != S1 and S1 != S2 and lp == recs[-1]["lambda_q16"]


def test_loop_restart_and_early_stop_inputs():
    """At 50 times the world's capacities some record k has lambda = 0 with mu
    or nu > 0; record k + 1 then has mu = nu = 0 although the sums would have
    said otherwise, and the loop stops short of the 12 iterations asked at a
    record with lambda = 0 and mu = nu = alpha = 0.  At capacities no volume
    comes near it stops after record 2, in branch 1."""
    recs = loop_bi_want(iters=12, capacity=restart_capacity())[0]
    for k, r in enumerate(recs):
        print(f"k={k + 1}: branch {r['branch']} mu {r['mu_q16']} nu {r['nu_q16']} lambda "
              f"{r['lambda_q16']}")
    hits = [k for k, r in enumerate(recs) if r["lambda_q16"] == 0 and (r["mu_q16"] or r["nu_q16"])]
    assert hits and hits[0] + 1 < len(recs)
    nxt = recs[hits[0] + 1]
    assert nxt["branch"] == 2 and (nxt["mu_q16"], nxt["nu_q16"]) == (0, 0)
    assert mu_rule(nxt["a2"], nxt["b2"]) > 0 or nu1_rule(nxt["a1"], nxt["b1"]) > 0
    last = recs[-1]
    assert len(recs) < 12 and (last["lambda_q16"], last["mu_q16"], last["nu_q16"],
                               last["alpha_q16"]) == (0, 0, 0, 0)
    huge = np.full(loop_world()["g"].m, 0xFFFFFFFF, np.uint32)
    recs = loop_bi_want(capacity=huge)[0]
    assert len(recs) == 2 and recs[1]["branch"] == 1
    assert [recs[1][k] for k in ("alpha_q16", "lambda_q16", "evals", "a1", "b1", "gy", "g0")] == \
        [0, 0, 1, 0, 0, 0, 0]


def test_entry_points_refuse_before_touching_a_device():
    f = cpd.Vdf(3, 20, 4, 1)
    info = cpd.BiInfo()
    cap = np.ones(4, np.uint32)
    x = np.zeros(4, np.uint64)
    out = (cpd.AssignBiIter * 2)()
    done = C.c_uint32(7)
    L = cpd.lib
    A = C.c_uint32(cpd.BI_AUTO)
    assert L.cpd_index_flow_step_bi(None, cpd._ptr(cap, cpd.u32p), C.byref(f), A, A,
                                    C.c_uint32(cpd.STEP_LINE), C.byref(info)) == cpd.CPD_E_ARG
    assert "null index" in L.cpd_last_error().decode()
    assert L.cpd_index_target2_fetch(None, cpd._ptr(x, cpd.u64p)) == cpd.CPD_E_ARG
    assert "null index" in L.cpd_last_error().decode()
    assert L.cpd_query_assign_bi(None, None, C.c_uint64(0), None, cpd._ptr(cap, cpd.u32p),
                                 C.byref(f), C.c_uint32(2), out, C.byref(done)) == cpd.CPD_E_ARG
    assert "null argument" in L.cpd_last_error().decode() and done.value == 7
