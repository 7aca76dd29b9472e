"""CPU: the flow step's definition (tests/flow_ref.py restates cpd_api.h "The
flow step", cpd_index_flow_step and cpd_query_assign_line in Python ints)
pinned by hand-worked values, the condition on the GPU loop test's inputs, and
what the new entry points refuse before they touch a device."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import cpd
from assign_ref import LOOP_ITERS, loop_world, vdf_ref
from flow_ref import (LINE, ONE, FlowRange, flow_at, g_of, gaps, line_rule, loop_line_want,
                      ref_flow_step)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cpd_index_flow_step", "cpd_index_flow_fetch", "cpd_index_flow_clear",
         "cpd_query_assign_line")
BIG = 0xFFFFFFFF  # a capacity no volume here comes near: w' = w0


def test_header_and_mirror_declare_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "cpd_api.h")).read()
    declared = set(re.findall(r"\b(cpd_[a-z_]+)\s*\(", hdr))
    assert set(NAMES) <= declared
    for word in ("The flow step", "#define CPD_STEP_LINE 0xFFFFFFFFu", "} cpd_flow_info;",
                 "} cpd_assign_line_iter;", "-g0 / xw0", "from ONE record"):
        assert word in hdr, word
    assert not re.search(r"line search, Frank-Wolfe and other step rules", hdr)
    so = C.CDLL(cpd.LIB_PATH)
    for name in NAMES:
        assert name in cpd.EXPORTED and getattr(so, name, None) is not None
    for attr in ("flow_step", "flow_fetch", "flow_clear", "assign_line", "assign_line_run"):
        assert callable(getattr(cpd.Index, attr))
    assert cpd.STEP_LINE == 0xFFFFFFFF
    # the header's layouts: 2 u32 + 7 u64 + 2 double; cpd_assign_iter's 80 B + 2 u32 + 4 u64 + double
    assert C.sizeof(cpd.FlowInfo) == 80 and C.sizeof(cpd.AssignLineIter) == 128
    assert cpd.AssignLineIter.lambda_q16.offset == C.sizeof(cpd.AssignIter) == 80
    assert cpd._s128(2 ** 64 - 1, 2 ** 64 - 1) == -1 and cpd._s128(5, 0) == 5
    assert cpd._s128(0, 1 << 63) == -(1 << 127)


def test_flow_at_hand_worked():
    # D > 0, not a multiple of 2^16: D = 10 * 65536 - 1
    X, D = (10 << 16) + 1, 655359
    assert flow_at(X, D, 0) == X
    assert flow_at(X, D, 1) == X + 9              # 655359 / 65536 = 9.99998
    assert flow_at(X, D, 65535) == X + 655349     # D - 9.99998 = 655349.00002
    assert flow_at(X, D, ONE) == X + D == 20 << 16
    # D < 0: the floor goes toward minus infinity
    X, D = (20 << 16) + 1, -655361
    assert flow_at(X, D, 0) == X
    assert flow_at(X, D, 1) == X - 11             # -10.000015 floors to -11
    assert flow_at(X, D, 65535) == X - 655351     # -(655361 - 10.000015) = -655350.99998
    assert flow_at(X, D, ONE) == X + D == 10 << 16
    # X(lambda) stays between X and Y << 16, whatever the sign
    rng = np.random.default_rng(3)
    for _ in range(2000):
        x = int(rng.integers(0, 1 << 63, dtype=np.uint64))
        y = int(rng.integers(0, 1 << 47, dtype=np.uint64)) << 16
        lam = int(rng.integers(0, ONE + 1))
        got = flow_at(x, y - x, lam)
        assert min(x, y) <= got <= max(x, y)
        assert got == x + math.floor(Fraction(lam * (y - x), 65536))


def test_product_beyond_64_bits():
    X = (1 << 62) + 12345
    D = -X                                        # Y = 0
    lam = 40000
    assert abs(lam * D) >= 1 << 77
    want = X + math.floor(Fraction(lam * D, 65536))
    assert flow_at(X, D, lam) == want and 0 < want < X
    # the largest counter the step accepts, from X = 0
    D = ((1 << 47) - 1) << 16
    assert 65535 * D >= 1 << 78
    assert flow_at(0, D, 65535) == math.floor(Fraction(65535 * D, 65536))
    # one step of the reference over both, D taking both signs (a_num = 0: w' = w0)
    Xn, w, info = ref_flow_step([7, 9], [0, (1 << 47) - 1], [X, 0], [BIG, BIG], (0, 1, 1), lam)
    assert Xn == [want, flow_at(0, D, lam)] and info["g0"] == -X * 7 + D * 9
    assert info["xw0"] == X * 7


def test_one_step_hand_worked():
    """Two edges of w0 1000, c 50 (BPR): volume 100 on edge 0 steps half way
    towards volume 100 on edge 1."""
    w0, cap, vdf = [1000, 1000], [50, 50], (3, 20, 4)
    X = [100 << 16, 0]
    Y = [0, 100]
    Xn, w, info = ref_flow_step(w0, Y, X, cap, vdf, 32768)
    assert Xn == [50 << 16, 50 << 16]
    assert w.tolist() == [1150, 1150]             # x = c: w0 * 3 // 20 is added
    # g(0) = D . w(0) = -(100 << 16) * 3400 + (100 << 16) * 1000   (x = 2 c: w = 3400)
    assert info["g0"] == (100 << 16) * (1000 - 3400)
    assert info["xw0"] == (100 << 16) * 3400
    assert info["tstt"] == 2 * 50 * 1150 and info["changed"] == 2
    assert (info["lambda_q16"], info["evals"]) == (32768, 1)
    assert -info["g0"] / info["xw0"] == pytest.approx(2400 / 3400)
    for lam in (0, 1, 65535, ONE):
        Xn, w, info = ref_flow_step(w0, Y, X, cap, vdf, lam)
        assert Xn == [flow_at(100 << 16, -(100 << 16), lam), flow_at(0, 100 << 16, lam)]
        assert w.tolist() == [vdf_ref(1000, x >> 16, 50, 3, 20, 4, 1) for x in Xn]
    assert ref_flow_step(w0, Y, X, cap, vdf, 1)[0] == [(100 << 16) - 100, 100]
    assert ref_flow_step(w0, Y, X, cap, vdf, 0)[0] == X


def test_line_rule_branches():
    vdf = (3, 20, 4)
    # 1: g(0) >= 0 — the flow sits on the cheap edge, the loading on the dear one
    Xn, w, info = ref_flow_step([10, 1000], [0, 5], [5 << 16, 0], [BIG, BIG], vdf, LINE)
    assert info["g0"] == (5 << 16) * 990 and (info["lambda_q16"], info["evals"]) == (0, 1)
    assert Xn == [5 << 16, 0]
    # ... and g(0) == 0 exactly: the flow is the loading (3 edges)
    Xn, w, info = ref_flow_step([3, 4, 5], [1, 2, 3], [1 << 16, 2 << 16, 3 << 16], [1, 1, 1], vdf)
    assert (info["g0"], info["lambda_q16"], info["evals"]) == (0, 0, 1)
    # 2: g(65536) < 0 — the other way round: the whole step is taken
    Xn, w, info = ref_flow_step([10, 1000], [5, 0], [0, 5 << 16], [BIG, BIG], vdf, LINE)
    assert info["g0"] == -(5 << 16) * 990 and (info["lambda_q16"], info["evals"]) == (ONE, 2)
    assert Xn == [5 << 16, 0]
    # 3: two equal parallel edges: the flow splits in the middle
    w0, cap = [100, 100], [10, 10]
    X, Y = [20 << 16, 0], [0, 20]
    Xn, w, info = ref_flow_step(w0, Y, X, cap, vdf, LINE)
    lam = info["lambda_q16"]
    assert info["evals"] == 18 and 0 < lam < ONE
    D = [-(20 << 16), 20 << 16]
    assert g_of(w0, D, X, cap, vdf, lam) >= 0 > g_of(w0, D, X, cap, vdf, lam - 1)
    assert abs(lam - 32768) <= 3277 and w[0] == w[1]  # within one unit of volume of the middle
    # 3 again on 4 edges with unequal capacities and an edge nothing moves on
    w0, cap = [100, 120, 50, 7], [10, 30, 5, 1]
    X, Y = [30 << 16, (2 << 16) + 77, 0, 9 << 16], [0, 12, 20, 9]
    Xn, w, info = ref_flow_step(w0, Y, X, cap, vdf, LINE)
    lam, D = info["lambda_q16"], info["D"]
    assert D[3] == 0 and Xn[3] == 9 << 16 and sum(d < 0 for d in D) == 1
    assert info["evals"] == 18 and 0 < lam < ONE
    assert g_of(w0, D, X, cap, vdf, lam) >= 0 > g_of(w0, D, X, cap, vdf, lam - 1)
    # the procedure itself, on a step function: the first lambda with g >= 0
    for edge in (1, 2, 777, 32768, 65535, ONE):
        assert line_rule(lambda l: -1 if l < edge else 0) == (edge, 18)
    assert line_rule(lambda l: 5) == (0, 1) and line_rule(lambda l: -5) == (ONE, 2)


def test_no_table_initialises():
    w0, Y, cap = [1000, 20, 0], [100, 0, 7], [50, 1, 1]
    for lam in (LINE, 0, 1, ONE):
        Xn, w, info = ref_flow_step(w0, Y, None, cap, (3, 20, 4), lam)
        assert Xn == [100 << 16, 0, 7 << 16] and w.tolist() == [3400, 20, 0]
        assert (info["lambda_q16"], info["evals"], info["g0"], info["xw0"]) == (ONE, 0, 0, 0)
        assert info["tstt"] == 100 * 3400 and info["changed"] == 1
    # the range check: 2^47 - 1 passes, 2^47 names its edge
    ref_flow_step(w0, [0, (1 << 47) - 1, 0], None, cap, (3, 20, 4))
    with pytest.raises(FlowRange) as err:
        ref_flow_step(w0, [0, 1 << 47, 1 << 50], None, cap, (3, 20, 4))
    assert err.value.edge == 1


def test_loop_inputs_exercise_the_line_rule():
    """The condition on the GPU loop test's inputs (assign_ref.loop_world(),
    LOOP_ITERS iterations at fscale 0): some iteration k >= 2 takes a step
    strictly inside 0..65536 that is not MSA's 65536 // k, and some slot has D <
    0.  Prints the relative gap -g0 / xw0 per iteration under the line rule and
    under MSA's step (nothing is asserted about which is smaller: four
    iterations on 300 queries prove nothing about convergence)."""
    wd = loop_world()
    recs, X, w, last, loads, Ds = loop_line_want()
    msa = loop_line_want(rule="msa")[0]
    for name, rs in (("line", recs), ("msa", msa)):
        for k, (r, gap) in enumerate(zip(rs, gaps(rs))):
            print(f"{name} k={k + 1}: lambda {r['lambda_q16']} evals {r['evals']} gap {gap} "
                  f"sptt {r['sptt']} tstt {r['tstt']}")
    assert len(recs) == LOOP_ITERS and len(Ds) == LOOP_ITERS
    assert (recs[0]["lambda_q16"], recs[0]["evals"], recs[0]["g0"], recs[0]["xw0"]) == (ONE, 0, 0, 0)
    assert any(0 < r["lambda_q16"] < ONE and r["lambda_q16"] != ONE // (k + 1)
               for k, r in enumerate(recs) if k >= 1)
    assert any(d < 0 for D in Ds for d in D)
    assert all(r["finished"] == len(wd["s"]) for r in recs)
    # X is the flow the weights were made from, and it carries every trip's volume
    assert [int(v) for v in w.tolist()] == [vdf_ref(a, int(x) >> 16, c, 3, 20, 4, 1) for a, x, c in
                                            zip(wd["g"].w.tolist(), X.tolist(), wd["capacity"].tolist())]
    assert recs[1]["g0"] < 0 and 0 < -recs[1]["g0"] <= recs[1]["xw0"]


def test_entry_points_refuse_before_touching_a_device():
    f = cpd.Vdf(3, 20, 4, 1)
    info = cpd.FlowInfo()
    cap = np.ones(4, np.uint32)
    x = np.zeros(4, np.uint64)
    out = (cpd.AssignLineIter * 2)()
    done = C.c_uint32(7)
    L = cpd.lib
    assert L.cpd_index_flow_step(None, cpd._ptr(cap, cpd.u32p), C.byref(f),
                                 C.c_uint32(cpd.STEP_LINE), C.byref(info)) == cpd.CPD_E_ARG
    assert "null index" in L.cpd_last_error().decode()
    assert L.cpd_index_flow_fetch(None, cpd._ptr(x, cpd.u64p)) == cpd.CPD_E_ARG
    assert "null index" in L.cpd_last_error().decode()
    assert L.cpd_index_flow_clear(None) == cpd.CPD_E_ARG
    assert L.cpd_query_assign_line(None, None, C.c_uint64(0), None, cpd._ptr(cap, cpd.u32p),
                                   C.byref(f), C.c_uint32(2), out, C.byref(done)) == cpd.CPD_E_ARG
    assert "null argument" in L.cpd_last_error().decode() and done.value == 7
