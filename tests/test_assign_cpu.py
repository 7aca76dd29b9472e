"""CPU: the assignment loop's definition (tests/assign_ref.py restates cpd_api.h
"The delay function", cpd_index_weights_from_loads and cpd_query_assign in
Python ints) pinned by hand-worked values and by its own properties, the
condition on the GPU loop test's inputs, and what the new entry points refuse
before they touch a device."""
import ctypes as C
import os
import re

import numpy as np

import cpd
from assign_ref import (BPR, U32, loop_want, loop_world, ref_assign, ref_weights_from_loads,
                        vdf_ref, vdf_steps)
from search_loads_ref import ref_search_loads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cpd_index_weights_from_loads", "cpd_index_get_weights", "cpd_index_get_weight_sets",
         "cpd_query_assign")


def test_header_and_mirror_declare_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "cpd_api.h")).read()
    declared = set(re.findall(r"\b(cpd_[a-z_]+)\s*\(", hdr))
    assert set(NAMES) <= declared
    for word in ("typedef struct cpd_vdf {", "} cpd_vdf_info;", "} cpd_assign_iter;",
                 "The delay function", "Out of scope", "relative gap"):
        assert word in hdr, word
    so = C.CDLL(cpd.LIB_PATH)
    for name in NAMES:
        assert name in cpd.EXPORTED and getattr(so, name, None) is not None
    for attr in ("weights_from_loads", "get_weights", "get_weight_sets", "assign", "assign_run"):
        assert callable(getattr(cpd.Index, attr))
    assert C.sizeof(cpd.Vdf) == 16 and C.sizeof(cpd.VdfInfo) == 40
    assert C.sizeof(cpd.AssignIter) == 80


def test_vdf_hand_worked():
    # BPR at x = c: r = 1.0 (65536), p = 65536, t = w0, add = w0 * 3 // 20
    assert vdf_ref(1000, 50, 50, 3, 20, 4, 1) == 1150
    # x = 2 c, power 4: p = 16.0, add = 1000 * 16 * 3 // 20 = 2400
    assert vdf_ref(1000, 100, 50, 3, 20, 4, 1) == 3400
    # x = c / 2, power 2: r = 32768, p = 16384 (0.25), t = 250, add = 250 * 3 // 20 = 37
    assert vdf_ref(1000, 25, 50, 3, 20, 2, 1) == 1037
    # load_div: x = 7 // 2 = 3; c = 4: r = 3 * 65536 // 4 = 49152; power 1: t = 750
    assert vdf_ref(1000, 7, 4, 1, 1, 1, 2) == 1750
    # truncation of r: x = 1, c = 3: r = 21845, power 1, w0 = 3: t = 65535 >> 16 = 0
    assert vdf_ref(3, 1, 3, 1, 1, 1, 1) == 3
    # L = 0, w0 = 0, a_num = 0: nothing is added
    assert vdf_ref(77, 0, 1, 65535, 1, 4, 1) == 77
    assert vdf_ref(0, 10 ** 12, 1, 65535, 1, 4, 1) == 0
    assert vdf_ref(77, 10 ** 12, 1, 0, 1, 4, 1) == 77
    # the clamp: x >= 16 c gives r = 16.0 whatever x; power 4: p = 2^32
    assert vdf_ref(10, 16 * 5, 5, 1, 1, 4, 1) == 10 + 10 * 65536
    assert vdf_ref(10, 2 ** 64 - 1, 5, 1, 1, 4, 1) == 10 + 10 * 65536


def test_vdf_monotone_in_load():
    rng = np.random.default_rng(1)
    for _ in range(300):
        w0 = int(rng.integers(0, 1 << 32))
        c = int(rng.integers(1, 1 << int(rng.integers(1, 33))))
        a_num, a_den = int(rng.integers(0, 65536)), int(rng.integers(1, 65536))
        power, div = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        loads = sorted(int(x) for x in rng.integers(0, 40 * c * div, 30))
        ws = [vdf_ref(w0, L, c, a_num, a_den, power, div) for L in loads]
        assert all(a <= b for a, b in zip(ws, ws[1:]))
        assert all(w >= w0 for w in ws)


def test_vdf_clamp_is_continuous():
    """Just below x = 16 c the ratio is just below 16.0, never above it."""
    for c in (1, 3, 1000, 0xFFFFFFFF):
        for power in (1, 2, 3, 4):
            below = vdf_steps(1 << 20, 16 * c - 1, c, 3, 20, power, 1)
            at = vdf_steps(1 << 20, 16 * c, c, 3, 20, power, 1)
            above = vdf_steps(1 << 20, 16 * c + 1, c, 3, 20, power, 1)
            assert below[2][3] <= (1 << 20) == at[2][3] == above[2][3]
            assert (1 << 20) - below[2][3] <= (1 << 16) // c + 1  # one step of x below 16.0
            assert below[0] <= at[0] == above[0]


def test_vdf_saturates():
    assert vdf_ref(U32, 16, 1, 65535, 1, 4, 1) == U32
    assert vdf_ref(U32, 2 ** 64 - 1, 1, 65535, 1, 4, 1) == U32
    assert vdf_ref(U32 - 1, 1, 1, 1, 1, 1, 1) == U32  # w0 + w0 clamps, does not wrap
    assert vdf_ref(1 << 31, 1, 1, 1, 1, 1, 1) == U32
    assert vdf_ref((1 << 31) - 1, 1, 1, 1, 1, 1, 1) == U32 - 1


def test_vdf_intermediates_fit_64_bits():
    rng = np.random.default_rng(2)
    ends = {"w0": (0, 1, U32), "L": (0, 1, 2 ** 64 - 1), "c": (1, 2, U32), "a_num": (0, 65535),
            "a_den": (1, 65535), "power": (1, 4), "div": (1, U32)}
    cases = [(w0, L, c, an, ad, p, d) for w0 in ends["w0"] for L in ends["L"] for c in ends["c"]
             for an in ends["a_num"] for ad in ends["a_den"] for p in ends["power"]
             for d in ends["div"]]
    for _ in range(3000):
        bits = int(rng.integers(1, 65))
        cases.append((int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << bits, dtype=np.uint64)),
                      int(rng.integers(1, 1 << int(rng.integers(1, 33)))),
                      int(rng.integers(0, 65536)), int(rng.integers(1, 65536)),
                      int(rng.integers(1, 5)), int(rng.integers(1, 1 << int(rng.integers(1, 33))))))
    for case in cases:
        w, x, mids = vdf_steps(*case)
        assert all(0 <= v < 2 ** 64 for v in mids), case
        assert mids[-3] <= 2 ** 32 and case[0] <= w <= U32, case  # p, w'


def test_ref_weights_from_loads_sums():
    w0 = np.array([10, 20, 30, 0], np.uint32)
    loads = np.array([0, 40, 5, 9], np.uint64)
    cap = np.array([1, 20, 10, 1], np.uint32)
    w, tstt, changed = ref_weights_from_loads(w0, loads, cap, 3, 20, 4, 1)
    # edge 1: x = 2 c: add = 20 * 16 * 3 // 20 = 48; edge 2: x = c / 2: p = 4096, t = 1, add = 0
    assert w.tolist() == [10, 68, 30, 0]
    assert tstt == 40 * 68 + 5 * 30 and changed == 1


def test_ref_assign_first_iteration_is_search_loads():
    wd = loop_world()
    recs, total, w, last = ref_assign(wd["ref"], wd["g"].w, wd["s"], wd["t"], wd["demand"],
                                      wd["capacity"], BPR, 1)
    r = ref_search_loads(wd["ref"], wd["g"].w, wd["s"], wd["t"], wd["demand"])
    np.testing.assert_array_equal(total, r[6])
    np.testing.assert_array_equal(last[0], r[0])
    assert recs[0]["moves"] == r[7] and recs[0]["finished"] == int(r[2].sum())
    assert recs[0]["sptt"] == sum(int(d) * int(c) for d, c in zip(wd["demand"], r[0]))
    want = ref_weights_from_loads(wd["g"].w, r[6], wd["capacity"], *BPR, 1)
    np.testing.assert_array_equal(w, want[0])
    assert (recs[0]["tstt"], recs[0]["changed"]) == want[1:]


def test_loop_inputs_give_feedback():
    """On the GPU loop test's graph and capacity the second iteration loads
    other edges than the first: the weights the first update wrote are felt."""
    wd = loop_world()
    assert int(wd["capacity"].min()) == 1
    one = loop_want(iters=1)
    two = loop_want(iters=2)
    first, second = one[1], two[1] - one[1]
    assert first.any() and (first != second).any()
    assert one[0][0]["changed"] > 100
    four = loop_want()
    assert [r["finished"] for r in four[0]] == [len(wd["s"])] * 4
    assert len({r["sptt"] for r in four[0]}) == 4  # every iteration searched other weights


def test_entry_points_refuse_before_touching_a_device():
    f = cpd.Vdf(3, 20, 4, 1)
    info = cpd.VdfInfo()
    cap = np.ones(4, np.uint32)
    w = np.zeros(4, np.uint32)
    k = C.c_uint32()
    out = (cpd.AssignIter * 2)()
    L = cpd.lib
    assert L.cpd_index_weights_from_loads(None, cpd._ptr(cap, cpd.u32p), C.byref(f),
                                          C.byref(info)) == cpd.CPD_E_ARG
    assert "null index" in L.cpd_last_error().decode()
    assert L.cpd_index_get_weights(None, cpd._ptr(w, cpd.u32p)) == cpd.CPD_E_ARG
    assert L.cpd_index_get_weight_sets(None, C.byref(k), None) == cpd.CPD_E_ARG
    assert L.cpd_query_assign(None, None, C.c_uint64(0), None, cpd._ptr(cap, cpd.u32p),
                              C.byref(f), C.c_uint32(2), out) == cpd.CPD_E_ARG
    assert L.cpd_last_error()
