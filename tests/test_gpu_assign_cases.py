"""GPU: the assignment kernels at their arithmetic edges.  The case list of
tests/assign_cases.py (pinned without a device by test_assign_cases_cpu.py) is
placed edge by edge through tests/directed_loads.py — every placement asserts
the table it left — and run through cpd_index_weights_from_loads in the
one-plane form and with 2, 4, 5 and 8 planes, and through cpd_index_flow_step,
on the purpose-made graph (2 and 16 slots per column) and on ring2 and
lattice15; then the line rule's outcomes, each as its own step; then a graph
with more adjacency slots than one launch has lanes, so that the grid-stride
loops take a second trip.  Everything is compared exactly with
tests/assign_ref.py and tests/flow_ref.py.  (sptt_reduce's second trip needs
more than 2^20 queries and is not here.)"""
import numpy as np
import pytest

import assign_cases as A
from assign_ref import ref_weights_from_loads
from flow_ref import ref_flow_step

pytestmark = pytest.mark.gpu
PLANES = (2, 4, 5, 8)
INFO_KEYS = ("lambda_q16", "evals", "g0", "xw0", "tstt", "changed")


@pytest.fixture(scope="module", params=A.WORLD_NAMES)
def placed(request):
    return request.param, A.world(request.param)


def groups_on(name, kind):
    """(group, capacity u32[m], Y, X) of every group of the kind with cases on
    the world."""
    out = []
    for g in A.GROUPS:
        w, cases, edge_of = A.placement(name, g)
        if g["kind"] == kind and cases:
            cap, Y, X = A.tables(w.g.m, g, edge_of, w.g.w, cases)
            out.append((g, np.array(cap, np.uint32), Y, X))
    return out


def check_vdf(ix, w, g, cap, planes, msg):
    """weights_from_loads on the resident table, which must be `planes`."""
    a_num, a_den, power = g["vdf"]
    K = len(planes)
    info = ix.weights_from_loads(cap, a=(a_num, a_den), power=power, load_div=g["load_div"])
    got = ix.get_weights()[None, :] if K == 1 else ix.get_weight_sets()
    assert got.shape == (K, w.g.m), msg
    tstt = changed = 0
    for j, Y in enumerate(planes):
        want, tj, cj = ref_weights_from_loads(w.g.w, Y, cap, a_num, a_den, power, g["load_div"])
        np.testing.assert_array_equal(got[j], want, err_msg=f"{msg} plane {j}")
        tstt, changed = tstt + tj, changed + cj
    print(f"{msg}: tstt {info['tstt']} want {tstt}; changed {info['changed']} want {changed}")
    assert (info["tstt"], info["changed"], info["planes"]) == (tstt, changed, K), msg
    assert ix.loads_fetch().tolist() == [[int(v) for v in Y] for Y in planes], msg  # only read


def test_cases_one_plane(placed):
    name, w = placed
    ix = w.index()
    todo = groups_on(name, "vdf")
    assert todo
    for g, cap, Y, _ in todo:
        w.place(ix, Y)
        check_vdf(ix, w, g, cap, [Y], f"{name} {g['name']}")
        if name.startswith("made"):  # the cases did move their weights
            assert (ix.get_weights() != w.g.w).any()


@pytest.mark.parametrize("K", PLANES)
def test_cases_k_planes(placed, K):
    name, w = placed
    ix = w.index()
    for g, cap, Y, _ in groups_on(name, "vdf"):
        planes = A.plane_tables(Y, K)
        w.place_planes(ix, planes)
        check_vdf(ix, w, g, cap, planes, f"{name} {g['name']} K={K}")
        sets = ix.get_weight_sets()
        np.testing.assert_array_equal(sets[1], w.g.w)  # the all-zero plane: w0
        np.testing.assert_array_equal(ix.get_weights(), w.g.w)  # the current weights stay


def check_flow(ix, w, g, cap, Y, X, msg):
    """The flow X placed, the loading Y placed, then the group's step."""
    w.place_flow(ix, X, cap)
    w.place(ix, Y)
    a_num, a_den, power = g["vdf"]
    info = ix.flow_step(cap, lam=g["lam"], a=(a_num, a_den), power=power)
    Xn, wn, want = ref_flow_step(w.g.w, Y, X, cap, g["vdf"], g["lam"])
    want.pop("D")
    print(f"{msg}: got {({k: info[k] for k in INFO_KEYS})} want {want}")
    assert {k: info[k] for k in INFO_KEYS} == want, msg
    assert ix.flow_fetch().tolist() == Xn, msg
    np.testing.assert_array_equal(ix.get_weights(), wn, err_msg=msg)
    assert ix.loads_fetch()[0].tolist() == Y, msg  # the table is only read
    return info


def test_cases_flow_steps(placed):
    name, w = placed
    ix = w.index()
    todo = [t for t in groups_on(name, "flow") if t[0]["lam"] != A.LINE]
    assert todo
    for g, cap, Y, X in todo:
        check_flow(ix, w, g, cap, Y, X, f"{name} {g['name']}")


@pytest.mark.parametrize("name", ["made2", "made16"])
def test_line_rule_outcomes(name):
    w = A.world(name)
    ix = w.index()
    todo = [t for t in groups_on(name, "flow") if t[0]["lam"] == A.LINE]
    assert len(todo) == 5
    for g, cap, Y, X in todo:
        info = check_flow(ix, w, g, cap, Y, X, f"{name} {g['name']}")
        assert (info["lambda_q16"], info["evals"]) == g["want"], g["name"]


def test_second_grid_stride_trip():
    """More adjacency slots than the 4096 x 256 lanes of one launch, loaded on
    both sides of that index: one weights_from_loads, one two-plane update and
    one explicit step."""
    w = A.big_world()
    n, m = w.g.n, w.g.m
    shift = int(np.ceil(np.log2(np.diff(w.g.row_ptr.astype(np.int64)).max())))
    assert n << shift > 4096 * 256
    ix = w.index()
    slot = w._dev.plan.order().astype(np.int64)[w.src] << shift
    for Y in w.tables:
        assert ((slot < 4096 * 256) & (Y > 0)).any() and ((slot >= 4096 * 256) & (Y > 0)).any()
    Y0, Y1, Y2 = ([int(v) for v in Y] for Y in w.tables)
    g = dict(vdf=(7, 2, 2), load_div=1)
    w.place(ix, Y0)
    check_vdf(ix, w, g, w.capacity, [Y0], "big one plane")
    late = (slot >= 4096 * 256) & (w.tables[0] > 0)
    assert (ix.get_weights()[late] != w.g.w[late]).any()  # the second trip's slots moved
    w.place_planes(ix, [Y0, Y1])
    check_vdf(ix, w, g, w.capacity, [Y0, Y1], "big two planes")
    ix.flow_clear()
    w.place(ix, Y1)
    ix.flow_step(w.capacity, lam=0)  # initialises
    X = [y << 16 for y in Y1]
    assert ix.flow_fetch().tolist() == X
    w.place(ix, Y2)
    info = ix.flow_step(w.capacity, lam=30000, a=(7, 2), power=2)
    Xn, wn, want = ref_flow_step(w.g.w, Y2, X, w.capacity, (7, 2, 2), 30000)
    D = want.pop("D")
    assert any(d < 0 for d in D) and any(d > 0 for d in D)
    print(f"big step: got {({k: info[k] for k in INFO_KEYS})} want {want}")
    assert {k: info[k] for k in INFO_KEYS} == want
    assert ix.flow_fetch().tolist() == Xn
    np.testing.assert_array_equal(ix.get_weights(), wn)
    assert ix.loads_fetch()[0].tolist() == Y2
