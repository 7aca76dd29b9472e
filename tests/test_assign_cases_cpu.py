"""CPU: the case list of tests/assign_cases.py is what it claims — every
case's predicate holds, every line-rule case gives the lambda and evaluation
count it names, every class of arithmetic edge is hit — and it fits where it
is placed: the placements of tests/directed_loads.py load exactly the wanted
tables under loads_ref.walk_loads / timed_ref.walk_timed, without a device."""
import numpy as np
import pytest

import assign_cases as A
from directed_loads import flow_loadings
from flow_ref import g_of, line_rule

# every bullet of the gap this list closes, by the class that stands for it
NEEDED = ("cap_at", "cap_below", "cap_large_c", "sat_last", "sat_first", "sat_past", "w0_zero",
          "t_anum_64", "trunc_p2", "trunc_p3", "trunc_p4", "ld_at", "ld_below", "flow_carry",
          "flow_ceil_is_floor", "flow_past64_pos", "mad_lo0", "g_zero", "g0_zero", "line_full",
          "line_last", "line_first", "line_mid_zero")
PLANES = (2, 4, 5, 8)


def test_every_predicate_holds():
    names = [g["name"] for g in A.GROUPS]
    assert len(set(names)) == len(names)
    for g in A.GROUPS:
        assert g["kind"] in ("vdf", "flow") and (g["kind"] == "flow") == ("lam" in g)
        for e in g["edges"]:
            assert 0 <= e["Y"] < 1 << 47 and 1 <= e["c"] <= A.U32
            assert (e["X"] is None) == (g["kind"] == "vdf")
            if e["X"] is not None:
                assert 0 <= e["X"] < 1 << 63
            for cls in e["classes"]:
                assert A.CLASSES[cls](e, g), f"{g['name']}.{e['name']} is no {cls}"


def test_every_class_is_hit():
    hit = {}
    for g in A.GROUPS:
        for e in g["edges"]:
            for cls in e["classes"]:
                hit.setdefault(cls, []).append(f"{g['name']}.{e['name']}")
    for cls in sorted(hit):
        print(f"{cls}: {', '.join(hit[cls])}")
    assert set(NEEDED) <= set(A.CLASSES) and set(hit) == set(A.CLASSES)
    # both sides of the cap at a small and at a 36-bit c << 4, with and without load_div
    for g in ("p1", "ld3"):
        grp = next(x for x in A.GROUPS if x["name"] == g)
        for large in (False, True):
            sides = {A._x(e, grp) - (e["c"] << 4) for e in grp["edges"]
                     if ("cap_large_c" in e["classes"]) == large and e["w0"] is None}
            assert sides == {0, -1}, (g, large)
    # every power has its truncation case
    assert sorted(g["vdf"][2] for g in A.GROUPS for e in g["edges"]
                  if any(c.startswith("trunc_p") for c in e["classes"])) == [2, 3, 4]


def _line_inputs(g):
    es = g["edges"]
    X = [e["X"] for e in es]
    return ([e["w0"] for e in es], [(e["Y"] << 16) - e["X"] for e in es], X, [e["c"] for e in es])


def test_line_cases_give_what_they_name():
    lines = [g for g in A.GROUPS if g.get("lam") == A.LINE]
    assert len(lines) == 5
    for g in lines:
        w0, D, X, cap = _line_inputs(g)
        gl = lambda lam: g_of(w0, D, X, cap, g["vdf"], lam)  # noqa: E731
        got = line_rule(gl)
        print(f"{g['name']}: {got}, g(0) {gl(0)}, g(65536) {gl(A.ONE)}")
        assert got == g["want"], g["name"]
        assert any(d > 0 for d in D) and any(d < 0 for d in D)
        if g["name"] == "line_last":
            assert gl(65535) < 0 <= gl(A.ONE)
        if g["name"] == "line_first":
            assert gl(0) < 0 <= gl(1)
        if g["name"] == "line_mid_zero":  # exactly 0 at the first mid: hi moves, lo does not
            assert gl(32767) < 0 == gl(32768) == gl(65535) < gl(A.ONE)
        if g["name"] == "line_g0_zero":
            assert gl(0) == 0


def test_plane_forms():
    p4 = next(g for g in A.GROUPS if g["name"] == "p4")
    Y = [e["Y"] for e in p4["edges"]]
    for K in PLANES:
        planes = A.plane_tables(Y, K)
        assert len(planes) == K and planes[0] == Y and not any(planes[1])
        assert len({tuple(p) for p in planes}) == min(K, 4)
    # an all-zero plane beside one that saturates
    assert any("sat_first" in e["classes"] for e in p4["edges"])
    # one less / one more swap the sides of the cap
    at = next(i for i, e in enumerate(p4["edges"]) if e["name"] == "cap_at")
    c = p4["edges"][at]["c"]
    assert [A.plane_tables(Y, 4)[j][at] - (c << 4) for j in (0, 2, 3)] == [0, -1, 1]


@pytest.mark.parametrize("name", A.WORLD_NAMES)
def test_cases_fit_the_loadable_edges(name):
    """A condition on the graphs: a graph with fewer loadable edges than its
    cases need fails here."""
    w = A.world(name)
    ok = w.loadable()
    used = set()
    for g in A.GROUPS:
        w, cases, edge_of = A.placement(name, g)
        if name.startswith("made"):
            assert len(cases) == len(g["edges"])
        assert len(ok) >= len(cases) and set(edge_of) <= set(ok.tolist()), g["name"]
        if not cases:
            continue
        used |= set(edge_of)
        cap, Y, X = A.tables(w.g.m, g, edge_of, w.g.w, cases)
        assert min(cap) >= 1
        if X is None:
            w.check_place(Y)
            for K in PLANES:
                w.check_place_planes(A.plane_tables(Y, K))
        else:
            Y1, Y2 = flow_loadings(X)
            assert [(a << 16) + (b - a) for a, b in zip(Y1, Y2)] == X
            for T in (Y1, Y2, Y):
                w.check_place(T)
    print(f"{name}: n {w.g.n}, m {w.g.m}, loadable {len(ok)}, edges used by cases {sorted(used)}")
    if name.startswith("made"):  # a feeder's move is forced: every one is loadable
        assert set(w.feeders.tolist()) <= set(ok.tolist())
        assert w.g.w[w.feeders].tolist() == A.FEEDER_W0
        deg = int(np.diff(w.g.row_ptr.astype(np.int64)).max())
        assert 1 << int(np.ceil(np.log2(deg))) == int(name[4:])  # slots per column
    else:
        free = sum(len(A.free_cases(g)) for g in A.GROUPS)
        assert free >= 20 and len(used) >= 6


def test_big_world_places_on_both_sides_of_one_launch():
    w = A.big_world()
    n, m = w.g.n, w.g.m
    shift = int(np.ceil(np.log2(np.diff(w.g.row_ptr.astype(np.int64)).max())))
    assert shift == 4 and n << shift > 4096 * 256
    print(f"big: n {n}, m {m}, loadable {len(w.loadable())}, {A.BIG_EDGES} edges per table")
    col = w.order.astype(np.int64)[w.src]  # a slot is (column << shift) + move
    for Y in w.tables:
        slot = col[Y > 0] << shift
        assert (slot < 4096 * 256).sum() > 500 and (slot >= 4096 * 256).sum() > 500
        w.check_place(Y)
    w.check_place_planes(w.tables[:2])
