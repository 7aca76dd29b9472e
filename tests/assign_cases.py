"""The assignment kernels' arithmetic edges as data: one list of groups, a
group being one launch (a delay function, a load_div, a step) over a handful
of named edge cases, each (w0, capacity, Y, X or None).  A case names the
classes it claims to hit; CLASSES holds, per class, a predicate in Python ints
written from cpd_api.h's wording ("The delay function", "The flow step") — it
classifies the inputs, it computes no result, and it calls nothing of
assign_ref.py / flow_ref.py.  tests/test_assign_cases_cpu.py checks the claims
without a device; tests/test_gpu_assign_cases.py runs the groups through the
kernels.

w0 = None: any free-flow weight will do, so the case is also placed on the
suite's ordinary graphs; a number: the case needs that weight and lives on the
purpose-made graph (directed_loads.made_graph), whose feeders carry
FEEDER_W0."""
U32 = 0xFFFFFFFF
ONE = 1 << 16
LINE = "line"
BIG = U32          # a capacity under which volumes below 65536 give r = 0: w = w0
SPARE_W0 = 1000    # the feeder weight a w0 = None case gets on the purpose-made graph
IDLE_CAP = 7       # capacity of the edges no case uses


def E(name, w0, c, Y, X=None, *classes):
    return dict(name=name, w0=w0, c=c, Y=Y, X=X, classes=classes)


def cap_pair(c, ld=1, tag=""):
    """Both sides of the ratio cap at capacity c: x = 16 c and one below."""
    return [E(f"cap_at{tag}", None, c, (c << 4) * ld, None, "cap_at"),
            E(f"cap_below{tag}", None, c, ((c << 4) - 1) * ld, None, "cap_below")]


HEAVY = 0x7FFFFFFF  # makes a one-unit difference in p visible: t = (w0 * p) >> 16

GROUPS = [
    dict(name="p1", kind="vdf", vdf=(1, 1, 1), load_div=1, edges=cap_pair(5) + [
        E("cap_at_large", None, U32, U32 << 4, None, "cap_at", "cap_large_c"),
        E("cap_below_large", None, U32, (U32 << 4) - 1, None, "cap_below", "cap_large_c"),
        E("sat_last", (1 << 31) - 1, 1, 1, None, "sat_last"),          # w' = 0xFFFFFFFE
        E("sat_first", 0x0F0F0F0F, 1, 16, None, "sat_first", "cap_at"),  # 17 w0 = 2^32 - 1
        E("sat_past", 1 << 31, 1, 1, None, "sat_past"),
        E("w0_zero", 0, 1, 100, None, "w0_zero"),
    ]),
    dict(name="p2", kind="vdf", vdf=(1, 1, 2), load_div=1, edges=cap_pair(3) + [
        E("trunc2", HEAVY, 6, 5, None, "trunc_p2"),
    ]),
    dict(name="p3", kind="vdf", vdf=(1, 1, 3), load_div=1, edges=cap_pair(3) + [
        E("trunc3", HEAVY, 6, 5, None, "trunc_p3"),
    ]),
    dict(name="p4", kind="vdf", vdf=(1, 1, 4), load_div=1, edges=cap_pair(3) + [
        E("sat_first_p4", 65535, 5, 80, None, "sat_first", "cap_at"),  # add = 0xFFFF0000
        E("under_cap_p4", 65535, 5, 79, None, "cap_below"),
        E("trunc4", HEAVY, 6, 5, None, "trunc_p4"),
    ]),
    dict(name="big", kind="vdf", vdf=(65535, 65535, 4), load_div=1, edges=cap_pair(9) + [
        E("t_anum", 0xFFFFF000, 1, 16, None, "t_anum_64"),
        E("t_small", 1, 1, 16, None, "cap_at"),                        # w' = 65537
    ]),
    dict(name="ld3", kind="vdf", vdf=(7, 2, 2), load_div=3, edges=[
        E("ld_at", None, 5, 241, None, "ld_at"),
        E("ld_below", None, 5, 239, None, "ld_below"),
        E("ld_at_large", None, U32, (U32 << 4) * 3 + 2, None, "ld_at", "cap_large_c"),
        E("ld_below_large", None, U32, ((U32 << 4) - 1) * 3 + 1, None, "ld_below", "cap_large_c"),
    ]),
    # explicit steps
    dict(name="f65535", kind="flow", vdf=(1, 1, 1), lam=65535, edges=[
        E("carry", None, BIG, 0, 0x0001000100010001, "flow_carry"),    # |D| lam = 2^64 - 1
        E("ceil_is_floor", None, 3, 2, 5 << 16, "flow_ceil_is_floor"),
        E("past64", None, BIG, 1 << 33, 0, "flow_past64_pos"),         # D lam ~ 2^65
        E("d_zero", None, 1, 9, 9 << 16, "flow_d_zero"),               # counts in xw0 only
        E("flow_cap_at", None, 5, 81, 0, "flow_cap_at"),               # X(lam) >> 16 = 80
        E("flow_cap_below", None, 5, 80, 0, "flow_cap_below"),         # ... = 79
    ]),
    dict(name="f32768", kind="flow", vdf=(0, 1, 1), lam=32768, edges=[  # a_num = 0: w = w0
        E("mad_lo0", 65536, BIG, 0, 1 << 48, "mad_lo0"),
        E("mad_plain", None, 7, 7, 0),
    ]),
    # the line rule's outcomes, each its own step; want = (lambda, evaluations)
    dict(name="line_full", kind="flow", vdf=(1, 1, 1), lam=LINE, want=(ONE, 2), edges=[
        E("cheap", 10, BIG, 5, 0, "line_full"),
        E("dear", 1000, BIG, 0, 5 << 16),
    ]),
    dict(name="line_last", kind="flow", vdf=(1, 1, 1), lam=LINE, want=(ONE, 18), edges=[
        E("jumps_at_one", 100, 1, 1, 0, "line_last"),    # x = 0 below lambda 65536, then 1: w 100 -> 200
        E("const", 150, BIG, 0, 1 << 16),
    ]),
    dict(name="line_first", kind="flow", vdf=(1, 1, 1), lam=LINE, want=(1, 18), edges=[
        E("const", 150, BIG, 1, 0, "line_first"),
        E("drops_at_1", 100, 1, 0, 1 << 16),             # x = 1 at lambda 0, 0 from 1 on: w 200 -> 100
    ]),
    dict(name="line_mid_zero", kind="flow", vdf=(1, 1, 1), lam=LINE, want=(32768, 18), edges=[
        E("steps", 100, 1, 2, 0, "line_mid_zero", "g_zero"),  # w 100, 200 from 32768, 300 at 65536
        E("const", 200, BIG, 0, 2 << 16),
    ]),
    dict(name="line_g0_zero", kind="flow", vdf=(1, 1, 1), lam=LINE, want=(0, 1), edges=[
        E("minus", 200, BIG, 0, 5 << 16, "g0_zero", "g_zero"),
        E("plus", 200, BIG, 5, 0),
    ]),
]


def feeder_weights():
    """The purpose-made graph's feeder weights: for every w0 the most any one
    group needs of it (None counted as SPARE_W0)."""
    need = {}
    for g in GROUPS:
        cnt = {}
        for e in g["edges"]:
            w = SPARE_W0 if e["w0"] is None else e["w0"]
            cnt[w] = cnt.get(w, 0) + 1
        for w, k in cnt.items():
            need[w] = max(need.get(w, 0), k)
    return [w for w in sorted(need) for _ in range(need[w])]


FEEDER_W0 = feeder_weights()


def assign_feeders(group):
    """Feeder number per case of the group: the first unused feeder of the
    case's weight."""
    used, out = set(), []
    for e in group["edges"]:
        w = SPARE_W0 if e["w0"] is None else e["w0"]
        k = next(i for i, v in enumerate(FEEDER_W0) if v == w and i not in used)
        used.add(k)
        out.append(k)
    return out


def free_cases(group):
    """The cases of the group that any weight serves."""
    return [e for e in group["edges"] if e["w0"] is None]


def tables(m, group, edge_of, w0, cases=None):
    """(capacity, Y, X or None) over m edges with case i of the group on edge
    edge_of[i]; edges no case uses carry nothing.  w0: the graph's weights,
    checked against the weights the cases ask for."""
    cases = group["edges"] if cases is None else cases
    assert len(set(edge_of)) == len(cases) == len(edge_of)
    cap, Y, X = [IDLE_CAP] * m, [0] * m, [0] * m
    for e, c in zip(edge_of, cases):
        assert c["w0"] is None or c["w0"] == int(w0[e]), c["name"]
        cap[e], Y[e], X[e] = c["c"], c["Y"], c["X"] or 0
    return cap, Y, (X if group["kind"] == "flow" else None)


PLANE_FORMS = ("Y", "zero", "minus", "plus", "Y", "minus", "zero", "plus")


def plane_tables(Y, K):
    """K planes that differ at the boundaries: the table itself, an all-zero
    plane, every loaded counter one less, one more, and round again."""
    form = {"Y": lambda y: y, "zero": lambda y: 0, "minus": lambda y: y - 1 if y else 0,
            "plus": lambda y: y + 1 if y else 0}
    return [[form[PLANE_FORMS[j]](y) for y in Y] for j in range(K)]


# --- the predicates ---------------------------------------------------------

def _x(e, g):
    return e["Y"] // g.get("load_div", 1)


def _r(x, c):  # "the ratio x / c in Q16, clamped at 16.0"
    return (1 << 20) if x >= (c << 4) else (x << 16) // c


def _p(r, power):
    p = r
    for _ in range(power - 1):
        p = (p * r) >> 16
    return p


def _t(e, g):
    return (e["w0"] * _p(_r(_x(e, g), e["c"]), g["vdf"][2])) >> 16


def _add(e, g):
    return _t(e, g) * g["vdf"][0] // g["vdf"][1]


def _D(e):
    return (e["Y"] << 16) - e["X"]


def _xl(e, g):  # X(lambda) >> 16, the floor toward minus infinity
    return (e["X"] + ((g["lam"] * _D(e)) >> 16)) >> 16


def _trunc(e, g, power):
    r = _r(_x(e, g), e["c"])
    exact = r ** power >> (16 * (power - 1))
    lost = (_p(r, power) << (16 * (power - 1))) != r ** power
    differs = _p(r, power) != exact if power > 2 else lost
    seen = (e["w0"] * _p(r, power)) >> 16 != (e["w0"] * r ** power) >> (16 * power)
    return g["vdf"][2] == power and r < (1 << 20) and differs and seen and _add(e, g) < U32 - e["w0"]


CLASSES = {
    # vdf_weight, the ratio cap
    "cap_at": lambda e, g: _x(e, g) == e["c"] << 4,
    "cap_below": lambda e, g: _x(e, g) == (e["c"] << 4) - 1 and (_x(e, g) << 16) // e["c"] < 1 << 20,
    "cap_large_c": lambda e, g: (e["c"] << 4) >= 1 << 35 and 0 <= (e["c"] << 4) - _x(e, g) <= 1,
    # vdf_weight, saturation
    "sat_last": lambda e, g: _add(e, g) == U32 - e["w0"] - 1,
    "sat_first": lambda e, g: _add(e, g) == U32 - e["w0"],
    "sat_past": lambda e, g: _add(e, g) == U32 - e["w0"] + 1,
    "w0_zero": lambda e, g: e["w0"] == 0 and _x(e, g) > 0 and g["vdf"][0] > 0,
    "t_anum_64": lambda e, g: (g["vdf"][0] == 65535 and (1 << 48) - (1 << 36) <= _t(e, g) < 1 << 48
                               and (1 << 64) - (1 << 52) <= _t(e, g) * 65535 < 1 << 64),
    "trunc_p2": lambda e, g: _trunc(e, g, 2),
    "trunc_p3": lambda e, g: _trunc(e, g, 3),
    "trunc_p4": lambda e, g: _trunc(e, g, 4),
    # load_div
    "ld_at": lambda e, g: (g["load_div"] > 1 and e["Y"] % g["load_div"] != 0
                           and e["Y"] // g["load_div"] == e["c"] << 4),
    "ld_below": lambda e, g: (g["load_div"] > 1 and e["Y"] % g["load_div"] != 0
                              and e["Y"] // g["load_div"] == (e["c"] << 4) - 1),
    # flow_at
    "flow_carry": lambda e, g: (_D(e) < 0 and (abs(_D(e)) * g["lam"]) % 2 ** 64 >= 2 ** 64 - 65535
                                and (abs(_D(e)) * g["lam"]) % 65536 != 0),
    "flow_ceil_is_floor": lambda e, g: (_D(e) < 0 and g["lam"] > 0
                                        and (abs(_D(e)) * g["lam"]) % 65536 == 0),
    "flow_past64_pos": lambda e, g: _D(e) > 0 and _D(e) * g["lam"] >= 1 << 64,
    "flow_d_zero": lambda e, g: _D(e) == 0 and e["X"] > 0,
    "flow_cap_at": lambda e, g: _xl(e, g) == e["c"] << 4,
    "flow_cap_below": lambda e, g: _xl(e, g) == (e["c"] << 4) - 1,
    # mad128_signed: with a_num = 0 the weight is w0 at every lambda
    "mad_lo0": lambda e, g: (_D(e) < 0 and g["vdf"][0] == 0 and (abs(_D(e)) * e["w0"]) % 2 ** 64 == 0
                             and (abs(_D(e)) * e["w0"]) >> 64 != 0),
    # g exactly 0 from non-zero terms of both signs; which lambda it is zero at
    # is the CPU test's to show (it needs the delay function)
    "g_zero": lambda e, g: {(_D(c) > 0) - (_D(c) < 0) for c in g["edges"]} == {1, -1},
    "g0_zero": lambda e, g: (all(c["c"] == BIG and c["X"] >> 16 < 65536 for c in g["edges"])
                             and sum(_D(c) * c["w0"] for c in g["edges"]) == 0),
    # the line rule's outcomes: the case names them, flow_ref.line_rule confirms
    "line_full": lambda e, g: g["lam"] == LINE and g["want"] == (ONE, 2),
    "line_last": lambda e, g: g["lam"] == LINE and g["want"] == (ONE, 18),
    "line_first": lambda e, g: g["lam"] == LINE and g["want"] == (1, 18),
    "line_mid_zero": lambda e, g: g["lam"] == LINE and g["want"] == (32768, 18),
}


# --- where the cases are placed ----------------------------------------------

WORLD_NAMES = ("made2", "made16", "ring2", "lattice15")
_WORLDS = {}


def world(name):
    """The worlds the case list is placed on, built once: the purpose-made
    graph with 2 and with 16 adjacency slots per column (targets: two ring
    nodes) and two of test_gpu_assign.py's graphs, ring2 (2 slots) and
    lattice15 (16, with padding), every node a target.  A made world also
    carries .feeders, the edge of every feeder."""
    if name not in _WORLDS:
        import numpy as np
        from directed_loads import World, made_graph
        from graphs import lattice_wide, ring2_graph
        if name.startswith("made"):
            # out-degree 2, and 15 (the most a 4-bit move names)
            g, feeders = made_graph(FEEDER_W0, {"made2": 1, "made16": 14}[name])
            w = World(g, [0, 1])
            w.feeders = feeders
        else:
            g = ring2_graph() if name == "ring2" else lattice_wide(20, 15, 15, seed=15)
            w = World(g, np.arange(g.n))
        _WORLDS[name] = w
    return _WORLDS[name]


def placement(name, group):
    """(world, the cases of the group placed there, their edges); on an
    ordinary graph only the cases any weight serves, spread over the loadable
    edges.  The cases may be none."""
    w = world(name)
    if name.startswith("made"):
        return w, group["edges"], [int(w.feeders[k]) for k in assign_feeders(group)]
    cases, ok = free_cases(group), w.loadable()
    return w, cases, [int(ok[(i + 1) * len(ok) // (len(cases) + 1)]) for i in range(len(cases))]


BIG_GRAPH = (70000, 12, 3)  # chain_hub: 16 slots per column, 1,120,000 slots
BIG_EDGES = 20000


def big_world():
    """The second grid-stride trip's world: chain_hub with more adjacency slots
    than one launch has lanes, 8 targets, and three tables over BIG_EDGES
    random loadable edges (counters of 1..599 against capacities of 1..39:
    both sides of the cap; a few past 2^32)."""
    if "big" not in _WORLDS:
        import numpy as np
        from directed_loads import World
        from graphs import chain_hub
        g = chain_hub(*BIG_GRAPH)
        rng = np.random.default_rng(70)
        w = World(g, rng.choice(g.n, size=8, replace=False))
        w.tables = []
        for _ in range(3):
            Y = np.zeros(g.m, np.uint64)
            e = rng.choice(w.loadable(), size=BIG_EDGES, replace=False)
            Y[e] = rng.integers(1, 600, BIG_EDGES, dtype=np.uint64)
            Y[e[:5]] += np.uint64(1 << 32)
            w.tables.append(Y)
        w.capacity = rng.integers(1, 40, g.m).astype(np.uint32)
        _WORLDS["big"] = w
    return _WORLDS["big"]
