"""The GPU contraction (ch_gpu.cpp / ch_kernels.hip) where road-like graphs
never take it: witness searches with 31 .. 300 targets, across the lane
workspace's cap of 32, the wave kernel's 32 / 64 / 128 and into the large HBM
workspace sized from the largest degree; arena compaction; growth of the two
arc pools.  The reference is the host contraction (ch.cpp), all nine exported
arrays; test_ch_edges_cpu.py pins the gadgets' shape and checks the host
hierarchies against Dijkstra.

Every case runs in a child process (the knobs are read from the environment;
the route is read from the contraction's summary line on stderr) and asserts
both: the same hierarchy, and that the route it is about carried searches.
The contraction is asked for alone (Plan(ch_only=True)): the gadgets' degrees
are past what a plan's rows hold, and a GPU contraction that fails is an error
there, not a host build."""
import os
import subprocess
import sys

import pytest

import cpd
from graphs import CH_FAN_D, CH_HUB_D, CH_LANE_EDGE_D, CH_TIE_D
from test_ch_gpu import summary

pytestmark = pytest.mark.gpu

TIMEOUT = 8  # seconds per child: ten times the slowest (0.5 .. 0.8 s on an MI355X)

PATHS = [os.path.dirname(os.path.abspath(cpd.__file__)), os.path.dirname(os.path.abspath(__file__))]


def contract_both(graph, env=None, settle=0):
    """Contract `graph` (an expression over the graphs module) on the host and
    on GPU 0 in a child process under `env`, compare the nine arrays there,
    and return the GPU contraction's summary line as a dict of ints."""
    code = (
        "import sys; sys.path[:0] = %r\n"
        "import cpd, graphs\n"
        "from test_ch_gpu import same_hierarchy\n"
        "g = %s\n"
        "g = g[0] if isinstance(g, tuple) else g\n"
        "a = cpd.Plan(g, settle=%d, ch_only=True).export_ch()\n"
        "b = cpd.Plan(g, settle=%d, gpu=0, verbose=True, ch_only=True).export_ch()\n"
        "same_hierarchy(a, b)\n"
        "print('same')\n" % (PATHS, graph, settle, settle))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **(env or {})),
                       capture_output=True, text=True, timeout=TIMEOUT)
    assert r.returncode == 0 and "same" in r.stdout, r.stderr[-2000:]
    s = summary(r.stderr)
    print(graph, env or "", s)
    return s


def check_degree_route(s, D):
    """What the summary must show for a graph with a search of exactly D
    targets, under default knobs (rounds of so few searches skip the lane
    kernel: test_lane_cap_edge runs it)."""
    if D <= 32:
        assert s["large"] == 0
    if D >= 33:
        assert s["waves"] >= 1
    if D >= 129:
        assert s["large"] >= 1     # past the largest LDS size


@pytest.mark.parametrize("D", CH_FAN_D)
def test_fan_contraction_search_of_D_targets(D):
    """Each of the three fans is contracted by one search of exactly D targets
    (all tied on their via weight), and its source keeps D + 3 out-arcs: D + 2
    or D + 3 targets in every simulation there."""
    s = contract_both(f"graphs.ch_fan_case({D})")
    check_degree_route(s, D)
    if 33 <= D <= 64:
        assert s["w1"] >= 1        # contraction searches start at the 64-target size
    if 65 <= D <= 128:
        assert s["w2"] >= 1


@pytest.mark.parametrize("D", CH_HUB_D)
def test_hub_simulation_search_of_D_targets(D):
    """The hub goes last: its searches are simulations, of D targets from its
    extra in-neighbour and D - 1 from its two path neighbours; they start at
    the wave kernel's smallest size."""
    s = contract_both(f"graphs.ch_hub_case({D})")
    check_degree_route(s, D)
    assert s["w0"] >= 1
    assert s["w1"] >= 1            # 33 targets and more leave the 32-target size
    if D >= 65:
        assert s["w2"] >= 1


@pytest.mark.parametrize("case", [f"fan_case({D})" for D in (31, 32, 33)] +
                         [f"hub_case({D})" for D in CH_LANE_EDGE_D])
def test_lane_cap_edge(case):
    """CPD_CH_WAVE=0 starts every search in the lane kernel, whose workspace
    holds 32 targets: the fans' contraction searches of 31 and 32 targets end
    there, the one of 33 and the simulations at the fans' sources (D + 2
    targets and more) move on to the waves; so do the hub's once shortcuts
    have added to its D out-arcs.  The counters cannot tell which search
    moved on — the hierarchy is the check."""
    s = contract_both(f"graphs.ch_{case}", {"CPD_CH_WAVE": "0"})
    assert 1 <= s["waves"] < s["searches"] and s["large"] == 0


@pytest.mark.parametrize("gadget", ["fan", "hub"])
@pytest.mark.parametrize("D", [129, 300])
def test_lane_straight_to_large_workspace(gadget, D):
    s = contract_both(f"graphs.ch_{gadget}_case({D})", {"CPD_CH_NOWAVE": "1"})
    assert s["waves"] == 0 and s["large"] >= 1


@pytest.mark.parametrize("gadget", ["fan", "hub"])
@pytest.mark.parametrize("D", [129, 300])
def test_everything_starts_in_waves(gadget, D):
    s = contract_both(f"graphs.ch_{gadget}_case({D})", {"CPD_CH_WAVE": "1000000000"})
    assert s["waves"] >= s["searches"] and s["large"] >= 1


@pytest.mark.parametrize("gadget", ["fan", "hub"])
@pytest.mark.parametrize("D", CH_TIE_D)
def test_ties_on_via(gadget, D):
    """Weights 1..2: nearly all targets of a search tie on via, and most heap
    keys tie too — the target order and the heap's replay decide."""
    check_degree_route(contract_both(f"graphs.ch_{gadget}_case({D}, wmax=2)"), D)


def test_two_way_hub_many_large_searches_at_once():
    """302 in-neighbours: the hub's first priority alone is 302 simulations of
    299 or 300 targets, side by side in the large workspace."""
    s = contract_both("graphs.ch_hub_two_way()")
    assert s["large"] >= 302


@pytest.mark.parametrize("settle", [3, 20])
def test_settle_limit_with_130_arcs_at_the_source(settle):
    """The cut at the settle limit falls at the same settled node when the
    source's arcs take many relax groups (lane) and rounds of 64 (wave)."""
    s = contract_both("graphs.ch_fan_case(129)", settle=settle)
    check_degree_route(s, 129)


@pytest.mark.parametrize("graph,twice", [("cpd.synth_road_graph(60, 50, seed=3)", True),
                                         ("graphs.ch_fan_case(65)", False),
                                         ("graphs.GRAPHS['deg8']()", False)])
def test_arena_compaction_and_pool_growth(graph, twice):
    """CPD_CH_ARENA=1,1: the arena starts with room for the initial lists and
    nothing else, the pools with one arc."""
    s = contract_both(graph, {"CPD_CH_ARENA": "1,1"})
    assert s["compactions"] >= (2 if twice else 1)
    assert s["up"] >= 1 and s["down"] >= 1


def test_defaults_neither_compact_nor_grow():
    """The knob is what makes the case above: unset, a 3000-node graph stays
    far inside the arena and the pools."""
    s = contract_both("cpd.synth_road_graph(60, 50, seed=3)")
    assert s["compactions"] == 0 and s["up"] == 0 and s["down"] == 0
