"""Every optimisation switch left in libcpd, turned off, still gives bit-exact
rows and walks (each shipped kernel instantiation is
reached by a default or fallback path that a GPU test covers).

The switches are read once per process (cpd_kernels.hip / cpd_switches.cpp), so
each setting runs in a child process, one after another (never two on the
GPU at once): build the rows of a synthetic road graph (4-bit sets, the
narrow path) and of the degree-8 graph (8-bit sets), compare with the
oracle, walk queries over them dense and RLE.  What each reaches:
  CPD_LIVE=0      sweep_level<true> (dense up-sweep), sweep_down8 without masks
  CPD_SORT=0      batch lanes in caller order
  CPD_LANE_KEY=0  column lane order despite coordinates
  CPD_XCD=0       identity block mapping
  CPD_ASYNC=0     the emit in line (one buffer set)
  CPD_RLE_FUSED=0 the count (rle_count_ch + rle_fix), then rle_moves4, instead
                  of the one-pass rle_emit8 + rle_emit_fix
  CPD_LEAFFM=0    leaf first-move sets recomputed by first_moves
  CPD_OVERLAP=0   each batch's up-sweep on the main stream, after the previous
                  batch's first moves (no second up store in use)
  CPD_FM_ORDER=0  first_moves' segments in column order (not Hilbert order)
Both graphs have one 2048-column tile and one 1024-target slab.  Past that:
test_unfused_rle_past_one_tile (below) runs CPD_RLE_FUSED=0 over 3 and 17
tiles; rle_scan<8|16>, rle_moves<8|16> (second 16-tile chunk included),
first_moves<8|16,1,true|false> and first_moves<4,2,false> at a second slab
are reached by tests/test_gpu_wide_degree.py, cpd_search<1|3|4,*> by
tests/test_gpu_search_widths.py (<2,*>: tests/test_gpu_search.py).
Round 6 removed the switches whose variants lost their A/Bs (VERDICT r05
item 7): CPD_FM_N4, CPD_RLE_CH, CPD_MOVES_SWAR, CPD_TABLE_BITS, CPD_TS_SHARE,
CPD_EMIT_DEFER, CPD_UP_HEAD, CPD_EMIT_WIDE, CPD_ROWS_NIBBLE (and the schedule
knobs CPD_CU_RESERVE(_MAIN), CPD_FM_LDS, CPD_EMIT_LDS, CPD_UP_PRIO,
CPD_SEARCH_RESIDENT, CPD_SEARCH_GROW, CPD_SEARCH_LANE_MAJOR, CPD_EXP_CPW,
CPD_TS_CHUNK_MAX, CPD_UP_INIT_BLOCKS, CPD_UP_PERSIST with its persistent
sweep_up_narrow, CPD_UP_CUS with the CU-masked streams).
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

CHILD = r"""
import json, sys
import numpy as np
sys.path[:0] = [%r, %r, %r]
import cpd, oracle
from graphs import GRAPHS
out = {}
for name in ("synth", "deg8"):
    g = GRAPHS[name]()
    plan = cpd.Plan(g)
    dev = cpd.Graph(plan, batch=1024)
    if g.x is not None:
        dev.set_coords(g.x, g.y)
    rng = np.random.default_rng(4)
    targets = rng.permutation(g.n).astype(np.uint32)[:1500]
    rows = dev.build_rows(targets)
    off, runs = rows.export()
    ref_off, ref_runs = oracle.build_rows(g.row_ptr, g.dst, g.w, plan.order(), targets)
    ok = bool(np.array_equal(off, ref_off) and np.array_equal(runs, ref_runs))
    bits = rows.move_bits()
    mv = rows.export_moves(0, 300)
    ok = ok and bool(np.array_equal(mv, oracle.moves_from_runs(ref_off[:301], ref_runs, g.n, bits)))
    s = rng.integers(0, g.n, 3000).astype(np.uint32)
    t = targets[rng.integers(0, len(targets), 3000)]
    rc, rh, rf = oracle.table_search(g.row_ptr, g.dst, g.w, plan.order(), targets, ref_off,
                                     ref_runs, s, t)
    ix = cpd.Index(dev, rows=rows)
    for mode in ("dense", "rle"):
        ix.set_mode(mode)
        c, h, f, _ = ix.query(s, t)
        ok = ok and bool(np.array_equal(c, rc) and np.array_equal(h, rh) and np.array_equal(f, rf))
    out[name] = ok
print(json.dumps(out))
"""

SWITCHES = ["CPD_LIVE", "CPD_SORT", "CPD_LANE_KEY", "CPD_XCD", "CPD_ASYNC", "CPD_RLE_FUSED",
            "CPD_LEAFFM", "CPD_OVERLAP", "CPD_FM_ORDER"]
OFF = {}   # switches whose "off" value is not 0
WITH = {}  # switches whose path needs another one set


@pytest.mark.parametrize("switch", SWITCHES)
def test_switch_off_bit_exact(switch):
    code = CHILD % (HERE, os.path.join(ROOT, "distributed-oracle-search_amd"),
                    os.path.join(ROOT, "oracle"))
    env = dict(os.environ, **{switch: OFF.get(switch, "0")}, **WITH.get(switch, {}))
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res == {"synth": True, "deg8": True}, (switch, res)


# CPD_RLE_FUSED=0 past one tile.  The graphs above have one 2048-column tile
# (synth: 2 count chunks), so the unfused 4-bit path's tile carries and its
# second 16-tile chunk would go unrun now that the fused emit is the default:
#   synth70  4900 nodes: 3 tiles, 6 chunks of rle_count_ch<32>, seams for rle_fix
#   chain    34000 nodes: 17 tiles = 2 chunks of rle_moves4, 3 grid columns of
#            rle_count_ch<32>; a handful of runs per row, far past rle_fix's rescan
#            budget, so the gated rle_scan<4> re-counts the batch
#   hub8     the same path with a degree-8 node: rle_scan<8> + rle_moves<8>
#            (what the switch must leave alone)
#   band2048 graphs.band, 2048 nodes, 1029 targets: one tile with no padded
#            column, a second batch of five rows
#   band2049 2049 nodes: a second tile of one column and 2047 padded ones
#            (both pinned by test_oracle_cpu.py with the other size-edge cases)
CHILD_UNFUSED = r"""
import json, sys
import numpy as np
sys.path[:0] = [%r, %r, %r]
import cpd, oracle
from graphs import chain_graph, chain_hub, edge_graph
out = {}
for name, make, k in (("synth70", lambda: cpd.synth_road_graph(70, 70, seed=70), 1500),
                      ("chain", lambda: chain_graph(34000, seed=34), 300),
                      ("hub8", lambda: chain_hub(34000, 8, seed=8), 300),
                      ("band2048", lambda: edge_graph(2048, 4), 1029),
                      ("band2049", lambda: edge_graph(2049, 4), 1029)):
    g = make()
    plan = cpd.Plan(g)
    dev = cpd.Graph(plan, batch=1024)
    targets = np.random.default_rng(4).permutation(g.n).astype(np.uint32)[:k]
    rows = dev.build_rows(targets)
    off, runs = rows.export()
    ref_off, ref_runs = oracle.build_rows(g.row_ptr, g.dst, g.w, plan.order(), targets)
    mv = rows.export_moves()
    ref_mv = oracle.moves_from_runs(ref_off, ref_runs, g.n, rows.move_bits())
    out[name] = {"offsets": bool(np.array_equal(off, ref_off)),
                 "runs": bool(np.array_equal(runs, ref_runs)),
                 "moves": bool(np.array_equal(mv, ref_mv)),
                 "tiles": (g.n + 2047) // 2048, "bits": rows.move_bits(),
                 "runs_per_row": float(ref_off[-1]) / k}
print(json.dumps(out))
"""


def test_unfused_rle_past_one_tile():
    code = CHILD_UNFUSED % (HERE, os.path.join(ROOT, "distributed-oracle-search_amd"),
                            os.path.join(ROOT, "oracle"))
    env = dict(os.environ, CPD_RLE_FUSED="0")
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    shape = {k: (v["tiles"], v["bits"]) for k, v in res.items()}
    assert shape == {"synth70": (3, 2), "chain": (17, 1), "hub8": (17, 4), "band2048": (1, 2),
                     "band2049": (2, 2)}, shape
    assert res["chain"]["runs_per_row"] < 8 and res["hub8"]["runs_per_row"] < 16
    for name, v in res.items():
        assert v["offsets"] and v["runs"] and v["moves"], (name, v)
