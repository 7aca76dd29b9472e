"""fifo_auto's start-up contract, without a GPU and without an index: which
flag combinations are refused, with which exit status and exactly which text,
and which message wins when two rules are broken at once (the order of the
checks).  Every refusal happens before anything is read or made, so every row
runs against an empty directory and leaves no FIFO behind.  The texts are
literals: what bin/fifo_auto printed when this table was written."""
import os
import subprocess

import pytest

import driver_harness as H

USAGE = """\
usage: fifo_auto --input X.xy [DIFF] --partmethod {div|mod} --partkey K --workerid I --maxworker W --outdir D --alg table-search|cpd-search
       [--paths]  table-search only: answer through cpd_query_paths and write every
                  walk's nodes to <query file>.paths, one line per query:
                  s t finished n v0 ... v(n-1)
       [--search-paths]  cpd-search only: answer through cpd_query_search_paths and
                  write every route's nodes to <query file>.paths, same format
       [--search-loads]  cpd-search only: answer through cpd_query_search_loads (demand 1
                  per query) and write every loaded edge of the routes found to
                  <query file>.loads: edge from to load
       [--costs [--slice-moves S]]  table-search only: the request's diff field may list
                  up to 8 diffs ("-,a.diff,b.diff"); one walk costs every query under each
                  (cpd_query_costs) and <query file>.res gets, per query:
                  s t moves finished cost_0 ... cost_{C-1}
                  (with --slice-moves S one cost: move h under diff min(h / S, last));
                  "debug": true in a request adds nothing: .res is the costs file
       [--loads [--load-slices K --load-slice-moves S]]  table-search only: answer through
                  cpd_query_loads (demand 1 per query) and write every loaded edge to
                  <query file>.loads: edge from to load_0 ... load_{K-1}
                  (K slices: move h counts in slice min(h / S, K - 1))
       [--timed P [--loads]]  table-search only: answer through cpd_query_timed; the
                  request's diff field lists up to 8 diffs, diff j the network during clock
                  time [j P, (j + 1) P); departures from <query file>.dep (one per query
                  line; absent: 0); <query file>.res gets, per query:
                  s t moves finished depart cost
                  (with --loads <query file>.loads has one column per diff)
       [--assign K --capacity C [--vdf A/B^P]]  cpd-search only: answer through
                  cpd_query_assign (K iterations, demand 1 per query, every edge at capacity C,
                  delay w0 (1 + A/B (x/C)^P), default 3/20^4); writes <query file>.loads,
                  .assign (k finished sptt tstt moves changed) and .diff (the final weights)
       [--step msa|line|conj]  with --assign: msa (default) as above; line answers through
                  cpd_query_assign_line (the line-search step): .assign lines end in
                  lambda g0 xw0, .loads holds the final flow's volumes; conj answers through
                  cpd_query_assign_conj (the conjugate step): .assign lines end in lambda gy xw0 alpha
"""
ALG = "fifo_auto: --alg must be table-search or cpd-search (got '%s')\n"
PATHS = ("fifo_auto: --paths needs --alg table-search (the paths of a cpd-search are extracted "
         "with --search-paths)\n")
SEARCH_PATHS = ("fifo_auto: --search-paths needs --alg cpd-search (the walks of a table-search "
                "are extracted with --paths)\n")
COSTS = ("fifo_auto: --costs needs --alg table-search without --paths (a cpd-search's route "
         "depends on the weights; --paths answers through cpd_query_paths)\n")
SLICE_MOVES = "fifo_auto: --slice-moves S needs --costs and 0 <= S < 2^32\n"
LOADS = ("fifo_auto: --loads needs --alg table-search without --paths or --costs (a cpd-search's "
         "route is not the walk's: --search-loads loads it; --paths and --costs answer through "
         "cpd_query_paths and cpd_query_costs)\n")
TIMED = ("fifo_auto: --timed needs --alg table-search without --paths, --costs, --load-slices or "
         "--load-slice-moves (a cpd-search's route is not the walk's; --paths and --costs answer "
         "through cpd_query_paths and cpd_query_costs; a timed walk's load planes are its "
         "diffs)\n")
PERIOD = "fifo_auto: --timed P needs 1 <= P <= 2^60\n"
SEARCH_LOADS = ("fifo_auto: --search-loads needs --alg cpd-search without --search-paths, "
                "--load-slices or --load-slice-moves (the walks of a table-search are loaded with "
                "--loads; --search-paths answers through cpd_query_search_paths; a search loads "
                "one plane)\n")
LOAD_SLICES = ("fifo_auto: --load-slices K --load-slice-moves S need --loads, 2 <= K <= 8 and "
               "0 < S < 2^32 (both or neither)\n")
ASSIGN = ("fifo_auto: --assign needs --alg cpd-search without --search-paths, --search-loads, "
          "--loads or --timed (the loop answers through cpd_query_assign and writes the loads "
          "itself)\n")
CAPACITY = "fifo_auto: --capacity and --vdf need --assign\n"
RANGES = ("fifo_auto: --assign K --capacity C [--vdf A/B^P] need 1 <= K <= 65535, 1 <= C < 2^32, "
          "A <= 65535, 1 <= B <= 65535 and 1 <= P <= 4\n")
STEP = "fifo_auto: --step msa|line|conj needs --assign\n"
PARTMETHOD = "partmethod must be 'div' or 'mod', got '%s'\n"

TS, CS = ["--alg", "table-search"], ["--alg", "cpd-search"]
LOOP = ["--assign", "3", "--capacity", "2"]

# (extra argv, exit status, exact stderr[, what replaces a default of the command line])
ROWS = [
    # one row per refusal, in the order of the checks
    ([], 2, USAGE, {"workerid": "2"}),
    (["--alg", "astar"], 2, ALG % "astar"),
    (CS + ["--paths"], 2, PATHS),
    (TS + ["--search-paths"], 2, SEARCH_PATHS),
    (["--search-paths"], 2, SEARCH_PATHS),               # --alg defaults to table-search
    (CS + ["--costs"], 2, COSTS),
    (TS + ["--slice-moves", "4"], 2, SLICE_MOVES),
    (TS + ["--costs", "--slice-moves", "-1"], 2, SLICE_MOVES),
    (TS + ["--costs", "--slice-moves", str(1 << 32)], 2, SLICE_MOVES),
    (CS + ["--loads"], 2, LOADS),
    (CS + ["--timed", "100"], 2, TIMED),
    (TS + ["--timed", "0"], 2, PERIOD),
    (TS + ["--timed"], 2, PERIOD),                       # no value reads as 0
    (TS + ["--search-loads"], 2, SEARCH_LOADS),
    (TS + ["--load-slices", "3", "--load-slice-moves", "4"], 2, LOAD_SLICES),
    (TS + ["--loads", "--load-slices", "9", "--load-slice-moves", "4"], 2, LOAD_SLICES),
    (TS + ["--loads", "--load-slices", "3"], 2, LOAD_SLICES),
    (TS + LOOP, 2, ASSIGN),
    (CS + ["--capacity", "2"], 2, CAPACITY),
    (CS + ["--vdf", "3/20^4"], 2, CAPACITY),
    (CS + ["--assign", "3"], 2, RANGES),
    (CS + ["--assign", "65536", "--capacity", "2"], 2, RANGES),
    (CS + ["--assign", "3", "--capacity", str(1 << 32)], 2, RANGES),
    (CS + ["--vdf", "3/0^4"] + LOOP, 2, RANGES),
    (CS + ["--vdf", "3/20^4x"] + LOOP, 2, RANGES),
    (CS + ["--step", "line"], 2, STEP),
    # what the driver tests try (tests/test_gpu_*_driver.py), beyond the rows above
    (TS + ["--paths", "--costs"], 2, COSTS),
    (TS + ["--paths", "--loads"], 2, LOADS),
    (TS + ["--costs", "--loads"], 2, LOADS),
    (TS + ["--paths", "--timed", "100"], 2, TIMED),
    (TS + ["--costs", "--timed", "100"], 2, TIMED),
    (TS + ["--timed", "100", "--loads", "--load-slices", "2", "--load-slice-moves", "3"], 2,
     TIMED),
    (TS + ["--timed", "100", "--load-slice-moves", "3"], 2, TIMED),
    (TS + ["--timed", str((1 << 60) + 1)], 2, PERIOD),
    (CS + ["--search-paths", "--search-loads"], 2, SEARCH_LOADS),
    (CS + ["--search-loads", "--load-slices", "3", "--load-slice-moves", "4"], 2, SEARCH_LOADS),
    (CS + ["--search-paths"] + LOOP, 2, ASSIGN),
    (CS + ["--search-loads"] + LOOP, 2, ASSIGN),
    (CS + ["--loads"] + LOOP, 2, LOADS),
    (CS + ["--timed", "100"] + LOOP, 2, TIMED),
    (CS + ["--assign", "0", "--capacity", "2"], 2, RANGES),
    (CS + ["--vdf", "3/20^5"] + LOOP, 2, RANGES),
    (CS + ["--step", "msa"], 2, STEP),
    (CS + ["--step", "conj"], 2, STEP),
    (CS + ["--step", "fw"] + LOOP, 2, STEP),
    # two rules broken at once: the earlier check's message wins
    (["--alg", "astar", "--paths"], 2, ALG % "astar"),
    (CS + ["--paths", "--costs"], 2, PATHS),
    (TS + ["--search-paths"] + LOOP, 2, SEARCH_PATHS),
    (CS + ["--costs", "--loads"], 2, COSTS),
    (TS + ["--paths", "--costs", "--loads"], 2, COSTS),
    (TS + ["--slice-moves", "4", "--loads"], 2, SLICE_MOVES),
    (TS + ["--timed", "0", "--paths"], 2, TIMED),
    (CS + ["--timed", "0"], 2, TIMED),
    (TS + ["--timed", "0", "--search-loads"], 2, PERIOD),
    (TS + ["--loads", "--load-slices", "1", "--load-slice-moves", "4"], 2, LOAD_SLICES),
    (TS + ["--search-loads", "--load-slices", "3"], 2, SEARCH_LOADS),
    (CS + ["--search-loads", "--search-paths"] + LOOP, 2, SEARCH_LOADS),
    (TS + ["--load-slices", "3"] + LOOP, 2, LOAD_SLICES),
    (TS + ["--assign", "0"], 2, ASSIGN),
    (CS + ["--step", "line", "--vdf", "3/20^4"], 2, CAPACITY),
    (CS + ["--assign", "0", "--capacity", "2", "--step", "fw"], 2, RANGES),
    (CS + ["--paths"], 2, PATHS, {"partmethod": "hash"}),  # the flag checks come first
    (["--alg", "astar"], 2, USAGE, {"workerid": "2"}),
    # cli.hpp's own refusals
    (TS, 2, PARTMETHOD % "hash", {"partmethod": "hash"}),
    (CS + LOOP + ["--step", "conj"], 2, PARTMETHOD % "hash", {"partmethod": "hash"}),
    (TS, 2, "unexpected argument 'stray'\n", {"lead": ["stray"]}),
]


def _run(tmp_path, extra, partmethod="mod", workerid="0", lead=()):
    argv = [os.path.join(H.BIN, "fifo_auto")] + list(lead) + [
        "--input", str(tmp_path / "g.xy"), str(tmp_path / "g.xy.diff"), "--partmethod",
        partmethod, "--partkey", "3", "--workerid", workerid, "--maxworker", "2", "--outdir",
        str(tmp_path / "index"), "--fifo", str(tmp_path / "never.fifo")] + extra
    return subprocess.run(argv, capture_output=True, text=True, timeout=60)


def _row_id(row):
    return " ".join(row[0] + [f"{k}={v}" for k, v in (row[3] if len(row) > 3 else {}).items()])


@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_refused_at_start(tmp_path, row):
    extra, status, stderr = row[:3]
    p = _run(tmp_path, extra, **(row[3] if len(row) > 3 else {}))
    assert (p.returncode, p.stderr, p.stdout) == (status, stderr, "")
    assert os.listdir(tmp_path) == []  # nothing read, nothing made: no FIFO either


@pytest.mark.parametrize("extra", [TS, CS + LOOP + ["--step", "line"]], ids=["plain", "assign"])
def test_failed_load_removes_the_fifo(tmp_path, extra):
    """Valid flags, no index: the FIFO is made before the load, the load fails
    at the order file (before any GPU is asked for) and takes the FIFO away."""
    p = _run(tmp_path, extra)
    assert p.returncode == 1 and p.stdout == ""
    lines = p.stderr.splitlines()
    assert len(lines) == 1 and lines[0].startswith("fifo_auto: ")
    assert str(tmp_path / "index") in lines[0]  # names what it could not open
    assert not os.path.lexists(tmp_path / "never.fifo")
