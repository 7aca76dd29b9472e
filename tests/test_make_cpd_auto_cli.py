"""make_cpd_auto's start-up contract, without a GPU: which arguments are
refused, with which exit status and exactly which text, and which message wins
when two rules are broken at once (the order of the checks).  Every refusal
happens before anything is read or made, so every row names an --input that
does not exist and leaves its directory empty.  The texts are literals: what
bin/make_cpd_auto printed when this table was written.  Then, on an 8 x 6
graph, the ways out that need no GPU: --plan-only, a scenario target outside
the graph, and the plain run on a machine without one."""
import os
import subprocess

import pytest

import cpd
import driver_harness as H

EXE = os.path.join(H.BIN, "make_cpd_auto")

USAGE = ("usage: make_cpd_auto --input X.xy --partmethod|--partition {div|mod} --partkey K "
         "--workerid I --maxworker W [--outdir D] [--device G] [--batch B] [--no-arena] "
         "[--arena-touch] [--threads T] [--ch-host] [--plan P | --no-plan-cache] "
         "[--write-threads T] [--no-pipeline] [--plan-only] [--targets-from SCEN] "
         "[--format moves|rle] [--stripes K] [--discard] [--hbm-reserve GIB] [--verbose]\n")
PARTMETHOD = "partmethod must be 'div' or 'mod', got '%s'\n"
FORMAT = "make_cpd_auto: --format must be moves or rle\n"
STRIPES = "make_cpd_auto: --stripes must be in [1, 4096]\n"
DISCARD = "make_cpd_auto: --discard needs the pipelined writer\n"
NO_XY = "make_cpd_auto: cannot open %s\n"
SINK = ["--discard", "--no-pipeline"]

# (extra argv, exit status, exact stderr[, what replaces a default of the command line])
ROWS = [
    # one row per refusal, in the order of the checks
    ([], 2, USAGE, {"bare": True}),                      # no arguments at all
    ([], 2, USAGE, {"workerid": "2"}),                   # --workerid >= --maxworker
    ([], 2, USAGE, {"workerid": "3"}),
    ([], 2, PARTMETHOD % "x", {"partmethod": "x"}),
    (["--format", "x"], 2, FORMAT),
    (["--stripes", "0"], 2, STRIPES),
    (["--stripes", "4097"], 2, STRIPES),
    (SINK, 1, DISCARD),
    ([], 2, "unexpected argument 'stray'\n", {"lead": ["stray"]}),
    # two rules broken at once: the earlier check's message wins
    (["--format", "x"], 2, USAGE, {"workerid": "2", "partmethod": "x"}),
    (["--format", "x"], 2, PARTMETHOD % "x", {"partmethod": "x"}),
    (SINK, 2, PARTMETHOD % "hash", {"partmethod": "hash"}),
    (["--format", "x", "--stripes", "0"], 2, FORMAT),
    (["--format", "x"] + SINK, 2, FORMAT),
    (["--stripes", "4097"] + SINK, 2, STRIPES),
    (SINK, 2, "unexpected argument 'stray'\n", {"lead": ["stray"], "workerid": "2"}),
    # the two layouts and the stripe counts at the edges pass the checks: the read refuses
    (["--format", "rle", "--stripes", "1"], 1, NO_XY),
    (["--format", "moves", "--stripes", "4096"], 1, NO_XY),
]


def _run(tmp_path, extra, partmethod="mod", workerid="1", lead=(), bare=False):
    argv = [EXE] if bare else [EXE] + list(lead) + [
        "--input", str(tmp_path / "g.xy"), "--partmethod", partmethod, "--partkey", "5",
        "--workerid", workerid, "--maxworker", "2", "--outdir", str(tmp_path / "index")] + extra
    return subprocess.run(argv, capture_output=True, text=True, timeout=60)


def _row_id(row):
    return " ".join(row[0] + [f"{k}={v}" for k, v in (row[3] if len(row) > 3 else {}).items()])


@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_refused_at_start(tmp_path, row):
    extra, status, stderr = row[:3]
    p = _run(tmp_path, extra, **(row[3] if len(row) > 3 else {}))
    if stderr is NO_XY:  # past the flag checks: --outdir is made, then the .xy is not there
        assert (p.returncode, p.stderr, p.stdout) == (status, stderr % (tmp_path / "g.xy"), "")
        assert os.listdir(tmp_path) == ["index"] and os.listdir(tmp_path / "index") == []
        return
    assert (p.returncode, p.stderr, p.stdout) == (status, stderr, "")
    assert os.listdir(tmp_path) == []  # nothing read, nothing made: no --outdir either


@pytest.fixture
def small(tmp_path):
    """An 8 x 6 gen_synth graph (48 nodes) and the command line of worker 0 of 2."""
    prefix = str(tmp_path / "s")
    subprocess.run([os.path.join(H.BIN, "gen_synth"), "--width", "8", "--height", "6", "--seed",
                    "3", "--out", prefix, "--queries", "20"], check=True, capture_output=True)
    out = tmp_path / "idx"
    return out, [EXE, "--input", prefix + ".xy", "--partmethod", "mod", "--partkey", "2",
                 "--workerid", "0", "--maxworker", "2", "--outdir", str(out)]


def test_plan_only_needs_no_gpu(small):
    """--plan-only warms the plan cache and stops: no order file, no bucket.
    (--ch-host: the hierarchy on host threads wherever this runs.)"""
    out, cmd = small
    p = subprocess.run(cmd + ["--plan-only", "--ch-host"], capture_output=True, text=True,
                       timeout=60)
    assert p.returncode == 0 and p.stderr == "", p.stderr
    lines = p.stdout.splitlines()
    assert len(lines) == 2 and lines[0].startswith("make_cpd_auto: built and cached plan ")
    assert lines[1].startswith("make_cpd_auto: plan ready in ")
    files = os.listdir(out)  # the plan and the cache's lock file
    plan, = [f for f in files if f.endswith(".plan")]
    assert lines[0].endswith(" " + str(out / plan))
    assert not [f for f in files if f.endswith(".order") or ".cpd" in f]


def test_scenario_target_out_of_range(small, tmp_path):
    """--targets-from: a target that is no node is an error of the read,
    before the preflight, the plan and any device work."""
    out, cmd = small
    scen = tmp_path / "bad.scen"
    scen.write_text("q 0 47\nq 1 48\n")
    p = subprocess.run(cmd + ["--targets-from", str(scen)], capture_output=True, text=True,
                       timeout=60)
    assert (p.returncode, p.stderr, p.stdout) == (
        1, "make_cpd_auto: scenario target out of range\n", "")
    assert os.listdir(out) == []


def test_no_gpu_is_refused_before_the_order_file(small):
    if cpd.device_count() == 0:
        out, cmd = small
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1
        assert p.stderr == "make_cpd_auto: no GPU visible (this build has no CPU path)\n"
        assert not [f for f in os.listdir(out) if f.endswith(".order") or ".cpd" in f]
