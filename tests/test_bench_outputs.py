"""bench.py's plain line (no --full) and --dump-outputs: the line of a run
without the query legs, and the dumped arrays against the rows' own export."""
import os

import numpy as np
import pytest

import bench


def test_plain_line_has_the_headline_and_no_query_figures():
    args = bench.parse(["--steps", "4", "--warmup", "1", "--width", "40"])
    assert not args.full and args.dump_outputs == ""
    assert bench.parse(["--full", "--dump-outputs", "d"]).full
    out = bench.assemble(args, 1, (1600, 4000), 1024, 0.5, None, 0.0, 1024, 2048, {}, None, None,
                         None)
    assert out["value"] == pytest.approx(4 * 1024 / 0.5)
    assert out["ms_per_step"] == pytest.approx(125.0)
    assert out["steps"] == 4 and out["warmup"] == 1
    assert out["unit"] == "sources/s" and out["higher_is_better"] is True and out["dtype"] == "u32"
    assert out["queries_per_s"] is None and out["query_mean_moves"] is None
    assert out["cpu_baseline"] is None and out["step_pmc"] is None


@pytest.mark.gpu
def test_dump_outputs_matches_export(small_graph, tmp_path, monkeypatch):
    import cpd
    g = small_graph
    dev = cpd.Graph(cpd.Plan(g), device=0, batch=1024)
    targets = np.arange(3, 3 + 200, dtype=np.uint32)
    rows = dev.build_rows(targets)
    off, runs = rows.export()
    # a run budget small enough that the per-row cap cuts some rows
    monkeypatch.setattr(bench, "DUMP_RUNS_BYTES", 8 * bench.DUMP_ROWS * 40)
    d = str(tmp_path / "dump")
    bench.dump_outputs(d, rows, targets)
    bench.dump_outputs(d, rows, targets)  # same rows, same files
    a = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert sorted(a) == ["offsets", "sample_moves", "sample_rows", "sample_run_counts",
                         "sample_runs", "targets"]
    assert all(v.dtype == np.float64 for v in a.values())
    assert np.array_equal(a["targets"], targets) and np.array_equal(a["offsets"], off)
    pick = a["sample_rows"].astype(np.int64)
    assert len(pick) == bench.DUMP_ROWS and np.all(np.diff(pick) > 0) and pick[-1] < len(targets)
    assert np.array_equal(a["sample_run_counts"], (off[pick + 1] - off[pick]))
    want = np.concatenate([runs[int(off[r]):int(off[r + 1])][:40] for r in pick])
    assert np.array_equal(a["sample_runs"], want)
    assert np.array_equal(a["sample_moves"], np.stack([rows.export_moves(int(r), 1)[0] for r in pick]))
