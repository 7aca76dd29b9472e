"""GPU: what the host side of the query calls (cpd_query_prepare .. _fetch and
the two search calls' tails) promises beside its results: the timing ledger
each call books (the keys, launches and bytes per key, the bytes against a
Python restatement of the models the library's comments state), the call
stats against each other and against the fetched arrays, and the code and
whole text of every refusal a small graph can reach.  Batches of 0, 1 and 65
queries (one past the 64-query chunk unit), RLE and dense rows, a graph with
unreachable pairs, parallel edges and a wide node and one of adjacency shift 3."""
import ctypes as C
import math

import numpy as np
import pytest

import cpd
from test_gpu_paths import draw, world

pytestmark = pytest.mark.gpu
MODES = ["rle", "dense"]
WORLDS = {"irregular": 4, "deg8": 3}  # name -> adjacency shift
BATCHES = [0, 1, 65]
_worlds = {}


def shared(name):
    """world(name), built once for the module and never changed; its device
    graph has timing on."""
    if name not in _worlds:
        _worlds[name] = world(name)
        _worlds[name][2].timing(True)
    return _worlds[name]


def index(dev, rows, mode):
    ix = cpd.Index(dev, rows=rows)
    ix.set_mode(mode)
    assert ix.mode == mode
    return ix


def weight_sets(g, k):
    return [None] + [cpd.synth_congestion(g.w, frac=0.3, lo=1.0, hi=3.0, seed=40 + j)
                     for j in range(1, k)]


def walk_bytes(mode, off, nq, moves):
    """walk_model_bytes: dense, per query 8 (s, t) + 13 (outputs) + 4 (row) and
    per move a 4-B move word + an 8-B packed edge; RLE, SURVEY.md 8(d): 28 per
    query, per move 4 ceil(log2 R) + 16 at the mean over the rows."""
    if mode == "dense":
        return 25.0 * nq + 12.0 * float(moves)
    lens = np.diff(off.astype(np.int64))
    mean_log = sum(math.ceil(math.log2(max(2, int(r)))) for r in lens) / len(lens)
    return 28.0 * nq + float(moves) * (4.0 * mean_log + 16.0)


def booked(dev, call, *args, **kw):
    """(what the call returns, the ledger it alone booked)."""
    dev.timing_reset()
    out = call(*args, **kw)
    return out, dev.timing_get()


def expect(ledger, want):
    """want: key -> (launches, bytes); the keys are all the call booked."""
    assert set(ledger) == set(want)
    for key, (launches, nbytes) in want.items():
        assert ledger[key]["launches"] == launches, key
        # sums of fewer than ten terms below 2^53
        assert ledger[key]["bytes"] == pytest.approx(nbytes, rel=1e-12, abs=0), key
        assert ledger[key]["ms"] >= 0.0, key


def lib_fetch(fn, ix, nq, cols=None):
    cost = np.empty(nq if cols is None else (nq, cols), np.uint64)
    hops = np.empty(nq, np.uint32)
    fin = np.empty(nq, np.uint8)
    cpd._check(fn(ix._h, cpd._ptr(cost, cpd.u64p), cpd._ptr(hops, cpd.u32p),
                  cpd._ptr(fin, cpd.u8p)))
    return cost, hops, fin


@pytest.mark.parametrize("nq", BATCHES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("graph", list(WORLDS))
def test_ledger_walks(graph, mode, nq):
    g, plan, dev, targets, rows, order, off, runs = shared(graph)
    ix = index(dev, rows, mode)
    s65, t65 = draw(g, targets, 65, seed=31)
    ix.query(s65, t65)  # the dense tables are made here, under their own keys
    s, t = s65[:nq], t65[:nq]
    rng = np.random.default_rng(32)
    demand = rng.integers(0, 1 << 32, nq, dtype=np.uint64).astype(np.uint32)
    depart = rng.integers(0, 40, nq, dtype=np.uint64)

    def key(stem):
        return stem + ("_dense" if mode == "dense" else "")

    def walk(st):
        assert st["queries"] == nq
        return walk_bytes(mode, off, nq, st["hops"])

    ix.prepare(s, t)
    st, led = booked(dev, ix.run)
    expect(led, {key("table_search"): (1, walk(st))})

    (poff, st), led = booked(dev, ix.paths_run)
    want = {key("table_search"): (1, walk(st))}
    if nq:  # the empty batch ends after the walk
        total = int(poff[-1])
        assert total == st["hops"] + nq
        want["table_paths_offsets"] = (1, 44.0 * nq)
        want[key("table_paths")] = (1, walk(st) + 4.0 * total + 8.0 * nq)
    expect(led, want)

    # costs: the walk + a record (sliced: one word) per move + the stored columns
    sets = weight_sets(g, 5)
    for nsets, words in ((3, 4), (5, 8)):
        ix.set_weight_sets(sets[:nsets])
        for slice_moves in (0, 2):
            st, led = booked(dev, ix.costs_run, -1, slice_moves)
            cols = 1 if slice_moves else nsets
            per_move = 4.0 if slice_moves else 4.0 * words
            expect(led, {key("table_costs"): (1, walk(st) + per_move * st["hops"] +
                                              8.0 * cols * nq)})

    # loads: the walk + a demand and its index per query + a counter per move
    for dem in (None, demand):
        for slices, slice_moves in ((1, 0), (3, 2)):
            st, led = booked(dev, ix.loads_run, dem, -1, slices, slice_moves)
            per_q = 8.0 if dem is not None and nq else 0.0
            expect(led, {key("table_loads"): (1, walk(st) + per_q * nq + 8.0 * st["hops"])})

    # timed: the walk + a record per move (+ a counter with loads) + the
    # permutation word and what is read through it per query + the stored cost
    ix.set_weight_sets(sets[:3])
    for dep in (None, depart):
        for dem in (None, demand):
            for loads in (False, True):
                st, led = booked(dev, ix.timed_run, dep, 5, dem, -1, loads)
                per_q = (8.0 if dep is not None and nq else 0.0) + \
                        (4.0 if loads and dem is not None and nq else 0.0)
                expect(led, {key("table_timed"): (
                    1, walk(st) + (4.0 * 4 + (8.0 if loads else 0.0)) * st["hops"] +
                    (per_q + 4.0) * nq + 8.0 * nq)})


@pytest.mark.parametrize("nq", BATCHES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("graph", list(WORLDS))
def test_ledger_search(graph, mode, nq):
    """The two search calls' own keys (the table-building keys beside them vary)."""
    g, plan, dev, targets, rows, order, off, runs = shared(graph)
    ix = index(dev, rows, mode)
    s, t = draw(g, targets, 65, seed=33)
    s, t = s[:nq], t[:nq]
    demand = np.random.default_rng(34).integers(0, 1 << 32, nq, dtype=np.uint64).astype(np.uint32)
    ix.prepare(s, t)

    (poff, st), led = booked(dev, ix.search_paths_run)
    assert led["cpd_search"]["launches"] == st["passes"] and (st["passes"] > 0) == (nq > 0)
    if nq:  # nodes written, prefixes read
        info = st["paths"]
        assert info["nodes"] == int(poff[-1])
        assert led["search_paths"]["launches"] == 1
        assert led["search_paths"]["bytes"] == pytest.approx(
            4.0 * info["nodes"] + 4.0 * info["prefix_nodes"], rel=1e-12, abs=0)
    else:  # the empty batch ends before its own key
        assert "search_paths" not in led and poff.tolist() == [0]

    for dem in (None, demand):
        st, led = booked(dev, ix.search_loads_run, dem)
        assert led["cpd_search"]["launches"] == st["passes"] and (st["passes"] > 0) == (nq > 0)
        if nq:  # a counter per move, the prefixes read, a row per prefix move
            info = st["loads"]
            assert led["search_loads"]["launches"] == 2
            assert led["search_loads"]["bytes"] == pytest.approx(
                8.0 * info["moves"] + 4.0 * info["prefix_nodes"] +
                8.0 * (info["prefix_moves"] << WORLDS[graph]), rel=1e-12, abs=0)
        else:
            assert "search_loads" not in led


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("graph", list(WORLDS))
def test_stats_agree(graph, mode):
    """One prepared batch: queries / finished / hops of run, loads, costs and a
    timed walk of one set without departures are the same, and those of the
    arrays each of them fetches."""
    g, plan, dev, targets, rows, order, off, runs = shared(graph)
    ix = index(dev, rows, mode)
    ix.set_weight_sets([None])
    s, t = draw(g, targets, 65, seed=35)
    ix.prepare(s, t)
    got = []
    for run, fetch in ((ix.run, lambda: lib_fetch(cpd.lib.cpd_query_fetch, ix, 65)),
                       (ix.loads_run, lambda: lib_fetch(cpd.lib.cpd_query_fetch, ix, 65)),
                       (ix.costs_run, lambda: ix.costs_fetch()),
                       (lambda: ix.timed_run(period=3), lambda: ix.timed_fetch())):
        st = run()
        cost, hops, fin = fetch()
        assert st["queries"] == 65
        assert st["finished"] == int(fin.sum()) and st["hops"] == int(hops.sum())
        got.append((st["queries"], st["finished"], st["hops"]))
    assert len(set(got)) == 1
    if graph == "irregular":  # the unfinished walks are there
        assert 0 < got[0][1] < 65


def refused(code, msg, call, *args, **kw):
    with pytest.raises(cpd.CpdError) as e:
        call(*args, **kw)
    assert e.value.code == code
    assert str(e.value) == f"libcpd error {code}: {msg}"


def lib_refused(code, msg, rc):
    """rc: what a call of cpd.lib itself returned (the wrapper would refuse first)."""
    assert rc == code
    assert cpd.lib.cpd_last_error().decode() == msg


@pytest.mark.parametrize("mode", MODES)
def test_refusals_incomplete_index(mode):
    g, plan, dev, targets, rows, order, off, runs = shared("deg8")
    part = cpd.Index.streamed(dev, targets, int(off[-1]), mode=mode)
    part.append(off[:8], runs[:int(off[7])])
    part.set_weight_sets([None])
    s, t = draw(g, targets, 65, seed=36)
    tail = f"index incomplete (7 of {len(targets)} rows appended)"
    refused(cpd.CPD_E_ARG, "query: " + tail, part.prepare, s, t)
    refused(cpd.CPD_E_ARG, "costs: " + tail, part.costs_run)
    refused(cpd.CPD_E_ARG, "loads: " + tail, part.loads_run)
    refused(cpd.CPD_E_ARG, "timed: " + tail, part.timed_run, period=1)


def test_refusals_arguments():
    g, plan, dev, targets, rows, order, off, runs = shared("deg8")
    ix = index(dev, rows, "rle")
    s, t = draw(g, targets, 65, seed=37)
    E = cpd.CPD_E_ARG
    # query preparation
    lib_refused(E, "query: null argument",
                cpd.lib.cpd_query_prepare(ix._h, None, None, C.c_uint32(1)))
    bad = s.copy()
    bad[9] = g.n
    refused(E, "query node out of range", ix.prepare, bad, t)
    stray = int(np.setdiff1d(np.arange(g.n, dtype=np.uint32), targets)[0])
    bad = t.copy()
    bad[9] = stray
    refused(cpd.CPD_E_NOROW, f"target {stray} has no CPD row in this index", ix.prepare, s, bad)
    ix.prepare(s, t)
    # no weight sets
    refused(E, "costs: no weight sets loaded (cpd_index_set_weight_sets)", ix.costs_run)
    refused(E, "timed: no weight sets loaded (cpd_index_set_weight_sets)", ix.timed_run, period=1)
    # the slices of a loads call
    refused(E, "loads: 0 slices, 1 to 8", ix.loads_run, slices=0)
    refused(E, "loads: 9 slices, 1 to 8", ix.loads_run, slices=9, slice_moves=1)
    for slices, slice_moves in ((2, 0), (1, 3)):
        refused(E, "loads: slice_moves must be 0 with one slice and non-zero with more",
                ix.loads_run, slices=slices, slice_moves=slice_moves)
    # a timed call's flags, period and departures
    ix.set_weight_sets(weight_sets(g, 2))
    refused(E, "timed: CPD_LOADS_ACCUMULATE without CPD_TIMED_LOADS", ix.timed_run, period=1,
            accumulate=True)
    refused(E, "timed: period 0, 1 to 2^60", ix.timed_run, period=0)
    refused(E, f"timed: period {(1 << 60) + 1}, 1 to 2^60", ix.timed_run, period=(1 << 60) + 1)
    depart = np.zeros(65, np.uint64)
    depart[3] = 1 << 63
    refused(E, "timed: departure 9223372036854775808 of query 3, must be below 2^63",
            ix.timed_run, depart, 1)
    refused(E, "search loads: unknown flag bits 6", ix.search_loads_run, flags=7)
    lib_refused(E, "paths: null argument",
                cpd.lib.cpd_query_paths(ix._h, C.c_int32(-1), None, None))
    lib_refused(E, "null index", cpd.lib.cpd_query_run(None, C.c_int32(-1), None))


def test_refusals_accumulate():
    """A load table is of one kind, accumulated into only by its own."""
    g, plan, dev, targets, rows, order, off, runs = shared("deg8")
    ix = index(dev, rows, "dense")
    ix.set_weight_sets(weight_sets(g, 2))
    s, t = draw(g, targets, 65, seed=38)
    E = cpd.CPD_E_ARG
    ix.prepare(s, t)
    ix.timed_run(period=7, loads=True)
    timed = ix.loads_fetch()
    refused(E, "loads: accumulate into the table of a timed walk (period 7)", ix.loads_run,
            accumulate=True)
    refused(E, "search loads: accumulate into the table of a timed walk (period 7)",
            ix.search_loads_run, accumulate=True)
    refused(E, "timed: accumulate into a table of 2 planes of period 7 asked with 2 sets of "
               "period 9", ix.timed_run, period=9, loads=True, accumulate=True)
    np.testing.assert_array_equal(ix.loads_fetch(), timed)  # the table stays
    ix.loads_run(slices=3, slice_moves=2)
    sliced = ix.loads_fetch()
    refused(E, "loads: accumulate into a table of 3 slices of 2 moves asked with 2 of 2",
            ix.loads_run, slices=2, slice_moves=2, accumulate=True)
    refused(E, "timed: accumulate into a table of 3 planes of 2 moves asked with 2 sets of "
               "period 9", ix.timed_run, period=9, loads=True, accumulate=True)
    refused(E, "search loads: accumulate into a table of 3 slices of 2 moves: a search loads "
               "one plane", ix.search_loads_run, accumulate=True)
    np.testing.assert_array_equal(ix.loads_fetch(), sliced)


def test_refusals_fetch():
    g, plan, dev, targets, rows, order, off, runs = shared("irregular")
    ix = index(dev, rows, "rle")
    ix.set_weight_sets([None])
    s, t = draw(g, targets, 65, seed=39)
    ix.prepare(s, t)
    E = cpd.CPD_E_ARG
    out = np.zeros(4 * max(65, g.m), np.uint64)
    p64, p32, p8 = (cpd._ptr(out, p) for p in (cpd.u64p, cpd.u32p, cpd.u8p))
    none_yet = "paths fetch: no cpd_query_paths / cpd_query_search_paths on the prepared queries yet"
    lib_refused(E, none_yet, cpd.lib.cpd_query_paths_fetch(ix._h, C.c_uint32(0), C.c_uint32(1), p32))
    lib_refused(E, "costs fetch: no cpd_query_costs on the prepared queries yet",
                cpd.lib.cpd_query_costs_fetch(ix._h, p64, p32, p8))
    lib_refused(E, "timed fetch: no cpd_query_timed on the prepared queries yet",
                cpd.lib.cpd_query_timed_fetch(ix._h, p64, p32, p8))
    lib_refused(E, "loads fetch: no cpd_query_loads on this index since it was made or cleared",
                cpd.lib.cpd_query_loads_fetch(ix._h, p64))
    # each run opens its own fetch; a new batch closes the three of the batch
    ix.paths_run()
    ix.costs_run()
    ix.timed_run(period=2)
    assert cpd.lib.cpd_query_costs_fetch(ix._h, p64, p32, p8) == cpd.CPD_OK
    assert cpd.lib.cpd_query_timed_fetch(ix._h, p64, p32, p8) == cpd.CPD_OK
    lib_refused(E, "paths fetch: queries [60, 70) past the batch's 65",
                cpd.lib.cpd_query_paths_fetch(ix._h, C.c_uint32(60), C.c_uint32(10), p32))
    lib_refused(E, "paths fetch: null argument",
                cpd.lib.cpd_query_paths_fetch(ix._h, C.c_uint32(0), C.c_uint32(65), None))
    ix.loads_run()  # ... and, like a plain run, ends the paths
    lib_refused(E, none_yet, cpd.lib.cpd_query_paths_fetch(ix._h, C.c_uint32(0), C.c_uint32(1), p32))
    lib_refused(E, "loads fetch: null argument", cpd.lib.cpd_query_loads_fetch(ix._h, None))
    ix.loads_clear()
    lib_refused(E, "loads fetch: no cpd_query_loads on this index since it was made or cleared",
                cpd.lib.cpd_query_loads_fetch(ix._h, p64))
    ix.prepare(s, t)
    lib_refused(E, "costs fetch: no cpd_query_costs on the prepared queries yet",
                cpd.lib.cpd_query_costs_fetch(ix._h, p64, p32, p8))
    lib_refused(E, "timed fetch: no cpd_query_timed on the prepared queries yet",
                cpd.lib.cpd_query_timed_fetch(ix._h, p64, p32, p8))


@pytest.mark.parametrize("mode", MODES)
def test_refusals_prefix_pool(mode):
    """A prefix pool of 64 bytes: both search calls name the bytes to ask for."""
    g, plan, dev, targets, rows, order, off, runs = shared("deg8")
    ix = index(dev, rows, mode)
    s, t = draw(g, targets, 65, seed=41)
    ix.prepare(s, t)
    opts = cpd._search_opts(1.0, 0.0, -1, -1, 0, 0, 0, "auto", 0.0, 0)
    offsets = np.empty(66, np.uint64)
    st, info = cpd.SearchStats(), cpd.SearchPathsInfo()
    rc = cpd.lib.cpd_query_search_paths(ix._h, C.byref(opts), C.c_uint64(64),
                                        cpd._ptr(offsets, cpd.u64p), C.byref(st), C.byref(info))
    need = 4 * info.prefix_nodes
    assert need > 64 and info.prefix_bytes == 64
    lib_refused(cpd.CPD_E_OOM, f"search paths: the prefixes need {need} bytes of prefix pool, 64 "
                               f"were given: call again with prefix_bytes >= {need}", rc)
    st, info = cpd.SearchStats(), cpd.SearchLoadsInfo()
    rc = cpd.lib.cpd_query_search_loads(ix._h, C.byref(opts), C.c_uint64(64), None, C.c_uint32(0),
                                        C.byref(st), C.byref(info))
    assert 4 * info.prefix_nodes == need and info.prefix_bytes == 64
    lib_refused(cpd.CPD_E_OOM, f"search loads: the prefixes need {need} bytes of prefix pool, 64 "
                               f"were given: call again with prefix_bytes >= {need}", rc)
