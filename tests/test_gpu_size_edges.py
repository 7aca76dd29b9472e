"""GPU: the build, the emit and the row converters at column- and row-count
edges, bit-exact against the oracle.

The kernels pad a row to npad = ceil(n / 2048) * 2048 columns, a wave owns a
2048-column tile and a lane a 32-column segment; a batch is cut into
1024-target slabs and 256-target groups, and the fused emit takes 8 rows per
wave.  Every kernel guards its own tail (first_moves_n4's c >= n, moves_runs'
shift mask and prefetch guard, rle_emit8's last lane and its rows past nrows,
repack_moves' partial last word, validate_rows' c >= n, expand_rows'
lookahead).  Here those tails are run on purpose:

- column counts n = 31, 32, 33 (n % 32 = 31, 0, 1: the shift mask at
  0x7FFFFFFF, unused and 1) and 2047 .. 2049, 4095 .. 4097 (npad - n = 1, 0,
  2047), on graphs.band at every adjacency width: 1-bit moves, 2-bit moves on
  the fused narrow path, 8-bit and 16-bit first-move sets;
- 32768 and 32769 columns: exactly the 16 tiles of one move chunk
  (kMoveTiles), and one tile into a second chunk;
- row counts on and around 8, 256 and 1024, and short batches after full ones
  on the same graph, whose device rows past nrows still hold the earlier
  batch's sets;
- the same rows through the streamed index: runs (validate_rows, expand_rows),
  compact rows at the graph's width and at 4 bits (repack_moves, moves_runs),
  walks from and to columns 0 and n - 1, and rows malformed at column n.

tests/test_oracle_cpu.py pins, from the oracle alone, that these cases hold
what they are named for (rows whose last run starts at column n - 1, rows
whose last run spans the whole last segment, run starts on a tile's first
column)."""
import numpy as np
import pytest

import cpd
import oracle
from graphs import BAND, EDGE_DMAX, EDGE_N, chain_hub, edge_graph, edge_queries, edge_targets
from test_gpu_parity import make_graph

pytestmark = pytest.mark.gpu

CASES = [(n, dmax) for n in EDGE_N for dmax in EDGE_DMAX]
NARROW = pytest.mark.parametrize("narrow", [True, False], ids=["narrow", "wide"])
NQ = 3000


class Env:
    pass


_ENV = {}
_ROWS = {}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


def env_of(n, dmax):
    """Graph, plan, targets and oracle rows of one column-count case, made
    once and never written to."""
    if (n, dmax) not in _ENV:
        e = Env()
        e.n, e.dmax, e.bits = n, dmax, BAND[dmax][2]
        g = e.g = edge_graph(n, dmax)
        e.plan = cpd.Plan(g)
        e.order = e.plan.order()
        e.col_node = np.argsort(e.order).astype(np.uint32)  # node at each column
        e.targets = edge_targets(e.order)
        e.off, e.runs = oracle.build_rows(g.row_ptr, g.dst, g.w, e.order, e.targets)
        e.mv = oracle.moves_from_runs(e.off, e.runs, n, e.bits)
        _frozen(e.order, e.col_node, e.targets, e.off, e.runs, e.mv)
        _ENV[(n, dmax)] = e
    return _ENV[(n, dmax)]


@pytest.fixture(scope="module", params=CASES, ids=lambda p: f"n{p[0]}-d{p[1]}")
def env(request):
    return env_of(*request.param)


def check_rows(rows, off, runs, mv, bits, msg):
    o, r = rows.export()
    np.testing.assert_array_equal(o, off, err_msg=f"{msg} offsets")
    np.testing.assert_array_equal(r, runs, err_msg=f"{msg} runs")
    assert rows.move_bits() == bits, msg
    np.testing.assert_array_equal(rows.export_moves(), mv, err_msg=f"{msg} moves")


# ---------------------------------------------------------------------------
# column-count edges

@NARROW
def test_distances_and_first_moves(env, narrow):
    """The four targets at columns 0, 1, n - 2 and n - 1 and 20 others, over
    all n columns."""
    e, g = env, env.g
    dev = make_graph(e.plan, 1024, narrow)
    tcol = e.order[e.targets]
    edge = np.flatnonzero(np.isin(tcol, [0, 1, e.n - 2, e.n - 1]))
    assert len(edge) == 4
    other = np.flatnonzero(~np.isin(np.arange(len(e.targets)), edge))[:20]
    tg = e.targets[np.concatenate([edge, other])]
    dist, fm = dev.debug_rows(tg)
    for i, t in enumerate(tg):
        np.testing.assert_array_equal(dist[:, i], oracle.reverse_dijkstra(g.row_ptr, g.dst, g.w, t),
                                      err_msg=f"n={e.n} dmax={e.dmax} dist t={t}")
        np.testing.assert_array_equal(fm[i], oracle.first_moves(g.row_ptr, g.dst, g.w, t),
                                      err_msg=f"n={e.n} dmax={e.dmax} fm t={t}")


@NARROW
def test_rows_and_moves(env, narrow):
    """Offsets, runs and compact rows of every target, then a range that ends
    at the last row, as compact rows and as runs."""
    e = env
    dev = make_graph(e.plan, 1024, narrow)
    assert dev.move_bits() == e.bits
    rows = dev.build_rows(e.targets)
    msg = f"n={e.n} dmax={e.dmax}"
    check_rows(rows, e.off, e.runs, e.mv, e.bits, msg)
    k = len(e.targets)
    for a in (k - 1, k - min(k, 9), k // 3):
        np.testing.assert_array_equal(rows.export_moves(a, k - a), e.mv[a:], err_msg=msg)
        o, r = rows.export_range(a, k - a)
        np.testing.assert_array_equal(o, e.off[a:] - e.off[a], err_msg=msg)
        np.testing.assert_array_equal(r, e.runs[int(e.off[a]):], err_msg=msg)


@pytest.mark.parametrize("dmax", EDGE_DMAX)
def test_rows_in_hilbert_lane_order(dmax):
    """Seeded random coordinates: the lanes leave the column order, the rows
    stay what they were."""
    e = env_of(2049, dmax)
    dev = make_graph(e.plan, 1024, True)
    rng = np.random.default_rng(5)
    dev.set_coords(rng.integers(-1000, 1000, e.n, dtype=np.int32),
                   rng.integers(-1000, 1000, e.n, dtype=np.int32))
    check_rows(dev.build_rows(e.targets), e.off, e.runs, e.mv, e.bits, f"xy dmax={dmax}")


@pytest.mark.parametrize("n,tiles", [(32768, 16), (32769, 17)])
def test_move_chunk_of_16_tiles(n, tiles):
    """rle_moves<8> takes 16 tiles per block: one block exactly, and one block
    plus a second of a single tile whose first column is the last."""
    g = chain_hub(n, 8, seed=8)
    assert (g.n + 2047) // 2048 == tiles
    plan = cpd.Plan(g)
    dev = cpd.Graph(plan, batch=1024)
    targets = np.random.default_rng(1).permutation(g.n).astype(np.uint32)[:100]
    off, runs = oracle.build_rows(g.row_ptr, g.dst, g.w, plan.order(), targets)
    rows = dev.build_rows(targets)
    check_rows(rows, off, runs, oracle.moves_from_runs(off, runs, g.n, 4), 4, f"hub {n}")


# ---------------------------------------------------------------------------
# row-count edges

ROW_N = 2049
ROW_KS = (1, 2, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 1031, 2048, 2049)


def rows_of(dmax):
    """edge_graph(2049, dmax) with the oracle rows of every node, in a
    shuffled order: the rows of perm[a:b] are a slice of them."""
    if dmax not in _ROWS:
        e = env_of(ROW_N, dmax)
        r = Env()
        r.e = e
        r.perm = np.random.default_rng(dmax).permutation(e.n).astype(np.uint32)
        r.off, r.runs = oracle.build_rows(e.g.row_ptr, e.g.dst, e.g.w, e.order, r.perm)
        r.mv = oracle.moves_from_runs(r.off, r.runs, e.n, e.bits)
        _frozen(r.perm, r.off, r.runs, r.mv)
        _ROWS[dmax] = r
    return _ROWS[dmax]


def check_slice(rows, r, a, b, msg):
    """rows against the oracle's rows of perm[a:b]."""
    check_rows(rows, r.off[a:b + 1] - r.off[a], r.runs[int(r.off[a]):int(r.off[b])], r.mv[a:b],
               r.e.bits, msg)


@NARROW
@pytest.mark.parametrize("dmax", EDGE_DMAX)
def test_row_counts(dmax, narrow):
    """One build per row count, each into a row set of its own: one row, a
    partial and a whole octet, group, slab and batch, and one row past each."""
    r = rows_of(dmax)
    dev = make_graph(r.e.plan, 1024, narrow)
    for k in ROW_KS:
        check_slice(dev.build_rows(r.perm[:k]), r, 0, k, f"dmax={dmax} k={k}")


@pytest.mark.parametrize("hint", [False, True], ids=["plain", "hinted"])
@NARROW
@pytest.mark.parametrize("dmax", EDGE_DMAX)
def test_short_batch_after_full_batch(dmax, narrow, hint):
    """A full batch leaves 1024 rows of sets on the device; the short batches
    that follow fill fewer than an octet of them (or one octet and a row) and
    the emit reads whole octets.  Targets from another part of the
    permutation, so a stale row is a wrong row."""
    r = rows_of(dmax)
    dev = make_graph(r.e.plan, 1024, narrow)
    rows = None
    a = 1024
    for k in (1, 3, 5, 6, 7, 9):
        if hint:
            dev.hint_next(r.perm[a:a + k])
        rows = dev.build_rows(r.perm[:1024], reuse=rows)
        check_slice(rows, r, 0, 1024, f"dmax={dmax} full before k={k}")
        rows = dev.build_rows(r.perm[a:a + k], reuse=rows)
        check_slice(rows, r, a, a + k, f"dmax={dmax} k={k}")
        a += k
    rows = dev.build_rows(r.perm[:1024], reuse=rows)
    check_slice(rows, r, 0, 1024, f"dmax={dmax} full, last")


@pytest.mark.parametrize("k", [257, 1025])
@pytest.mark.parametrize("dmax", EDGE_DMAX)
def test_partial_group_in_hilbert_order(dmax, k):
    """The batch of one row: a 256-target narrow group of one real lane, the
    rest copies of lane 0, the lanes in Hilbert order."""
    r = rows_of(dmax)
    dev = make_graph(r.e.plan, 1024, True)
    rng = np.random.default_rng(5)
    dev.set_coords(rng.integers(-1000, 1000, ROW_N, dtype=np.int32),
                   rng.integers(-1000, 1000, ROW_N, dtype=np.int32))
    check_slice(dev.build_rows(r.perm[:k]), r, 0, k, f"xy dmax={dmax} k={k}")


# ---------------------------------------------------------------------------
# round trips through the index

INDEX_CASES = [(n, dmax) for n in (33, 2047, 2048, 2049) for dmax in EDGE_DMAX]
_WALK = {}
_DEV = {}


def walk_of(e):
    """Queries over a case's rows and the oracle's walks; sources and targets
    at columns 0 and n - 1 forced in, in every pairing."""
    if (e.n, e.dmax) not in _WALK:
        s, t = edge_queries(e.order, e.targets, NQ)
        g = e.g
        ref = oracle.table_search(g.row_ptr, g.dst, g.w, e.order, e.targets, e.off, e.runs, s, t)
        _WALK[(e.n, e.dmax)] = (s, t, ref)
    return _WALK[(e.n, e.dmax)]


def dev_of(e):
    if (e.n, e.dmax) not in _DEV:
        _DEV[(e.n, e.dmax)] = cpd.Graph(e.plan, batch=1024)
    return _DEV[(e.n, e.dmax)]


def check_walks(ix, e, msg):
    s, t, ref = walk_of(e)
    cost, hops, fin, _ = ix.query(s, t)
    np.testing.assert_array_equal(cost, ref[0], err_msg=f"{msg} cost")
    np.testing.assert_array_equal(hops, ref[1], err_msg=f"{msg} hops")
    np.testing.assert_array_equal(fin, ref[2], err_msg=f"{msg} finished")


@pytest.mark.parametrize("mode", ["dense", "rle"])
@pytest.mark.parametrize("n,dmax", INDEX_CASES)
def test_index_from_runs(n, dmax, mode):
    """The oracle's runs in two chunks, the first ending in a row whose last
    run starts at column n - 1."""
    e = env_of(n, dmax)
    k = len(e.targets)
    last = (e.runs[e.off[1:].astype(np.int64) - 1] >> 4).astype(np.int64)
    cut = int(np.flatnonzero(last[:k - 1] == n - 1)[-1]) + 1
    ix = cpd.Index.streamed(dev_of(e), e.targets, int(e.off[-1]), mode=mode)
    for a, b in ((0, cut), (cut, k)):
        ix.append(e.off[a:b + 1] - e.off[a], e.runs[int(e.off[a]):int(e.off[b])])
    info = ix.info()
    assert ix.mode == mode and info["added"] == k
    if mode == "rle":
        assert info["runs_resident"] == int(e.off[-1])
    check_walks(ix, e, f"n={n} dmax={dmax} runs {mode}")


def spoil_spare_fields(mv, n, bits):
    """mv with the fields past column n - 1 of every row's last word set to
    another move than column n - 1's (one that fits 1 bit)."""
    out = mv.copy()
    per = 32 // bits
    used = n - (out.shape[1] - 1) * per          # columns in the last word
    if used == per:
        return out
    last = (out[:, -1] >> np.uint32(bits * (used - 1))) & np.uint32((1 << bits) - 1)
    keep = np.uint32((1 << (bits * used)) - 1)
    fill = np.zeros(len(out), np.uint32)
    for k in range(used, per):
        fill |= (last ^ np.uint32(1)) << np.uint32(bits * k)
    out[:, -1] = (out[:, -1] & keep) | fill
    return out


@pytest.mark.parametrize("spare", ["exported", "spoiled"])
@pytest.mark.parametrize("mode", ["dense", "rle"])
@pytest.mark.parametrize("n,dmax", INDEX_CASES)
def test_index_from_compact_rows(n, dmax, mode, spare):
    """Half the rows at the graph's own width, half at 4 bits: the last word
    of a row holds n * bits % 32 bits of it.  The fields past column n - 1
    repeat the last move in exported rows; columns >= n are ignored, so with
    other moves there the index counts the same runs and walks the same."""
    e = env_of(n, dmax)
    k = len(e.targets)
    half = k // 2
    mv = e.mv[:half]
    mv4 = oracle.moves_from_runs(e.off[half:] - e.off[half], e.runs[int(e.off[half]):], n, 4)
    if spare == "spoiled":
        mv, mv4 = spoil_spare_fields(mv, n, e.bits), spoil_spare_fields(mv4, n, 4)
    ix = cpd.Index.streamed(dev_of(e), e.targets, int(e.off[-1]), mode=mode)
    ix.append_moves(mv, e.bits)
    ix.append_moves(mv4, 4)
    info = ix.info()
    assert ix.mode == mode and info["added"] == k
    if mode == "rle":
        assert info["runs_resident"] == int(e.off[-1])
    check_walks(ix, e, f"n={n} dmax={dmax} moves {mode} {spare}")


@pytest.mark.parametrize("mode", ["dense", "rle"])
@pytest.mark.parametrize("n,dmax", INDEX_CASES)
def test_rows_malformed_at_the_last_column(n, dmax, mode):
    """A last run at column n - 1 is a row; at column n or n + 1 it is not.
    Into tables narrower than 4 bits a move too wide for them at column n - 1
    is refused, never truncated."""
    e = env_of(n, dmax)
    dev = dev_of(e)
    row = e.runs[:int(e.off[1])]
    row = row[(row >> 4) < n - 1]
    assert len(row) >= 1
    one = np.array([0, len(row) + 1], np.uint64)

    def with_last(col, move):
        return np.concatenate([row, [np.uint32((col << 4) | move)]]).astype(np.uint32)

    move = int(row[-1] & 0xF) ^ 1  # differs from the run before it, fits 1 bit
    ix = cpd.Index.streamed(dev, e.targets[:1], len(row) + 1, mode=mode)
    ix.append(one, with_last(n - 1, move))
    assert ix.info()["added"] == 1
    for col in (n, n + 1):
        ix = cpd.Index.streamed(dev, e.targets[:1], len(row) + 1, mode=mode)
        with pytest.raises(cpd.CpdError) as ei:
            ix.append(one, with_last(col, move))
        assert ei.value.code == cpd.CPD_E_ARG, col
    if e.bits < 4:
        if mode == "dense":  # an RLE index keeps the run words as they are
            ix = cpd.Index.streamed(dev, e.targets[:1], len(row) + 1, mode=mode)
            with pytest.raises(cpd.CpdError) as ei:
                ix.append(one, with_last(n - 1, 1 << e.bits))
            assert ei.value.code == cpd.CPD_E_ARG and "moves <" in str(ei.value)
        mv4 = oracle.moves_from_runs(e.off[:2], e.runs, n, 4)
        c = n - 1
        mv4[0, c // 8] = (mv4[0, c // 8] & ~np.uint32(0xF << (4 * (c % 8)))) | \
            np.uint32((1 << e.bits) << (4 * (c % 8)))
        ix = cpd.Index.streamed(dev, e.targets[:1], int(e.off[1]) + 2, mode=mode)
        with pytest.raises(cpd.CpdError) as ei:
            ix.append_moves(mv4, 4)
        assert ei.value.code == cpd.CPD_E_ARG
