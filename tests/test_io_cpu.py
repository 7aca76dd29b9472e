"""The file readers and writers of csrc/cpd_io.cpp at the drop-in boundary,
through a stand-alone harness (tests/io_check.cpp, and tests/query_file_check.cpp
for the query file), against an independent Python statement of each format
written from the layout comments of csrc/cpd_io.hpp (here and in
tests/bucket_files.py): edge values in every numeric field, malformed
structure, writers byte for byte, windows of rows and runs, corrupted and
truncated binary files, and headers that claim more than the file holds.

Every case runs against two builds of the harness: a plain one and one with
the host sanitizers (address, undefined), where any report fails the case
(non-zero exit, text on stderr).  Both are stand-alone programs; nothing here
needs or touches a GPU."""
import os
import re
import resource
import shutil
import struct
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import bucket_files as BF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-oracle-search_amd", "csrc")
SAN_FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
E_ARG, E_IO = -1, -6  # include/cpd_api.h


def _compile(outdir, flags, skip_on_failure):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    h = SimpleNamespace()
    for name, src in (("io", "io_check.cpp"), ("qf", "query_file_check.cpp")):
        out = str(outdir / name)
        p = subprocess.run([gxx, *flags, "-std=c++17", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                            os.path.join(CSRC, "cpd_io.cpp"), os.path.join(ROOT, "tests", src),
                            "-o", out, "-lpthread"], capture_output=True, text=True, timeout=480)
        if p.returncode != 0 and skip_on_failure:
            pytest.skip("no sanitizer build: " + p.stderr.strip()[-400:])
        assert p.returncode == 0, p.stderr
        setattr(h, name, out)
    return h


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("io_plain"), ["-O2"], False)


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("io_san"), SAN_FLAGS, True)


@pytest.fixture(params=["plain", "sanitized"])
def h(request):
    return request.getfixturevalue(request.param)


def run(exe, *args, limit_as=None):
    """The harness's stdout; a sanitizer report (or any crash) fails here."""
    def limit():
        resource.setrlimit(resource.RLIMIT_AS, (limit_as, limit_as))
    p = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=120,
                       preexec_fn=limit if limit_as else None)
    assert p.returncode == 0 and p.stderr == "", (args, p.returncode, p.stderr[-2000:])
    return p.stdout


def refused(out, *names):
    """ERR -6 (CPD_E_IO) with one of the paths in the message."""
    return out.startswith(f"ERR {E_IO} ") and out.count("\n") == 1 and any(n in out for n in names)


def put(path, data):
    with open(path, "wb") as f:
        f.write(data if isinstance(data, bytes) else data.encode())
    return str(path)


# ---------------------------------------------------------------------------
# The text formats, stated independently (cpd_io.hpp's head comment): Python
# integers do not wrap, so a field's range is checked on its true value.

class Refused(Exception):
    pass


U32 = 2**32 - 1
MAX_NODES = 2**28 - 1
EDGE_VALUES = ["4294967295", "4294967296", "9223372036854775807", "9223372036854775808",
               "18446744073709551621", "1234567890" * 4, "-1", "+7"]


def _tokens(line):
    return [t for t in re.split(r"[ \t\r]+", line) if t]


def _int(tok, lo, hi):
    if not re.fullmatch(r"[+-]?[0-9]+", tok):
        raise Refused(tok)
    v = int(tok)
    if not lo <= v <= hi:
        raise Refused(tok)
    return v


def _ints(toks, ranges):
    if len(toks) < len(ranges):
        raise Refused(toks)
    return [_int(t, lo, hi) for t, (lo, hi) in zip(toks, ranges)]


def ref_xy(text):
    """n, row_ptr, dst, w, x, y of an .xy text: out-edge k of a node is its k-th
    "e" line in file order (a stable grouping by tail)."""
    header, verts, edges = None, [], []
    for line in text.split("\n"):
        t = _tokens(line)
        if not t:
            continue
        if t[0] == "nodes":
            if len(t) < 4 or t[2] != "edges":
                raise Refused(line)
            header = (_int(t[1], 0, MAX_NODES), _int(t[3], 0, U32))
        elif t[0] == "v":
            verts.append(_ints(t[1:], [(0, U32), (-2**31, 2**31 - 1), (-2**31, 2**31 - 1)]))
        elif t[0] == "e":
            edges.append(_ints(t[1:], [(0, U32)] * 3))
    if header is None or header[1] != len(edges):
        raise Refused("header")
    n = header[0]
    x, y = [0] * n, [0] * n
    for i, vx, vy in verts:
        if i >= n:
            raise Refused("vertex id")
        x[i], y[i] = vx, vy
    if any(a >= n or b >= n for a, b, _ in edges):
        raise Refused("endpoint")
    grouped = sorted(edges, key=lambda e: e[0])  # stable
    row_ptr = [0] * (n + 1)
    for a, _, _ in edges:
        row_ptr[a + 1] += 1
    row_ptr = np.cumsum(row_ptr).tolist()
    return n, row_ptr, [e[1] for e in grouped], [e[2] for e in grouped], x, y


def xy_output(g):
    n, row_ptr, dst, w, x, y = g
    rows = [("row_ptr", row_ptr), ("dst", dst), ("w", w), ("x", x), ("y", y)]
    return f"n {n} m {len(dst)}\n" + "".join(" ".join([k] + [str(v) for v in a]) + "\n" for k, a in rows)


def ref_diff(text, g):
    """Weights after a .diff: "e from to cost" or "from to cost" lines, each
    replacing the weight of the FIRST from->to edge; other lines are comments."""
    n, row_ptr, dst, w, _, _ = g
    w = list(w)
    for line in text.split("\n"):
        t = _tokens(line)
        if not t:
            continue
        if t[0] == "e":
            t = t[1:]
        elif not re.match(r"[+-]?[0-9]", t[0]):
            continue
        a, b, c = _ints(t, [(0, U32)] * 3)
        if a >= n or b >= n:
            raise Refused(line)
        hits = [e for e in range(row_ptr[a], row_ptr[a + 1]) if dst[e] == b]
        if not hits:
            raise Refused(line)
        w[hits[0]] = c
    return w


def ref_scen(text):
    return [tuple(_ints(_tokens(line[1:]), [(0, U32)] * 2)) for line in text.split("\n") if line[:1] == "q"]


def check_xy(h, tmp_path, text, name="g.xy"):
    path = put(tmp_path / name, text)
    out = run(h.io, "xy", path)
    try:
        want = xy_output(ref_xy(text))
    except Refused:
        assert refused(out, path), (text[:200], out[:200])
        return None
    assert out == want, text[:200]
    return out


# 8 declared nodes, ids 0..6 used, 7 edges: "+7" is a valid value of every field
BASE_XY = ["c a graph", "c", "c", "nodes 8 edges 7", "v 0 10 -20", "v 6 -2147483648 2147483647",
           "e 0 1 5", "e 1 2 4294967295", "e 6 6 1", "e 0 2 6", "e 2 0 0", "e 1 0 9", "e 0 6 3"]
XY_FIELDS = {"nodes": (3, 1), "edges": (3, 3), "v_id": (4, 1), "v_x": (4, 2), "v_y": (4, 3),
             "e_tail": (6, 1), "e_head": (6, 2), "e_cost": (6, 3)}


def _with(lines, line, tok, value):
    lines = list(lines)
    t = lines[line].split(" ")
    t[tok] = value
    lines[line] = " ".join(t)
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("field", sorted(XY_FIELDS))
def test_xy_field_edges(h, tmp_path, field):
    """Each numeric field of an .xy at the edges of u32, int64 and beyond: read
    as its true value where the field admits it, refused (CPD_E_IO naming the
    file) otherwise, never wrapped."""
    line, tok = XY_FIELDS[field]
    accepted = []
    for i, value in enumerate(EDGE_VALUES):
        if check_xy(h, tmp_path, _with(BASE_XY, line, tok, value), f"g{i}.xy") is not None:
            accepted.append(value)
    # the reference's own verdicts, pinned so that it cannot drift to "refuse all"
    want = {"e_cost": ["4294967295", "+7"], "v_x": ["-1", "+7"], "v_y": ["-1", "+7"]}.get(field, ["+7"])
    assert accepted == want


def test_xy_coordinate_range(h, tmp_path):
    for i, (value, ok) in enumerate([("2147483647", True), ("-2147483648", True), ("2147483648", False),
                                     ("-2147483649", False), ("-18446744073709551621", False)]):
        for field in ("v_x", "v_y"):
            got = check_xy(h, tmp_path, _with(BASE_XY, *XY_FIELDS[field], value), f"c{i}{field}.xy")
            assert (got is not None) == ok, (field, value)


def test_xy_node_count_limit(h, tmp_path):
    """More nodes than the library admits (2^28 - 1, the 28-bit run start
    column) are refused at the header; the arrays are not sized by it first."""
    assert check_xy(h, tmp_path, f"nodes {MAX_NODES + 1} edges 0\n") is None
    assert check_xy(h, tmp_path, "nodes 4294967298 edges 1\ne 0 1 1\n") is None


XY_STRUCTURE = {
    "missing_header": ("v 0 1 1\ne 0 0 1\n", False),
    # deliberate: the lines are collected in any order, the header is not
    # required to come first
    "header_after_edges": ("e 0 1 3\ne 1 0 4\nv 1 5 6\nnodes 2 edges 2\n", True),
    "count_too_big": ("nodes 2 edges 3\ne 0 1 3\ne 1 0 4\n", False),
    "count_too_small": ("nodes 2 edges 1\ne 0 1 3\ne 1 0 4\n", False),
    "edges_minus_one": ("nodes 2 edges -1\n", False),
    "huge_edge_count": ("nodes 2 edges 4294967295\ne 0 1 3\n", False),
    "tail_eq_n": ("nodes 2 edges 1\ne 2 1 3\n", False),
    "head_eq_n": ("nodes 2 edges 1\ne 1 2 3\n", False),
    "vertex_eq_n": ("nodes 2 edges 0\nv 2 0 0\n", False),
    # deliberate: an empty graph reads (the library refuses it later, check_csr)
    "no_nodes": ("nodes 0 edges 0\n", True),
    "no_nodes_one_edge": ("nodes 0 edges 1\ne 0 0 1\n", False),
    "no_edges": ("nodes 3 edges 0\nv 1 4 5\n", True),
    "crlf": ("c x\r\nnodes 2 edges 2\r\nv 0 1 2\r\ne 0 1 3\r\ne 1 0 4\r\n", True),
    "tabs": ("nodes\t2  edges \t2\nv\t1\t-5\t6\n \te\t0\t1\t3\ne 1\t0 4\t\n", True),
    "blank_lines": ("\n\nnodes 2 edges 1\n\n   \n\t\ne 0 1 3\n\n", True),
    "no_trailing_newline": ("nodes 2 edges 1\ne 0 1 3", True),
    "comments": ("c nodes 9 edges 9\n# e 0 1 2\nnodes 2 edges 1\nc e 1 1 1\np sp 2 1\ne 0 1 3\n", True),
    "short_e_line": ("nodes 2 edges 1\ne 0 1\n", False),
    "word_for_number": ("nodes 2 edges 1\ne 0 x 3\n", False),
    "header_without_edges": ("nodes 2\n", False),
    "empty_file": ("", False),
}


@pytest.mark.parametrize("case", sorted(XY_STRUCTURE))
def test_xy_structure(h, tmp_path, case):
    text, ok = XY_STRUCTURE[case]
    assert (check_xy(h, tmp_path, text) is not None) == ok


def test_xy_out_edge_order(h, tmp_path):
    """Out-edge k of a node is its k-th "e" line: tails interleaved in the
    file, parallel edges and self loops present."""
    rng = np.random.default_rng(11)
    n, m = 9, 60
    a, b = rng.integers(0, n, m), rng.integers(0, 3, m)  # few heads: many parallel edges
    lines = [f"nodes {n} edges {m}"] + [f"e {a[i]} {b[i]} {i + 1}" for i in range(m)]
    lines[20:20] = [f"v {i} {i} {-i}" for i in range(n)]  # v lines among the e lines
    out = check_xy(h, tmp_path, "\n".join(lines) + "\n")
    want_w = [i + 1 for v in range(n) for i in range(m) if a[i] == v]
    assert out.split("\n")[3] == " ".join(["w"] + [str(x) for x in want_w])


DIFF_GRAPH = "nodes 4 edges 6\ne 0 1 5\ne 0 1 6\ne 1 2 7\ne 3 3 8\ne 2 0 9\ne 0 2 10\n"
DIFF_CASES = {
    "both_forms": ("e 1 2 70\n2 0 90\n", True),
    "comments_and_header": ("c cpd-mi355x congestion diff: e from to new_cost\n# 1 2 3\n\nx 1 2 3\ne 3 3 1\n", True),
    "later_overrides": ("e 1 2 70\ne 0 2 1\n1 2 71\n", True),
    "first_parallel_edge": ("e 0 1 50\n", True),  # [5, 6] -> [50, 6]: the second 0->1 edge cannot be named
    "crlf_tabs": ("e\t1 2\t70\r\n 2  0 90\r\n", True),
    "max_cost": ("e 1 2 4294967295\n", True),
    "no_trailing_newline": ("e 1 2 70", True),
    "empty": ("", True),
    "missing_edge": ("e 1 3 4\n", False),
    "node_eq_n": ("e 4 0 4\n", False),
    "short_line": ("e 1 2\n", False),
    "bare_short_line": ("1 2\n", False),
    "bare_negative_tail": ("-1 2 5\n", False),
}


def check_diff(h, tmp_path, graph_text, text, name="d.diff"):
    xy, path = put(tmp_path / "dg.xy", graph_text), put(tmp_path / name, text)
    out = run(h.io, "diff", xy, path)
    try:
        want = " ".join(["w"] + [str(v) for v in ref_diff(text, ref_xy(graph_text))]) + "\n"
    except Refused:
        assert refused(out, path), (text, out)
        return None
    assert out == want, text
    return out


@pytest.mark.parametrize("case", sorted(DIFF_CASES))
def test_diff_lines(h, tmp_path, case):
    text, ok = DIFF_CASES[case]
    assert (check_diff(h, tmp_path, DIFF_GRAPH, text) is not None) == ok


def test_diff_no_file(h, tmp_path):
    """"" and "-" as the path: the free-flow weights."""
    xy = put(tmp_path / "g.xy", DIFF_GRAPH)
    for path in ("", "-"):
        assert run(h.io, "diff", xy, path) == "w 5 6 10 7 9 8\n"


@pytest.mark.parametrize("form", ["e", "bare"])
@pytest.mark.parametrize("tok", [0, 1, 2])
def test_diff_field_edges(h, tmp_path, form, tok):
    graph = "nodes 8 edges 2\ne 7 7 1\ne 0 1 2\n"
    accepted = []
    for i, value in enumerate(EDGE_VALUES):
        t = ["7", "7", "2"]
        t[tok] = value
        text = ("e " if form == "e" else "") + " ".join(t) + "\n"
        if check_diff(h, tmp_path, graph, text, f"d{i}.diff") is not None:
            accepted.append(value)
    assert accepted == (["4294967295", "+7"] if tok == 2 else ["+7"])


@pytest.mark.parametrize("tok", [0, 1])
def test_scen_field_edges(h, tmp_path, tok):
    accepted = []
    for i, value in enumerate(EDGE_VALUES):
        t = ["3", "4"]
        t[tok] = value
        text = f"p aux sp p2p 2\nq 1 2\nq {' '.join(t)}\n"
        path = put(tmp_path / f"s{i}.scen", text)
        out = run(h.io, "scen", path)
        try:
            q = ref_scen(text)
            assert out == f"{len(q)}\n" + "".join(f"{a} {b}\n" for a, b in q)
            accepted.append(value)
        except Refused:
            assert refused(out, path), (text, out)
    assert accepted == ["4294967295", "+7"]


def test_scen_structure(h, tmp_path):
    for i, (text, ok) in enumerate([("", True), ("p aux sp p2p 0\n", True), ("c x\nq 1 2\r\nq\t3\t4\nq 5 6", True),
                                    ("q 1\n", False), ("q 1 x\n", False), ("q\n", False)]):
        path = put(tmp_path / f"t{i}.scen", text)
        out = run(h.io, "scen", path)
        if ok:
            q = ref_scen(text)
            assert out == f"{len(q)}\n" + "".join(f"{a} {b}\n" for a, b in q)
        else:
            assert refused(out, path), (text, out)


def test_query_count_edges(h, tmp_path):
    """The query file's header count through tests/query_file_check.cpp (which
    prints "ERR <message>"): a count that is not the number of lines is an
    error naming the file, whatever its magnitude; "+7" counts 7 lines."""
    body = "".join(f"{i} {i + 1}\n" for i in range(7))
    for i, value in enumerate(EDGE_VALUES):
        path = put(tmp_path / f"q{i}", f"{value}\n{body}")
        for threads in (1, 4):
            out = run(h.qf, path, threads)
            if value == "+7":
                assert out == "7\n" + body
            else:
                assert out.startswith("ERR ") and path in out and out.count("\n") == 1, (value, out)


def test_query_file_small_edges(h, tmp_path):
    """An empty file is no queries (and no call on a null buffer); a 25-digit
    source is an error, not a clamped value that passes."""
    assert run(h.qf, put(tmp_path / "empty", ""), 4) == "0\n"
    assert run(h.qf, put(tmp_path / "zero", "0\n"), 4) == "0\n"
    path = put(tmp_path / "long", "1\n1234567890123456789012345 2\n")
    assert run(h.qf, path, 1).startswith("ERR " + path + ": bad query line 2")


# ---------------------------------------------------------------------------
# Round trips through the text writers.

def _xy_input(n, row_ptr, dst, w, x, y):
    return (struct.pack("<2I", n, len(dst)) + np.asarray(row_ptr, "<u4").tobytes() + np.asarray(dst, "<u4").tobytes()
            + np.asarray(w, "<u4").tobytes() + np.asarray(x, "<i4").tobytes() + np.asarray(y, "<i4").tobytes())


def _random_graph(rng, n, m, parallel):
    while True:
        a, b = np.sort(rng.integers(0, n, m)), rng.integers(0, n, m)
        if parallel or len(set(zip(a.tolist(), b.tolist()))) == m:
            break
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=n))])
    w = rng.integers(0, 2**32, m, dtype=np.uint64)
    w[:2] = [0, U32]
    x = rng.integers(-2**31, 2**31, n)
    x[:2] = [-2**31, 2**31 - 1]
    return n, row_ptr.tolist(), b.tolist(), w.tolist(), x.tolist(), x[::-1].tolist()


def test_xy_round_trip(h, tmp_path):
    g = _random_graph(np.random.default_rng(5), 12, 40, True)
    path = str(tmp_path / "w.xy")
    assert run(h.io, "write-xy", put(tmp_path / "in", _xy_input(*g)), path) == "ok\n"
    text = open(path).read()
    assert text.split("\n")[3] == "nodes 12 edges 40"  # line 4, after 3 comment lines
    assert run(h.io, "xy", path) == xy_output(g) == xy_output(ref_xy(text))
    # without coordinates: zeros
    assert run(h.io, "write-xy", str(tmp_path / "in"), path, "nocoords") == "ok\n"
    assert run(h.io, "xy", path) == xy_output(g[:4] + ([0] * 12, [0] * 12))
    # no nodes at all
    assert run(h.io, "write-xy", put(tmp_path / "in0", _xy_input(0, [0], [], [], [], [])), path) == "ok\n"
    assert run(h.io, "xy", path) == xy_output((0, [0], [], [], [], []))


def test_scen_round_trip(h, tmp_path):
    rng = np.random.default_rng(6)
    for count in (0, 1, 50):
        q = rng.integers(0, 2**32, (count, 2), dtype=np.uint64)
        if count:
            q[0] = [U32, 0]
        path = str(tmp_path / f"w{count}.scen")
        data = struct.pack("<I", count) + q.astype("<u4").tobytes()
        assert run(h.io, "write-scen", put(tmp_path / "in", data), path) == "ok\n"
        assert run(h.io, "scen", path) == f"{count}\n" + "".join(f"{a} {b}\n" for a, b in q.tolist())
        assert ref_scen(open(path).read()) == [tuple(p) for p in q.tolist()]


def _diff_round_trip(h, tmp_path, g, new_w):
    xy = str(tmp_path / "rt.xy")
    assert run(h.io, "write-xy", put(tmp_path / "in", _xy_input(*g)), xy) == "ok\n"
    data = struct.pack("<I", len(new_w)) + np.asarray(new_w, "<u4").tobytes()
    path = str(tmp_path / "rt.diff")
    assert run(h.io, "write-diff", xy, put(tmp_path / "inw", data), path) == "ok\n"
    out = run(h.io, "diff", xy, path)
    assert out.startswith("w")
    return [int(v) for v in out.split()[1:]], open(path).read()


def test_diff_round_trip(h, tmp_path):
    """write_diff -> read_diff is the identity on a graph without parallel edges."""
    rng = np.random.default_rng(7)
    g = _random_graph(rng, 12, 40, False)
    new_w = list(g[3])
    for e in rng.choice(40, 15, replace=False):
        new_w[e] = int(rng.integers(0, 2**32))
    new_w[3] = U32
    got, text = _diff_round_trip(h, tmp_path, g, new_w)
    assert got == new_w
    assert len(text.strip().split("\n")) == 1 + sum(a != b for a, b in zip(new_w, g[3]))
    assert _diff_round_trip(h, tmp_path, g, g[3])[0] == g[3]  # nothing changed: a header only


def test_diff_round_trip_parallel_edges(h, tmp_path):
    """A .diff line names an edge by (from, to) and read_diff applies it to the
    FIRST such edge, so the round trip is not the identity when the second of
    two parallel edges changed: [5, 6] -> [5, 9] is written "e 0 1 9" and read
    back as [9, 6].  A limitation of the format (cpd_io.hpp), pinned here; what
    write_diff emits is not to change."""
    g = (2, [0, 2, 2], [1, 1], [5, 6], [0, 0], [0, 0])
    got, text = _diff_round_trip(h, tmp_path, g, [5, 9])
    assert text.split("\n")[1:] == ["e 0 1 9", ""]
    assert got == [9, 6]
    # both changed: two lines, both land on the first edge, the later one wins
    got, text = _diff_round_trip(h, tmp_path, g, [7, 9])
    assert text.split("\n")[1:] == ["e 0 1 7", "e 0 1 9", ""]
    assert got == [9, 6]


# ---------------------------------------------------------------------------
# The binary files.

FP = 0xFEDCBA9876543210
ROW_COUNTS = {S: sorted({0, 1, S - 1, S, S + 1}) for S in (1, 64)}


def _row_counts(S, K):
    return sorted(set(ROW_COUNTS[S]) | {K * S - 1, K * S, K * S + 1})


def make_bucket(nrows, seed=1):
    rng = np.random.default_rng(seed + nrows)
    b = SimpleNamespace(n=100000, bid=3, method=1, key=7, maxworker=2, fingerprint=FP)
    b.targets = rng.integers(0, b.n, nrows, dtype=np.uint32)
    b.offsets = np.concatenate([[0], np.cumsum(rng.integers(1, 5, nrows))]).astype(np.uint64)
    b.runs = rng.integers(0, 2**32, int(b.offsets[-1]), dtype=np.uint32)
    return b


def bucket_input(b):
    return (struct.pack("<6IQQ", b.n, b.bid, b.method, b.key, b.maxworker, len(b.targets), b.fingerprint, len(b.runs))
            + b.targets.tobytes() + b.offsets.tobytes() + b.runs.tobytes())


def bucket_bytes(b):
    return BF.pack_bucket(b.n, b.bid, b.method, b.key, b.maxworker, b.fingerprint, b.targets, b.offsets, b.runs)


def bucket_line(b, runs):
    return (f"n {b.n} nrows {len(b.targets)} bid {b.bid} method {b.method} key {b.key} maxworker {b.maxworker} "
            f"total {len(b.runs)} fingerprint {b.fingerprint} runs {runs}\n")


@pytest.mark.parametrize("nrows", sorted(set(_row_counts(1, 3) + _row_counts(64, 3))))
def test_bucket_writers(h, tmp_path, nrows):
    """write_bucket against the packed layout, BucketFile in pieces (4 threads,
    shuffled) against the same bytes, and both readers on the result."""
    b = make_bucket(nrows)
    src = put(tmp_path / "in", bucket_input(b))
    want = bucket_bytes(b)
    for cmd in ("write-bucket", "bucket-pieces"):
        path = str(tmp_path / f"{cmd}.cpd")
        assert run(h.io, cmd, src, path) == "ok\n"
        assert open(path, "rb").read() == want, cmd
    assert sorted(os.listdir(tmp_path)) == ["bucket-pieces.cpd", "in", "write-bucket.cpd"]  # no .tmp
    out = str(tmp_path / "out")
    assert run(h.io, "bucket", path, out) == bucket_line(b, len(b.runs))
    assert open(out, "rb").read() == want[48:]
    assert run(h.io, "bucket-head", path, out) == bucket_line(b, 0)
    assert open(out, "rb").read() == want[48:48 + 12 * nrows + 8]
    assert run(h.io, "bucket-format", path) == "1\n"
    t, off, runs = BF.read_bucket(path)
    assert (t == b.targets).all() and (off == b.offsets).all() and (runs == b.runs).all()


def test_bucket_file_abandoned(h, tmp_path):
    """A BucketFile destroyed without close() leaves nothing behind."""
    src = put(tmp_path / "in", bucket_input(make_bucket(5)))
    assert run(h.io, "bucket-pieces", src, tmp_path / "b.cpd", "noclose") == "ok\n"
    assert os.listdir(tmp_path) == ["in"]


def test_bucket_runs_windows(h, tmp_path):
    """read_bucket_runs for every (first, count) window of a small bucket."""
    b = make_bucket(6)
    path, out = put(tmp_path / "b.cpd", bucket_bytes(b)), str(tmp_path / "out")
    total = len(b.runs)
    assert run(h.io, "bucket-runs-windows", path, out) == f"{total}\n"
    want = [b.runs[f:f + c] for f in range(total + 1) for c in range(total - f + 1)]
    assert open(out, "rb").read() == np.concatenate(want).tobytes()
    assert run(h.io, "bucket-runs", path, 2, 3, out) == "3\n"
    assert open(out, "rb").read() == b.runs[2:5].tobytes()
    assert run(h.io, "bucket-runs", path, total - 1, 2, out).startswith(f"ERR {E_ARG} ")


def make_moves(nrows, n=48, bits=2, seed=2):
    rng = np.random.default_rng(seed + nrows)
    b = SimpleNamespace(n=n, bid=4, method=0, key=5, maxworker=3, bits=bits, fingerprint=FP)
    b.words = (n * bits + 31) // 32
    b.targets = rng.integers(0, n, nrows, dtype=np.uint32)
    b.counts = rng.integers(1, 9, nrows, dtype=np.uint32)
    b.rows = rng.integers(0, 2**32, (nrows, b.words), dtype=np.uint32)
    return b


def moves_input(b):
    return (struct.pack("<8IQQ", b.n, b.bid, b.method, b.key, b.maxworker, b.words, b.bits, len(b.targets),
                        b.fingerprint, int(b.counts.sum()))
            + b.targets.tobytes() + b.counts.tobytes() + b.rows.tobytes())


def moves_files(b, stripes, stripe_rows):
    return BF.pack_move_bucket(b.n, b.bid, b.method, b.key, b.maxworker, b.bits, b.fingerprint, b.targets,
                               b.counts, b.rows, stripes, stripe_rows)


def put_moves(tmp_path, b, stripes, stripe_rows, name="m.cpd"):
    for suffix, data in moves_files(b, stripes, stripe_rows).items():
        put(str(tmp_path / name) + suffix, data)
    return str(tmp_path / name)


def moves_head_output(b, stripes, stripe_rows):
    nrows = len(b.targets)
    return (f"n {b.n} nrows {nrows} bid {b.bid} method {b.method} key {b.key} maxworker {b.maxworker} "
            f"words {b.words} bits {b.bits} total_runs {int(b.counts.sum())} fingerprint {b.fingerprint} "
            f"stripes {stripes} stripe_rows {stripe_rows if stripes > 1 else 0} "
            f"rows_offset {-(-(56 + 8 * nrows) // 4096) * 4096} head_bytes {64 + 8 * nrows}\n"
            + " ".join(["targets"] + [str(v) for v in b.targets]) + "\n"
            + " ".join(["counts"] + [str(v) for v in b.counts]) + "\n")


def check_move_writer(h, tmp_path, b, stripes, stripe_rows):
    src = put(tmp_path / "in", moves_input(b))
    path = str(tmp_path / "m.cpd")
    assert run(h.io, "move-pieces", src, path, stripes, stripe_rows) == "ok\n"
    want = moves_files(b, stripes, stripe_rows)
    assert sorted(os.listdir(tmp_path)) == sorted(["in"] + ["m.cpd" + s for s in want])  # no .tmp, no other part
    for suffix, data in want.items():
        assert open(path + suffix, "rb").read() == data, suffix
    assert run(h.io, "move-head", path) == moves_head_output(b, stripes, stripe_rows)
    assert run(h.io, "bucket-format", path) == "2\n"
    if stripes > 16:  # (the Python reader adds nothing to the byte comparison; 4096 files once is enough)
        return
    t, c, rows, bits = BF.read_move_bucket(path)
    assert (t == b.targets).all() and (c == b.counts).all() and (rows == b.rows).all() and bits == b.bits


@pytest.mark.parametrize("stripes,stripe_rows,nrows",
                         [(K, S, r) for K in (1, 2, 16, 4096) for S in (1, 64) for r in _row_counts(S, K)])
def test_move_bucket_writer(h, tmp_path, stripes, stripe_rows, nrows):
    """MoveBucketFile in pieces (4 threads, shuffled; row pieces that straddle
    stripe units) against the packed layouts: DOSCPD02 at stripes 1, DOSCPD03
    with its part files above, at row counts around the stripe unit S and a
    full round K S of the deal."""
    check_move_writer(h, tmp_path, make_moves(nrows, n=16), stripes, stripe_rows)


@pytest.mark.parametrize("bits", [1, 2, 4])
@pytest.mark.parametrize("stripes", [1, 2])
def test_move_bucket_row_width(h, tmp_path, bits, stripes):
    """The row width words = ceil(n bits / 32) at its rounding edge: n bits
    just below, at (where bits divides it) and just above 32."""
    for n in sorted({31 // bits, 32 // bits, -(-33 // bits)}):
        sub = tmp_path / f"n{n}"
        sub.mkdir()
        check_move_writer(h, sub, make_moves(5, n=n, bits=bits), stripes, 2)


def test_move_bucket_writer_refusals(h, tmp_path):
    b = make_moves(3)
    src = put(tmp_path / "in", moves_input(b))
    assert run(h.io, "move-pieces", src, tmp_path / "m.cpd", 4097, 64).startswith(f"ERR {E_ARG} ")
    b.words += 1  # not ceil(n bits / 32)
    b.rows = np.zeros((3, b.words), np.uint32)
    assert run(h.io, "move-pieces", put(tmp_path / "in", moves_input(b)), tmp_path / "m.cpd", 1, 64) \
        .startswith(f"ERR {E_ARG} ")
    b = make_moves(3)
    b.bits = 3
    assert run(h.io, "move-pieces", put(tmp_path / "in", moves_input(b)), tmp_path / "m.cpd", 1, 64) \
        .startswith(f"ERR {E_ARG} ")
    assert os.listdir(tmp_path) == ["in"]


@pytest.mark.parametrize("nrows", [504, 505, 506])
def test_move_bucket_pad(h, tmp_path, nrows):
    """DOSCPD02's zero pad to 4 KiB: 56 + 8 nrows ends exactly on the boundary
    at 505 rows (the rows start at 4096, no pad), one row more starts them at 8192."""
    b = make_moves(nrows, n=16)
    check_move_writer(h, tmp_path, b, 1, 64)
    assert os.path.getsize(tmp_path / "m.cpd") == (4096 if nrows <= 505 else 8192) + 4 * nrows


@pytest.mark.parametrize("stripes", [1, 3])
def test_move_bucket_abandoned(h, tmp_path, stripes):
    """A MoveBucketFile destroyed without close() leaves no .tmp and no part."""
    src = put(tmp_path / "in", moves_input(make_moves(23)))
    assert run(h.io, "move-pieces", src, tmp_path / "m.cpd", stripes, 4, "noclose") == "ok\n"
    assert os.listdir(tmp_path) == ["in"]


def test_move_bucket_rebuild_removes_old_parts(h, tmp_path):
    """close() over an earlier bucket of another graph or with more stripes
    removes the parts the new main file does not name."""
    old = make_moves(23)
    old.fingerprint = FP + 1
    src = put(tmp_path / "in", moves_input(old))
    assert run(h.io, "move-pieces", src, tmp_path / "m.cpd", 5, 4) == "ok\n"
    check_move_writer(h, tmp_path, make_moves(23), 3, 4)  # lists the directory


def test_part_rows(h):
    """MoveBucket::part_rows against a brute-force deal of the rows."""
    out = run(h.io, "part-rows-grid", 40, 5, 7)
    want = "".join(" ".join(str(v) for v in [nr, S, K] + [len(p) for p in BF.deal_rows(nr, S, K)]) + "\n"
                   for nr in range(41) for S in range(1, 6) for K in range(1, 8))
    assert out == want
    assert run(h.io, "part-rows", 23, 4, 3) == "part_rows 8 8 7\n"
    assert run(h.io, "part-rows", 262145, 64, 4096) == \
        " ".join(["part_rows"] + [str(len(p)) for p in BF.deal_rows(262145, 64, 4096)]) + "\n"


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("stripes", [1, 3])
def test_move_rows_windows(h, tmp_path, stripes, threads):
    """read_move_bucket_rows for every (first, count) window of a 23-row
    bucket, striped (S = 4, K = 3) and in one file."""
    b = make_moves(23)
    path, out = put_moves(tmp_path, b, stripes, 4), str(tmp_path / "out")
    assert run(h.io, "move-rows-windows", path, threads, out) == "23\n"
    want = [b.rows[f:f + c].ravel() for f in range(24) for c in range(24 - f)]
    assert open(out, "rb").read() == np.concatenate(want).tobytes()
    assert run(h.io, "move-rows", path, 5, 9, threads, out) == "9\n"
    assert open(out, "rb").read() == b.rows[5:14].tobytes()
    assert run(h.io, "move-rows", path, 20, 4, threads, out).startswith(f"ERR {E_ARG} ")
    assert run(h.io, "move-rows", path, 4294967295, 2, threads, out).startswith(f"ERR {E_ARG} ")


@pytest.mark.parametrize("n", [0, 1, 1000])
def test_order_round_trip(h, tmp_path, n):
    order = np.random.default_rng(n).permutation(n).astype(np.uint32)
    path = str(tmp_path / "g.order")
    data = struct.pack("<I", n) + order.tobytes()
    assert run(h.io, "write-order", put(tmp_path / "in", data), path, FP) == "ok\n"
    assert open(path, "rb").read() == BF.pack_order(FP, order)
    assert sorted(os.listdir(tmp_path)) == ["g.order", "in"]
    assert run(h.io, "order", path, FP) == f"{n}\n" + " ".join(["order"] + [str(v) for v in order]) + "\n"
    assert run(h.io, "order-n", path) == f"{n}\n"


# ---------------------------------------------------------------------------
# Corrupted files: each starts from a valid one and must be refused with
# CPD_E_IO naming the file (or the part file, where that is what is wrong).

def _set(raw, at, fmt, value):
    return raw[:at] + struct.pack(fmt, value) + raw[at + struct.calcsize(fmt):]


def _get(raw, at, fmt):
    return struct.unpack_from(fmt, raw, at)[0]


def _bump(raw, at, fmt, step):
    """The word at `at` one up or down (modulo its width)."""
    return _set(raw, at, fmt, (_get(raw, at, fmt) + step) % 2**(8 * struct.calcsize(fmt)))


def ref_bucket_ok(raw):
    """What DOSCPD01's layout requires of a file."""
    if len(raw) < 48 or raw[:8] != b"DOSCPD01":
        return False
    nrows, total = _get(raw, 12, "<I"), _get(raw, 32, "<Q")
    if len(raw) != 48 + 4 * nrows + 8 * (nrows + 1) + 4 * total:
        return False
    off = np.frombuffer(raw, "<u8", nrows + 1, 48 + 4 * nrows)
    return int(off[0]) == 0 and int(off[-1]) == total


def ref_moves_ok(files):
    """What DOSCPD02 / DOSCPD03 require of a main file and its parts
    ({suffix: bytes}, "" the main file)."""
    raw = files[""]
    striped = raw[:8] == b"DOSCPD03"
    head = 64 if striped else 56
    if len(raw) < head or raw[:8] not in (b"DOSCPD02", b"DOSCPD03"):
        return False
    n, nrows, _, _, _, _, words, bits = struct.unpack_from("<8I", raw, 8)
    total, fp = struct.unpack_from("<2Q", raw, 40)
    if bits not in (1, 2, 4) or words != (n * bits + 31) // 32:
        return False
    if striped:
        K, S = struct.unpack_from("<2I", raw, 56)
        if not 2 <= K <= 4096 or S == 0 or len(raw) != head + 8 * nrows:
            return False
        for j, mine in enumerate(BF.deal_rows(nrows, S, K)):
            part = files.get(f".{fp:016x}.p{j}")
            if part is None or len(part) != 4 * words * len(mine):
                return False
    elif len(raw) != -(-(head + 8 * nrows) // 4096) * 4096 + 4 * words * nrows:
        return False
    counts = np.frombuffer(raw, "<u4", nrows, head + 4 * nrows)
    return bool((counts != 0).all()) and int(counts.sum(dtype=np.uint64)) == total


BUCKET_WORDS = {"n": (8, "<I"), "nrows": (12, "<I"), "bid": (16, "<I"), "method": (20, "<I"), "key": (24, "<I"),
                "maxworker": (28, "<I"), "total": (32, "<Q"), "fingerprint": (40, "<Q")}
MOVE_WORDS = {"n": (8, "<I"), "nrows": (12, "<I"), "bid": (16, "<I"), "method": (20, "<I"), "key": (24, "<I"),
              "maxworker": (28, "<I"), "words": (32, "<I"), "bits": (36, "<I"), "total_runs": (40, "<Q"),
              "fingerprint": (48, "<Q"), "stripes": (56, "<I"), "stripe_rows": (60, "<I")}


def test_bucket_header_words_off_by_one(h, tmp_path):
    """Every DOSCPD01 header word one up and one down.  The words the layout
    hangs on (nrows, total) make the file inconsistent and it is refused by
    both readers; the others (n, bid, method, key, maxworker, fingerprint) are
    the reader's to report, not to judge — deliberately: the loader compares
    them with the graph and the request."""
    b = make_bucket(5)
    good = bucket_bytes(b)
    assert ref_bucket_ok(good)
    for word, (at, fmt) in BUCKET_WORDS.items():
        for step in (1, -1):
            raw = _bump(good, at, fmt, step)
            path, out = put(tmp_path / "b.cpd", raw), str(tmp_path / "out")
            assert ref_bucket_ok(raw) == (word not in ("nrows", "total"))
            for cmd in ("bucket", "bucket-head"):
                got = run(h.io, cmd, path, out)
                if word in ("nrows", "total"):
                    assert refused(got, path), (word, step, cmd, got)
                else:
                    assert f"{word} {_get(raw, at, fmt)} " in got, (word, step, cmd, got)


@pytest.mark.parametrize("stripes", [1, 3])
def test_move_header_words_off_by_one(h, tmp_path, stripes):
    """The same for DOSCPD02 and DOSCPD03 (23 rows of 3 words, S = 4): nrows,
    words, bits, total_runs, and with parts stripes, stripe_rows and the
    fingerprint their names carry, are refused; n one down still rounds to the
    same row width and reads, like the words the reader only reports."""
    b = make_moves(23)
    good = moves_files(b, stripes, 4)
    assert ref_moves_ok(good)
    structural = {"nrows", "words", "bits", "total_runs"} | ({"stripes", "stripe_rows", "fingerprint"}
                                                            if stripes > 1 else set())
    for word, (at, fmt) in MOVE_WORDS.items():
        if at >= 56 and stripes == 1:
            continue
        for step in (1, -1):
            sub = tmp_path / f"{word}{step}"
            sub.mkdir()
            files = dict(good)
            files[""] = _bump(good[""], at, fmt, step)
            for suffix, data in files.items():
                path = put(str(sub / "m.cpd") + suffix, data)
            path = str(sub / "m.cpd")
            ok = ref_moves_ok(files)
            assert ok == (word not in structural and (word, step) != ("n", 1)), (word, step)
            got = run(h.io, "move-head", path)
            if ok:
                assert f" {word} {_get(files[''], at, fmt)} " in " " + got, (word, step, got)
            else:
                assert refused(got, path), (word, step, got)  # `path` is a prefix of the parts' names too


def _order_file():
    return BF.pack_order(FP, np.arange(6, dtype=np.uint32)[::-1])


def _bucket_corruptions():
    b = make_bucket(5)
    good = bucket_bytes(b)
    off0, runs0 = 48 + 4 * 5, 48 + 4 * 5 + 8 * 6
    cases = {"magic": b"DOSCPD00" + good[8:], "magic_02": b"DOSCPD02" + good[8:], "order_magic": b"DOSORD01" + good[8:],
             "first_offset": _set(good, off0, "<Q", 1),
             "last_offset": _set(good, runs0 - 8, "<Q", len(b.runs) - 1),
             "last_offset_up": _set(good, runs0 - 8, "<Q", len(b.runs) + 1),
             "total_wraps": _set(good, 32, "<Q", 2**62),  # 4 * total wraps to 0
             "byte_short": good[:-1], "byte_long": good + b"\0", "empty": b""}
    for name, cut in (("cut_magic", 8), ("cut_magic_mid", 5), ("cut_header", 48), ("cut_header_mid", 40),
                      ("cut_targets", off0), ("cut_offsets", runs0)):
        cases[name] = good[:cut]
    return cases


BUCKET_CORRUPTIONS = _bucket_corruptions()


@pytest.mark.parametrize("case", sorted(BUCKET_CORRUPTIONS))
def test_bucket_corruptions(h, tmp_path, case):
    raw = BUCKET_CORRUPTIONS[case]
    assert not ref_bucket_ok(raw)
    path, out = put(tmp_path / "b.cpd", raw), str(tmp_path / "out")
    for cmd in ("bucket", "bucket-head"):
        got = run(h.io, cmd, path, out)
        assert refused(got, path), (cmd, got)


def _move_corruptions(stripes):
    b = make_moves(23)
    good = moves_files(b, stripes, 4)
    main = good[""]
    head = 64 if stripes > 1 else 56
    cases = {}

    def case(name, new_main=None, **parts):
        files = dict(good)
        if new_main is not None:
            files[""] = new_main
        for suffix, data in parts.items():
            if data is None:
                del files[suffix]
            else:
                files[suffix] = data
        cases[name] = files

    case("magic", b"DOSCPD04" + main[8:])
    case("magic_01", b"DOSCPD01" + main[8:])
    case("magic_other_layout", (b"DOSCPD02" if stripes > 1 else b"DOSCPD03") + main[8:])
    case("bits_3", _set(main, 36, "<I", 3))
    case("bits_8_words_match", _set(_set(main, 36, "<I", 8), 32, "<I", 12))
    case("zero_count", _set(_set(main, head + 4 * 23, "<I", 0), head + 4 * 24, "<I",
                            _get(main, head + 4 * 23, "<I") + _get(main, head + 4 * 24, "<I")))
    case("total_runs_up", _set(main, 40, "<Q", _get(main, 40, "<Q") + 1))
    case("byte_short", main[:-1])
    case("byte_long", main + b"\0")
    case("empty", b"")
    for name, cut in (("cut_magic", 8), ("cut_fixed_header", 56), ("cut_header", head), ("cut_header_mid", 30),
                      ("cut_targets", head + 4 * 23), ("cut_counts", head + 8 * 23)):
        if cut < len(main):
            case(name, main[:cut])
    if stripes == 1:
        case("cut_pad", main[:4096])
        case("row_short", main[:-12])
    else:
        for k in (0, 1, 4097):
            case(f"stripes_{k}", _set(main, 56, "<I", k))
        case("stripe_rows_0", _set(main, 60, "<I", 0))
        p1 = f".{FP:016x}.p1"
        case("part_missing", **{p1: None})
        case("part_row_short", **{p1: good[p1][:-12]})
        case("part_byte_long", **{p1: good[p1] + b"\0"})
    return cases


MOVE_CORRUPTIONS = {(K, name): files for K in (1, 3) for name, files in _move_corruptions(K).items()}


@pytest.mark.parametrize("stripes,case", sorted(MOVE_CORRUPTIONS))
def test_move_bucket_corruptions(h, tmp_path, stripes, case):
    files = MOVE_CORRUPTIONS[(stripes, case)]
    assert not ref_moves_ok(files)
    for suffix, data in files.items():
        put(str(tmp_path / "m.cpd") + suffix, data)
    path = str(tmp_path / "m.cpd")
    got = run(h.io, "move-head", path)
    assert refused(got, path), got
    if case.startswith("part_"):  # the part is what is wrong: its own name in the message
        assert path + f".{FP:016x}.p1" in got, got
        assert run(h.io, "move-head", path, "noparts") == moves_head_output(make_moves(23), 3, 4)
        if case != "part_byte_long":  # the rows themselves are then missing
            assert refused(run(h.io, "move-rows-windows", path, 1, tmp_path / "out"), path)


def test_move_bucket_old_part_names(h, tmp_path):
    """Parts under the earlier {bucket}.p{j} names (no fingerprint) are not
    read; the message says what they are."""
    files = moves_files(make_moves(23), 3, 4)
    path = str(tmp_path / "m.cpd")
    for suffix, data in files.items():
        put(path + (suffix if not suffix else "." + suffix.split(".")[-1]), data)
    assert sorted(os.listdir(tmp_path)) == ["m.cpd", "m.cpd.p0", "m.cpd.p1", "m.cpd.p2"]
    got = run(h.io, "move-head", path)
    assert refused(got, path) and "older {bucket}.p{j} names" in got, got


def test_bucket_format(h, tmp_path):
    for magic, want in ((b"DOSCPD01", "1\n"), (b"DOSCPD02", "2\n"), (b"DOSCPD03", "2\n")):
        assert run(h.io, "bucket-format", put(tmp_path / "f", magic)) == want  # the magic alone decides
    for raw in (b"DOSCPD04" + bytes(100), b"DOSORD01" + bytes(100), b"doscpd01" + bytes(100), b"DOSCPD0", b"",
                bytes(range(256))):
        path = put(tmp_path / "f", raw)
        assert refused(run(h.io, "bucket-format", path), path), raw[:8]
    missing = str(tmp_path / "none")
    for cmd in (["bucket-format", missing], ["bucket", missing, missing + ".out"], ["move-head", missing],
                ["order", missing, 1], ["order-n", missing], ["xy", missing], ["scen", missing]):
        assert refused(run(h.io, *cmd), missing), cmd


def test_order_corruptions(h, tmp_path):
    good = _order_file()
    path = put(tmp_path / "g.order", good)
    assert run(h.io, "order", path, FP) == "6\norder 5 4 3 2 1 0\n"
    got = run(h.io, "order", path, FP + 1)
    assert refused(got, path) and "different graph" in got
    cases = {"magic": b"DOSORD02" + good[8:], "n_up": _set(good, 8, "<I", 7), "n_down": _set(good, 8, "<I", 5),
             "byte_short": good[:-1], "byte_long": good + b"\0", "cut_magic": good[:8], "cut_n": good[:12],
             "cut_header": good[:20], "cut_header_mid": good[:15], "empty": b""}
    for name, raw in cases.items():
        path = put(tmp_path / f"{name}.order", raw)
        assert refused(run(h.io, "order", path, FP), path), name
        if name in ("magic", "cut_magic", "empty"):
            assert refused(run(h.io, "order-n", path), path), name


def test_header_claims_more_than_the_file_holds(plain, tmp_path):
    """A row count (an .order's n) of 0xFFFFFFFF in an otherwise valid small
    file: the readers compare the file's size with its header before they size
    anything by the header, so under a 1-GiB address-space limit the answer is
    "size does not match its header", not std::bad_alloc.  The limit is a
    condition, not a measurement: no valid file here is more than a few MB, and
    the same harness reads the valid original under the same limit first.
    Plain build only: AddressSanitizer reserves its shadow memory up front."""
    gib = 1 << 30
    out = str(tmp_path / "out")
    b, m = make_bucket(5), make_moves(23)
    files = {"b.cpd": (bucket_bytes(b), 12, [["bucket", "{}", out], ["bucket-head", "{}", out]]),
             "g.order": (_order_file(), 8, [["order", "{}", FP]])}
    for name, stripes in (("m2.cpd", 1), ("m3.cpd", 3)):
        packed = moves_files(m, stripes, 4)
        for suffix, data in packed.items():
            put(str(tmp_path / name) + suffix, data)
        files[name] = (packed[""], 12, [["move-head", "{}"], ["move-head", "{}", "noparts"]])
    for name, (good, at, cmds) in files.items():
        path = put(tmp_path / name, good)
        for cmd in cmds:
            cmd = [path if a == "{}" else a for a in cmd]
            assert not run(plain.io, *cmd, limit_as=gib).startswith("ERR"), cmd
        put(path, _set(good, at, "<I", 0xFFFFFFFF))
        for cmd in cmds:
            cmd = [path if a == "{}" else a for a in cmd]
            got = run(plain.io, *cmd, limit_as=gib)
            assert refused(got, path) and "size does not match its header" in got, (cmd, got)
