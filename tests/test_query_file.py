"""The worker's query-file reader (csrc/cpd_io.cpp read_query_file: one
buffer, lines parsed by up to T threads) against the format
process_query.send_queries writes (process_query.py:93-96: "{n}\\n" then n
"s t" lines): every thread count gives the file's pairs in order; blank
lines are skipped; a bad line, a count that disagrees with the lines and a
missing header are errors.  Host only: the harness is compiled from the
library's sources with g++."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-oracle-search_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    out = str(tmp_path_factory.mktemp("qf") / "qf")
    subprocess.run([gxx, "-O2", "-std=c++17", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(CSRC, "cpd_io.cpp"), os.path.join(ROOT, "tests", "query_file_check.cpp"),
                    "-o", out, "-lpthread"], check=True, capture_output=True, timeout=240)
    return out


def _read(harness, path, threads):
    p = subprocess.run([harness, path, str(threads)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    return p.stdout


def test_pairs_in_order_any_thread_count(harness, tmp_path):
    rng = np.random.default_rng(3)
    for n in (0, 1, 7, 250_000):
        s = rng.integers(0, 2**32 - 1, n, dtype=np.uint64)
        t = rng.integers(0, 4_000_000, n, dtype=np.uint64)
        path = str(tmp_path / f"q{n}")
        body = "".join(f"{a} {b}\n" for a, b in zip(s.tolist(), t.tolist()))
        if n == 7:  # blank lines and CRLF endings are tolerated
            body = body.replace("\n", "\r\n", 2) + "\n\n"
        with open(path, "w") as f:
            f.write(f"{n}\n" + body)
        want = f"{n}\n" + "".join(f"{a} {b}\n" for a, b in zip(s.tolist(), t.tolist()))
        for threads in (1, 3, 16):
            assert _read(harness, path, threads) == want, (n, threads)


def test_errors(harness, tmp_path):
    cases = {"bad_line": "3\n1 2\n3 x\n5 6\n", "count": "4\n1 2\n3 4\n",
             "no_header": "\n1 2\n", "negative": "1\n-1 2\n"}
    for name, text in cases.items():
        path = str(tmp_path / name)
        with open(path, "w") as f:
            f.write(text)
        for threads in (1, 8):
            assert _read(harness, path, threads).startswith("ERR"), (name, threads)
    empty = str(tmp_path / "empty")
    open(empty, "w").close()
    assert _read(harness, empty, 4) == "0\n"


def _fixed_lines(n, ending, seed):
    """n "s t" lines of equal length (7-digit numbers) and their pairs."""
    rng = np.random.default_rng(seed)
    s = rng.integers(1_000_000, 10_000_000, n).tolist()
    t = rng.integers(1_000_000, 10_000_000, n).tolist()
    return [f"{a} {b}{ending}" for a, b in zip(s, t)], "".join(f"{a} {b}\n" for a, b in zip(s, t))


def test_bad_line_number_in_a_later_piece(harness, tmp_path):
    """A bad line in the second and in the last piece of a 4.8-MB body (3
    pieces at 3 threads, 4 at 16: pieces of >= 1 MB) reports its true 1-based
    line number, the header being line 1."""
    n = 300_000
    lines, _ = _fixed_lines(n, "\n", 4)
    for where in (int(0.4 * n), int(0.95 * n)):
        bad = list(lines)
        bad[where] = "1234567 x234567\n"
        path = str(tmp_path / f"bad{where}")
        with open(path, "w") as f:
            f.write(f"{n}\n" + "".join(bad))
        for threads, pieces in ((3, 3), (16, 4)):
            first, last = 16 * n * (pieces - 1) // pieces, 16 * n // pieces  # last piece from, second from
            assert (last <= 16 * where < 2 * last) if where < n // 2 else (16 * where >= first)
            assert _read(harness, path, threads) == f"ERR {path}: bad query line {where + 2}\n", (where, threads)


def test_source_of_25_digits_is_an_error(harness, tmp_path):
    for text in ("1\n1234567890123456789012345 2\n", "1\n2 1234567890123456789012345\n",
                 "1\n18446744073709551621 2\n", "1\n4294967296 2\n"):
        path = str(tmp_path / "long")
        with open(path, "w") as f:
            f.write(text)
        for threads in (1, 8):
            assert _read(harness, path, threads) == f"ERR {path}: bad query line 2\n", text
    with open(path, "w") as f:
        f.write("1\n4294967295 0\n")
    assert _read(harness, path, 1) == "1\n4294967295 0\n"


@pytest.mark.parametrize("ending", ["\n", "\r\n"])
def test_piece_boundary_on_a_line_start_and_inside_a_crlf(harness, tmp_path, ending):
    """The body is cut at body + len k / T, moved on to the next line start.
    With equal 16-byte lines and n a multiple of 12 the cuts at T = 3 and 4
    fall exactly on line starts; with 17-byte CRLF lines and one more digit in
    the first line they fall on the LF of a CRLF.  Either way the pairs come
    out once each, in order."""
    n = 300_000
    lines, want = _fixed_lines(n, ending, 5)
    if ending == "\r\n":
        lines[0] = "1" + lines[0]
        want = "1" + want
    body = "".join(lines)
    for pieces in (3, 4):
        for k in range(1, pieces):
            at = len(body) * k // pieces
            if ending == "\n":
                assert body[at - 1] == "\n"  # a line start
            elif k * 3 == pieces or k * 4 == pieces:
                assert body[at - 1:at + 1] == "\r\n"  # between the CR and the LF
    path = str(tmp_path / "q")
    with open(path, "w", newline="") as f:
        f.write(f"{n}{ending}" + body)
    for threads in (3, 16):
        assert _read(harness, path, threads) == f"{n}\n" + want, threads
