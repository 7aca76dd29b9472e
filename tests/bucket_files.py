"""The binary files of csrc/cpd_io.hpp stated in Python, from its layout
comments: readers (used by the driver tests on what make_cpd_auto wrote) and
packers (what the writers must produce byte for byte, tests/test_io_cpu.py).
Nothing here calls the library."""
import struct

import numpy as np

MOVE_ROWS_ALIGN = 4096


def read_bucket(path):
    """The bucket layout of csrc/cpd_io.cpp (write_bucket / BucketFile)."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"DOSCPD01"
    n, nrows, bid, method, key, maxworker = np.frombuffer(raw, np.uint32, 6, 8)
    total = int(np.frombuffer(raw, np.uint64, 1, 32)[0])
    p = 48
    targets = np.frombuffer(raw, np.uint32, nrows, p)
    p += 4 * int(nrows)
    off = np.frombuffer(raw, np.uint64, nrows + 1, p)
    p += 8 * (int(nrows) + 1)
    runs = np.frombuffer(raw, np.uint32, total, p)
    assert p + 4 * total == len(raw)
    return targets, off, runs


def read_move_bucket(path):
    """The compact bucket layouts of csrc/cpd_io.cpp (MoveBucketFile): DOSCPD02
    (rows after the header) or DOSCPD03 (rows striped over part files
    {path}.{fingerprint:016x}.p{j}: unit u of stripe_rows rows is unit u // K of
    part u % K)."""
    raw = open(path, "rb").read()
    assert raw[:8] in (b"DOSCPD02", b"DOSCPD03")
    n, nrows, bid, method, key, maxworker, words, bits = (int(x) for x in np.frombuffer(raw, np.uint32, 8, 8))
    assert bits in (1, 2, 4) and words == (n * bits + 31) // 32
    total = int(np.frombuffer(raw, np.uint64, 1, 40)[0])
    if raw[:8] == b"DOSCPD02":
        p = 56
        targets = np.frombuffer(raw, np.uint32, nrows, p)
        counts = np.frombuffer(raw, np.uint32, nrows, p + 4 * nrows)
        rows_at = -(-(p + 8 * nrows) // 4096) * 4096
        assert len(raw) == rows_at + 4 * words * nrows
        moves = np.frombuffer(raw, np.uint32, nrows * words, rows_at).reshape(nrows, words)
    else:
        K, S = (int(x) for x in np.frombuffer(raw, np.uint32, 2, 56))
        p = 64
        targets = np.frombuffer(raw, np.uint32, nrows, p)
        counts = np.frombuffer(raw, np.uint32, nrows, p + 4 * nrows)
        assert len(raw) == p + 8 * nrows
        fp = int(np.frombuffer(raw, np.uint64, 1, 48)[0])
        parts = [np.fromfile(f"{path}.{fp:016x}.p{j}", np.uint32).reshape(-1, words)
                 for j in range(K)]
        moves = np.empty((nrows, words), np.uint32)
        for u in range(-(-nrows // S)):
            r0, r1 = u * S, min(nrows, u * S + S)
            q = (u // K) * S
            moves[r0:r1] = parts[u % K][q:q + (r1 - r0)]
        assert sum(len(x) for x in parts) == nrows
    assert int(counts.sum()) == total
    return targets, counts, moves, bits


def _u32(a):
    return np.ascontiguousarray(a, dtype="<u4").tobytes()


def _u64(a):
    return np.ascontiguousarray(a, dtype="<u8").tobytes()


def pack_bucket(n, bid, method, key, maxworker, fingerprint, targets, offsets, runs):
    """DOSCPD01: magic | n nrows bid method key maxworker (6 x u32) | total u64 |
    fingerprint u64 | targets u32[nrows] | offsets u64[nrows + 1] | runs u32[total]."""
    nrows, total = len(targets), len(runs)
    assert len(offsets) == nrows + 1
    return (b"DOSCPD01" + struct.pack("<6IQQ", n, nrows, bid, method, key, maxworker, total, fingerprint)
            + _u32(targets) + _u64(offsets) + _u32(runs))


def part_name(path, fingerprint, j):
    return f"{path}.{fingerprint:016x}.p{j}"


def deal_rows(nrows, S, K):
    """Row numbers of each part: units of S rows dealt round robin, unit u to
    part u % K, in order (brute force, one row at a time)."""
    parts = [[] for _ in range(K)]
    for r in range(nrows):
        parts[(r // S) % K].append(r)
    return parts


def pack_move_bucket(n, bid, method, key, maxworker, bits, fingerprint, targets, counts, rows,
                     stripes=1, stripe_rows=64):
    """{file name suffix: bytes}: "" is the main file.  stripes 1 is DOSCPD02
    (magic | 8 x u32 | total_runs u64 | fingerprint u64 | targets | counts | zero
    pad to 4 KiB | rows); more is DOSCPD03 (the same 56 bytes | stripes
    stripe_rows | targets | counts, and the rows in part files)."""
    nrows = len(targets)
    words = (n * bits + 31) // 32
    rows = np.ascontiguousarray(rows, dtype="<u4").reshape(nrows, words)
    head = struct.pack("<8IQQ", n, nrows, bid, method, key, maxworker, words, bits,
                       int(np.asarray(counts, dtype=np.uint64).sum()), fingerprint)
    if stripes <= 1:
        main = b"DOSCPD02" + head + _u32(targets) + _u32(counts)
        main += b"\0" * (-len(main) % MOVE_ROWS_ALIGN)
        return {"": main + rows.tobytes()}
    files = {"": b"DOSCPD03" + head + struct.pack("<2I", stripes, stripe_rows) + _u32(targets) + _u32(counts)}
    for j, mine in enumerate(deal_rows(nrows, stripe_rows, stripes)):
        files[f".{fingerprint:016x}.p{j}"] = rows[mine].tobytes() if mine else b""
    return files


def pack_order(fingerprint, order):
    """.order: magic "DOSORD01" | n u32 | fingerprint u64 | order u32[n]."""
    return b"DOSORD01" + struct.pack("<IQ", len(order), fingerprint) + _u32(order)
