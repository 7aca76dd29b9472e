"""Python mirror of the libcpd C ABI (include/cpd_api.h) over ctypes.

Host-side glue for tests, bench.py and __graft_entry__: numpy arrays in, numpy
arrays out, CPD_E_* codes raised as CpdError.  The compute path is libcpd.so
(HIP kernels for gfx950); there is no Python or CPU fallback here — if the
shared library is missing, importing this module raises.

Reference interfaces mirrored (the reference has no FFI; these are the
executables' contracts):
  partition()          <- distribution_controller / gen_distribute_conf
                          (process_query.py:46-53)
  Graph.build_rows()   <- make_cpd_auto's per-node row loop (README.md:82-95)
  Index.query()        <- fifo_auto --alg table-search (make_fifos.py:20-21)
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CPD_LIB: another build of the library (A/B runs of two builds in one job)
LIB_PATH = os.environ.get("CPD_LIB") or os.path.join(_HERE, "libcpd.so")

CPD_OK = 0
CPD_E_ARG = -1
CPD_E_HIP = -2
CPD_E_OOM = -3
CPD_E_NOROW = -4
CPD_E_RANGE = -5
CPD_E_IO = -6
PART_DIV = 0
PART_MOD = 1
INF = 0xFFFFFFFF
FM_ALL = 0xFFFF
MAX_WEIGHT_SETS = 8
MAX_LOAD_SLICES = 8
LOADS_ACCUMULATE = 1
TIMED_LOADS = 2
STEP_LINE = 0xFFFFFFFF
ALPHA_CONJ = 0xFFFFFFFF
ALPHA_MAX = 64881
BI_AUTO = 0xFFFFFFFF
BI_MAX = (1 << 23) - 1

EXPORTED = [
    "cpd_last_error", "cpd_version", "cpd_partition", "cpd_partition_nbuckets",
    "cpd_dfs_preorder", "cpd_synth_road_graph", "cpd_synth_congestion",
    "cpd_plan_create", "cpd_hierarchy_create", "cpd_plan_info_get", "cpd_plan_order",
    "cpd_plan_export_ch",
    "cpd_plan_save", "cpd_plan_load", "cpd_plan_free", "cpd_device_count",
    "cpd_graph_create", "cpd_graph_set_batch", "cpd_graph_get_batch", "cpd_graph_free",
    "cpd_build_rows", "cpd_rows_count", "cpd_rows_export", "cpd_rows_export_range",
    "cpd_rows_targets", "cpd_rows_wait", "cpd_rows_free",
    "cpd_debug_rows", "cpd_index_create", "cpd_index_from_rows", "cpd_index_set_weights",
    "cpd_query_batch", "cpd_query_prepare", "cpd_query_run", "cpd_query_fetch",
    "cpd_index_free", "cpd_timing_enable", "cpd_timing_reset", "cpd_timing_get",
    "cpd_index_set_mode", "cpd_index_get_mode", "cpd_plan_cache", "cpd_index_create_empty",
    "cpd_index_append_rows", "cpd_index_append_built_rows", "cpd_index_info",
    "cpd_synth_road_graph_ex", "cpd_query_search", "cpd_query_search_counters",
    "cpd_graph_set_coords", "cpd_host_alloc", "cpd_host_free",
    "cpd_rows_lanes", "cpd_graph_hint_next", "cpd_graph_set_hbm_reserve",
    "cpd_device_mem_info", "cpd_rows_move_words", "cpd_rows_export_moves",
    "cpd_index_append_moves", "cpd_device_arena", "cpd_device_arena_release", "cpd_batch_bytes",
    "cpd_rows_move_bits", "cpd_graph_move_bits", "cpd_bucket_bytes", "cpd_space_check",
    "cpd_query_paths", "cpd_query_paths_fetch", "cpd_query_search_paths",
    "cpd_index_set_weight_sets", "cpd_query_costs", "cpd_query_costs_fetch",
    "cpd_query_loads", "cpd_query_loads_fetch", "cpd_query_loads_clear", "cpd_query_search_loads",
    "cpd_query_timed", "cpd_query_timed_fetch",
    "cpd_index_weights_from_loads", "cpd_index_get_weights", "cpd_index_get_weight_sets",
    "cpd_query_assign",
    "cpd_index_flow_step", "cpd_index_flow_fetch", "cpd_index_flow_clear", "cpd_query_assign_line",
    "cpd_index_flow_step_conj", "cpd_index_target_fetch", "cpd_query_assign_conj",
    "cpd_index_flow_step_bi", "cpd_query_assign_bi",
]
# entry points with a digit in the name, listed apart: EXPORTED is compared with
# a scan of the header for names of letters and underscores
EXPORTED_MORE = ["cpd_index_target2_fetch"]
# generator styles (cpd_synth_road_graph_ex flags): "shuffled" is round 1's
# graph (ids permuted, one-way streets, out-edge order shuffled); "spec" is
# SURVEY.md §8(d) as written (row-major ids, bidirectional, E/N/W/S order)
SYNTH_STYLES = {"shuffled": 7, "spec": 0}
INDEX_MODES = {"auto": 0, "rle": 1, "dense": 2}
SEARCH_FORMS = {"auto": 0, "tables": 1, "walks": 2}


class CpdError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libcpd error {code}: {msg}")
        self.code = code


class PlanOpts(C.Structure):
    _fields_ = [("threads", C.c_int), ("witness_settle", C.c_uint32), ("verbose", C.c_int),
                ("no_hierarchy", C.c_int), ("ch_gpu", C.c_int), ("ch_device", C.c_int)]


class PlanInfo(C.Structure):
    _fields_ = [("n", C.c_uint32), ("m", C.c_uint32), ("ch_up_arcs", C.c_uint64),
                ("ch_dn_arcs", C.c_uint64), ("levels_up", C.c_uint32),
                ("levels_dn", C.c_uint32), ("dist_bound", C.c_uint64),
                ("ch_seconds", C.c_double)]


class QueryStats(C.Structure):
    _fields_ = [("queries", C.c_uint64), ("finished", C.c_uint64), ("hops", C.c_uint64),
                ("cost", C.c_uint64), ("kernel_ms", C.c_double)]


class SearchOpts(C.Structure):
    _fields_ = [("hscale", C.c_double), ("fscale", C.c_double), ("k_moves", C.c_int32),
                ("itrs", C.c_int64), ("time_ns", C.c_uint64), ("capacity", C.c_uint32),
                ("virtual_tick_ns", C.c_uint64), ("tables", C.c_int32),
                ("workspace_frac", C.c_double), ("capacity_max", C.c_uint32)]


class SearchStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("queries", "finished", "expanded", "inserted",
                                          "touched", "updated", "surplus", "plen", "overflow")] + \
               [("kernel_ms", C.c_double), ("lanes", C.c_uint64), ("tables_ms", C.c_double),
                ("tables", C.c_int32), ("reruns", C.c_uint64), ("resumed", C.c_uint64),
                ("restarted", C.c_uint64), ("wasted_expanded", C.c_uint64),
                ("passes", C.c_uint32), ("capacity", C.c_uint32), ("capacity_last", C.c_uint32)]


class SearchPathsInfo(C.Structure):
    _fields_ = [("nodes", C.c_uint64), ("prefix_nodes", C.c_uint64),
                ("prefix_bytes", C.c_uint64), ("paths_ms", C.c_double)]


class SearchLoadsInfo(C.Structure):
    _fields_ = [("moves", C.c_uint64), ("prefix_moves", C.c_uint64),
                ("prefix_nodes", C.c_uint64), ("prefix_bytes", C.c_uint64),
                ("loads_ms", C.c_double)]


class Vdf(C.Structure):
    _fields_ = [("a_num", C.c_uint32), ("a_den", C.c_uint32), ("power", C.c_uint32),
                ("load_div", C.c_uint32)]


class VdfInfo(C.Structure):
    _fields_ = [("tstt_lo", C.c_uint64), ("tstt_hi", C.c_uint64), ("changed", C.c_uint64),
                ("planes", C.c_uint32), ("vdf_ms", C.c_double)]


class AssignIter(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("finished", "sptt_lo", "sptt_hi", "tstt_lo", "tstt_hi",
                                          "moves", "changed")] + \
               [("search_ms", C.c_double), ("loads_ms", C.c_double), ("vdf_ms", C.c_double)]


class FlowInfo(C.Structure):
    _fields_ = [("lambda_q16", C.c_uint32), ("evals", C.c_uint32)] + \
               [(k, C.c_uint64) for k in ("g0_lo", "g0_hi", "xw0_lo", "xw0_hi", "tstt_lo",
                                          "tstt_hi", "changed")] + \
               [("line_ms", C.c_double), ("apply_ms", C.c_double)]


class AssignLineIter(C.Structure):
    _fields_ = AssignIter._fields_ + [("lambda_q16", C.c_uint32), ("evals", C.c_uint32)] + \
               [(k, C.c_uint64) for k in ("g0_lo", "g0_hi", "xw0_lo", "xw0_hi")] + \
               [("line_ms", C.c_double)]


class ConjInfo(C.Structure):
    _fields_ = [("alpha_q16", C.c_uint32), ("lambda_q16", C.c_uint32), ("evals", C.c_uint32)] + \
               [(k, C.c_uint64) for k in ("n_lo", "n_hi", "m_lo", "m_hi", "gy_lo", "gy_hi",
                                          "xw0_lo", "xw0_hi", "g0_lo", "g0_hi", "tstt_lo",
                                          "tstt_hi", "changed")] + \
               [("conj_ms", C.c_double), ("line_ms", C.c_double), ("apply_ms", C.c_double)]


class AssignConjIter(C.Structure):
    _fields_ = AssignLineIter._fields_ + [("alpha_q16", C.c_uint32)] + \
               [(k, C.c_uint64) for k in ("n_lo", "n_hi", "m_lo", "m_hi", "gy_lo", "gy_hi")]


class BiInfo(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("branch", "mu_q16", "nu_q16", "beta0_q16", "beta1_q16",
                                          "beta2_q16", "alpha_q16", "lambda_prev_q16",
                                          "lambda_q16", "evals")] + \
               [(k, C.c_uint64) for k in ("a1_lo", "a1_hi", "b1_lo", "b1_hi", "a2_lo", "a2_hi",
                                          "b2_lo", "b2_hi", "gy_lo", "gy_hi", "xw0_lo", "xw0_hi",
                                          "g0_lo", "g0_hi", "tstt_lo", "tstt_hi", "changed")] + \
               [("bi_ms", C.c_double), ("line_ms", C.c_double), ("apply_ms", C.c_double)]


class AssignBiIter(C.Structure):
    _fields_ = AssignLineIter._fields_ + \
               [(k, C.c_uint32) for k in ("branch", "mu_q16", "nu_q16", "beta0_q16", "beta1_q16",
                                          "beta2_q16", "alpha_q16")] + \
               [(k, C.c_uint64) for k in ("a1_lo", "a1_hi", "b1_lo", "b1_hi", "a2_lo", "a2_hi",
                                          "b2_lo", "b2_hi", "gy_lo", "gy_hi")]


def _u128(lo: int, hi: int) -> int:
    """An unsigned 128-bit value from its two u64 halves."""
    return (hi << 64) | lo


def _s128(lo: int, hi: int) -> int:
    """A signed 128-bit value from its two u64 halves."""
    v = _u128(lo, hi)
    return v - (1 << 128) if hi >> 63 else v


# The keys of an assignment loop's record, in the order of cpd_assign_conj_iter
# (whose fields begin with cpd_assign_line_iter's, which begin with
# cpd_assign_iter's): key, then kind — "plain" the field of that name, "u128" /
# "s128" the value of its _lo and _hi halves.
_ITER_KEYS = (("finished", "plain"), ("sptt", "u128"), ("tstt", "u128"), ("moves", "plain"),
              ("changed", "plain"), ("search_ms", "plain"), ("loads_ms", "plain"),
              ("vdf_ms", "plain"), ("lambda_q16", "plain"), ("evals", "plain"), ("g0", "s128"),
              ("xw0", "u128"), ("line_ms", "plain"), ("alpha_q16", "plain"), ("n", "s128"),
              ("m", "u128"), ("gy", "s128"))
_ITER_NKEYS = {AssignIter: 8, AssignLineIter: 13, AssignConjIter: 17}  # the leading keys a type holds
# cpd_assign_bi_iter: cpd_assign_line_iter's keys, then its own
_BI_KEYS = _ITER_KEYS[:13] + tuple((k, "plain") for k in ("branch", "mu_q16", "nu_q16", "beta0_q16",
                                                          "beta1_q16", "beta2_q16", "alpha_q16")) + \
    (("a1", "s128"), ("b1", "u128"), ("a2", "s128"), ("b2", "s128"), ("gy", "s128"))


def _iter_dict(r) -> dict:
    """One record of an assignment loop as a dict."""
    d = {}
    keys = _BI_KEYS if type(r) is AssignBiIter else _ITER_KEYS[:_ITER_NKEYS[type(r)]]
    for key, kind in keys:
        if kind == "plain":
            d[key] = getattr(r, key)
        else:
            lo, hi = getattr(r, key + "_lo"), getattr(r, key + "_hi")
            d[key] = _s128(lo, hi) if kind == "s128" else _u128(lo, hi)
    return d


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("launches", C.c_uint64), ("ms", C.c_double),
                ("bytes", C.c_double)]


def _load() -> C.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it first (make lib, or "
                          "__graft_entry__.build()); there is no fallback")
    lib = C.CDLL(LIB_PATH)
    lib.cpd_last_error.restype = C.c_char_p
    lib.cpd_version.restype = C.c_char_p
    for name in EXPORTED + EXPORTED_MORE:
        if name not in ("cpd_last_error", "cpd_version"):
            fn = getattr(lib, name)
            if not name.endswith("_free"):
                fn.restype = C.c_int
            else:
                fn.restype = None
    return lib


lib = _load()

u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
u16p = C.POINTER(C.c_uint16)
u8p = C.POINTER(C.c_uint8)
i32p = C.POINTER(C.c_int32)


def _check(rc: int) -> None:
    if rc != CPD_OK:
        raise CpdError(rc, lib.cpd_last_error().decode())


def _ptr(a, ctype):
    if a is None:
        return None
    return a.ctypes.data_as(ctype)


def _u32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint32)


def _search_opts(hscale, fscale, k_moves, itrs, time_ns, capacity, virtual_tick_ns, tables,
                 workspace_frac, capacity_max) -> SearchOpts:
    """cpd_search_opts from the search methods' keywords, in the struct's order."""
    return SearchOpts(float(hscale), float(fscale), int(k_moves), int(itrs), int(time_ns),
                      int(capacity), int(virtual_tick_ns), SEARCH_FORMS[tables],
                      float(workspace_frac), int(capacity_max))


def version() -> str:
    return lib.cpd_version().decode()


def lib_src_sha() -> str:
    """The source hash libcpd.so was built from (embedded by the Makefile)."""
    v = version()
    return v.split("src:", 1)[1] if "src:" in v else ""


def src_sha(root: str | None = None) -> str:
    """sha256 (16 hex) of the library and tool sources in the tree at `root`,
    computed exactly as the Makefile's PROV_SRCS / SRC_SHA: the files sorted by
    repo-relative path, contents concatenated."""
    import glob
    import hashlib
    root = root or os.path.dirname(_HERE)
    pats = ["include/*.h", "distributed-oracle-search_amd/csrc/*.cpp",
            "distributed-oracle-search_amd/csrc/*.hpp", "distributed-oracle-search_amd/csrc/*.hip",
            "distributed-oracle-search_amd/tools/*.cpp", "distributed-oracle-search_amd/tools/*.hpp"]
    files = sorted({os.path.relpath(f, root) for p in pats for f in glob.glob(os.path.join(root, p))})
    h = hashlib.sha256()
    for f in files:
        with open(os.path.join(root, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


# --------------------------------------------------------------------------
# host utilities

def partition(nodenum: int, maxworker: int, method: str, key: int, node: int):
    """(wid, bid, bidx) of `node` — distribution_controller semantics [U]."""
    wid, bid, bidx = C.c_uint32(), C.c_uint32(), C.c_uint32()
    m = PART_MOD if method == "mod" else PART_DIV if method == "div" else -1
    _check(lib.cpd_partition(C.c_uint32(nodenum), C.c_uint32(maxworker), C.c_int(m),
                             C.c_uint32(key), C.c_uint32(node), C.byref(wid), C.byref(bid),
                             C.byref(bidx)))
    return wid.value, bid.value, bidx.value


def owned_nodes(nodenum: int, maxworker: int, method: str, key: int, wid: int) -> np.ndarray:
    """All nodes assigned to worker `wid` (vectorised restatement of partition())."""
    nodes = np.arange(nodenum, dtype=np.int64)
    if method == "mod":
        bid = nodes % key
    elif method == "div":
        chunk = -(-nodenum // key)
        bid = nodes // chunk
    else:
        raise ValueError("partmethod must be div or mod")
    return nodes[(bid % maxworker) == wid].astype(np.uint32)


def bucket_bytes(n: int, bits: int, nrows: int, nbuckets: int = 1, stripes: int = 16) -> int:
    """Bytes of a worker's compact bucket files (cpd_bucket_bytes)."""
    out = C.c_uint64()
    _check(lib.cpd_bucket_bytes(C.c_uint32(n), C.c_uint32(bits), C.c_uint64(nrows),
                                C.c_uint32(nbuckets), C.c_uint32(stripes), C.byref(out)))
    return out.value


def space_check(directory: str, nbytes: int) -> int:
    """Free bytes of the file system holding `directory`; CpdError (CPD_E_IO)
    when fewer than `nbytes` (cpd_space_check: make_cpd_auto's preflight)."""
    avail = C.c_uint64()
    _check(lib.cpd_space_check(directory.encode(), C.c_uint64(nbytes), C.byref(avail)))
    return avail.value


def dfs_preorder(row_ptr, dst) -> np.ndarray:
    row_ptr, dst = _u32(row_ptr), _u32(dst)
    n = len(row_ptr) - 1
    order = np.empty(n, dtype=np.uint32)
    _check(lib.cpd_dfs_preorder(C.c_uint32(n), _ptr(row_ptr, u32p), _ptr(dst, u32p),
                                _ptr(order, u32p)))
    return order


class RoadGraph:
    """CSR graph (node space, file edge order) + coordinates."""

    def __init__(self, row_ptr, dst, w, x=None, y=None):
        self.row_ptr, self.dst, self.w = _u32(row_ptr), _u32(dst), _u32(w)
        self.x, self.y = x, y

    @property
    def n(self) -> int:
        return len(self.row_ptr) - 1

    @property
    def m(self) -> int:
        return len(self.dst)


def synth_road_graph(width: int, height: int, seed: int, mean_outdeg: float = 2.5,
                     style: str = "shuffled") -> RoadGraph:
    flags = SYNTH_STYLES[style]
    n, m = C.c_uint32(), C.c_uint32()
    _check(lib.cpd_synth_road_graph_ex(width, height, C.c_double(mean_outdeg), C.c_uint64(seed),
                                       C.c_uint32(flags), C.byref(n), C.byref(m), None, None,
                                       None, None, None))
    rp = np.empty(n.value + 1, np.uint32)
    dst = np.empty(m.value, np.uint32)
    w = np.empty(m.value, np.uint32)
    x = np.empty(n.value, np.int32)
    y = np.empty(n.value, np.int32)
    _check(lib.cpd_synth_road_graph_ex(width, height, C.c_double(mean_outdeg), C.c_uint64(seed),
                                       C.c_uint32(flags), C.byref(n), C.byref(m), _ptr(rp, u32p),
                                       _ptr(dst, u32p), _ptr(w, u32p), _ptr(x, i32p),
                                       _ptr(y, i32p)))
    return RoadGraph(rp, dst, w, x, y)


def synth_congestion(w, frac=0.1, lo=1.0, hi=3.0, seed=3) -> np.ndarray:
    w = _u32(w)
    out = np.empty_like(w)
    _check(lib.cpd_synth_congestion(C.c_uint32(len(w)), _ptr(w, u32p), C.c_double(frac),
                                    C.c_double(lo), C.c_double(hi), C.c_uint64(seed),
                                    _ptr(out, u32p)))
    return out


# --------------------------------------------------------------------------
# plan (host preprocessing)

class Plan:
    def __init__(self, g: RoadGraph | None = None, threads: int = 0, settle: int = 0,
                 verbose: bool = False, hierarchy: bool = True, gpu: int | None = None,
                 ch_only: bool = False, _handle=None):
        """gpu: contract the hierarchy on this device (None: host threads).
        ch_only: the contraction alone, at any out-degree (cpd_hierarchy_create):
        only info() and export_ch() take such a plan."""
        self._h = C.c_void_p()
        if _handle is not None:
            self._h = _handle
        else:
            opts = PlanOpts(threads, settle, int(verbose), int(not hierarchy),
                            int(gpu is not None), int(gpu or 0))
            create = lib.cpd_hierarchy_create if ch_only else lib.cpd_plan_create
            _check(create(_ptr(g.row_ptr, u32p), _ptr(g.dst, u32p),
                          _ptr(g.w, u32p), C.c_uint32(g.n), C.c_uint32(g.m),
                          C.byref(opts), C.byref(self._h)))

    @classmethod
    def load(cls, path: str) -> "Plan":
        h = C.c_void_p()
        _check(lib.cpd_plan_load(path.encode(), C.byref(h)))
        return cls(_handle=h)

    @classmethod
    def cache(cls, path: str, g: RoadGraph, threads: int = 0, hierarchy: bool = True,
              gpu: int | None = None):
        """(plan, status): the plan cached at `path` for this graph, built and
        saved under an flock if absent (status 0 loaded, 1 built and saved,
        2 built but not saved) — cpd_plan_cache."""
        h = C.c_void_p()
        st = C.c_int()
        opts = PlanOpts(threads, 0, 0, int(not hierarchy), int(gpu is not None), int(gpu or 0))
        _check(lib.cpd_plan_cache(path.encode(), _ptr(g.row_ptr, u32p), _ptr(g.dst, u32p),
                                  _ptr(g.w, u32p), C.c_uint32(g.n), C.c_uint32(g.m),
                                  C.byref(opts), C.byref(h), C.byref(st)))
        return cls(_handle=h), st.value

    def save(self, path: str) -> None:
        _check(lib.cpd_plan_save(self._h, path.encode()))

    def info(self) -> dict:
        i = PlanInfo()
        _check(lib.cpd_plan_info_get(self._h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in PlanInfo._fields_}

    def order(self) -> np.ndarray:
        o = np.empty(self.info()["n"], np.uint32)
        _check(lib.cpd_plan_order(self._h, _ptr(o, u32p)))
        return o

    def export_ch(self) -> dict:
        inf = self.info()
        n, up, dn = inf["n"], inf["ch_up_arcs"], inf["ch_dn_arcs"]
        out = {
            "rank": np.empty(n, np.uint32),
            "up_off": np.empty(n + 1, np.uint64), "up_dst": np.empty(up, np.uint32),
            "up_w": np.empty(up, np.uint32),
            "dn_off": np.empty(n + 1, np.uint64), "dn_dst": np.empty(dn, np.uint32),
            "dn_w": np.empty(dn, np.uint32),
            "level_up": np.empty(n, np.uint32), "level_dn": np.empty(n, np.uint32),
        }
        _check(lib.cpd_plan_export_ch(
            self._h, _ptr(out["rank"], u32p), _ptr(out["up_off"], u64p),
            _ptr(out["up_dst"], u32p), _ptr(out["up_w"], u32p), _ptr(out["dn_off"], u64p),
            _ptr(out["dn_dst"], u32p), _ptr(out["dn_w"], u32p), _ptr(out["level_up"], u32p),
            _ptr(out["level_dn"], u32p)))
        return out

    def __del__(self):
        if getattr(self, "_h", None):
            lib.cpd_plan_free(self._h)
            self._h = None


# --------------------------------------------------------------------------
# GPU

def device_count() -> int:
    c = C.c_int()
    _check(lib.cpd_device_count(C.byref(c)))
    return c.value


def device_mem_info(device: int = 0):
    """(free, total) HBM bytes of `device` (cpd_device_mem_info)."""
    f, t = C.c_uint64(), C.c_uint64()
    _check(lib.cpd_device_mem_info(C.c_int(device), C.byref(f), C.byref(t)))
    return f.value, t.value


class Rows:
    def __init__(self, h):
        self._h = h

    def wait(self) -> None:
        """Finish the (possibly deferred) device work behind these rows."""
        _check(lib.cpd_rows_wait(self._h))

    def count(self):
        nr, tot = C.c_uint32(), C.c_uint64()
        _check(lib.cpd_rows_count(self._h, C.byref(nr), C.byref(tot)))
        return nr.value, tot.value

    def export(self):
        nr, tot = self.count()
        off = np.empty(nr + 1, np.uint64)
        runs = np.empty(tot, np.uint32)
        _check(lib.cpd_rows_export(self._h, _ptr(off, u64p), _ptr(runs, u32p)))
        return off, runs

    def export_range(self, first: int, count: int):
        """Rows [first, first+count): offsets relative to row `first`, runs."""
        off = np.empty(count + 1, np.uint64)
        _check(lib.cpd_rows_export_range(self._h, C.c_uint32(first), C.c_uint32(count),
                                         _ptr(off, u64p), None))
        runs = np.empty(int(off[-1]), np.uint32)
        _check(lib.cpd_rows_export_range(self._h, C.c_uint32(first), C.c_uint32(count),
                                         None, _ptr(runs, u32p)))
        return off, runs

    def offsets(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """Run offsets of rows [first, first+count) relative to row `first`
        (count + 1 values), without the runs."""
        if count is None:
            count = self.count()[0] - first
        off = np.empty(count + 1, np.uint64)
        _check(lib.cpd_rows_export_range(self._h, C.c_uint32(first), C.c_uint32(count),
                                         _ptr(off, u64p), None))
        return off

    def move_words(self) -> int:
        """Words per row of the compact form (ceil(n * bits / 32))."""
        w = C.c_uint32()
        _check(lib.cpd_rows_move_words(self._h, C.byref(w)))
        return w.value

    def move_bits(self) -> int:
        """Bits per move of the compact form (1, 2 or 4)."""
        b = C.c_uint32()
        _check(lib.cpd_rows_move_bits(self._h, C.byref(b)))
        return b.value

    def export_moves(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """Rows [first, first+count) in the compact form: (count, words) u32,
        column c's move in bits [b*c, b*c + b) of the row, b = move_bits()
        (cpd_rows_export_moves)."""
        if count is None:
            count = self.count()[0] - first
        out = np.empty((count, self.move_words()), np.uint32)
        _check(lib.cpd_rows_export_moves(self._h, C.c_uint32(first), C.c_uint32(count),
                                         _ptr(out, u32p)))
        return out

    def targets(self):
        nr, _ = self.count()
        t = np.empty(nr, np.uint32)
        _check(lib.cpd_rows_targets(self._h, _ptr(t, u32p)))
        return t

    def lanes(self):
        """The batch lane each row was built in (cpd_rows_lanes)."""
        nr, _ = self.count()
        a = np.empty(nr, np.uint32)
        _check(lib.cpd_rows_lanes(self._h, _ptr(a, u32p)))
        return a

    def __del__(self):
        if getattr(self, "_h", None):
            lib.cpd_rows_free(self._h)
            self._h = None


class Graph:
    """A plan resident on one GPU."""

    def __init__(self, plan: Plan, device: int = 0, batch: int = 0, hbm_reserve: int = 0):
        self._h = C.c_void_p()
        self.plan = plan
        _check(lib.cpd_graph_create(plan._h, C.c_int(device), C.byref(self._h)))
        if hbm_reserve:
            self.set_hbm_reserve(hbm_reserve)
        # 0 = the largest batch that fits in free HBM above the reserve (<= 24576)
        _check(lib.cpd_graph_set_batch(self._h, C.c_uint32(batch)))

    @property
    def batch(self) -> int:
        b = C.c_uint32()
        _check(lib.cpd_graph_get_batch(self._h, C.byref(b)))
        return b.value

    def set_batch(self, batch: int) -> None:
        """Rows per sweep (multiple of 1024; 0 = what fits in free HBM)."""
        _check(lib.cpd_graph_set_batch(self._h, C.c_uint32(batch)))

    def set_hbm_reserve(self, nbytes: int) -> None:
        """HBM the auto batch leaves free for what follows on this GPU
        (cpd_graph_set_hbm_reserve); applies at the next set_batch(0)."""
        _check(lib.cpd_graph_set_hbm_reserve(self._h, C.c_uint64(nbytes)))

    def move_bits(self) -> int:
        """Bits per move of the compact rows this graph builds."""
        b = C.c_uint32()
        _check(lib.cpd_graph_move_bits(self._h, C.byref(b)))
        return b.value

    def set_coords(self, x, y) -> None:
        """Node coordinates (node-id space; None clears them): a batch's
        targets are laid out over the lanes along a Hilbert curve of them
        (compact 256-target groups; identical results, fewer wide rows)."""
        if x is None or y is None:
            _check(lib.cpd_graph_set_coords(self._h, None, None))
            return
        xs = np.ascontiguousarray(x, dtype=np.int32)
        ys = np.ascontiguousarray(y, dtype=np.int32)
        if len(xs) != self.plan.info()["n"] or len(ys) != len(xs):
            raise ValueError("coordinates must have one entry per node")
        _check(lib.cpd_graph_set_coords(self._h, _ptr(xs, i32p), _ptr(ys, i32p)))

    def build_rows(self, targets, reuse: Rows | None = None) -> Rows:
        t = _u32(targets)
        h = C.c_void_p()
        _check(lib.cpd_build_rows(self._h, _ptr(t, u32p), C.c_uint32(len(t)),
                                  reuse._h if reuse else None, C.byref(h)))
        if reuse is not None:
            return reuse
        return Rows(h)

    def hint_next(self, targets) -> None:
        """The targets the next build_rows() call starts with: its first
        batch's up-sweep may start during the current call (cpd_graph_hint_next)."""
        t = _u32(targets)
        _check(lib.cpd_graph_hint_next(self._h, _ptr(t, u32p), C.c_uint32(len(t))))

    def debug_rows(self, targets, want_dist=True, want_fm=True):
        t = _u32(targets)
        n = self.plan.info()["n"]
        dist = np.empty((n, len(t)), np.uint32) if want_dist else None
        fm = np.empty((len(t), n), np.uint16) if want_fm else None
        _check(lib.cpd_debug_rows(self._h, _ptr(t, u32p), C.c_uint32(len(t)),
                                  _ptr(dist, u32p), _ptr(fm, u16p)))
        return dist, fm

    def timing(self, enable: bool = True) -> None:
        _check(lib.cpd_timing_enable(self._h, C.c_int(int(enable))))

    def timing_reset(self) -> None:
        _check(lib.cpd_timing_reset(self._h))

    def timing_get(self) -> dict:
        arr = (KernelTime * 32)()
        cnt = C.c_int()
        _check(lib.cpd_timing_get(self._h, arr, 32, C.byref(cnt)))
        return {arr[i].name.decode(): {"launches": arr[i].launches, "ms": arr[i].ms,
                                       "bytes": arr[i].bytes} for i in range(cnt.value)}

    def __del__(self):
        if getattr(self, "_h", None):
            lib.cpd_graph_free(self._h)
            self._h = None


class Index:
    def __init__(self, graph: Graph, rows: Rows | None = None, row_targets=None,
                 offsets=None, runs=None, _handle=None):
        self.graph = graph
        self._nq, self._path_offsets = 0, None  # prepared queries; offsets of their paths
        self._nsets, self._cost_cols = 0, None  # weight sets loaded; columns of the last costs_run
        self._load_slices = None                # slices of the resident load table
        self._timed = False                     # a timed_run on the prepared queries
        self._h = C.c_void_p()
        if _handle is not None:
            self._h = _handle
        elif rows is not None:
            _check(lib.cpd_index_from_rows(graph._h, rows._h, C.byref(self._h)))
        else:
            rt, off = _u32(row_targets), np.ascontiguousarray(offsets, np.uint64)
            rn = _u32(runs)
            _check(lib.cpd_index_create(graph._h, _ptr(rt, u32p), C.c_uint32(len(rt)),
                                        _ptr(off, u64p), _ptr(rn, u32p), C.byref(self._h)))

    @classmethod
    def streamed(cls, graph: Graph, row_targets, total_runs: int, mode: str = "auto") -> "Index":
        """Empty index of len(row_targets) rows filled by append()/append_rows()
        in order (cpd_index_create_empty)."""
        rt = _u32(row_targets)
        h = C.c_void_p()
        _check(lib.cpd_index_create_empty(graph._h, _ptr(rt, u32p), C.c_uint32(len(rt)),
                                          C.c_int(INDEX_MODES[mode]), C.c_uint64(total_runs),
                                          C.byref(h)))
        return cls(graph, _handle=h)

    def append(self, offsets, runs) -> None:
        """Host rows: offsets relative to the chunk (count + 1 values)."""
        off = np.ascontiguousarray(offsets, np.uint64)
        rn = _u32(runs)
        _check(lib.cpd_index_append_rows(self._h, C.c_uint32(len(off) - 1), _ptr(off, u64p),
                                         _ptr(rn, u32p)))

    def append_moves(self, moves, bits: int = 4) -> None:
        """Host rows in the compact form: (count, ceil(n * bits / 32)) u32
        (cpd_index_append_moves)."""
        mv = np.ascontiguousarray(moves, np.uint32)
        if mv.ndim != 2:
            raise ValueError("moves must be (rows, words)")
        _check(lib.cpd_index_append_moves(self._h, C.c_uint32(mv.shape[0]), C.c_uint32(bits),
                                          _ptr(mv, u32p)))

    def append_rows(self, rows: Rows) -> None:
        _check(lib.cpd_index_append_built_rows(self._h, rows._h))

    def info(self) -> dict:
        nr, ad, rr, db = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64()
        _check(lib.cpd_index_info(self._h, C.byref(nr), C.byref(ad), C.byref(rr), C.byref(db)))
        return {"nrows": nr.value, "added": ad.value, "runs_resident": rr.value,
                "dense_bytes": db.value}

    def set_mode(self, mode: str) -> None:
        """'auto' (default), 'rle' or 'dense' — see cpd_index_set_mode."""
        _check(lib.cpd_index_set_mode(self._h, C.c_int(INDEX_MODES[mode])))

    @property
    def mode(self) -> str:
        m = C.c_int()
        _check(lib.cpd_index_get_mode(self._h, C.byref(m)))
        return {v: k for k, v in INDEX_MODES.items()}[m.value]

    def set_weights(self, w=None) -> None:
        if w is None:
            _check(lib.cpd_index_set_weights(self._h, None))
        else:
            w = _u32(w)
            _check(lib.cpd_index_set_weights(self._h, _ptr(w, u32p)))

    def query(self, s, t, k_moves: int = -1):
        s, t = _u32(s), _u32(t)
        nq = len(s)
        self._nq, self._path_offsets = 0, None  # cpd_query_batch prepares and runs
        self._cost_cols = None
        self._timed = False
        cost = np.empty(nq, np.uint64)
        hops = np.empty(nq, np.uint32)
        fin = np.empty(nq, np.uint8)
        st = QueryStats()
        _check(lib.cpd_query_batch(self._h, _ptr(s, u32p), _ptr(t, u32p), C.c_uint32(nq),
                                   C.c_int32(k_moves), _ptr(cost, u64p), _ptr(hops, u32p),
                                   _ptr(fin, u8p), C.byref(st)))
        self._nq = nq
        return cost, hops, fin, {k: getattr(st, k) for k, _ in QueryStats._fields_}

    def prepare(self, s, t) -> None:
        s, t = _u32(s), _u32(t)
        self._nq, self._path_offsets = 0, None  # the library drops the last batch's paths
        self._cost_cols = None                  # ... and its costs
        self._timed = False                     # ... and its timed results
        _check(lib.cpd_query_prepare(self._h, _ptr(s, u32p), _ptr(t, u32p), C.c_uint32(len(s))))
        self._nq = len(s)

    def run(self, k_moves: int = -1) -> dict:
        self._path_offsets = None
        st = QueryStats()
        _check(lib.cpd_query_run(self._h, C.c_int32(k_moves), C.byref(st)))
        return {k: getattr(st, k) for k, _ in QueryStats._fields_}

    def paths(self, s, t, k_moves: int = -1):
        """The table-search walks of (s, t) with their nodes (cpd_query_paths):
        (offsets u64[nq + 1], nodes u32[offsets[-1]], cost, hops, finished,
        stats); path q is nodes[offsets[q]:offsets[q + 1]], hops[q] + 1 node
        ids from s[q] to where the walk ended."""
        self.prepare(s, t)
        nq = len(s)
        offsets, st = self.paths_run(k_moves)
        nodes = self.paths_fetch(0, nq)
        cost = np.empty(nq, np.uint64)
        hops = np.empty(nq, np.uint32)
        fin = np.empty(nq, np.uint8)
        _check(lib.cpd_query_fetch(self._h, _ptr(cost, u64p), _ptr(hops, u32p), _ptr(fin, u8p)))
        return offsets, nodes, cost, hops, fin, st

    def paths_run(self, k_moves: int = -1):
        """cpd_query_paths on the prepared queries: (offsets u64[nq + 1], stats).
        The offsets are kept: paths_fetch sizes its buffers from them."""
        self._path_offsets = None
        offsets = np.empty(self._nq + 1, np.uint64)
        st = QueryStats()
        _check(lib.cpd_query_paths(self._h, C.c_int32(k_moves), _ptr(offsets, u64p), C.byref(st)))
        self._path_offsets = offsets.copy()
        return offsets, {k: getattr(st, k) for k, _ in QueryStats._fields_}

    def paths_fetch(self, first: int, count: int) -> np.ndarray:
        """Nodes of paths [first, first + count) of the last paths() /
        paths_run(), back to back (cpd_query_paths_fetch).  The library copies
        as many nodes as ITS offsets say, so this refuses (CPD_E_ARG, as the
        library would) whenever the offsets of that very call are not at hand
        or the range leaves them: the buffer is never sized by guesswork."""
        off = self._path_offsets
        if off is None:
            raise CpdError(CPD_E_ARG, "paths fetch: no paths() / paths_run() on the prepared "
                                      "queries yet")
        if first < 0 or count < 0 or first + count > len(off) - 1:
            raise CpdError(CPD_E_ARG, f"paths fetch: queries [{first}, {first + count}) past the "
                                      f"batch's {len(off) - 1}")
        nodes = np.empty(int(off[first + count]) - int(off[first]), np.uint32)
        _check(lib.cpd_query_paths_fetch(self._h, C.c_uint32(first), C.c_uint32(count),
                                         _ptr(nodes, u32p)))
        return nodes

    def set_weight_sets(self, sets=None) -> None:
        """Weight sets for costs() (cpd_index_set_weight_sets): a list of up to
        MAX_WEIGHT_SETS arrays of m weights in original edge order, None in
        the list = the free-flow weights; None or an empty list clears them.
        Independent of set_weights()."""
        sets = [] if sets is None else list(sets)
        arrs = [None if w is None else _u32(w) for w in sets]
        ptrs = (u32p * max(1, len(arrs)))(*[_ptr(a, u32p) for a in arrs])
        _check(lib.cpd_index_set_weight_sets(self._h, C.c_uint32(len(arrs)),
                                             ptrs if arrs else None))
        self._nsets = len(arrs)

    def costs(self, s, t, k_moves: int = -1, slice_moves: int = 0):
        """The table-search walks of (s, t) costed under the loaded weight sets
        in one walk (cpd_query_costs): (costs u64[nq, C], hops, finished,
        stats).  slice_moves = 0: C = the number of sets, column j the cost
        under set j; slice_moves = S > 0: C = 1, move h of a walk costed under
        set min(h // S, nsets - 1)."""
        self.prepare(s, t)
        st = self.costs_run(k_moves, slice_moves)
        costs, hops, fin = self.costs_fetch()
        return costs, hops, fin, st

    def costs_run(self, k_moves: int = -1, slice_moves: int = 0) -> dict:
        """cpd_query_costs on the prepared queries: stats."""
        self._cost_cols = None
        st = QueryStats()
        _check(lib.cpd_query_costs(self._h, C.c_int32(k_moves), C.c_uint32(slice_moves),
                                   C.byref(st)))
        self._cost_cols = 1 if slice_moves else self._nsets
        return {k: getattr(st, k) for k, _ in QueryStats._fields_}

    def costs_fetch(self):
        """(costs u64[nq, C], hops, finished) of the last costs_run()
        (cpd_query_costs_fetch).  The library copies nq * C values, so this
        refuses (CPD_E_ARG, as the library would) when the C of that very call
        is not at hand."""
        if self._cost_cols is None:
            raise CpdError(CPD_E_ARG, "costs fetch: no costs() / costs_run() on the prepared "
                                      "queries yet")
        nq = self._nq
        costs = np.empty((nq, self._cost_cols), np.uint64)
        hops = np.empty(nq, np.uint32)
        fin = np.empty(nq, np.uint8)
        _check(lib.cpd_query_costs_fetch(self._h, _ptr(costs, u64p), _ptr(hops, u32p),
                                         _ptr(fin, u8p)))
        return costs, hops, fin

    def loads(self, s, t, demand=None, k_moves: int = -1, slices: int = 1, slice_moves: int = 0,
              accumulate: bool = False):
        """The demand every edge carries when the table-search walks of (s, t)
        are routed (cpd_query_loads): (loads u64[slices, m], stats).  demand:
        one u32 per query (None = 1 each), added to loads[j, e] for every move
        of the query's walk, e = the original index of the edge taken (the
        index set_weights() uses), j = min(h // slice_moves, slices - 1) for
        move number h (slices = 1: j = 0, slice_moves = 0).  accumulate=True
        adds to the table earlier calls on this index left."""
        self.prepare(s, t)
        st = self.loads_run(demand, k_moves, slices, slice_moves, accumulate)
        return self.loads_fetch(), st

    def loads_run(self, demand=None, k_moves: int = -1, slices: int = 1, slice_moves: int = 0,
                  accumulate: bool = False) -> dict:
        """cpd_query_loads on the prepared queries: stats (cost / hops /
        finished of this walk then come from cpd_query_fetch)."""
        self._path_offsets = None
        d = self._demand(demand)
        st = QueryStats()
        _check(lib.cpd_query_loads(self._h, C.c_int32(k_moves), _ptr(d, u32p), C.c_uint32(slices),
                                   C.c_uint32(slice_moves),
                                   C.c_uint32(LOADS_ACCUMULATE if accumulate else 0), C.byref(st)))
        self._load_slices = slices
        return {k: getattr(st, k) for k, _ in QueryStats._fields_}

    def loads_fetch(self) -> np.ndarray:
        """loads u64[slices, m] of the resident table (cpd_query_loads_fetch).
        The library copies slices * m values, so this refuses (CPD_E_ARG, as
        the library would) when no loads_run() has made a table since the
        index was created or cleared."""
        if self._load_slices is None:
            raise CpdError(CPD_E_ARG, "loads fetch: no loads() / loads_run() on this index since "
                                      "it was made or cleared")
        out = np.empty((self._load_slices, self.graph.plan.info()["m"]), np.uint64)
        _check(lib.cpd_query_loads_fetch(self._h, _ptr(out, u64p)))
        return out

    def loads_clear(self) -> None:
        """Drop the resident load table (cpd_query_loads_clear)."""
        _check(lib.cpd_query_loads_clear(self._h))
        self._load_slices = None

    def timed(self, s, t, depart=None, period=None, demand=None, k_moves: int = -1,
              loads: bool = False, accumulate: bool = False):
        """The table-search walks of (s, t) on a clock (cpd_query_timed):
        (cost, hops, finished, stats).  Query q leaves at depart[q] (u64,
        weight units; None = 0 each); a move whose edge is entered at clock
        time tau is costed under weight set min(tau // period, nsets - 1) and
        advances the clock by that weight; cost = arrival - departure.
        loads=True: demand[q] (u32; None = 1 each) is added to counter (set,
        edge) of the load table for every move — loads_fetch() returns its
        nsets planes; accumulate=True adds to a resident timed table of the
        same sets and period."""
        self.prepare(s, t)
        st = self.timed_run(depart, period, demand, k_moves, loads, accumulate)
        cost, hops, fin = self.timed_fetch()
        return cost, hops, fin, st

    def timed_run(self, depart=None, period=None, demand=None, k_moves: int = -1,
                  loads: bool = False, accumulate: bool = False) -> dict:
        """cpd_query_timed on the prepared queries: stats."""
        if period is None:
            raise ValueError("period is required")
        self._timed = False
        dp = None
        if depart is not None:
            dp = np.ascontiguousarray(depart, dtype=np.uint64)
            if dp.shape != (self._nq,):
                raise ValueError("depart must have one entry per prepared query")
        d = self._demand(demand)
        flags = (TIMED_LOADS if loads else 0) | (LOADS_ACCUMULATE if accumulate else 0)
        st = QueryStats()
        _check(lib.cpd_query_timed(self._h, C.c_int32(k_moves), _ptr(dp, u64p),
                                   C.c_uint64(period), _ptr(d, u32p), C.c_uint32(flags),
                                   C.byref(st)))
        self._timed = True
        if loads:
            self._load_slices = self._nsets
        return {k: getattr(st, k) for k, _ in QueryStats._fields_}

    def timed_fetch(self):
        """(cost u64[nq], hops, finished) of the last timed_run() in the
        caller's order (cpd_query_timed_fetch)."""
        if not self._timed:
            raise CpdError(CPD_E_ARG, "timed fetch: no timed() / timed_run() on the prepared "
                                      "queries yet")
        nq = self._nq
        cost = np.empty(nq, np.uint64)
        hops = np.empty(nq, np.uint32)
        fin = np.empty(nq, np.uint8)
        _check(lib.cpd_query_timed_fetch(self._h, _ptr(cost, u64p), _ptr(hops, u32p),
                                         _ptr(fin, u8p)))
        return cost, hops, fin

    def search(self, s, t, hscale=1.0, fscale=0.0, k_moves=-1, itrs=-1, time_ns=0,
               capacity=0, virtual_tick_ns=0, tables="auto", workspace_frac=0.0,
               capacity_max=0):
        """CPD-heuristic search (cpd_query_search) for queries (s, t):
        (cost, plen, finished, counters[nq, 5], stats); finished = 2: the
        search outgrew its workspace (after the capacity_max reruns)."""
        self.prepare(s, t)
        o = _search_opts(hscale, fscale, k_moves, itrs, time_ns, capacity, virtual_tick_ns,
                         tables, workspace_frac, capacity_max)
        st = SearchStats()
        _check(lib.cpd_query_search(self._h, C.byref(o), C.byref(st)))
        nq = len(s)
        cost = np.empty(nq, np.uint64)
        plen = np.empty(nq, np.uint32)
        fin = np.empty(nq, np.uint8)
        _check(lib.cpd_query_fetch(self._h, _ptr(cost, u64p), _ptr(plen, u32p), _ptr(fin, u8p)))
        cnt = np.empty((nq, 5), np.uint32)
        if nq:
            _check(lib.cpd_query_search_counters(self._h, _ptr(cnt, u32p)))
        return cost, plen, fin, cnt, {k: getattr(st, k) for k, _ in SearchStats._fields_}

    def search_paths(self, s, t, hscale=1.0, fscale=0.0, k_moves=-1, itrs=-1, time_ns=0,
                     capacity=0, virtual_tick_ns=0, tables="auto", workspace_frac=0.0,
                     capacity_max=0, prefix_bytes=0):
        """search() with the nodes of every route found (cpd_query_search_paths):
        (offsets u64[nq + 1], nodes u32[offsets[-1]], cost, plen, finished,
        counters[nq, 5], stats).  Path q is nodes[offsets[q]:offsets[q + 1]]:
        the A* tree's chain from s[q] to the incumbent's node, then the CPD
        walk from there to t[q]; no nodes when finished[q] != 1.  stats holds
        the search's and, under "paths", nodes / prefix_nodes / prefix_bytes /
        paths_ms.  prefix_bytes: the prefix pool's size (0 = automatic); too
        small raises CpdError(CPD_E_OOM) naming the bytes needed, with the
        search's results still fetchable (search_fetch)."""
        self.prepare(s, t)
        offsets, st = self.search_paths_run(hscale, fscale, k_moves, itrs, time_ns, capacity,
                                            virtual_tick_ns, tables, workspace_frac,
                                            capacity_max, prefix_bytes)
        nodes = self.paths_fetch(0, len(s))
        cost, plen, fin, cnt = self.search_fetch()
        return offsets, nodes, cost, plen, fin, cnt, st

    def search_paths_run(self, hscale=1.0, fscale=0.0, k_moves=-1, itrs=-1, time_ns=0,
                         capacity=0, virtual_tick_ns=0, tables="auto", workspace_frac=0.0,
                         capacity_max=0, prefix_bytes=0):
        """cpd_query_search_paths on the prepared queries: (offsets u64[nq + 1],
        stats).  The offsets are kept: paths_fetch sizes its buffers from them."""
        self._path_offsets = None
        o = _search_opts(hscale, fscale, k_moves, itrs, time_ns, capacity, virtual_tick_ns,
                         tables, workspace_frac, capacity_max)
        st = SearchStats()
        info = SearchPathsInfo()
        offsets = np.empty(self._nq + 1, np.uint64)
        _check(lib.cpd_query_search_paths(self._h, C.byref(o), C.c_uint64(int(prefix_bytes)),
                                          _ptr(offsets, u64p), C.byref(st), C.byref(info)))
        self._path_offsets = offsets.copy()
        d = {k: getattr(st, k) for k, _ in SearchStats._fields_}
        d["paths"] = {k: getattr(info, k) for k, _ in SearchPathsInfo._fields_}
        return offsets, d

    def search_loads(self, s, t, demand=None, accumulate: bool = False, prefix_bytes=0,
                     hscale=1.0, fscale=0.0, k_moves=-1, itrs=-1, time_ns=0, capacity=0,
                     virtual_tick_ns=0, tables="auto", workspace_frac=0.0, capacity_max=0):
        """search() with the demand every edge carries when the routes found
        are loaded (cpd_query_search_loads): (loads u64[1, m], cost, plen,
        finished, counters[nq, 5], stats).  demand: one u32 per query (None =
        1 each), added to loads[0, e] for every edge e (original index) of the
        route search_paths() returns for a query with finished == 1 — on the
        A* tree's chain the cheapest edge under the current weights between
        the two nodes (the first of equals), on the CPD walk the edge the
        row's move names.  accumulate=True adds to a resident one-plane table
        (loads(), earlier search_loads()).  stats holds the search's and,
        under "loads", moves / prefix_moves / prefix_nodes / prefix_bytes /
        loads_ms.  prefix_bytes as for search_paths(): too small raises
        CpdError(CPD_E_OOM) naming the bytes needed, the table untouched and
        the search's results still fetchable (search_fetch)."""
        self.prepare(s, t)
        st = self.search_loads_run(demand, accumulate, prefix_bytes, hscale, fscale, k_moves,
                                   itrs, time_ns, capacity, virtual_tick_ns, tables,
                                   workspace_frac, capacity_max)
        cost, plen, fin, cnt = self.search_fetch()
        return self.loads_fetch(), cost, plen, fin, cnt, st

    def search_loads_run(self, demand=None, accumulate: bool = False, prefix_bytes=0, hscale=1.0,
                         fscale=0.0, k_moves=-1, itrs=-1, time_ns=0, capacity=0,
                         virtual_tick_ns=0, tables="auto", workspace_frac=0.0, capacity_max=0,
                         flags=None):
        """cpd_query_search_loads on the prepared queries: stats (flags: the
        call's flag word, instead of the one accumulate gives)."""
        self._path_offsets = None
        d = self._demand(demand)
        o = _search_opts(hscale, fscale, k_moves, itrs, time_ns, capacity, virtual_tick_ns,
                         tables, workspace_frac, capacity_max)
        st = SearchStats()
        info = SearchLoadsInfo()
        if flags is None:
            flags = LOADS_ACCUMULATE if accumulate else 0
        _check(lib.cpd_query_search_loads(self._h, C.byref(o), C.c_uint64(int(prefix_bytes)),
                                          _ptr(d, u32p), C.c_uint32(flags), C.byref(st),
                                          C.byref(info)))
        self._load_slices = 1
        out = {k: getattr(st, k) for k, _ in SearchStats._fields_}
        out["loads"] = {k: getattr(info, k) for k, _ in SearchLoadsInfo._fields_}
        return out

    def search_fetch(self):
        """(cost, plen, finished, counters[nq, 5]) of the last search on the
        prepared queries (cpd_query_fetch + cpd_query_search_counters)."""
        nq = self._nq
        cost = np.empty(nq, np.uint64)
        plen = np.empty(nq, np.uint32)
        fin = np.empty(nq, np.uint8)
        _check(lib.cpd_query_fetch(self._h, _ptr(cost, u64p), _ptr(plen, u32p), _ptr(fin, u8p)))
        cnt = np.empty((nq, 5), np.uint32)
        if nq:
            _check(lib.cpd_query_search_counters(self._h, _ptr(cnt, u32p)))
        return cost, plen, fin, cnt

    def _capacity(self, capacity) -> np.ndarray:
        c = _u32(capacity)
        if c.shape != (self.graph.plan.info()["m"],):
            raise ValueError("capacity must have one entry per edge")
        return c

    def _demand(self, demand):
        if demand is None:
            return None
        d = _u32(demand)
        if d.shape != (self._nq,):
            raise ValueError("demand must have one entry per prepared query")
        return d

    def weights_from_loads(self, capacity, a=(3, 20), power: int = 4, load_div: int = 1) -> dict:
        """The resident load table turned into weights in HBM
        (cpd_index_weights_from_loads) by the delay function of cpd_api.h: w' =
        w0 + w0 * a * (x / c) ** power in integers, x = load // load_div,
        capacity c one u32 >= 1 per edge (original order).  A one-plane table
        rewrites the current weights (as set_weights(w') would), K >= 2 planes
        write weight set j from plane j.  Returns tstt (a Python int: the sum
        of x * w'), changed, planes, vdf_ms."""
        c = self._capacity(capacity)
        f = Vdf(int(a[0]), int(a[1]), int(power), int(load_div))
        info = VdfInfo()
        _check(lib.cpd_index_weights_from_loads(self._h, _ptr(c, u32p), C.byref(f),
                                                C.byref(info)))
        if info.planes >= 2:
            self._nsets = info.planes
        return {"tstt": _u128(info.tstt_lo, info.tstt_hi), "changed": info.changed,
                "planes": info.planes, "vdf_ms": info.vdf_ms}

    def get_weights(self) -> np.ndarray:
        """The current weights, u32[m] in original edge order
        (cpd_index_get_weights): free flow when none are set."""
        w = np.empty(self.graph.plan.info()["m"], np.uint32)
        _check(lib.cpd_index_get_weights(self._h, _ptr(w, u32p)))
        return w

    def get_weight_sets(self) -> np.ndarray:
        """The loaded weight sets, u32[nsets, m] (cpd_index_get_weight_sets)."""
        k = C.c_uint32()
        _check(lib.cpd_index_get_weight_sets(self._h, C.byref(k), None))
        w = np.empty((k.value, self.graph.plan.info()["m"]), np.uint32)
        if k.value:
            _check(lib.cpd_index_get_weight_sets(self._h, C.byref(k), _ptr(w, u32p)))
        return w

    def assign(self, s, t, capacity, iters: int, demand=None, a=(3, 20), power: int = 4,
               **search_opts):
        """The method of successive averages on the queries (s, t)
        (cpd_query_assign): `iters` rounds of search_loads under the current
        weights, then weights_from_loads of the mean loading.  Returns one dict
        per iteration: finished, sptt and tstt (Python ints), moves, changed,
        search_ms, loads_ms, vdf_ms.  Afterwards search_fetch() returns the
        last iteration's search, loads_fetch() the summed loadings and
        get_weights() the final weights.  search_opts: search_loads' keywords
        (hscale, fscale, ..., prefix_bytes)."""
        self.prepare(s, t)
        return self.assign_run(capacity, iters, demand, a, power, **search_opts)

    def assign_run(self, capacity, iters: int, demand=None, a=(3, 20), power: int = 4,
                   prefix_bytes=0, hscale=1.0, fscale=0.0, k_moves=-1, itrs=-1, time_ns=0,
                   capacity_cols=0, virtual_tick_ns=0, tables="auto", workspace_frac=0.0,
                   capacity_max=0):
        """cpd_query_assign on the prepared queries (capacity_cols: the
        search's `capacity` option, renamed beside the edge capacities)."""
        return self._assign_loop(lib.cpd_query_assign, AssignIter, False, (CPD_E_OOM,), capacity,
                                 iters, demand, a, power, prefix_bytes,
                                 (hscale, fscale, k_moves, itrs, time_ns, capacity_cols,
                                  virtual_tick_ns, tables, workspace_frac, capacity_max))

    def _assign_loop(self, entry, record_type, with_done, resident_codes, capacity, iters,
                     demand, a, power, prefix_bytes, search) -> list:
        """One of the three loops on the prepared queries: `entry` over records
        of `record_type`, one dict per record made (`with_done`: as many as the
        entry point reports; else min(iters, 65535)).  resident_codes: the
        errors after which, when they name an iteration, the completed
        iterations have left a loading resident.  search: _search_opts'
        arguments."""
        self._path_offsets = None
        c = self._capacity(capacity)
        d = self._demand(demand)
        o = _search_opts(*search)
        f = Vdf(int(a[0]), int(a[1]), int(power), 1)
        n = max(0, min(int(iters), 65535))
        out = (record_type * max(1, n))()
        done = C.c_uint32()
        rc = entry(self._h, C.byref(o), C.c_uint64(int(prefix_bytes)), _ptr(d, u32p),
                   _ptr(c, u32p), C.byref(f), C.c_uint32(int(iters) & 0xFFFFFFFF), out,
                   *([C.byref(done)] if with_done else []))
        if rc == CPD_OK or (rc in resident_codes
                            and "iteration" in lib.cpd_last_error().decode()):
            self._load_slices = 1  # a loading of the completed iterations is resident
        _check(rc)
        return [_iter_dict(r) for r in out[:done.value if with_done else n]]

    @staticmethod
    def _lambda(lam) -> int:
        return STEP_LINE if lam == "line" else int(lam) & 0xFFFFFFFF

    def flow_step(self, capacity, lam="line", a=(3, 20), power: int = 4) -> dict:
        """One flow step towards the resident one-plane load table
        (cpd_index_flow_step, cpd_api.h "The flow step"): lam = "line" for the
        line rule or a step in 0..65536 (Q16).  Without a flow table the step
        initialises it from the loads.  Returns lambda_q16, evals, g0 (a signed
        Python int), xw0 and tstt (Python ints), changed, line_ms, apply_ms;
        the relative gap before the step is -g0 / xw0."""
        c = self._capacity(capacity)
        f = Vdf(int(a[0]), int(a[1]), int(power), 1)
        info = FlowInfo()
        _check(lib.cpd_index_flow_step(self._h, _ptr(c, u32p), C.byref(f),
                                       C.c_uint32(self._lambda(lam)), C.byref(info)))
        return {"lambda_q16": info.lambda_q16, "evals": info.evals,
                "g0": _s128(info.g0_lo, info.g0_hi), "xw0": _u128(info.xw0_lo, info.xw0_hi),
                "tstt": _u128(info.tstt_lo, info.tstt_hi), "changed": info.changed,
                "line_ms": info.line_ms, "apply_ms": info.apply_ms}

    def flow_fetch(self) -> np.ndarray:
        """The flow table, u64[m] in original edge order, Q16
        (cpd_index_flow_fetch): the volume of edge e is flow[e] >> 16."""
        x = np.empty(self.graph.plan.info()["m"], np.uint64)
        _check(lib.cpd_index_flow_fetch(self._h, _ptr(x, u64p)))
        return x

    def flow_clear(self) -> None:
        """Drop the flow table (cpd_index_flow_clear)."""
        _check(lib.cpd_index_flow_clear(self._h))

    def assign_line(self, s, t, capacity, iters: int, demand=None, a=(3, 20), power: int = 4,
                    **search_opts):
        """assign() with the line-search step (cpd_query_assign_line): one dict
        per iteration made — the loop stops early after an iteration k >= 2
        with lambda 0 — holding assign()'s keys and lambda_q16, evals, g0
        (signed), xw0 and line_ms.  Afterwards flow_fetch() returns the flow,
        loads_fetch() the last loading and get_weights() the final weights."""
        self.prepare(s, t)
        return self.assign_line_run(capacity, iters, demand, a, power, **search_opts)

    def assign_line_run(self, capacity, iters: int, demand=None, a=(3, 20), power: int = 4,
                        prefix_bytes=0, hscale=1.0, fscale=0.0, k_moves=-1, itrs=-1, time_ns=0,
                        capacity_cols=0, virtual_tick_ns=0, tables="auto", workspace_frac=0.0,
                        capacity_max=0):
        """cpd_query_assign_line on the prepared queries (capacity_cols as in
        assign_run)."""
        return self._assign_loop(lib.cpd_query_assign_line, AssignLineIter, True,
                                 (CPD_E_OOM, CPD_E_RANGE), capacity, iters, demand, a, power,
                                 prefix_bytes,
                                 (hscale, fscale, k_moves, itrs, time_ns, capacity_cols,
                                  virtual_tick_ns, tables, workspace_frac, capacity_max))

    @staticmethod
    def _alpha(alpha) -> int:
        return ALPHA_CONJ if alpha == "conj" else int(alpha) & 0xFFFFFFFF

    def flow_step_conj(self, capacity, alpha="conj", lam="line", a=(3, 20), power: int = 4) -> dict:
        """One conjugate step towards the resident one-plane load table
        (cpd_index_flow_step_conj, cpd_api.h "The conjugate step"): alpha =
        "conj" for the rule or a value in 0..ALPHA_MAX (Q16), lam as
        flow_step's.  Returns alpha_q16, lambda_q16, evals, n, gy and g0
        (signed Python ints), m, xw0 and tstt (Python ints), changed, conj_ms,
        line_ms, apply_ms; the relative gap before the step is -gy / xw0."""
        c = self._capacity(capacity)
        f = Vdf(int(a[0]), int(a[1]), int(power), 1)
        info = ConjInfo()
        _check(lib.cpd_index_flow_step_conj(self._h, _ptr(c, u32p), C.byref(f),
                                            C.c_uint32(self._alpha(alpha)),
                                            C.c_uint32(self._lambda(lam)), C.byref(info)))
        return {"alpha_q16": info.alpha_q16, "lambda_q16": info.lambda_q16, "evals": info.evals,
                "n": _s128(info.n_lo, info.n_hi), "m": _u128(info.m_lo, info.m_hi),
                "gy": _s128(info.gy_lo, info.gy_hi), "xw0": _u128(info.xw0_lo, info.xw0_hi),
                "g0": _s128(info.g0_lo, info.g0_hi),
                "tstt": _u128(info.tstt_lo, info.tstt_hi), "changed": info.changed,
                "conj_ms": info.conj_ms, "line_ms": info.line_ms, "apply_ms": info.apply_ms}

    def target_fetch(self) -> np.ndarray:
        """The target table, u64[m] in original edge order, Q16
        (cpd_index_target_fetch): the point the last conjugate step aimed at."""
        x = np.empty(self.graph.plan.info()["m"], np.uint64)
        _check(lib.cpd_index_target_fetch(self._h, _ptr(x, u64p)))
        return x

    def assign_conj(self, s, t, capacity, iters: int, demand=None, a=(3, 20), power: int = 4,
                    **search_opts):
        """assign_line() with the conjugate step (cpd_query_assign_conj): one
        dict per iteration made, holding assign_line()'s keys (g0 along S - X)
        and alpha_q16, n, m, gy; the gap before step k is -gy / xw0.
        Afterwards target_fetch() returns the last target."""
        self.prepare(s, t)
        return self.assign_conj_run(capacity, iters, demand, a, power, **search_opts)

    def assign_conj_run(self, capacity, iters: int, demand=None, a=(3, 20), power: int = 4,
                        prefix_bytes=0, hscale=1.0, fscale=0.0, k_moves=-1, itrs=-1, time_ns=0,
                        capacity_cols=0, virtual_tick_ns=0, tables="auto", workspace_frac=0.0,
                        capacity_max=0):
        """cpd_query_assign_conj on the prepared queries (capacity_cols as in
        assign_run)."""
        return self._assign_loop(lib.cpd_query_assign_conj, AssignConjIter, True,
                                 (CPD_E_OOM, CPD_E_RANGE), capacity, iters, demand, a, power,
                                 prefix_bytes,
                                 (hscale, fscale, k_moves, itrs, time_ns, capacity_cols,
                                  virtual_tick_ns, tables, workspace_frac, capacity_max))

    @staticmethod
    def _bi(v) -> int:
        return BI_AUTO if v == "auto" else int(v) & 0xFFFFFFFF

    def flow_step_bi(self, capacity, mu="auto", nu="auto", lam="line", a=(3, 20),
                     power: int = 4) -> dict:
        """One bi-conjugate step towards the resident one-plane load table
        (cpd_index_flow_step_bi, cpd_api.h "The bi-conjugate step"): mu and nu
        = "auto" for the rules or values in 0..BI_MAX (Q16), lam as
        flow_step's.  Returns branch, mu_q16, nu_q16, beta0_q16..beta2_q16,
        alpha_q16, lambda_prev_q16, lambda_q16, evals, a1, a2, b2, gy and g0
        (signed Python ints), b1, xw0 and tstt (Python ints), changed, bi_ms,
        line_ms, apply_ms; the relative gap before the step is -gy / xw0."""
        c = self._capacity(capacity)
        f = Vdf(int(a[0]), int(a[1]), int(power), 1)
        info = BiInfo()
        _check(lib.cpd_index_flow_step_bi(self._h, _ptr(c, u32p), C.byref(f),
                                          C.c_uint32(self._bi(mu)), C.c_uint32(self._bi(nu)),
                                          C.c_uint32(self._lambda(lam)), C.byref(info)))
        d = {k: getattr(info, k) for k in ("branch", "mu_q16", "nu_q16", "beta0_q16", "beta1_q16",
                                           "beta2_q16", "alpha_q16", "lambda_prev_q16",
                                           "lambda_q16", "evals", "changed", "bi_ms", "line_ms",
                                           "apply_ms")}
        for k in ("a1", "a2", "b2", "gy", "g0"):
            d[k] = _s128(getattr(info, k + "_lo"), getattr(info, k + "_hi"))
        for k in ("b1", "xw0", "tstt"):
            d[k] = _u128(getattr(info, k + "_lo"), getattr(info, k + "_hi"))
        return d

    def target2_fetch(self) -> np.ndarray:
        """The second target table, u64[m] in original edge order, Q16
        (cpd_index_target2_fetch): the target before target_fetch()'s."""
        x = np.empty(self.graph.plan.info()["m"], np.uint64)
        _check(lib.cpd_index_target2_fetch(self._h, _ptr(x, u64p)))
        return x

    def assign_bi(self, s, t, capacity, iters: int, demand=None, a=(3, 20), power: int = 4,
                  **search_opts):
        """assign_conj() with the bi-conjugate step (cpd_query_assign_bi): one
        dict per iteration made, holding assign_line()'s keys (g0 along S1 - X)
        and branch, mu_q16, nu_q16, beta0_q16..beta2_q16, alpha_q16, a1, b1,
        a2, b2, gy; the gap before step k is -gy / xw0.  Afterwards
        target_fetch() and target2_fetch() return the last two targets."""
        self.prepare(s, t)
        return self.assign_bi_run(capacity, iters, demand, a, power, **search_opts)

    def assign_bi_run(self, capacity, iters: int, demand=None, a=(3, 20), power: int = 4,
                      prefix_bytes=0, hscale=1.0, fscale=0.0, k_moves=-1, itrs=-1, time_ns=0,
                      capacity_cols=0, virtual_tick_ns=0, tables="auto", workspace_frac=0.0,
                      capacity_max=0):
        """cpd_query_assign_bi on the prepared queries (capacity_cols as in
        assign_run)."""
        return self._assign_loop(lib.cpd_query_assign_bi, AssignBiIter, True,
                                 (CPD_E_OOM, CPD_E_RANGE), capacity, iters, demand, a, power,
                                 prefix_bytes,
                                 (hscale, fscale, k_moves, itrs, time_ns, capacity_cols,
                                  virtual_tick_ns, tables, workspace_frac, capacity_max))

    def __del__(self):
        if getattr(self, "_h", None):
            lib.cpd_index_free(self._h)
            self._h = None
