"""Path extraction's interface, without a GPU: the header declares it, libcpd.so
exports it, cpd.Index mirrors it, and what it needs fails loudly (CPD_E_HIP)
when there is no device."""
import ctypes as C
import os
import re

import pytest

import cpd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cpd_query_paths", "cpd_query_paths_fetch")


def test_header_declares_paths_entry_points():
    hdr = open(os.path.join(ROOT, "include", "cpd_api.h")).read()
    declared = set(re.findall(r"\b(cpd_[a-z_]+)\s*\(", hdr))
    assert set(NAMES) <= declared
    # the header says that a search's paths are not what this returns
    assert re.search(r"cpd_query_search\s+are\s+NOT", hdr)


def test_python_mirror_has_paths():
    assert callable(cpd.Index.paths) and callable(cpd.Index.paths_fetch)
    for name in NAMES:
        assert name in cpd.EXPORTED and hasattr(cpd.lib, name)


def test_library_exports_paths_symbols():
    so = C.CDLL(cpd.LIB_PATH)  # dlsym on the shared library itself
    for name in NAMES:
        assert getattr(so, name, None) is not None, name


def test_paths_need_a_device():
    if cpd.device_count() > 0:
        pytest.skip("a GPU is present")
    g = cpd.synth_road_graph(5, 5, seed=1)
    with pytest.raises(cpd.CpdError) as e:  # the graph an index for paths() lives on
        cpd.Graph(cpd.Plan(g, hierarchy=False))
    assert e.value.code == cpd.CPD_E_HIP and "no CPU fallback" in str(e.value)
