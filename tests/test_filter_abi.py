"""CPU tests of the filtered-search surface: the C ABI exports vdb_ivf_search_filtered and
vdb_filter_last_timing, the header declares them, the Python class and the C++ drop-in class
carry the method, and a null handle is refused before any device call (so it can be checked
without a GPU)."""
import ctypes
import re
import subprocess

from conftest import load_vdb

vdb = load_vdb()


def test_library_exports_search_filtered():
    out = subprocess.check_output(["nm", "-D", "--defined-only", vdb.LIB_PATH], text=True)
    exported = set(re.findall(r" T (vdb_\w+)", out))
    assert "vdb_ivf_search_filtered" in exported
    assert "vdb_filter_last_timing" in exported


def test_header_declares_both():
    header = open(vdb.HEADER).read()
    assert re.search(r"int vdb_ivf_search_filtered\(vdb_ivf\* index, const float\* queries, uint32_t n, "
                     r"uint32_t nprobe, uint32_t k,\s+const uint64_t\* filter_ids, uint64_t n_filter, int mode,"
                     r"\s+float\* distances, uint64_t\* ids\);", header)
    assert re.search(r"int vdb_filter_last_timing\(double\* mark_ms, double\* scan_ms, double\* merge_ms, "
                     r"uint64_t\* pairs_scanned\);", header)
    assert re.search(r"enum \{ VDB_FILTER_EXCLUDE = 0, VDB_FILTER_INCLUDE = 1 \};", header)


def test_python_class_has_search_filtered():
    assert callable(getattr(vdb.IVFFlatIndex, "search_filtered", None))
    assert callable(getattr(vdb.IVFFlatIndex, "filter_last_timing", None))
    fn = vdb.lib().vdb_ivf_search_filtered
    assert fn.argtypes is not None and len(fn.argtypes) == 10


def test_null_handle_is_an_invalid_argument():
    L = vdb.lib()
    ids = (ctypes.c_uint64 * 2)(1, 2)
    assert L.vdb_ivf_search_filtered(None, None, 0, 1, 1, ids, 2, 0, None, None) == -1  # VDB_ERR_INVALID_ARGUMENT
    assert b"null" in L.vdb_last_error()


def test_last_timing_of_a_thread_without_a_call_is_zero():
    L = vdb.lib()
    a, b, c, r = ctypes.c_double(1), ctypes.c_double(1), ctypes.c_double(1), ctypes.c_uint64(1)
    assert L.vdb_filter_last_timing(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(r)) == 0
    assert (a.value, b.value, c.value, r.value) == (0.0, 0.0, 0.0, 0)
    assert L.vdb_filter_last_timing(None, None, None, None) == 0


def test_cpp_class_exports_search_filtered():
    out = subprocess.check_output(["nm", "-DC", "--defined-only", vdb.CPP_LIB_PATH], text=True)
    assert "vdb::IVFFlatIndex::search_filtered(" in out
