"""CPU tests of the exhaustive-search surface: the C ABI exports vdb_ivf_search_exhaustive and
vdb_exhaustive_last_timing, the Python class and the C++ drop-in class carry the method, and a
null handle is refused before any device call (so it can be checked without a GPU)."""
import ctypes
import re
import subprocess

from conftest import load_vdb

vdb = load_vdb()


def test_library_exports_search_exhaustive():
    out = subprocess.check_output(["nm", "-D", "--defined-only", vdb.LIB_PATH], text=True)
    exported = set(re.findall(r" T (vdb_\w+)", out))
    assert "vdb_ivf_search_exhaustive" in exported
    assert "vdb_exhaustive_last_timing" in exported
    assert callable(getattr(vdb.IVFFlatIndex, "search_exhaustive", None))
    assert callable(getattr(vdb.IVFFlatIndex, "exhaustive_last_timing", None))


def test_cpp_class_exports_search_exhaustive():
    out = subprocess.check_output(["nm", "-DC", "--defined-only", vdb.CPP_LIB_PATH], text=True)
    assert "vdb::IVFFlatIndex::search_exhaustive(" in out


def test_null_handle_is_an_invalid_argument():
    L = vdb.lib()
    assert L.vdb_ivf_search_exhaustive(None, None, 0, 1, None, None) == -1  # VDB_ERR_INVALID_ARGUMENT
    assert b"null" in L.vdb_last_error()


def test_last_timing_of_a_thread_without_a_call_is_zero():
    L = vdb.lib()
    a, b, r, p = ctypes.c_double(1), ctypes.c_double(1), ctypes.c_uint64(1), ctypes.c_uint64(1)
    assert L.vdb_exhaustive_last_timing(ctypes.byref(a), ctypes.byref(b), ctypes.byref(r), ctypes.byref(p)) == 0
    assert (a.value, b.value, r.value, p.value) == (0.0, 0.0, 0, 0)
    assert L.vdb_exhaustive_last_timing(None, None, None, None) == 0
