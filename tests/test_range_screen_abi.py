"""CPU tests of the screened range search's surface: the C ABI exports
vdb_ivf_range_search_screened and vdb_range_screen_last_timing, the header declares them, the
Python class carries the `screen` keyword and the timing method, the C++ drop-in class carries
range_search_screened, and a null handle is refused before any device call (so it can be checked
without a GPU)."""
import ctypes
import inspect
import re
import subprocess
import threading

from conftest import load_vdb

vdb = load_vdb()

EXPORTS = ["vdb_ivf_range_search_screened", "vdb_range_screen_last_timing"]


def test_library_exports_both():
    out = subprocess.check_output(["nm", "-D", "--defined-only", vdb.LIB_PATH], text=True)
    exported = set(re.findall(r" T (vdb_\w+)", out))
    for name in EXPORTS:
        assert name in exported, name


def test_header_declares_both():
    header = open(vdb.HEADER).read()
    assert re.search(r"int vdb_ivf_range_search_screened\(vdb_ivf\* index, const vdb_filter\* filter, "
                     r"const float\* queries, uint32_t n,\s+uint32_t nprobe, float radius, uint64_t reserve, "
                     r"vdb_range_result\*\* out\);", header)
    assert re.search(r"int vdb_range_screen_last_timing\(double\* pairs_ms, double\* bound_ms, double\* recheck_ms, "
                     r"uint64_t\* pairs_bounded,\s+uint64_t\* candidates, uint32_t\* screened_batches, "
                     r"uint32_t\* exact_batches\);", header)
    assert "Not offered yet: a screened range scan" not in header


def test_python_class_has_the_keyword_and_the_timing():
    for name in ("range_search", "range_search_prepared"):
        p = inspect.signature(getattr(vdb.IVFFlatIndex, name)).parameters["screen"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY, name
    assert callable(getattr(vdb.IVFFlatIndex, "range_screen_last_timing", None))
    L = vdb.lib()
    assert L.vdb_ivf_range_search_screened.argtypes is not None and len(L.vdb_ivf_range_search_screened.argtypes) == 8
    assert L.vdb_range_screen_last_timing.argtypes is not None and len(L.vdb_range_screen_last_timing.argtypes) == 7


def test_cpp_class_exports_range_search_screened():
    out = subprocess.check_output(["nm", "-DC", "--defined-only", vdb.CPP_LIB_PATH], text=True)
    assert "vdb::IVFFlatIndex::range_search_screened(" in out


def test_null_handle_is_an_invalid_argument():
    L = vdb.lib()
    q = (ctypes.c_float * 4)(0, 0, 0, 0)
    out = ctypes.c_void_p(0x1234)
    rc = L.vdb_ivf_range_search_screened(None, None, q, 1, 1, 1.0, 0, ctypes.byref(out))
    assert rc == -1  # VDB_ERR_INVALID_ARGUMENT
    assert b"null" in L.vdb_last_error()
    assert out.value == 0x1234  # written only on success


def test_timing_of_a_thread_without_a_call_is_zero():
    L = vdb.lib()
    got = []

    def fresh():
        a, b, c = ctypes.c_double(1), ctypes.c_double(1), ctypes.c_double(1)
        p, m = ctypes.c_uint64(1), ctypes.c_uint64(1)
        s, e = ctypes.c_uint32(1), ctypes.c_uint32(1)
        rc = L.vdb_range_screen_last_timing(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(p),
                                            ctypes.byref(m), ctypes.byref(s), ctypes.byref(e))
        got.append((rc, a.value, b.value, c.value, p.value, m.value, s.value, e.value))
        got.append(L.vdb_range_screen_last_timing(None, None, None, None, None, None, None))

    t = threading.Thread(target=fresh)
    t.start()
    t.join()
    assert got == [(0, 0.0, 0.0, 0.0, 0, 0, 0, 0), 0]
