"""CPU tests of the range-search surface: the C ABI exports vdb_ivf_range_search, the five
vdb_range_result_* accessors and vdb_range_last_timing, the header declares them, the Python
class and the C++ drop-in class carry the method, and a null handle is refused before any
device call (so it can be checked without a GPU)."""
import ctypes
import re
import subprocess
import threading

from conftest import load_vdb

vdb = load_vdb()

EXPORTS = ["vdb_ivf_range_search", "vdb_range_result_n", "vdb_range_result_lims", "vdb_range_result_distances",
           "vdb_range_result_ids", "vdb_range_result_free", "vdb_range_last_timing"]


def test_library_exports_range_search():
    out = subprocess.check_output(["nm", "-D", "--defined-only", vdb.LIB_PATH], text=True)
    exported = set(re.findall(r" T (vdb_\w+)", out))
    for name in EXPORTS:
        assert name in exported, name
    assert len(EXPORTS) == 7


def test_header_declares_all():
    header = open(vdb.HEADER).read()
    assert re.search(r"typedef struct vdb_range_result vdb_range_result;", header)
    assert re.search(r"int vdb_ivf_range_search\(vdb_ivf\* index, const float\* queries, uint32_t n, uint32_t nprobe, "
                     r"float radius,\s+uint64_t reserve, vdb_range_result\*\* out\);", header)
    assert re.search(r"uint32_t\s+vdb_range_result_n\(const vdb_range_result\* r\);", header)
    assert re.search(r"const uint64_t\*\s+vdb_range_result_lims\(const vdb_range_result\* r\);", header)
    assert re.search(r"const float\*\s+vdb_range_result_distances\(const vdb_range_result\* r\);", header)
    assert re.search(r"const uint64_t\*\s+vdb_range_result_ids\(const vdb_range_result\* r\);", header)
    assert re.search(r"void\s+vdb_range_result_free\(vdb_range_result\* r\);", header)
    assert re.search(r"int vdb_range_last_timing\(double\* scan_ms, double\* order_ms, uint64_t\* pairs_scanned, "
                     r"uint64_t\* hits,\s+uint32_t\* reruns\);", header)


def test_python_class_has_range_search():
    assert callable(getattr(vdb.IVFFlatIndex, "range_search", None))
    assert callable(getattr(vdb.IVFFlatIndex, "range_last_timing", None))
    L = vdb.lib()
    assert L.vdb_ivf_range_search.argtypes is not None and len(L.vdb_ivf_range_search.argtypes) == 7
    assert L.vdb_range_last_timing.argtypes is not None and len(L.vdb_range_last_timing.argtypes) == 5
    for name in EXPORTS[1:6]:
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == 1


def test_cpp_class_exports_range_search():
    out = subprocess.check_output(["nm", "-DC", "--defined-only", vdb.CPP_LIB_PATH], text=True)
    assert "vdb::IVFFlatIndex::range_search(" in out


def test_null_handle_is_an_invalid_argument():
    L = vdb.lib()
    q = (ctypes.c_float * 4)(0, 0, 0, 0)
    out = ctypes.c_void_p(0x1234)
    rc = L.vdb_ivf_range_search(None, q, 1, 1, 1.0, 0, ctypes.byref(out))
    assert rc == -1  # VDB_ERR_INVALID_ARGUMENT
    assert b"null" in L.vdb_last_error()
    assert out.value == 0x1234  # written only on success


def test_free_of_null_returns():
    L = vdb.lib()
    L.vdb_range_result_free(None)
    assert L.vdb_range_result_n(None) == 0


def test_last_timing_of_a_thread_without_a_call_is_zero():
    L = vdb.lib()
    got = []

    def fresh():
        a, b = ctypes.c_double(1), ctypes.c_double(1)
        p, h, r = ctypes.c_uint64(1), ctypes.c_uint64(1), ctypes.c_uint32(1)
        rc = L.vdb_range_last_timing(ctypes.byref(a), ctypes.byref(b), ctypes.byref(p), ctypes.byref(h),
                                     ctypes.byref(r))
        got.append((rc, a.value, b.value, p.value, h.value, r.value))
        got.append(L.vdb_range_last_timing(None, None, None, None, None))

    t = threading.Thread(target=fresh)
    t.start()
    t.join()
    assert got == [(0, 0.0, 0.0, 0, 0, 0), 0]
