"""CPU tests of the fetch-by-id surface: the C ABI exports vdb_ivf_fetch_ids,
vdb_ivf_fetch_ids_device, vdb_ivf_search_ids and vdb_fetch_last_timing, the Python class and the
C++ drop-in class carry the methods, and a null handle is refused before any device call (so it
can be checked without a GPU)."""
import ctypes
import re
import subprocess
import threading

from conftest import load_vdb

vdb = load_vdb()

SYMBOLS = ("vdb_ivf_fetch_ids", "vdb_ivf_fetch_ids_device", "vdb_ivf_search_ids", "vdb_fetch_last_timing")


def test_library_exports_fetch():
    out = subprocess.check_output(["nm", "-D", "--defined-only", vdb.LIB_PATH], text=True)
    exported = set(re.findall(r" T (vdb_\w+)", out))
    header = open(vdb.HEADER).read()
    for name in SYMBOLS:
        assert name in exported, name
        assert re.search(r"\b%s\(" % name, header), name


def test_python_class_has_fetch_and_search_ids():
    for name in ("fetch_ids", "fetch_ids_device", "search_ids", "fetch_last_timing"):
        assert callable(getattr(vdb.IVFFlatIndex, name, None)), name
    L = vdb.lib()
    assert L.vdb_ivf_fetch_ids.argtypes is not None and len(L.vdb_ivf_fetch_ids.argtypes) == 6
    assert L.vdb_ivf_fetch_ids_device.argtypes is not None and len(L.vdb_ivf_fetch_ids_device.argtypes) == 6
    assert L.vdb_ivf_search_ids.argtypes is not None and len(L.vdb_ivf_search_ids.argtypes) == 8
    assert L.vdb_fetch_last_timing.argtypes is not None and len(L.vdb_fetch_last_timing.argtypes) == 4


def test_null_handle_is_an_invalid_argument():
    L = vdb.lib()
    ids = (ctypes.c_uint64 * 2)(1, 2)
    vec = (ctypes.c_float * 8)()
    found = (ctypes.c_uint8 * 2)(9, 9)
    hits = ctypes.c_uint64(7)
    dist = (ctypes.c_float * 2)()
    out = (ctypes.c_uint64 * 2)()
    calls = (
        lambda: L.vdb_ivf_fetch_ids(None, ids, 2, vec, found, ctypes.byref(hits)),
        lambda: L.vdb_ivf_fetch_ids_device(None, ids, 2, vec, found, ctypes.byref(hits)),
        lambda: L.vdb_ivf_search_ids(None, ids, 2, 1, 1, dist, out, found),
    )
    for call in calls:
        L.vdb_ivf_remove_ids(None, None, 0, None)  # (some other error in between)
        assert call() == -1  # VDB_ERR_INVALID_ARGUMENT
        assert b"null" in L.vdb_last_error()
    assert hits.value == 7 and list(found) == [9, 9]  # nothing was written
    assert L.vdb_ivf_fetch_ids(None, None, 0, None, None, None) == -1


def test_last_timing_reads_zeros_without_a_call():
    a, b, c, r = ctypes.c_double(1), ctypes.c_double(1), ctypes.c_double(1), ctypes.c_uint64(1)
    rc = []
    t = threading.Thread(target=lambda: rc.append(  # (the record is per thread: a thread of its own has none)
        vdb.lib().vdb_fetch_last_timing(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(r))))
    t.start()
    t.join()
    assert rc == [0]
    assert (a.value, b.value, c.value, r.value) == (0.0, 0.0, 0.0, 0)
    assert vdb.lib().vdb_fetch_last_timing(None, None, None, None) == 0


def test_cpp_class_exports_fetch():
    out = subprocess.check_output(["nm", "-DC", "--defined-only", vdb.CPP_LIB_PATH], text=True)
    assert "vdb::IVFFlatIndex::fetch(" in out
    assert "vdb::IVFFlatIndex::search_by_ids(" in out
