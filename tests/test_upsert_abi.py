"""CPU tests of the upsert surface: the C ABI exports vdb_ivf_upsert, vdb_ivf_upsert_device and
vdb_upsert_last_timing, the Python class and the C++ drop-in class carry the methods, and a null
handle is refused before any device call (so it can be checked without a GPU)."""
import ctypes
import re
import subprocess
import threading

from conftest import load_vdb

vdb = load_vdb()

SYMBOLS = ("vdb_ivf_upsert", "vdb_ivf_upsert_device", "vdb_upsert_last_timing")


def test_library_exports_upsert():
    out = subprocess.check_output(["nm", "-D", "--defined-only", vdb.LIB_PATH], text=True)
    exported = set(re.findall(r" T (vdb_\w+)", out))
    header = open(vdb.HEADER).read()
    for name in SYMBOLS:
        assert name in exported, name
        assert re.search(r"\b%s\(" % name, header), name


def test_python_class_has_upsert():
    for name in ("upsert", "upsert_device", "upsert_last_timing"):
        assert callable(getattr(vdb.IVFFlatIndex, name, None)), name
    L = vdb.lib()
    assert L.vdb_ivf_upsert.argtypes is not None and len(L.vdb_ivf_upsert.argtypes) == 6
    assert L.vdb_ivf_upsert_device.argtypes is not None and len(L.vdb_ivf_upsert_device.argtypes) == 6
    assert L.vdb_upsert_last_timing.argtypes is not None and len(L.vdb_upsert_last_timing.argtypes) == 6


def test_null_handle_is_an_invalid_argument():
    L = vdb.lib()
    ids = (ctypes.c_uint64 * 2)(1, 2)
    vec = (ctypes.c_float * 8)()
    r, w = ctypes.c_uint64(7), ctypes.c_uint64(7)
    for fn in (L.vdb_ivf_upsert, L.vdb_ivf_upsert_device):
        L.vdb_ivf_get_list(None, 0, None, None)  # (some other error in between)
        assert fn(None, vec, ids, 2, ctypes.byref(r), ctypes.byref(w)) == -1  # VDB_ERR_INVALID_ARGUMENT
        assert b"null" in L.vdb_last_error()
        assert fn(None, None, None, 0, None, None) == -1
    assert (r.value, w.value) == (7, 7)  # nothing was written


def test_last_timing_reads_zeros_without_a_call():
    d = [ctypes.c_double(1) for _ in range(4)]
    u = [ctypes.c_uint64(1) for _ in range(2)]
    rc = []
    t = threading.Thread(target=lambda: rc.append(  # (the record is per thread: a thread of its own has none)
        vdb.lib().vdb_upsert_last_timing(*[ctypes.byref(x) for x in d + u])))
    t.start()
    t.join()
    assert rc == [0]
    assert [x.value for x in d] == [0.0] * 4 and [x.value for x in u] == [0, 0]
    assert vdb.lib().vdb_upsert_last_timing(None, None, None, None, None, None) == 0


def test_cpp_class_exports_upsert():
    out = subprocess.check_output(["nm", "-DC", "--defined-only", vdb.CPP_LIB_PATH], text=True)
    assert "vdb::IVFFlatIndex::upsert(" in out
