"""CPU tests of the screened exhaustive search's surface: the C ABI exports, the Python keywords and
timing method, the C++ drop-in method, a null handle refused before any device call, zero timing on
a fresh thread, and the g++ test of the host-only routing header
(tests/cpp/exhaustive_screen_route_test.cpp)."""
import ctypes
import inspect
import os
import re
import subprocess
import threading

from conftest import load_vdb

vdb = load_vdb()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_and_methods():
    out = subprocess.check_output(["nm", "-D", "--defined-only", vdb.LIB_PATH], text=True)
    exported = set(re.findall(r" T (vdb_\w+)", out))
    assert {"vdb_ivf_search_exhaustive_screened", "vdb_exhaustive_screen_last_timing"} <= exported
    cpp = subprocess.check_output(["nm", "-DC", "--defined-only", vdb.CPP_LIB_PATH], text=True)
    assert "vdb::IVFFlatIndex::search_exhaustive_screened(" in cpp
    params = inspect.signature(vdb.IVFFlatIndex.search_exhaustive).parameters
    assert params["k"].default == 10
    assert params["screen"].default is False and params["screen"].kind is inspect.Parameter.KEYWORD_ONLY
    assert params["reserve"].default == 0 and params["reserve"].kind is inspect.Parameter.KEYWORD_ONLY
    assert callable(getattr(vdb.IVFFlatIndex, "exhaustive_screen_last_timing", None))
    L = vdb.lib()
    assert len(L.vdb_ivf_search_exhaustive_screened.argtypes) == 7
    assert len(L.vdb_exhaustive_screen_last_timing.argtypes) == 8


def test_null_handle_is_refused_and_a_fresh_thread_reads_zeros():
    L = vdb.lib()
    q = (ctypes.c_float * 4)(0, 0, 0, 0)
    d = (ctypes.c_float * 1)(7.0)
    i = (ctypes.c_uint64 * 1)(7)
    assert L.vdb_ivf_search_exhaustive_screened(None, q, 1, 1, 0, d, i) == -1  # VDB_ERR_INVALID_ARGUMENT
    assert b"null" in L.vdb_last_error()
    assert d[0] == 7.0 and i[0] == 7  # the outputs are not written
    got = []

    def fresh():
        t = [ctypes.c_double(1) for _ in range(4)] + [ctypes.c_uint64(1), ctypes.c_uint64(1), ctypes.c_uint32(1),
                                                      ctypes.c_uint32(1)]
        got.append(L.vdb_exhaustive_screen_last_timing(*[ctypes.byref(x) for x in t]))
        got.append([x.value for x in t])
        got.append(L.vdb_exhaustive_screen_last_timing(*[None] * 8))

    th = threading.Thread(target=fresh)
    th.start()
    th.join()
    assert got == [0, [0.0] * 4 + [0] * 4, 0]


def test_route_header(tmp_path):
    """exhaustive_screen_route.hpp is host-only (plain g++) and its rules are the hand-derived ones."""
    exe = tmp_path / "exhaustive_screen_route_test"
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-std=c++17", "-Wall", "-Werror", "-o",
                           str(exe), os.path.join(ROOT, "tests", "cpp", "exhaustive_screen_route_test.cpp")])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout
