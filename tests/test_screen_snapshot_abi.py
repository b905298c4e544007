"""CPU tests of the screen snapshot's surface: the C ABI exports vdb_ivf_screen_snapshot, the
header declares it, the Python class carries screen_snapshot(), and null or unknown names and a
null handle are refused before any device call (so it can be checked without a GPU)."""
import ctypes
import re
import subprocess

from conftest import load_vdb

vdb = load_vdb()


def test_library_exports_screen_snapshot():
    out = subprocess.check_output(["nm", "-D", "--defined-only", vdb.LIB_PATH], text=True)
    assert "vdb_ivf_screen_snapshot" in set(re.findall(r" T (vdb_\w+)", out))


def test_header_declares_it():
    header = open(vdb.HEADER).read()
    assert re.search(r"int vdb_ivf_screen_snapshot\(vdb_ivf\* index, const char\* name, void\* out, "
                     r"uint64_t cap_bytes, uint64_t\* bytes\);", header)


def test_python_class_has_screen_snapshot():
    assert callable(getattr(vdb.IVFFlatIndex, "screen_snapshot", None))
    fn = vdb.lib().vdb_ivf_screen_snapshot
    assert fn.argtypes is not None and len(fn.argtypes) == 5
    # every per-batch and per-handle buffer the contract checker reads has a dtype
    for name in ("probes", "sorted_pair", "counters", "cand", "ovf", "thr", "thr4", "ublist", "ubcnt", "scnt", "soff",
                 "surv", "pst", "qscale", "qres", "block_off", "count", "meta", "sscale", "shadow"):
        assert name in vdb.IVFFlatIndex._SNAPSHOT
    assert vdb.IVFFlatIndex._SNAPSHOT_SCALARS[:10] == ("B", "P", "k", "dp", "seg_blocks", "segs_item", "wide_q",
                                                       "cand_cap", "i8", "metric")


def test_null_and_unknown_names_are_invalid_arguments():
    L = vdb.lib()
    n = ctypes.c_uint64(7)
    assert L.vdb_ivf_screen_snapshot(None, None, None, 0, ctypes.byref(n)) == -1  # VDB_ERR_INVALID_ARGUMENT
    assert b"null" in L.vdb_last_error()
    assert L.vdb_ivf_screen_snapshot(None, b"cand", None, 0, None) == -1
    assert b"null" in L.vdb_last_error()
    assert L.vdb_ivf_screen_snapshot(None, b"no_such_buffer", None, 0, ctypes.byref(n)) == -1
    assert b"unknown snapshot buffer no_such_buffer" in L.vdb_last_error()
    assert L.vdb_ivf_screen_snapshot(None, b"cand", None, 0, ctypes.byref(n)) == -1
    assert b"null handle" in L.vdb_last_error()
    assert n.value == 7  # (nothing written on a refusal)
