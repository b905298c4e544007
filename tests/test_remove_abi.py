"""CPU tests of the remove-by-id surface: the C ABI exports vdb_ivf_remove_ids, the Python
class and the C++ drop-in class carry the method, and a null handle is refused before any
device call (so it can be checked without a GPU)."""
import ctypes
import re
import subprocess

from conftest import load_vdb

vdb = load_vdb()


def test_library_exports_remove_ids():
    out = subprocess.check_output(["nm", "-D", "--defined-only", vdb.LIB_PATH], text=True)
    exported = set(re.findall(r" T (vdb_\w+)", out))
    assert "vdb_ivf_remove_ids" in exported
    assert "vdb_remove_last_timing" in exported
    assert "vdb_ivf_remove_ids" in open(vdb.HEADER).read()


def test_python_class_has_remove_ids():
    assert callable(getattr(vdb.IVFFlatIndex, "remove_ids", None))
    fn = vdb.lib().vdb_ivf_remove_ids
    assert fn.argtypes is not None and len(fn.argtypes) == 4


def test_null_handle_is_an_invalid_argument():
    L = vdb.lib()
    gone = ctypes.c_uint64(7)
    ids = (ctypes.c_uint64 * 2)(1, 2)
    assert L.vdb_ivf_remove_ids(None, ids, 2, ctypes.byref(gone)) == -1  # VDB_ERR_INVALID_ARGUMENT
    assert b"null" in L.vdb_last_error()
    assert L.vdb_ivf_remove_ids(None, None, 0, None) == -1


def test_cpp_class_exports_remove():
    out = subprocess.check_output(["nm", "-DC", "--defined-only", vdb.CPP_LIB_PATH], text=True)
    assert "vdb::IVFFlatIndex::remove(" in out
