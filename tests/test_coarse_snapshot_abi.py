"""CPU tests of the coarse snapshot's surface: the C ABI exports vdb_ivf_coarse_snapshot, the
header declares it, the Python class carries coarse_snapshot(), the build id is computed from
sources that do not include it, and a null handle or null rows are refused before any device call
(so it can be checked without a GPU)."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import load_vdb

vdb = load_vdb()


def test_library_exports_coarse_snapshot():
    out = subprocess.check_output(["nm", "-D", "--defined-only", vdb.LIB_PATH], text=True)
    assert "vdb_ivf_coarse_snapshot" in set(re.findall(r" T (vdb_\w+)", out))


def test_header_declares_it():
    header = open(vdb.HEADER).read()
    assert re.search(r"int vdb_ivf_coarse_snapshot\(vdb_ivf\* index, const float\* rows, uint32_t n, uint32_t nprobe,\s+"
                     r"float\* approx, float\* delta, uint32_t\* cand, uint32_t\* probes, uint32_t\* assign\);", header)
    assert "Diagnostics: the coarse step's buffers" in header


def test_python_class_has_coarse_snapshot():
    assert callable(getattr(vdb.IVFFlatIndex, "coarse_snapshot", None))
    fn = vdb.lib().vdb_ivf_coarse_snapshot
    assert fn.restype is ctypes.c_int
    assert fn.argtypes is not None and len(fn.argtypes) == 9
    assert fn.argtypes[2] is ctypes.c_uint32 and fn.argtypes[3] is ctypes.c_uint32


def test_its_source_is_outside_the_build_id():
    mk = open(os.path.join(os.path.dirname(vdb.LIB_PATH), "..", "Makefile")).read()
    id_srcs = re.search(r"^ID_SRCS = (.*)$", mk, re.M).group(1)
    assert "coarse_probe" not in id_srcs
    assert re.search(r"^\$\(BUILD\)/coarse_probe\.o: \$\(HERE\)csrc/coarse_probe\.cpp", mk, re.M)
    assert "$(BUILD)/coarse_probe.o" in re.search(r"^OBJS = ((?:.*\\\n)*.*)$", mk, re.M).group(1)


def test_null_handle_and_null_rows_are_invalid_arguments():
    L = vdb.lib()
    rows = np.zeros((2, 8), np.float32)
    out = np.full(16, 7, np.uint32)
    p = out.ctypes.data_as(ctypes.c_void_p)
    assert L.vdb_ivf_coarse_snapshot(None, rows.ctypes.data_as(ctypes.c_void_p), 2, 1, None, None, p, p, p) == -1
    assert b"null handle" in L.vdb_last_error()  # VDB_ERR_INVALID_ARGUMENT
    assert L.vdb_ivf_coarse_snapshot(None, None, 2, 0, None, None, None, None, None) == -1
    assert b"null" in L.vdb_last_error()
    assert (out == 7).all()  # (nothing written on a refusal)
