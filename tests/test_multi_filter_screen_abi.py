"""CPU tests of the surface of per-query prepared filters through the screen
(vdb_ivf_search_prepared_multi_screened): the C ABI export, the header declaration, the Python
keywords, the C++ drop-in method, and a null handle, a null `filters` and a null `filter_of`
refused before any device call with the outputs not written."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np

from conftest import load_vdb

vdb = load_vdb()


def test_exports_and_declarations():
    out = subprocess.check_output(["nm", "-D", "--defined-only", vdb.LIB_PATH], text=True)
    assert "vdb_ivf_search_prepared_multi_screened" in set(re.findall(r" T (vdb_\w+)", out))
    header = re.sub(r"\s+", " ", open(vdb.HEADER).read())
    assert ("int vdb_ivf_search_prepared_multi_screened(vdb_ivf* index, const vdb_filter* const* filters, "
            "uint32_t n_filters, const uint32_t* filter_of, const float* queries, uint32_t n, uint32_t nprobe, "
            "uint32_t k, uint64_t reserve, float* distances, uint64_t* ids);") in header
    cpp_header = re.sub(r"\s+", " ", open(os.path.join(os.path.dirname(vdb.HEADER), "vdb", "ivf_flat_index.h")).read())
    assert ("void search_prepared_multi_screened(const float* queries, uint32_t n_queries, const SearchParams& params, "
            "const Filter* const* filters, uint32_t n_filters, const uint32_t* filter_of, float* distances, "
            "uint64_t* indices, uint64_t reserve = 0);") in cpp_header
    cpp = subprocess.check_output(["nm", "-DC", "--defined-only", vdb.CPP_LIB_PATH], text=True)
    assert "vdb::IVFFlatIndex::search_prepared_multi_screened(" in cpp


def test_python_keywords():
    params = inspect.signature(vdb.IVFFlatIndex.search_prepared_multi).parameters
    assert params["screen"].default is False and params["screen"].kind is inspect.Parameter.KEYWORD_ONLY
    assert params["reserve"].default == 0 and params["reserve"].kind is inspect.Parameter.KEYWORD_ONLY
    call = vdb.lib().vdb_ivf_search_prepared_multi_screened
    assert len(call.argtypes) == 11 and call.restype is ctypes.c_int


def test_null_arguments_are_refused_before_any_device_call():
    L = vdb.lib()
    fake = ctypes.c_void_p(0x1000)  # (never dereferenced: the argument checks come first)
    q = np.zeros((2, 4), np.float32)
    D, I = np.full((2, 3), 7.0, np.float32), np.full((2, 3), 7, np.uint64)
    fo = np.array([0, 1], np.uint32)
    tab = (ctypes.c_void_p * 2)(0x2000, 0x3000)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    good = dict(h=fake, filters=tab, fo=P(fo))
    for bad in ("h", "filters", "fo"):
        a = dict(good, **{bad: None})
        assert L.vdb_ivf_search_prepared_multi_screened(a["h"], a["filters"], 2, a["fo"], P(q), 2, 1, 3, 0, P(D),
                                                        P(I)) == -1, bad  # VDB_ERR_INVALID_ARGUMENT
        assert b"null" in L.vdb_last_error(), bad
    assert np.all(D == 7.0) and np.all(I == 7)  # the outputs are not written
