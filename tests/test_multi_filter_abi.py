"""CPU tests of the per-query prepared-filter surface (vdb_ivf_search_prepared_multi): the C ABI
exports the call, the header declares it, the Python class and the C++ drop-in class carry it,
and every null or out-of-range argument is refused before any device call, so all of it can be
checked without a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import load_vdb

vdb = load_vdb()

INVALID = -1  # VDB_ERR_INVALID_ARGUMENT


def test_library_exports_the_call():
    out = subprocess.check_output(["nm", "-D", "--defined-only", vdb.LIB_PATH], text=True)
    assert "vdb_ivf_search_prepared_multi" in set(re.findall(r" T (vdb_\w+)", out))


def test_header_declares_it():
    header = re.sub(r"\s+", " ", open(vdb.HEADER).read())
    decl = ("int vdb_ivf_search_prepared_multi(vdb_ivf* index, const vdb_filter* const* filters, uint32_t n_filters, "
            "const uint32_t* filter_of, const float* queries, uint32_t n, uint32_t nprobe, uint32_t k, "
            "float* distances, uint64_t* ids);")
    assert decl in header
    # the filtered and the prepared calls point to it where they speak of coalescing
    header = header.replace(" * ", " ")  # (the comment's line starts)
    assert len(re.findall(r"coalescing of concurrent (?:filtered|prepared) calls[^.]*vdb_ivf_search_prepared_multi",
                          header)) == 2
    # the contract
    for words in ("scattered back into request order", "never crosses filters", "a null entry of filters[]",
                  "a filter_of[i] >= n_filters", "a device-pointer variant"):
        assert words in header, words


def test_python_surface():
    assert callable(getattr(vdb.IVFFlatIndex, "search_prepared_multi", None))
    L = vdb.lib()
    assert len(L.vdb_ivf_search_prepared_multi.argtypes) == 10
    assert L.vdb_ivf_search_prepared_multi.restype is ctypes.c_int


def test_cpp_class_declares_and_exports_the_method():
    header = re.sub(r"\s+", " ", open(os.path.join(os.path.dirname(vdb.HEADER), "vdb", "ivf_flat_index.h")).read())
    assert ("void search_prepared_multi(const float* queries, uint32_t n_queries, const SearchParams& params, "
            "const Filter* const* filters, uint32_t n_filters, const uint32_t* filter_of, float* distances, "
            "uint64_t* indices);") in header
    out = subprocess.check_output(["nm", "-DC", "--defined-only", vdb.CPP_LIB_PATH], text=True)
    assert "vdb::IVFFlatIndex::search_prepared_multi(" in out


def test_null_and_out_of_range_arguments_are_refused_before_any_device_call():
    L = vdb.lib()
    call = L.vdb_ivf_search_prepared_multi
    fake = ctypes.c_void_p(0x1000)  # (never dereferenced: the argument checks come first)
    q = np.zeros((2, 4), np.float32)
    D = np.full((2, 3), 7.0, np.float32)
    I = np.full((2, 3), 7, np.uint64)
    fo = np.array([0, 1], np.uint32)
    tab = (ctypes.c_void_p * 2)(0x2000, 0x3000)
    vp = ctypes.c_void_p
    P = lambda a: vp(a.ctypes.data)  # noqa: E731
    good = dict(h=fake, filters=tab, nf=2, fo=P(fo), q=P(q), n=2, nprobe=1, k=3, D=P(D), I=P(I))

    def refused(text, **kw):
        a = dict(good, **kw)
        rc = call(a["h"], a["filters"], a["nf"], a["fo"], a["q"], a["n"], a["nprobe"], a["k"], a["D"], a["I"])
        assert rc == INVALID, kw
        assert text in L.vdb_last_error(), (kw, L.vdb_last_error())

    refused(b"null", h=None)
    refused(b"null", q=None)
    refused(b"null", D=None)
    refused(b"null", I=None)
    refused(b"null", filters=None)
    refused(b"null", fo=None)
    refused(b"n_filters", nf=0)
    refused(b"null entry", filters=(ctypes.c_void_p * 2)(0x2000, None))
    refused(b"null entry", filters=(ctypes.c_void_p * 2)(None, 0x3000))
    refused(b"out of range", fo=P(np.array([0, 2], np.uint32)))
    refused(b"out of range", fo=P(np.array([0xFFFFFFFF, 0], np.uint32)))
    refused(b"out of range", nf=1)  # (filter_of[1] == 1)
    refused(b"null", h=None, n=0)  # a null handle is refused whatever n is
    # no output was written
    assert np.all(D == 7.0) and np.all(I == 7)


def test_n_zero_succeeds_and_touches_nothing():
    L = vdb.lib()
    fake = ctypes.c_void_p(0x1000)
    assert L.vdb_ivf_search_prepared_multi(fake, None, 0, None, None, 0, 1, 1, None, None) == 0
    tab = (ctypes.c_void_p * 1)(0x2000)
    assert L.vdb_ivf_search_prepared_multi(fake, tab, 1, None, None, 0, 5, 10, None, None) == 0
