"""CPU tests of the prepared-filter surface: the C ABI exports the calls, the header declares
them, the Python class and the C++ drop-in class carry them, and null arguments are refused (or,
for free and stale, accepted) before any device call, so they can be checked without a GPU."""
import ctypes
import re
import subprocess

from conftest import load_vdb

vdb = load_vdb()

EXPORTS = ["vdb_ivf_filter_create", "vdb_ivf_filter_create_device", "vdb_filter_combine", "vdb_filter_allowed",
           "vdb_filter_stale", "vdb_filter_free", "vdb_ivf_search_prepared", "vdb_ivf_range_search_prepared",
           "vdb_filter_create_last_timing"]
INVALID = -1  # VDB_ERR_INVALID_ARGUMENT


def test_library_exports_the_prepared_calls():
    out = subprocess.check_output(["nm", "-D", "--defined-only", vdb.LIB_PATH], text=True)
    exported = set(re.findall(r" T (vdb_\w+)", out))
    for name in EXPORTS:
        assert name in exported, name


def test_header_declares_them():
    header = re.sub(r"\s+", " ", open(vdb.HEADER).read())
    for decl in (
            "typedef struct vdb_filter vdb_filter;",
            "enum { VDB_FILTER_AND = 0, VDB_FILTER_OR = 1, VDB_FILTER_ANDNOT = 2 };",
            "int vdb_ivf_filter_create(vdb_ivf* index, const uint64_t* filter_ids, uint64_t n_filter, int mode, "
            "vdb_filter** out);",
            "int vdb_ivf_filter_create_device(vdb_ivf* index, const uint64_t* d_filter_ids, uint64_t n_filter, "
            "int mode, vdb_filter** out);",
            "int vdb_filter_combine(const vdb_filter* a, const vdb_filter* b, int op, vdb_filter** out);",
            "uint64_t vdb_filter_allowed(const vdb_filter* filter);",
            "int vdb_filter_stale(const vdb_filter* filter);",
            "void vdb_filter_free(vdb_filter* filter);",
            "int vdb_ivf_search_prepared(vdb_ivf* index, const vdb_filter* filter, const float* queries, uint32_t n, "
            "uint32_t nprobe, uint32_t k, float* distances, uint64_t* ids);",
            "int vdb_ivf_range_search_prepared(vdb_ivf* index, const vdb_filter* filter, const float* queries, "
            "uint32_t n, uint32_t nprobe, float radius, uint64_t reserve, vdb_range_result** out);",
            "int vdb_filter_create_last_timing(double* sort_ms, double* mark_ms);"):
        assert decl in header, decl
    # the one-shot calls no longer list them as missing
    assert "Not offered yet: a prepared" not in header
    assert "a filter combined with a radius, the gRPC" not in header


def test_python_surface():
    for name in ("prepare_filter", "search_prepared", "range_search_prepared", "filter_create_last_timing"):
        assert callable(getattr(vdb.IVFFlatIndex, name, None)), name
    F = vdb.Filter
    assert isinstance(F.allowed, property) and isinstance(F.stale, property)
    for name in ("close", "andnot", "__and__", "__or__"):
        assert callable(getattr(F, name, None)), name
    L = vdb.lib()
    assert len(L.vdb_ivf_search_prepared.argtypes) == 8
    assert len(L.vdb_ivf_range_search_prepared.argtypes) == 8
    assert len(L.vdb_ivf_filter_create.argtypes) == 5 and len(L.vdb_ivf_filter_create_device.argtypes) == 5
    assert len(L.vdb_filter_combine.argtypes) == 4


def test_null_arguments_are_refused_before_any_device_call():
    L = vdb.lib()
    ids = (ctypes.c_uint64 * 2)(1, 2)
    out = ctypes.c_void_p(0x1234)
    fake = ctypes.c_void_p(0x1000)  # (never dereferenced: the null check comes first)
    for create in (L.vdb_ivf_filter_create, L.vdb_ivf_filter_create_device):
        assert create(None, ids, 2, 0, ctypes.byref(out)) == INVALID
        assert b"null" in L.vdb_last_error()
        assert out.value == 0x1234  # written on success only
    assert L.vdb_ivf_search_prepared(None, fake, None, 0, 1, 1, None, None) == INVALID
    assert b"null" in L.vdb_last_error()
    assert L.vdb_ivf_search_prepared(fake, None, None, 0, 1, 1, None, None) == INVALID  # a null filter
    assert b"null" in L.vdb_last_error()
    assert L.vdb_ivf_range_search_prepared(None, None, None, 0, 1, 1.0, 0, ctypes.byref(out)) == INVALID
    assert b"null" in L.vdb_last_error()
    assert L.vdb_ivf_range_search_prepared(None, fake, None, 0, 1, 1.0, 0, ctypes.byref(out)) == INVALID
    assert L.vdb_ivf_range_search_prepared(fake, fake, None, 0, 1, 1.0, 0, None) == INVALID
    assert L.vdb_filter_combine(None, None, 0, ctypes.byref(out)) == INVALID
    assert L.vdb_filter_combine(fake, None, 0, ctypes.byref(out)) == INVALID
    assert L.vdb_filter_combine(None, fake, 0, ctypes.byref(out)) == INVALID
    assert out.value == 0x1234


def test_free_stale_and_allowed_take_null():
    L = vdb.lib()
    L.vdb_filter_free(None)
    assert L.vdb_filter_stale(None) == 1
    assert L.vdb_filter_allowed(None) == 0


def test_create_timing_of_a_thread_without_a_call_is_zero():
    L = vdb.lib()
    a, b = ctypes.c_double(1), ctypes.c_double(1)
    assert L.vdb_filter_create_last_timing(ctypes.byref(a), ctypes.byref(b)) == 0
    assert (a.value, b.value) == (0.0, 0.0)
    assert L.vdb_filter_create_last_timing(None, None) == 0


def test_cpp_class_exports_the_prepared_methods():
    out = subprocess.check_output(["nm", "-DC", "--defined-only", vdb.CPP_LIB_PATH], text=True)
    for sym in ("vdb::IVFFlatIndex::prepare_filter(", "vdb::IVFFlatIndex::search_prepared(",
                "vdb::IVFFlatIndex::range_search_prepared(", "vdb::IVFFlatIndex::Filter::~Filter()",
                "vdb::IVFFlatIndex::Filter::stale() const", "vdb::IVFFlatIndex::Filter::allowed() const"):
        assert sym in out, sym
