"""CPU tests of the CosineDistance surface: the C header declares VDB_METRIC_COSINE_DISTANCE = 3
and vdb_unit_rows_device, the library exports it, the Python enum and the C++ enum carry the
new ordinal with 0 to 2 unchanged, the service's metadata round-trips it, and the numpy
restatement of unit(row) behaves on its edge rows."""
import json
import os
import re
import subprocess

import numpy as np

from conftest import ROOT, load_vdb
from cosine_ref import NONE, cos_map, unit_rows_ref

vdb = load_vdb()


def test_header_declares_the_metric_and_the_function():
    header = re.sub(r"\s+", " ", open(vdb.HEADER).read())
    assert re.search(r"VDB_METRIC_L2 = 0, VDB_METRIC_INNER_PRODUCT = 1, VDB_METRIC_COSINE = 2, "
                     r"VDB_METRIC_COSINE_DISTANCE = 3 \}", header)
    assert re.search(r"int vdb_unit_rows_device\(const float\* d_in, uint64_t n, uint32_t dim, float\* d_out, "
                     r"void\* stream\);", header)


def test_library_exports_unit_rows_device():
    out = subprocess.check_output(["nm", "-D", "--defined-only", vdb.LIB_PATH], text=True)
    assert "vdb_unit_rows_device" in set(re.findall(r" T (vdb_\w+)", out))
    L = vdb.lib()
    assert L.vdb_unit_rows_device.argtypes is not None and len(L.vdb_unit_rows_device.argtypes) == 5
    assert callable(vdb.unit_rows_device)
    # nothing to do for n = 0, and null rows are refused, both before any device call
    assert L.vdb_unit_rows_device(None, 0, 8, None, None) == 0
    assert L.vdb_unit_rows_device(None, 4, 8, None, None) == -1
    assert b"null" in L.vdb_last_error()


def test_metric_ordinals():
    assert int(vdb.Metric.CosineDistance) == 3
    assert (int(vdb.Metric.L2), int(vdb.Metric.InnerProduct), int(vdb.Metric.Cosine)) == (0, 1, 2)
    assert len(vdb.Metric) == 4


def test_cpp_enum_names_cosine_distance():
    src = ('#include "vdb/ivf_flat_index.h"\n#include "vdb_ivf.h"\n'
           "using M = vdb::kernels::Metric;\n"
           "static_assert((int)M::L2 == 0 && (int)M::InnerProduct == 1 && (int)M::Cosine == 2, \"\");\n"
           "static_assert((int)M::CosineDistance == 3 && VDB_METRIC_COSINE_DISTANCE == 3, \"\");\n"
           "int main(){vdb::IVFFlatIndex::Config c{64,16,M::CosineDistance};return (int)c.nlist-16;}\n")
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"],
                       input=src, text=True, capture_output=True)
    assert p.returncode == 0, p.stderr


def test_service_metadata_round_trips_metric_3():
    cfg = vdb.IVFFlatIndex.Config(16, 4, vdb.Metric.CosineDistance)
    meta = json.loads(json.dumps({"dimension": cfg.dimension, "nlist": cfg.nlist, "metric": int(cfg.metric)}))
    assert vdb.Metric(int(meta.get("metric", 0))) is vdb.Metric.CosineDistance


def test_unit_rows_ref_edge_rows():
    rng = np.random.default_rng(3)
    for d in (1, 3, 20, 64, 65, 128, 257, 768):
        X = rng.standard_normal((50, d)).astype(np.float32)
        X[0] = 0.0
        X[1] = 1e30
        U = unit_rows_ref(X)
        assert np.array_equal(U[0].view(np.uint32), X[0].view(np.uint32))  # a zero row stays
        assert np.array_equal(U[1].view(np.uint32), X[1].view(np.uint32))  # an overflowing sum: kept
        norms = np.sqrt((U[2:].astype(np.float64) ** 2).sum(axis=1))
        assert np.all(np.abs(norms - 1.0) < 2.5e-7), (d, norms.min(), norms.max())
    D = np.array([[-0.5, 3.4e38]], np.float32)
    I = np.array([[7, NONE]], np.uint64)
    assert cos_map(D, I).tolist() == [[0.5, float(np.float32(3.4e38))]]
