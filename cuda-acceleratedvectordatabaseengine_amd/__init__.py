"""MI355X-native IVF-Flat search engine — Python host mirror of the reference API.

The product is ``lib/libvdb_ivf.so`` (hand-written gfx950 HIP kernels behind the C ABI
in ``include/vdb_ivf.h``). This module binds that ABI with ctypes and mirrors the
reference's ``vdb::IVFFlatIndex`` surface (``engine/ivf_flat_index.h:14-67``):
``Config``, ``SearchParams``, ``train``, ``add``, ``search``, ``warmup_lists``,
``evict_list``, ``get_gpu_memory_usage``, ``get_total_vectors``, plus the
device-resident and list-sharded forms used by ``bench.py``.

There is no CPU fallback: if the library is missing or no GPU is present, calls
raise. Import under any name, e.g. ``importlib`` with the directory path
(the directory name is not a Python identifier); ``load()`` below does that.
"""
from __future__ import annotations

import ctypes
import enum
import os
import subprocess
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VDB_IVF_LIB") or os.path.join(_HERE, "lib", "libvdb_ivf.so")  # override: A/B builds
CPP_LIB_PATH = os.path.join(_HERE, "lib", "libvdb_ivf_cpp.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "vdb_ivf.h")

_lib = None


class Metric(enum.IntEnum):
    """kernels::Metric (engine/kernels.cuh:24-28), and this engine's own CosineDistance: true
    cosine distance, an inner-product index over unit rows whose distances are reported as
    1.0f + (-dot) (include/vdb_ivf.h, VDB_METRIC_COSINE_DISTANCE). Cosine (2) stays the
    reference CPU path's 0.0f."""
    L2 = 0
    InnerProduct = 1
    Cosine = 2
    CosineDistance = 3


class VdbError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"vdb error {code}: {msg}")
        self.code = code


class _Config(ctypes.Structure):
    _fields_ = [("dimension", ctypes.c_uint32), ("nlist", ctypes.c_uint32), ("metric", ctypes.c_int32),
                ("use_gpu", ctypes.c_int32), ("max_gpu_memory", ctypes.c_uint64), ("device", ctypes.c_int32)]


class CacheStats(ctypes.Structure):
    _fields_ = [("capacity_bytes", ctypes.c_uint64), ("resident_bytes", ctypes.c_uint64),
                ("resident_lists", ctypes.c_uint64), ("loads", ctypes.c_uint64), ("evictions", ctypes.c_uint64),
                ("bytes_loaded", ctypes.c_uint64), ("file_bytes_read", ctypes.c_uint64),
                ("subbatches", ctypes.c_uint64), ("prefetches", ctypes.c_uint64), ("sync_loads", ctypes.c_uint64),
                ("io_uring", ctypes.c_int32), ("o_direct", ctypes.c_int32),
                ("screen_resident", ctypes.c_int32), ("reserved", ctypes.c_int32), ("screen_bytes", ctypes.c_uint64),
                ("screen_batches", ctypes.c_uint64), ("screen_rows_fetched", ctypes.c_uint64),
                ("screen_row_bytes", ctypes.c_uint64), ("screen_reruns", ctypes.c_uint64),
                ("screen_rows_cached", ctypes.c_uint64), ("screen_fallbacks", ctypes.c_uint64)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class Profile(ctypes.Structure):
    _fields_ = [("batches", ctypes.c_uint64), ("scan_launches", ctypes.c_uint64), ("scan_ms", ctypes.c_double),
                ("coarse_ms", ctypes.c_double), ("total_ms", ctypes.c_double), ("scan_vectors", ctypes.c_uint64),
                ("distinct_lists", ctypes.c_uint64), ("work_items", ctypes.c_uint64),
                ("scan_bytes", ctypes.c_uint64), ("pair_vectors", ctypes.c_uint64),
                ("exact_reranks", ctypes.c_uint64), ("bounded_blocks", ctypes.c_uint64),
                ("computed_vectors", ctypes.c_uint64), ("local_merge_ms", ctypes.c_double),
                ("exchanges", ctypes.c_uint64), ("exchange_ms", ctypes.c_double), ("rank_merge_ms", ctypes.c_double),
                ("screen_collected", ctypes.c_uint64), ("collect_ms", ctypes.c_double),
                ("recheck_ms", ctypes.c_double), ("screen_floor_batches", ctypes.c_uint64),
                ("screen_floor_trips", ctypes.c_uint64), ("screen_shadow", ctypes.c_uint32),
                ("reserved0", ctypes.c_uint32)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


def build(jobs: int = 8) -> str:
    """Compile the HIP library for gfx950 (hipcc; cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-s", f"-j{jobs}", "-C", _HERE])
    return LIB_PATH


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `make -C {_HERE}` (no CPU fallback exists)")
    # torch ships its own libamdhip64 (SONAME libamdhip64.so.7). Loading torch first
    # lets libvdb_ivf.so bind to that same HIP runtime by SONAME, so torch tensors and
    # streams and this library share one runtime; the other order loads two.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int32
    sigs = {
        "vdb_last_error": (ctypes.c_char_p, []),
        "vdb_version": (ctypes.c_char_p, []),
        "vdb_build_id": (ctypes.c_char_p, []),
        "vdb_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
        "vdb_ivf_create": (ctypes.c_int, [ctypes.POINTER(_Config), ctypes.POINTER(vp)]),
        "vdb_ivf_destroy": (ctypes.c_int, [vp]),
        "vdb_ivf_train": (ctypes.c_int, [vp, vp, u64]),
        "vdb_ivf_train_device": (ctypes.c_int, [vp, vp, u64]),
        "vdb_ivf_set_centroids": (ctypes.c_int, [vp, vp]),
        "vdb_ivf_get_centroids": (ctypes.c_int, [vp, vp]),
        "vdb_ivf_add": (ctypes.c_int, [vp, vp, vp, u64]),
        "vdb_ivf_add_device": (ctypes.c_int, [vp, vp, vp, u64]),
        "vdb_ivf_add_to_lists": (ctypes.c_int, [vp, vp, vp, vp, u64]),
        "vdb_ivf_remove_ids": (ctypes.c_int, [vp, vp, u64, ctypes.POINTER(ctypes.c_uint64)]),
        "vdb_remove_last_timing": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                                  ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)]),
        "vdb_ivf_upsert": (ctypes.c_int, [vp, vp, vp, u64, ctypes.POINTER(ctypes.c_uint64),
                                          ctypes.POINTER(ctypes.c_uint64)]),
        "vdb_ivf_upsert_device": (ctypes.c_int, [vp, vp, vp, u64, ctypes.POINTER(ctypes.c_uint64),
                                                 ctypes.POINTER(ctypes.c_uint64)]),
        "vdb_upsert_last_timing": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                                  ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                                  ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "vdb_ivf_search": (ctypes.c_int, [vp, vp, u32, u32, u32, vp, vp]),
        "vdb_ivf_search_filtered": (ctypes.c_int, [vp, vp, u32, u32, u32, vp, u64, ctypes.c_int, vp, vp]),
        "vdb_filter_last_timing": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                                  ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)]),
        "vdb_ivf_range_search": (ctypes.c_int, [vp, vp, u32, u32, ctypes.c_float, u64, ctypes.POINTER(vp)]),
        "vdb_range_result_n": (u32, [vp]),
        "vdb_range_result_lims": (vp, [vp]),
        "vdb_range_result_distances": (vp, [vp]),
        "vdb_range_result_ids": (vp, [vp]),
        "vdb_range_result_free": (None, [vp]),
        "vdb_range_last_timing": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                                 ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                                 ctypes.POINTER(ctypes.c_uint32)]),
        "vdb_ivf_filter_create": (ctypes.c_int, [vp, vp, u64, ctypes.c_int, ctypes.POINTER(vp)]),
        "vdb_ivf_filter_create_device": (ctypes.c_int, [vp, vp, u64, ctypes.c_int, ctypes.POINTER(vp)]),
        "vdb_filter_combine": (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.POINTER(vp)]),
        "vdb_filter_allowed": (u64, [vp]),
        "vdb_filter_stale": (ctypes.c_int, [vp]),
        "vdb_filter_free": (None, [vp]),
        "vdb_ivf_search_prepared": (ctypes.c_int, [vp, vp, vp, u32, u32, u32, vp, vp]),
        "vdb_ivf_search_prepared_multi": (ctypes.c_int, [vp, vp, u32, vp, vp, u32, u32, u32, vp, vp]),
        "vdb_ivf_range_search_prepared": (ctypes.c_int, [vp, vp, vp, u32, u32, ctypes.c_float, u64,
                                                         ctypes.POINTER(vp)]),
        "vdb_ivf_range_search_screened": (ctypes.c_int, [vp, vp, vp, u32, u32, ctypes.c_float, u64,
                                                         ctypes.POINTER(vp)]),
        "vdb_range_screen_last_timing": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                                        ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64),
                                                        ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32),
                                                        ctypes.POINTER(ctypes.c_uint32)]),
        "vdb_filter_create_last_timing": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double),
                                                         ctypes.POINTER(ctypes.c_double)]),
        "vdb_ivf_fetch_ids": (ctypes.c_int, [vp, vp, u64, vp, vp, ctypes.POINTER(ctypes.c_uint64)]),
        "vdb_ivf_fetch_ids_device": (ctypes.c_int, [vp, vp, u64, vp, vp, ctypes.POINTER(ctypes.c_uint64)]),
        "vdb_ivf_search_ids": (ctypes.c_int, [vp, vp, u32, u32, u32, vp, vp, vp]),
        "vdb_fetch_last_timing": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                                 ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)]),
        "vdb_ivf_search_device": (ctypes.c_int, [vp, vp, u32, u32, u32, vp, vp, vp]),
        "vdb_ivf_set_shard": (ctypes.c_int, [vp, u32, u32]),
        "vdb_ivf_plan_shard": (ctypes.c_int, [vp, u32, u32, vp]),
        "vdb_ivf_assign_device": (ctypes.c_int, [vp, vp, u64, vp]),
        "vdb_ivf_add_to_lists_device": (ctypes.c_int, [vp, vp, vp, vp, u64]),
        "vdb_ivf_save": (ctypes.c_int, [vp, ctypes.c_char_p]),
        "vdb_ivf_load": (ctypes.c_int, [vp, ctypes.c_char_p]),
        "vdb_merge_ranks_device": (ctypes.c_int, [vp, vp, u32, u32, u32, vp, vp, vp]),
        "vdb_shard_plan": (ctypes.c_int, [vp, u32, u32, vp]),
        "vdb_shard_plan_probe_weighted": (ctypes.c_int, [vp, vp, u64, u32, u32, u32, vp]),
        "vdb_ivf_probe_census": (ctypes.c_int, [vp, vp, u64, u32, vp]),
        "vdb_ivf_set_shard_owners": (ctypes.c_int, [vp, u32, u32, vp]),
        "vdb_ivf_plan_shard_owners": (ctypes.c_int, [vp, u32, u32, vp, vp]),
        "vdb_rank_record_bytes": (u64, [u32, u32]),
        "vdb_merge_ranks_packed_device": (ctypes.c_int, [vp, u32, u32, u32, vp, vp, vp]),
        "vdb_ivf_warmup": (ctypes.c_int, [vp, vp, u32]),
        "vdb_ivf_evict": (ctypes.c_int, [vp, u32]),
        "vdb_ivf_gpu_bytes": (u64, [vp]),
        "vdb_ivf_gpu_bytes_allocated": (u64, [vp]),
        "vdb_ivf_ntotal": (u64, [vp]),
        "vdb_ivf_list_sizes": (ctypes.c_int, [vp, vp]),
        "vdb_ivf_get_list": (ctypes.c_int, [vp, u32, vp, vp]),
        "vdb_ivf_set_batch": (ctypes.c_int, [vp, u32]),
        "vdb_ivf_set_stale_slots": (ctypes.c_int, [vp, i32]),
        "vdb_ivf_set_coarse_mode": (ctypes.c_int, [vp, i32]),
        "vdb_ivf_set_option": (ctypes.c_int, [vp, ctypes.c_char_p, ctypes.c_int64]),
        "vdb_ivf_coalesce_stats": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "vdb_ivf_cache_stats": (ctypes.c_int, [vp, ctypes.POINTER(CacheStats)]),
        "vdb_ivf_fill_row_cache": (ctypes.c_int, [vp, vp]),
        "vdb_ivf_survivor_histogram": (ctypes.c_int, [vp, vp]),
        "vdb_ivf_collect_stamps": (ctypes.c_int, [vp, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64),
                                                  ctypes.POINTER(ctypes.c_uint64)]),
        "vdb_ivf_screen_snapshot": (ctypes.c_int, [vp, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint64,
                                                   ctypes.POINTER(ctypes.c_uint64)]),
        "vdb_ivf_coarse_snapshot": (ctypes.c_int, [vp, vp, u32, u32, vp, vp, vp, vp, vp]),
        "vdb_ivf_open_lists": (ctypes.c_int, [vp, ctypes.c_char_p]),
        "vdb_ivf_profile_enable": (ctypes.c_int, [vp, i32]),
        "vdb_ivf_profile_reset": (ctypes.c_int, [vp]),
        "vdb_ivf_profile_read": (ctypes.c_int, [vp, ctypes.POINTER(Profile)]),
        "vdb_ivf_synchronize": (ctypes.c_int, [vp]),
        "vdb_ivf_stream": (vp, [vp]),
        "vdb_gen_normal_device": (ctypes.c_int, [vp, u64, u64, u64, vp]),
        "vdb_gen_mixture_device": (ctypes.c_int, [vp, u64, u32, vp, u32, ctypes.c_float, u64, u64, vp]),
        "vdb_unit_rows_device": (ctypes.c_int, [vp, u64, u32, vp, vp]),
        "vdb_comm_unique_id": (ctypes.c_int, [vp]),
        "vdb_ivf_attach_comm": (ctypes.c_int, [vp, vp, u32, u32]),
        "vdb_ivf_detach_comm": (ctypes.c_int, [vp]),
        "vdb_ivf_comm_status": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "vdb_ivf_create_group": (ctypes.c_int, [ctypes.POINTER(_Config), vp, u32, ctypes.POINTER(vp)]),
        "vdb_ivf_group_size": (u32, [vp]),
        "vdb_ivf_list_owners": (ctypes.c_int, [vp, vp]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def _check(rc: int):
    if rc != 0:
        raise VdbError(rc, lib().vdb_last_error().decode())


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def build_id() -> str:
    """Hash of the sources behind the scan kernels of the loaded library (vdb_build_id)."""
    return lib().vdb_build_id().decode()


def device_count() -> int:
    c = ctypes.c_int(0)
    _check(lib().vdb_device_count(ctypes.byref(c)))
    return c.value


def shard_plan(list_sizes, world: int) -> np.ndarray:
    """LPT owner rank of every list (host-only, identical on every rank)."""
    s = np.ascontiguousarray(list_sizes, dtype=np.uint64)
    out = np.empty(len(s), dtype=np.uint32)
    _check(lib().vdb_shard_plan(_ptr(s), len(s), world, _ptr(out)))
    return out


def shard_plan_probe_weighted(list_sizes, probe_counts, n_sample: int, batch: int, world: int) -> np.ndarray:
    """LPT owner of every list over the expected scan cost per batch (probe census weights)."""
    s = np.ascontiguousarray(list_sizes, dtype=np.uint64)
    c = np.ascontiguousarray(probe_counts, dtype=np.uint64)
    out = np.empty(len(s), dtype=np.uint32)
    _check(lib().vdb_shard_plan_probe_weighted(_ptr(s), _ptr(c), n_sample, batch, len(s), world, _ptr(out)))
    return out


def gen_normal_device(ptr: int, n: int, seed: int, offset: int = 0, stream: int | None = None):
    """Fill n fp32 at device address ``ptr`` with deterministic N(0,1) draws."""
    _check(lib().vdb_gen_normal_device(ctypes.c_void_p(ptr), n, seed, offset, ctypes.c_void_p(stream or 0)))


def unit_rows_device(in_ptr: int, n: int, dim: int, out_ptr: int, stream: int | None = None):
    """unit(row) of Metric.CosineDistance for the n x dim fp32 rows at device address ``in_ptr``
    into the n x dim rows at ``out_ptr`` (may not alias the input, which is only read)."""
    _check(lib().vdb_unit_rows_device(ctypes.c_void_p(in_ptr), n, dim, ctypes.c_void_p(out_ptr),
                                      ctypes.c_void_p(stream or 0)))


def gen_mixture_device(ptr: int, rows: int, dim: int, centers_ptr: int, ncomp: int, sigma: float, seed: int,
                       row0: int = 0, stream: int | None = None):
    """Fill rows x dim fp32 at ``ptr`` with Gaussian-mixture draws around the ncomp x dim
    device centers (synthetic clustered data; rows row0.. of one deterministic stream)."""
    _check(lib().vdb_gen_mixture_device(ctypes.c_void_p(ptr), rows, dim, ctypes.c_void_p(centers_ptr), ncomp,
                                        ctypes.c_float(sigma), seed, row0, ctypes.c_void_p(stream or 0)))


def merge_ranks_device(dist_ptr: int, ids_ptr: int, nranks: int, n: int, k: int, out_dist_ptr: int,
                       out_ids_ptr: int, stream: int | None = None):
    _check(lib().vdb_merge_ranks_device(ctypes.c_void_p(dist_ptr), ctypes.c_void_p(ids_ptr), nranks, n, k,
                                        ctypes.c_void_p(out_dist_ptr), ctypes.c_void_p(out_ids_ptr),
                                        ctypes.c_void_p(stream or 0)))


COMM_ID_BYTES = 128  # VDB_COMM_ID_BYTES


def comm_unique_id() -> bytes:
    """A fresh RCCL communicator id (rank 0 draws it and shares it with the other ranks)."""
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    _check(lib().vdb_comm_unique_id(buf))
    return buf.raw


def rank_record_bytes(n: int, k: int) -> int:
    """Bytes of one rank's packed partial record (f32 dist [n][k], pad to 8, u64 ids [n][k])."""
    return int(lib().vdb_rank_record_bytes(n, k))


def rank_record_ids_offset(n: int, k: int) -> int:
    return (n * k * 4 + 7) // 8 * 8


def merge_ranks_packed_device(records_ptr: int, nranks: int, n: int, k: int, out_dist_ptr: int, out_ids_ptr: int,
                              stream: int | None = None):
    _check(lib().vdb_merge_ranks_packed_device(ctypes.c_void_p(records_ptr), nranks, n, k,
                                               ctypes.c_void_p(out_dist_ptr), ctypes.c_void_p(out_ids_ptr),
                                               ctypes.c_void_p(stream or 0)))


FILTER_AND, FILTER_OR, FILTER_ANDNOT = 0, 1, 2  # VDB_FILTER_AND / _OR / _ANDNOT


class Filter:
    """A prepared id filter (vdb_filter; not in the reference): the allow masks of one index's
    rows, kept on the device for any number of search_prepared / range_search_prepared calls.
    Made by IVFFlatIndex.prepare_filter or by combining two filters of one index: ``a & b``,
    ``a | b``, ``a.andnot(b)``. It may outlive its index; it is stale once the index's rows
    changed (add, a remove that removed, load, ...) or the index is gone."""

    def __init__(self, handle):
        self._f = handle

    @property
    def allowed(self) -> int:
        """Stored rows the filter lets through."""
        return int(lib().vdb_filter_allowed(self._f))

    @property
    def stale(self) -> bool:
        return bool(lib().vdb_filter_stale(self._f))

    def _combine(self, other: "Filter", op: int) -> "Filter":
        if not isinstance(other, Filter):
            return NotImplemented
        out = ctypes.c_void_p()
        _check(lib().vdb_filter_combine(self._f, other._f, op, ctypes.byref(out)))
        return Filter(out)

    def __and__(self, other):
        return self._combine(other, FILTER_AND)

    def __or__(self, other):
        return self._combine(other, FILTER_OR)

    def andnot(self, other: "Filter") -> "Filter":
        """The rows this filter allows and `other` does not."""
        return self._combine(other, FILTER_ANDNOT)

    def close(self):
        if getattr(self, "_f", None):
            lib().vdb_filter_free(self._f)
            self._f = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class IVFFlatIndex:
    """vdb::IVFFlatIndex (engine/ivf_flat_index.h:14-67) on one MI355X."""

    @dataclass
    class Config:
        dimension: int
        nlist: int
        metric: Metric = Metric.L2
        use_gpu: bool = True
        max_gpu_memory: int = 8 << 30
        device: int = 0
        devices: tuple = ()  # > 1 entries: one index sharded by list over these GPUs (group handle)

    @dataclass
    class SearchParams:
        nprobe: int = 10
        k: int = 10
        use_exact_rerank: bool = False  # accepted, unused — as in the reference

    def __init__(self, config: "IVFFlatIndex.Config"):
        self.config = config
        if config.dimension <= 0 or config.nlist <= 0:
            raise ValueError("Invalid configuration: dimension and nlist must be > 0")
        c = _Config(config.dimension, config.nlist, int(config.metric), int(config.use_gpu),
                    config.max_gpu_memory, config.device)
        h = ctypes.c_void_p()
        if config.devices:
            devs = (ctypes.c_int * len(config.devices))(*config.devices)
            _check(lib().vdb_ivf_create_group(ctypes.byref(c), devs, len(config.devices), ctypes.byref(h)))
        else:
            _check(lib().vdb_ivf_create(ctypes.byref(c), ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().vdb_ivf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def dimension(self) -> int:
        return self.config.dimension

    # ---- build ----
    def train(self, vectors: np.ndarray):
        v = np.ascontiguousarray(vectors, dtype=np.float32).reshape(-1, self.dimension)
        _check(lib().vdb_ivf_train(self._h, _ptr(v), v.shape[0]))

    def train_device(self, ptr: int, n: int):
        _check(lib().vdb_ivf_train_device(self._h, ctypes.c_void_p(ptr), n))

    def add(self, vectors: np.ndarray, ids: np.ndarray):
        v = np.ascontiguousarray(vectors, dtype=np.float32).reshape(-1, self.dimension)
        i = np.ascontiguousarray(ids, dtype=np.uint64)
        if i.shape[0] != v.shape[0]:
            raise ValueError("vectors and ids differ in length")
        _check(lib().vdb_ivf_add(self._h, _ptr(v), _ptr(i), v.shape[0]))

    def add_device(self, vec_ptr: int, ids_ptr: int, n: int):
        _check(lib().vdb_ivf_add_device(self._h, ctypes.c_void_p(vec_ptr), ctypes.c_void_p(ids_ptr), n))

    def add_to_lists(self, vectors: np.ndarray, ids: np.ndarray, lists: np.ndarray):
        """Append host rows to explicitly given lists, input order kept per list (vdb_ivf_add_to_lists)."""
        v = np.ascontiguousarray(vectors, dtype=np.float32).reshape(-1, self.dimension)
        i = np.ascontiguousarray(ids, dtype=np.uint64)
        l = np.ascontiguousarray(lists, dtype=np.uint32)
        if i.shape[0] != v.shape[0] or l.shape[0] != v.shape[0]:
            raise ValueError("vectors, ids and lists differ in length")
        _check(lib().vdb_ivf_add_to_lists(self._h, _ptr(v), _ptr(i), _ptr(l), v.shape[0]))

    def remove_ids(self, ids) -> int:
        """Remove every stored row whose id is listed (vdb_ivf_remove_ids; not in the reference).
        Returns the number of rows removed; the index is afterwards the one built by adding the
        surviving rows in their original order."""
        i = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        gone = ctypes.c_uint64(0)
        _check(lib().vdb_ivf_remove_ids(self._h, _ptr(i), i.shape[0], ctypes.byref(gone)))
        return int(gone.value)

    def remove_last_timing(self) -> dict:
        """The calling thread's latest remove_ids by step (vdb_remove_last_timing)."""
        a, b, c, r = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0), ctypes.c_uint64(0)
        _check(lib().vdb_remove_last_timing(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(r)))
        return {"mark_ms": a.value, "plan_ms": b.value, "compact_ms": c.value, "rows_kept": r.value}

    def upsert(self, vectors: np.ndarray, ids: np.ndarray):
        """Replace the rows of the listed ids that are stored and insert the others, in one pass
        over the lists (vdb_ivf_upsert; not in the reference). An id listed more than once takes
        its last entry. Returns (replaced, inserted): stored rows that went, distinct ids. The
        index is afterwards the one remove_ids(ids) followed by add(those entries) leaves."""
        v = np.ascontiguousarray(vectors, dtype=np.float32).reshape(-1, self.dimension)
        i = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        if i.shape[0] != v.shape[0]:
            raise ValueError("vectors and ids differ in length")
        r, w = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(lib().vdb_ivf_upsert(self._h, _ptr(v), _ptr(i), v.shape[0], ctypes.byref(r), ctypes.byref(w)))
        return int(r.value), int(w.value)

    def upsert_device(self, vec_ptr: int, ids_ptr: int, n: int):
        """upsert on buffers of the index's device that are complete before the call
        (vdb_ivf_upsert_device): n x dimension floats and n uint64 ids. Returns (replaced, inserted)."""
        r, w = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(lib().vdb_ivf_upsert_device(self._h, ctypes.c_void_p(vec_ptr), ctypes.c_void_p(ids_ptr), n,
                                           ctypes.byref(r), ctypes.byref(w)))
        return int(r.value), int(w.value)

    def upsert_last_timing(self) -> dict:
        """The calling thread's latest upsert by step (vdb_upsert_last_timing)."""
        a, b, c, d = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
        k, w = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(lib().vdb_upsert_last_timing(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d),
                                            ctypes.byref(k), ctypes.byref(w)))
        return {"resolve_ms": a.value, "mark_ms": b.value, "plan_ms": c.value, "move_ms": d.value,
                "rows_kept": k.value, "rows_written": w.value}

    def assign_device(self, vec_ptr: int, n: int, lists_ptr: int):
        """Exact nearest-centroid list of n device rows into u32 lists_ptr (assign_to_lists, cpp:259-295)."""
        _check(lib().vdb_ivf_assign_device(self._h, ctypes.c_void_p(vec_ptr), n, ctypes.c_void_p(lists_ptr)))

    def add_to_lists_device(self, vec_ptr: int, ids_ptr: int, lists_ptr: int, n: int):
        _check(lib().vdb_ivf_add_to_lists_device(self._h, ctypes.c_void_p(vec_ptr), ctypes.c_void_p(ids_ptr),
                                                 ctypes.c_void_p(lists_ptr), n))

    @property
    def centroids(self) -> np.ndarray:
        out = np.empty((self.config.nlist, self.dimension), dtype=np.float32)
        _check(lib().vdb_ivf_get_centroids(self._h, _ptr(out)))
        return out

    @centroids.setter
    def centroids(self, c: np.ndarray):
        c = np.ascontiguousarray(c, dtype=np.float32).reshape(self.config.nlist, self.dimension)
        _check(lib().vdb_ivf_set_centroids(self._h, _ptr(c)))

    # ---- search ----
    def search(self, queries: np.ndarray, params: "IVFFlatIndex.SearchParams | None" = None, *,
               nprobe: int | None = None, k: int | None = None):
        p = params or IVFFlatIndex.SearchParams()
        nprobe = p.nprobe if nprobe is None else nprobe
        k = p.k if k is None else k
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dimension)
        n = q.shape[0]
        D = np.empty((n, k), dtype=np.float32)
        I = np.empty((n, k), dtype=np.uint64)
        _check(lib().vdb_ivf_search(self._h, _ptr(q), n, nprobe, k, _ptr(D), _ptr(I)))
        return D, I

    def search_filtered(self, queries: np.ndarray, params: "IVFFlatIndex.SearchParams | None" = None, *,
                        ids, include: bool = False, nprobe: int | None = None, k: int | None = None):
        """search over the stored rows an id filter allows (vdb_ivf_search_filtered; not in the
        reference). include=False: every row whose id is not in `ids`; include=True: only rows
        whose id is. Returns (distances, indices) like search: the result search gives on an
        index holding only the allowed rows."""
        p = params or IVFFlatIndex.SearchParams()
        nprobe = p.nprobe if nprobe is None else nprobe
        k = p.k if k is None else k
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dimension)
        f = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        n = q.shape[0]
        D = np.empty((n, k), dtype=np.float32)
        I = np.empty((n, k), dtype=np.uint64)
        _check(lib().vdb_ivf_search_filtered(self._h, _ptr(q), n, nprobe, k, _ptr(f), f.shape[0],
                                             1 if include else 0, _ptr(D), _ptr(I)))
        return D, I

    def filter_last_timing(self) -> dict:
        """The calling thread's latest search_filtered by step (vdb_filter_last_timing)."""
        a, b, c, r = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0), ctypes.c_uint64(0)
        _check(lib().vdb_filter_last_timing(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(r)))
        return {"mark_ms": a.value, "scan_ms": b.value, "merge_ms": c.value, "pairs_scanned": r.value}

    def fetch_ids(self, ids):
        """The stored rows carrying `ids` (vdb_ivf_fetch_ids; not in the reference). Returns
        (vectors, found): vectors[i] is the row of ids[i] bit for bit as stored (the one at the
        lowest (list, position) if the id is stored more than once), zeros with found[i] = 0
        where no row carries it."""
        i = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        n = i.shape[0]
        V = np.empty((n, self.dimension), dtype=np.float32)
        F = np.empty(n, dtype=np.uint8)
        _check(lib().vdb_ivf_fetch_ids(self._h, _ptr(i), n, _ptr(V), _ptr(F), None))
        return V, F

    def fetch_ids_device(self, ids_ptr: int, n: int, vec_ptr: int | None = None, found_ptr: int | None = None) -> int:
        """fetch_ids on buffers of the index's device that are complete before the call
        (vdb_ivf_fetch_ids_device): n uint64 ids in, n x dimension floats and n bytes out, either
        of which may be None. Returns the entries found."""
        c = ctypes.c_uint64(0)
        _check(lib().vdb_ivf_fetch_ids_device(self._h, ctypes.c_void_p(ids_ptr), n, ctypes.c_void_p(vec_ptr or 0),
                                              ctypes.c_void_p(found_ptr or 0), ctypes.byref(c)))
        return int(c.value)

    def search_ids(self, ids, nprobe: int = 10, k: int = 10):
        """search with the stored rows of `ids` as the queries (vdb_ivf_search_ids; not in the
        reference); the rows never leave the device. Returns (distances, indices, found): the
        found entries' results are search's over their rows in request order, the others hold
        (FLT_MAX, UINT64_MAX)."""
        i = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        n = i.shape[0]
        D = np.empty((n, k), dtype=np.float32)
        I = np.empty((n, k), dtype=np.uint64)
        F = np.empty(n, dtype=np.uint8)
        _check(lib().vdb_ivf_search_ids(self._h, _ptr(i), n, nprobe, k, _ptr(D), _ptr(I), _ptr(F)))
        return D, I, F

    def fetch_last_timing(self) -> dict:
        """The calling thread's latest fetch_ids / search_ids by step (vdb_fetch_last_timing)."""
        a, b, c, r = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0), ctypes.c_uint64(0)
        _check(lib().vdb_fetch_last_timing(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(r)))
        return {"sort_ms": a.value, "locate_ms": b.value, "gather_ms": c.value, "rows_found": r.value}

    def prepare_filter(self, ids, include: bool = False, *, device_ptr: int | None = None, n: int = 0) -> Filter:
        """The id filter of search_filtered, prepared once (vdb_ivf_filter_create; not in the
        reference). include=False: every row whose id is not in `ids`; include=True: only rows
        whose id is. With device_ptr, the n uint64 ids are read from that address on the index's
        device (vdb_ivf_filter_create_device) and `ids` is ignored."""
        out = ctypes.c_void_p()
        mode = 1 if include else 0
        if device_ptr is not None:
            _check(lib().vdb_ivf_filter_create_device(self._h, ctypes.c_void_p(device_ptr), n, mode, ctypes.byref(out)))
        else:
            f = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
            _check(lib().vdb_ivf_filter_create(self._h, _ptr(f), f.shape[0], mode, ctypes.byref(out)))
        return Filter(out)

    def filter_create_last_timing(self) -> dict:
        """The calling thread's latest prepare_filter by step (vdb_filter_create_last_timing)."""
        a, b = ctypes.c_double(0), ctypes.c_double(0)
        _check(lib().vdb_filter_create_last_timing(ctypes.byref(a), ctypes.byref(b)))
        return {"sort_ms": a.value, "mark_ms": b.value}

    def search_prepared(self, queries: np.ndarray, flt: Filter, params: "IVFFlatIndex.SearchParams | None" = None, *,
                        nprobe: int | None = None, k: int | None = None):
        """search_filtered's result for the filter's rows, without taking the masks again
        (vdb_ivf_search_prepared). Returns (distances, indices)."""
        p = params or IVFFlatIndex.SearchParams()
        nprobe = p.nprobe if nprobe is None else nprobe
        k = p.k if k is None else k
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dimension)
        n = q.shape[0]
        D = np.empty((n, k), dtype=np.float32)
        I = np.empty((n, k), dtype=np.uint64)
        _check(lib().vdb_ivf_search_prepared(self._h, flt._f, _ptr(q), n, nprobe, k, _ptr(D), _ptr(I)))
        return D, I

    def search_prepared_multi(self, queries: np.ndarray, filters, filter_of,
                              params: "IVFFlatIndex.SearchParams | None" = None, *, nprobe: int | None = None,
                              k: int | None = None):
        """One search for a batch whose queries each name their own prepared filter
        (vdb_ivf_search_prepared_multi): query i is searched under filters[filter_of[i]]. For
        every filter, the rows of its queries are what search_prepared returns for those queries
        in call order. filters: a sequence of Filter. Returns (distances, indices)."""
        p = params or IVFFlatIndex.SearchParams()
        nprobe = p.nprobe if nprobe is None else nprobe
        k = p.k if k is None else k
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dimension)
        n = q.shape[0]
        fo = np.ascontiguousarray(filter_of, dtype=np.uint32).reshape(-1)
        if fo.shape[0] != n:
            raise ValueError("filter_of needs one entry per query")
        filters = list(filters)
        # (a Filter holds a c_void_p, or None once closed: a null entry, which the library refuses)
        tab = (ctypes.c_void_p * max(len(filters), 1))(*[getattr(f._f, "value", f._f) for f in filters])
        D = np.empty((n, k), dtype=np.float32)
        I = np.empty((n, k), dtype=np.uint64)
        _check(lib().vdb_ivf_search_prepared_multi(self._h, tab, len(filters), _ptr(fo), _ptr(q), n, nprobe, k,
                                                   _ptr(D), _ptr(I)))
        return D, I

    def range_search_prepared(self, queries: np.ndarray, flt: "Filter | None", radius: float, *, nprobe: int = 10,
                              reserve: int = 0, screen: bool = False):
        """range_search over the rows the filter allows (vdb_ivf_range_search_prepared): the
        result range_search gives on an index holding only those rows. flt=None: range_search.
        screen: as for range_search. Returns (lims, distances, ids)."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dimension)
        r = ctypes.c_void_p()
        call = lib().vdb_ivf_range_search_screened if screen else lib().vdb_ivf_range_search_prepared
        _check(call(self._h, flt._f if flt is not None else None, _ptr(q), q.shape[0], nprobe, float(radius), reserve,
                    ctypes.byref(r)))
        return self._take_range_result(r, q.shape[0])

    def range_search(self, queries: np.ndarray, radius: float, *, nprobe: int = 10, reserve: int = 0,
                     screen: bool = False):
        """Every stored row within `radius` of each query among the lists it probes
        (vdb_ivf_range_search; not in the reference). Returns (lims, distances, ids): query i
        owns entries [lims[i], lims[i + 1]), ascending by (distance, id) — search's entries for
        that query alone with d <= radius, however many there are. reserve: entries of the
        device hit buffer a batch starts with (0: automatic). screen=True serves the call through
        the screen the index holds at that moment (vdb_ivf_range_search_screened): the same
        result bit for bit, from a quarter or half of the bytes; without a live screen the exact
        scan serves."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dimension)
        n = q.shape[0]
        L = lib()
        r = ctypes.c_void_p()
        if screen:
            _check(L.vdb_ivf_range_search_screened(self._h, None, _ptr(q), n, nprobe, float(radius), reserve,
                                                   ctypes.byref(r)))
        else:
            _check(L.vdb_ivf_range_search(self._h, _ptr(q), n, nprobe, float(radius), reserve, ctypes.byref(r)))
        return self._take_range_result(r, n)

    @staticmethod
    def _take_range_result(r, n: int):
        """A vdb_range_result into (lims, distances, ids) arrays of the caller's, then released."""
        L = lib()
        try:
            lims = np.ctypeslib.as_array(ctypes.cast(L.vdb_range_result_lims(r), ctypes.POINTER(ctypes.c_uint64)),
                                         shape=(n + 1,)).copy()
            total = int(lims[n])
            if total:
                D = np.ctypeslib.as_array(ctypes.cast(L.vdb_range_result_distances(r), ctypes.POINTER(ctypes.c_float)),
                                          shape=(total,)).copy()
                I = np.ctypeslib.as_array(ctypes.cast(L.vdb_range_result_ids(r), ctypes.POINTER(ctypes.c_uint64)),
                                          shape=(total,)).copy()
            else:
                D, I = np.empty(0, dtype=np.float32), np.empty(0, dtype=np.uint64)
        finally:
            L.vdb_range_result_free(r)
        return lims, D, I

    def range_last_timing(self) -> dict:
        """The calling thread's latest range_search by step (vdb_range_last_timing)."""
        a, b = ctypes.c_double(0), ctypes.c_double(0)
        p, h, r = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
        _check(lib().vdb_range_last_timing(ctypes.byref(a), ctypes.byref(b), ctypes.byref(p), ctypes.byref(h),
                                           ctypes.byref(r)))
        return {"scan_ms": a.value, "order_ms": b.value, "pairs_scanned": p.value, "hits": h.value, "reruns": r.value}

    def range_screen_last_timing(self) -> dict:
        """The calling thread's latest range_search(..., screen=True) by step (vdb_range_screen_last_timing)."""
        a, b, c = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
        p, m = ctypes.c_uint64(0), ctypes.c_uint64(0)
        sb, eb = ctypes.c_uint32(0), ctypes.c_uint32(0)
        _check(lib().vdb_range_screen_last_timing(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(p),
                                                  ctypes.byref(m), ctypes.byref(sb), ctypes.byref(eb)))
        return {"pairs_ms": a.value, "bound_ms": b.value, "recheck_ms": c.value, "pairs_bounded": p.value,
                "candidates": m.value, "screened_batches": sb.value, "exact_batches": eb.value}

    def search_device(self, q_ptr: int, n: int, nprobe: int, k: int, d_ptr: int, i_ptr: int,
                      stream: int | None = None):
        _check(lib().vdb_ivf_search_device(self._h, ctypes.c_void_p(q_ptr), n, nprobe, k, ctypes.c_void_p(d_ptr),
                                           ctypes.c_void_p(i_ptr), ctypes.c_void_p(stream or 0)))

    def search_batch(self, queries, params, distances, indices):
        """search_batch (ivf_flat_index.h:55-58; declared, never defined in the reference)."""
        for q, p, d, i in zip(queries, params, distances, indices):
            D, I = self.search(q, p)
            d[...] = D.reshape(d.shape)
            i[...] = I.reshape(i.shape)

    # ---- persistence (IVFFlatIndex::save/load, ivf_flat_index.h:66-67) ----
    def save(self, path: str):
        _check(lib().vdb_ivf_save(self._h, os.fsencode(path)))

    def load(self, path: str):
        _check(lib().vdb_ivf_load(self._h, os.fsencode(path)))

    def get_dimension(self) -> int:
        return self.config.dimension

    # ---- sharding ----
    def set_shard(self, rank: int, world: int, owners=None):
        """Keep rank's lists of `world` (the LPT plan, or an explicit `owners` array)."""
        if owners is None:
            _check(lib().vdb_ivf_set_shard(self._h, rank, world))
        else:
            o = np.ascontiguousarray(owners, dtype=np.uint32)
            _check(lib().vdb_ivf_set_shard_owners(self._h, rank, world, _ptr(o)))

    def probe_census(self, rows_ptr: int, n: int, nprobe: int) -> np.ndarray:
        """Per list: how many of n device rows probe it (vdb_ivf_probe_census)."""
        out = np.empty(self.config.nlist, dtype=np.uint64)
        _check(lib().vdb_ivf_probe_census(self._h, ctypes.c_void_p(rows_ptr), n, nprobe, _ptr(out)))
        return out

    def attach_comm(self, comm_id: bytes, rank: int, world: int):
        """Join the RCCL communicator `comm_id` as `rank` of `world` (after set_shard /
        plan_shard with the same rank and world): searches then return final results."""
        if len(comm_id) != COMM_ID_BYTES:
            raise ValueError("comm_id must be COMM_ID_BYTES long")
        _check(lib().vdb_ivf_attach_comm(self._h, ctypes.c_char_p(comm_id), rank, world))

    def detach_comm(self):
        _check(lib().vdb_ivf_detach_comm(self._h))

    def comm_status(self):
        """(error message or None, exchanges issued, exchanges completed) of the attached
        communicator (vdb_ivf_comm_status)."""
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = lib().vdb_ivf_comm_status(self._h, ctypes.byref(a), ctypes.byref(b))
        return (lib().vdb_last_error().decode() if rc != 0 else None), a.value, b.value

    @property
    def group_size(self) -> int:
        return int(lib().vdb_ivf_group_size(self._h))

    def list_owners(self) -> np.ndarray:
        """Per list: the member (group) or rank (shard) storing it; 2**32 - 1 = none."""
        out = np.empty(self.config.nlist, dtype=np.uint32)
        _check(lib().vdb_ivf_list_owners(self._h, _ptr(out)))
        return out

    def plan_shard(self, rank: int, world: int, final_sizes, owners=None):
        """Sharded build: fix this rank's lists from the final list sizes before any add
        (the LPT plan, or an explicit `owners` array)."""
        s = np.ascontiguousarray(final_sizes, dtype=np.uint64)
        if len(s) != self.config.nlist:
            raise ValueError("final_sizes needs one entry per list")
        if owners is None:
            _check(lib().vdb_ivf_plan_shard(self._h, rank, world, _ptr(s)))
        else:
            o = np.ascontiguousarray(owners, dtype=np.uint32)
            _check(lib().vdb_ivf_plan_shard_owners(self._h, rank, world, _ptr(s), _ptr(o)))

    # ---- residency / stats ----
    def warmup_lists(self, list_ids):
        a = np.ascontiguousarray(list_ids, dtype=np.uint32)
        _check(lib().vdb_ivf_warmup(self._h, _ptr(a), len(a)))

    def evict_list(self, list_id: int):
        _check(lib().vdb_ivf_evict(self._h, list_id))

    def get_gpu_memory_usage(self) -> int:
        """Bytes of the GPU-resident lists, count * (dim * 4 + 8) each (ivf_flat_index.cpp:393-443)."""
        return int(lib().vdb_ivf_gpu_bytes(self._h))

    def gpu_bytes_allocated(self) -> int:
        """HBM really held for lists (padded 64-row blocks, whole cache in the tier) and centroids."""
        return int(lib().vdb_ivf_gpu_bytes_allocated(self._h))

    def get_total_vectors(self) -> int:
        return int(lib().vdb_ivf_ntotal(self._h))

    def list_sizes(self) -> np.ndarray:
        out = np.empty(self.config.nlist, dtype=np.uint64)
        _check(lib().vdb_ivf_list_sizes(self._h, _ptr(out)))
        return out

    def get_list(self, list_id: int):
        n = int(self.list_sizes()[list_id])
        v = np.empty((n, self.dimension), dtype=np.float32)
        i = np.empty(n, dtype=np.uint64)
        _check(lib().vdb_ivf_get_list(self._h, list_id, _ptr(v), _ptr(i)))
        return v, i

    def get_list_into(self, list_id: int, vectors: np.ndarray, ids: np.ndarray):
        """Copy list `list_id` into caller arrays (C-contiguous, sized count x dim / count)."""
        assert vectors.flags.c_contiguous and ids.flags.c_contiguous
        assert vectors.dtype == np.float32 and ids.dtype == np.uint64
        _check(lib().vdb_ivf_get_list(self._h, list_id, _ptr(vectors), _ptr(ids)))

    def set_batch(self, batch: int):
        _check(lib().vdb_ivf_set_batch(self._h, batch))

    def set_stale_slots(self, enable: bool):
        _check(lib().vdb_ivf_set_stale_slots(self._h, int(enable)))

    def set_coarse_mode(self, mode: int):
        """1: MFMA bounds + exact re-rank (default); 0: exact VALU coarse distances."""
        _check(lib().vdb_ivf_set_coarse_mode(self._h, mode))

    def set_option(self, name: str, value: int):
        """Engine option (vdb_ivf_set_option): tuning knobs and residency; never changes results."""
        _check(lib().vdb_ivf_set_option(self._h, name.encode(), int(value)))

    def coalesce_stats(self):
        """(device batches, search() calls served) of the host-API coalescing queue."""
        b, r = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(lib().vdb_ivf_coalesce_stats(self._h, ctypes.byref(b), ctypes.byref(r)))
        return b.value, r.value

    def open_lists(self, path: str):
        """Serve the lists from an index file written by save() through the list-cache
        tier (set_option("list_cache_bytes", n) first); the handle becomes read-only."""
        _check(lib().vdb_ivf_open_lists(self._h, path.encode()))

    def cache_stats(self) -> dict:
        """List-cache tier counters (option list_cache_bytes; capacity 0 = tier off)."""
        st = CacheStats()
        _check(lib().vdb_ivf_cache_stats(self._h, ctypes.byref(st)))
        return st.as_dict()

    def fill_row_cache(self, weights=None):
        """Screened tier, file home: refill the row cache by expected survivor rows per vector
        (weights per list, e.g. survivor_histogram()) or by list size (None)."""
        if weights is None:
            _check(lib().vdb_ivf_fill_row_cache(self._h, None))
        else:
            c = np.ascontiguousarray(weights, dtype=np.uint64)
            if c.shape != (self.config.nlist,):
                raise ValueError("weights needs one entry per list")
            _check(lib().vdb_ivf_fill_row_cache(self._h, _ptr(c)))

    def survivor_histogram(self) -> np.ndarray:
        """Per list: the survivor rows the screened tier's batches needed so far."""
        out = np.zeros(self.config.nlist, dtype=np.uint64)
        _check(lib().vdb_ivf_survivor_histogram(self._h, _ptr(out)))
        return out

    def collect_stamps(self):
        """(option collect_stamps) the collect kernel's item timeline: (records [n, 4] uint64,
        wall clock Hz); resets the buffer."""
        n, hz = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(lib().vdb_ivf_collect_stamps(self._h, None, 0, ctypes.byref(n), ctypes.byref(hz)))
        out = np.zeros((n.value, 4), dtype=np.uint64)
        if n.value:
            _check(lib().vdb_ivf_collect_stamps(self._h, out.ctypes.data, n.value, ctypes.byref(n), ctypes.byref(hz)))
        return out, hz.value

    _SNAPSHOT = {"probes": (np.uint32, ()), "sorted_pair": (np.uint32, ()), "counters": (np.uint32, ()),
                 "cand": (np.uint32, (4,)), "ovf": (np.uint32, ()), "thr": (np.uint32, ()), "thr4": (np.uint32, (4,)),
                 "ublist": (np.float32, ()), "ubcnt": (np.uint32, ()), "scnt": (np.uint32, ()),
                 "soff": (np.uint32, ()), "surv": (np.uint32, (2,)), "pst": (np.float32, (4,)),
                 "qscale": (np.float32, ()), "qres": (np.uint8, ()), "block_off": (np.uint64, ()),
                 "count": (np.uint32, ()), "meta": (np.float32, (4,)), "sscale": (np.float32, ()),
                 "shadow": (np.uint8, ())}
    _SNAPSHOT_SCALARS = ("B", "P", "k", "dp", "seg_blocks", "segs_item", "wide_q", "cand_cap", "i8", "metric",
                         "grid", "nlist", "blocks", "ub_lists", "cand_chunk", "dim", "slot", "cand_alloc")

    def screen_snapshot_raw(self, name: str, dtype) -> np.ndarray:
        """One named buffer of vdb_ivf_screen_snapshot as a flat array of dtype ("cand_alloc": the
        slot's whole candidate allocation, not part of screen_snapshot())."""
        n = ctypes.c_uint64(0)
        _check(lib().vdb_ivf_screen_snapshot(self._h, name.encode(), None, 0, ctypes.byref(n)))
        out = np.zeros(n.value // np.dtype(dtype).itemsize, dtype=dtype)
        if n.value:
            _check(lib().vdb_ivf_screen_snapshot(self._h, name.encode(), out.ctypes.data, n.value, ctypes.byref(n)))
        return out

    def screen_snapshot(self) -> dict:
        """(diagnostics) every buffer of the most recently issued deferred screened batch (rows in
        HBM) and the handle's screen data, as numpy arrays, plus the batch's scalars as ints
        (vdb_ivf_screen_snapshot; include/vdb_ivf.h has the layouts). thr / thr4 keep their
        order-preserving encoding; qres and shadow are raw bytes. Changes nothing."""
        fetch = self.screen_snapshot_raw
        snap = {k: int(v) for k, v in zip(self._SNAPSHOT_SCALARS, fetch("scalars", np.uint64))}
        for name, (dtype, tail) in self._SNAPSHOT.items():
            snap[name] = fetch(name, dtype).reshape((-1,) + tail)
        snap["ublist"] = snap["ublist"].reshape(snap["B"] * snap["P"], snap["ub_lists"], snap["k"])
        return snap

    def coarse_snapshot(self, rows, nprobe: int = 0, assign: bool = False) -> dict:
        """(diagnostics) the coarse step's buffers for `rows` (vdb_ivf_coarse_snapshot): "approx" and
        "delta" f32 [n, nlist], the matrix-core distances and their error bounds; with nprobe > 0
        "cand" u32 [n, nlist] (row i: its candidate lists in any order, then 0xFFFFFFFF) and "probes"
        u32 [n, min(nprobe, nlist)]; with assign "assign" u32 [n]. Changes nothing."""
        r = np.ascontiguousarray(rows, dtype=np.float32)
        if r.ndim != 2 or r.shape[1] != self.dimension:
            raise ValueError("rows must be [n, dim]")
        n, nlist = r.shape[0], self.config.nlist
        out = {"approx": np.empty((n, nlist), np.float32), "delta": np.empty((n, nlist), np.float32)}
        if nprobe > 0:
            out["cand"] = np.empty((n, nlist), np.uint32)
            out["probes"] = np.empty((n, min(nprobe, nlist)), np.uint32)
        if assign:
            out["assign"] = np.empty(n, np.uint32)
        ptr = {k: _ptr(v) for k, v in out.items()}
        _check(lib().vdb_ivf_coarse_snapshot(self._h, _ptr(r), n, nprobe, ptr["approx"], ptr["delta"], ptr.get("cand"),
                                             ptr.get("probes"), ptr.get("assign")))
        return out

    def profile_enable(self, on: bool = True):
        _check(lib().vdb_ivf_profile_enable(self._h, int(on)))

    def profile_reset(self):
        _check(lib().vdb_ivf_profile_reset(self._h))

    def profile_read(self) -> dict:
        p = Profile()
        _check(lib().vdb_ivf_profile_read(self._h, ctypes.byref(p)))
        return p.as_dict()

    def synchronize(self):
        _check(lib().vdb_ivf_synchronize(self._h))

    @property
    def stream(self) -> int:
        return int(lib().vdb_ivf_stream(self._h) or 0)
