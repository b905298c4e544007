"""GPU: vdb_ivf_search_prepared_multi_screened (per-query prepared filters served through the
screen) against vdb_ivf_search_prepared_multi on the same handle, the CPU oracle holding only a
filter's rows, and the single-filter screened call's candidate counts.

The fixture and the handles are test_gpu_range_screen.py's (40 queries; nprobe 5 = nlist: every
list's pairs form items of 16, 16 and 8; the hub in two segments). Filter tables: `mix` (all, half,
other half, sparse, none; filter i % 5), `runs` (the same filters in contiguous runs that end and
start off the boundaries of batches of 8, in request and in scanned order), `sixteen` (16 disjoint
INCLUDE filters, ids = j mod 16: every row of an item's MFMA operand under another mask) and `one`
(one filter for all). Parity cases pass reserve = 1 << 17, room for every (query, row) pair of the
fixture (about 85 K), so the route under test does not rest on a candidate count."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
from conftest import load_vdb
from test_gpu_filter_screen import NOIDS, assert_same, filter_sets
from test_gpu_range_screen import NPROBE, NQ, PARENT_BUILD_ID, fixture, handle, make

vdb = load_vdb()
pytestmark = pytest.mark.gpu

ROOM = 1 << 17
RUNS = np.repeat([3, 0, 4, 1, 2], [6, 9, 3, 12, 10]).astype(np.uint32)  # scanned order: runs end at 9, 21, 31, 37


def table_specs(fx, name):
    """(specs, filter_of); specs[f] = (ids, include)."""
    s = filter_sets(fx)
    five = [s["all"], s["half"], (s["half"][0], True), s["sparse"], s["none"]]
    i = np.arange(NQ, dtype=np.uint32)
    if name == "mix":
        return five, i % 5
    if name == "runs":
        return five, RUNS
    if name == "sixteen":
        return [(fx["ids"][fx["ids"] % np.uint64(16) == j], True) for j in range(16)], i % 16
    return [s["half"]], i * 0


@functools.lru_cache(maxsize=None)
def prepared(dim, metric, i8, kind, name):
    """(the shared read-only handle, the table's filters on it, filter_of), prepared once."""
    specs, fo = table_specs(fixture(dim, kind), name)
    g = handle(dim, metric, i8, kind)
    return g, [g.prepare_filter(ids, include=inc) for ids, inc in specs], fo


@functools.lru_cache(maxsize=None)
def oracle_search(dim, metric, name, f, k):
    """Filter f's queries, in call order, on an oracle that holds only the rows filter f allows."""
    fx = fixture(dim)
    specs, fo = table_specs(fx, name)
    allow = np.isin(fx["ids"], specs[f][0]) == specs[f][1]
    o = oracle.OracleIndex(dim, 5, metric)
    o.centroids = fx["C"]
    for l in range(5):
        m = (fx["assign"] == l) & allow
        o.set_list(l, fx["X"][m], fx["ids"][m])
    return o.search(fx["Q"][fo == f], NPROBE, k)


def both(g, Q, flts, fo, k, **kw):
    ex = g.search_prepared_multi(Q, flts, fo, nprobe=NPROBE, k=k)
    sc = g.search_prepared_multi(Q, flts, fo, nprobe=NPROBE, k=k, screen=True, **kw)
    return ex, sc, g.filter_screen_last_timing()


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("kind", ["plain", "special", "ties"])
@pytest.mark.parametrize("dim", [64, 200])
@pytest.mark.parametrize("i8", [1, 0])
@pytest.mark.parametrize("metric", [0, 1, 3])
def test_parity(metric, i8, dim, kind, k):
    fx = fixture(dim, kind)
    for name in ("mix", "runs", "sixteen", "one"):
        g, flts, fo = prepared(dim, metric, i8, kind, name)
        ex, sc, st = both(g, fx["Q"], flts, fo, k, reserve=ROOM)
        assert_same(sc, ex)
        assert st["screened_batches"] == 1 and st["exact_batches"] == 0, (name, st)
        assert st["pairs_bounded"] == sum(flts[f].allowed for f in fo), (name, st)  # (every list is probed)
        assert st["candidates"] <= st["pairs_bounded"]
        if kind == "plain" and metric != 3:
            for f in range(len(flts)):
                D, I = oracle_search(dim, metric, name, f, k)
                assert_same((sc[0][fo == f], sc[1][fo == f]), (D, I))


@pytest.mark.parametrize("name", ["mix", "sixteen"])
@pytest.mark.parametrize("i8", [1, 0])
@pytest.mark.parametrize("metric", [0, 1])
def test_the_threshold_is_the_pairs_own(metric, i8, name):
    """A (pair, slot) bound depends on that pair's A row and the slot's shadow only and tau is the
    exact k-th smallest, so the mixed call keeps exactly the candidates the single-filter screened
    call (the parent's kernels) keeps for each filter's queries."""
    fx = fixture(200)
    g, flts, fo = prepared(200, metric, i8, "plain", name)
    for k in (1, 10):
        _, _, st = both(g, fx["Q"], flts, fo, k, reserve=ROOM)
        per = 0
        for f, flt in enumerate(flts):
            g.search_prepared(fx["Q"][fo == f], flt, nprobe=NPROBE, k=k, screen=True, reserve=ROOM)
            per += g.filter_screen_last_timing()["candidates"]
        print("metric %d i8 %d %s k %d: %d candidates, per filter %d" % (metric, i8, name, k, st["candidates"], per))
        assert st["candidates"] == per


@pytest.mark.parametrize("stale", [0, 1])
@pytest.mark.parametrize("i8", [1, 0])
def test_batches_and_carry(i8, stale):
    fx = fixture(200)
    g = make(fx, 0, i8)
    g.set_stale_slots(bool(stale))
    specs, fo = table_specs(fx, "runs")
    flts = [g.prepare_filter(ids, include=inc) for ids, inc in specs]
    whole = g.search_prepared_multi(fx["Q"], flts, fo, nprobe=NPROBE, k=10)
    g.set_batch(8)
    ex, sc, st = both(g, fx["Q"], flts, fo, 10)  # (the default reserve)
    assert_same(ex, whole)
    assert_same(sc, whole)
    assert st["screened_batches"] + st["exact_batches"] == 5, st


@pytest.mark.parametrize("i8", [1, 0])
def test_fallback(i8):
    fx = fixture(64)
    g, flts, fo = prepared(64, 1, i8, "plain", "mix")
    ex, sc, st = both(g, fx["Q"], flts, fo, 10, reserve=1)
    assert_same(sc, ex)
    assert st["exact_batches"] == 1 and st["screened_batches"] == 0 and st["candidates"] > 1


@pytest.mark.parametrize("why", ["fresh", "after_add"])
def test_without_a_live_screen_the_exact_call_serves(why):
    fx = fixture(64)
    g = make(fx, 0, 1, live=why != "fresh")
    if why == "after_add":
        g.add_to_lists(fx["X"][:3] + np.float32(0.25), np.array([7, 8, 9], np.uint64), np.array([1, 2, 3], np.uint32))
    specs, fo = table_specs(fx, "mix")
    flts = [g.prepare_filter(ids, include=inc) for ids, inc in specs]
    before = g.gpu_bytes_allocated()
    ex, sc, st = both(g, fx["Q"], flts, fo, 10)
    assert_same(sc, ex)
    assert st["screened_batches"] == 0 and st["exact_batches"] == 1 and st["pairs_bounded"] == 0, st
    assert g.gpu_bytes_allocated() == before


def test_handle_is_left_as_found():
    fx = fixture(64)
    g = make(fx, 0, 1)
    specs, fo = table_specs(fx, "sixteen")
    flts = [g.prepare_filter(ids, include=inc) for ids, inc in specs]
    D0, I0 = g.search(fx["Q"], nprobe=NPROBE, k=10)
    before = g.gpu_bytes_allocated()
    ex, sc, st = both(g, fx["Q"], flts, fo, 10, reserve=ROOM)
    assert_same(sc, ex)
    assert st["screened_batches"] == 1
    assert g.gpu_bytes_allocated() == before and not any(f.stale for f in flts)
    D1, I1 = g.search(fx["Q"], nprobe=NPROBE, k=10)
    assert D0.tobytes() == D1.tobytes() and I0.tobytes() == I1.tobytes()
    assert g.filter_last_timing()["pairs_scanned"] == sum(flts[f].allowed for f in fo)
    assert vdb.build_id() == PARENT_BUILD_ID


def test_refusals():
    fx = fixture(64)
    g, other = make(fx, 0, 1), make(fx, 0, 1)
    mine, theirs = g.prepare_filter(fx["ids"][:50], include=True), other.prepare_filter(NOIDS, include=False)
    Q, fo = np.ascontiguousarray(fx["Q"]), np.arange(NQ, dtype=np.uint32) % 2
    D, I = np.full((NQ, 65), 7, np.float32), np.full((NQ, 65), 7, np.uint64)

    def call(flts, fo, k):
        tab = (ctypes.c_void_p * len(flts))(*[f._f.value for f in flts])
        rc = vdb.lib().vdb_ivf_search_prepared_multi_screened(g._h, tab, len(flts), fo.ctypes.data, Q.ctypes.data, NQ,
                                                              NPROBE, k, 0, D.ctypes.data, I.ctypes.data)
        assert (D == 7).all() and (I == 7).all()  # the outputs are not written
        return rc

    assert call([mine, theirs], fo, 10) == -1  # VDB_ERR_INVALID_ARGUMENT: another handle's filter
    assert call([mine, mine], fo + np.uint32(1), 10) == -1  # filter_of[i] >= n_filters
    assert call([mine, mine], fo, 65) == -4  # VDB_ERR_UNSUPPORTED
    g.add(fx["X"][:2] + np.float32(0.5), np.array([5, 6], np.uint64))
    assert mine.stale and call([mine, mine], fo, 10) == -5  # VDB_ERR_STATE
