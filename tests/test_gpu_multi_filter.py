"""GPU: per-query prepared filters (vdb_ivf_search_prepared_multi) against the CPU oracle.

Definition under test. For every filter index f, the rows of the queries S_f that name it are
what vdb_ivf_search returns, for the queries of S_f in call order, on a handle with the same
centroids that holds only the rows filter f allows: the mixed call equals the per-filter calls
scattered back into request order, and the stale-slot reuse never crosses filters. So every
expected value comes from an OracleIndex whose lists are set_list to the rows filter f allows,
searched with the queries of S_f in order (one by one with stale_slots off), never from the
library; the tests also check equality with the library's own search_prepared per filter group.

Shape (that of test_gpu_prepared.py): 2,940 rows placed with add_to_lists into nlist = 12 lists
of 0, 1, 63, 64, 65, 130 rows, one hub list of 1,500 rows (24 blocks: every wave of a workgroup
and two segments of 12 blocks) and five more of a few blocks each; dimensions 20 (padded) and
128; 40 queries. Ten ids are stored twice, in two different lists.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle
from conftest import load_vdb

vdb = load_vdb()
pytestmark = pytest.mark.gpu

NLIST, NQ = 12, 40
LENS = [0, 1, 63, 64, 65, 130, 1500, 257, 320, 200, 191, 149]
HUB = 6
N = sum(LENS)
TAIL = 300  # rows of the second add in the "stale" layout
NONE = np.iinfo(np.uint64).max
FMAX = np.finfo(np.float32).max
EXCLUDE, INCLUDE = False, True
INVALID, UNSUPPORTED, STATE = -1, -4, -5
SHAPES = [(5, 10), (12, 64), (12, 1)]  # (nprobe, k)
_data = {}
_oracles = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(D, I, Dr, Ir):
    assert I.shape == Ir.shape
    bad = np.argwhere(I != Ir)
    assert bad.size == 0, f"ids differ at {bad[:5].tolist()}: gpu {I[tuple(bad[0])]} ref {Ir[tuple(bad[0])]}"
    badd = np.argwhere(bits(D) != bits(Dr))
    assert badd.size == 0, f"dist bits differ at {badd[:5].tolist()}: gpu {D[tuple(badd[0])]!r} ref {Dr[tuple(badd[0])]!r}"


def data(dim):
    """(X, Q, ids, lists, C) computed once per dimension and never changed. Row r goes to list
    lists[r]; the rows of a list keep their global order."""
    if dim not in _data:
        X, Q, ids = oracle.reference_test_data(N, NQ, dim, seed=2000 + dim)
        C = oracle.gen_normal(3000 + dim, NLIST * dim).reshape(NLIST, dim)
        rng = np.random.RandomState(dim)
        lists = rng.permutation(np.repeat(np.arange(NLIST, dtype=np.uint32), LENS))
        ids = ids.copy() * 3 + 7
        # ten ids stored twice: the first ten rows of the last list carry the ids of ten hub rows
        hub_rows = np.flatnonzero(lists == HUB)[100:110]
        ids[np.flatnonzero(lists == NLIST - 1)[:10]] = ids[hub_rows]
        for a in (X, Q, ids, lists, C):
            a.setflags(write=False)
        _data[dim] = (X, Q, ids, lists, C)
    return _data[dim]


def make(dim, metric=0, layout="il", **cfg):
    """A handle in one of the three list layouts a prepared call can meet."""
    X, Q, ids, lists, C = data(dim)
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, NLIST, vdb.Metric(metric), **cfg))
    g.centroids = C
    if layout == "il":  # the interleaved arena
        g.set_option("screen", 0)
        g.add_to_lists(X, ids, lists)
    elif layout == "rows":  # the screen built: its row-major copy is the lists' only fp32 copy
        g.add_to_lists(X, ids, lists)
        g.search(Q, nprobe=5, k=10)
        if metric in (0, 1):  # (no screen for Cosine: its lists stay interleaved)
            assert g.profile_read()["screen_shadow"] in (1, 2)
    else:  # "stale": right after an add, no search since
        g.add_to_lists(X[:N - TAIL], ids[:N - TAIL], lists[:N - TAIL])
        g.search(Q, nprobe=5, k=10)
        g.add_to_lists(X[N - TAIL:], ids[N - TAIL:], lists[N - TAIL:])
    assert g.list_sizes().tolist() == LENS
    return g


def allowed_rows(ids, flt, include):
    hit = np.isin(ids, np.asarray(flt, dtype=np.uint64))
    return hit if include else ~hit


def oracle_of(dim, metric, key, allow):
    """The oracle holding only the rows of `allow`, built once per (dim, metric, key)."""
    kk = (dim, metric, key)
    if kk not in _oracles:
        X, _, ids, lists, C = data(dim)
        o = oracle.OracleIndex(dim, NLIST, metric)
        o.centroids = C
        for l in range(NLIST):
            rows = np.flatnonzero((lists == l) & allow)
            o.set_list(l, X[rows], ids[rows])
        _oracles[kk] = o
    return _oracles[kk]


def expect(dim, metric, specs, filter_of, Q, nprobe, k, stale=True):
    """The definition: per filter f its oracle searched with the queries of S_f in call order
    (stale_slots off: one by one), scattered back. specs[f] = (key, ids, include)."""
    ids = data(dim)[2]
    filter_of = np.asarray(filter_of)
    D = np.empty((Q.shape[0], k), np.float32)
    I = np.empty((Q.shape[0], k), np.uint64)
    for f, (key, f_ids, inc) in enumerate(specs):
        S = np.flatnonzero(filter_of == f)
        if S.size == 0:
            continue
        o = oracle_of(dim, metric, key, allowed_rows(ids, f_ids, inc))
        if stale:
            D[S], I[S] = o.search(Q[S], nprobe, k)
        else:
            for i in S:
                D[i:i + 1], I[i:i + 1] = o.search(Q[i:i + 1], nprobe, k)
    return D, I


def per_group(g, flts, filter_of, Q, nprobe, k):
    """The library's own search_prepared per filter group, scattered back."""
    filter_of = np.asarray(filter_of)
    D = np.empty((Q.shape[0], k), np.float32)
    I = np.empty((Q.shape[0], k), np.uint64)
    for f, flt in enumerate(flts):
        S = np.flatnonzero(filter_of == f)
        if S.size:
            D[S], I[S] = g.search_prepared(Q[S], flt, nprobe=nprobe, k=k)
    return D, I


def three(dim):
    ids = data(dim)[2]
    return [("exclude 50%", ids[::2], EXCLUDE), ("include 1%", ids[5::97], INCLUDE),
            ("include nothing", np.empty(0, np.uint64), INCLUDE)]


def prepare(g, specs):
    return [g.prepare_filter(f_ids, include=inc) for _, f_ids, inc in specs]


# ---- 1. one filter for all queries: the prepared call, bit for bit ----
@pytest.mark.parametrize("dim", [20, 128])
@pytest.mark.parametrize("layout", ["il", "rows", "stale"])
@pytest.mark.parametrize("metric", [0, 1, 2, 3])
def test_one_filter_for_all(metric, layout, dim):
    X, Q, ids, lists, C = data(dim)
    g = make(dim, metric, layout)
    specs = three(dim)[:2]
    flts = prepare(g, specs)
    for stale in (True, False):
        g.set_stale_slots(stale)
        for f, flt in enumerate(flts):
            for nprobe, k in SHAPES:
                D, I = g.search_prepared_multi(Q, [flt], np.zeros(NQ, np.uint32), nprobe=nprobe, k=k)
                assert D.dtype == np.float32 and I.dtype == np.uint64 and D.shape == (NQ, k)
                Dp, Ip = g.search_prepared(Q, flt, nprobe=nprobe, k=k)
                assert_same(D, I, Dp, Ip)
                if metric != 3:  # (CosineDistance: the oracle's side is test_gpu_cosine.py's, through search_prepared)
                    assert_same(D, I, *expect(dim, metric, [specs[f]], np.zeros(NQ, int), Q, nprobe, k, stale))
    # the same filter twice in the table, and an entry no query names
    fo = (np.arange(NQ) % 2).astype(np.uint32)
    D, I = g.search_prepared_multi(Q, [flts[0], flts[0], flts[1]], fo, nprobe=5, k=10)
    assert_same(D, I, *per_group(g, [flts[0], flts[0]], fo, Q, 5, 10))


# ---- 2. three filters interleaved: no carry crosses filters ----
@pytest.mark.parametrize("dim", [20, 128])
@pytest.mark.parametrize("layout", ["il", "rows", "stale"])
@pytest.mark.parametrize("stale", [True, False], ids=["stale_slots", "no_stale_slots"])
def test_three_filters_interleaved(stale, layout, dim):
    X, Q, ids, lists, C = data(dim)
    fo = (np.arange(NQ) % 3).astype(np.uint32)
    for metric in (0, 1, 2):
        g = make(dim, metric, layout)
        g.set_stale_slots(stale)
        specs = three(dim)
        flts = prepare(g, specs)
        for nprobe, k in SHAPES:
            D, I = g.search_prepared_multi(Q, flts, fo, nprobe=nprobe, k=k)
            # the include-nothing group stays entirely unfilled while its neighbours fill their slots
            assert np.all(I[fo == 2] == NONE) and np.all(D[fo == 2] == FMAX)
            assert np.all(I[fo == 0][:, 0] != NONE)
            assert_same(D, I, *expect(dim, metric, specs, fo, Q, nprobe, k, stale))
            assert_same(D, I, *per_group(g, flts, fo, Q, nprobe, k))


# ---- 3. one filter per query: four different masks inside a hub item ----
@pytest.mark.parametrize("dim", [20, 128])
@pytest.mark.parametrize("layout", ["il", "rows"])
def test_one_filter_per_query(layout, dim):
    X, Q, ids, lists, C = data(dim)
    hub = ids[lists == HUB]  # the hub's rows in list order: block b holds hub[64 b : 64 b + 64]
    specs = []
    for j in range(NQ):
        b = j % 24
        f_ids = np.unique(np.concatenate([hub[64 * b:64 * b + 64], ids[j::40]]))
        specs.append((f"per-query {j}", f_ids, INCLUDE))
    fo = np.arange(NQ, dtype=np.uint32)
    g = make(dim, 0, layout)
    flts = prepare(g, specs)
    for stale in (True, False):
        g.set_stale_slots(stale)
        for nprobe, k in SHAPES:
            D, I = g.search_prepared_multi(Q, flts, fo, nprobe=nprobe, k=k)
            # (a filter of its own: no earlier query of the same filter, so stale or not is the same)
            assert_same(D, I, *expect(dim, 0, specs, fo, Q, nprobe, k, stale))
            for j in range(NQ):  # independently: nothing a query's own filter does not allow
                real = I[j][I[j] != NONE]
                assert np.all(np.isin(real, specs[j][1])), j
    assert np.all(I[:, 0] != NONE)  # (nprobe 12: the hub is probed, and every filter has rows there)


# ---- 4. tenant isolation: the same query vector under two disjoint filters, sharing an item ----
@pytest.mark.parametrize("layout", ["il", "rows"])
def test_same_query_two_disjoint_filters(layout):
    dim = 20
    X, Q, ids, lists, C = data(dim)
    u = np.unique(ids)
    specs = [("even unique ids", u[::2], INCLUDE), ("odd unique ids", u[1::2], INCLUDE)]
    g = make(dim, 0, layout)
    flts = prepare(g, specs)
    fo2 = np.array([0, 1], np.uint32)
    for i in (0, 7, 23):
        Q2 = np.ascontiguousarray(np.stack([Q[i], Q[i]]))  # both probe the same lists: every item holds both
        for nprobe, k in SHAPES:
            D, I = g.search_prepared_multi(Q2, flts, fo2, nprobe=nprobe, k=k)
            assert_same(D, I, *expect(dim, 0, specs, fo2, Q2, nprobe, k))
            a, b = I[0][I[0] != NONE], I[1][I[1] != NONE]
            assert a.size and b.size and np.intersect1d(a, b).size == 0
            assert np.all(np.isin(a, specs[0][1])) and np.all(np.isin(b, specs[1][1]))
    # the whole batch doubled, each vector at two adjacent positions
    QQ = np.ascontiguousarray(np.repeat(Q, 2, axis=0))
    fo = (np.arange(2 * NQ) % 2).astype(np.uint32)
    D, I = g.search_prepared_multi(QQ, flts, fo, nprobe=5, k=10)
    assert_same(D, I, *expect(dim, 0, specs, fo, QQ, 5, 10))
    for j in range(2 * NQ):
        real = I[j][I[j] != NONE]
        assert np.all(np.isin(real, specs[j % 2][1]))


# ---- 5. segments: the fold goes by the pair's gate ----
@pytest.mark.parametrize("dim", [20, 128])
@pytest.mark.parametrize("layout", ["il", "rows"])
def test_segments(layout, dim):
    X, Q, ids, lists, C = data(dim)
    hub = ids[lists == HUB]
    specs = [("exclude the hub's first segment", hub[:768], EXCLUDE),
             ("exclude the hub's last 732 rows", hub[768:], EXCLUDE),
             ("include the hub's second segment only", hub[768:], INCLUDE)]
    fo = (np.arange(NQ) % 3).astype(np.uint32)
    g = make(dim, 0, layout)
    flts = prepare(g, specs)
    for nprobe, k in SHAPES:
        D, I = g.search_prepared_multi(Q, flts, fo, nprobe=nprobe, k=k)
        assert_same(D, I, *expect(dim, 0, specs, fo, Q, nprobe, k))
        assert_same(D, I, *per_group(g, flts, fo, Q, nprobe, k))


# ---- 6. the batch option ----
@pytest.mark.parametrize("layout", ["il", "rows"])
def test_batch_option(layout):
    dim = 20
    X, Q, ids, lists, C = data(dim)
    specs = three(dim)
    fo = (np.arange(NQ) % 3).astype(np.uint32)
    want = expect(dim, 0, specs, fo, Q, 5, 10)
    # a second pattern: runs of one filter longer than a batch, and a filter that comes back
    fo2 = np.array(([0] * 9 + [2] * 3 + [1] * 8) * 2, np.uint32)
    want2 = expect(dim, 0, specs, fo2, Q, 12, 10)
    out = []
    for batch in (1, 7, 64):
        g = make(dim, 0, layout)
        g.set_batch(batch)
        g.set_stale_slots(True)
        flts = prepare(g, specs)
        D, I = g.search_prepared_multi(Q, flts, fo, nprobe=5, k=10)
        assert_same(D, I, *want)
        D2, I2 = g.search_prepared_multi(Q, flts, fo2, nprobe=12, k=10)
        assert_same(D2, I2, *want2)
        out.append((D.tobytes(), I.tobytes(), D2.tobytes(), I2.tobytes()))
    assert out[0] == out[1] == out[2]


# ---- 7. refusals and side effects ----
def refused(g, flts, fo, Q, code, match, k=10):
    sizes = g.list_sizes().tolist()
    with pytest.raises(vdb.VdbError, match=match) as e:
        g.search_prepared_multi(Q, flts, fo, nprobe=5, k=k)
    assert e.value.code == code
    assert g.list_sizes().tolist() == sizes


def test_refusals_and_side_effects():
    dim = 20
    X, Q, ids, lists, C = data(dim)
    specs = three(dim)
    fo = (np.arange(NQ) % 3).astype(np.uint32)
    g, twin = make(dim, 0, "rows"), make(dim, 0, "rows")
    flts = prepare(g, specs)
    # a successful call: nothing built, refreshed or released
    before = g.gpu_bytes_allocated()
    shadow = g.profile_read()["screen_shadow"]
    D, I = g.search_prepared_multi(Q, flts, fo, nprobe=5, k=10)
    assert_same(D, I, *expect(dim, 0, specs, fo, Q, 5, 10))
    assert g.gpu_bytes_allocated() == before
    assert g.profile_read()["screen_shadow"] == shadow
    assert all(not f.stale for f in flts)
    assert_same(*g.search(Q, nprobe=5, k=10), *twin.search(Q, nprobe=5, k=10))
    # k = 65
    refused(g, flts, fo, Q, UNSUPPORTED, "k <= 64", k=65)
    # a filter of a second handle, named by no query
    other = twin.prepare_filter(ids[::2])
    refused(g, flts + [other], fo, Q, INVALID, "another handle")
    assert not other.stale
    # a closed filter: a null entry
    gone = g.prepare_filter(ids[::2])
    gone.close()
    refused(g, flts + [gone], fo, Q, INVALID, "null entry")
    # an index out of range
    refused(g, flts[:2], fo, Q, INVALID, "out of range")
    # after all these refusals the handle answers as before
    assert_same(*g.search_prepared_multi(Q, flts, fo, nprobe=5, k=10), D, I)
    assert_same(*g.search(Q, nprobe=5, k=10), *twin.search(Q, nprobe=5, k=10))
    # n == 0 and k == 0 succeed; nprobe == 0 and an empty index leave every slot unfilled
    D0, I0 = g.search_prepared_multi(np.empty((0, dim), np.float32), flts, np.empty(0, np.uint32), nprobe=5, k=10)
    assert D0.shape == (0, 10) and I0.shape == (0, 10)
    D0, I0 = g.search_prepared_multi(Q, flts, fo, nprobe=5, k=0)
    assert D0.shape == (NQ, 0)
    D0, I0 = g.search_prepared_multi(Q, flts, fo, nprobe=0, k=10)
    assert np.all(I0 == NONE) and np.all(D0 == FMAX)
    e = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, NLIST, vdb.Metric(0)))
    e.centroids = C
    fe = [e.prepare_filter(ids[:10], include=inc) for inc in (EXCLUDE, INCLUDE, EXCLUDE)]
    D0, I0 = e.search_prepared_multi(Q, fe, fo, nprobe=5, k=10)
    assert np.all(I0 == NONE) and np.all(D0 == FMAX)
    # a filter made stale by an add: refused even where no query names it
    X2, _, _ = oracle.reference_test_data(4, 1, dim, seed=91)
    old = g.prepare_filter(ids[::3])
    g.add_to_lists(X2, np.arange(10 ** 6, 10 ** 6 + 4, dtype=np.uint64), np.array([1, 3, 3, 7], dtype=np.uint32))
    assert old.stale
    fresh = prepare(g, specs)
    refused(g, fresh + [old], fo, Q, STATE, "stale")
    D1, I1 = g.search_prepared_multi(Q, fresh, fo, nprobe=5, k=10)  # (the fresh ones alone are served)
    assert_same(D1, I1, *per_group(g, fresh, fo, Q, 5, 10))
    # the list-cache tier
    t = make(dim, 0, "il", max_gpu_memory=0)
    ft = prepare(t, specs)
    t.set_option("list_cache_bytes", 60 * 64 * (128 * 4 + 8))  # room for every list
    assert t.cache_stats()["capacity_bytes"] > 0
    refused(t, ft, fo, Q, UNSUPPORTED, "list-cache tier")


# ---- 8. the timing ----
@pytest.mark.parametrize("layout", ["il", "rows"])
def test_filter_last_timing(layout):
    dim = 20
    X, Q, ids, lists, C = data(dim)
    specs = three(dim)
    fo = (np.arange(NQ) % 3).astype(np.uint32)
    g = make(dim, 0, layout)
    g.set_batch(7)  # (summed over the batches)
    flts = prepare(g, specs)
    o = oracle.OracleIndex(dim, NLIST, 0)
    o.centroids = C
    allow = [allowed_rows(ids, f_ids, inc) for _, f_ids, inc in specs]
    for nprobe in (5, 12):
        g.search_prepared_multi(Q, flts, fo, nprobe=nprobe, k=10)
        t = g.filter_last_timing()
        want = sum(int(allow[fo[i]][lists == l].sum()) for i in range(NQ) for l in o.select_nprobe(Q[i], nprobe))
        assert t["mark_ms"] == 0.0
        assert t["pairs_scanned"] == want
        assert t["scan_ms"] > 0.0 and t["merge_ms"] > 0.0


# ---- 9. the drop-in C++ class ----
def test_cpp_class_multi_filter():
    cpp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    exe = os.path.join(cpp, "bin", "multi_filter_test")
    subprocess.check_call(["make", "-s", "-C", cpp, exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "mixed batch bit-identical to search_prepared per filter group: yes" in p.stdout
    assert "include-nothing group unfilled: yes" in p.stdout
