"""GPU: vdb_ivf_range_search (all rows within a radius through a thresholded exact scan) against
the CPU oracle.

Definition under test: for each query on its own, a range search returns every entry (d, id) of
the result a plain search gives that single query with the same nprobe and a k no smaller than
the rows it probes, keeping id != UINT64_MAX and d <= radius, in that result's order. So the
expected answer for query i is OracleIndex.search(Q[i:i+1], nprobe, k=stored rows), cut by
(I != NONE) & (D <= radius); lims, ids and distance bits must match it.

Shape (that of test_gpu_filter.py): 2,940 rows placed with add_to_lists into nlist = 12 lists of
0, 1, 63, 64, 65, 130 rows, one hub list of 1,500 rows (24 blocks: every wave of a workgroup and
two segments) and five more of a few blocks each; dimensions 20 (padded) and 128; 40 queries.
Ten ids are stored twice, in two different lists.
"""
import ctypes
import functools
import os
import subprocess
import threading

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
INF = np.float32(np.inf)
_data = {}
_full = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, ref):
    (l, D, I), (lr, Dr, Ir) = got, ref
    assert l.dtype == np.uint64 and D.dtype == np.float32 and I.dtype == np.uint64
    assert l.tolist() == lr.tolist(), f"lims differ: gpu {l.tolist()} ref {lr.tolist()}"
    bad = np.flatnonzero(I != Ir)
    assert bad.size == 0, f"ids differ at {bad[:5].tolist()}: gpu {I[bad[0]]} ref {Ir[bad[0]]}"
    badd = np.flatnonzero(bits(D) != bits(Dr))
    assert badd.size == 0, f"dist bits differ at {badd[:5].tolist()}: gpu {D[badd[0]]!r} ref {Dr[badd[0]]!r}"


def raw(r):
    return tuple(a.tobytes() for a in r)


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
    """A handle in one of the three list layouts a range call can meet."""
    X, Q, ids, lists, C = data(dim)
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, NLIST, vdb.Metric(metric), **cfg))
    g.centroids = C
    if layout == "il":  # the interleaved arena
        g.set_option("screen", 0)
        g.add_to_lists(X, ids, lists)
    elif layout == "rows":  # the screen built: its row-major copy is the lists' only fp32 copy
        g.add_to_lists(X, ids, lists)
        g.search(Q, nprobe=5, k=10)
        if metric != 2:  # (no screen for Cosine: its lists stay interleaved)
            assert g.profile_read()["screen_shadow"] in (1, 2)
    else:  # "stale": right after an add, no search since
        g.add_to_lists(X[:N - TAIL], ids[:N - TAIL], lists[:N - TAIL])
        g.search(Q, nprobe=5, k=10)
        g.add_to_lists(X[N - TAIL:], ids[N - TAIL:], lists[N - TAIL:])
    assert g.list_sizes().tolist() == LENS
    return g


def oracle_of(dim, metric, rows):
    X, _, ids, lists, C = rows
    o = oracle.OracleIndex(dim, NLIST, metric)
    o.centroids = C
    for l in range(NLIST):
        sel = np.flatnonzero(lists == l)
        o.set_list(l, X[sel], ids[sel])
    return o


def full(dim, metric, nprobe, rows=None, key="base", Q=None):
    """Per query the oracle's whole single-query result (its real entries), computed once per
    configuration and shared."""
    k = (dim, metric, nprobe, key)
    if k not in _full:
        rows = rows or data(dim)
        Qs = rows[1] if Q is None else Q
        o = oracle_of(dim, metric, rows)
        n = rows[0].shape[0]
        out = []
        for i in range(Qs.shape[0]):
            D, I = o.search(Qs[i:i + 1], nprobe, n)
            real = I[0] != NONE
            out.append((D[0][real].copy(), I[0][real].copy()))
        _full[k] = out
    return _full[k]


def cut(per_query, radius):
    r = np.float32(radius)
    lims = [0]
    Ds, Is = [], []
    for D, I in per_query:
        keep = D <= r
        Ds.append(D[keep])
        Is.append(I[keep])
        lims.append(lims[-1] + int(keep.sum()))
    return np.array(lims, dtype=np.uint64), np.concatenate(Ds).astype(np.float32), np.concatenate(Is).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def probed_rows(dim, metric, nprobe, q):
    """(rows of the lists query q probes, twice-stored ids with both copies among them)."""
    _, Q, ids, lists, C = data(dim)
    o = oracle.OracleIndex(dim, NLIST, metric)
    o.centroids = C
    pl = [int(l) for l in o.select_nprobe(Q[q], min(nprobe, NLIST))]
    return sum(LENS[l] for l in pl), (10 if HUB in pl and NLIST - 1 in pl else 0)


def median_radius(per_query):
    return np.float32(np.median(np.concatenate([D for D, _ in per_query])))


# ---- 1. radii x metrics x layouts x dims ----
@pytest.mark.parametrize("dim", [20, 128])
@pytest.mark.parametrize("layout", ["il", "rows", "stale"])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_radii(metric, layout, dim):
    X, Q, ids, lists, C = data(dim)
    g = make(dim, metric, layout)
    ref = full(dim, metric, 5)
    allD = np.concatenate([D for D, _ in ref])

    # below the smallest distance of any query: nothing
    below = np.nextafter(allD.min(), np.float32(-np.inf), dtype=np.float32)
    got = g.range_search(Q, below, nprobe=5)
    assert got[0].tolist() == [0] * (NQ + 1) and got[1].size == 0 and got[2].size == 0
    assert_same(got, cut(ref, below))
    # exactly the bits of query 0's 5th distance: inclusive
    D0, I0 = ref[0]
    assert D0.size >= 5
    r5 = D0[4]
    got = g.range_search(Q, r5, nprobe=5)
    assert_same(got, cut(ref, r5))
    n0 = int(got[0][1])
    assert n0 >= 5 and got[2][4] == I0[4] and bits(got[1][4:5])[0] == bits(D0[4:5])[0]
    # one step below it: absent
    lower = np.nextafter(r5, np.float32(-np.inf), dtype=np.float32)
    got = g.range_search(Q, lower, nprobe=5)
    assert_same(got, cut(ref, lower))
    assert int(got[0][1]) < n0 and I0[4] not in got[2][:int(got[0][1])].tolist()
    # the median of all distances
    assert_same(g.range_search(Q, median_radius(ref), nprobe=5), cut(ref, median_radius(ref)))
    # FLT_MAX and +inf: every probed row, a twice-stored id once
    for r in (FMAX, INF):
        got = g.range_search(Q, r, nprobe=5)
        assert_same(got, cut(ref, r))
        for i in range(NQ):
            rows, twice = probed_rows(dim, metric, 5, i)
            assert int(got[0][i + 1] - got[0][i]) == rows - twice
    if metric == 2:  # every row at 0.0f: radius 0 gives everything in id order, -1 nothing
        got = g.range_search(Q, 0.0, nprobe=5)
        assert_same(got, cut(ref, INF))
        assert np.all(bits(got[1]) == 0)
        for i in range(NQ):
            mine = got[2][int(got[0][i]):int(got[0][i + 1])]
            assert np.all(mine[1:] > mine[:-1])
        got = g.range_search(Q, -1.0, nprobe=5)
        assert got[0].tolist() == [0] * (NQ + 1)


# ---- 2. nprobe, the twice-stored ids, the counters ----
@pytest.mark.parametrize("layout", ["il", "rows"])
def test_nprobe(layout):
    dim = 20
    X, Q, ids, lists, C = data(dim)
    g = make(dim, 0, layout)
    for nprobe in (1, 5, 12, 40):  # (40: clamped to nlist)
        ref = full(dim, 0, min(nprobe, NLIST))
        for r in (median_radius(full(dim, 0, 5)), INF):
            got = g.range_search(Q, r, nprobe=nprobe, reserve=N * NQ)
            assert_same(got, cut(ref, r))
            t = g.range_last_timing()
            want = sum(probed_rows(dim, 0, nprobe, i)[0] for i in range(NQ))
            assert t["pairs_scanned"] == want
            assert t["reruns"] == 0
            assert t["hits"] == got[2].size
    # nprobe = 12, radius +inf: each twice-stored id once per query, at the smaller distance
    got = g.range_search(Q, INF, nprobe=12)
    twice = ids[np.flatnonzero(lists == HUB)[100:110]]
    copies = []
    for l in (HUB, NLIST - 1):  # the distances of each copy alone, from the oracle
        o = oracle.OracleIndex(dim, NLIST, 0)
        o.centroids = C
        sel = np.flatnonzero((lists == l) & np.isin(ids, twice))
        assert sel.size == 10
        o.set_list(l, X[sel], ids[sel])
        per = []
        for i in range(NQ):
            D, I = o.search(Q[i:i + 1], 12, 10)
            per.append(dict(zip(I[0].tolist(), D[0].tolist())))
        copies.append(per)
    for i in range(NQ):
        lo, hi = int(got[0][i]), int(got[0][i + 1])
        mine_i, mine_d = got[2][lo:hi], got[1][lo:hi]
        for t in twice.tolist():
            at = np.flatnonzero(mine_i == t)
            assert at.size == 1
            assert mine_d[at[0]] == np.float32(min(copies[0][i][t], copies[1][i][t]))


# ---- 3. signed zeros ----
@pytest.mark.parametrize("layout", ["il", "rows"])
def test_signed_zeros(layout):
    dim = 20
    X, Q, ids, lists, C = data(dim)
    g = make(dim, 1, layout)
    Qz = np.zeros((1, dim), dtype=np.float32)
    ref = full(dim, 1, 5, key="zero-query", Q=Qz)
    assert ref[0][0].size > 0 and np.all(ref[0][0] == 0)
    for r in (0.0, -0.0):
        got = g.range_search(Qz, np.float32(r), nprobe=5)
        assert_same(got, cut(ref, INF))  # every probed row, the oracle's bits
        assert np.all(got[2][1:] > got[2][:-1])  # id order
    # L2, a stored row as the query, radius 0: that row
    g = make(dim, 0, layout)
    r = int(np.flatnonzero(lists == 7)[5])
    Qr = X[r:r + 1]
    ref = full(dim, 0, NLIST, key="row-query", Q=Qr)
    got = g.range_search(Qr, 0.0, nprobe=NLIST)
    assert_same(got, cut(ref, 0.0))
    assert got[2].tolist() == [int(ids[r])] and bits(got[1]).tolist() == [0]


# ---- 4. overflow: a batch that finds more hits than the buffer holds is run again ----
@pytest.mark.parametrize("layout", ["il", "rows"])
def test_overflow_rerun(layout):
    dim = 20
    X, Q, ids, lists, C = data(dim)
    g = make(dim, 0, layout)
    ref = full(dim, 0, 5)
    r = median_radius(ref)
    ample = g.range_search(Q, r, nprobe=5, reserve=N * NQ)
    assert g.range_last_timing()["reruns"] == 0
    tight = g.range_search(Q, r, nprobe=5, reserve=1)
    assert g.range_last_timing()["reruns"] >= 1
    assert raw(tight) == raw(ample)
    assert_same(tight, cut(ref, r))


# ---- 5. batch independence and determinism ----
def test_batch_independence_and_determinism():
    dim = 20
    X, Q, ids, lists, C = data(dim)
    ref = full(dim, 0, 5)
    r = median_radius(ref)
    g = make(dim, 0, "rows")
    a = g.range_search(Q, r, nprobe=5)
    assert raw(g.range_search(Q, r, nprobe=5)) == raw(a)
    g.set_stale_slots(False)
    assert raw(g.range_search(Q, r, nprobe=5)) == raw(a)
    g.set_stale_slots(True)
    assert raw(g.range_search(Q, r, nprobe=5)) == raw(a)
    g8 = make(dim, 0, "rows")
    g8.set_batch(8)
    assert raw(g8.range_search(Q, r, nprobe=5)) == raw(a)
    assert raw(g8.range_search(Q, r, nprobe=5, reserve=1)) == raw(a)
    assert g8.range_last_timing()["reruns"] >= 1
    assert_same(a, cut(ref, r))


# ---- 6. the handle is left exactly as found ----
@pytest.mark.parametrize("layout", ["il", "rows", "stale"])
def test_handle_untouched(layout):
    dim = 20
    X, Q, ids, lists, C = data(dim)
    g = make(dim, 0, layout)
    plain_only = make(dim, 0, layout)

    def state(h):
        return (h.list_sizes().tolist(), h.get_total_vectors(), h.profile_read()["screen_shadow"],
                [(a.tobytes(), b.tobytes()) for a, b in (h.get_list(HUB), h.get_list(4))])

    before = state(g)
    for r, reserve in ((median_radius(full(dim, 0, 5)), 0), (INF, 1), (-1.0, 0)):
        g.range_search(Q, r, nprobe=5, reserve=reserve)
        assert state(g) == before
    D0, I0 = plain_only.search(Q, nprobe=5, k=10)
    D1, I1 = g.search(Q, nprobe=5, k=10)
    assert I1.tobytes() == I0.tobytes() and D1.tobytes() == D0.tobytes()
    g.range_search(Q, INF, nprobe=5)
    D1, I1 = g.search(Q, nprobe=5, k=10)
    assert I1.tobytes() == I0.tobytes() and D1.tobytes() == D0.tobytes()
    assert state(g) == state(plain_only)


# ---- 7. after remove_ids and a further add ----
def test_after_mutations():
    dim = 20
    X, Q, ids, lists, C = data(dim)
    g = make(dim, 0, "rows")
    gone = np.isin(ids, ids[::3])
    assert g.remove_ids(ids[::3]) == int(gone.sum())
    keep = ~gone
    rows = (X[keep], Q, ids[keep], lists[keep], C)
    ref = full(dim, 0, 5, rows=rows, key="removed")
    r = median_radius(ref)
    assert_same(g.range_search(Q, r, nprobe=5), cut(ref, r))  # (screen stale: interleaved)
    g.search(Q, nprobe=5, k=10)
    assert_same(g.range_search(Q, r, nprobe=5), cut(ref, r))  # (row-major again)
    assert_same(g.range_search(Q, INF, nprobe=5), cut(ref, INF))
    X2, _, _ = oracle.reference_test_data(400, 1, dim, seed=91)
    ids2 = np.arange(10 ** 6, 10 ** 6 + 400, dtype=np.uint64)
    lists2 = (np.arange(400) % NLIST).astype(np.uint32)
    g.add_to_lists(X2, ids2, lists2)
    rows = (np.concatenate([X[keep], X2]), Q, np.concatenate([ids[keep], ids2]), np.concatenate([lists[keep], lists2]), C)
    ref = full(dim, 0, 5, rows=rows, key="removed+added")
    for rr in (r, INF):
        assert_same(g.range_search(Q, rr, nprobe=5), cut(ref, rr))  # (screen stale)
    g.search(Q, nprobe=5, k=10)
    for rr in (r, INF):
        assert_same(g.range_search(Q, rr, nprobe=5), cut(ref, rr))  # (screen rebuilt)


# ---- 8. plain, filtered and range searches from four threads ----
def test_concurrent_plain_filtered_and_range():
    dim = 20
    X, Q, ids, lists, C = data(dim)
    g = make(dim, 0, "rows")
    r = median_radius(full(dim, 0, 5))
    T, loops = 4, 12
    batches = [Q[t * 10:(t + 1) * 10] for t in range(T)]

    def run(t, j):
        if j == 0:
            return g.search(batches[t], nprobe=5, k=10)
        if j == 1:
            return g.search_filtered(batches[t], ids=ids[::2], include=False, nprobe=5, k=10)
        if j == 2:
            return g.range_search(batches[t], r, nprobe=5)
        return g.range_search(batches[t], INF, nprobe=5, reserve=1)

    alone = [[raw(run(t, j)) for j in range(4)] for t in range(T)]
    results = [[] for _ in range(T)]
    errors = []

    def worker(t):
        try:
            for i in range(loops):
                j = (t + i) % 4
                results[t].append((j, raw(run(t, j))))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
    for t in range(T):
        assert len(results[t]) == loops
        for j, got in results[t]:
            assert got == alone[t][j]
    ref = full(dim, 0, 5)
    for t in range(T):
        assert_same(g.range_search(batches[t], r, nprobe=5), cut(ref[t * 10:(t + 1) * 10], r))


# ---- 9. refusals name their cause and leave the handle untouched ----
def refused(g, Q, code, match, radius=1.0):
    D0, I0 = g.search(Q, nprobe=5, k=10)
    sizes = g.list_sizes().tolist()
    with pytest.raises(vdb.VdbError, match=match) as e:
        g.range_search(Q, radius, nprobe=5)
    assert e.value.code == code
    assert g.list_sizes().tolist() == sizes
    D1, I1 = g.search(Q, nprobe=5, k=10)
    assert I1.tobytes() == I0.tobytes() and D1.tobytes() == D0.tobytes()


def test_refusals_and_empty_cases():
    dim = 20
    X, Q, ids, lists, C = data(dim)
    UNSUPPORTED, INVALID = -4, -1
    g = make(dim, 0, "rows")
    refused(g, Q, INVALID, "radius", radius=float("nan"))
    # null queries and a null out, through the C ABI
    L = vdb.lib()
    out = ctypes.c_void_p()
    q = np.ascontiguousarray(Q)
    vp = ctypes.c_void_p
    assert L.vdb_ivf_range_search(g._h, None, NQ, 5, 1.0, 0, ctypes.byref(out)) == INVALID
    assert b"null" in L.vdb_last_error() and not out.value
    assert L.vdb_ivf_range_search(g._h, vp(q.ctypes.data), NQ, 5, 1.0, 0, None) == INVALID
    assert b"null" in L.vdb_last_error()
    # the list-cache tier
    t = make(dim, 0, "il", max_gpu_memory=0)
    t.set_option("list_cache_bytes", 60 * 64 * (128 * 4 + 8))  # room for every list
    assert t.cache_stats()["capacity_bytes"] > 0
    refused(t, Q, UNSUPPORTED, "list-cache tier")
    # a group of two members on the one device
    grp = make(dim, 0, "rows", devices=(0, 0))
    assert grp.group_size == 2
    refused(grp, Q, UNSUPPORTED, "group")
    # a shard
    s = make(dim, 0, "rows")
    s.set_shard(0, 2)
    refused(s, Q, UNSUPPORTED, "sharded")
    # n = 0, nprobe = 0, and an empty trained index
    lims, D, I = g.range_search(np.empty((0, dim), np.float32), 1.0, nprobe=5)
    assert lims.tolist() == [0] and D.size == 0 and I.size == 0
    lims, D, I = g.range_search(Q, INF, nprobe=0)
    assert lims.tolist() == [0] * (NQ + 1) and D.size == 0 and I.size == 0
    e = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, NLIST, vdb.Metric(0)))
    e.centroids = C
    lims, D, I = e.range_search(Q, INF, nprobe=5)
    assert lims.tolist() == [0] * (NQ + 1) and D.size == 0 and I.size == 0
    # the result outlives the handle: host memory only
    r = ctypes.c_void_p()
    h = make(dim, 0, "il")
    assert L.vdb_ivf_range_search(h._h, vp(q.ctypes.data), NQ, 5, float(INF), 0, ctypes.byref(r)) == 0
    del h
    n = L.vdb_range_result_n(r)
    assert n == NQ
    lims = np.ctypeslib.as_array(ctypes.cast(L.vdb_range_result_lims(r), ctypes.POINTER(ctypes.c_uint64)), shape=(n + 1,))
    want = cut(full(dim, 0, 5), INF)
    assert lims.tolist() == want[0].tolist()
    got_i = np.ctypeslib.as_array(ctypes.cast(L.vdb_range_result_ids(r), ctypes.POINTER(ctypes.c_uint64)),
                                  shape=(int(lims[n]),))
    assert got_i.tolist() == want[2].tolist()
    L.vdb_range_result_free(r)


# ---- 10. the drop-in C++ class ----
def test_cpp_class_range_search():
    cpp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    exe = os.path.join(cpp, "bin", "range_test")
    subprocess.check_call(["make", "-s", "-C", cpp, exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "range searches bit-identical to the CPU path cut at the radius: yes" in p.stdout
