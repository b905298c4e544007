"""GPU: prepared id filters (vdb_ivf_filter_create, vdb_filter_combine, vdb_ivf_search_prepared,
vdb_ivf_range_search_prepared) against the CPU oracle.

Definitions under test. A prepared search returns what vdb_ivf_search returns on a handle with
the same centroids that holds only the rows the filter allows, in their original order; it must
also equal, bit for bit, the one-shot vdb_ivf_search_filtered of the same id set. A filtered
range search returns, for each query on its own, that handle's whole single-query result cut by
(I != NONE) & (D <= radius). So every expected value comes from an OracleIndex whose lists are
set_list to the allowed rows in order, never from the library.

Shape (that of test_gpu_filter.py): 2,940 rows placed with add_to_lists into nlist = 12 lists of
0, 1, 63, 64, 65, 130 rows, one hub list of 1,500 rows (24 blocks: every wave of a workgroup and
two segments of 12 blocks) and five more of a few blocks each; dimensions 20 (padded) and 128;
40 queries. Ten ids are stored twice, in two different lists.
"""
import ctypes
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
EXCLUDE, INCLUDE = False, True
INVALID, UNSUPPORTED, STATE = -1, -4, -5
NPROBE, K = 5, 10
_data = {}
_expect = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(D, I, Dr, Ir):
    assert I.shape == Ir.shape
    bad = np.argwhere(I != Ir)
    assert bad.size == 0, f"ids differ at {bad[:5].tolist()}: gpu {I[tuple(bad[0])]} ref {Ir[tuple(bad[0])]}"
    badd = np.argwhere(bits(D) != bits(Dr))
    assert badd.size == 0, f"dist bits differ at {badd[:5].tolist()}: gpu {D[tuple(badd[0])]!r} ref {Dr[tuple(badd[0])]!r}"


def assert_same_range(got, ref):
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
    """A handle in one of the three list layouts a prepared call can meet."""
    X, Q, ids, lists, C = data(dim)
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, NLIST, vdb.Metric(metric), **cfg))
    g.centroids = C
    if layout == "il":  # the interleaved arena
        g.set_option("screen", 0)
        g.add_to_lists(X, ids, lists)
    elif layout == "rows":  # the screen built: its row-major copy is the lists' only fp32 copy
        g.add_to_lists(X, ids, lists)
        g.search(Q, nprobe=NPROBE, k=K)
        if metric != 2:  # (no screen for Cosine: its lists stay interleaved)
            assert g.profile_read()["screen_shadow"] in (1, 2)
    else:  # "stale": right after an add, no search since
        g.add_to_lists(X[:N - TAIL], ids[:N - TAIL], lists[:N - TAIL])
        g.search(Q, nprobe=NPROBE, k=K)
        g.add_to_lists(X[N - TAIL:], ids[N - TAIL:], lists[N - TAIL:])
    assert g.list_sizes().tolist() == LENS
    return g


def filters(dim):
    """name -> (ids as handed to the library, include). The cases the feature's issue lists."""
    _, _, ids, lists, _ = data(dim)
    hub = ids[lists == HUB]
    rng = np.random.RandomState(77)
    some = ids[3::5]
    odd = np.concatenate([some, some[::2], np.array([1, 2 ** 40, NONE, 5], dtype=np.uint64)])
    odd = odd[rng.permutation(odd.size)]  # unsorted, repeats, ids that are not stored
    last = np.array([ids[np.flatnonzero(lists == 2)[-1]], ids[np.flatnonzero(lists == 4)[-1]]], dtype=np.uint64)
    return {
        "exclude nothing": (np.empty(0, np.uint64), EXCLUDE),
        "exclude 1%": (ids[::97], EXCLUDE),
        "exclude 50%": (ids[::2], EXCLUDE),
        "include 1%": (ids[5::97], INCLUDE),
        "include nothing": (np.empty(0, np.uint64), INCLUDE),
        "include the last rows of the 63- and 65-row lists": (last, INCLUDE),  # (the single-row second block)
        "exclude the hub's first segment": (hub[:768], EXCLUDE),  # 12 of its 24 blocks
        "exclude unsorted, repeats, not stored": (odd, EXCLUDE),
        "include unsorted, repeats, not stored": (odd, INCLUDE),
    }


def allowed_rows(ids, flt, include):
    hit = np.isin(ids, np.asarray(flt, dtype=np.uint64))
    return hit if include else ~hit


def oracle_of(dim, metric, allow):
    X, _, ids, lists, C = data(dim)
    o = oracle.OracleIndex(dim, NLIST, metric)
    o.centroids = C
    for l in range(NLIST):
        rows = np.flatnonzero((lists == l) & allow)
        o.set_list(l, X[rows], ids[rows])
    return o


def expect(dim, metric, key, allow, Q=None, nprobe=NPROBE):
    """What the oracle holding only the rows of `allow` answers, computed once per (dim, metric,
    key) and shared: (search(Q, nprobe, K), per query the whole single-query result's real entries)."""
    kk = (dim, metric, key)
    if kk not in _expect:
        Qs = data(dim)[1] if Q is None else Q
        o = oracle_of(dim, metric, allow)
        top = o.search(Qs, nprobe, K)
        per = []
        kfull = N  # (no smaller than the rows any query probes)
        for i in range(Qs.shape[0]):
            D, I = o.search(Qs[i:i + 1], nprobe, kfull)
            real = I[0] != NONE
            per.append((D[0][real].copy(), I[0][real].copy()))
        _expect[kk] = (top, per)
    return _expect[kk]


def cut(per_query, radius):
    r = np.float32(radius)
    lims, Ds, Is = [0], [np.empty(0, np.float32)], [np.empty(0, np.uint64)]
    for D, I in per_query:
        keep = D <= r
        Ds.append(D[keep])
        Is.append(I[keep])
        lims.append(lims[-1] + int(keep.sum()))
    return np.array(lims, dtype=np.uint64), np.concatenate(Ds).astype(np.float32), np.concatenate(Is).astype(np.uint64)


def radii(per_query):
    """Below every distance, the median over the queries of the 10th distance (of the last one
    where a query has fewer; 0 where no query has any), +inf and FLT_MAX."""
    have = [D for D, _ in per_query if D.size]
    if have:
        below = np.nextafter(min(D.min() for D in have), np.float32(-np.inf), dtype=np.float32)
        med = np.float32(np.median([D[min(K - 1, D.size - 1)] for D in have]))
    else:
        below, med = np.float32(-1.0), np.float32(0.0)
    return [below, med, INF, FMAX]


def device_ids(a):
    """(tensor kept alive, device address) of a uint64 array on device 0, complete."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr()


def check_both(g, dim, metric, flt, key, allow, one_shot=None):
    """search_prepared and range_search_prepared of `flt` against the oracle over `allow`."""
    Q = data(dim)[1]
    (Dr, Ir), per = expect(dim, metric, key, allow)
    assert flt.allowed == int(allow.sum())
    assert not flt.stale
    D, I = g.search_prepared(Q, flt, nprobe=NPROBE, k=K)
    assert_same(D, I, Dr, Ir)
    t = g.filter_last_timing()
    assert t["mark_ms"] == 0.0
    if one_shot is not None:
        Df, If = g.search_filtered(Q, ids=one_shot[0], include=one_shot[1], nprobe=NPROBE, k=K)
        assert_same(D, I, Df, If)
        assert g.filter_last_timing()["pairs_scanned"] == t["pairs_scanned"]
    for r in radii(per):
        got = g.range_search_prepared(Q, flt, r, nprobe=NPROBE)
        assert_same_range(got, cut(per, r))
        assert g.range_last_timing()["hits"] == got[2].size
    # +inf counted one distance per allowed row of every probed list, no more
    o = oracle.OracleIndex(dim, NLIST, metric)
    o.centroids = data(dim)[4]
    lists = data(dim)[3]
    g.range_search_prepared(Q, flt, INF, nprobe=NPROBE, reserve=N * NQ)
    want = sum(int(allow[lists == l].sum()) for q in Q for l in o.select_nprobe(q, NPROBE))
    assert g.range_last_timing()["pairs_scanned"] == want
    assert t["pairs_scanned"] == want


# ---- 1. filters x metrics x layouts x dims: both calls, host and device creation ----
@pytest.mark.parametrize("dim", [20, 128])
@pytest.mark.parametrize("layout", ["il", "rows", "stale"])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_filters(metric, layout, dim):
    X, Q, ids, lists, C = data(dim)
    g = make(dim, metric, layout)
    for name, (f_ids, inc) in filters(dim).items():
        allow = allowed_rows(ids, f_ids, inc)
        flt = g.prepare_filter(f_ids, include=inc)
        check_both(g, dim, metric, flt, name, allow, one_shot=(f_ids, inc))
        # the same ids from the device: the same masks, judged by the count and the results
        keep, ptr = device_ids(f_ids) if f_ids.size else (None, 0)  # (no ids: a null pointer will do)
        fd = g.prepare_filter(None, include=inc, device_ptr=ptr, n=f_ids.size)
        assert fd.allowed == flt.allowed
        assert raw(g.search_prepared(Q, fd, nprobe=NPROBE, k=K)) == raw(g.search_prepared(Q, flt, nprobe=NPROBE, k=K))
        assert raw(g.range_search_prepared(Q, fd, INF, nprobe=NPROBE)) == raw(g.range_search_prepared(Q, flt, INF, nprobe=NPROBE))
        del keep
        fd.close()
        flt.close()
    if layout == "stale":  # the plain search rebuilds the screen: the layout switch keeps a filter
        f_ids, inc = filters(dim)["exclude 50%"]
        flt = g.prepare_filter(f_ids, include=inc)
        g.search(Q, nprobe=NPROBE, k=K)
        check_both(g, dim, metric, flt, "exclude 50%", allowed_rows(ids, f_ids, inc))


# ---- 2. a NULL filter, the empty id set from the device, an empty handle ----
def test_null_filter_and_empty_cases():
    dim = 20
    X, Q, ids, lists, C = data(dim)
    g = make(dim, 0, "rows")
    _, per = expect(dim, 0, "exclude nothing", np.ones(N, bool))
    for r in radii(per):
        a = g.range_search_prepared(Q, None, r, nprobe=NPROBE)
        assert raw(a) == raw(g.range_search(Q, r, nprobe=NPROBE))
        assert_same_range(a, cut(per, r))
    # n_filter == 0 through the device entry (the pointer may be null)
    L = vdb.lib()
    for mode, want in ((0, N), (1, 0)):
        out = ctypes.c_void_p()
        assert L.vdb_ivf_filter_create_device(g._h, None, 0, mode, ctypes.byref(out)) == 0
        f = vdb.Filter(out)
        assert f.allowed == want and not f.stale
    # n = 0, nprobe = 0, k = 0
    f = g.prepare_filter(ids[::2])
    lims, D, I = g.range_search_prepared(np.empty((0, dim), np.float32), f, 1.0, nprobe=NPROBE)
    assert lims.tolist() == [0] and D.size == 0 and I.size == 0
    lims, D, I = g.range_search_prepared(Q, f, INF, nprobe=0)
    assert lims.tolist() == [0] * (NQ + 1) and D.size == 0
    D, I = g.search_prepared(Q, f, nprobe=0, k=K)
    assert np.all(I == NONE) and np.all(D == FMAX)
    # an empty trained index: a filter of nothing, every slot unfilled
    e = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, NLIST, vdb.Metric(0)))
    e.centroids = C
    for inc in (EXCLUDE, INCLUDE):
        fe = e.prepare_filter(ids[:10], include=inc)
        assert fe.allowed == 0 and not fe.stale
        D, I = e.search_prepared(Q, fe, nprobe=NPROBE, k=K)
        assert np.all(I == NONE) and np.all(D == FMAX)
        assert e.range_search_prepared(Q, fe, INF, nprobe=NPROBE)[0].tolist() == [0] * (NQ + 1)
    both = fe & fe
    assert both.allowed == 0


# ---- 3. signed zeros under a filter ----
@pytest.mark.parametrize("layout", ["il", "rows"])
def test_signed_zeros(layout):
    dim = 20
    X, Q, ids, lists, C = data(dim)
    f_ids = ids[::2]
    allow = allowed_rows(ids, f_ids, EXCLUDE)
    g = make(dim, 1, layout)
    flt = g.prepare_filter(f_ids)
    Qz = np.zeros((1, dim), dtype=np.float32)
    _, per = expect(dim, 1, "zero-query, exclude 50%", allow, Q=Qz)
    assert per[0][0].size > 0 and np.all(per[0][0] == 0)
    for r in (0.0, -0.0):
        got = g.range_search_prepared(Qz, flt, np.float32(r), nprobe=NPROBE)
        assert_same_range(got, cut(per, INF))  # every allowed probed row, the oracle's bits
        assert np.all(got[2][1:] > got[2][:-1])  # id order
    # L2, a stored row as the query, radius 0: that row if it is allowed, nothing if it is not
    g = make(dim, 0, layout)
    flt = g.prepare_filter(f_ids)
    for r in (int(np.flatnonzero((lists == 7) & allow)[5]), int(np.flatnonzero((lists == 7) & ~allow)[5])):
        Qr = X[r:r + 1]
        _, per = expect(dim, 0, f"row-query {r}, exclude 50%", allow, Q=Qr, nprobe=NLIST)
        got = g.range_search_prepared(Qr, flt, 0.0, nprobe=NLIST)
        assert_same_range(got, cut(per, 0.0))
        assert got[2].tolist() == ([int(ids[r])] if allow[r] else [])


# ---- 4. overflow re-run and batch independence ----
@pytest.mark.parametrize("layout", ["il", "rows"])
def test_rerun_and_batch(layout):
    dim = 20
    X, Q, ids, lists, C = data(dim)
    f_ids, inc = filters(dim)["exclude 50%"]
    allow = allowed_rows(ids, f_ids, inc)
    (Dr, Ir), per = expect(dim, 0, "exclude 50%", allow)
    r = radii(per)[1]
    want = cut(per, r)
    assert want[2].size > NQ  # (more hits than a buffer of one entry holds)
    out = []
    for batch in (1, 7, None):
        g = make(dim, 0, layout)
        if batch:
            g.set_batch(batch)
        flt = g.prepare_filter(f_ids, include=inc)
        ample = g.range_search_prepared(Q, flt, r, nprobe=NPROBE, reserve=N * NQ)
        assert g.range_last_timing()["reruns"] == 0
        tight = g.range_search_prepared(Q, flt, r, nprobe=NPROBE, reserve=1)
        assert g.range_last_timing()["reruns"] >= 1
        assert raw(tight) == raw(ample)
        assert_same_range(tight, want)
        g.set_stale_slots(False)
        assert raw(g.range_search_prepared(Q, flt, r, nprobe=NPROBE)) == raw(ample)
        g.set_stale_slots(True)
        D, I = g.search_prepared(Q, flt, nprobe=NPROBE, k=K)
        assert_same(D, I, Dr, Ir)
        out.append(raw(ample) + (D.tobytes(), I.tobytes()))
    assert out[0] == out[1] == out[2]


# ---- 5. combine ----
@pytest.mark.parametrize("layout", ["il", "rows"])
def test_combine(layout):
    dim = 20
    X, Q, ids, lists, C = data(dim)
    g = make(dim, 0, layout)
    A, B = ids[::3], ids[::2]
    inA, inB = np.isin(ids, A), np.isin(ids, B)
    fa, fb = g.prepare_filter(A, include=True), g.prepare_filter(B, include=True)
    xb = g.prepare_filter(B, include=False)
    assert fa.allowed == int(inA.sum()) and xb.allowed == int((~inB).sum())
    cases = {
        "include A and exclude B": (fa & xb, inA & ~inB),
        "A or B": (fa | fb, inA | inB),
        "A and not B": (fa.andnot(fb), inA & ~inB),
        "A with itself, and": (fa & fa, inA),
        "A with itself, or": (fa | fa, inA),
        "A and not A": (fa.andnot(fa), np.zeros(N, bool)),
        "B and exclude B": (fb & xb, np.zeros(N, bool)),
        "(A or B) and not A": ((fa | fb).andnot(fa), inB & ~inA),
    }
    for name, (f, allow) in cases.items():
        assert f.allowed == int(np.count_nonzero(allow)), name
        check_both(g, dim, 0, f, "combine: " + name, allow)
    # the inputs are as they were
    check_both(g, dim, 0, fa, "combine: A", inA)
    # an invalid operation, through the C ABI
    L = vdb.lib()
    out = ctypes.c_void_p()
    assert L.vdb_filter_combine(fa._f, fb._f, 3, ctypes.byref(out)) == INVALID and not out.value
    # filters of two handles
    g2 = make(dim, 0, layout)
    other = g2.prepare_filter(A, include=True)
    with pytest.raises(vdb.VdbError, match="different handles") as e:
        fa & other
    assert e.value.code == INVALID


# ---- 6. lifetime ----
def state(h, deep=True):
    if not deep:  # (a tier, group or shard handle: its sizes, as test_gpu_filter.py's `refused` judges)
        return h.list_sizes().tolist()
    return (h.list_sizes().tolist(), h.get_total_vectors(), h.profile_read()["screen_shadow"],
            [(a.tobytes(), b.tobytes()) for a, b in (h.get_list(HUB), h.get_list(4))])


def refused_both(g, flt, Q, code, match, k=K, radius=1.0, deep=True):
    """Both prepared calls refuse with `code`, and the handle is as it was (deep: down to the
    rows of two lists, as test_handle_untouched of test_gpu_filter.py judges it)."""
    D0, I0 = g.search(Q, nprobe=NPROBE, k=K)
    before = state(g, deep)
    with pytest.raises(vdb.VdbError, match=match) as e:
        g.search_prepared(Q, flt, nprobe=NPROBE, k=k)
    assert e.value.code == code
    if k == K:
        with pytest.raises(vdb.VdbError, match=match) as e:
            g.range_search_prepared(Q, flt, radius, nprobe=NPROBE)
        assert e.value.code == code
    assert state(g, deep) == before
    assert_same(*g.search(Q, nprobe=NPROBE, k=K), D0, I0)


def test_filter_survives_the_layout_switch():
    dim = 20
    X, Q, ids, lists, C = data(dim)
    f_ids, inc = filters(dim)["include 1%"]
    allow = allowed_rows(ids, f_ids, inc)
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, NLIST, vdb.Metric(0)))
    g.centroids = C
    g.add_to_lists(X, ids, lists)  # interleaved: no search has built the screen yet
    assert g.profile_read()["screen_shadow"] == 0
    flt = g.prepare_filter(f_ids, include=inc)
    half = g.prepare_filter(ids[::2])
    check_both(g, dim, 0, flt, "include 1%", allow)
    g.search(Q, nprobe=NPROBE, k=K)  # builds the screen and drops the arena: row-major now
    assert g.profile_read()["screen_shadow"] in (1, 2)
    assert not flt.stale and not half.stale
    check_both(g, dim, 0, flt, "include 1%", allow)
    check_both(g, dim, 0, half, "exclude 50%", allowed_rows(ids, ids[::2], EXCLUDE))
    g.set_option("screen", 0)  # and back to the arena
    assert g.profile_read()["screen_shadow"] == 0
    assert not flt.stale
    check_both(g, dim, 0, flt, "include 1%", allow)


def test_stale_after_mutations(tmp_path):
    dim = 20
    X, Q, ids, lists, C = data(dim)
    stale = "stale"
    # add
    g = make(dim, 0, "rows")
    flt = g.prepare_filter(ids[::2])
    X2, _, _ = oracle.reference_test_data(4, 1, dim, seed=91)
    g.add_to_lists(X2, np.arange(10 ** 6, 10 ** 6 + 4, dtype=np.uint64), np.array([1, 3, 3, 7], dtype=np.uint32))
    assert flt.stale
    refused_both(g, flt, Q, STATE, stale)
    with pytest.raises(vdb.VdbError, match=stale) as e:
        flt & flt
    assert e.value.code == STATE
    # a filter made now is live and right (after the add the rows lie interleaved again)
    ids_now = np.concatenate([ids, np.arange(10 ** 6, 10 ** 6 + 4, dtype=np.uint64)])
    fresh = g.prepare_filter(ids[::2])
    assert not fresh.stale and fresh.allowed == int((~np.isin(ids_now, ids[::2])).sum())
    # remove: one that matches nothing keeps the filter, one that removes a row does not
    g = make(dim, 0, "rows")
    flt = g.prepare_filter(ids[::2])
    assert g.remove_ids(np.array([1, 2, 2 ** 40], dtype=np.uint64)) == 0
    assert not flt.stale
    check_both(g, dim, 0, flt, "exclude 50%", allowed_rows(ids, ids[::2], EXCLUDE))
    # (removing one row and adding one to the same list restores every count: the epoch tells)
    victim = int(np.flatnonzero(lists == 7)[3])
    assert g.remove_ids(ids[victim:victim + 1]) == 1
    assert flt.stale
    g.add_to_lists(X[victim:victim + 1], ids[victim:victim + 1], lists[victim:victim + 1])
    assert g.list_sizes().tolist() == LENS
    assert flt.stale
    refused_both(g, flt, Q, STATE, stale)
    # load (into an empty handle, whose filter allows nothing)
    path = str(tmp_path / "index.ivf")
    g.save(path)
    e = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, NLIST, vdb.Metric(0)))
    e.centroids = C
    fe = e.prepare_filter(ids[::2])
    assert fe.allowed == 0 and not fe.stale
    e.load(path)
    assert fe.stale
    refused_both(e, fe, Q, STATE, stale)
    # a filter of another handle
    g2 = make(dim, 0, "rows")
    f2 = g2.prepare_filter(ids[::2])
    refused_both(g, f2, Q, INVALID, "another handle")
    assert not f2.stale
    # destroy: stale at once; a later handle refuses the filter (as another handle's, or as stale
    # where the new handle took the old one's address), and freeing it afterwards works
    old = g2._h.value
    g2.close()
    assert f2.stale
    g3 = make(dim, 0, "rows")
    refused_both(g3, f2, Q, STATE if g3._h.value == old else INVALID, stale if g3._h.value == old else "another handle")
    f2.close()
    assert f2._f is None


# ---- 7. refusals: the one-shot call's set, on create and on use ----
def refused_create(g, code, match):
    sizes = g.list_sizes().tolist()
    for kw in ({}, {"device": True}):
        with pytest.raises(vdb.VdbError, match=match) as e:
            if kw:
                keep, ptr = device_ids(np.array([1, 2, 3], dtype=np.uint64))
                g.prepare_filter(None, device_ptr=ptr, n=3)
            else:
                g.prepare_filter([1, 2, 3])
        assert e.value.code == code
    assert g.list_sizes().tolist() == sizes


def test_refusals():
    dim = 20
    X, Q, ids, lists, C = data(dim)
    g = make(dim, 0, "rows")
    flt = g.prepare_filter(ids[::2])
    refused_both(g, flt, Q, UNSUPPORTED, "k <= 64", k=65)
    with pytest.raises(vdb.VdbError, match="radius") as e:
        g.range_search_prepared(Q, flt, float("nan"), nprobe=NPROBE)
    assert e.value.code == INVALID
    # an invalid mode and null ids, through the C ABI; *out is written on success only
    L = vdb.lib()
    out = ctypes.c_void_p()
    f = np.array([1, 2], dtype=np.uint64)
    vp = ctypes.c_void_p
    assert L.vdb_ivf_filter_create(g._h, vp(f.ctypes.data), 2, 2, ctypes.byref(out)) == INVALID
    assert b"mode" in L.vdb_last_error() and not out.value
    assert L.vdb_ivf_filter_create(g._h, None, 2, 0, ctypes.byref(out)) == INVALID
    assert b"null" in L.vdb_last_error() and not out.value
    assert L.vdb_ivf_filter_create(g._h, vp(f.ctypes.data), 2, 0, None) == INVALID
    assert L.vdb_ivf_filter_create(g._h, vp(f.ctypes.data), 1 << 31, 0, ctypes.byref(out)) == UNSUPPORTED
    assert not out.value
    check_both(g, dim, 0, flt, "exclude 50%", allowed_rows(ids, ids[::2], EXCLUDE))  # (still live and right)
    # the list-cache tier: no filter is made; one made before is refused
    t = make(dim, 0, "il", max_gpu_memory=0)
    ft = t.prepare_filter(ids[::2])
    t.set_option("list_cache_bytes", 60 * 64 * (128 * 4 + 8))  # room for every list
    assert t.cache_stats()["capacity_bytes"] > 0
    refused_create(t, UNSUPPORTED, "list-cache tier")
    refused_both(t, ft, Q, UNSUPPORTED, "list-cache tier", deep=False)
    assert ft.stale
    # a group of two members on the one device
    grp = make(dim, 0, "rows", devices=(0, 0))
    assert grp.group_size == 2
    refused_create(grp, UNSUPPORTED, "group")
    refused_both(grp, flt, Q, INVALID, "another handle", deep=False)
    # a shard
    s = make(dim, 0, "rows")
    fs = s.prepare_filter(ids[::2])
    s.set_shard(0, 2)
    refused_create(s, UNSUPPORTED, "sharded")
    refused_both(s, fs, Q, UNSUPPORTED, "sharded", deep=False)
    assert fs.stale


# ---- 8. plain, prepared and prepared-range calls from four threads, one shared filter ----
def test_concurrent_plain_and_prepared():
    dim = 20
    X, Q, ids, lists, C = data(dim)
    g = make(dim, 0, "rows")
    f_ids, inc = filters(dim)["exclude 50%"]
    allow = allowed_rows(ids, f_ids, inc)
    flt = g.prepare_filter(f_ids, include=inc)
    (Dr, Ir), per = expect(dim, 0, "exclude 50%", allow)
    r = radii(per)[1]
    T, loops = 4, 12
    batches = [Q[t * 10:(t + 1) * 10] for t in range(T)]

    def run(t, j):
        if j == 0:
            return g.search(batches[t], nprobe=NPROBE, k=K)
        if j == 1:
            return g.search_prepared(batches[t], flt, nprobe=NPROBE, k=K)
        if j == 2:
            return g.range_search_prepared(batches[t], flt, r, nprobe=NPROBE)
        return g.range_search_prepared(batches[t], flt, INF, nprobe=NPROBE, reserve=1)

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
    for t in range(T):
        assert_same_range(g.range_search_prepared(batches[t], flt, r, nprobe=NPROBE), cut(per[t * 10:(t + 1) * 10], r))
    assert not flt.stale


# ---- 9. the drop-in C++ class ----
def test_cpp_class_prepared():
    cpp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    exe = os.path.join(cpp, "bin", "prepared_test")
    subprocess.check_call(["make", "-s", "-C", cpp, exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "prepared searches and range searches bit-identical to the CPU path over the allowed rows: yes" in p.stdout
    assert "stale after an add, refused, freed after the index: yes" in p.stdout
