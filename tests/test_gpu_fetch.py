"""GPU: vdb_ivf_fetch_ids(_device) and vdb_ivf_search_ids against the handle's own lists.

Definition under test: the row of a requested id is the stored row carrying it at the lowest
(list, position), bit for bit as get_list returns it, and dim zeros with found = 0 where no row
carries it. So in every case the expected answer is built on the host from g.get_list(l) over
all lists (unchanged code): for each requested id the first (list, position) that holds it.
search_ids must give, for the found entries in request order, the bits of one g.search over
their fetched rows, and (FLT_MAX, UINT64_MAX) for the others.

Base shape: N = 3000, nlist = 8, centroids from the data (lists of several 64-slot blocks ending
in a partial one). Every request runs on both fp32 layouts of the lists: "il", option screen =
0 (the interleaved arena), and "rows", the default after one search has built the screen (the
row-major copy; the arena is dropped).
"""
import ctypes
import threading

import numpy as np
import pytest

from conftest import load_vdb

vdb = load_vdb()
pytestmark = pytest.mark.gpu

N, NQ, NLIST = 3000, 16, 8
NONE = np.iinfo(np.uint64).max
FMAX = np.finfo(np.float32).max
UNSUPPORTED = -4
BLOCK_BYTES = 64 * (64 * 4 + 8)  # one arena block at dimension 32 (padded to 64 floats)
LAYOUTS = ["il", "rows"]
_data = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def U(*parts):
    """One uint64 request from arrays and plain ints (no detour through another dtype)."""
    return np.concatenate([np.atleast_1d(np.asarray(p, dtype=np.uint64)) for p in parts])


def data(dim, n=N, nlist=NLIST):
    """(X, Q, ids, centroids), computed once per shape and never changed. Ids 0 and
    UINT64_MAX - 1 are stored; UINT64_MAX is not."""
    key = (dim, n, nlist)
    if key not in _data:
        rng = np.random.default_rng(4000 + dim)
        X = rng.standard_normal((n, dim), dtype=np.float32)
        Q = rng.standard_normal((NQ, dim), dtype=np.float32)
        ids = np.arange(n, dtype=np.uint64)
        ids[-1] = NONE - 1
        C = np.ascontiguousarray(X[:: n // nlist][:nlist])
        for a in (X, Q, ids, C):
            a.setflags(write=False)
        _data[key] = (X, Q, ids, C)
    return _data[key]


def shape_of(dim):
    return (600, 4) if dim == 260 else (N, NLIST)


def make(dim, layout, metric=0, centroids=None, **cfg):
    n, nlist = shape_of(dim)
    X, Q, ids, C = data(dim, n, nlist)
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, nlist, vdb.Metric(metric), **cfg))
    g.centroids = C if centroids is None else centroids
    if layout == "il":
        g.set_option("screen", 0)
    g.add(X, ids)
    settle(g, layout, Q)
    return g


def settle(g, layout, Q):
    """Bring the handle into the layout under test: "rows" after one search has built the screen."""
    if layout == "rows":
        g.search(Q, nprobe=3, k=10)
        assert g.profile_read()["screen_shadow"] != 0, "the screen was not built: the rows layout is not under test"
    else:
        assert g.profile_read()["screen_shadow"] == 0


def first_rows(g):
    """id -> the stored row at the lowest (list, position), from get_list over all lists."""
    first = {}
    for l in range(g.config.nlist):
        V, I = g.get_list(l)
        for p in range(len(I)):
            first.setdefault(int(I[p]), V[p])
    return first


def expected(g, req, first=None):
    first = first_rows(g) if first is None else first
    req = np.asarray(req, dtype=np.uint64).reshape(-1)
    V = np.zeros((len(req), g.dimension), dtype=np.float32)
    F = np.zeros(len(req), dtype=np.uint8)
    for i, r in enumerate(req.tolist()):
        row = first.get(r)
        if row is not None:
            V[i], F[i] = row, 1
    return V, F


def check_fetch(g, req, first=None):
    req = np.asarray(req, dtype=np.uint64).reshape(-1)
    Ve, Fe = expected(g, req, first)
    V, F = g.fetch_ids(req)
    assert V.shape == Ve.shape and F.shape == Fe.shape
    assert np.array_equal(F, Fe), f"found differs at {np.argwhere(F != Fe)[:5].ravel().tolist()}"
    bad = np.argwhere(bits(V) != bits(Ve))
    assert bad.size == 0, f"row bits differ at {bad[:5].tolist()}"
    assert g.fetch_last_timing()["rows_found"] == int(Fe.sum())
    return V, F


def raw_fetch(g, req, vectors=True, found=True, count=True):
    """vdb_ivf_fetch_ids with any of its three outputs NULL."""
    req = np.ascontiguousarray(req, dtype=np.uint64)
    n = len(req)
    V = np.full((n, g.dimension), 7.0, dtype=np.float32) if vectors else None
    F = np.full(n, 9, dtype=np.uint8) if found else None
    c = ctypes.c_uint64(12345)
    rc = vdb.lib().vdb_ivf_fetch_ids(g._h, req.ctypes.data_as(ctypes.c_void_p), n,
                                     V.ctypes.data_as(ctypes.c_void_p) if vectors else None,
                                     F.ctypes.data_as(ctypes.c_void_p) if found else None,
                                     ctypes.byref(c) if count else None)
    assert rc == 0, vdb.lib().vdb_last_error()
    return V, F, (int(c.value) if count else None)


def requests(ids, rng):
    """The request kinds of the issue, by name."""
    absent = np.array([len(ids) + 5, 2 ** 40, NONE - 2, NONE], dtype=np.uint64)
    some = rng.permutation(ids)[:40]
    mixed = np.empty(len(some) + len(absent), dtype=np.uint64)
    mixed[::11], mixed[np.arange(len(mixed)) % 11 != 0] = absent, some  # absent ones between stored ones
    return {
        "all_shuffled": rng.permutation(ids),
        "one": ids[len(ids) // 2: len(ids) // 2 + 1],
        "absent_mixed": mixed,
        "five_times": np.repeat(ids[17:18], 5),
        "zero_and_max_minus_1": np.array([NONE - 1, 0, NONE - 1], dtype=np.uint64),
        "pad_value": U(NONE, ids[3], NONE),
        "longer_than_index": np.concatenate([ids, absent, ids[::-1], ids[:100]]),
    }


# ---- 1. dimensions x layouts x requests ----
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dim", [4, 30, 32, 260])
def test_requests(dim, layout):
    n, nlist = shape_of(dim)
    X, Q, ids, _ = data(dim, n, nlist)
    g = make(dim, layout)
    sizes = g.list_sizes()
    assert (sizes > 128).any() and (sizes % 64 != 0).any()  # several blocks, a partial one at the end
    first = first_rows(g)
    assert 0 in first and int(NONE - 1) in first and int(NONE) not in first
    for name, req in requests(ids, np.random.default_rng(dim)).items():
        V, F = check_fetch(g, req, first)
        if name == "all_shuffled":
            assert F.all() and np.array_equal(bits(V), bits(X[np.searchsorted(ids, req)]))  # (ids ascend)
        if name == "pad_value":
            assert F.tolist() == [0, 1, 0] and not V[0].any() and not V[2].any()
        if name == "longer_than_index":
            assert len(req) > 2 * n
    # n == 0 succeeds and touches nothing
    V, F = g.fetch_ids(np.empty(0, dtype=np.uint64))
    assert V.shape == (0, dim) and F.shape == (0,)
    assert vdb.lib().vdb_ivf_fetch_ids(g._h, None, 0, None, None, None) == 0
    assert g.fetch_last_timing() == {"sort_ms": 0.0, "locate_ms": 0.0, "gather_ms": 0.0, "rows_found": 0}
    settle_check(g, layout)


def settle_check(g, layout):
    """The layout under test is still the one the handle holds (a fetch builds or drops no screen)."""
    shadow = g.profile_read()["screen_shadow"]
    assert (shadow != 0) if layout == "rows" else (shadow == 0)


# ---- 2. ids stored twice ----
@pytest.mark.parametrize("layout", LAYOUTS)
def test_ids_stored_twice(layout):
    dim = 32
    X, Q, ids, _ = data(dim)
    g = make(dim, layout)
    lists = [g.get_list(l)[1] for l in range(NLIST)]
    rng = np.random.default_rng(5)
    dup_ids, dup_lists = [], []
    for l in range(NLIST):  # 8 ids of every list stored again in the next list (the last list's: in list 0)
        assert len(lists[l]) >= 9
        for p in np.linspace(0, len(lists[l]) - 2, 8).astype(int):
            dup_ids.append(int(lists[l][p]))
            dup_lists.append((l + 1) % NLIST)
    dup_ids[-1], dup_lists[-1] = int(lists[4][-1]), 4  # one pair within one list
    assert len(dup_ids) == 64
    V2 = rng.standard_normal((64, dim), dtype=np.float32)
    g.add_to_lists(V2, np.array(dup_ids, dtype=np.uint64), np.array(dup_lists, dtype=np.uint32))
    settle(g, layout, Q)
    first = first_rows(g)
    V, F = check_fetch(g, rng.permutation(ids), first)
    assert F.all()
    # the copies put into list 0 come before the originals in list 7; every other original wins
    got = {int(i): first[int(i)] for i in dup_ids}
    new_wins = [j for j, i in enumerate(dup_ids) if np.array_equal(bits(got[int(i)]), bits(V2[j]))]
    assert sorted(new_wins) == [j for j in range(63) if dup_lists[j] == 0] and len(new_wins) == 7
    check_fetch(g, U(dup_ids, dup_ids[::-1]), first)


# ---- 3. after a remove and an add ----
@pytest.mark.parametrize("layout", LAYOUTS)
def test_after_remove_and_add(layout):
    dim = 30
    X, Q, ids, _ = data(dim)
    g = make(dim, layout)
    gone = ids[::3]
    assert g.remove_ids(gone) == len(gone)
    for again in (False, True):  # as the remove left the lists, then (rows) with the screen built again
        if again:
            settle(g, layout, Q)
        V, F = check_fetch(g, ids)
        assert not F[::3].any() and F[1::3].all() and F[2::3].all()
        assert np.array_equal(bits(V[F == 1]), bits(X[F == 1]))
    X2 = np.random.default_rng(6).standard_normal((500, dim), dtype=np.float32)
    ids2 = np.arange(N + 10, N + 510, dtype=np.uint64)
    g.add(X2, ids2)
    for again in (False, True):
        if again:
            settle(g, layout, Q)
        V, F = check_fetch(g, U(ids2[::-1], gone[:50], ids[1::3][:50]))
        assert F[:500].all() and np.array_equal(bits(V[:500]), bits(X2[::-1]))
        assert not F[500:550].any() and F[550:].all()


# ---- 4. buffers and counts ----
@pytest.mark.parametrize("layout", LAYOUTS)
def test_buffers_and_counts(layout):
    import torch
    dim = 30
    X, Q, ids, _ = data(dim)
    g = make(dim, layout)
    req = U(ids[5:9], NONE, N + 1, np.repeat(ids[100:101], 5), ids[5:9])
    Ve, Fe = expected(g, req)
    hits = int(Fe.sum())
    assert hits == 13  # repeats count every time they appear
    for vectors in (True, False):
        for found in (True, False):
            for count in (True, False):
                V, F, c = raw_fetch(g, req, vectors, found, count)
                if vectors:
                    assert np.array_equal(bits(V), bits(Ve))
                if found:
                    assert np.array_equal(F, Fe)
                if count:
                    assert c == hits
                assert g.fetch_last_timing()["rows_found"] == hits
    # the device variant through torch tensors equals the host call
    t_ids = torch.from_numpy(req.view(np.int64).copy()).to("cuda:0")
    t_vec = torch.full((len(req), dim), 7.0, dtype=torch.float32, device="cuda:0")
    t_found = torch.full((len(req),), 9, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert g.fetch_ids_device(t_ids.data_ptr(), len(req), t_vec.data_ptr(), t_found.data_ptr()) == hits
    assert np.array_equal(bits(t_vec.cpu().numpy()), bits(Ve))
    assert np.array_equal(t_found.cpu().numpy(), Fe)
    assert np.array_equal(t_ids.cpu().numpy().view(np.uint64), req)  # the request is left as given
    assert g.fetch_ids_device(t_ids.data_ptr(), len(req)) == hits  # existence only
    # output rows that are not 16-byte aligned: a view one float into a larger tensor (dim 32)
    g32 = make(32, layout)
    ids32 = data(32)[2]
    r32 = U(ids32[40:50], NONE)
    big = torch.full((len(r32) * 32 + 2,), 7.0, dtype=torch.float32, device="cuda:0")
    t32 = torch.from_numpy(r32.view(np.int64).copy()).to("cuda:0")
    torch.cuda.synchronize()
    assert g32.fetch_ids_device(t32.data_ptr(), len(r32), big.data_ptr() + 4, None) == 10
    out = big.cpu().numpy()
    assert out[0] == 7.0 and out[-1] == 7.0  # nothing before the first row or past the last
    assert np.array_equal(bits(out[1:-1].reshape(len(r32), 32)), bits(expected(g32, r32)[0]))


# ---- 5. the handle is left as found ----
@pytest.mark.parametrize("layout", LAYOUTS)
def test_handle_left_as_found(layout):
    dim = 32
    X, Q, ids, _ = data(dim)
    g = make(dim, layout)
    flt = g.prepare_filter(ids[::2])
    D0, I0 = g.search(Q, nprobe=3, k=10)
    Df0, If0 = g.search_prepared(Q, flt, nprobe=3, k=10)
    held = g.gpu_bytes_allocated()
    shadow = g.profile_read()["screen_shadow"]
    check_fetch(g, U(ids[::-1], NONE))
    check_fetch(g, ids[7:8])
    assert g.gpu_bytes_allocated() == held
    assert not flt.stale
    assert g.profile_read()["screen_shadow"] == shadow
    settle_check(g, layout)
    D1, I1 = g.search(Q, nprobe=3, k=10)
    assert np.array_equal(I1, I0) and np.array_equal(bits(D1), bits(D0))
    Df1, If1 = g.search_prepared(Q, flt, nprobe=3, k=10)
    assert np.array_equal(If1, If0) and np.array_equal(bits(Df1), bits(Df0))


# ---- 6. metrics ----
@pytest.mark.parametrize("metric", [0, 1, 2, 3])
def test_metrics(metric):
    dim = 30
    X, Q, ids, _ = data(dim)
    for layout in LAYOUTS:
        if metric == 2 and layout == "rows":
            continue  # no screen is built for Cosine: the arena is its only layout
        g = make(dim, layout, metric)
        req = np.random.default_rng(metric).permutation(ids)
        V, F = check_fetch(g, req)  # (equal to get_list's rows: for Cosine and CosineDistance, as stored)
        assert F.all()
        added = X[np.searchsorted(ids, req)]  # (ids ascend)
        if metric == 3:
            # the unit rows, not the rows added: every component is one fp32 rounding (2^-24
            # relative) from the exact unit vector's, so the norm is within 1e-5 of 1 with room
            assert np.allclose(np.linalg.norm(V.astype(np.float64), axis=1), 1.0, rtol=0, atol=1e-5)
            assert not np.array_equal(bits(V), bits(added))
        elif metric != 2:
            assert np.array_equal(bits(V), bits(added))


# ---- 7. search_ids ----
def twin_centroids(dim):
    """The base centroids with list 5's centroid a copy of list 1's: every row of that region goes
    to list 1 (ties go to the lower list), list 5 stays empty and is probed with its twin."""
    C = np.array(data(dim)[3])
    C[5] = C[1]
    return C


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("stale", [1, 0])
@pytest.mark.parametrize("nprobe,k", [(3, 10), (8, 10), (2, 1024)])
def test_search_ids(nprobe, k, stale, layout):
    dim = 32
    X, Q, ids, _ = data(dim)
    C = twin_centroids(dim)
    g = make(dim, layout, centroids=C)
    g.set_stale_slots(bool(stale))
    sizes = g.list_sizes()
    assert sizes[5] == 0 and sizes[1] > 0
    # found ids in descending order (a slot carried over from an earlier query then never holds a
    # lower id at distance 0), rows of list 1 among them, ids that are not stored between them
    l1 = np.sort(g.get_list(1)[1])[::-1][:6]
    stored = np.sort(np.concatenate([ids[10:600:37], l1]))[::-1]
    req, absent = [], []
    for j, i in enumerate(np.unique(stored)[::-1].tolist()):
        if j % 3 == 1:
            req.append(NONE - 5 - j)
            absent.append(True)
        req.append(i)
        absent.append(False)
    req, absent = U(req), np.array(absent)
    Vf, Ff = check_fetch(g, req)
    assert np.array_equal(Ff == 0, absent)
    rows = Vf[Ff == 1]
    # an empty list is probed by at least one found query (the twin of its nearest centroid)
    d2 = ((rows[:, None, :].astype(np.float64) - C[None].astype(np.float64)) ** 2).sum(-1)
    rank_of_empty = (d2 < d2[:, 5:6]).sum(1)  # centroids strictly nearer than the empty list's
    assert (rank_of_empty < nprobe - (nprobe < NLIST)).any()
    Dr, Ir = g.search(rows, nprobe=nprobe, k=k)
    D, I, F = g.search_ids(req, nprobe=nprobe, k=k)
    assert np.array_equal(F, Ff)
    assert D.shape == (len(req), k) and I.shape == (len(req), k)
    assert np.all(I[absent] == NONE) and np.all(D[absent] == FMAX)
    bad = np.argwhere(I[~absent] != Ir)
    assert bad.size == 0, f"ids differ at {bad[:5].tolist()}"
    badd = np.argwhere(bits(D[~absent]) != bits(Dr))
    assert badd.size == 0, f"distance bits differ at {badd[:5].tolist()}"
    # L2: a stored row's nearest row is itself, at +0.0f
    assert np.array_equal(I[~absent][:, 0], req[~absent])
    assert np.all(bits(D[~absent][:, 0]) == 0)
    if k == 1024:
        assert (I[~absent] == NONE).any()  # two lists hold fewer rows: unfilled slots take part
    assert g.fetch_last_timing()["rows_found"] == int(Ff.sum())
    # nothing found: nothing searched
    D, I, F = g.search_ids(req[absent], nprobe=nprobe, k=k)
    assert not F.any() and np.all(I == NONE) and np.all(D == FMAX)
    D, I, F = g.search_ids(np.empty(0, dtype=np.uint64), nprobe=nprobe, k=k)
    assert D.shape == (0, k) and F.shape == (0,)


def test_search_ids_unit_rows():
    """CosineDistance: the stored unit rows are normalised like any query."""
    dim = 30
    X, Q, ids, _ = data(dim)
    g = make(dim, "rows", 3)
    req = U(ids[900:940:3], NONE, ids[5:8])
    Vf, Ff = check_fetch(g, req)
    Dr, Ir = g.search(Vf[Ff == 1], nprobe=3, k=10)
    D, I, F = g.search_ids(req, nprobe=3, k=10)
    assert np.array_equal(F, Ff) and Ff.sum() == len(req) - 1
    assert np.array_equal(I[F == 1], Ir) and np.array_equal(bits(D[F == 1]), bits(Dr))
    assert np.all(I[F == 0] == NONE) and np.all(D[F == 0] == FMAX)
    assert np.array_equal(I[F == 1][:, 0], req[F == 1])


# ---- 8. refusals leave the handle untouched ----
def refused(g, Q, ids, match):
    import torch
    D0, I0 = g.search(Q, nprobe=3, k=10)
    held = g.gpu_bytes_allocated()
    with pytest.raises(vdb.VdbError, match=match) as e:
        g.fetch_ids(ids[:10])
    assert e.value.code == UNSUPPORTED
    with pytest.raises(vdb.VdbError, match=match) as e:
        g.search_ids(ids[:10], nprobe=3, k=10)
    assert e.value.code == UNSUPPORTED
    t = torch.from_numpy(ids[:10].view(np.int64).copy()).to("cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(vdb.VdbError, match=match) as e:
        g.fetch_ids_device(t.data_ptr(), 10)
    assert e.value.code == UNSUPPORTED
    assert g.gpu_bytes_allocated() == held
    D1, I1 = g.search(Q, nprobe=3, k=10)
    assert np.array_equal(I1, I0) and np.array_equal(bits(D1), bits(D0))


def test_refused_in_the_list_cache_tier():
    dim = 32
    X, Q, ids, _ = data(dim)
    g = make(dim, "il", max_gpu_memory=0)
    g.set_option("list_cache_bytes", 64 * BLOCK_BYTES)  # room for every list
    assert g.cache_stats()["capacity_bytes"] > 0
    refused(g, Q, ids, "list-cache tier")


def test_refused_on_a_shard():
    dim = 32
    X, Q, ids, _ = data(dim)
    g = make(dim, "il")
    g.set_shard(0, 2)
    refused(g, Q, ids, "sharded")


def test_refused_on_a_group():
    dim = 32
    X, Q, ids, _ = data(dim)
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, NLIST, devices=(0, 0)))
    assert g.group_size == 2
    g.centroids = data(dim)[3]
    g.add(X, ids)
    refused(g, Q, ids, "group")


def test_refused_arguments():
    dim = 32
    X, Q, ids, _ = data(dim)
    g = make(dim, "il")
    L = vdb.lib()
    req = np.ascontiguousarray(ids[:4])
    p = req.ctypes.data_as(ctypes.c_void_p)
    D, I = np.empty((4, 10), dtype=np.float32), np.empty((4, 10), dtype=np.uint64)
    dp, ip = D.ctypes.data_as(ctypes.c_void_p), I.ctypes.data_as(ctypes.c_void_p)
    assert L.vdb_ivf_fetch_ids(g._h, None, 4, None, None, None) == -1  # null ids with n > 0
    assert L.vdb_ivf_search_ids(g._h, None, 4, 3, 10, dp, ip, None) == -1
    assert L.vdb_ivf_search_ids(g._h, p, 4, 3, 10, None, ip, None) == -1  # null distances
    assert L.vdb_ivf_search_ids(g._h, p, 4, 3, 10, dp, None, None) == -1  # null result_ids
    assert L.vdb_ivf_fetch_ids(g._h, p, 2 ** 31, None, None, None) == UNSUPPORTED  # (refused before ids is read)
    assert L.vdb_ivf_fetch_ids_device(g._h, p, 2 ** 31, None, None, None) == UNSUPPORTED
    assert L.vdb_ivf_search_ids(g._h, p, 2 ** 31, 3, 10, dp, ip, None) == UNSUPPORTED
    assert L.vdb_ivf_search_ids(g._h, p, 4, 3, 10, dp, ip, None) == 0  # found may be NULL
    Dr, Ir = g.search(X[:4], nprobe=3, k=10)
    assert np.array_equal(I, Ir) and np.array_equal(bits(D), bits(Dr))


def test_empty_index():
    dim = 32
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, NLIST))
    g.centroids = data(dim)[3]
    V, F = g.fetch_ids([0, 1, NONE])
    assert not F.any() and not V.any()
    D, I, F = g.search_ids([0, 1], nprobe=3, k=5)
    assert not F.any() and np.all(I == NONE) and np.all(D == FMAX)


# ---- 9. searches concurrent with fetches ----
def test_concurrent_with_searches():
    dim = 32
    X, Q, ids, _ = data(dim)
    g = make(dim, "rows")
    rounds = 20
    batches = [Q[:8], Q[8:]]
    want_s = [g.search(b, nprobe=3, k=10) for b in batches]
    req = U(np.random.default_rng(9).permutation(ids)[:500], NONE, N + 3)
    want_f = g.fetch_ids(req)
    want_q = g.search_ids(req[490:], nprobe=3, k=10)
    results = {0: [], 1: [], 2: []}
    errors = []

    def searcher(t):
        try:
            for _ in range(rounds):
                results[t].append(g.search(batches[t], nprobe=3, k=10))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    def fetcher():
        try:
            for _ in range(rounds):
                results[2].append((g.fetch_ids(req), g.search_ids(req[490:], nprobe=3, k=10)))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=searcher, args=(0,)), threading.Thread(target=searcher, args=(1,)),
          threading.Thread(target=fetcher)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
    for t in (0, 1):
        assert len(results[t]) == rounds
        for D, I in results[t]:
            assert np.array_equal(I, want_s[t][1]) and np.array_equal(bits(D), bits(want_s[t][0]))
    assert len(results[2]) == rounds
    for (V, F), (D, I, Fq) in results[2]:
        assert np.array_equal(F, want_f[1]) and np.array_equal(bits(V), bits(want_f[0]))
        assert np.array_equal(Fq, want_q[2]) and np.array_equal(I, want_q[1])
        assert np.array_equal(bits(D), bits(want_q[0]))
