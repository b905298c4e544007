"""GPU: vdb_ivf_search_filtered (allow / deny id sets through a masked exact scan) against the
CPU oracle.

Definition under test: a filtered search returns exactly what vdb_ivf_search returns on a handle
built from the same centroids that holds only the allowed rows in their original order. So in
every case the expected answer is an OracleIndex with the handle's centroids whose lists are
set_list to the allowed rows in order, and ids and distance bits must match it.

Shape: 2,940 rows placed with add_to_lists into nlist = 12 lists of 0, 1, 63, 64, 65, 130 rows,
one hub list of 1,500 rows (24 blocks: every wave of a workgroup and two segments) and five
more of a few blocks each; dimensions 20 (padded) and 128; 40 queries. Ten ids are stored
twice, in two different lists.
"""
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
EXCLUDE, INCLUDE = False, True
_data = {}


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
    """A handle in one of the three list layouts a filtered call can meet."""
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


def allowed_rows(ids, flt, include):
    hit = np.isin(ids, np.asarray(flt, dtype=np.uint64))
    return hit if include else ~hit


def oracle_of(dim, metric, C, X, ids, lists, allow):
    o = oracle.OracleIndex(dim, NLIST, metric)
    o.centroids = C
    for l in range(NLIST):
        rows = np.flatnonzero((lists == l) & allow)
        o.set_list(l, X[rows], ids[rows])
    return o


def oracle_search(o, Q, nprobe, k, stale=True):
    if stale:
        return o.search(Q, nprobe, k)
    # stale_slots 0: an empty probed list contributes nothing, which is what the reference's
    # per-call slot logic gives a call of one query
    out = [o.search(Q[i:i + 1], nprobe, k) for i in range(Q.shape[0])]
    return np.concatenate([d for d, _ in out]), np.concatenate([i for _, i in out])


def check(g, dim, metric, flt, include, nprobe=5, k=10, stale=True, rows=None):
    X, Q, ids, lists, C = rows or data(dim)
    allow = allowed_rows(ids, flt, include)
    o = oracle_of(dim, metric, C, X, ids, lists, allow)
    Dr, Ir = oracle_search(o, Q, nprobe, k, stale)
    assert_same(*g.search_filtered(Q, ids=flt, include=include, nprobe=nprobe, k=k), Dr, Ir)
    return allow, o, (Dr, Ir)


def first_probes(dim, metric, nprobe=5):
    _, Q, _, _, C = data(dim)
    o = oracle.OracleIndex(dim, NLIST, metric)
    o.centroids = C
    return o.select_nprobe(Q[0], nprobe)


# ---- 1. filters x metrics x layouts ----
@pytest.mark.parametrize("dim", [20, 128])
@pytest.mark.parametrize("layout", ["il", "rows", "stale"])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_filters(metric, layout, dim):
    X, Q, ids, lists, C = data(dim)
    g = make(dim, metric, layout)
    hub = ids[lists == HUB]
    twice = hub[100]
    assert (ids == twice).sum() == 2 and len(set(lists[ids == twice].tolist())) == 2

    # EXCLUDE of every id, INCLUDE of nothing: every slot unfilled
    for flt, inc in ((ids, EXCLUDE), ([], INCLUDE)):
        D, I = g.search_filtered(Q, ids=flt, include=inc, nprobe=5, k=10)
        assert np.all(I == NONE) and np.all(D == FMAX)
        check(g, dim, metric, flt, inc)
    # INCLUDE of one id
    allow, _, _ = check(g, dim, metric, [hub[700]], INCLUDE)
    assert allow.sum() == 1
    # every other stored row: the masks alternate
    check(g, dim, metric, ids[::2], EXCLUDE)
    check(g, dim, metric, ids[::2], INCLUDE)
    # whole 64-slot blocks in the middle of the hub list go (and half of the block after them)
    check(g, dim, metric, hub[128:416], EXCLUDE)
    check(g, dim, metric, np.concatenate([hub[:64], hub[448:]]), INCLUDE)
    # whole lists go, among them lists the first query probes (and the list of exactly one block)
    probed = first_probes(dim, metric)
    gone = np.isin(lists, np.concatenate([probed[:2], [3]]))
    for stale in (True, False):
        g.set_stale_slots(stale)
        check(g, dim, metric, ids[gone], EXCLUDE, stale=stale)
        check(g, dim, metric, ids[~gone], INCLUDE, stale=stale)
    g.set_stale_slots(True)
    # ids that are not stored, repeats and UINT64_MAX (the pad slots' value), in both modes
    other = ids[lists == 7][3]
    odd = np.array([1, 2 ** 40, NONE, hub[5], hub[5], other, NONE, other, 5], dtype=np.uint64)
    for inc in (EXCLUDE, INCLUDE):
        allow, _, _ = check(g, dim, metric, odd, inc)
        assert allow.sum() == (2 if inc else N - 2)
    # an id stored in two lists, excluded and included
    allow, _, _ = check(g, dim, metric, [twice], EXCLUDE, nprobe=NLIST)
    assert allow.sum() == N - 2
    check(g, dim, metric, [twice], INCLUDE, nprobe=NLIST)
    # EXCLUDE of nothing: the oracle over every row, and the plain search of the same handle
    # (last: in the "stale" layout the plain search rebuilds the screen)
    _, _, (Dr, Ir) = check(g, dim, metric, [], EXCLUDE)
    assert_same(*g.search(Q, nprobe=5, k=10), Dr, Ir)
    assert_same(*g.search_filtered(Q, ids=[], nprobe=5, k=10), Dr, Ir)


# ---- 2. k and nprobe ----
@pytest.mark.parametrize("layout", ["il", "rows"])
def test_k_and_nprobe(layout):
    dim = 20
    X, Q, ids, lists, C = data(dim)
    g = make(dim, 0, layout)
    sparse = ids[::40]  # at most 38 allowed rows in any list: k = 64 exceeds every probed list
    assert max(np.bincount(lists[::40], minlength=NLIST)) < 64
    for k in (1, 10, 64):
        for nprobe in (1, 5, 12, 40):  # (40: clamped to nlist)
            allow, o, _ = check(g, dim, 0, sparse, INCLUDE, nprobe=nprobe, k=k)
            # the scan computed one distance per allowed row of every probed list, no more
            want = sum(int(allow[lists == l].sum()) for q in Q for l in o.select_nprobe(q, nprobe))
            assert g.filter_last_timing()["pairs_scanned"] == want
            check(g, dim, 0, ids[1::2], EXCLUDE, nprobe=nprobe, k=k)


# ---- 3. stale slots across batch boundaries ----
@pytest.mark.parametrize("stale", [True, False])
def test_stale_slots_do_not_depend_on_batch(stale):
    dim = 20
    X, Q, ids, lists, C = data(dim)
    got = []
    for batch in (8, None):
        g = make(dim, 0, "il")
        g.set_stale_slots(stale)
        if batch:
            g.set_batch(batch)
        out = []
        for nprobe, keep_lists in ((5, [HUB, 1, 4]), (12, [7]), (3, [2, 9, 10])):
            flt = ids[np.isin(lists, keep_lists)]  # every other list has no allowed row
            _, _, ref = check(g, dim, 0, flt, INCLUDE, nprobe=nprobe, k=10, stale=stale)
            out.append(g.search_filtered(Q, ids=flt, include=True, nprobe=nprobe, k=10))
            assert_same(*out[-1], *ref)
        got.append(out)
    for (Da, Ia), (Db, Ib) in zip(*got):
        assert_same(Da, Ia, Db, Ib)


# ---- 4. the handle is left exactly as found ----
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
    for flt, inc in ((ids[::2], EXCLUDE), (ids[::7], INCLUDE), ([], INCLUDE)):
        g.search_filtered(Q, ids=flt, include=inc, nprobe=5, k=10)
        assert state(g) == before
    D0, I0 = plain_only.search(Q, nprobe=5, k=10)
    assert_same(*g.search(Q, nprobe=5, k=10), D0, I0)
    g.search_filtered(Q, ids=ids[::2], nprobe=5, k=10)
    assert_same(*g.search(Q, nprobe=5, k=10), D0, I0)
    assert state(g) == state(plain_only)


# ---- 5. after remove_ids and a further add ----
def test_after_mutations():
    dim = 20
    X, Q, ids, lists, C = data(dim)
    g = make(dim, 0, "rows")
    gone = np.isin(ids, ids[::3])
    assert g.remove_ids(ids[::3]) == int(gone.sum())
    keep = ~gone
    rows = (X[keep], Q, ids[keep], lists[keep], C)
    flt = ids[::2]
    check(g, dim, 0, flt, EXCLUDE, rows=rows)  # (screen stale: interleaved)
    g.search(Q, nprobe=5, k=10)
    check(g, dim, 0, flt, INCLUDE, rows=rows)  # (row-major again)
    X2, _, _ = oracle.reference_test_data(400, 1, dim, seed=91)
    ids2 = np.arange(10 ** 6, 10 ** 6 + 400, dtype=np.uint64)
    lists2 = (np.arange(400) % NLIST).astype(np.uint32)
    g.add_to_lists(X2, ids2, lists2)
    rows = (np.concatenate([X[keep], X2]), Q, np.concatenate([ids[keep], ids2]), np.concatenate([lists[keep], lists2]), C)
    for inc in (EXCLUDE, INCLUDE):
        check(g, dim, 0, np.concatenate([flt, ids2[::3]]), inc, rows=rows)


# ---- 6. plain and filtered searches from four threads ----
def test_concurrent_plain_and_filtered():
    dim = 20
    X, Q, ids, lists, C = data(dim)
    g = make(dim, 0, "rows")
    T, loops = 4, 12
    jobs = [(None, None), (ids[::2], EXCLUDE), (ids[::5], INCLUDE), (ids[np.isin(lists, [HUB, 2])], EXCLUDE)]
    batches = [Q[t * 10:(t + 1) * 10] for t in range(T)]

    def run(t, j):
        flt, inc = jobs[j]
        if flt is None:
            return g.search(batches[t], nprobe=5, k=10)
        return g.search_filtered(batches[t], ids=flt, include=inc, nprobe=5, k=10)

    alone = [[run(t, j) for j in range(len(jobs))] for t in range(T)]
    results = [[] for _ in range(T)]
    errors = []

    def worker(t):
        try:
            for i in range(loops):
                j = (t + i) % len(jobs)
                results[t].append((j, run(t, j)))
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
        for j, (D, I) in results[t]:
            assert_same(D, I, *alone[t][j])


# ---- 7. refusals name their cause and leave the handle untouched ----
def refused(g, Q, code, match, **kw):
    D0, I0 = g.search(Q, nprobe=5, k=10)
    sizes = g.list_sizes().tolist()
    args = dict(ids=[1, 2, 3], nprobe=5, k=10)
    args.update(kw)
    with pytest.raises(vdb.VdbError, match=match) as e:
        g.search_filtered(Q, **args)
    assert e.value.code == code
    assert g.list_sizes().tolist() == sizes
    assert_same(*g.search(Q, nprobe=5, k=10), D0, I0)


def test_refusals():
    dim = 20
    X, Q, ids, lists, C = data(dim)
    UNSUPPORTED, INVALID = -4, -1
    g = make(dim, 0, "rows")
    refused(g, Q, UNSUPPORTED, "k <= 64", k=65)
    # an invalid mode, through the C ABI
    import ctypes
    L = vdb.lib()
    q = np.ascontiguousarray(Q)
    f = np.array([1, 2], dtype=np.uint64)
    D = np.empty((NQ, 10), np.float32)
    I = np.empty((NQ, 10), np.uint64)
    D0, I0 = g.search(Q, nprobe=5, k=10)
    vp = ctypes.c_void_p
    rc = L.vdb_ivf_search_filtered(g._h, vp(q.ctypes.data), NQ, 5, 10, vp(f.ctypes.data), 2, 2, vp(D.ctypes.data),
                                   vp(I.ctypes.data))
    assert rc == INVALID and b"mode" in L.vdb_last_error()
    rc = L.vdb_ivf_search_filtered(g._h, vp(q.ctypes.data), NQ, 5, 10, None, 2, 0, vp(D.ctypes.data), vp(I.ctypes.data))
    assert rc == INVALID and b"null" in L.vdb_last_error()
    assert_same(*g.search(Q, nprobe=5, k=10), D0, I0)
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


# ---- 8. the drop-in C++ class ----
def test_cpp_class_search_filtered():
    cpp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    exe = os.path.join(cpp, "bin", "filter_test")
    subprocess.check_call(["make", "-s", "-C", cpp, exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "filtered searches bit-identical to the CPU path over the allowed rows: yes" in p.stdout
