"""GPU: vdb_ivf_upsert(_device) (replace and insert in one device compaction) against the CPU oracle.

Definition under test: the winners W of a request are, for every distinct id, the entry with the
largest index (last write wins), in request order; the handle after the call is the handle after
remove_ids(all request ids) followed by add(W). So in every case the expected state is a fresh
OracleIndex with the handle's centroids, add(surviving old rows in original order), then add(W),
and totals, list sizes, every list's contents (ids and row bits) and searches at (nprobe 3, k 10),
(nlist, 10) and (2, 1024) (ids and distance bits) must match it.

Base shape (that of test_gpu_remove.py): N = 3000, Q = 32, nlist = 8, dimensions 32 and 30 (30
pads); requests are chosen from the handle's own lists so each condition holds by construction.
Every case starts from a handle that has searched once, so that a screen exists.
"""
import numpy as np
import pytest

import oracle
from conftest import load_vdb
from cosine_ref import cos_map, unit_rows_ref

vdb = load_vdb()
pytestmark = pytest.mark.gpu

N, NQ, NLIST = 3000, 32, 8
NONE = np.iinfo(np.uint64).max
K_BIG = 1024  # above the rows two probed lists hold: unfilled slots and pad lanes take part
BLOCK_BYTES = 64 * (64 * 4 + 8)  # one arena block: dimensions 30 and 32 both pad to 64 floats
SEARCHES = ((3, 10), (NLIST, 10), (2, K_BIG))
STATE, UNSUPPORTED = -5, -4
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
    """(X, Q, ids, centroids, X2) of the base shape, computed once per dimension and never
    changed. ids ascend, so searchsorted maps an id to its row; X2: 1000 rows that are not stored."""
    if dim not in _data:
        X, Q, ids = oracle.reference_test_data(N, NQ, dim, seed=1000 + dim)
        assert np.all(np.diff(ids.astype(np.int64)) > 0) and int(ids[-1]) < 10 ** 6
        C = np.ascontiguousarray(X[:: N // NLIST][:NLIST])
        X2, _, _ = oracle.reference_test_data(1000, 1, dim, seed=4000 + dim)
        for a in (X, Q, ids, C, X2):
            a.setflags(write=False)
        _data[dim] = (X, Q, ids, C, X2)
    return _data[dim]


def fresh_ids(n, start=10 ** 6):
    return np.arange(start, start + n, dtype=np.uint64)


def make(dim, metric=0, ids=None, searched=True, **cfg):
    X, Q, ids0, C, _ = data(dim)
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, NLIST, vdb.Metric(metric), **cfg))
    g.centroids = C
    g.add(X, ids0 if ids is None else ids)
    if searched:
        g.search(Q, nprobe=3, k=10)
    return g


def winners(req):
    """Mask over the request: the last entry of every distinct id."""
    req = np.asarray(req, dtype=np.uint64)
    last = {}
    for i, v in enumerate(req.tolist()):
        last[v] = i
    w = np.zeros(len(req), bool)
    w[list(last.values())] = True
    return w


def expected(g, dim, metric, parts):
    """The oracle given the handle's centroids and `parts`, a sequence of (rows, ids) adds."""
    o = oracle.OracleIndex(dim, NLIST, metric)
    o.centroids = g.centroids
    for V, I in parts:
        if len(I):
            o.add(V, I)
    return o


def assert_after(g, o, Q, searches=SEARCHES, unfilled=True, mapped=False):
    assert g.get_total_vectors() == o.total_vectors
    sizes = g.list_sizes()
    assert sizes.tolist() == [o.list_count(l) for l in range(NLIST)]
    dim = Q.shape[1]
    usage = int(sizes.sum()) * (dim * 4 + 8)
    if g.cache_stats()["capacity_bytes"]:  # the tier: only the lists the cache holds count
        assert g.get_gpu_memory_usage() <= usage
    else:
        assert g.get_gpu_memory_usage() == usage
    for l in range(NLIST):
        gv, gi = g.get_list(l)
        ov, oi = o.get_list(l)
        assert np.array_equal(gi, oi), f"list {l}: ids or their order differ"
        assert np.array_equal(bits(gv), bits(ov)), f"list {l}: row bits differ"
    for nprobe, k in searches:
        Dr, Ir = o.search(unit_rows_ref(Q) if mapped else Q, nprobe, k)
        if mapped:
            Dr = cos_map(Dr, Ir)
        if k == K_BIG and unfilled:
            assert (Ir == NONE).any(), "the large-k search must leave unfilled slots"
        assert_same(*g.search(Q, nprobe=nprobe, k=k), Dr, Ir)


def lists_of(g):
    return [g.get_list(l)[1] for l in range(NLIST)]


def snapshot(g):
    """Every list's (row bits, ids); None for a list this handle does not store."""
    out = []
    for l in range(NLIST):
        try:
            v, i = g.get_list(l)
            out.append((bits(v).copy(), i.copy()))
        except vdb.VdbError:
            out.append(None)
    return out


def same_snapshot(a, b):
    return all((x is None and y is None) or (x is not None and y is not None and np.array_equal(x[0], y[0])
                                             and np.array_equal(x[1], y[1])) for x, y in zip(a, b))


def upsert_and_check(g, dim, metric, cur_X, cur_ids, V, req, call=None, **after):
    """Upsert (V, req) into g, which stores (cur_X, cur_ids) in that add order; compare with the
    oracle. Returns the oracle."""
    Q = data(dim)[1]
    V = np.ascontiguousarray(V, dtype=np.float32).reshape(-1, dim)
    req = np.asarray(req, dtype=np.uint64)
    keep = ~np.isin(cur_ids, req)
    w = winners(req)
    replaced, inserted = (call or g.upsert)(V, req)
    assert replaced == int((~keep).sum())
    assert inserted == int(w.sum()) == len(set(req.tolist()))
    o = expected(g, dim, metric, [(cur_X[keep], cur_ids[keep]), (V[w], req[w])])
    assert_after(g, o, Q, unfilled=metric != 2, **after)
    return o


# ---- 1. request patterns ----
@pytest.mark.parametrize("dim", [32, 30])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_patterns(metric, dim):
    X, Q, ids, C, X2 = data(dim)
    # (Cosine (2) leaves every centroid distance at 0.0f, so every row is assigned to list 0: the
    # conditions about rows changing list cannot hold for it and are asserted for metrics 0 and 1)
    moves = metric != 2

    def run(pick):
        """A fresh, searched handle; upsert pick(lists) -> (rows, ids); compare. Returns
        (handle, lists before, lists after, request ids)."""
        g = make(dim, metric)
        before = lists_of(g)
        V, req = pick(before)
        upsert_and_check(g, dim, metric, X, ids, V, req)
        return g, before, lists_of(g), np.asarray(req, dtype=np.uint64)

    def list_of(ls):
        return {int(i): l for l in range(NLIST) for i in ls[l]}

    def middle(ls):  # a stored list of middling size
        order = sorted((l for l in range(NLIST) if len(ls[l])), key=lambda l: len(ls[l]))
        return order[len(order) // 2]

    # (a) every id is stored
    g, _, _, req = run(lambda ls: (X2, ids[::3]))
    assert np.isin(req, ids).all() and g.get_total_vectors() == N
    # (b) no id is stored: an add
    g, before, after, req = run(lambda ls: (X2[:500], fresh_ids(500)))
    assert not np.isin(req, ids).any() and g.get_total_vectors() == N + 500
    for l in range(NLIST):  # the old rows stay where they were
        assert np.array_equal(after[l][:len(before[l])], before[l])
    # (c) mixed, in shuffled order
    perm = np.random.RandomState(7).permutation(700)
    g, _, _, req = run(lambda ls: (X2[:700][perm], np.concatenate([ids[5::7][:400], fresh_ids(300)])[perm]))
    assert np.isin(req, ids).sum() == 400 and g.get_total_vectors() == N + 300
    # (d) the new vectors are other rows' vectors: most rows change list
    g, before, after, req = run(lambda ls: (X[(np.arange(1000) * 3 + 1501) % N], ids[::3]))
    was, now = list_of(before), list_of(after)
    changed = sum(was[int(i)] != now[int(i)] for i in req)
    assert changed > len(req) // 2 if moves else changed == 0
    # (e) the new vectors equal the old ones: every row lands in its own list, at its end
    g, before, after, req = run(lambda ls: (X[::4], ids[::4]))
    was = list_of(before)
    for l in range(NLIST):
        mine = np.array([i for i in req if was[int(i)] == l], dtype=np.uint64)
        assert np.array_equal(after[l][len(after[l]) - len(mine):], mine)
        assert len(after[l]) == len(before[l])
    # (f) every row of one list, with the vectors of rows another list holds: the list ends empty
    picked = []

    def whole_list(ls):
        m = middle(ls)
        t = next(l for l in range(NLIST) if l != m and len(ls[l])) if moves else m
        picked.append((m, t))
        donors = np.searchsorted(ids, ls[t])
        return X[donors[np.arange(len(ls[m])) % len(donors)]], ls[m]

    g, before, after, req = run(whole_list)
    m, t = picked[0]
    if moves:
        assert len(after[m]) == 0 and len(after[t]) == len(before[t]) + len(before[m])
        assert g.get_total_vectors() == N
    # (g) exactly the rows of a list's last, partial block
    tail = []

    def last_block(ls):
        l = next(l for l in range(NLIST) if len(ls[l]) > 64 and len(ls[l]) % 64)
        tail.append(l)
        r = ls[l][len(ls[l]) // 64 * 64:]
        return X2[:len(r)], r

    g, before, after, req = run(last_block)
    assert 0 < len(req) < 64 and len(before[tail[0]]) % 64 == len(req)
    # (h) a request of one row
    g, _, _, req = run(lambda ls: (X2[:1], ids[17:18]))
    assert len(req) == 1 and g.get_total_vectors() == N


# ---- 2. last write wins ----
def test_last_write_wins():
    dim = 32
    X, Q, ids, C, X2 = data(dim)
    # 200 entries: id A at 0, 63, 64 and 199, id B at 127 and 128 (both cross the 64-entry
    # ballot boundary), the others distinct, half of them stored
    A, B = ids[1234], np.uint64(10 ** 6 + 5000)
    req = np.concatenate([ids[7::29][:100], fresh_ids(100)]).astype(np.uint64)
    assert A not in req and B not in req
    for p in (0, 63, 64, 199):
        req[p] = A
    for p in (127, 128):
        req[p] = B
    V = X2[:200]
    assert len({bits(V[p]).tobytes() for p in (0, 63, 64, 199)}) == 4
    g = make(dim)
    upsert_and_check(g, dim, 0, X, ids, V, req)
    assert len(set(req.tolist())) == 200 - 3 - 1
    got, found = g.fetch_ids(np.array([A, B], dtype=np.uint64))
    assert found.tolist() == [1, 1]
    assert np.array_equal(bits(got[0]), bits(V[199])) and np.array_equal(bits(got[1]), bits(V[128]))
    for i in (A, B):
        assert sum(int((l == i).sum()) for l in lists_of(g)) == 1
    # one id 130 times
    g = make(dim)
    req = np.full(130, ids[77], dtype=np.uint64)
    V = X2[200:330]
    upsert_and_check(g, dim, 0, X, ids, V, req)
    got, found = g.fetch_ids(req[:1])
    assert found[0] == 1 and np.array_equal(bits(got[0]), bits(V[129]))
    assert g.get_total_vectors() == N


# ---- 3. an id stored more than once ----
def test_ids_stored_twice_all_go():
    dim = 32
    X, Q, ids, C, X2 = data(dim)
    dup = ids % 1500
    g = make(dim, ids=dup)
    ls = lists_of(g)
    where = {}
    for l in range(NLIST):
        for i in ls[l]:
            where.setdefault(int(i), []).append(l)
    two = next(i for i, w in sorted(where.items()) if len(w) == 2 and w[0] != w[1])
    keep = dup != two
    assert int((~keep).sum()) == 2
    req = np.array([two], dtype=np.uint64)
    r, w = g.upsert(X2[:1], req)
    assert (r, w) == (2, 1) and g.get_total_vectors() == N - 1
    assert_after(g, expected(g, dim, 0, [(X[keep], dup[keep]), (X2[:1], req)]), Q)


# ---- 4. the twin: remove_ids + add(W) on a second handle ----
@pytest.mark.parametrize("dim", [32, 30])
def test_twin_of_remove_then_add(dim):
    X, Q, ids, C, X2 = data(dim)
    req = np.concatenate([ids[3::5], fresh_ids(150), ids[3::50], fresh_ids(20)])
    V = X2[:len(req)]
    w = winners(req)
    assert not w.all()
    a, b = make(dim), make(dim)
    replaced, inserted = a.upsert(V, req)
    assert b.remove_ids(req) == replaced == 600
    b.add(V[w], req[w])
    assert inserted == int(w.sum())
    assert same_snapshot(snapshot(a), snapshot(b))
    assert a.get_total_vectors() == b.get_total_vectors()
    for nprobe, k in SEARCHES:
        assert_same(*a.search(Q, nprobe=nprobe, k=k), *b.search(Q, nprobe=nprobe, k=k))


# ---- 5. Metric.CosineDistance: the winners are normalised once ----
@pytest.mark.parametrize("dim", [32, 30])
def test_cosine_distance(dim):
    X, Q, ids, C, X2 = data(dim)
    g = make(dim, 3)
    req = np.concatenate([ids[2::6], fresh_ids(200), ids[2:200:6]])
    V = np.ascontiguousarray(X2[:len(req)] * np.float32(3.5))  # (far from unit length)
    w = winners(req)
    keep = ~np.isin(ids, req)
    replaced, inserted = g.upsert(V, req)
    assert (replaced, inserted) == (500, int(w.sum()))
    WU = unit_rows_ref(V[w])
    got, found = g.fetch_ids(req[w])
    assert found.all() and np.array_equal(bits(got), bits(WU))
    o = oracle.OracleIndex(dim, NLIST, 1)  # InnerProduct over unit rows, mapped by 1 + d
    o.centroids = g.centroids
    o.add(unit_rows_ref(X[keep]), ids[keep])
    o.add(WU, req[w])
    assert_after(g, o, Q, mapped=True, unfilled=False)


# ---- 6. the device variant ----
def test_device_variant_equals_host():
    import torch
    dim = 30
    X, Q, ids, C, X2 = data(dim)
    perm = np.random.RandomState(11).permutation(500)
    req = np.concatenate([ids[1::10], fresh_ids(150), ids[1:500:10]])[perm]
    V = np.ascontiguousarray(X2[:500][perm])
    a, b = make(dim), make(dim)
    t_vec = torch.from_numpy(V).to("cuda:0")
    t_ids = torch.from_numpy(req.view(np.int64).copy()).to("cuda:0")
    torch.cuda.synchronize()
    upsert_and_check(a, dim, 0, X, ids, V, req, call=lambda v, r: a.upsert_device(t_vec.data_ptr(), t_ids.data_ptr(), len(r)))
    assert b.upsert(V, req) == (300, 450)
    assert same_snapshot(snapshot(a), snapshot(b))
    assert np.array_equal(t_vec.cpu().numpy(), V) and np.array_equal(t_ids.cpu().numpy().view(np.uint64), req)


# ---- 7. edges ----
def test_empty_request_touches_nothing():
    dim = 32
    X, Q, ids, C, X2 = data(dim)
    g = make(dim)
    flt = g.prepare_filter(ids[::2], include=True)
    want = g.search_prepared(Q, flt, nprobe=3, k=10)
    held, snap = g.gpu_bytes_allocated(), snapshot(g)
    assert g.upsert(np.empty((0, dim), np.float32), np.empty(0, np.uint64)) == (0, 0)
    assert not flt.stale and g.gpu_bytes_allocated() == held and same_snapshot(snapshot(g), snap)
    assert_same(*g.search_prepared(Q, flt, nprobe=3, k=10), *want)
    # any n > 0 makes the filter stale
    assert g.upsert(X2[:1], fresh_ids(1)) == (0, 1)
    assert flt.stale
    with pytest.raises(vdb.VdbError) as e:
        g.search_prepared(Q, flt, nprobe=3, k=10)
    assert e.value.code == STATE


def test_fetch_returns_the_new_row():
    dim = 30
    X, Q, ids, C, X2 = data(dim)
    g = make(dim)
    req = np.concatenate([ids[100:110], fresh_ids(5)])
    g.upsert(X2[:15], req)
    got, found = g.fetch_ids(np.concatenate([req, ids[99:100]]))
    assert found.all()
    assert np.array_equal(bits(got[:15]), bits(X2[:15])) and np.array_equal(bits(got[15]), bits(X[99]))


def test_trained_empty_index():
    dim = 32
    X, Q, ids, C, X2 = data(dim)
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, NLIST))
    g.centroids = C
    g.search(Q, nprobe=3, k=10)
    req = np.concatenate([ids[:400], ids[:40]])  # 40 ids twice
    V = X2[:440]
    empty = np.empty(0, np.uint64)
    upsert_and_check(g, dim, 0, np.empty((0, dim), np.float32), empty, V, req)
    assert g.get_total_vectors() == 400


def test_uint64_max_is_an_id_like_any_other():
    dim = 32
    X, Q, ids, C, X2 = data(dim)
    g = make(dim)
    req = np.array([NONE], dtype=np.uint64)
    assert g.upsert(X2[:1], req) == (0, 1)
    assert g.upsert(X2[1:2], req) == (1, 1)  # (the pad slots' value: only the stored row matched)
    assert g.get_total_vectors() == N + 1
    o = expected(g, dim, 0, [(X, ids), (X2[1:2], req)])
    assert_after(g, o, Q, searches=())
    assert sum(int((l == NONE).sum()) for l in lists_of(g)) == 1
    # and every other row is still found where the oracle has it
    keep_mask = g.prepare_filter(req, include=False)
    assert keep_mask.allowed == N


# ---- 8. the list-cache tier ----
# In the tier an exact-path search (k > 64) needs every list a query probes resident at once,
# and the cache here is about as large as the lists before the upsert: that search probes one
# list, as in test_gpu_remove.py. The screened searches load no list.
TIER_SEARCHES = ((3, 10), (NLIST, 10), (1, K_BIG))


def test_tier_entered_by_an_insert_heavy_upsert():
    dim, metric = 32, 1  # (inner product: lists of similar size, each far below the cache)
    X, Q, ids, C, X2 = data(dim)
    row = dim * 4 + 8
    g = make(dim, metric, max_gpu_memory=N * row + 10 * row)  # just above the lists' bytes
    assert g.cache_stats()["capacity_bytes"] == 0
    req = np.concatenate([ids[::30], fresh_ids(500)])  # 100 replaced, 500 more rows
    upsert_and_check(g, dim, metric, X, ids, X2[:600], req, searches=TIER_SEARCHES)
    assert g.cache_stats()["capacity_bytes"] > 0


def test_tier_left_by_a_shrinking_upsert():
    dim = 32
    X, Q, ids, C, X2 = data(dim)
    row = dim * 4 + 8
    dup = ids % 1500  # every id twice
    g = make(dim, ids=dup, max_gpu_memory=N * row * 3 // 4)  # the add exceeds it: the tier
    assert g.cache_stats()["capacity_bytes"] > 0
    req = np.arange(1000, dtype=np.uint64)  # 2000 rows go, 1000 come: under the cap
    upsert_and_check(g, dim, 0, X, dup, X2, req)
    assert g.cache_stats()["capacity_bytes"] == 0 and g.get_total_vectors() == 2000


def test_tier_host_home_replace_only():
    # Inner product: its lists are of similar size here, so a cache of a quarter of the blocks
    # holds any one list; the exact-path search (k > 64) probes one list, the screened tier
    # loads no list and also runs nprobe = nlist (as in test_gpu_remove.py).
    dim, metric = 32, 1
    X, Q, ids, C, X2 = data(dim)
    g = make(dim, metric, searched=False, max_gpu_memory=0)
    per_list = [(int(c) + 63) // 64 for c in g.list_sizes()]
    quarter = sum(per_list) // 4
    assert max(per_list) <= quarter
    g.set_option("list_cache_bytes", quarter * BLOCK_BYTES)
    assert g.cache_stats()["capacity_bytes"] > 0
    g.search(Q, nprobe=1, k=10)
    # the rows keep their vectors, so every list keeps its size and still fits the cache
    upsert_and_check(g, dim, metric, X, ids, X[1::3], ids[1::3], searches=((1, 10), (1, K_BIG), (NLIST, 10)))
    assert g.cache_stats()["capacity_bytes"] > 0


# ---- 9. refusals leave the handle untouched ----
def test_refused_on_a_file_home(tmp_path):
    dim = 32
    X, Q, ids, C, X2 = data(dim)
    g = make(dim)
    path = str(tmp_path / "lists.ivf")
    g.save(path)
    sizes = g.list_sizes()
    h = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, NLIST))
    h.set_option("list_cache_bytes", (int(((sizes + 63) // 64).sum()) + 2) * BLOCK_BYTES)
    h.open_lists(path)
    h.search(Q, nprobe=3, k=10)
    snap = snapshot(h)
    with pytest.raises(vdb.VdbError, match="read-only") as e:
        h.upsert(X2[:10], ids[:10])
    assert e.value.code == STATE
    assert same_snapshot(snapshot(h), snap) and np.array_equal(h.list_sizes(), sizes)


def test_refused_on_a_shard():
    dim = 32
    X, Q, ids, C, X2 = data(dim)
    g = make(dim)
    g.set_shard(0, 2)
    g.search(Q, nprobe=3, k=10)
    sizes, snap = g.list_sizes(), snapshot(g)
    assert any(s is None for s in snap) and any(s is not None for s in snap)
    with pytest.raises(vdb.VdbError, match="sharded") as e:
        g.upsert(X2[:10], ids[:10])
    assert e.value.code == UNSUPPORTED
    assert same_snapshot(snapshot(g), snap) and np.array_equal(g.list_sizes(), sizes)


def test_refused_on_a_group():
    dim = 32
    X, Q, ids, C, X2 = data(dim)
    g = make(dim, devices=(0, 0))
    assert g.group_size == 2
    sizes, snap = g.list_sizes(), snapshot(g)
    with pytest.raises(vdb.VdbError, match="group") as e:
        g.upsert(X2[:10], ids[:10])
    assert e.value.code == UNSUPPORTED
    assert same_snapshot(snapshot(g), snap) and np.array_equal(g.list_sizes(), sizes)


# ---- 10. the timing record ----
def test_timing_record():
    dim = 32
    X, Q, ids, C, X2 = data(dim)
    g = make(dim)
    req = np.concatenate([ids[::10], fresh_ids(100), ids[:50:10]])
    replaced, inserted = g.upsert(X2[:len(req)], req)
    t = g.upsert_last_timing()
    assert t["rows_written"] == inserted == 400 and t["rows_kept"] == N - replaced
    assert t["rows_kept"] + t["rows_written"] == g.get_total_vectors()
    assert all(t[k] >= 0.0 for k in ("resolve_ms", "mark_ms", "plan_ms", "move_ms"))
    g.upsert(np.empty((0, dim), np.float32), np.empty(0, np.uint64))
    assert g.upsert_last_timing() == {"resolve_ms": 0.0, "mark_ms": 0.0, "plan_ms": 0.0, "move_ms": 0.0,
                                      "rows_kept": 0, "rows_written": 0}
