"""GPU: Metric.CosineDistance (3), true cosine distance served as an inner-product index over
unit rows (include/vdb_ivf.h).

Definition under test: every call's result is the result of the same call on an InnerProduct
handle with the same centroids that stores unit(row) and is asked unit(query), each filled
distance d then reported as 1.0f + d; order, unique-id merge, stale slots and refusals are that
handle's. unit() is cosine_ref.unit_rows_ref, bit for bit. So the expected values come from
oracle.OracleIndex(dim, NLIST, 1) holding unit_rows_ref(X) and asked unit_rows_ref(Q), mapped by
cosine_ref.cos_map; ids and distance bits must match.

Shape (that of test_gpu_range.py): 2,940 rows placed with add_to_lists into nlist = 12 lists of
0, 1, 63, 64, 65, 130 rows, one hub list of 1,500 rows and five more of a few blocks each;
dimensions 20 (padded) and 128; 40 queries; ten ids stored twice, in two different lists.
"""
import numpy as np
import pytest

import oracle
from conftest import load_vdb
from cosine_ref import NONE, cos_map, unit_rows_ref

vdb = load_vdb()
pytestmark = pytest.mark.gpu

NLIST, NQ = 12, 40
LENS = [0, 1, 63, 64, 65, 130, 1500, 257, 320, 200, 191, 149]
HUB = 6
N = sum(LENS)
FMAX = np.finfo(np.float32).max
INF = np.float32(np.inf)
COS, IP = 3, 1
UNSUPPORTED, INVALID = -4, -1
SEARCHES = ((1, 10), (5, 10), (12, 64), (12, 100))  # (nprobe, k); k = 100 takes the exact path
_data = {}
_full = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, ref):
    (D, I), (Dr, Ir) = got, ref
    assert D.shape == Dr.shape and I.shape == Ir.shape
    bad = np.argwhere(I != Ir)
    assert bad.size == 0, f"ids differ at {bad[:5].tolist()}: gpu {I[tuple(bad[0])]} ref {Ir[tuple(bad[0])]}"
    badd = np.argwhere(bits(D) != bits(Dr))
    assert badd.size == 0, f"dist bits differ at {badd[:5].tolist()}: gpu {D[tuple(badd[0])]!r} ref {Dr[tuple(badd[0])]!r}"


def assert_same_range(got, ref):
    (l, D, I), (lr, Dr, Ir) = got, ref
    assert l.tolist() == lr.tolist(), f"lims differ: gpu {l.tolist()} ref {lr.tolist()}"
    assert_same((D, I), (Dr, Ir))


def data(dim):
    """(X, Q, ids, lists, C, XU, QU) computed once per dimension and never changed."""
    if dim not in _data:
        X, Q, ids = oracle.reference_test_data(N, NQ, dim, seed=2000 + dim)
        C = oracle.gen_normal(3000 + dim, NLIST * dim).reshape(NLIST, dim)
        rng = np.random.RandomState(dim)
        lists = rng.permutation(np.repeat(np.arange(NLIST, dtype=np.uint32), LENS))
        ids = ids.copy() * 3 + 7
        hub_rows = np.flatnonzero(lists == HUB)[100:110]
        ids[np.flatnonzero(lists == NLIST - 1)[:10]] = ids[hub_rows]
        XU, QU = unit_rows_ref(X), unit_rows_ref(Q)
        for a in (X, Q, ids, lists, C, XU, QU):
            a.setflags(write=False)
        _data[dim] = (X, Q, ids, lists, C, XU, QU)
    return _data[dim]


def make(dim, metric=COS, screen=1, keep=None, **cfg):
    """A handle holding the test rows: the raw rows in a CosineDistance handle, their unit rows
    (cosine_ref, no product code) in any other. keep: a row mask."""
    X, Q, ids, lists, C, XU, QU = data(dim)
    keep = slice(None) if keep is None else keep
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, NLIST, vdb.Metric(metric), **cfg))
    g.centroids = C
    if not screen:
        g.set_option("screen", 0)
    g.add_to_lists((X if metric == COS else XU)[keep], ids[keep], lists[keep])
    return g


def ip_oracle(dim, keep=None):
    X, Q, ids, lists, C, XU, QU = data(dim)
    keep = np.ones(N, bool) if keep is None else keep
    o = oracle.OracleIndex(dim, NLIST, IP)
    o.centroids = C
    for l in range(NLIST):
        sel = np.flatnonzero((lists == l) & keep)
        o.set_list(l, XU[sel], ids[sel])
    return o


def expected(o, QU, nprobe, k, stale=True):
    """The mapped oracle: the whole call, or (stale_slots off) every query on its own."""
    if stale:
        D, I = o.search(QU, nprobe, k)
    else:
        parts = [o.search(QU[i:i + 1], nprobe, k) for i in range(QU.shape[0])]
        D, I = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    return cos_map(D, I), I


def full(dim, nprobe, keep=None, key="base"):
    """Per query the oracle's whole single-query result: (-dot, mapped distance, id)."""
    kk = (dim, nprobe, key)
    if kk not in _full:
        o, QU = ip_oracle(dim, keep), data(dim)[6]
        out = []
        for i in range(NQ):
            D, I = o.search(QU[i:i + 1], nprobe, N)
            real = I[0] != NONE
            out.append((D[0][real].copy(), cos_map(D[0][real], I[0][real]), I[0][real].copy()))
        _full[kk] = out
    return _full[kk]


def cut(per_query, radius):
    r = np.float32(radius)
    lims, Ds, Is = [0], [], []
    for _, M, I in per_query:
        keep = M <= r
        Ds.append(M[keep])
        Is.append(I[keep])
        lims.append(lims[-1] + int(keep.sum()))
    return np.array(lims, dtype=np.uint64), np.concatenate(Ds).astype(np.float32), np.concatenate(Is).astype(np.uint64)


# ---- 1. the kernel on its own ----
@pytest.mark.parametrize("dim", [1, 3, 20, 64, 65, 128, 257, 768])
def test_unit_rows_kernel(dim):
    import torch
    n = 300
    X = oracle.gen_normal(500 + dim, n * dim).reshape(n, dim).copy()
    X[0] = 0.0
    X[1] = 1e30  # the sum of squares overflows: the row is kept
    X[n - 1] = 0.0
    X[n - 1, dim // 2] = -3.5
    ref = unit_rows_ref(X)
    assert np.array_equal(bits(ref[0]), bits(X[0])) and np.array_equal(bits(ref[1]), bits(X[1]))
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    # (offset 1: a base 4 bytes past a 16-byte boundary: the scalar loads, or the scalar stores)
    for off, ooff in ((0, 0), (1, 0), (0, 1), (1, 1)):
        buf = torch.zeros(n * dim + 1, dtype=torch.float32, device=dev)
        src = buf[off:off + n * dim]
        src.copy_(torch.from_numpy(X.ravel()))
        assert src.data_ptr() % 16 == 4 * off
        out = torch.full((n * dim + 1,), 7.0, dtype=torch.float32, device=dev)
        vdb.unit_rows_device(src.data_ptr(), n, dim, out[ooff:].data_ptr(), s)
        torch.cuda.synchronize()
        got = out[ooff:ooff + n * dim].cpu().numpy().reshape(n, dim)
        bad = np.argwhere(bits(got) != bits(ref))
        assert bad.size == 0, f"dim {dim} offsets {off}, {ooff}: rows differ at {bad[:5].tolist()}"
        assert np.array_equal(bits(src.cpu().numpy()), bits(X.ravel()))  # the input is only read
        assert float(out[0 if ooff else n * dim]) == 7.0  # nothing beside the output is written
    with pytest.raises(vdb.VdbError, match="alias"):
        vdb.unit_rows_device(buf.data_ptr(), n, dim, buf.data_ptr(), s)


# ---- 2. stored rows are unit rows, normalised exactly once ----
@pytest.mark.parametrize("dim", [20, 128])
def test_stored_rows(tmp_path, dim):
    X, Q, ids, lists, C, XU, QU = data(dim)
    g = make(dim)
    assert g.list_sizes().tolist() == LENS

    def check(h):
        for l in range(NLIST):
            sel = np.flatnonzero(lists == l)
            V, I = h.get_list(l)
            assert np.array_equal(I, ids[sel])
            assert np.array_equal(bits(V), bits(XU[sel])), f"list {l}"

    check(g)
    g.search(Q, nprobe=5, k=10)  # (the screen built: the row-major copy)
    check(g)
    path = str(tmp_path / "cos.ivf")
    g.save(path)
    h = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, NLIST, vdb.Metric.CosineDistance))
    h.load(path)
    assert h.list_sizes().tolist() == LENS
    check(h)  # (a second normalisation would change bits)
    assert np.array_equal(bits(h.centroids), bits(C))
    for nprobe, k in SEARCHES[:2]:
        assert_same(h.search(Q, nprobe=nprobe, k=k), g.search(Q, nprobe=nprobe, k=k))


# ---- 3. search parity with the mapped oracle ----
@pytest.mark.parametrize("dim", [20, 128])
@pytest.mark.parametrize("screen", [0, 1])
def test_search_parity(dim, screen):
    X, Q, ids, lists, C, XU, QU = data(dim)
    o = ip_oracle(dim)
    g = make(dim, screen=screen)
    for stale in (True, False):
        g.set_stale_slots(stale)
        for nprobe, k in SEARCHES:
            assert_same(g.search(Q, nprobe=nprobe, k=k), expected(o, QU, nprobe, k, stale))
    shadow = g.profile_read()["screen_shadow"]
    assert shadow in (1, 2) if screen else shadow == 0  # the screen serves cosine
    # unfilled slots stay (FLT_MAX, UINT64_MAX)
    D, I = g.search(Q, nprobe=1, k=10)
    assert np.all(D[I == NONE] == FMAX)


# ---- 4. the same answer from an InnerProduct handle fed the unit rows ----
@pytest.mark.parametrize("dim", [20, 128])
def test_same_as_ip_handle(dim):
    X, Q, ids, lists, C, XU, QU = data(dim)
    g, p = make(dim), make(dim, IP)
    for stale in (True, False):
        g.set_stale_slots(stale)
        p.set_stale_slots(stale)
        for nprobe, k in SEARCHES:
            D, I = p.search(QU, nprobe=nprobe, k=k)
            assert_same(g.search(Q, nprobe=nprobe, k=k), (cos_map(D, I), I))


# ---- 5. add's assignment and train ----
def test_train_and_add():
    n, dim, nlist = 2000, 32, 8
    X, Q, ids = oracle.reference_test_data(n, 10, dim, seed=77)
    XU = unit_rows_ref(X)
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, nlist, vdb.Metric.CosineDistance))
    p = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, nlist, vdb.Metric.InnerProduct))
    g.train(X)
    p.train(XU)
    Cg = g.centroids
    assert np.array_equal(bits(Cg), bits(unit_rows_ref(p.centroids)))
    p.centroids = Cg
    g.add(X, ids)
    p.add(XU, ids)
    assert g.list_sizes().tolist() == p.list_sizes().tolist()
    assert g.get_total_vectors() == n
    for l in range(nlist):
        (Vg, Ig), (Vp, Ip) = g.get_list(l), p.get_list(l)
        assert np.array_equal(Ig, Ip) and np.array_equal(bits(Vg), bits(Vp)), f"list {l}"
    D, I = p.search(unit_rows_ref(Q), nprobe=4, k=10)
    assert_same(g.search(Q, nprobe=4, k=10), (cos_map(D, I), I))


# ---- 6. filtered, prepared and range searches ----
@pytest.mark.parametrize("dim", [20, 128])
def test_filtered_and_prepared(dim):
    X, Q, ids, lists, C, XU, QU = data(dim)
    g = make(dim)
    g.search(Q, nprobe=5, k=10)
    flt = ids[::3]
    for include in (False, True):
        keep = np.isin(ids, flt) == include
        o = ip_oracle(dim, keep)
        f = g.prepare_filter(flt, include=include)
        for nprobe, k in SEARCHES[:3]:
            ref = expected(o, QU, nprobe, k)
            assert_same(g.search_filtered(Q, ids=flt, include=include, nprobe=nprobe, k=k), ref)
            assert_same(g.search_prepared(Q, f, nprobe=nprobe, k=k), ref)
        per = full(dim, 5, keep, key=("filter", include))
        for r in (0.9, INF):
            assert_same_range(g.range_search_prepared(Q, f, r, nprobe=5, reserve=N * NQ), cut(per, r))


@pytest.mark.parametrize("dim", [20, 128])
@pytest.mark.parametrize("screen", [0, 1])
def test_range_search(dim, screen):
    X, Q, ids, lists, C, XU, QU = data(dim)
    g = make(dim, screen=screen)
    g.search(Q, nprobe=5, k=10)
    per = full(dim, 5)
    exact = per[0][1][4]  # a returned (mapped) distance: the comparison is inclusive
    for r in (0.0, 0.9, 1.0, 1.1, 2.5, INF, FMAX, exact, np.nextafter(exact, np.float32(-np.inf), dtype=np.float32)):
        ref = cut(per, r)
        assert_same_range(g.range_search(Q, r, nprobe=5, reserve=N * NQ), ref)
        if r in (1.0, INF):  # (a null filter: the unfiltered call)
            assert_same_range(g.range_search_prepared(Q, None, r, nprobe=5, reserve=N * NQ), ref)
    got = g.range_search(Q, exact, nprobe=5, reserve=N * NQ)
    assert int(got[0][1]) >= 5 and bits(got[1][4:5])[0] == bits(exact)[0] and got[2][4] == per[0][2][4]
    assert g.range_search(Q, -INF, nprobe=5)[0].tolist() == [0] * (NQ + 1)
    with pytest.raises(vdb.VdbError, match="radius"):
        g.range_search(Q, float("nan"), nprobe=5)
    # The order is (-dot, id), not (mapped distance, id): where the map collapses two
    # neighbours of distinct -dot, they stand in -dot order whatever their ids.
    lims, D, I = g.range_search(Q, INF, nprobe=5, reserve=N * NQ)
    collapsed = swapped = 0
    for i, (dot, M, Ir) in enumerate(per):
        mine = I[int(lims[i]):int(lims[i + 1])]
        assert np.array_equal(mine, Ir)
        assert np.all(dot[1:] >= dot[:-1])
        same = (bits(M[1:]) == bits(M[:-1])) & (dot[1:] != dot[:-1])
        collapsed += int(same.sum())
        swapped += int((same & (Ir[1:] < Ir[:-1])).sum())
    print(f"dim {dim}: {collapsed} neighbours of distinct -dot share a mapped distance, {swapped} in descending id order")


def test_equal_rows_order_by_id():
    """A row stored twice under two ids (the larger first): equal -dot, so id order."""
    dim = 20
    X, Q, ids, lists, C, XU, QU = data(dim)
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, NLIST, vdb.Metric.CosineDistance))
    g.centroids = C
    rows = np.stack([X[5], X[9], X[5] * np.float32(2)])  # (a scaled copy: the same direction)
    g.add_to_lists(rows, np.array([900, 17, 3], np.uint64), np.array([4, 4, 4], np.uint32))
    lims, D, I = g.range_search(X[5:6], INF, nprobe=NLIST)
    U = unit_rows_ref(rows)
    if np.array_equal(bits(U[0]), bits(U[2])):  # (x / norm of 2x: exact scaling, equal bits)
        at = {int(v): j for j, v in enumerate(I.tolist())}
        assert at[3] + 1 == at[900] and bits(D[at[3]:at[3] + 1])[0] == bits(D[at[900]:at[900] + 1])[0]
    assert sorted(I.tolist()) == [3, 17, 900]


# ---- 7. remove_ids, then search parity again ----
def test_remove_ids():
    dim = 20
    X, Q, ids, lists, C, XU, QU = data(dim)
    g = make(dim)
    g.search(Q, nprobe=5, k=10)
    gone_ids = ids[np.arange(200) * 7]
    gone = np.isin(ids, gone_ids)
    assert g.remove_ids(gone_ids) == int(gone.sum())
    o = ip_oracle(dim, ~gone)
    for nprobe, k in SEARCHES:
        assert_same(g.search(Q, nprobe=nprobe, k=k), expected(o, QU, nprobe, k))
    for l in range(NLIST):
        sel = np.flatnonzero((lists == l) & ~gone)
        assert np.array_equal(bits(g.get_list(l)[0]), bits(XU[sel]))


# ---- 8. the list-cache tier with a host home ----
def test_tier_host_home():
    dim = 128
    X, Q, ids, lists, C, XU, QU = data(dim)
    g = make(dim)
    t = make(dim, max_gpu_memory=N * (dim * 4 + 8) * 3 // 4)  # the add exceeds it: the tier
    assert t.cache_stats()["capacity_bytes"] > 0 and g.cache_stats()["capacity_bytes"] == 0
    for nprobe, k in ((5, 10), (12, 64), (1, 100)):  # (k = 100: the list cache; one list fits it)
        assert_same(t.search(Q, nprobe=nprobe, k=k), g.search(Q, nprobe=nprobe, k=k))
    st = t.cache_stats()
    assert st["screen_resident"] == 1 and st["screen_batches"] > 0, st
    for l in (HUB, 4):
        assert np.array_equal(bits(t.get_list(l)[0]), bits(g.get_list(l)[0]))


# ---- 9. a group of two members on the one device ----
def test_group():
    n, dim, nlist = 2000, 32, 8
    X, Q, ids = oracle.reference_test_data(n, 30, dim, seed=78)
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, nlist, vdb.Metric.CosineDistance))
    grp = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, nlist, vdb.Metric.CosineDistance, devices=(0, 0)))
    assert grp.group_size == 2
    for h in (g, grp):
        h.train(X)
        h.add(X[:1200], ids[:1200])
        h.add(X[1200:], ids[1200:])
    assert np.array_equal(bits(grp.centroids), bits(g.centroids))
    assert grp.list_sizes().tolist() == g.list_sizes().tolist()
    assert len(set(grp.list_owners().tolist())) == 2
    for l in range(nlist):  # (a member normalising again would change bits)
        (Va, Ia), (Vb, Ib) = grp.get_list(l), g.get_list(l)
        assert np.array_equal(Ia, Ib) and np.array_equal(bits(Va), bits(Vb)), f"list {l}"
    for nprobe, k in ((1, 10), (4, 10), (8, 64), (8, 100)):
        assert_same(grp.search(Q, nprobe=nprobe, k=k), g.search(Q, nprobe=nprobe, k=k))


# ---- 10. device buffers in and out ----
@pytest.mark.parametrize("dim", [20, 128])
def test_search_device(dim):
    import torch
    X, Q, ids, lists, C, XU, QU = data(dim)
    g = make(dim)
    dev = torch.device("cuda:0")
    qd = torch.from_numpy(Q.copy()).to(dev)
    od = torch.empty((NQ, 10), dtype=torch.float32, device=dev)
    oi = torch.empty((NQ, 10), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    g.search_device(qd.data_ptr(), NQ, 5, 10, od.data_ptr(), oi.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert_same((od.cpu().numpy(), oi.cpu().numpy().view(np.uint64)), expected(ip_oracle(dim), QU, 5, 10))
    assert np.array_equal(bits(qd.cpu().numpy()), bits(Q))  # the caller's queries are only read


# ---- 11. refusals ----
def test_refusals(tmp_path):
    dim = 20
    X, Q, ids, lists, C, XU, QU = data(dim)
    g = make(dim)
    before = g.search(Q, nprobe=5, k=10)

    def refused(call, match="COSINE_DISTANCE"):
        with pytest.raises(vdb.VdbError, match=match) as e:
            call()
        assert e.value.code == UNSUPPORTED
        assert g.list_sizes().tolist() == LENS
        assert_same(g.search(Q, nprobe=5, k=10), before)

    owners = np.arange(NLIST, dtype=np.uint32) % 2
    refused(lambda: g.set_shard(0, 2))
    refused(lambda: g.set_shard(0, 2, owners))
    e = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, NLIST, vdb.Metric.CosineDistance))
    with pytest.raises(vdb.VdbError, match="COSINE_DISTANCE") as x:
        e.plan_shard(0, 2, np.array(LENS, np.uint64))
    assert x.value.code == UNSUPPORTED
    with pytest.raises(vdb.VdbError, match="COSINE_DISTANCE") as x:
        e.plan_shard(0, 2, np.array(LENS, np.uint64), owners)
    assert x.value.code == UNSUPPORTED
    refused(lambda: g.attach_comm(bytes(vdb.COMM_ID_BYTES), 0, 1))
    # files: metric 3 and the others do not mix, either way
    cos_path, ip_path, shard_path = (str(tmp_path / n) for n in ("cos.ivf", "ip.ivf", "shard.ivf"))
    g.save(cos_path)
    p = make(dim, IP)
    p.save(ip_path)
    for metric, path in ((IP, cos_path), (0, cos_path), (2, cos_path), (COS, ip_path)):
        h = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, NLIST, vdb.Metric(metric)))
        with pytest.raises(vdb.VdbError, match="does not match") as x:
            h.load(path)
        assert x.value.code == INVALID and h.get_total_vectors() == 0
    # a plain metric-3 file serves a metric-3 tier; a shard file does not
    t = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, NLIST, vdb.Metric.CosineDistance, max_gpu_memory=0))
    t.set_option("list_cache_bytes", 60 * 64 * (64 * 4 + 8))
    p.set_shard(0, 2)
    p.save(shard_path)
    with pytest.raises(vdb.VdbError, match="shard file") as x:
        t.open_lists(shard_path)
    assert x.value.code == UNSUPPORTED
    t.open_lists(cos_path)
    assert_same(t.search(Q, nprobe=5, k=10), before)


# ---- 12. ordinal 2 keeps the reference CPU path's 0.0f ----
def test_cosine_2_unchanged():
    dim = 20
    X, Q, ids, lists, C, XU, QU = data(dim)
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, NLIST, vdb.Metric.Cosine))
    g.centroids = C
    g.add_to_lists(X, ids, lists)
    D, I = g.search(Q, nprobe=5, k=10)
    assert np.all(bits(D[I != NONE]) == 0) and np.any(I != NONE)
    assert np.array_equal(bits(g.get_list(HUB)[0]), bits(X[lists == HUB]))  # (rows stored as given)
