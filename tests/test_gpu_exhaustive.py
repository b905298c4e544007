"""GPU: vdb_ivf_search_exhaustive (the exact top-k over every stored row) against plain numpy.

Definition under test: per query the entries (d, id) of every stored row, each id once at its
smallest (d, id), ascending by (d, id), the first k, unfilled slots (FLT_MAX, UINT64_MAX). The
expected answer is oracle.np_ref.distances over all stored rows, np.lexsort((ids, d)), repeated
ids dropped keeping the first. Ids and distance bits must be equal.

Base shape: test_gpu_filter's (12 lists of 0 .. 1,500 rows, ten ids stored in two lists, three
list layouts), 33 queries: one past a full tile of 32.
"""
import numpy as np
import pytest

from conftest import load_vdb
from cosine_ref import cos_map, unit_rows_ref
from oracle import np_ref
from test_gpu_filter import FMAX, LENS, NLIST, NONE, assert_same, data, make

vdb = load_vdb()
pytestmark = pytest.mark.gpu

NQ = 33
KS = (1, 10, 64, 65, 128, 129, 1024)  # every tile width, both sides of each register boundary
UNSUPPORTED, INVALID = -4, -1
_dist = {}


def ref(metric, Q, X, ids, k, key=None):
    """The definition in numpy. key: cache the distances (the base shape's, shared by its cases)."""
    d = _dist.get(key)
    if key is None or d is None:
        d = (np_ref.distances(1, unit_rows_ref(Q), unit_rows_ref(X)) if metric == 3 else np_ref.distances(metric, Q, X))
        if key is not None:
            _dist[key] = d
    D = np.full((Q.shape[0], k), FMAX, np.float32)
    I = np.full((Q.shape[0], k), NONE, np.uint64)
    for i in range(Q.shape[0]):
        o = np.lexsort((ids, d[i]))
        o = o[np.sort(np.unique(ids[o], return_index=True)[1])][:k]
        D[i, :o.size], I[i, :o.size] = d[i][o], ids[o]
    return (cos_map(D, I) if metric == 3 else D), I


@pytest.mark.parametrize("layout", ["il", "rows", "stale"])
@pytest.mark.parametrize("metric", [0, 1, 3])
@pytest.mark.parametrize("dim", [20, 128])
def test_base_shape(dim, metric, layout):
    X, Q, ids, lists, C = data(dim)
    Q = Q[:NQ]
    g = make(dim, metric, layout)
    for k in KS:
        assert_same(*g.search_exhaustive(Q, k), *ref(metric, Q, X, ids, k, key=(dim, metric)))
    t = g.exhaustive_last_timing()
    assert t["rows_scanned"] == sum(LENS) * 17 and t["pairs_computed"] == sum(LENS) * NQ and t["scan_ms"] > 0
    # no list stores an id twice: with stale_slots off, nprobe = nlist is the same answer
    g.set_stale_slots(False)
    for k in (10, 129):
        assert_same(*g.search_exhaustive(Q, k), *g.search(Q, nprobe=NLIST, k=k))


def test_cosine_gives_the_smallest_ids():
    X, Q, ids, lists, C = data(20)
    g = make(20, 2, "il")
    D, I = g.search_exhaustive(Q[:NQ], 10)
    assert_same(D, I, *ref(2, Q[:NQ], X, ids, 10))
    assert np.array_equal(I[0], np.unique(ids)[:10]) and not D.any()


def small(dim, nlist, X, ids, lists, metric=0):
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, nlist, vdb.Metric(metric)))
    g.centroids = np.random.RandomState(1).randn(nlist, dim).astype(np.float32)
    g.set_option("screen", 0)
    if len(ids):
        g.add_to_lists(X, ids, lists)
    return g


def test_k_above_the_row_count_and_an_empty_index():
    r = np.random.RandomState(5)
    X, Q = r.randn(5, 20).astype(np.float32), r.randn(3, 20).astype(np.float32)
    ids = np.arange(5, dtype=np.uint64) + 40
    g = small(20, 3, X, ids, np.array([2, 0, 2, 2, 0], np.uint32))
    D, I = g.search_exhaustive(Q, 10)
    assert_same(D, I, *ref(0, Q, X, ids, 10))
    assert (I[:, 5:] == NONE).all() and (D[:, 5:] == FMAX).all()
    D, I = small(20, 3, X[:0], ids[:0], ids[:0]).search_exhaustive(Q, 4)
    assert (I == NONE).all() and (D == FMAX).all()


@pytest.mark.parametrize("k", [2, 10])
@pytest.mark.parametrize("where", ["block", "blocks", "lists"])
def test_an_id_stored_twice(where, k):
    """20 rows B stand twice, with their ids: in one 64-row block, in two blocks of one list, in
    two lists. The queries sit on rows of B, so a multiset top-k holds a row of B twice and a
    row that belongs in the answer is crowded out of it."""
    r = np.random.RandomState(11)
    B, O = r.randn(20, 20).astype(np.float32), r.randn(180, 20).astype(np.float32)
    ib, io = np.arange(20, dtype=np.uint64) + 1000, np.arange(180, dtype=np.uint64)
    l0 = {"block": [B, B, O[:90]], "blocks": [B, O[:60], B, O[60:90]], "lists": [B, O[:90]]}[where]
    i0 = {"block": [ib, ib, io[:90]], "blocks": [ib, io[:60], ib, io[60:90]], "lists": [ib, io[:90]]}[where]
    l1, i1 = ([B, O[90:]], [ib, io[90:]]) if where == "lists" else ([O[90:]], [io[90:]])
    X, ids = np.concatenate(l0 + l1), np.concatenate(i0 + i1)
    lists = np.repeat(np.array([0, 1], np.uint32), [sum(map(len, i0)), sum(map(len, i1))])
    Q = B[:8] + np.float32(0.01) * r.randn(8, 20).astype(np.float32)
    Dr, Ir = ref(0, Q, X, ids, k)
    # here on the CPU: the multiset top-k repeats an id, so it misses the unique answer's last row
    for i, d in enumerate(np_ref.distances(0, Q, X)):
        multi = ids[np.lexsort((ids, d))[:k]]
        assert len(set(multi.tolist())) < k and Ir[i, k - 1] not in multi
    assert_same(*small(20, 2, X, ids, lists).search_exhaustive(Q, k), Dr, Ir)


@pytest.mark.parametrize("nlist,rows,nq", [(1500, 3000, NQ), (4, 200_000, 5)])
def test_above_the_nprobe_cap_and_more_chunks_than_waves(nlist, rows, nq):
    """nlist 1500: no nprobe reaches every list. 200,000 rows: 3,125 blocks and more against 1,024
    waves, so every wave folds several chunks."""
    r = np.random.RandomState(rows)
    X, Q = r.randn(rows, 20).astype(np.float32), r.randn(nq, 20).astype(np.float32)
    ids = r.permutation(rows).astype(np.uint64)
    g = small(20, nlist, X, ids, r.randint(0, nlist, rows).astype(np.uint32))
    for k in (10, 65):
        assert_same(*g.search_exhaustive(Q, k), *ref(0, Q, X, ids, k, key=rows))


def refused(g, Q, code, match, k=10):
    D0, I0 = g.search(Q, nprobe=5, k=10)
    with pytest.raises(vdb.VdbError, match=match) as e:
        g.search_exhaustive(Q, k)
    assert e.value.code == code
    assert_same(*g.search(Q, nprobe=5, k=10), D0, I0)


def test_refusals():
    X, Q, ids, lists, C = data(20)
    g = make(20, 0, "rows")
    refused(g, Q, UNSUPPORTED, "1024", k=1025)
    refused(g, Q, INVALID, "k is", k=0)
    t = make(20, 0, "il", max_gpu_memory=0)
    t.set_option("list_cache_bytes", 60 * 64 * (128 * 4 + 8))
    refused(t, Q, UNSUPPORTED, "list-cache tier")
    refused(make(20, 0, "rows", devices=(0, 0)), Q, UNSUPPORTED, "group")
    s = make(20, 0, "rows")
    s.set_shard(0, 2)
    refused(s, Q, UNSUPPORTED, "sharded")
