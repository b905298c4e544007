"""GPU: vdb_ivf_search_exhaustive_screened (the exact unique-id top-k over every stored row, read
through the screen's shadow) against the exact call on the same handle and the numpy definition.
Every comparison is ids equal and distance bits equal.

Fixture: test_gpu_range_screen's (screen_ref.contract_fixture, 2,119 rows: a hub of 31 blocks + 5
rows, lists of 64, 65, 1 and 0 rows; 40 queries, so a full tile of 32 and a tile of 8 with one A
operand). One search first makes the screen live.

test_it_prunes' cap, restated on the CPU before it was fixed (screen_ref: pairs_restated,
build_restated, pair_bounds; T_q the 10th smallest ub over the fixture's distinct ids; the count of
lb <= T_q; of 84,760 pairs, cap 10,595; bf16 as [low, high] with every bound moved by its tolerance):
    metric  dim   int8              bf16
    0       64    682               465
    0       200   1,084             [511, 512]
    1       64    661               460
    1       200   1,010             490
    3       64    890               514
    3       200   1,733             [581, 582]
"""
import functools

import numpy as np
import pytest

import screen_ref as sr
from conftest import load_vdb
from oracle import np_ref
from test_gpu_exhaustive import ref
from test_gpu_range_screen import bits, centroids_of, fixture, handle, make, unit

vdb = load_vdb()
pytestmark = pytest.mark.gpu

NQ, ROWS = 40, 2119


def same(got, want):
    assert got[0].dtype == np.float32 and got[1].dtype == np.uint64
    bad = np.argwhere(got[1] != want[1])
    assert bad.size == 0, f"ids differ at {bad[:3].tolist()}"
    badd = np.argwhere(bits(got[0]) != bits(want[0]))
    assert badd.size == 0, f"distance bits differ at {badd[:3].tolist()}"


def both(g, Q, k, **kw):
    ex = g.search_exhaustive(Q, k)
    sc = g.search_exhaustive(Q, k, screen=True, **kw)
    return ex, sc, g.exhaustive_screen_last_timing()


def check_parity(dim, metric, i8, kind, k):
    fx = fixture(dim, kind)
    g = handle(dim, metric, i8, kind)
    # ties: 200 equal rows share every bound; special: the zero query's bounds are NaN under
    # InnerProduct and keep its every row: a region of every row keeps the route under test
    rows = len(fx["X"])  # (2,119; `special` adds a few rows of its own)
    ex, sc, st = both(g, fx["Q"], k, reserve=0 if kind == "plain" else rows)
    same(sc, ex)
    assert st["screened_tiles"] == 2 and st["exact_tiles"] == 0, st
    assert st["rows_bounded"] == NQ * rows and st["candidates"] <= st["rows_bounded"], st
    if kind == "plain":
        same(sc, ref(metric, fx["Q"], fx["X"], fx["ids"], k, key=("exs", dim, metric)))


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("kind", ["plain", "special", "ties"])
@pytest.mark.parametrize("dim", [64, 200])
@pytest.mark.parametrize("i8", [1, 0])
@pytest.mark.parametrize("metric", [0, 1, 3])
def test_parity(metric, i8, dim, kind, k):
    check_parity(dim, metric, i8, kind, k)


def test_parity_at_768():
    check_parity(768, 0, 1, "plain", 10)


def live_small(dim, nlist, X, ids, lists, i8, Q):
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, nlist, vdb.Metric(0)))
    g.centroids = np.random.RandomState(1).randn(nlist, dim).astype(np.float32)
    g.set_option("screen_i8", i8)
    g.set_option("screen_floor_ppm", 0)
    g.add_to_lists(X, ids, lists)
    g.search(Q, nprobe=min(nlist, 4), k=10)  # makes the screen live
    assert g.profile_read()["screen_shadow"] == (2 if i8 else 1)
    return g


@pytest.mark.parametrize("i8", [1, 0])
@pytest.mark.parametrize("k", [2, 10])
@pytest.mark.parametrize("where", ["block", "blocks", "lists"])
def test_an_id_stored_twice(where, k, i8):
    """test_gpu_exhaustive's three placements of 20 rows that stand twice with their ids, with a
    live screen: a multiset k-th upper bound would count a copy twice and discard a row of the
    answer."""
    r = np.random.RandomState(11)
    B, O = r.randn(20, 64).astype(np.float32), r.randn(180, 64).astype(np.float32)
    ib, io = np.arange(20, dtype=np.uint64) + 1000, np.arange(180, dtype=np.uint64)
    l0 = {"block": [B, B, O[:90]], "blocks": [B, O[:60], B, O[60:90]], "lists": [B, O[:90]]}[where]
    i0 = {"block": [ib, ib, io[:90]], "blocks": [ib, io[:60], ib, io[60:90]], "lists": [ib, io[:90]]}[where]
    l1, i1 = ([B, O[90:]], [ib, io[90:]]) if where == "lists" else ([O[90:]], [io[90:]])
    X, ids = np.concatenate(l0 + l1), np.concatenate(i0 + i1)
    lists = np.repeat(np.array([0, 1], np.uint32), [sum(map(len, i0)), sum(map(len, i1))])
    Q = B[:8] + np.float32(0.01) * r.randn(8, 64).astype(np.float32)
    Dr, Ir = ref(0, Q, X, ids, k)
    # here on the CPU: the multiset top-k repeats an id, so it misses the unique answer's last row
    for i, d in enumerate(np_ref.distances(0, Q, X)):
        multi = ids[np.lexsort((ids, d))[:k]]
        assert len(set(multi.tolist())) < k and Ir[i, k - 1] not in multi
    g = live_small(64, 2, X, ids, lists, i8, Q)
    ex, sc, st = both(g, Q, k)
    same(sc, (Dr, Ir))
    assert st["screened_tiles"] == 1 and st["exact_tiles"] == 0


@functools.lru_cache(maxsize=None)
def restated_kept(dim, metric, i8, k=10):
    """(low, high) of the candidates of the plain fixture: T_q the k-th smallest ub over every row
    (its ids are distinct; a NaN never counts), kept = not lb > T_q, with every bound moved by its
    tolerance against and for a row (int8: tol 0, low == high)."""
    fx = fixture(dim)
    dp = (dim + 63) // 64 * 64
    to = unit if metric == 3 else (lambda a: a)
    m = 1 if metric == 3 else metric
    Cp, Qp = sr.pad_dp(centroids_of(fx, metric), dp), sr.pad_dp(to(fx["Q"]), dp)
    lb, ub, tol = [], [], []
    for l in range(5):
        if not len(fx["lists"][l]):
            continue
        sh, sc, meta = sr.build_restated(sr.pad_dp(to(fx["lists"][l]), dp), Cp[l], bool(i8))
        per = [sr.pair_bounds(*sr.pairs_restated(Qp[q], Cp[l], m, bool(i8)), sh, sc, meta, dp, m, bool(i8))
               for q in range(NQ)]
        for dst, j in ((lb, 0), (ub, 1), (tol, 3)):
            dst.append(np.array([np.asarray(p[j], np.float64) for p in per]))
    lb, ub, tol = (np.concatenate(a, axis=1) for a in (lb, ub, tol))
    out = []
    for sign in (-1.0, 1.0):
        with np.errstate(invalid="ignore"):
            u = ub + sign * tol
            T = np.partition(np.where(np.isnan(u), np.inf, u), k - 1, axis=1)[:, k - 1]
            out.append(int((~(lb - sign * tol > T[:, None])).sum()))
    return tuple(out)


@pytest.mark.parametrize("dim", [64, 200])
@pytest.mark.parametrize("i8", [1, 0])
@pytest.mark.parametrize("metric", [0, 1, 3])
def test_it_prunes(metric, i8, dim):
    """k 10 on the plain fixture: at most an eighth of the (query, row) pairs reach the select
    kernel; the restated bound alone stays within the cap (module docstring)."""
    fx = fixture(dim)
    g = handle(dim, metric, i8)
    assert len(np.unique(fx["ids"])) == ROWS
    ex, sc, st = both(g, fx["Q"], 10)
    same(sc, ex)
    lo, hi = restated_kept(dim, metric, i8)
    print("metric %d i8 %d dim %d: %d candidates of %d, restated [%d, %d]" %
          (metric, i8, dim, st["candidates"], st["rows_bounded"], lo, hi))
    assert hi <= (NQ * ROWS) // 8
    assert NQ * 10 <= st["candidates"] <= (NQ * ROWS) // 8
    assert lo <= st["candidates"] <= hi


@pytest.mark.parametrize("why", ["fresh", "k65", "reserve1", "after_add"])
def test_fallbacks_give_the_same_answer_and_say_so(why):
    fx = fixture(64)
    k, kw = (65, {}) if why == "k65" else (10, {"reserve": 1} if why == "reserve1" else {})
    g = make(fx, 0, 1, live=why != "fresh")
    if why == "after_add":  # the screen goes stale
        g.add_to_lists(fx["X"][:3] + np.float32(0.25), np.array([7, 8, 9], np.uint64), np.array([1, 2, 3], np.uint32))
    ex, sc, st = both(g, fx["Q"], k, **kw)
    same(sc, ex)
    # k 65: the exact call's tiles are 16 wide; reserve 1: both tiles overflow, and only they count
    assert st["screened_tiles"] == 0 and st["exact_tiles"] == (3 if why == "k65" else 2), st
    assert (st["candidates"] > NQ) == (why == "reserve1")


@pytest.mark.parametrize("i8", [1, 0])
@pytest.mark.parametrize("nlist,rows,nq", [(4, 200_000, 5), (1500, 3000, 33)])
def test_chunks_and_list_switches(nlist, rows, nq, i8):
    """200,000 rows in 4 lists: 3,125 blocks and more against 1,024 waves, so every wave folds
    several chunks. 3,000 rows in 1,500 lists: a list change at almost every block, empty lists."""
    r = np.random.RandomState(rows)
    X, Q = r.randn(rows, 64).astype(np.float32), r.randn(nq, 64).astype(np.float32)
    ids = r.permutation(rows).astype(np.uint64)
    g = live_small(64, nlist, X, ids, r.randint(0, nlist, rows).astype(np.uint32), i8, Q)
    same(g.search_exhaustive(Q, 10, screen=True), ref(0, Q, X, ids, 10))
    st = g.exhaustive_screen_last_timing()
    assert st["exact_tiles"] == 0 and st["rows_bounded"] == nq * rows


def test_refusals_equal_the_exact_call_s():
    fx = fixture(64)
    Q = fx["Q"]

    def refused(g, code, match, k=10):
        D0, I0 = g.search(Q, nprobe=5, k=10)
        for screen in (False, True):
            with pytest.raises(vdb.VdbError, match=match) as e:
                g.search_exhaustive(Q, k, screen=screen)
            assert e.value.code == code
        same(g.search(Q, nprobe=5, k=10), (D0, I0))

    g = make(fx, 0, 1)
    refused(g, -4, "1024", k=1025)
    refused(g, -1, "k is", k=0)
    t = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(64, 5, vdb.Metric(0), max_gpu_memory=0))
    t.centroids = fx["C"]
    t.set_option("screen", 0)
    t.add_to_lists(fx["X"], fx["ids"], fx["assign"].astype(np.uint32))
    t.set_option("list_cache_bytes", 60 * 64 * (64 * 4 + 8))
    refused(t, -4, "list-cache tier")
    grp = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(64, 5, vdb.Metric(0), devices=(0, 0)))
    grp.centroids = fx["C"]
    grp.add_to_lists(fx["X"], fx["ids"], fx["assign"].astype(np.uint32))
    refused(grp, -4, "group")
    s = make(fx, 0, 1, live=False)
    s.set_shard(0, 2)
    refused(s, -4, "sharded")
