"""GPU: vdb_ivf_search_prepared_screened (a prepared filter's top-k served through the screen: per
pair the k-th smallest upper bound, the rows whose lower bound does not exceed it, their exact
top-k) against vdb_ivf_search_prepared on the same handle, the CPU oracle holding only the
allowed rows, and the numpy restatement of the screen's bounds (screen_ref.py).

The fixture and the handles are test_gpu_range_screen.py's (screen_ref.contract_fixture, seed 1, 40
queries; nprobe 5 = nlist: items of 16, 16 and 8 pairs; the hub in two segments).

test_it_prunes' cap, restated on the CPU for every case before it was fixed (every-second-id
filter, k 10, 42,360 allowed pairs, so 5,295 = pairs // 8). Kept at dim 64 / 200: L2 1,624 / 2,150
(int8) and 1,286 / 1,424 (bf16, upper edge of the band); InnerProduct 1,638 / 2,234 and 1,307 /
1,430; CosineDistance 1,804 / 2,702 and 1,322 / 1,479. No case was dropped."""
import functools

import numpy as np
import pytest

import oracle
import screen_ref as sr
from conftest import load_vdb
from test_gpu_range_screen import NPROBE, NQ, PARENT_BUILD_ID, bits, centroids_of, fixture, handle, make, unit

vdb = load_vdb()
pytestmark = pytest.mark.gpu

NONE = np.iinfo(np.uint64).max
NOIDS = np.zeros(0, np.uint64)


def list_ids(fx, l):
    return fx["ids"][fx["assign"] == l]


def filter_sets(fx):
    """name -> (ids, include). sparse: 22 rows of the hub's block 0 and 30 of its block 10 (every
    other block of the hub masked out), 3 rows of the 64-row list, the 1-row list's row."""
    hub = list_ids(fx, 0)
    sparse = np.concatenate([hub[0:64:3], hub[640:700:2], list_ids(fx, 1)[:3], list_ids(fx, 3)])
    return {"all": (NOIDS, False), "half": (np.sort(fx["ids"])[::2], False), "sparse": (sparse, True),
            "none": (NOIDS, True)}


def both(g, Q, flt, k, **kw):
    ex = g.search_prepared(Q, flt, nprobe=NPROBE, k=k)
    sc = g.search_prepared(Q, flt, nprobe=NPROBE, k=k, screen=True, **kw)
    return ex, sc, g.filter_screen_last_timing()


def assert_same(sc, ex):
    assert sc[1].dtype == np.uint64 and sc[0].dtype == np.float32
    bad = np.argwhere(sc[1] != ex[1])
    assert bad.size == 0, f"ids differ at {bad[:3].tolist()}"
    badd = np.argwhere(bits(sc[0]) != bits(ex[0]))
    assert badd.size == 0, f"distance bits differ at {badd[:3].tolist()}"


def check_parity(dim, metric, i8, kind, k):
    fx = fixture(dim, kind)
    g = handle(dim, metric, i8, kind)
    for name, (ids, include) in filter_sets(fx).items():
        flt = g.prepare_filter(ids, include=include)
        # ties: 200 equal rows share every bound, so at k 1 each of them is a candidate (5,808 in
        # all); special: the zero query's bounds are NaN under InnerProduct and keep its every row
        # (2,419). Both exceed the default capacity at k 1 (4 x 40 x 5 x 1): room for every pair
        # keeps the route under test
        ex, sc, st = both(g, fx["Q"], flt, k, reserve=0 if kind == "plain" else 1 << 17)
        assert_same(sc, ex)
        assert st["screened_batches"] == 1 and st["exact_batches"] == 0, (name, st)
        assert st["pairs_bounded"] == NQ * flt.allowed, (name, st)
        assert st["candidates"] <= st["pairs_bounded"]
        if name == "none":
            assert (sc[1] == NONE).all() and (sc[0] == np.finfo(np.float32).max).all()
        if kind == "plain" and metric != 3:
            allow = np.isin(fx["ids"], ids) == include
            o = oracle.OracleIndex(dim, 5, metric)
            o.centroids = fx["C"]
            for l in range(5):
                m = (fx["assign"] == l) & allow
                o.set_list(l, fx["X"][m], fx["ids"][m])
            assert_same(sc, o.search(fx["Q"], NPROBE, k))


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("kind", ["plain", "special", "ties"])
@pytest.mark.parametrize("dim", [64, 200])
@pytest.mark.parametrize("i8", [1, 0])
@pytest.mark.parametrize("metric", [0, 1, 3])
def test_parity(metric, i8, dim, kind, k):
    check_parity(dim, metric, i8, kind, k)


def test_parity_at_768():
    check_parity(768, 0, 1, "plain", 10)


@pytest.mark.parametrize("stale", [0, 1])
@pytest.mark.parametrize("i8", [1, 0])
def test_stale_slots_and_batches(i8, stale):
    """Batches of 8 of 40 queries under the sparse filter (the empty list and, for the carry, a
    slot without an allowed row in every batch): the carry crosses the batches."""
    fx = fixture(200)
    g = make(fx, 0, i8)
    g.set_stale_slots(bool(stale))
    name_ids = filter_sets(fx)
    for name in ("sparse", "half"):
        flt = g.prepare_filter(name_ids[name][0], include=name_ids[name][1])
        g.set_batch(64)
        whole = g.search_prepared(fx["Q"], flt, nprobe=NPROBE, k=10)
        g.set_batch(8)
        ex, sc, st = both(g, fx["Q"], flt, 10)
        assert_same(ex, whole)
        assert_same(sc, whole)
        assert st["screened_batches"] == 5 and st["exact_batches"] == 0


@functools.lru_cache(maxsize=None)
def bounds(dim, metric, i8):
    """Per non-empty list of the plain fixture the restated (lb, ub, tol), each [NQ][rows]
    (screen_ref: the build, the pairs and the bound; int8: the kernel's bits, tol 0)."""
    fx = fixture(dim)
    dp = (dim + 63) // 64 * 64
    to = unit if metric == 3 else (lambda a: a)
    m = 1 if metric == 3 else metric
    Cp, Qp = sr.pad_dp(centroids_of(fx, metric), dp), sr.pad_dp(to(fx["Q"]), dp)
    out = {}
    for l in range(5):
        if not len(fx["lists"][l]):
            continue
        sh, sc, meta = sr.build_restated(sr.pad_dp(to(fx["lists"][l]), dp), Cp[l], bool(i8))
        per = [sr.pair_bounds(*sr.pairs_restated(Qp[q], Cp[l], m, bool(i8)), sh, sc, meta, dp, m, bool(i8))
               for q in range(NQ)]
        out[l] = tuple(np.array([np.asarray(p[j], np.float64) for p in per]) for j in (0, 1, 3))
    return out


def restated_kept(dim, metric, i8, ids, include, k):
    """(low, high) of the candidates: per pair tau = the k-th smallest ub over the allowed rows
    (a NaN never counts, +inf below k), kept = allowed and not lb > tau. The device's bounds lie
    within tol of the restated ones and the k-th smallest is monotone in every entry, so the count
    lies between the one with every bound moved against a row and the one with every bound moved
    for it. tol 0 (int8): low == high, the kernel's count."""
    fx = fixture(dim)
    lo = hi = 0
    for l, (lb, ub, tol) in bounds(dim, metric, i8).items():
        a = np.isin(list_ids(fx, l), ids) == include
        if not a.any():
            continue
        for s, sign in ((0, -1.0), (1, 1.0)):
            with np.errstate(invalid="ignore"):
                u = ub[:, a] + sign * tol[:, a]
                u = np.where(np.isnan(u), np.inf, u)
                tau = np.partition(u, k - 1, axis=1)[:, k - 1] if a.sum() >= k else np.full(NQ, np.inf)
                n = int((~(lb[:, a] - sign * tol[:, a] > tau[:, None])).sum())
            lo, hi = (lo + n, hi) if s == 0 else (lo, hi + n)
    return lo, hi


@pytest.mark.parametrize("name", ["half", "sparse"])
@pytest.mark.parametrize("dim", [64, 200])
@pytest.mark.parametrize("i8", [1, 0])
@pytest.mark.parametrize("metric", [0, 1])
def test_candidates_are_the_restated_bound(metric, i8, dim, name):
    fx = fixture(dim)
    g = handle(dim, metric, i8)
    ids, include = filter_sets(fx)[name]
    flt = g.prepare_filter(ids, include=include)
    for k in (1, 10):
        _, _, st = both(g, fx["Q"], flt, k)
        lo, hi = restated_kept(dim, metric, i8, ids, include, k)
        print("metric %d i8 %d dim %d %s k %d: %d candidates, restated [%d, %d]" %
              (metric, i8, dim, name, k, st["candidates"], lo, hi))
        if i8:
            assert lo == hi == st["candidates"]
        else:
            assert lo <= st["candidates"] <= hi


@pytest.mark.parametrize("dim", [64, 200])
@pytest.mark.parametrize("i8", [1, 0])
@pytest.mark.parametrize("metric", [0, 1, 3])
def test_it_prunes(metric, i8, dim):
    """Every second id excluded, k 10: at most a quarter of the allowed pairs reach the select
    kernel. The restated bound keeps at most an eighth in every case (module docstring)."""
    fx = fixture(dim)
    g = handle(dim, metric, i8)
    ids, include = filter_sets(fx)["half"]
    flt = g.prepare_filter(ids, include=include)
    ex, sc, st = both(g, fx["Q"], flt, 10)
    assert_same(sc, ex)
    print("metric %d i8 %d dim %d: %d candidates of %d pairs" % (metric, i8, dim, st["candidates"], st["pairs_bounded"]))
    assert st["pairs_bounded"] == NQ * flt.allowed
    assert NQ * 3 * 10 <= st["candidates"] <= st["pairs_bounded"] // 4
    assert restated_kept(dim, metric, i8, ids, include, 10)[1] <= st["pairs_bounded"] // 8


@pytest.mark.parametrize("i8", [1, 0])
def test_fallback(i8):
    fx = fixture(64, "special")
    g = handle(64, 1, i8, "special")
    flt = g.prepare_filter(*filter_sets(fx)["half"][:1], include=False)
    ex, sc, st = both(g, fx["Q"], flt, 10, reserve=1)
    assert_same(sc, ex)
    assert st["exact_batches"] == 1 and st["screened_batches"] == 0 and st["candidates"] > 1


@pytest.mark.parametrize("why", ["cosine", "fresh", "screen_off", "after_add"])
def test_without_a_live_screen_the_exact_path_serves(why):
    fx = fixture(64)
    if why == "cosine":
        g = make(fx, 2, 1, live=False)
        g.search(fx["Q"], nprobe=NPROBE, k=10)
    elif why == "fresh":
        g = make(fx, 0, 1, live=False)
    elif why == "screen_off":
        g = make(fx, 0, 1, live=False, screen=0)
        g.search(fx["Q"], nprobe=NPROBE, k=10)
    else:
        g = make(fx, 0, 1)
        g.add_to_lists(fx["X"][:3] + np.float32(0.25), np.array([7, 8, 9], np.uint64), np.array([1, 2, 3], np.uint32))
    flt = g.prepare_filter(*filter_sets(fx)["half"][:1], include=False)
    shadow, before = g.profile_read()["screen_shadow"], g.gpu_bytes_allocated()
    ex, sc, st = both(g, fx["Q"], flt, 10)
    assert_same(sc, ex)
    assert st["screened_batches"] == 0 and st["exact_batches"] == 1 and st["pairs_bounded"] == 0, st
    assert g.gpu_bytes_allocated() == before and g.profile_read()["screen_shadow"] == shadow


def test_handle_is_left_as_found():
    fx = fixture(64)
    g = make(fx, 0, 1)
    flt = g.prepare_filter(*filter_sets(fx)["half"][:1], include=False)
    D0, I0 = g.search(fx["Q"], nprobe=NPROBE, k=10)
    before = g.gpu_bytes_allocated()
    ex, sc, st = both(g, fx["Q"], flt, 10)
    assert_same(sc, ex)
    assert st["screened_batches"] == 1
    assert g.gpu_bytes_allocated() == before and not flt.stale
    D1, I1 = g.search(fx["Q"], nprobe=NPROBE, k=10)
    assert D0.tobytes() == D1.tobytes() and I0.tobytes() == I1.tobytes()
    ft = g.filter_last_timing()
    assert ft["mark_ms"] == 0 and ft["pairs_scanned"] == NQ * flt.allowed
    assert vdb.build_id() == PARENT_BUILD_ID


def test_refusals():
    fx = fixture(64)
    g, other = make(fx, 0, 1), make(fx, 0, 1)
    flt = g.prepare_filter(fx["ids"][:50], include=True)
    L, q = vdb.lib(), np.ascontiguousarray(fx["Q"])
    D, I = np.full((NQ, 65), 7, np.float32), np.full((NQ, 65), 7, np.uint64)

    def call(h, f, k, d=D):
        rc = L.vdb_ivf_search_prepared_screened(h._h, f._f if f else None, q.ctypes.data, NQ, NPROBE, k, 0,
                                                d.ctypes.data if d is not None else None, I.ctypes.data)
        assert (D == 7).all() and (I == 7).all()  # the outputs are not written
        return rc

    assert call(other, flt, 10) == -1  # VDB_ERR_INVALID_ARGUMENT: another handle's filter
    assert call(g, None, 10) == -1 and call(g, flt, 10, None) == -1
    assert call(g, flt, 65) == -4  # VDB_ERR_UNSUPPORTED
    with pytest.raises(vdb.VdbError) as e:
        g.search_prepared(fx["Q"], flt, nprobe=NPROBE, k=65)
    assert e.value.code == -4  # (the prepared call's own code for the same request)
    g.add(fx["X"][:2] + np.float32(0.5), np.array([5, 6], np.uint64))
    assert flt.stale and call(g, flt, 10) == -5  # VDB_ERR_STATE
