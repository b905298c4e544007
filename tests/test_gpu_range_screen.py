"""GPU: vdb_ivf_range_search_screened (range search served through the screen: lower bounds on
the matrix cores, exact re-checks of the rest) against the exact range call on the same handle,
the CPU oracle and the numpy restatement of the screen's bound (screen_ref.py).

Fixture (screen_ref.contract_fixture, seed 1, 40 queries): five lists with explicit centroids, a
hub of 31 full blocks + 5 rows (two segments), lists of 64, 65, 1 and 0 rows; 2,119 rows. nprobe 5
= nlist, so every list is probed by all 40 queries: items of 16, 16 and 8 pairs. One search first
makes the screen live. Dims 64 (one int8 k-step), 200 (padded to 256) and one case at 768; both
shadow formats (screen_i8 1 and 0). The radii are taken from the fixture's own exact distances.

CosineDistance handles get the fixture's centroids at unit length, which is what a trained
CosineDistance index holds (spherical k-means' last step) and what the pruning figure for unit
rows behind test_it_prunes' cap (229 of 84,760 pairs, 0.27 %, int8 at dim 200) was computed with. With the raw
centroids (norm ~28 against unit rows) the residuals of the three small lists are all but the
centroid itself, the int8 scale follows the centroid's largest entry, and the bound keeps every
pair of those lists: 5,338 candidates (6.3 %) at dim 200 int8, 428 at dim 64, 358 / 99 with bf16
(measured on the MI355X and restated on the CPU to the same counts). Results are exact either
way; DESIGN 7j records it."""
import functools

import numpy as np
import pytest

import oracle
import screen_ref as sr
from conftest import load_vdb

vdb = load_vdb()
pytestmark = pytest.mark.gpu

NPROBE, NQ = 5, 40
NONE = np.iinfo(np.uint64).max
FMAX = np.float32(np.finfo(np.float32).max)
INF = np.float32(np.inf)
PARENT_BUILD_ID = "94dadf6f86d76b82"  # vdb_build_id() of the commit this call was added to: no scan source changed


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, ref):
    (l, D, I), (lr, Dr, Ir) = got, ref
    assert l.dtype == np.uint64 and D.dtype == np.float32 and I.dtype == np.uint64
    assert l.tolist() == lr.tolist(), f"lims differ: {l.tolist()} ref {lr.tolist()}"
    bad = np.flatnonzero(I != Ir)
    assert bad.size == 0, f"ids differ at {bad[:5].tolist()}: {I[bad[0]]} ref {Ir[bad[0]]}"
    badd = np.flatnonzero(bits(D) != bits(Dr))
    assert badd.size == 0, f"dist bits differ at {badd[:5].tolist()}: {D[badd[0]]!r} ref {Dr[badd[0]]!r}"


@functools.lru_cache(maxsize=None)
def fixture(dim, kind="plain"):
    fx = sr.contract_fixture(dim, seed=1, nq=NQ, special=kind == "special", ties=kind == "ties")
    for a in (fx["X"], fx["ids"], fx["assign"], fx["C"], fx["Q"]):
        a.setflags(write=False)
    return fx


def unit(a):
    a64 = np.asarray(a, np.float64)
    n = np.sqrt((a64 * a64).sum(-1, keepdims=True))
    return (a64 / np.where(n > 0, n, 1.0)).astype(np.float32)


def centroids_of(fx, metric):
    return unit(fx["C"]) if metric == 3 else fx["C"]


def make(fx, metric, i8, live=True, **options):
    dim = fx["X"].shape[1]
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, 5, vdb.Metric(metric)))
    g.centroids = centroids_of(fx, metric)
    g.set_option("screen_i8", i8)
    g.set_option("screen_floor_ppm", 0)
    for name, value in options.items():
        g.set_option(name, value)
    g.set_batch(64)
    g.add_to_lists(fx["X"], fx["ids"], fx["assign"].astype(np.uint32))
    if live:
        g.search(fx["Q"], nprobe=NPROBE, k=10)
        assert g.profile_read()["screen_shadow"] == (2 if i8 else 1)
    return g


@functools.lru_cache(maxsize=None)
def handle(dim, metric, i8, kind="plain"):
    """A live-screen handle that the tests only read."""
    return make(fixture(dim, kind), metric, i8)


def radii_of(g, Q):
    """The radii under test, from the handle's own exact distances."""
    _, D, _ = g.range_search(Q, INF, nprobe=NPROBE)
    fin = np.sort(D[np.isfinite(D)])
    n = fin.size
    assert n > 80000
    return {"below": np.nextafter(fin[0], -INF, dtype=np.float32), "q001": fin[int(0.001 * n)], "q01": fin[int(0.01 * n)],
            "stored": fin[n // 3], "inf": INF, "fmax": FMAX, "ninf": -INF}


def both(g, Q, r, flt=None, **kw):
    """(exact result, screened result, the screened call's two timings)."""
    if flt is None:
        ex = g.range_search(Q, r, nprobe=NPROBE, **kw)
        sc = g.range_search(Q, r, nprobe=NPROBE, screen=True, **kw)
    else:
        ex = g.range_search_prepared(Q, flt, r, nprobe=NPROBE, **kw)
        sc = g.range_search_prepared(Q, flt, r, nprobe=NPROBE, screen=True, **kw)
    return ex, sc, g.range_screen_last_timing(), g.range_last_timing()


@functools.lru_cache(maxsize=None)
def oracle_full(dim, metric, kind):
    """Per query the oracle's whole single-query result (its real entries), computed once."""
    fx = fixture(dim, kind)
    o = oracle.OracleIndex(dim, 5, metric)
    o.centroids = fx["C"]
    for l in range(5):
        o.set_list(l, fx["lists"][l], fx["ids"][fx["assign"] == l])
    out = []
    for i in range(NQ):
        D, I = o.search(fx["Q"][i:i + 1], NPROBE, len(fx["X"]))
        real = I[0] != NONE
        out.append((D[0][real].copy(), I[0][real].copy()))
    return out


def oracle_cut(per_query, radius, keep):
    lims, Ds, Is = [0], [], []
    for i, (D, I) in enumerate(per_query):
        m = (D <= np.float32(radius)) & bool(keep[i])
        Ds.append(D[m])
        Is.append(I[m])
        lims.append(lims[-1] + int(m.sum()))
    return np.array(lims, np.uint64), np.concatenate(Ds).astype(np.float32), np.concatenate(Is).astype(np.uint64)


def mask_queries(res, keep):
    """A range result with the entries of the queries not kept dropped."""
    l, D, I = res
    m = np.zeros(D.size, bool)
    for i in range(len(l) - 1):
        m[int(l[i]):int(l[i + 1])] = keep[i]
    per = [int(m[int(l[i]):int(l[i + 1])].sum()) for i in range(len(l) - 1)]
    return np.concatenate([[0], np.cumsum(per)]).astype(np.uint64), D[m], I[m]


@functools.lru_cache(maxsize=None)
def restated(dim, metric, i8, kind):
    """(lb, tol) of every (query, row) pair of the fixture from screen_ref's restatement: the
    build, the pairs and the bound. int8: the kernel's bits (tol 0). CosineDistance (3): inner
    product over rows, queries and centroids brought to unit length here in float64, so close
    to the handle's bounds and not their bits."""
    fx = fixture(dim, kind)
    dp = (dim + 63) // 64 * 64
    to = unit if metric == 3 else (lambda a: a)
    m = 1 if metric == 3 else metric
    Cp, Qp = sr.pad_dp(centroids_of(fx, metric), dp), sr.pad_dp(to(fx["Q"]), dp)
    lbs, tols = [], []
    for l in range(5):
        if not len(fx["lists"][l]):
            continue
        sh, sc, meta = sr.build_restated(sr.pad_dp(to(fx["lists"][l]), dp), Cp[l], bool(i8))
        for q in range(NQ):
            row, asc, pst = sr.pairs_restated(Qp[q], Cp[l], m, bool(i8))
            lb, _, _, tol = sr.pair_bounds(row, asc, pst, sh, sc, meta, dp, m, bool(i8))
            lbs.append(lb.astype(np.float64))
            tols.append(np.asarray(tol, np.float64))
    return np.concatenate(lbs), np.concatenate(tols)


def kept(lb, r):
    with np.errstate(invalid="ignore"):
        return int((~(lb > np.float64(r))).sum())


# ---- 1. parity with the exact call and the oracle; 2. it is the screen that served ----
@pytest.mark.parametrize("kind", ["plain", "special", "ties"])
@pytest.mark.parametrize("dim", [64, 200])
@pytest.mark.parametrize("i8", [1, 0])
@pytest.mark.parametrize("metric", [0, 1, 3])
def test_parity_and_route(metric, i8, dim, kind):
    fx = fixture(dim, kind)
    g = handle(dim, metric, i8, kind)
    Q = fx["Q"]
    nrows = len(fx["X"])
    keep = np.ones(NQ, bool)
    if kind == "special" and metric != 0:
        keep[7] = False  # (the zero query against the +inf row: a NaN distance, the oracle's ranking undefined)
    for name, r in radii_of(g, Q).items():
        ex, sc, st, rt = both(g, Q, r)
        assert_same(sc, ex)
        assert not np.isnan(sc[1]).any()
        if metric != 3:
            assert_same(mask_queries(sc, keep), oracle_cut(oracle_full(dim, metric, kind), r, keep))
        assert st["screened_batches"] == 1 and st["exact_batches"] == 0, (name, st)
        assert st["pairs_bounded"] == NQ * nrows, (name, st)
        assert rt["pairs_scanned"] == st["candidates"] and rt["reruns"] == 0
        assert rt["hits"] == sc[2].size <= st["candidates"] <= st["pairs_bounded"]
        if name in ("inf", "fmax"):
            assert st["candidates"] == st["pairs_bounded"]
            assert sc[2].size >= NQ * (nrows - 5)
        if name == "below":  # (below every finite distance: only a -inf distance, the +inf row's under IP, is left)
            assert not np.isfinite(sc[1]).any() and (kind == "special" or sc[2].size == 0)
        if name == "stored":  # the inclusive compare: the row whose distance has exactly these bits is returned
            assert (bits(sc[1]) == bits(np.float32(r))).any()


def test_parity_at_768():
    fx = fixture(768)
    g = handle(768, 0, 1)
    for name, r in radii_of(g, fx["Q"]).items():
        ex, sc, st, rt = both(g, fx["Q"], r)
        assert_same(sc, ex)
        assert st["screened_batches"] == 1 and st["exact_batches"] == 0 and st["pairs_bounded"] == NQ * 2119
        assert rt["pairs_scanned"] == st["candidates"]
    lb, _ = restated(768, 0, 1, "plain")
    r = radii_of(g, fx["Q"])["q001"]
    assert both(g, fx["Q"], r)[2]["candidates"] == kept(lb, r)


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
        extra = fx["X"][:3] + np.float32(0.25)
        g.add_to_lists(extra, np.array([7, 8, 9], np.uint64), np.array([1, 2, 3], np.uint32))
    shadow = g.profile_read()["screen_shadow"]
    before = g.gpu_bytes_allocated()
    for r in (np.float32(0.0) if why == "cosine" else np.float32(60.0), INF):
        ex, sc, st, rt = both(g, fx["Q"], r)
        assert_same(sc, ex)
        assert st["screened_batches"] == 0 and st["exact_batches"] == 1, st
        assert st["pairs_bounded"] == 0 and st["candidates"] == 0
        assert rt["pairs_scanned"] == NQ * (2119 + (3 if why == "after_add" else 0))
    assert g.gpu_bytes_allocated() == before
    assert g.profile_read()["screen_shadow"] == shadow  # nothing built, nothing released
    if why in ("cosine", "fresh", "screen_off"):
        assert shadow == 0


def test_handle_is_left_as_found():
    fx = fixture(64)
    g = make(fx, 0, 1)
    r = radii_of(g, fx["Q"])["q01"]
    flt = g.prepare_filter(fx["ids"][:100], include=True)
    D0, I0 = g.search(fx["Q"], nprobe=NPROBE, k=10)
    before = g.gpu_bytes_allocated()
    ex, sc, st, _ = both(g, fx["Q"], r)
    assert_same(sc, ex)
    assert st["screened_batches"] == 1
    assert g.gpu_bytes_allocated() == before
    assert not flt.stale
    D1, I1 = g.search(fx["Q"], nprobe=NPROBE, k=10)
    assert D0.tobytes() == D1.tobytes() and I0.tobytes() == I1.tobytes()
    assert vdb.build_id() == PARENT_BUILD_ID


# ---- 3. the bound is the screen's; 4. it prunes ----
@pytest.mark.parametrize("kind", ["plain", "special"])
@pytest.mark.parametrize("dim", [64, 200])
@pytest.mark.parametrize("i8", [1, 0])
@pytest.mark.parametrize("metric", [0, 1])
def test_candidates_are_the_restated_bound(metric, i8, dim, kind):
    fx = fixture(dim, kind)
    g = handle(dim, metric, i8, kind)
    lb, tol = restated(dim, metric, i8, kind)
    assert lb.size == NQ * len(fx["X"])
    rs = radii_of(g, fx["Q"])
    for name in ("below", "q001", "q01", "stored", "fmax"):
        r = rs[name]
        _, _, st, _ = both(g, fx["Q"], r)
        if i8:
            assert st["candidates"] == kept(lb, r), (name, st["candidates"], kept(lb, r))
        else:
            lo, hi = kept(lb + tol, r), kept(lb - tol, r)
            print("bf16 candidates %s: %d in [%d, %d]" % (name, st["candidates"], lo, hi))
            assert lo <= st["candidates"] <= hi, (name, lo, st["candidates"], hi)


@pytest.mark.parametrize("dim", [64, 200])
@pytest.mark.parametrize("i8", [1, 0])
@pytest.mark.parametrize("metric", [0, 1, 3])
def test_it_prunes(metric, i8, dim):
    """At the 0.1 % quantile of the exact distances at most 1 % of the pairs are re-checked. The
    restated bound alone keeps at most 0.27 % on this fixture; it is recomputed here."""
    fx = fixture(dim)
    g = handle(dim, metric, i8)
    r = radii_of(g, fx["Q"])["q001"]
    ex, sc, st, rt = both(g, fx["Q"], r)
    assert_same(sc, ex)
    print("metric %d i8 %d dim %d: %d candidates of %d pairs, %d hits" %
          (metric, i8, dim, st["candidates"], st["pairs_bounded"], rt["hits"]))
    assert st["pairs_bounded"] == NQ * 2119
    assert rt["hits"] <= st["candidates"] <= st["pairs_bounded"] // 100
    assert rt["hits"] >= 80
    # the restated bound alone, at the same threshold (CosineDistance: the radius is a mapped
    # distance; the scan thresholds -dot at the largest t with fl(1.0f + t) <= r)
    lb, tol = restated(dim, metric, i8, "plain")
    t = r
    if metric == 3:
        t = np.float32(r) - np.float32(1.0)
        while np.float32(1.0) + np.nextafter(t, INF, dtype=np.float32) <= np.float32(r):
            t = np.nextafter(t, INF, dtype=np.float32)
        while np.float32(1.0) + t > np.float32(r):
            t = np.nextafter(t, -INF, dtype=np.float32)
    print("restated: %d" % kept(lb - tol, t))
    assert kept(lb - tol, t) <= lb.size // 100


# ---- 5. filters ----
@pytest.mark.parametrize("i8", [1, 0])
@pytest.mark.parametrize("metric", [0, 1])
def test_filters(metric, i8):
    fx = fixture(200)
    g = handle(200, metric, i8)
    Q, ids = fx["Q"], fx["ids"]
    rs = radii_of(g, Q)
    hub_ids = g.get_list(0)[1]  # the hub's ids in slot order
    rng = np.random.default_rng(7)
    filters = {"include 5 %": g.prepare_filter(rng.choice(ids, len(ids) // 20, replace=False), include=True),
               "exclude ten": g.prepare_filter(ids[100:110], include=False),
               "hub blocks 1..9 emptied": g.prepare_filter(hub_ids[64:640], include=False)}
    for what, flt in filters.items():
        for name in ("q001", "q01", "inf", "ninf"):
            ex, sc, st, rt = both(g, Q, rs[name], flt)
            assert_same(sc, ex)
            assert st["screened_batches"] == 1 and st["exact_batches"] == 0, (what, name, st)
            assert st["pairs_bounded"] == NQ * flt.allowed, (what, name)
            assert rt["pairs_scanned"] == st["candidates"]
            if name == "inf":
                assert st["candidates"] == NQ * flt.allowed and sc[2].size == NQ * flt.allowed
        assert not flt.stale
    # flt = None is the unfiltered call
    ex, sc, st, _ = both(g, Q, rs["q01"])
    assert_same(g.range_search_prepared(Q, None, rs["q01"], nprobe=NPROBE, screen=True), ex)


def test_filter_refusals():
    fx = fixture(64)
    g, other = make(fx, 0, 1), make(fx, 0, 1)
    flt = g.prepare_filter(fx["ids"][:50], include=True)
    with pytest.raises(vdb.VdbError) as e:
        other.range_search_prepared(fx["Q"], flt, 10.0, nprobe=NPROBE, screen=True)
    assert e.value.code == -1  # VDB_ERR_INVALID_ARGUMENT
    with pytest.raises(vdb.VdbError) as e:
        g.range_search(fx["Q"], np.float32(np.nan), nprobe=NPROBE, screen=True)
    assert e.value.code == -1
    g.add(fx["X"][:2] + np.float32(0.5), np.array([5, 6], np.uint64))
    assert flt.stale
    with pytest.raises(vdb.VdbError) as e:
        g.range_search_prepared(fx["Q"], flt, 10.0, nprobe=NPROBE, screen=True)
    assert e.value.code == -5  # VDB_ERR_STATE


# ---- 6. fallback and re-run ----
@pytest.mark.parametrize("i8", [1, 0])
def test_fallback_and_rerun(i8):
    fx = fixture(64, "special")
    g = handle(64, 0, i8, "special")
    Q = fx["Q"]
    rs = radii_of(g, Q)
    ex, sc, st, rt = both(g, Q, rs["q01"])
    cand, hits = st["candidates"], rt["hits"]
    assert cand > 64 and rt["reruns"] == 0
    # reserve 16: 64 candidate entries, the bound keeps more: the exact scan serves the batch
    ex16, sc16, st16, rt16 = both(g, Q, rs["q01"], reserve=16)
    assert_same(sc16, ex)
    assert_same(ex16, ex)
    assert st16["screened_batches"] == 0 and st16["exact_batches"] == 1
    assert st16["candidates"] == cand and rt16["pairs_scanned"] == NQ * len(fx["X"]) * (1 + rt16["reruns"])
    assert rt16["reruns"] == 1  # (the exact scan's own re-run: 16 entries do not hold the hits)
    # candidates fit, hits do not: only the re-check runs again
    reserve = (cand + 3) // 4
    assert reserve < hits, (cand, hits)
    exr, scr, str_, rtr = both(g, Q, rs["q01"], reserve=reserve)
    assert_same(scr, ex)
    assert str_["screened_batches"] == 1 and str_["exact_batches"] == 0 and rtr["reruns"] == 1
    assert str_["candidates"] == cand and rtr["pairs_scanned"] == 2 * cand
    # +inf at the default reserve: every pair is a candidate; rows with an inf entry come back as
    # the exact call returns them, NaN distances never
    exi, sci, sti, rti = both(g, Q, INF)
    assert_same(sci, exi)
    assert sti["candidates"] == sti["pairs_bounded"] == NQ * len(fx["X"]) and sti["screened_batches"] == 1
    assert np.isinf(sci[1]).any() and not np.isnan(sci[1]).any()


# ---- 7. shapes ----
@pytest.mark.parametrize("i8", [1, 0])
def test_batches_and_degenerate_shapes(i8):
    fx = fixture(200)
    g = make(fx, 1, i8)
    Q = fx["Q"]
    r = radii_of(g, Q)["q01"]
    ex, sc, st, rt = both(g, Q, r)
    assert_same(sc, ex)
    g.set_batch(8)
    ex8, sc8, st8, rt8 = both(g, Q, r)
    assert_same(sc8, ex)
    assert_same(ex8, ex)
    assert st8["screened_batches"] == 5 and st8["exact_batches"] == 0
    assert st8["pairs_bounded"] == st["pairs_bounded"] and st8["candidates"] == st["candidates"]
    assert rt8["pairs_scanned"] == st8["candidates"]
    one = g.range_search(Q[3:4], r, nprobe=NPROBE, screen=True)
    lo, hi = int(ex[0][3]), int(ex[0][4])
    assert one[0].tolist() == [0, hi - lo]
    assert one[1].tobytes() == ex[1][lo:hi].tobytes() and one[2].tobytes() == ex[2][lo:hi].tobytes()
    none = g.range_search(Q[:0], r, nprobe=NPROBE, screen=True)
    assert none[0].tolist() == [0] and none[1].size == 0
    zero = g.range_search(Q, INF, nprobe=0, screen=True)
    assert zero[0].tolist() == [0] * (NQ + 1) and zero[2].size == 0
    empty = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(200, 5, vdb.Metric.InnerProduct))
    empty.centroids = fx["C"]
    got = empty.range_search(Q, INF, nprobe=NPROBE, screen=True)
    assert got[0].tolist() == [0] * (NQ + 1) and got[2].size == 0
