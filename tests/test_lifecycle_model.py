"""CPU: the lifecycle model (lifecycle_model.py) against itself and the oracle, so that a wrong
model cannot agree with a wrong kernel in test_gpu_lifecycle.py; and the scripted scenario on the
model alone: every step hits its edge (the generator's own assertions) and leaves the list sizes
that SCRIPT_SIZES pins."""

import numpy as np
import pytest

import lifecycle_model as lm
import oracle
from lifecycle_model import NLIST, NONE, NQ
from test_gpu_upsert import bits, winners

CASES = [(30, 0), (30, 3), (200, 1)]


def same_state(a, b):
    assert a.sizes() == b.sizes()
    for (va, ia), (vb, ib) in zip(a.lists, b.lists):
        assert np.array_equal(ia, ib) and np.array_equal(bits(va), bits(vb))


def same(got, want):
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(bits(got[0]), bits(want[0]))


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "dim%d-metric%d" % c)
def base(request):
    dim, metric = request.param
    return dim, metric, lm.start(dim, metric)


def requests(m, src):
    stored = np.unique(m.stored_ids())
    a = stored[::9]  # every id stored
    b = np.concatenate([stored[5::40], src.ids(40)])  # mixed
    c = np.concatenate([stored[7::50], src.ids(20), stored[7::100], stored[7:8]])  # an id three times, others twice
    return [a, b, c[src.r.permutation(len(c))]]


def test_start_is_the_oracle_s_add(base):
    dim, metric, m = base
    X, Q, ids, C = lm.fixture(dim)
    o = oracle.OracleIndex(dim, NLIST, m.om)
    o.centroids = C
    o.add(m.prep(X), ids)
    assert m.total == lm.N == o.total_vectors
    for l in range(NLIST):
        v, i = o.get_list(l)
        assert np.array_equal(m.lists[l][1], i) and np.array_equal(bits(m.lists[l][0]), bits(v))
    if metric != 3:
        same(m.search(Q, 3, 10), o.search(Q, 3, 10))


def test_upsert_is_remove_then_add(base):
    dim, metric, m0 = base
    src = lm.Source(dim, 3)
    for req in requests(m0, src):
        V = src.rows(len(req))
        a, b = m0.copy(), m0.copy()
        w = winners(req)
        replaced, inserted = a.upsert(V, req)
        assert b.remove(req) == replaced == int(np.isin(m0.stored_ids(), req).sum())
        b.add(V[w], req[w])
        assert inserted == int(w.sum()) == len(set(req.tolist()))
        same_state(a, b)
        got, found = a.fetch(req)  # the last write of every id is the one stored
        last = {int(i): j for j, i in enumerate(req)}
        assert found.all() and np.array_equal(bits(got), bits(a.prep(V)[[last[int(i)] for i in req]]))
    assert not winners(requests(m0, src)[2]).all()  # (the third pattern repeats ids)


def test_remove_of_absent_ids_is_the_identity(base):
    dim, metric, m0 = base
    m = m0.copy()
    assert m.remove(lm.ABSENT) == 0
    same_state(m, m0)
    assert not m.fetch(lm.ABSENT)[1].any() and not m.fetch(lm.ABSENT)[0].any()


def test_an_empty_exclude_is_the_plain_search(base):
    dim, metric, m = base
    Q = lm.fixture(dim)[1]
    none = np.zeros(0, np.uint64)
    for nprobe, k in ((3, 10), (NLIST, 10), (2, 1024)):
        same(m.search_allowed(Q, nprobe, k, none, False), m.search(Q, nprobe, k))
    assert m.allowed_count(none, False) == m.total and m.allowed_count(none, True) == 0
    D, I = m.search_allowed(Q, 3, 10, none, True)
    assert (I == NONE).all() and (D == lm.FMAX).all()
    # per-query filters: each filter's queries, in call order, are that filter's own search
    half = (np.unique(m.stored_ids())[::2], True)
    fo = np.random.RandomState(2).permutation(np.arange(NQ) % 2)
    D, I = m.search_multi(Q, 3, 10, [(none, False), half], fo)
    same((D[fo == 0], I[fo == 0]), m.search(Q[fo == 0], 3, 10))
    same((D[fo == 1], I[fo == 1]), m.search_allowed(Q[fo == 1], 3, 10, *half))


def test_range_at_inf_is_the_search_s_real_entries(base):
    dim, metric, m = base
    Q = lm.fixture(dim)[1]
    lims, D, I = m.range(Q, 3, np.inf)
    for i in range(NQ):
        Ds, Is = m.search(Q[i:i + 1], 3, m.total)
        real = Is[0] != NONE
        lo, hi = int(lims[i]), int(lims[i + 1])
        assert hi - lo == int(real.sum()) > 0
        same((D[lo:hi], I[lo:hi]), (Ds[0][real], Is[0][real]))
    allD = np.concatenate([d for d, _ in m.full(Q, 3)])
    below = np.nextafter(allD.min(), np.float32(-np.inf), dtype=np.float32)
    assert m.range(Q, 3, below)[0].tolist() == [0] * (NQ + 1)
    lims, D, I = m.range(Q, 3, np.median(allD))
    assert 0 < D.size < allD.size and (D <= np.float32(np.median(allD))).all()


def test_exhaustive_is_the_search_of_every_list(base):
    dim, metric, m = base
    Q = lm.fixture(dim)[1]
    assert len(m.twice()) == 0
    for k in (10, 64):
        D, I = m.exhaustive(Q, k)
        for i in range(NQ):  # (a query on its own: no slot of an earlier query takes part)
            Ds, Is = m.search(Q[i:i + 1], NLIST, k)
            same((D[i], I[i]), (Ds[0], Is[0]))


def test_fetch_and_search_ids(base):
    dim, metric, m0 = base
    m = m0.copy()
    la, lb = [l for l in range(NLIST) if m.sizes()[l] > 3][:2]  # (la < lb)
    i0, i1 = m.lists[lb][1][3], m.lists[la][1][0]
    extra = lm.Source(dim, 4).rows(2)
    m.add_to_lists(extra, np.array([i0, i1], np.uint64), np.array([la, lb], np.uint32))
    req = np.concatenate([[i0, i1], lm.ABSENT[:2], m.lists[lb][1][:3]]).astype(np.uint64)
    V, F = m.fetch(req)
    assert F.tolist() == [1, 1, 0, 0, 1, 1, 1] and not V[2:4].any()
    assert np.array_equal(bits(V[0]), bits(m.prep(extra)[0]))  # the copy in the lower list comes first
    assert np.array_equal(bits(V[1]), bits(m0.lists[la][0][0]))  # the original is in the lower list
    D, I, Fs = m.search_ids(req, 3, 10)
    assert np.array_equal(Fs, F) and (I[F == 0] == NONE).all() and (D[F == 0] == lm.FMAX).all()
    same((D[F == 1], I[F == 1]), m.search(V[F == 1], 3, 10))
    if metric != 1:  # (L2 and unit rows: a stored row's nearest row is itself)
        assert np.array_equal(I[F == 1][:, 0], req[F == 1])


def test_new_centroids_keep_every_row_in_its_list(base):
    dim, metric, m0 = base
    m = m0.copy()
    m.set_centroids(m.C + np.float32(0.05))
    same_state(m, m0)
    assert not np.array_equal(bits(m.C), bits(m0.C))


def run_on_model(gen, m):
    sizes = [m.sizes()]
    names = ["start"]
    for name, ops in gen:
        for op in ops:
            lm.apply(m, op)
        sizes.append(m.sizes())
        names.append(name)
    return names, sizes


@pytest.mark.parametrize("dim,metric", CASES)
def test_scripted_hits_every_edge(dim, metric):
    m = lm.start(dim, metric)
    names, sizes = run_on_model(lm.scripted(m, dim), m)
    for n, s in zip(names, sizes):
        print("%-30s %s  %d rows, %d blocks" % (n, s, sum(s), lm.blocks(s)))
    assert len(names) == 1 + 15
    assert sizes == lm.SCRIPT_SIZES[(dim, metric)]
    # an arena whose block count went down and then up again, past where it started
    b = [lm.blocks(s) for s in sizes]
    assert min(b) < b[0] * 6 // 10 and max(b[b.index(min(b)):]) > b[0]
    # a list that became empty, one at exactly 64 rows, one of one row; an id stored twice
    assert any(0 in s for s in sizes[1:]) and any(64 in s for s in sizes) and any(1 in s for s in sizes)
    assert len(m.twice()) > 0


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("dim,metric", CASES[:2])
def test_walk_runs_on_the_model(dim, metric, seed):
    m = lm.start(dim, metric)
    names, sizes = run_on_model(lm.walk(m, dim, seed), m)
    assert len(names) == 1 + lm.WALK_STEPS and all(sum(s) > 0 for s in sizes)
    # every operation is drawn, whatever the seed, and the steps are the ones walk_ops names
    ops = lm.walk_ops(seed)
    assert set(ops) == set(lm.WALK_OPS) and len(ops) == lm.WALK_STEPS, f"seed {seed}: {ops}"
    assert [n.split(": ")[1] for n in names[1:]] == ops
    # a remove and an upsert run while ids are stored twice (add_to_lists stores a quarter of its ids again)
    assert {"remove", "upsert"} <= set(ops[ops.index("add_to_lists") + 1:]), f"seed {seed}: {ops}"
    for n, s in zip(names, sizes):
        print("%-36s %s" % (n, s))
