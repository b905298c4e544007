"""k and nprobe at the register boundaries of the wave top-k (csrc/wave_topk.hpp), end to end.

A wave's top-k list is spread over 64 lanes x R registers, R = 1, 2, 4, 8, 16 chosen by
topk_regs(k) for the scans and merges and by topk_regs(nprobe) for the coarse selection. KS
holds the values at which R changes and at which the `e < k` guards meet `r * 64 + lane`. The
reference is the CPU oracle everywhere, ids and distance bits equal.

Fixture of the k tests: dim 20 (padded), 24 queries, nlist 12, 4,492 rows placed with
add_to_lists / set_list into lists of LENS rows (two empty, so at nprobe 12 every query has
stale slots; the hub list has 35 segments at seg_vectors 64, above kMergeFan = 32, so the
un-fused chain runs its level-1 merge). The ids of 60 hub rows are stored a second time in list
9: 30 with the same vector (equal (d, id) pairs), 30 with another vector (one id at two
distances). Two data kinds: `normal` (distance bits depend on the summation order) and `grid`
(coordinates in {-1, 0, 1}: distances are small integers, so ranks are decided by id and
equal-distance pairs straddle every register edge). test_fixture_preconditions asserts on the
oracle alone, without a GPU, that the fixture has these properties.

Which kernel instantiation each test launches, from the dispatch in engine.hpp (scan_batch,
coarse_batch) and kernels.hip; R(v) = 1 for v = 64, 2 for 65 and 128, 4 for 129 and 256, 8 for 257
and 512, 16 for 513, 1023 and 1024:
* ivf_select_probes<R(nprobe)>: test_nprobe_boundaries, coarse mode 0 (every metric) and Cosine
  in both modes; ivf_select_rerank<R(nprobe)>: the same test, mode 1, L2 and IP.
* ivf_scan_narrow<R(k), metric, interleaved>: test_k_boundaries[*-il], test_k_above_candidates
  and test_k_boundaries_without_stale_slots (R = 16, and 2, 8, 16); ivf_scan_narrow<R(k), metric,
  rows> for R >= 2: test_k_boundaries[*-rows] (at k = 64 the screen serves that layout).
* ivf_merge_fused<R(k)>: every search at default options, so every test above.
* ivf_merge_partials / ivf_merge_slots / ivf_merge_query<R> and ivf_carry_slots, R = 2, 4, 8, 16
  (k = 65, 129, 257, 513 and 1024): test_k_boundaries with fused_merge 0; the level-1 merge has
  items at seg_vectors 64, the carry is read at set_batch 7. Also R = 2, 8, 16 in
  test_k_boundaries_without_stale_slots. (R = 1 un-fused stays with
  test_gpu_tier_shard.py::test_queries_read_in_place_and_misaligned.)
* ivf_merge_ranks<R(k)>, R = 1 also at k = 1 and 10: test_merge_ranks_boundaries, both entry points.
"""
import numpy as np
import pytest

import oracle
from conftest import load_vdb
from test_gpu_parity import assert_same, bits, mirror_from_oracle

vdb = load_vdb()
gpu = pytest.mark.gpu

KS = [64, 65, 128, 129, 256, 257, 512, 513, 1023, 1024]
EDGES = [64, 128, 256, 512]  # elements e - 1 | e lie in two registers
DIM, NQ, NLIST = 20, 24, 12
LENS = [0, 1, 63, 64, 65, 127, 129, 300, 513, 1030, 2200, 0]
N = sum(LENS)
HUB, TWIN = 10, 9
NONE = np.iinfo(np.uint64).max
FMAX = np.finfo(np.float32).max
BATCH_DEFAULT = 256
KINDS = ["normal", "grid"]
_data, _oracles, _answers = {}, {}, {}


def data(kind):
    """(X, Q, ids, lists, C) computed once per kind and never changed. Row r goes to list
    lists[r]; the rows of a list keep their global order."""
    if kind not in _data:
        rng = np.random.RandomState(41)
        if kind == "normal":
            X, Q, _ = oracle.reference_test_data(N, NQ, DIM, seed=5100)
            C = oracle.gen_normal(5101, NLIST * DIM).reshape(NLIST, DIM)
            X = X.copy()
        else:
            g = np.random.RandomState(43)
            X = g.randint(-1, 2, size=(N, DIM)).astype(np.float32)
            Q = g.randint(-1, 2, size=(NQ, DIM)).astype(np.float32)
            C = g.randint(-1, 2, size=(NLIST, DIM)).astype(np.float32)
        lists = rng.permutation(np.repeat(np.arange(NLIST, dtype=np.uint32), LENS))
        ids = rng.permutation(N).astype(np.uint64) * 3 + 7
        hub_rows = np.flatnonzero(lists == HUB)[200:260]
        twin_rows = np.flatnonzero(lists == TWIN)[40:100]
        ids[twin_rows] = ids[hub_rows]
        X[twin_rows[:30]] = X[hub_rows[:30]]
        if kind == "grid":  # (the other 30 must differ from their hub rows)
            X[twin_rows[30:]] = -X[hub_rows[30:]] + (np.abs(X[hub_rows[30:]]).sum(axis=1, keepdims=True) == 0)
        for a in (X, Q, ids, lists, C):
            a.setflags(write=False)
        _data[kind] = (X, Q, ids, lists, C)
    return _data[kind]


def oracle_of(kind, metric):
    if (kind, metric) not in _oracles:
        X, Q, ids, lists, C = data(kind)
        o = oracle.OracleIndex(DIM, NLIST, metric)
        o.centroids = C
        for l in range(NLIST):
            rows = np.flatnonzero(lists == l)
            o.set_list(l, X[rows], ids[rows])
        _oracles[(kind, metric)] = o
    return _oracles[(kind, metric)]


def answer(kind, metric, k, nprobe, stale=True):
    """The oracle's answer, computed once per (k, nprobe) and reused. stale=False: the oracle one
    query at a time, where an empty probed list contributes nothing (set_stale_slots(False))."""
    key = (kind, metric, k, nprobe, stale)
    if key not in _answers:
        o, Q = oracle_of(kind, metric), data(kind)[1]
        if stale:
            D, I = o.search(Q, nprobe, k)
        else:
            out = [o.search(Q[i:i + 1], nprobe, k) for i in range(NQ)]
            D, I = np.concatenate([d for d, _ in out]), np.concatenate([i for _, i in out])
        D.setflags(write=False)
        I.setflags(write=False)
        _answers[key] = (D, I)
    return _answers[key]


def make(kind, metric, layout):
    X, Q, ids, lists, C = data(kind)
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(DIM, NLIST, vdb.Metric(metric)))
    g.centroids = C
    if layout == "il":  # the interleaved arena
        g.set_option("screen", 0)
        g.add_to_lists(X, ids, lists)
    else:  # "rows": the screen built, its row-major copy is what the exact scans of k > 64 read
        g.add_to_lists(X, ids, lists)
        assert_same(*g.search(Q, nprobe=5, k=10), *answer(kind, metric, 10, 5))
        assert g.profile_read()["screen_shadow"] in (1, 2)
    assert g.list_sizes().tolist() == LENS
    return g


# ---- the fixture is what the tests need it to be (oracle only, no GPU) -------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_fixture_preconditions(kind):
    X, Q, ids, lists, C = data(kind)
    assert np.bincount(lists, minlength=NLIST).tolist() == LENS
    # the hub list: more than kMergeFan = 32 segments at seg_vectors 64
    assert (LENS[HUB] + 63) // 64 > 32
    # 60 ids stored twice, in the hub list and in list 9: 30 with one vector, 30 with two
    u, cnt = np.unique(ids, return_counts=True)
    twice = u[cnt == 2]
    assert len(twice) == 60 and cnt.max() == 2
    same = 0
    for t in twice:
        a, b = np.flatnonzero(ids == t)
        assert {int(lists[a]), int(lists[b])} == {HUB, TWIN}
        same += bool(np.array_equal(X[a], X[b]))
    assert same == 30
    for metric in (0, 1, 2):
        o = oracle_of(kind, metric)
        # both empty lists are probed at nprobe 12: every query after the first has stale slots
        for q in Q:
            assert {0, NLIST - 1} <= set(o.select_nprobe(q, 12).tolist())
        D, I = answer(kind, metric, 1024, 12)
        assert np.all(I != NONE), "every query fills all 1024 slots"
        for row in I:
            assert len(np.unique(row)) == len(row), "no output row repeats an id"
        D5, I5 = answer(kind, metric, 1024, 5)
        filled = (I5 != NONE).sum(axis=1)
        assert filled.min() < 1024 and filled.min() >= 64, "padding starts inside the list at nprobe 5"
        assert np.all(D5[I5 == NONE] == FMAX)
        if kind == "grid" or metric == 2:
            # an equal-distance pair straddles each register edge: the order there is by id alone
            for e in EDGES:
                straddle = int((bits(D[:, e - 1]) == bits(D[:, e])).sum())
                assert straddle >= 20, (kind, metric, e, straddle)
                assert np.all(I[:, e - 1][D[:, e - 1] == D[:, e]] < I[:, e][D[:, e - 1] == D[:, e]])


class Differences:
    """Compares like assert_same, for every setting of a case before it fails: the failure then
    names each (k, nprobe, options) that differed, which tells the register count at fault."""

    def __init__(self):
        self.bad = []

    def same(self, what, D, I, Dr, Ir):
        try:
            assert_same(D, I, Dr, Ir)
        except AssertionError as e:
            self.bad.append(f"{what}: {e}")

    def none(self):
        assert not self.bad, f"{len(self.bad)} settings differ:\n" + "\n".join(self.bad)


# ---- k at the register boundaries -------------------------------------------------------------
K_CASES = [(kind, metric, layout) for kind in KINDS for metric in (0, 1, 2) for layout in ("il", "rows")
           if not (layout == "rows" and metric == 2)]  # (no screen for Cosine: its lists stay interleaved)
OPTION_KS = [65, 129, 257, 513, 1024]


@gpu
@pytest.mark.parametrize("kind,metric,layout", K_CASES, ids=[f"{a}-m{m}-{l}" for a, m, l in K_CASES])
def test_k_boundaries(kind, metric, layout):
    """Every k of KS at nprobe 5 (padding starts inside and across registers) and 12 (all 1024
    slots filled, stale slots, duplicates across two lists) at default options. Then both merge
    chains at the first k of every R > 1 and at 1024: seg_vectors 64 cuts the hub list into 35
    segments (the un-fused chain then runs its level-1 merge), set_batch 7 makes the carry cross
    internal batches."""
    Q = data(kind)[1]
    g = make(kind, metric, layout)
    diff = Differences()
    for k in KS:
        for nprobe in (5, 12):
            diff.same(f"k={k} nprobe={nprobe}", *g.search(Q, nprobe=nprobe, k=k), *answer(kind, metric, k, nprobe))
    for fused in (1, 0):
        g.set_option("fused_merge", fused)
        for seg in (0, 64):
            g.set_option("seg_vectors", seg)
            for batch in (BATCH_DEFAULT, 7):
                g.set_batch(batch)
                for k in OPTION_KS:
                    diff.same(f"k={k} nprobe=12 fused_merge={fused} seg_vectors={seg} batch={batch}",
                              *g.search(Q, nprobe=12, k=k), *answer(kind, metric, k, 12))
    diff.none()


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_k_boundaries_without_stale_slots(kind):
    """set_stale_slots(False): an empty probed list contributes nothing, which is what the oracle
    gives a call of one query. Both merge chains."""
    Q = data(kind)[1]
    diff = Differences()
    for metric in (0, 2):
        g = make(kind, metric, "il")
        g.set_stale_slots(False)
        for fused in (1, 0):
            g.set_option("fused_merge", fused)
            for k in (65, 257, 1024):
                diff.same(f"metric={metric} k={k} fused_merge={fused}", *g.search(Q, nprobe=12, k=k),
                          *answer(kind, metric, k, 12, stale=False))
    diff.none()


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_k_above_candidates(kind):
    """nprobe 1 and 2 at k = 1024: each slot's min(k, n_l) cut-off falls at 1, 63, 64, 65, 127,
    129, 300, ...; everything behind the candidates is (FLT_MAX, UINT64_MAX)."""
    Q = data(kind)[1]
    seen = set()
    for metric in (0, 1, 2):
        g = make(kind, metric, "il")
        for nprobe in (1, 2):
            D, I = g.search(Q, nprobe=nprobe, k=1024)
            Dr, Ir = answer(kind, metric, 1024, nprobe)
            assert_same(D, I, Dr, Ir)
            filled = (Ir != NONE).sum(axis=1)
            seen |= set(filled.tolist())
            for q in range(NQ):
                assert np.all(I[q, filled[q]:] == NONE) and np.all(bits(D[q, filled[q]:]) == bits(FMAX))
                assert np.all(I[q, :filled[q]] != NONE)
    # (cut-offs inside and between registers; Cosine, every coarse distance 0.0f, probes lists 0, 1)
    assert len(seen & {1, 63, 64, 65, 127, 129, 300, 513}) >= 5, seen


# ---- nprobe at the register boundaries ----------------------------------------------------------
P_NLIST, P_DIM, P_N, P_NQ = 1100, 8, 3000, 12
_pdata = {}


def probe_data(centroids):
    if centroids not in _pdata:
        X, Q, ids = oracle.reference_test_data(P_N, P_NQ, P_DIM, seed=5200)
        if centroids == "normal":
            C = oracle.gen_normal(5201, P_NLIST * P_DIM).reshape(P_NLIST, P_DIM)
        else:  # exact coarse ties, decided by list id
            C = np.random.RandomState(44).randint(-1, 2, size=(P_NLIST, P_DIM)).astype(np.float32)
            Q = np.random.RandomState(45).randint(-1, 2, size=(P_NQ, P_DIM)).astype(np.float32)
        ids = ids * 5 + 11
        for a in (X, Q, ids, C):
            a.setflags(write=False)
        _pdata[centroids] = (X, Q, ids, C)
    return _pdata[centroids]


def probe_pair(centroids, metric):
    X, Q, ids, C = probe_data(centroids)
    o = oracle.OracleIndex(P_DIM, P_NLIST, metric)
    o.centroids = C
    o.add(X, ids)
    g = mirror_from_oracle(o, P_DIM, P_NLIST, metric)
    g.add(X, ids)
    return g, o


@pytest.mark.parametrize("centroids", ["normal", "grid"])
def test_probe_fixture_preconditions(centroids):
    X, Q, ids, C = probe_data(centroids)
    for metric in (0, 1, 2):
        o = oracle.OracleIndex(P_DIM, P_NLIST, metric)
        o.centroids = C
        o.add(X, ids)
        assert sum(o.list_count(l) == 0 for l in range(P_NLIST)) > 100, "many lists are empty"
    if centroids == "grid":  # duplicated centroids: coarse ties that the list id decides
        assert len(np.unique(C, axis=0)) < P_NLIST - 50


@gpu
@pytest.mark.parametrize("centroids", ["normal", "grid"])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_nprobe_boundaries(metric, centroids):
    """nprobe at every value of KS, through the MFMA bounds + exact re-rank (coarse mode 1) and
    the exact selection (mode 0; Cosine takes it either way)."""
    Q = probe_data(centroids)[1]
    g, o = probe_pair(centroids, metric)
    ref = {p: o.search(Q, p, 10) for p in KS}
    diff = Differences()
    for mode in (1, 0):
        g.set_coarse_mode(mode)
        for p in KS:
            diff.same(f"nprobe={p} coarse_mode={mode}", *g.search(Q, nprobe=p, k=10), *ref[p])
    diff.none()


# ---- the rank merge -----------------------------------------------------------------------------
def rank_partials(nranks, n, k, seed):
    """Per-rank partials [nranks][n][k], each row sorted by (dist, id) with unique ids, as a
    shard's search leaves them: distances from a tie-heavy pool, ids shared between ranks at
    equal and at different distances, (FLT_MAX, UINT64_MAX) tails of differing lengths, one rank
    that is all padding, one row in which every rank is."""
    rng = np.random.RandomState(seed)
    pool = np.array([-3.0, -0.5, 0.0, 0.25, 0.25000003, 1.0, 7.5, 1.0e10], np.float32)
    D = np.full((nranks, n, k), FMAX, np.float32)
    I = np.full((nranks, n, k), NONE, np.uint64)
    for q in range(n):
        universe = rng.permutation(3 * k + 8).astype(np.uint64) * 3 + 1 + (np.uint64(q % 2) << np.uint64(33))
        shared_d = pool[rng.randint(0, len(pool), size=len(universe))]
        for r in range(nranks):
            if q == n - 1 or (r == 1 and nranks > 2):
                continue  # all padding
            m = k if (r + q) % 3 == 0 else int(rng.randint(0, k + 1))
            pick = rng.choice(len(universe), size=m, replace=False)
            d = shared_d[pick].copy()  # a shared id at the same distance on every rank ...
            other = rng.random_sample(m) < 0.3
            d[other] = pool[rng.randint(0, len(pool), size=int(other.sum()))]  # ... or at another
            order = np.lexsort((universe[pick], d))
            D[r, q, :m] = d[order]
            I[r, q, :m] = universe[pick][order]
    return D, I


@gpu
@pytest.mark.parametrize("nranks", [1, 2, 3, 8])
def test_merge_ranks_boundaries(nranks):
    import torch
    dev = torch.device("cuda:0")
    n = 9  # two full workgroups of four waves and one wave
    s = torch.cuda.current_stream().cuda_stream
    for k in [1, 10] + KS:
        D, I = rank_partials(nranks, n, k, seed=1000 * nranks + k)
        Dr, Ir = oracle.merge_ranks(D, I, k)
        pd = torch.from_numpy(D).to(dev)
        pi = torch.from_numpy(I.view(np.int64)).to(dev)
        od = torch.empty((n, k), dtype=torch.float32, device=dev)
        oi = torch.empty((n, k), dtype=torch.int64, device=dev)
        vdb.merge_ranks_device(pd.data_ptr(), pi.data_ptr(), nranks, n, k, od.data_ptr(), oi.data_ptr(), s)
        torch.cuda.synchronize()
        assert_same(od.cpu().numpy(), oi.cpu().numpy().view(np.uint64), Dr, Ir)
        rec, off = vdb.rank_record_bytes(n, k), vdb.rank_record_ids_offset(n, k)
        recs = np.zeros((nranks, rec), np.uint8)
        for r in range(nranks):
            recs[r, :D[r].nbytes] = D[r].view(np.uint8).ravel()
            recs[r, off:off + I[r].nbytes] = I[r].view(np.uint8).ravel()
        rd = torch.from_numpy(recs.ravel()).to(dev)
        od.zero_()
        oi.zero_()
        vdb.merge_ranks_packed_device(rd.data_ptr(), nranks, n, k, od.data_ptr(), oi.data_ptr(), s)
        torch.cuda.synchronize()
        assert_same(od.cpu().numpy(), oi.cpu().numpy().view(np.uint64), Dr, Ir)


# ---- what is refused ------------------------------------------------------------------------------
@gpu
def test_refusals():
    Q = data("normal")[1]
    g = make("normal", 0, "il")
    with pytest.raises(vdb.VdbError) as e:
        g.search(Q, nprobe=5, k=1025)
    assert e.value.code == -4
    assert_same(*g.search(Q, nprobe=5, k=10), *answer("normal", 0, 10, 5))
    # nprobe above nlist clamps
    assert_same(*g.search(Q, nprobe=5000, k=10), *answer("normal", 0, 10, 12))
    PQ = probe_data("normal")[1]
    gp, op = probe_pair("normal", 0)
    with pytest.raises(vdb.VdbError) as e:
        gp.search(PQ, nprobe=1025, k=10)
    assert e.value.code == -4
    assert_same(*gp.search(PQ, nprobe=10, k=10), *op.search(PQ, 10, 10))
    # the rank merges refuse k = 1025 too (before anything is read)
    import torch
    buf = torch.zeros(4096, dtype=torch.int64, device="cuda:0")  # (holds a k = 1025 record)
    for call in (lambda: vdb.merge_ranks_device(buf.data_ptr(), buf.data_ptr(), 1, 1, 1025, buf.data_ptr(),
                                                buf.data_ptr(), 0),
                 lambda: vdb.merge_ranks_packed_device(buf.data_ptr(), 1, 1, 1025, buf.data_ptr(), buf.data_ptr(), 0)):
        with pytest.raises(vdb.VdbError) as e:
            call()
        assert e.value.code == -4
