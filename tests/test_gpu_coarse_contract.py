"""GPU check of the coarse step's contract (kernels.hip: ivf_coarse_mfma, ivf_coarse_mfma2x2,
ivf_select_rerank, ivf_assign_rerank) on a snapshot of its buffers (IVFFlatIndex.coarse_snapshot),
clause by clause (coarse_ref.violations):

  1. sound: |approx - d_seq| <= delta wherever all three are finite; a pair without a finite
     bound is a candidate;
  2. the bound is the stated one, 4 (dp + 4) u (|q| + |c|)^2 + 1e-30 (|q| |c| for the inner
     product), to within (dp + 32) u: neither loosened nor shrunk;
  3. the candidates are exactly the restated set, each listed once;
  4. the probes and the assignment are the reference's;
  5. on N(0,1) data the step prunes: at most 16 candidates per query for 8 probes.

The end-to-end parity tests use data of unit scale, where the bound has about 50x of slack: a
norm from the wrong lane, a halved coefficient or a bound that grew until every list is a
candidate all return the oracle's probes there. The regimes (coarse_ref.regime) leave unit scale:
a common offset, squares under the floor, norms that overflow, norms 2^40 apart inside one tile,
and zero, NaN, inf, duplicated and 1-ulp rows.

Handles hold centroids only. nlist 333 is ragged for 16, 32, 64 and 256; the dims reach every
launch path of the 16 x 16 kernel (dp 64: G = 4, one group; 128: G = 8, one group; 192: G = 4,
three groups; 256: G = 8, two groups; 768), n = 1, 17 and 40 its ragged row tiles, n = 1041 =
32 * 32 + 17 the 2 x 2 kernel with a ragged 32-row tile."""
import functools

import numpy as np
import pytest

import coarse_ref as cr
import oracle
from conftest import load_vdb
from cosine_ref import unit_rows_ref
from test_gpu_bounded import assert_same

vdb = load_vdb()
pytestmark = pytest.mark.gpu

NLIST = 333
ROWS = (1, 17, 40)
BLOCKED = 1041
SOME = ("plain", "offset", "mixed")
DIM_REGIMES = [(d, r) for d in (64, 80, 130, 200, 768) for r in (cr.REGIMES if d in (80, 130) else SOME)]
BLOCKED_REGIMES = [(80, r) for r in cr.REGIMES] + [(768, r) for r in SOME]


@functools.lru_cache(maxsize=None)
def case(metric, dim, name, nlist=NLIST, n=ROWS[-1]):
    """(C, X, nan_rows, d_seq) of one regime: computed once, shared and never changed. Fewer rows
    are a prefix."""
    C, X, nan_rows = cr.regime(name, *cr.base(dim, nlist, n, seed=1000 * dim + nlist))
    d = cr.d_seq(metric, X, C)
    for a in (C, X, nan_rows, d):
        a.setflags(write=False)
    return C, X, nan_rows, d


def handle(metric, C):
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(C.shape[1], C.shape[0], vdb.Metric(metric)))
    g.centroids = C
    return g


def check(g, metric, C, X, nan_rows, d, n, nprobe, stats=None):
    """One snapshot of the first n rows, every clause. Returns the violations."""
    snap = g.coarse_snapshot(X[:n], nprobe=nprobe, assign=True)
    P = min(nprobe, C.shape[0])
    assert snap["approx"].shape == snap["delta"].shape == snap["cand"].shape == (n, C.shape[0])
    assert snap["probes"].shape == (n, P) and snap["assign"].shape == (n,)
    return cr.violations(metric, cr.padded_dim(C.shape[1]), X[:n], C, d[:n], snap, P, nan_rows[:n], stats)


def told(V, **where):
    """The violated clauses, one per line and in full (a list's repr would be cut short)."""
    return "\n".join([" ".join(f"{k}={v}" for k, v in where.items())] + V)


def report(what, metric, dim, name, use):
    print("coarse bound in use |approx - d_seq| / delta, worst: %s metric=%d D=%d regime=%s: %.4f" %
          (what, metric, dim, name, use))


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("dim,name", DIM_REGIMES)
def test_contract_holds(metric, dim, name):
    """The 16 x 16 kernel at every launch path and ragged row tile, 8 probes."""
    C, X, nan_rows, d = case(metric, dim, name)
    g = handle(metric, C)
    use = 0.0
    for n in ROWS:
        st = {}
        V = check(g, metric, C, X, nan_rows, d, n, 8, st)
        assert not V, told(V, n=n)
        use = max(use, st["use"])
    report("16x16", metric, dim, name, use)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("dim,name", BLOCKED_REGIMES)
def test_contract_holds_blocked(metric, dim, name):
    """The 2 x 2 register-blocked kernel (from 1024 rows) with a ragged 32-row tile."""
    C, X, nan_rows, d = case(metric, dim, name, n=BLOCKED)
    g = handle(metric, C)
    st = {}
    V = check(g, metric, C, X, nan_rows, d, BLOCKED, 8, st)
    assert not V, told(V)
    report("2x2", metric, dim, name, st["use"])


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("nprobe", [1, 8, 64, 65, 300, 333])
def test_contract_holds_at_every_probe_count(metric, nprobe):
    """One, two and eight top-P registers and P = nlist: tau is the P-th smallest of the lane minima
    up to 64 probes, of all upper bounds above."""
    for name in ("plain", "offset", "special"):
        C, X, nan_rows, d = case(metric, 80, name)
        g = handle(metric, C)
        for n in (17, 40):
            V = check(g, metric, C, X, nan_rows, d, n, nprobe)
            assert not V, told(V, regime=name, n=n)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("nlist", [1, 15])
def test_contract_holds_below_one_tile(metric, nlist):
    """Fewer centroids than one 16-centroid tile; more probes asked for than there are lists."""
    for name in SOME + ("special",):
        C, X, nan_rows, d = case(metric, 64, name, nlist=nlist, n=17)
        V = check(handle(metric, C), metric, C, X, nan_rows, d, 17, 8)
        assert not V, told(V, regime=name)


def test_contract_holds_for_cosine_distance():
    """A CosineDistance handle is the inner product over unit rows: the snapshot's rows are brought
    to unit length as a batch's queries are, so |q| = |c| = 1 to within the unit kernel's rounding
    and clause 2 pins delta to 4 (dp + 4) u + 1e-30."""
    dim = 80
    C0, X0 = cr.base(dim, NLIST, 40, seed=77)
    C, X = unit_rows_ref(C0 * np.float32(3.0)), X0 * np.float32(0.25)
    XU = unit_rows_ref(X)
    g = handle(3, C)
    snap = g.coarse_snapshot(X, nprobe=8, assign=True)
    d = cr.d_seq(cr.IP, XU, C)
    V = cr.violations(cr.IP, cr.padded_dim(dim), XU, C, d, snap, 8, None)
    assert not V, told(V)
    one = 4.0 * (cr.padded_dim(dim) + 4) * cr.U + cr.FLOOR
    assert np.abs(snap["delta"].astype(np.float64) / one - 1).max() <= (cr.padded_dim(dim) + 32) * cr.U


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("dim", [64, 80, 200, 768])
def test_it_prunes(metric, dim):
    """Clause 5: on N(0,1) data, 8 probes of 333 lists leave at most 16 candidates per query (the
    restated bound alone leaves at most 10). A bound that silently grew keeps every result exact
    and turns the step into an exact scan of the centroid table: only a count can see it."""
    C, X, nan_rows, d = case(metric, dim, "plain")
    st = {}
    V = check(handle(metric, C), metric, C, X, nan_rows, d, 40, 8, st)
    dref = cr.delta_ref(metric, cr.padded_dim(dim), X, C).astype(np.float32)
    restated = cr.cand_ref(d, dref, 8).sum(axis=1)
    print("coarse candidates per query for 8 probes of %d, worst: metric=%d D=%d: kernel %d, restated %d" %
          (NLIST, metric, dim, st["ncand"].max(), restated.max()))
    assert not V, told(V)
    worst = int(np.argmax(st["ncand"]))
    assert st["ncand"].max() <= 16, f"clause 5 (prunes): row {worst}: {st['ncand'][worst]} candidates of {NLIST}"


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("name", ["offset", "tiny", "mixed"])
def test_end_to_end_off_unit_scale(metric, name):
    """add() and search() through the coarse step on data off unit scale: the oracle's list
    membership and result bits, with the matrix-core coarse step and with the exact one."""
    dim, n, nq = 80, 3000, 64
    C, R, _ = cr.regime(name, *cr.base(dim, NLIST, n + nq, seed=5 + metric))
    X, Q = np.ascontiguousarray(R[:n]), np.ascontiguousarray(R[n:])
    ids = np.arange(n, dtype=np.uint64) * 7 + 3
    o = oracle.OracleIndex(dim, NLIST, metric)
    o.centroids = C
    o.add(X, ids)
    ref = {p: o.search(Q, p, 10) for p in (1, 8)}
    g = handle(metric, C)
    g.add(X, ids)
    want = np.array([o.list_count(l) for l in range(NLIST)], np.uint64)
    assert np.array_equal(g.list_sizes(), want), "list sizes differ from the oracle's"
    for l in np.flatnonzero(want):
        assert np.array_equal(g.get_list(int(l))[1], o.get_list(int(l))[1]), f"list {l}: other members than the oracle's"
    for mode in (1, 0):
        g.set_coarse_mode(mode)
        for p in (1, 8):
            assert_same(*g.search(Q, nprobe=p, k=10), *ref[p])


def test_handle_is_left_as_found():
    """A coarse_snapshot between two searches changes neither their bits nor the memory held:
    both are those of a twin handle that ran the same searches without the call (a search takes
    the next workspace slot and may allocate it, with or without a snapshot before it)."""
    dim, n = 80, 2000
    C, R, _ = cr.regime("plain", *cr.base(dim, NLIST, n + 40, seed=9))
    X, Q = np.ascontiguousarray(R[:n]), np.ascontiguousarray(R[n:])
    g, twin = handle(0, C), handle(0, C)
    for h in (g, twin):
        h.add(X, np.arange(n, dtype=np.uint64))
    D0, I0 = g.search(Q, nprobe=8, k=10)
    assert_same(*twin.search(Q, nprobe=8, k=10), D0, I0)
    held = g.gpu_bytes_allocated()
    assert held == twin.gpu_bytes_allocated()
    snap = g.coarse_snapshot(Q, nprobe=300, assign=True)
    assert g.gpu_bytes_allocated() == held
    assert snap["probes"].shape == (40, 300)
    # refusals that need a handle
    raw = vdb.lib().vdb_ivf_coarse_snapshot
    assert raw(g._h, Q.ctypes.data, 40, 8, None, None, None, None, None) == -1      # nprobe > 0, nowhere to put it
    assert raw(g._h, Q.ctypes.data, 40, 0, None, None, None, snap["probes"].ctypes.data, None) == -1  # nprobe 0 with probes
    assert raw(g._h, Q.ctypes.data, 500000, 0, None, None, None, None, None) == -1  # n * nlist above 2^27, no row is read
    assert raw(g._h, None, 40, 0, None, None, None, None, None) == -1               # null rows
    with pytest.raises(vdb.VdbError) as e:  # (Metric.Cosine has no matrix-core path)
        handle(2, C).coarse_snapshot(Q)
    assert e.value.code == -4
    assert g.coarse_snapshot(Q, nprobe=2000)["probes"].shape == (40, NLIST)  # (min(nprobe, nlist) is served)
    assert g.gpu_bytes_allocated() == held
    for _ in range(2):
        D1, I1 = g.search(Q, nprobe=8, k=10)
        assert_same(*twin.search(Q, nprobe=8, k=10), D1, I1)
        assert_same(D1, I1, D0, I0)
        assert g.gpu_bytes_allocated() == twin.gpu_bytes_allocated()
