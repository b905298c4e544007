"""GPU parity: the HIP engine (through the C ABI) against the CPU oracle.

Bar: ids bit-exact and distance BITS equal to the reference CPU
path's restatement (oracle/cpu_ref.cpp) on the same inputs. Configurations follow
the reference's own tests: simple_test.cpp:111-165 (D=64, nlist=16, N=1000, Q=10,
train 100, nprobe=4, k=5) and the ctest args of gpu_vs_cpu_test
(test/CMakeLists.txt:56: N=10000, Q=100, D=64, nlist=32, nprobe=8, k=10).
"""
import numpy as np
import pytest

import oracle
from conftest import load_vdb

vdb = load_vdb()
pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(D, I, Dr, Ir):
    assert I.shape == Ir.shape
    bad = np.argwhere(I != Ir)
    assert bad.size == 0, f"ids differ at {bad[:5].tolist()}: gpu {I[tuple(bad[0])]} ref {Ir[tuple(bad[0])]}"
    badd = np.argwhere(bits(D) != bits(Dr))
    assert badd.size == 0, f"dist bits differ at {badd[:5].tolist()}: gpu {D[tuple(badd[0])]!r} ref {Dr[tuple(badd[0])]!r}"


def build_pair(X, ids, dim, nlist, metric=0, train=None):
    """Train+add on both the GPU engine and the oracle; returns (gpu, oracle)."""
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, nlist, vdb.Metric(metric)))
    o = oracle.OracleIndex(dim, nlist, metric)
    T = X if train is None else train
    g.train(T)
    o.train(T)
    g.add(X, ids)
    o.add(X, ids)
    return g, o


def mirror_from_oracle(o, dim, nlist, metric=0):
    """GPU index with the oracle's centroids and the same add() input order."""
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, nlist, vdb.Metric(metric)))
    g.centroids = o.centroids
    return g


def test_simple_test_config():
    # simple_test.cpp:111-165: mt19937(42) database then queries.
    flat = oracle.gen_normal(42, (1000 + 10) * 64)
    X, Q = flat[:64000].reshape(1000, 64), flat[64000:].reshape(10, 64)
    ids = np.arange(1000, dtype=np.uint64)
    g, o = build_pair(X, ids, 64, 16, train=X[:100])
    assert np.array_equal(bits(g.centroids), bits(o.centroids)), "train() centroids differ"
    for l in range(16):
        gv, gi = g.get_list(l)
        ov, oi = o.get_list(l)
        assert np.array_equal(gi, oi), f"list {l} membership/order differs"
        assert np.array_equal(bits(gv), bits(ov))
    D, I = g.search(Q, nprobe=4, k=5)
    Dr, Ir = o.search(Q, 4, 5)
    assert_same(D, I, Dr, Ir)
    # validity rules of simple_test.cpp:186 / gpu_vs_cpu_test.cpp:209-219
    assert np.all((I < 1000) | (I == np.iinfo(np.uint64).max))
    assert g.get_total_vectors() == 1000


def test_gpu_vs_cpu_ctest_config():
    X, Q, ids = oracle.reference_test_data(10000, 100, 64)
    g, o = build_pair(X, ids, 64, 32)
    assert np.array_equal(bits(g.centroids), bits(o.centroids))
    D, I = g.search(Q, nprobe=8, k=10)
    Dr, Ir = o.search(Q, 8, 10)
    assert_same(D, I, Dr, Ir)
    assert np.all(np.isfinite(D)) and np.all(D >= 0)


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_metrics_given_centroids(metric):
    X, Q, ids = oracle.reference_test_data(6000, 50, 32, seed=7)
    o = oracle.OracleIndex(32, 24, metric)
    o.centroids = X[::250][:24]
    o.add(X, ids)
    g = mirror_from_oracle(o, 32, 24, metric)
    g.add(X, ids)
    for l in range(24):
        assert np.array_equal(g.get_list(l)[1], o.get_list(l)[1]), f"assignment differs for list {l}"
    D, I = g.search(Q, nprobe=5, k=10)
    Dr, Ir = o.search(Q, 5, 10)
    assert_same(D, I, Dr, Ir)


def test_train_inner_product():
    X, Q, ids = oracle.reference_test_data(3000, 20, 16, seed=3)
    g, o = build_pair(X, ids, 16, 12, metric=1)
    assert np.array_equal(bits(g.centroids), bits(o.centroids))
    assert_same(*g.search(Q, nprobe=3, k=7), *o.search(Q, 3, 7))


@pytest.mark.parametrize("dim", [1, 3, 67, 130])
def test_odd_dimensions(dim):
    X, Q, ids = oracle.reference_test_data(2500, 30, dim, seed=dim)
    g, o = build_pair(X, ids, dim, 10, train=X[:500])
    assert np.array_equal(bits(g.centroids), bits(o.centroids))
    assert_same(*g.search(Q, nprobe=3, k=10), *o.search(Q, 3, 10))


@pytest.mark.parametrize("k", [1, 64, 65, 100, 1000])
def test_k_range(k):
    X, Q, ids = oracle.reference_test_data(5000, 20, 24, seed=11)
    o = oracle.OracleIndex(24, 8, 0)
    o.centroids = X[:8]
    o.add(X, ids)
    g = mirror_from_oracle(o, 24, 8)
    g.add(X, ids)
    assert_same(*g.search(Q, nprobe=3, k=k), *o.search(Q, 3, k))


def test_bruteforce_nprobe_equals_nlist():
    X, Q, ids = oracle.reference_test_data(4000, 25, 20, seed=5)
    o = oracle.OracleIndex(20, 128, 0)
    o.centroids = X[:128]
    o.add(X, ids)
    g = mirror_from_oracle(o, 20, 128)
    g.add(X, ids)
    D, I = g.search(Q, nprobe=128, k=10)
    assert_same(D, I, *o.search(Q, 128, 10))
    # nprobe = nlist is exact brute force under (dist, id) order
    import oracle.np_ref as npr
    full = npr.distances(0, Q, X)
    for q in range(Q.shape[0]):
        order = np.lexsort((ids, full[q]))[:10]
        assert np.array_equal(I[q], ids[order])


def test_nprobe_above_nlist_clamps():
    X, Q, ids = oracle.reference_test_data(2000, 10, 8, seed=9)
    o = oracle.OracleIndex(8, 6, 0)
    o.centroids = X[:6]
    o.add(X, ids)
    g = mirror_from_oracle(o, 8, 6)
    g.add(X, ids)
    assert_same(*g.search(Q, nprobe=50, k=5), *o.search(Q, 50, 5))


def test_empty_lists_stale_slots():
    """Reference quirk A1: an empty probed list leaves the previous query's slot."""
    rng = np.random.default_rng(0)
    X = rng.standard_normal((3000, 16)).astype(np.float32)
    Q = rng.standard_normal((300, 16)).astype(np.float32)
    ids = np.arange(3000, dtype=np.uint64)
    C = np.concatenate([X[:10], 6.0 + rng.standard_normal((6, 16)).astype(np.float32) * 0.1])
    C[10:] *= np.where(rng.random((6, 1)) < 0.5, -1, 1).astype(np.float32)
    o = oracle.OracleIndex(16, 16, 0)
    o.centroids = C
    o.add(X, ids)
    assert any(o.list_count(l) == 0 for l in range(16)), "fixture must contain empty lists"
    g = mirror_from_oracle(o, 16, 16)
    g.add(X, ids)
    for batch in (7, 64, 256):          # carry across internal batches of one call
        g.set_batch(batch)
        assert_same(*g.search(Q, nprobe=12, k=8), *o.search(Q, 12, 8))
    # with stale slots disabled, empty lists contribute nothing: compare with numpy
    # restatement after dropping the stale behaviour isn't defined by the reference,
    # so only check validity here.
    g.set_stale_slots(False)
    D, I = g.search(Q, nprobe=12, k=8)
    assert np.all(np.diff(D, axis=1) >= 0)


def test_duplicate_ids_and_vectors():
    rng = np.random.default_rng(1)
    base = rng.standard_normal((500, 12)).astype(np.float32)
    X = np.concatenate([base, base[:200], base[100:300]])            # exact duplicate vectors
    ids = np.concatenate([np.arange(500), np.arange(200), np.arange(1000, 1200)]).astype(np.uint64)  # dup ids
    Q = np.concatenate([base[:20], rng.standard_normal((20, 12)).astype(np.float32)])
    o = oracle.OracleIndex(12, 5, 0)
    o.centroids = base[:5]
    o.add(X, ids)
    g = mirror_from_oracle(o, 12, 5)
    g.add(X, ids)
    for k in (1, 5, 30):
        assert_same(*g.search(Q, nprobe=2, k=k), *o.search(Q, 2, k))


def test_incremental_add():
    X, Q, ids = oracle.reference_test_data(3000, 20, 16, seed=21)
    o = oracle.OracleIndex(16, 10, 0)
    o.centroids = X[:10]
    g = mirror_from_oracle(o, 16, 10)
    for a, b in ((0, 1000), (1000, 1001), (1001, 3000)):
        o.add(X[a:b], ids[a:b])
        g.add(X[a:b], ids[a:b])
    for l in range(10):
        assert np.array_equal(g.get_list(l)[1], o.get_list(l)[1])
    assert_same(*g.search(Q, nprobe=4, k=10), *o.search(Q, 4, 10))


def test_benchmark_kat_self_query():
    """bench/benchmark.cpp:130-138 re-seeds mt19937(42) for queries, so query i == vector i:
    the top-1 must be (i, 0.0f) for every i < N (known answer)."""
    n, d = 1000, 64
    X = oracle.gen_normal(42, n * d).reshape(n, d)
    Q = oracle.gen_normal(42, 50 * d).reshape(50, d)
    ids = np.arange(n, dtype=np.uint64)
    g, o = build_pair(X, ids, d, 32)
    D, I = g.search(Q, nprobe=5, k=10)
    assert np.array_equal(I[:, 0], np.arange(50, dtype=np.uint64))
    assert np.all(bits(D[:, 0]) == 0)
    assert_same(D, I, *o.search(Q, 5, 10))


def test_empty_index_and_degenerate_calls():
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(8, 4))
    Q = np.ones((3, 8), np.float32)
    D, I = g.search(Q, nprobe=2, k=4)
    assert np.all(I == np.iinfo(np.uint64).max) and np.all(D == np.finfo(np.float32).max)
    D, I = g.search(Q, nprobe=0, k=4)
    assert np.all(I == np.iinfo(np.uint64).max)
    D, I = g.search(np.zeros((0, 8), np.float32), nprobe=2, k=4)
    assert D.shape == (0, 4)
    with pytest.raises(ValueError):
        vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(0, 4))


def test_two_shards_merge_equals_single():
    import torch
    X, Q, ids = oracle.reference_test_data(8000, 40, 32, seed=4)
    o = oracle.OracleIndex(32, 20, 0)
    o.centroids = X[:20]
    o.add(X, ids)
    Dr, Ir = o.search(Q, 6, 10)
    parts_d, parts_i = [], []
    for r in range(2):
        g = mirror_from_oracle(o, 32, 20)
        g.add(X, ids)
        g.set_shard(r, 2)
        D, I = g.search(Q, nprobe=6, k=10)
        parts_d.append(D)
        parts_i.append(I)
        owner = vdb.shard_plan(g.list_sizes(), 2)
        Do, Io = o.search_shard(Q, 6, 10, (owner == r).astype(np.uint8))
        assert_same(D, I, Do, Io)
    dev = torch.device("cuda:0")
    pd = torch.from_numpy(np.stack(parts_d)).to(dev)
    pi = torch.from_numpy(np.stack(parts_i).view(np.int64)).to(dev)
    od = torch.empty((40, 10), dtype=torch.float32, device=dev)
    oi = torch.empty((40, 10), dtype=torch.int64, device=dev)
    vdb.merge_ranks_device(pd.data_ptr(), pi.data_ptr(), 2, 40, 10, od.data_ptr(), oi.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert_same(od.cpu().numpy(), oi.cpu().numpy().view(np.uint64), Dr, Ir)
    # the packed-record form bench.py gathers with one collective per batch
    rec, off = vdb.rank_record_bytes(40, 10), vdb.rank_record_ids_offset(40, 10)
    recs = np.zeros((2, rec), np.uint8)
    for r in range(2):
        recs[r, :parts_d[r].nbytes] = parts_d[r].view(np.uint8).ravel()
        recs[r, off:off + parts_i[r].nbytes] = parts_i[r].view(np.uint8).ravel()
    rd = torch.from_numpy(recs.ravel()).to(dev)
    vdb.merge_ranks_packed_device(rd.data_ptr(), 2, 40, 10, od.data_ptr(), oi.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert_same(od.cpu().numpy(), oi.cpu().numpy().view(np.uint64), Dr, Ir)


def test_sharded_build_equals_single():
    """cfg4 flow (an index larger than one GPU): assign pass -> final sizes -> plan_shard ->
    add_to_lists in chunks; each rank holds only its lists, the merge equals the oracle."""
    import torch
    dev = torch.device("cuda:0")
    X, Q, ids = oracle.reference_test_data(9000, 40, 48, seed=6)
    o = oracle.OracleIndex(48, 24, 0)
    o.train(X[:3000])
    o.add(X, ids)
    Dr, Ir = o.search(Q, 7, 10)
    Xd = torch.from_numpy(X).to(dev)
    idd = torch.from_numpy(ids.view(np.int64)).to(dev)
    chunks = [(0, 4000), (4000, 4001), (4001, 9000)]
    world, parts = 3, []
    for r in range(world):
        g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(48, 24, vdb.Metric.L2))
        g.train(X[:3000])
        asg = torch.empty(9000, dtype=torch.int32, device=dev)
        for a, b in chunks:  # pass 1: assignment only
            g.assign_device(Xd[a:].data_ptr(), b - a, asg[a:].data_ptr())
        torch.cuda.synchronize()
        sizes = np.bincount(asg.cpu().numpy(), minlength=24).astype(np.uint64)
        assert np.array_equal(sizes, np.array([len(o.get_list(l)[1]) for l in range(24)], np.uint64))
        g.plan_shard(r, world, sizes)
        for a, b in chunks:  # pass 2: store this rank's lists only
            g.add_to_lists_device(Xd[a:].data_ptr(), idd[a:].data_ptr(), asg[a:].data_ptr(), b - a)
        assert np.array_equal(g.list_sizes(), sizes) and g.get_total_vectors() == 9000
        owner = vdb.shard_plan(sizes, world)
        for l in range(24):
            if owner[l] == r and sizes[l]:
                gv, gi = g.get_list(l)
                ov, oi = o.get_list(l)
                assert np.array_equal(gi, oi) and np.array_equal(bits(gv), bits(ov))
        D, I = g.search(Q, nprobe=7, k=10)
        Do, Io = o.search_shard(Q, 7, 10, (owner == r).astype(np.uint8))
        assert_same(D, I, Do, Io)
        parts.append((D, I))
        with pytest.raises(vdb.VdbError):
            g.plan_shard(r, world, sizes)  # only on an empty index
    pd = torch.from_numpy(np.stack([p[0] for p in parts])).to(dev)
    pi = torch.from_numpy(np.stack([p[1] for p in parts]).view(np.int64)).to(dev)
    od = torch.empty((40, 10), dtype=torch.float32, device=dev)
    oi = torch.empty((40, 10), dtype=torch.int64, device=dev)
    vdb.merge_ranks_device(pd.data_ptr(), pi.data_ptr(), world, 40, 10, od.data_ptr(), oi.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert_same(od.cpu().numpy(), oi.cpu().numpy().view(np.uint64), Dr, Ir)


@pytest.mark.parametrize("seg", [0, 64, 512])
@pytest.mark.parametrize("k", [10, 64, 65])
def test_hub_lists_wide_items(k, seg):
    """Skewed lists probed by every query of the batch: wide scan items (groups of
    8 queries), XCD-alignment padding items and two-level partial merges."""
    rng = np.random.default_rng(7)
    X = rng.standard_normal((40000, 48)).astype(np.float32)
    Q = rng.standard_normal((130, 48)).astype(np.float32)
    ids = rng.permutation(40000).astype(np.uint64)
    C = np.zeros((6, 48), np.float32)                     # centroid 0 at the origin takes most vectors
    C[1:] = 3.0 * rng.standard_normal((5, 48)).astype(np.float32)
    o = oracle.OracleIndex(48, 6, 0)
    o.centroids = C
    o.add(X, ids)
    assert max(o.list_count(l) for l in range(6)) > 32 * 512, "need > kMergeFan segments in one list"
    g = mirror_from_oracle(o, 48, 6)
    g.add(X, ids)
    g.set_option("seg_vectors", seg)   # segment size never changes results
    for batch in (64, 130):
        g.set_batch(batch)
        for wg, stride, spi, fused in ((16, 40009, 0, 1), (16, 1, 4, 0), (16, 7, 12, 1),  # item shape /
                                       (32, 1, 0, 1), (32, 40009, 4, 0), (32, 7, 12, 1)):  # dispatch order /
            g.set_option("wide_group", wg)                                 # fused narrow+wide grid never
            g.set_option("wide_stride", stride)                            # change results
            g.set_option("segs_per_item", spi)
            g.set_option("fused_scan", fused)
            assert_same(*g.search(Q, nprobe=3, k=k), *o.search(Q, 3, k))
    g.set_option("wide_group", 16)


def test_launches_beyond_2_32_workitems():
    """HSA grid sizes are 32-bit in work-items: element-wise launchers must stride.
    (10M x 768 = 7.7e9 floats once left the tail of the synthetic data unwritten.)"""
    import torch
    n = (1 << 32) + 4096
    dev = torch.device("cuda:0")
    buf = torch.zeros(n, dtype=torch.float32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    vdb.gen_normal_device(buf.data_ptr(), n, seed=5, offset=0, stream=s)
    tail = torch.empty(4096, dtype=torch.float32, device=dev)
    vdb.gen_normal_device(tail.data_ptr(), 4096, seed=5, offset=n - 4096, stream=s)
    torch.cuda.synchronize()
    assert torch.equal(buf[-4096:], tail)
    assert int((buf[-(1 << 20):] == 0).sum()) < 16
    del buf
    torch.cuda.empty_cache()


GOLDEN_DIR = __import__("os").path.join(__import__("os").path.dirname(__file__), "golden")


@pytest.mark.parametrize("name", ["simple_test", "gpu_vs_cpu_ctest", "benchmark_small", "inner_product",
                                  "empty_lists_dups"])
def test_golden_fixture_on_gpu(name):
    import os
    from golden_data import load_golden
    f = load_golden(os.path.join(GOLDEN_DIR, name + ".npz"))
    dim, nlist, train_n, nprobe, k, metric = (int(x) for x in f["params"])
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, nlist, vdb.Metric(metric)))
    if train_n:
        g.train(f["X"][:train_n])
        assert np.array_equal(bits(g.centroids), bits(f["centroids"]))
    else:
        g.centroids = f["centroids"]
    g.add(f["X"], f["ids"])
    assert np.array_equal(g.list_sizes(), f["list_sizes"])
    assert_same(*g.search(f["Q"], nprobe=nprobe, k=k), f["D"], f["I"])


def test_save_load_round_trip(tmp_path):
    X, Q, ids = oracle.reference_test_data(4000, 30, 40, seed=31)
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(40, 12))
    g.train(X[:1000])
    g.add(X, ids)
    D, I = g.search(Q, nprobe=4, k=10)
    lib = vdb.lib()
    path = str(tmp_path / "idx.ivf").encode()
    import ctypes
    lib.vdb_ivf_save.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    lib.vdb_ivf_load.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    assert lib.vdb_ivf_save(g._h, path) == 0
    h = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(40, 12))
    assert lib.vdb_ivf_load(h._h, path) == 0
    assert np.array_equal(h.list_sizes(), g.list_sizes())
    assert_same(*h.search(Q, nprobe=4, k=10), D, I)


def test_concurrent_streams_match_sequential():
    """Batches issued alternately on two streams (two in flight, each in its own
    engine workspace slot, hub lists included) equal the oracle bit for bit."""
    import torch
    rng = np.random.default_rng(11)
    X = rng.standard_normal((30000, 64)).astype(np.float32)
    Q = rng.standard_normal((8 * 64, 64)).astype(np.float32)
    ids = np.arange(30000, dtype=np.uint64)
    C = np.zeros((12, 64), np.float32)
    C[1:] = 2.5 * rng.standard_normal((11, 64)).astype(np.float32)
    o = oracle.OracleIndex(64, 12, 0)
    o.centroids = C
    o.add(X, ids)
    g = mirror_from_oracle(o, 64, 12)
    g.add(X, ids)
    dev = torch.device("cuda:0")
    qd = torch.from_numpy(Q).to(dev)
    od = torch.empty((len(Q), 10), dtype=torch.float32, device=dev)
    oi = torch.empty((len(Q), 10), dtype=torch.int64, device=dev)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    torch.cuda.synchronize()
    for b in range(8):
        s = streams[b % 2]
        g.search_device(qd[b * 64:].data_ptr(), 64, 4, 10, od[b * 64:].data_ptr(), oi[b * 64:].data_ptr(),
                        s.cuda_stream)
    torch.cuda.synchronize()
    Dr = np.concatenate([o.search(Q[b * 64:(b + 1) * 64], 4, 10)[0] for b in range(8)])
    Ir = np.concatenate([o.search(Q[b * 64:(b + 1) * 64], 4, 10)[1] for b in range(8)])
    assert_same(od.cpu().numpy(), oi.cpu().numpy().view(np.uint64), Dr, Ir)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("nprobe", [1, 7, 64, 100, 300])
def test_mfma_coarse_selects_exact_probe_sets(metric, nprobe):
    """The MFMA coarse step (distance bounds + exact re-rank) must pick the same
    probe lists as the reference's sequential distances (select_nprobe_lists,
    ivf_flat_index.cpp:298-336), including P > 64 and P = nlist."""
    rng = np.random.default_rng(100 + nprobe)
    dim, nlist = 96, 300
    X = rng.standard_normal((20000, dim)).astype(np.float32)
    Q = rng.standard_normal((70, dim)).astype(np.float32)
    ids = np.arange(len(X), dtype=np.uint64)
    o = oracle.OracleIndex(dim, nlist, metric)
    o.centroids = X[:nlist] * 0.3
    o.add(X, ids)
    for mode in (1, 0):
        g = mirror_from_oracle(o, dim, nlist, metric)
        g.set_coarse_mode(mode)
        g.add(X, ids)
        assert_same(*g.search(Q, nprobe=nprobe, k=10), *o.search(Q, nprobe, 10))


def test_mfma_coarse_near_ties():
    """Centroids one ulp apart and exact duplicates: the approximate order differs
    from the exact one; the re-rank must restore (dist, list_id) order exactly."""
    rng = np.random.default_rng(5)
    dim, nlist = 64, 256
    base = rng.standard_normal((32, dim)).astype(np.float32)
    C = np.repeat(base, 8, axis=0)
    bump = rng.integers(-2, 3, size=C.shape).astype(np.int32)
    C = (C.view(np.int32) + bump * (np.arange(len(C)) % 8 != 0)[:, None]).view(np.float32)  # ulp jitter, 1 exact copy
    C[1::8] = C[0::8]                                                                       # exact duplicates
    X = rng.standard_normal((8000, dim)).astype(np.float32)
    Q = np.concatenate([base + 1e-3 * rng.standard_normal(base.shape).astype(np.float32),
                        rng.standard_normal((32, dim)).astype(np.float32)])
    ids = np.arange(len(X), dtype=np.uint64)
    o = oracle.OracleIndex(dim, nlist, 0)
    o.centroids = C
    o.add(X, ids)
    for nprobe in (3, 8, 20):
        probes_ref = np.stack([o.select_nprobe(q, nprobe) for q in Q])
        g = mirror_from_oracle(o, dim, nlist)
        g.add(X, ids)
        assert_same(*g.search(Q, nprobe=nprobe, k=10), *o.search(Q, nprobe, 10))
        assert probes_ref.shape == (len(Q), nprobe)


@pytest.mark.parametrize("metric", [0, 1])
def test_blocked_mfma_bounds_large_batches(metric):
    """From 1024 rows the coarse bounds come from the 2x2 register-blocked MFMA kernel:
    a search batch of 1500 queries and an add() of near-tie rows (centroid copies with
    ulp jitter, ragged 32-row / 32-centroid tiles) must still give the reference's
    probe sets and argmin (ties to the lowest centroid)."""
    rng = np.random.default_rng(17 + metric)
    dim, nlist = 80, 333                               # dp 128, nlist not a multiple of 32
    base = rng.standard_normal((111, dim)).astype(np.float32)
    C = np.repeat(base, 3, axis=0)
    C[1::3] = (C[1::3].view(np.int32) + rng.integers(-1, 2, size=C[1::3].shape).astype(np.int32)).view(np.float32)
    X = np.concatenate([np.repeat(C, 5, axis=0),                       # exact copies: distance 0 ties
                        rng.standard_normal((3001, dim)).astype(np.float32)])
    ids = rng.permutation(len(X)).astype(np.uint64)
    Q = np.concatenate([C[rng.integers(0, nlist, 700)] + 1e-4 * rng.standard_normal((700, dim)).astype(np.float32),
                        rng.standard_normal((800, dim)).astype(np.float32)])
    o = oracle.OracleIndex(dim, nlist, metric)
    o.centroids = C
    o.add(X, ids)
    g = mirror_from_oracle(o, dim, nlist, metric)
    g.add(X, ids)
    for l in range(nlist):
        assert np.array_equal(g.get_list(l)[1], o.get_list(l)[1]), f"list {l} membership differs"
    g.set_batch(4096)                                  # one internal batch of 1500 rows
    for nprobe in (1, 5):
        assert_same(*g.search(Q, nprobe=nprobe, k=10), *o.search(Q, nprobe, 10, threads=16))


def test_nan_query_is_contained():
    """A NaN query must not make the engine read outside its lists (no crash), and
    the other queries of the batch keep their exact results."""
    X, Q, ids = oracle.reference_test_data(3000, 12, 16, seed=8)
    o = oracle.OracleIndex(16, 10, 0)
    o.centroids = X[:10]
    o.add(X, ids)
    g = mirror_from_oracle(o, 16, 10)
    g.add(X, ids)
    Qn = Q.copy()
    Qn[3, 5] = np.nan
    for mode in (1, 0):
        g.set_coarse_mode(mode)
        D, I = g.search(Qn, nprobe=4, k=5)
        keep = np.arange(len(Q)) > 3          # rows after the NaN row (rows before it are unaffected too)
        Dr, Ir = o.search(Q[keep], 4, 5)
        assert_same(D[keep], I[keep], Dr, Ir)


def test_coalesced_concurrent_calls_keep_per_call_semantics():
    """Concurrent host-API search() calls are coalesced into shared device batches; every
    call must still get exactly what the reference gives that call alone — including the
    per-call stale-slot behaviour of empty lists (cpp:210-233), which must not leak
    between coalesced calls."""
    import threading
    rng = np.random.default_rng(3)
    X = rng.standard_normal((3000, 16)).astype(np.float32)
    ids = np.arange(3000, dtype=np.uint64)
    C = np.concatenate([X[:10], 6.0 + rng.standard_normal((6, 16)).astype(np.float32) * 0.1])
    C[10:] *= np.where(rng.random((6, 1)) < 0.5, -1, 1).astype(np.float32)
    o = oracle.OracleIndex(16, 16, 0)
    o.centroids = C
    o.add(X, ids)
    assert any(o.list_count(l) == 0 for l in range(16))
    g = mirror_from_oracle(o, 16, 16)
    g.add(X, ids)
    g.set_batch(7)                      # internal batches cut across coalesced calls too
    calls = []
    for t in range(12):
        for c in range(6):
            n = int(rng.integers(1, 20))
            nprobe, k = (12, 8) if (t + c) % 3 else (5, 3)
            calls.append((rng.standard_normal((n, 16)).astype(np.float32), nprobe, k))
    results = [None] * len(calls)
    errors = []

    def worker(t):
        try:
            for j in range(t, len(calls), 12):
                Q, nprobe, k = calls[j]
                results[j] = g.search(Q, nprobe=nprobe, k=k)
        except Exception as e:  # pragma: no cover - reported below
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(12)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for (Q, nprobe, k), (D, I) in zip(calls, results):
        assert_same(D, I, *o.search(Q, nprobe, k))
    batches, served = g.coalesce_stats()
    assert served == len(calls)
    assert batches <= served
