"""GPU: train() and add() against the oracle at the build kernels' edges.

The search path is compared with the oracle stage by stage elsewhere; this file does the same
for the build path that decides what sits in the lists: the k-means++ min-distance kernel, the
Lloyd assignment (both MFMA bound kernels and the exact ivf_assign), the stable radix grouping
and lloyd_update. The training sets (tests/train_fixtures.py; their properties are asserted on
the CPU in test_train_fixtures.py) reach radix keys wider than 8 bits, empty clusters, repeated
seeds, fewer rows than lists, one row, 63 / 64 / 65 rows, sums whose low bits depend on their
order, and one cluster holding almost every row. The Lloyd sum is s = s + v in input order over
fp32, so the final centroid bits change with almost any mistake in order, membership or seeds:
every comparison here is bit-exact (view(np.uint32)), there are no tolerances.
"""
import numpy as np
import pytest

import oracle
import train_fixtures as tf
from conftest import load_vdb
from cosine_ref import cos_map, unit_rows_ref

vdb = load_vdb()
pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, ref):
    (D, I), (Dr, Ir) = got, ref
    assert D.shape == Dr.shape and I.shape == Ir.shape
    bad = np.argwhere(I != Ir)
    assert bad.size == 0, f"ids differ at {bad[:5].tolist()}: gpu {I[tuple(bad[0])]} ref {Ir[tuple(bad[0])]}"
    badd = np.argwhere(bits(D) != bits(Dr))
    assert badd.size == 0, f"dist bits differ at {badd[:5].tolist()}: gpu {D[tuple(badd[0])]!r} ref {Dr[tuple(badd[0])]!r}"


def handle(dim, nlist, metric=0, coarse_mode=1, **cfg):
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, nlist, vdb.Metric(metric), **cfg))
    g.set_coarse_mode(coarse_mode)
    return g


def assert_centroids(name, C, what="train()"):
    """C against the oracle's centroids for the set; the message names the first differing
    centroid, its member count in the oracle's last assignment and whether it is empty there."""
    Cr = tf.oracle_centroids(name)
    assert C.shape == Cr.shape
    bad = np.flatnonzero((bits(C) != bits(Cr)).any(axis=1))
    if bad.size:
        c = int(bad[0])
        cnt = int(tf.last_counts(name)[c])
        d = int(np.flatnonzero(bits(C[c]) != bits(Cr[c]))[0])
        raise AssertionError(
            f"{name}: {what} centroids differ from the oracle's in {bad.size} of {len(Cr)} centroids; first: "
            f"centroid {c}, {cnt} members in the oracle's last assignment"
            f" ({'an empty cluster, it keeps its seed' if cnt == 0 else 'not empty'}), element {d}: "
            f"gpu {C[c, d]!r} oracle {Cr[c, d]!r}")


def assert_lists(g, o, nlist, lists=None):
    """Every list's ids and vector bits in append order."""
    sizes = g.list_sizes()
    ref = np.array([o.list_count(l) for l in range(nlist)], np.uint64)
    bad = np.flatnonzero(sizes != ref)
    assert bad.size == 0, f"list sizes differ at {bad[:5].tolist()}: gpu {sizes[bad[:5]].tolist()} ref {ref[bad[:5]].tolist()}"
    for l in (range(nlist) if lists is None else lists):
        if ref[l] == 0:
            continue
        (gv, gi), (ov, oi) = g.get_list(l), o.get_list(l)
        assert np.array_equal(gi, oi), f"list {l}: membership or append order differs"
        assert np.array_equal(bits(gv), bits(ov)), f"list {l}: vector bits differ"


def queries(name):
    """The set's first 20 rows and 10 fresh rows about the set's mean."""
    X, dim, nlist, metric = tf.training_set(name)
    rng = np.random.default_rng(1000 + tf.SETS[name][0])
    fresh = (X.mean(axis=0, dtype=np.float64) + rng.standard_normal((10, dim))).astype(np.float32)
    return np.concatenate([X[:min(len(X), 20)], fresh])


@pytest.mark.parametrize("coarse_mode", [1, 0])
@pytest.mark.parametrize("name", tf.NAMES)
def test_train_matches_oracle(name, coarse_mode):
    X, dim, nlist, metric = tf.training_set(name)
    o, ids = tf.oracle_index(name), tf.set_ids(name)
    g = handle(dim, nlist, metric, coarse_mode)
    g.train(X)
    assert_centroids(name, g.centroids)
    g.add(X, ids)
    assert g.get_total_vectors() == len(X)
    assert_lists(g, o, nlist)
    # empty lists among the probes leave stale slots (the reference's quirk, kept)
    nprobe = min(nlist, 8)
    assert_same(g.search(queries(name), nprobe=nprobe, k=5), o.search(queries(name), nprobe, 5))


@pytest.mark.parametrize("name", tf.NAMES)
def test_assignment_stage_alone(name):
    """The oracle's final centroids loaded into a fresh handle: assign_device over the set's rows
    is the oracle's assign. A failure of test_train_matches_oracle with this one passing lies in
    the seeding, the grouping or the update, not in the assignment."""
    import torch
    X, dim, nlist, metric = tf.training_set(name)
    o = tf.oracle_index(name)
    ref = o.assign(X)
    dev = torch.device("cuda:0")
    Xd = torch.from_numpy(np.array(X)).to(dev)
    for coarse_mode in (1, 0):
        g = handle(dim, nlist, metric, coarse_mode)
        g.centroids = tf.oracle_centroids(name)
        out = torch.full((len(X),), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        g.assign_device(Xd.data_ptr(), len(X), out.data_ptr())
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        bad = np.flatnonzero(got != ref)
        assert bad.size == 0, (f"{name}, coarse_mode {coarse_mode}: {bad.size} rows assigned differently; first row "
                               f"{int(bad[0])}: gpu {int(got[bad[0]])} oracle {int(ref[bad[0]])}")


@pytest.mark.parametrize("name", ["ragged_65", "wide_keys_small"])
def test_train_device_equals_host(name):
    import torch
    X, dim, nlist, metric = tf.training_set(name)
    g = handle(dim, nlist, metric)
    g.train(X)
    Xd = torch.from_numpy(np.array(X)).to(torch.device("cuda:0"))
    torch.cuda.synchronize()
    h = handle(dim, nlist, metric)
    h.train_device(Xd.data_ptr(), len(X))
    torch.cuda.synchronize()
    assert np.array_equal(bits(h.centroids), bits(g.centroids))
    assert np.array_equal(bits(Xd.cpu().numpy()), bits(X))  # the caller's rows are only read
    assert_centroids(name, h.centroids, "train_device()")


def test_second_train_replaces_the_first():
    """train() on hub, then on ragged_63b (the same dim, nlist and metric): nothing of the first
    training is left, the centroids are those of a fresh handle trained on the second set."""
    (A, dim, nlist, metric), B = tf.training_set("hub"), tf.training_set("ragged_63b")[0]
    g = handle(dim, nlist, metric)
    g.train(A)
    assert_centroids("hub", g.centroids)
    g.train(B)
    fresh = handle(dim, nlist, metric)
    fresh.train(B)
    assert np.array_equal(bits(g.centroids), bits(fresh.centroids))
    assert_centroids("ragged_63b", g.centroids, "the second train()")


def test_train_after_add():
    """train(A), add(A), search, train(B), search again, on both sides. The reference's train
    writes the centroids only: the lists keep A's membership under B's centroids, and the probes
    follow B's centroids. k = 5 takes the screened scan (its shadow holds residuals against the
    centroids and must be rebuilt), k = 100 the exact scan."""
    (A, dim, nlist, metric), B = tf.training_set("hub"), tf.training_set("ragged_63b")[0]
    ids = tf.set_ids("hub")
    Q = np.concatenate([queries("hub"), queries("ragged_63b")])
    o = oracle.OracleIndex(dim, nlist, metric)
    g = handle(dim, nlist, metric)
    o.train(A)
    g.train(A)
    assert np.array_equal(bits(o.centroids), bits(tf.oracle_centroids("hub")))
    o.add(A, ids)
    g.add(A, ids)
    for k in (5, 100):
        assert_same(g.search(Q, nprobe=8, k=k), o.search(Q, 8, k))
    before = [g.get_list(l) for l in range(nlist)]
    o.train(B)
    g.train(B)
    assert np.array_equal(bits(o.centroids), bits(tf.oracle_centroids("ragged_63b")))
    assert_centroids("ragged_63b", g.centroids, "train() after add()")
    assert g.get_total_vectors() == len(A)
    assert_lists(g, o, nlist)
    for l, (v, i) in enumerate(before):  # A's membership, untouched
        gv, gi = g.get_list(l)
        assert np.array_equal(gi, i) and np.array_equal(bits(gv), bits(v)), f"list {l} changed"
    for k in (5, 100):
        assert_same(g.search(Q, nprobe=8, k=k), o.search(Q, 8, k))
    for nprobe in (1, 3):  # the probes are B's: few lists, chosen by the new centroids
        assert_same(g.search(Q, nprobe=nprobe, k=5), o.search(Q, nprobe, 5))


@pytest.mark.parametrize("name", ["duplicates", "fewer_rows_than_lists"])
def test_group_train_edges(name):
    """A 2-member group on one device (as test_gpu_multi.py builds it): train on the group, then
    add: empty clusters and repeated seeds give the oracle's centroids, lists and results."""
    X, dim, nlist, metric = tf.training_set(name)
    o, ids = tf.oracle_index(name), tf.set_ids(name)
    g = handle(dim, nlist, metric, devices=(0, 0))
    assert g.group_size == 2
    g.train(X)
    assert_centroids(name, g.centroids, "train() on a 2-member group")
    g.add(X, ids)
    assert_lists(g, o, nlist)
    assert_same(g.search(queries(name), nprobe=8, k=5), o.search(queries(name), 8, 5))


def _zeroed_duplicates():
    """duplicates with every copy of its first row set to zero: a zero row among the seeds."""
    X = np.array(tf.training_set("duplicates")[0])
    X[(bits(X) == bits(X[0])).all(axis=1)] = 0.0
    return X


@pytest.mark.parametrize("name", ["duplicates", "one_row", "duplicates_zero_row"])
def test_cosine_distance_train_edges(name):
    """Metric.CosineDistance against the restatement of test_gpu_cosine.py::test_train_and_add: an
    InnerProduct handle trained on the unit rows, its centroids brought to unit length
    (cosine_ref.unit_rows_ref), and beside it the oracle's inner-product train on the same unit
    rows. Repeated seeds stay bit-equal after the normalisation; a zero centroid stays zero
    (duplicates_zero_row: duplicates with one of its 50 distinct rows zeroed)."""
    X, dim, nlist, _ = tf.training_set("duplicates" if name == "duplicates_zero_row" else name)
    if name == "duplicates_zero_row":
        X = _zeroed_duplicates()
        assert int((X == 0).all(axis=1).sum()) == 30
    XU = unit_rows_ref(X)
    ids = np.arange(len(X), dtype=np.uint64)
    g = handle(dim, nlist, 3)
    p = handle(dim, nlist, 1)
    g.train(X)
    p.train(XU)
    o = oracle.OracleIndex(dim, nlist, 1)
    o.train(XU)
    Co = o.centroids
    assert np.array_equal(bits(p.centroids), bits(Co)), "the InnerProduct handle's train() differs from the oracle's"
    Cg = g.centroids
    assert np.array_equal(bits(Cg), bits(unit_rows_ref(p.centroids)))
    assert np.array_equal(bits(Cg), bits(unit_rows_ref(Co)))
    # centroids equal before the normalisation are equal after it; a zero centroid stays zero
    _, first = np.unique(bits(Co), axis=0, return_index=True)
    assert len(first) < nlist, "the set must repeat a centroid"
    for c in range(nlist):
        same = np.flatnonzero((bits(Co) == bits(Co[c])).all(axis=1))
        assert np.array_equal(bits(Cg[same]), np.broadcast_to(bits(Cg[c]), (len(same), dim)))
    zero = (Co == 0).all(axis=1)
    if name == "duplicates_zero_row":
        assert zero.any(), "the set must leave a zero centroid"
    assert np.all(bits(Cg[zero]) == 0)
    p.centroids = Cg
    g.add(X, ids)
    p.add(XU, ids)
    assert g.list_sizes().tolist() == p.list_sizes().tolist()
    for l in range(nlist):
        (Vg, Ig), (Vp, Ip) = g.get_list(l), p.get_list(l)
        assert np.array_equal(Ig, Ip) and np.array_equal(bits(Vg), bits(Vp)), f"list {l}"
    Q = X[:min(len(X), 20)]
    D, I = p.search(unit_rows_ref(Q), nprobe=min(nlist, 8), k=5)
    assert_same(g.search(Q, nprobe=min(nlist, 8), k=5), (cos_map(D, I), I))


@pytest.mark.parametrize("nlist", [65537, 70001])
def test_add_and_search_above_65535_lists(nlist):
    """More lists than a grid's y extent is known to hold (DESIGN §1 documents nlist < 524287):
    ivf_copy_lists walks the lists by blockIdx.y. The centroids are given, not trained: the
    reference's k-means++ seeding is cubic (nlist 1000 at 3000 rows takes 16 s on one core), so
    train is not run at this size and lloyd_update's launch is not reached here. 6000 N(0,1) rows
    of dim 4 go in through three adds of 3000, 1 and 2999 rows; the second and the third move the
    existing lists through ivf_copy_lists. A launch the runtime refuses would surface as a
    VdbError (hipGetLastError after the launch), not as a fault."""
    dim, n = 4, 6000
    rng = np.random.default_rng(nlist)
    C = rng.standard_normal((nlist, dim)).astype(np.float32)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    C[65536], C[nlist - 1] = X[8], X[7]  # lists 65536 and nlist - 1 hold a row from the first add on
    Q = np.concatenate([X[:20], rng.standard_normal((20, dim)).astype(np.float32)])
    ids = rng.permutation(n).astype(np.uint64) + 5
    o = oracle.OracleIndex(dim, nlist, 0)
    o.centroids = C
    g = handle(dim, nlist)
    g.centroids = C
    for a, b in ((0, 3000), (3000, 3001), (3001, n)):
        o.add(X[a:b], ids[a:b])
        g.add(X[a:b], ids[a:b])
    assert g.get_total_vectors() == n
    ref = np.array([o.list_count(l) for l in range(nlist)], np.uint64)
    assert ref[65536] >= 1 and ref[nlist - 1] >= 1, "rows must land in lists above 65535"
    fullest = np.argsort(-ref.astype(np.int64), kind="stable")[:5]
    single = np.flatnonzero(ref == 1)
    single = single[[0, len(single) // 3, len(single) // 2, -2, -1]]  # (low and high list ids)
    assert int(ref[fullest].min()) >= 2 and len(set(single.tolist())) == 5
    assert_lists(g, o, nlist, lists=fullest.tolist() + single.tolist() + [65536, nlist - 1])
    for nprobe in (1, 70):
        assert_same(g.search(Q, nprobe=nprobe, k=5), o.search(Q, nprobe, 5))
