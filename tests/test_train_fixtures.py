"""CPU: the training sets of train_fixtures.py reach what they are named for, on the oracle.

The GPU tests (test_gpu_train_edges.py) compare train() and add() with the oracle on these sets;
a set that drifted away from its edge (no empty cluster left, keys that fit 8 bits, sums that no
longer depend on their order) would let them pass without testing anything. So every set's
property is asserted here, and the oracle's train is pinned to the numpy restatement of the
Lloyd loop from the oracle's own seeds, bit for bit.
"""
import numpy as np
import pytest

import oracle.np_ref as npr
import train_fixtures as tf


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", tf.NAMES)
def test_oracle_train_is_lloyd_from_its_seeds(name):
    X, dim, nlist, metric = tf.training_set(name)
    C = tf.oracle_centroids(name)
    assert C.shape == (nlist, dim) and np.all(np.isfinite(C))
    ref = npr.lloyd(metric, X, tf.oracle_seeds(name))
    bad = np.flatnonzero((bits(C) != bits(ref)).any(axis=1))
    assert bad.size == 0, f"{name}: oracle.train differs from np_ref.lloyd at centroids {bad[:5].tolist()}"
    # every seed is a training row
    rows = {r.tobytes() for r in X}
    assert all(s.tobytes() in rows for s in tf.oracle_seeds(name))


def test_sets_are_deterministic_and_read_only():
    for name in tf.NAMES:
        X, dim, nlist, metric = tf.training_set(name)
        Y = tf._make(name)[0]
        assert np.array_equal(bits(X), bits(Y)), name
        assert not X.flags.writeable and X.dtype == np.float32 and X.flags.c_contiguous
    shapes = {n: tf.training_set(n)[0].shape + tf.training_set(n)[2:] for n in tf.NAMES}
    assert shapes == {
        "wide_keys": (1500, 24, 300, 0), "wide_keys_small": (700, 24, 300, 0),
        "fewer_rows_than_lists": (40, 20, 100, 0), "one_row": (1, 20, 5, 0),
        "ragged_63": (63, 67, 7, 0), "ragged_64": (64, 67, 7, 0), "ragged_65": (65, 67, 7, 0),
        "ragged_63b": (63, 16, 12, 0), "duplicates": (1500, 16, 80, 0), "all_equal": (200, 16, 6, 0),
        "offset": (2000, 32, 40, 0), "hub": (5100, 16, 12, 0), "inner_product": (1200, 16, 30, 1)}


# (empty clusters after the last assignment, repeated seed rows): what the sets' structure fixes.
# fewer_rows_than_lists: 40 distinct rows are picked, then total_dist == 0 picks row 0 sixty times,
# and a repeated centroid never wins the strict '<' against its first copy.
EMPTY_AND_REPEATED = {"fewer_rows_than_lists": (60, 60), "duplicates": (30, 30), "one_row": (4, 4),
                      "all_equal": (5, 5)}


@pytest.mark.parametrize("name", sorted(EMPTY_AND_REPEATED))
def test_empty_clusters_and_repeated_seeds(name):
    counts = tf.last_counts(name)
    empty, repeated = int((counts == 0).sum()), tf.repeated_seeds(name)
    print(f"{name}: {empty} clusters empty after the last assignment, {repeated} repeated seeds")
    assert empty >= 1 and repeated >= 1
    assert (empty, repeated) == EMPTY_AND_REPEATED[name]
    assert int(counts.sum()) == tf.training_set(name)[0].shape[0]
    # an empty cluster keeps its seed: the final centroid is the seed row, bit for bit
    C, S = tf.oracle_centroids(name), tf.oracle_seeds(name)
    X, dim, nlist, metric = tf.training_set(name)
    never = np.ones(nlist, bool)          # clusters empty in every iteration
    Ci = np.array(S)
    for _ in range(10):
        a = npr.assign(metric, Ci, X)
        never &= np.bincount(a, minlength=nlist) == 0
        Ci = npr.lloyd(metric, X, Ci, iters=1)
    assert np.array_equal(bits(C[never]), bits(S[never]))
    # Clusters of one row have exact means (x / 1), so there the repeated seeds stay empty for
    # good. The mean of 30 or 200 equal rows is not the row (the fp32 sum rounds), so the rows
    # move on to a later exact copy of their seed: all_equal has no cluster empty throughout.
    print(f"{name}: {int(never.sum())} clusters empty in every iteration")
    if name in ("fewer_rows_than_lists", "one_row"):
        assert int(never.sum()) == EMPTY_AND_REPEATED[name][0]
    elif name == "duplicates":
        assert int(never.sum()) >= 1


@pytest.mark.parametrize("name", ["wide_keys", "wide_keys_small"])
def test_wide_keys_fill_every_cluster(name):
    X, dim, nlist, metric = tf.training_set(name)
    counts = tf.last_counts(name)
    assert nlist > 256 and int(counts.min()) >= 1, f"{name}: {int((counts == 0).sum())} empty clusters"
    assert int(tf.last_assignment(name).max()) >= 256          # a key that needs its ninth bit
    assert tf.repeated_seeds(name) == 0
    assert (X.shape[0] >= 1024) == (name == "wide_keys")       # the 2x2 MFMA kernel's threshold
    assert all(nlist % t for t in (16, 32, 64, 256))


def test_hub_has_one_cluster_above_4000_rows():
    counts = tf.last_counts("hub")
    print(f"hub: cluster sizes {sorted(counts.tolist(), reverse=True)}")
    assert int(counts.max()) > 4000 and int((counts > 4000).sum()) == 1


def test_offset_sums_depend_on_their_order():
    """The Lloyd update sums a cluster's members in input order, one fp32 add at a time. On this
    set the same members summed in reverse order give other bits, so a kernel that sums in
    another order cannot pass."""
    X, dim, nlist, metric = tf.training_set("offset")
    a, counts = tf.last_assignment("offset"), tf.last_counts("offset")
    c = int(np.argmax(counts))
    members = X[a == c]
    fwd, rev = np.zeros(dim, np.float32), np.zeros(dim, np.float32)
    for r in members:
        fwd = fwd + r
    for r in members[::-1]:
        rev = rev + r
    n = np.float32(len(members))
    differing = int((bits(fwd / n) != bits(rev / n)).sum())
    print(f"offset: cluster {c} of {len(members)} rows, sums near {float(fwd[0]):.0f}; "
          f"{differing} of {dim} centroid elements differ when summed in reverse")
    assert np.array_equal(bits(fwd / n), bits(tf.oracle_centroids("offset")[c]))  # (the forward sum is the oracle's)
    assert differing >= 1
    assert float(np.abs(fwd).min()) > 1e4     # sums far above the rows' spread: the low bits carry the order


@pytest.mark.parametrize("name", ["ragged_63", "ragged_64", "ragged_65", "ragged_63b"])
def test_ragged_sets_straddle_one_block(name):
    X, dim, nlist, metric = tf.training_set(name)
    assert X.shape[0] in (63, 64, 65) and (dim == 67 or name == "ragged_63b")
    assert int(tf.last_counts(name).sum()) == X.shape[0]
    # the last rows (the ragged block's highest lanes) do not all fall into one cluster
    a = tf.last_assignment(name)
    assert len(set(a[-16:].tolist())) >= 2


def test_inner_product_assignment_differs_from_l2():
    """k-means++ measures L2 whatever the metric; the Lloyd assignment follows the metric. The set
    must tell the two apart."""
    X, dim, nlist, metric = tf.training_set("inner_product")
    assert metric == 1
    S = tf.oracle_seeds("inner_product")
    assert not np.array_equal(npr.assign(0, S, X), npr.assign(1, S, X))
    assert not np.array_equal(bits(npr.lloyd(0, X, S, iters=1)), bits(npr.lloyd(1, X, S, iters=1)))


def test_second_train_pair_shares_a_shape():
    (_, da, la, ma), (_, db, lb, mb) = tf.training_set("hub"), tf.training_set("ragged_63b")
    assert (da, la, ma) == (db, lb, mb)
