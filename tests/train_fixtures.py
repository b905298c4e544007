"""Named training sets that reach the edges of train() and add(): radix keys wider than 8 bits,
empty clusters, repeated seeds, ragged 64-lane blocks, order-sensitive sums. TEST INFRASTRUCTURE:
no GPU, no package import.

training_set(name) -> (X, dim, nlist, metric). Every set comes from numpy.random.default_rng with
the seed fixed for its name below, is built once and is read-only afterwards. The oracle's results
for a set (its k-means++ seeds, its trained centroids, its last Lloyd assignment and an
OracleIndex trained on the set and holding it) are cached here too, so no test trains the oracle
twice: its seeding is cubic (wide_keys takes seconds on one core).
"""
import numpy as np

import oracle
import oracle.np_ref as npr

L2, IP = 0, 1

# name: (rng seed, what the set reaches)
SETS = {
    "wide_keys": (101, "9-bit radix keys, >= 1024 rows (the 2x2 MFMA kernel), nlist ragged for 16/32/64/256"),
    "wide_keys_small": (102, "9-bit radix keys below 1024 rows (the 16x16 MFMA kernel)"),
    "fewer_rows_than_lists": (103, "60 repeated seeds, 60 clusters empty in every iteration, ties to the lowest"),
    "one_row": (104, "uniform_int(0, 0) and total_dist == 0"),
    "ragged_63": (105, "a ragged last 64-lane block; dim padded 67 -> 128"),
    "ragged_64": (106, "exactly one 64-lane block"),
    "ragged_65": (107, "one row in the second 64-lane block"),
    "ragged_63b": (108, "ragged_63 at hub's dim and nlist: a second train() on one handle"),
    "duplicates": (109, "zero min-distances, repeated seeds, empty clusters, equal distances"),
    "all_equal": (110, "every distance +0.0f"),
    "offset": (111, "cancellation: every centroid a re-rank candidate; sums near 7e4 per cluster"),
    "hub": (112, "one cluster of thousands of rows summed in input order"),
    "inner_product": (113, "k-means++ in L2, Lloyd assignment in IP"),
}
NAMES = tuple(SETS)

_sets, _seeds, _trained, _last, _index = {}, {}, {}, {}, {}


def _normal(rng, n, dim):
    return rng.standard_normal((n, dim)).astype(np.float32)


def _make(name):
    rng = np.random.default_rng(SETS[name][0])
    if name == "wide_keys":
        return _normal(rng, 1500, 24), 24, 300, L2
    if name == "wide_keys_small":
        return _normal(rng, 700, 24), 24, 300, L2
    if name == "fewer_rows_than_lists":
        return _normal(rng, 40, 20), 20, 100, L2
    if name == "one_row":
        return _normal(rng, 1, 20), 20, 5, L2
    if name in ("ragged_63", "ragged_64", "ragged_65"):
        return _normal(rng, int(name[-2:]), 67), 67, 7, L2
    if name == "ragged_63b":
        return _normal(rng, 63, 16), 16, 12, L2
    if name == "duplicates":
        base = _normal(rng, 50, 16)
        return np.repeat(base, 30, axis=0)[rng.permutation(1500)], 16, 80, L2
    if name == "all_equal":
        return np.repeat(_normal(rng, 1, 16), 200, axis=0), 16, 6, L2
    if name == "offset":
        return (np.float32(1000) + _normal(rng, 2000, 32)).astype(np.float32), 32, 40, L2
    if name == "hub":
        return np.concatenate([np.float32(0.01) * _normal(rng, 5000, 16),
                               np.float32(5) + _normal(rng, 100, 16)]).astype(np.float32), 16, 12, L2
    if name == "inner_product":
        return _normal(rng, 1200, 16), 16, 30, IP
    raise KeyError(name)


def training_set(name):
    """(X, dim, nlist, metric) of the named set; X is float32, C-contiguous and read-only."""
    if name not in _sets:
        X, dim, nlist, metric = _make(name)
        X = np.ascontiguousarray(X, np.float32)
        assert X.shape[1] == dim
        X.setflags(write=False)
        _sets[name] = (X, dim, nlist, metric)
    return _sets[name]


def set_ids(name):
    """The ids the set is added under: not the row numbers, so an id taken for a row shows."""
    n = training_set(name)[0].shape[0]
    return np.arange(n, dtype=np.uint64) * 3 + 11


def oracle_index(name):
    """An OracleIndex trained on the set and holding it (add(X, set_ids)). Shared: only read it."""
    if name not in _index:
        X, dim, nlist, metric = training_set(name)
        o = oracle.OracleIndex(dim, nlist, metric)
        o.train(X)
        C = o.centroids
        C.setflags(write=False)
        _trained[name] = C
        o.add(X, set_ids(name))
        _index[name] = o
    return _index[name]


def oracle_centroids(name):
    """The oracle's train(X) centroids."""
    oracle_index(name)
    return _trained[name]


def oracle_seeds(name):
    """The oracle's k-means++ seeds (train_seed_only)."""
    if name not in _seeds:
        X, dim, nlist, metric = training_set(name)
        o = oracle.OracleIndex(dim, nlist, metric)
        o.train_seed_only(X)
        S = o.centroids
        S.setflags(write=False)
        _seeds[name] = S
    return _seeds[name]


def last_assignment(name):
    """The assignment of train's tenth Lloyd iteration (the one its final update sums over),
    from the numpy restatement: nine iterations from the oracle's seeds, then one assign."""
    if name not in _last:
        X, dim, nlist, metric = training_set(name)
        C9 = npr.lloyd(metric, X, oracle_seeds(name), iters=9)
        a = npr.assign(metric, C9, X)
        a.setflags(write=False)
        _last[name] = a
    return _last[name]


def last_counts(name):
    return np.bincount(last_assignment(name), minlength=training_set(name)[2])


def repeated_seeds(name):
    """How many seeds repeat an earlier seed bit for bit."""
    S = oracle_seeds(name)
    return len(S) - len({r.tobytes() for r in S})
