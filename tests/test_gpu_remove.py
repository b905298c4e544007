"""GPU: vdb_ivf_remove_ids (device-side list compaction) against the CPU oracle.

Definition under test: the index after a remove is the index built from the same centroids
by adding the surviving rows in their original order. So in every case the expected state is a
fresh OracleIndex with the handle's centroids and add(X[keep], ids[keep]), and totals, list
sizes, every list's contents (ids and row bits) and every search result (ids and distance bits)
must match it, for every metric, k and scan path.

Base shape: N = 3000, Q = 32, nlist = 8 (lists of several 64-slot blocks ending in a partial
one); removal sets are chosen from the handle's own lists so each condition holds by construction.
"""
import os
import subprocess
import threading

import numpy as np
import pytest

import oracle
from conftest import load_vdb

vdb = load_vdb()
pytestmark = pytest.mark.gpu

N, NQ, NLIST = 3000, 32, 8
NONE = np.iinfo(np.uint64).max
FMAX = np.finfo(np.float32).max
K_BIG = 1024  # above the rows two probed lists hold: unfilled slots and pad lanes take part
BLOCK_BYTES = 64 * (64 * 4 + 8)  # one arena block: dimensions 30 and 32 both pad to 64 floats
_data = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(D, I, Dr, Ir):
    assert I.shape == Ir.shape
    bad = np.argwhere(I != Ir)
    assert bad.size == 0, f"ids differ at {bad[:5].tolist()}: gpu {I[tuple(bad[0])]} ref {Ir[tuple(bad[0])]}"
    badd = np.argwhere(bits(D) != bits(Dr))
    assert badd.size == 0, f"dist bits differ at {badd[:5].tolist()}: gpu {D[tuple(badd[0])]!r} ref {Dr[tuple(badd[0])]!r}"


def data(dim):
    """(X, Q, ids, centroids) of the base shape, computed once per dimension and never changed."""
    if dim not in _data:
        X, Q, ids = oracle.reference_test_data(N, NQ, dim, seed=1000 + dim)
        C = np.ascontiguousarray(X[:: N // NLIST][:NLIST])
        for a in (X, Q, ids, C):
            a.setflags(write=False)
        _data[dim] = (X, Q, ids, C)
    return _data[dim]


def make(dim, metric=0, ids=None, **cfg):
    X, Q, ids0, C = data(dim)
    g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, NLIST, vdb.Metric(metric), **cfg))
    g.centroids = C
    g.add(X, ids0 if ids is None else ids)
    return g


def expected(g, dim, metric, parts):
    """The oracle given the handle's centroids and `parts`, a sequence of (rows, ids) adds."""
    o = oracle.OracleIndex(dim, NLIST, metric)
    o.centroids = g.centroids
    for V, I in parts:
        if len(I):
            o.add(V, I)
    return o


def oracle_search(o, Q, nprobe, k, stale=True):
    if stale:
        return o.search(Q, nprobe, k)
    # stale_slots 0: an empty probed list contributes nothing, which is what the reference's
    # per-call slot logic gives a call of one query (no previous query's slot to inherit)
    out = [o.search(Q[i:i + 1], nprobe, k) for i in range(Q.shape[0])]
    return np.concatenate([d for d, _ in out]), np.concatenate([i for _, i in out])


def assert_after(g, o, Q, stale=True, searches=((3, 10), (NLIST, 10), (2, K_BIG)), unfilled=True):
    assert g.get_total_vectors() == o.total_vectors
    sizes = g.list_sizes()
    assert sizes.tolist() == [o.list_count(l) for l in range(NLIST)]
    dim = Q.shape[1]
    usage = int(sizes.sum()) * (dim * 4 + 8)
    if g.cache_stats()["capacity_bytes"]:  # the tier: only the lists the cache holds count
        assert g.get_gpu_memory_usage() <= usage
    else:
        assert g.get_gpu_memory_usage() == usage
    for l in range(NLIST):
        gv, gi = g.get_list(l)
        ov, oi = o.get_list(l)
        assert np.array_equal(gi, oi), f"list {l}: ids or their order differ"
        assert np.array_equal(bits(gv), bits(ov)), f"list {l}: row bits differ"
    for nprobe, k in searches:
        Dr, Ir = oracle_search(o, Q, nprobe, k, stale)
        if k == K_BIG and unfilled:
            assert (Ir == NONE).any(), "the large-k search must leave unfilled slots"
        assert_same(*g.search(Q, nprobe=nprobe, k=k), Dr, Ir)


def lists_of(g):
    return [g.get_list(l)[1] for l in range(NLIST)]


# ---- 1. removal patterns ----
@pytest.mark.parametrize("dim", [32, 30])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_removal_patterns(metric, dim):
    X, Q, ids, _ = data(dim)

    def run(pick, stale=True, gone=None):
        """A fresh handle, one search (the screen is built), remove pick(lists), compare."""
        g = make(dim, metric)
        g.set_stale_slots(stale)
        g.search(Q, nprobe=3, k=10)
        req = np.asarray(pick(lists_of(g)), dtype=np.uint64)
        keep = ~np.isin(ids, req)
        held = g.gpu_bytes_allocated()
        n = g.remove_ids(req)
        assert n == int((~keep).sum())
        if gone is not None:
            assert n == gone
        if n == 0:  # nothing reallocated, the screen's data kept
            assert g.gpu_bytes_allocated() == held
        # (Cosine leaves every distance at 0.0f, so every row sits in list 0: more than K_BIG)
        assert_after(g, expected(g, dim, metric, [(X[keep], ids[keep])]), Q, stale, unfilled=metric != 2)
        return g

    def middle(ls):  # a stored list of middling size
        order = sorted((l for l in range(NLIST) if len(ls[l])), key=lambda l: len(ls[l]))
        return order[len(order) // 2]

    # (a) ids not in the index, the pad value among them: nothing changes
    run(lambda ls: [N, N + 7, 2 ** 40, NONE], gone=0)
    # (b) every third id, some repeated in the request
    run(lambda ls: np.concatenate([ids[::3], ids[:300:3], ids[::3][-5:]]), gone=1000)
    # (c) exactly the first 64 rows of one list: a whole block goes, the rest moves down one
    run(lambda ls: max(ls, key=len)[:64], gone=64)
    # (d) only the last row of each list: the partial blocks alone are touched
    run(lambda ls: [l[-1] for l in ls if len(l)])
    # (e) one whole list, with the empty-list quirk on and off
    for stale in (True, False):
        emptied = []
        g = run(lambda ls: emptied.append(middle(ls)) or ls[emptied[0]], stale=stale)
        assert g.list_sizes()[emptied[0]] == 0 and g.get_total_vectors() < N
    # (f) everything: every result slot is unfilled
    g = run(lambda ls: ids, gone=N)
    assert g.get_total_vectors() == 0
    D, I = g.search(Q, nprobe=3, k=10)
    assert np.all(I == NONE) and np.all(D == FMAX)
    assert g.remove_ids(ids) == 0 and g.remove_ids([]) == 0


# ---- 2. an id stored more than once ----
def test_duplicate_ids_all_go():
    dim = 32
    X, Q, ids, _ = data(dim)
    dup = ids % 1500
    g = make(dim, ids=dup)
    g.search(Q, nprobe=3, k=10)
    req = np.arange(100, 300, 2, dtype=np.uint64)
    keep = ~np.isin(dup, req)
    assert g.remove_ids(req) == 200
    assert_after(g, expected(g, dim, 0, [(X[keep], dup[keep])]), Q)


# ---- 3. remove, add, search, remove again ----
def test_remove_add_remove():
    dim = 32
    X, Q, ids, _ = data(dim)
    X2, _, _ = oracle.reference_test_data(500, 1, dim, seed=77)
    ids2 = np.arange(N, N + 500, dtype=np.uint64)
    g = make(dim)
    g.search(Q, nprobe=3, k=10)
    keep = ids % 4 != 1
    assert g.remove_ids(ids[~keep]) == int((~keep).sum())
    g.add(X2, ids2)  # appends land after the survivors
    assert_after(g, expected(g, dim, 0, [(X[keep], ids[keep]), (X2, ids2)]), Q)
    keep_b = keep & (ids % 5 != 0)
    keep2 = ids2 % 2 == 0
    req = np.concatenate([ids[ids % 5 == 0], ids2[~keep2]])
    assert g.remove_ids(req) == int((keep & ~keep_b).sum() + (~keep2).sum())
    assert_after(g, expected(g, dim, 0, [(X[keep_b], ids[keep_b]), (X2[keep2], ids2[keep2])]), Q)


# ---- 4. every scan path, starting from the arena_dropped state ----
@pytest.mark.parametrize("path", ["i8", "bf16", "screen_off", "inline", "k100"])
def test_scan_paths(path):
    dim = 32
    X, Q, ids, _ = data(dim)
    g = make(dim)
    opts = {"i8": {"screen_i8": 1}, "bf16": {"screen_i8": 0}, "screen_off": {}, "inline": {"screen_defer": 0},
            "k100": {}}[path]
    for name, v in opts.items():
        g.set_option(name, v)
    g.set_option("screen_floor_ppm", 0)
    g.search(Q, nprobe=3, k=10)  # builds the screen: the row copy is now the lists' only fp32 copy
    assert g.profile_read()["screen_shadow"] in (1, 2)
    if path == "screen_off":
        g.set_option("screen", 0)
    keep = ids % 3 != 0
    assert g.remove_ids(ids[~keep]) == 1000
    o = expected(g, dim, 0, [(X[keep], ids[keep])])
    k = 100 if path == "k100" else 10
    assert_same(*g.search(Q, nprobe=3, k=k), *o.search(Q, 3, k))
    shadow = g.profile_read()["screen_shadow"]
    if path == "i8":
        assert shadow == 2
    elif path in ("bf16", "inline"):
        assert shadow == 1
    elif path == "screen_off":
        assert shadow == 0
    assert_after(g, o, Q)


# ---- 5. host-home tier ----
@pytest.mark.parametrize("screen", [1, 0])
def test_tier_host_home(screen):
    # Inner product: its lists are of similar size here, so a cache of a quarter of the blocks
    # holds any one list. An exact-path search (the screen off, or k > 64) needs every list a
    # query probes resident at once, so those searches probe one list; the screened tier
    # loads no list and also runs nprobe = nlist.
    dim, metric = 32, 1
    X, Q, ids, _ = data(dim)
    g = make(dim, metric, max_gpu_memory=0)
    g.set_option("screen", screen)
    per_list = [(int(c) + 63) // 64 for c in g.list_sizes()]
    quarter = sum(per_list) // 4
    assert max(per_list) <= quarter
    g.set_option("list_cache_bytes", quarter * BLOCK_BYTES)
    assert g.cache_stats()["capacity_bytes"] > 0
    g.search(Q, nprobe=1, k=10)
    keep = ids % 3 != 1
    assert g.remove_ids(ids[~keep]) == int((~keep).sum())
    assert g.cache_stats()["capacity_bytes"] > 0
    o = expected(g, dim, metric, [(X[keep], ids[keep])])
    assert_after(g, o, Q, searches=((1, 10), (1, K_BIG)) + (((NLIST, 10),) if screen else ()))


def test_tier_entered_by_the_cap_is_left():
    dim = 32
    X, Q, ids, _ = data(dim)
    row = dim * 4 + 8
    g = make(dim, max_gpu_memory=N * row * 3 // 4)  # the add exceeds it: the tier
    assert g.cache_stats()["capacity_bytes"] > 0
    g.search(Q, nprobe=2, k=10)
    keep = ids % 2 == 0  # half the rows: back under the cap
    assert g.remove_ids(ids[~keep]) == N // 2
    assert g.cache_stats()["capacity_bytes"] == 0
    assert_after(g, expected(g, dim, 0, [(X[keep], ids[keep])]), Q)


# ---- 6. refusals leave the handle untouched ----
def test_refused_on_a_file_home(tmp_path):
    dim = 32
    X, Q, ids, _ = data(dim)
    g = make(dim)
    path = str(tmp_path / "lists.ivf")
    g.save(path)
    sizes = g.list_sizes()
    h = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, NLIST))
    h.set_option("list_cache_bytes", (int(((sizes + 63) // 64).sum()) + 2) * BLOCK_BYTES)
    h.open_lists(path)
    D0, I0 = h.search(Q, nprobe=3, k=10)
    with pytest.raises(vdb.VdbError, match="read-only") as e:
        h.remove_ids(ids[:10])
    assert e.value.code == -5  # VDB_ERR_STATE
    assert np.array_equal(h.list_sizes(), sizes)
    assert_same(*h.search(Q, nprobe=3, k=10), D0, I0)


def test_refused_on_a_shard():
    dim = 32
    X, Q, ids, _ = data(dim)
    g = make(dim)
    g.set_shard(0, 2)
    sizes = g.list_sizes()
    D0, I0 = g.search(Q, nprobe=3, k=10)
    with pytest.raises(vdb.VdbError, match="sharded") as e:
        g.remove_ids(ids[:10])
    assert e.value.code == -4  # VDB_ERR_UNSUPPORTED
    assert np.array_equal(g.list_sizes(), sizes)
    assert_same(*g.search(Q, nprobe=3, k=10), D0, I0)


# ---- 7. group handle: two members on the one device ----
def test_group():
    dim = 32
    X, Q, ids, _ = data(dim)
    g = make(dim, devices=(0, 0))
    assert g.group_size == 2
    g.search(Q, nprobe=3, k=10)
    owners = g.list_owners()
    assert set(owners.tolist()) == {0, 1}
    whole = g.get_list(5)[1]
    req = np.concatenate([ids[::3], whole])  # every third id and one whole list
    keep = ~np.isin(ids, req)
    assert g.remove_ids(req) == int((~keep).sum())
    assert np.array_equal(g.list_owners(), owners)  # an emptied list stays placed
    assert g.list_sizes()[5] == 0
    assert_after(g, expected(g, dim, 0, [(X[keep], ids[keep])]), Q)
    X2, _, _ = oracle.reference_test_data(400, 1, dim, seed=78)
    ids2 = np.arange(N, N + 400, dtype=np.uint64)
    g.add(X2, ids2)
    assert np.array_equal(g.list_owners(), owners)
    assert_after(g, expected(g, dim, 0, [(X[keep], ids[keep]), (X2, ids2)]), Q)


# ---- 8. save / load round trip ----
def test_save_load_after_remove(tmp_path):
    dim = 30
    X, Q, ids, _ = data(dim)
    g = make(dim)
    g.search(Q, nprobe=3, k=10)
    keep = ids % 3 != 2
    g.remove_ids(ids[~keep])
    path = str(tmp_path / "after.ivf")
    g.save(path)
    h = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(dim, NLIST))
    h.load(path)
    assert_after(h, expected(g, dim, 0, [(X[keep], ids[keep])]), Q)


# ---- 9. searches concurrent with one remove ----
def test_concurrent_searches_see_before_or_after():
    dim = 32
    X, Q, ids, _ = data(dim)
    g = make(dim)
    keep = ids % 3 != 0
    o_before = expected(g, dim, 0, [(X, ids)])
    o_after = expected(g, dim, 0, [(X[keep], ids[keep])])
    T, loops = 4, 50
    batches = [Q[t * 8:(t + 1) * 8] for t in range(T)]
    want = [(o_before.search(b, 3, 10), o_after.search(b, 3, 10)) for b in batches]
    g.search(Q, nprobe=3, k=10)
    results = [[] for _ in range(T)]
    errors = []

    started = [threading.Event() for _ in range(T)]

    def worker(t):
        try:
            for _ in range(loops):
                results[t].append(g.search(batches[t], nprobe=3, k=10))
                started[t].set()
        except Exception as e:  # noqa: BLE001
            errors.append(e)
            started[t].set()

    th = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
    for x in th:
        x.start()
    for e in started:  # every thread is inside its loop when the remove runs
        e.wait()
    assert g.remove_ids(ids[~keep]) == 1000
    for x in th:
        x.join()
    assert not errors, errors
    for t in range(T):
        assert len(results[t]) == loops
        for D, I in results[t]:
            (Db, Ib), (Da, Ia) = want[t]
            before = np.array_equal(I, Ib) and np.array_equal(bits(D), bits(Db))
            after = np.array_equal(I, Ia) and np.array_equal(bits(D), bits(Da))
            assert before or after, "a search saw neither the index before the remove nor the one after"
        assert_same(*g.search(batches[t], nprobe=3, k=10), *want[t][1])


# ---- 10. the drop-in C++ class ----
def test_cpp_class_remove():
    cpp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    exe = os.path.join(cpp, "bin", "remove_test")
    subprocess.check_call(["make", "-s", "-C", cpp, exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "after remove bit-identical to the CPU path over the survivors: yes" in p.stdout
