"""A CPU model of one index through its whole life, and the two scenarios that drive it.

Model: the centroids, the metric and per list the (rows, ids) in stored order. Its mutations
follow the definitions the per-feature GPU tests already fix (add: oracle assignment, appended in
request order; remove: a stable filter of every list; upsert: remove(all request ids) then
add(winners), test_gpu_upsert.winners; new centroids: every row stays in its list). Its reads
build one oracle.OracleIndex per state (set_list per list) and are cached until the next
mutation. Metric.CosineDistance (3) is an inner-product oracle over cosine_ref.unit_rows_ref rows
and queries with cos_map over the distances; Metric.Cosine (2) builds no screen and is not
modelled.

range(): the oracle's whole single-query result per query, cut by test_gpu_range.cut. (That
module's full() builds its oracle for its own 12 lists, so the per-query loop is this model's,
over its own cached oracle.)

scripted() and walk() are generators of steps. A step is (name, ops); the driver
applies the ops to the model (and to a handle, on the GPU) and resumes the generator, which then
asserts on the model that the step hit its edge. They need no GPU: test_lifecycle_model.py runs
them on the model alone and pins the list sizes after every scripted step (SCRIPT_SIZES).
"""
import hashlib

import numpy as np

import oracle
from cosine_ref import cos_map, unit_rows_ref
from test_gpu_exhaustive import ref as exhaustive_ref
from test_gpu_range import cut
from test_gpu_upsert import winners

NONE = np.iinfo(np.uint64).max
FMAX = np.finfo(np.float32).max
N, NQ, NLIST = 2500, 40, 8
FRESH0 = 10 ** 6  # ids from here on are never in the fixture
ABSENT = np.array([5 * 10 ** 8 + i for i in range(6)] + [NONE - 1, NONE], dtype=np.uint64)  # never stored
_fx = {}


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)


def blocks(sizes):
    return int(sum((int(s) + 63) // 64 for s in sizes))


class Model:
    def __init__(self, dim, nlist, metric, centroids):
        assert metric in (0, 1, 3)
        self.dim, self.nlist, self.metric = dim, nlist, metric
        self.om = 1 if metric == 3 else metric  # the oracle's metric
        self.C = f32(centroids).copy()
        self.lists = [(np.empty((0, dim), np.float32), np.empty(0, np.uint64)) for _ in range(nlist)]
        self.last = None  # what the latest mutation returned
        self._cache = {}

    def _changed(self):
        """Drop everything computed for the state that a mutation just left."""
        self._cache = {}

    # ---- state ----
    def copy(self):
        """The same state in a model of its own (the cached oracles stay with this one)."""
        c = Model(self.dim, self.nlist, self.metric, self.C)
        c.lists = [(v.copy(), i.copy()) for v, i in self.lists]
        return c

    def sizes(self):
        return [len(i) for _, i in self.lists]

    @property
    def total(self):
        return sum(self.sizes())

    def rows(self):
        """(rows, ids) of every stored row, in (list, position) order."""
        return np.concatenate([v for v, _ in self.lists]), np.concatenate([i for _, i in self.lists])

    def stored_ids(self):
        return self.rows()[1]

    def twice(self):
        """The ids stored more than once."""
        i, c = np.unique(self.stored_ids(), return_counts=True)
        return i[c > 1]

    def prep(self, V):
        V = f32(V).reshape(-1, self.dim)
        return unit_rows_ref(V) if self.metric == 3 else V

    def _oracle(self, key=None, allowed=None):
        """The state's oracle; with `allowed` (a set of ids, cached under `key`) over those rows only."""
        k = ("oracle", key)
        if k not in self._cache:
            o = oracle.OracleIndex(self.dim, self.nlist, self.om)
            o.centroids = self.C
            for l, (v, i) in enumerate(self.lists):
                keep = slice(None) if allowed is None else np.isin(i, allowed)
                o.set_list(l, v[keep], i[keep])
            self._cache[k] = o
        return self._cache[k]

    def assign(self, V):
        """The list add() puts each row of V in."""
        return self._oracle().assign(self.prep(V))

    # ---- mutations ----
    def _append(self, V, ids, lists):
        for l in range(self.nlist):
            sel = np.flatnonzero(lists == l)
            if sel.size:
                v, i = self.lists[l]
                self.lists[l] = (np.concatenate([v, V[sel]]), np.concatenate([i, ids[sel]]))
        self._changed()

    def add(self, V, ids):
        V, ids = self.prep(V), u64(ids)
        self._append(V, ids, self._oracle().assign(V) if len(ids) else np.empty(0, np.uint32))
        self.last = None

    def add_to_lists(self, V, ids, lists):
        self._append(self.prep(V), u64(ids), np.asarray(lists, dtype=np.uint32))
        self.last = None

    def remove(self, ids):
        ids = u64(ids)
        gone = 0
        for l, (v, i) in enumerate(self.lists):
            keep = ~np.isin(i, ids)
            gone += int((~keep).sum())
            self.lists[l] = (v[keep], i[keep])
        self._changed()
        self.last = gone
        return gone

    def upsert(self, V, ids):
        V, ids = f32(V).reshape(-1, self.dim), u64(ids)
        w = winners(ids)
        replaced = self.remove(ids)
        self.add(V[w], ids[w])
        self.last = (replaced, int(w.sum()))
        return self.last

    def set_centroids(self, C):
        self.C = f32(C).reshape(self.nlist, self.dim).copy()
        self._changed()
        self.last = None

    def save(self, path=None):
        pass

    def load(self, path=None):
        pass

    # ---- filters ----
    def allowed_ids(self, ids, include):
        """The stored ids a filter (ids, include) lets through, sorted."""
        stored = np.unique(self.stored_ids())
        hit = np.isin(stored, u64(ids))
        return stored[hit if include else ~hit]

    def allowed_count(self, ids, include):
        return int((np.isin(self.stored_ids(), u64(ids)) == bool(include)).sum())

    @staticmethod
    def _fkey(ids, include):
        return (hashlib.sha1(u64(ids).tobytes()).hexdigest(), bool(include))

    # ---- reads ----
    def _search(self, o, Q, nprobe, k):
        Q = f32(Q).reshape(-1, self.dim)
        if self.metric != 3:
            return o.search(Q, nprobe, k)
        D, I = o.search(unit_rows_ref(Q), nprobe, k)
        return cos_map(D, I), I

    def search(self, Q, nprobe, k):
        return self._search(self._oracle(), Q, nprobe, k)

    def search_allowed(self, Q, nprobe, k, allow_ids, include):
        key = self._fkey(allow_ids, include)
        return self._search(self._oracle(key, self.allowed_ids(allow_ids, include)), Q, nprobe, k)

    def search_multi(self, Q, nprobe, k, filters, filter_of):
        Q, fo = f32(Q).reshape(-1, self.dim), np.asarray(filter_of)
        D = np.full((len(Q), k), FMAX, np.float32)
        I = np.full((len(Q), k), NONE, np.uint64)
        for f, (ids, include) in enumerate(filters):
            if (fo == f).any():
                D[fo == f], I[fo == f] = self.search_allowed(Q[fo == f], nprobe, k, ids, include)
        return D, I

    def full(self, Q, nprobe, allow=None):
        """Per query the oracle's whole single-query result (its real entries), once per state."""
        Q = f32(Q).reshape(-1, self.dim)
        fkey = None if allow is None else self._fkey(*allow)
        k = ("full", hashlib.sha1(Q.tobytes()).hexdigest(), nprobe, fkey)
        if k not in self._cache:
            o = self._oracle() if allow is None else self._oracle(fkey, self.allowed_ids(*allow))
            out = []
            for i in range(len(Q)):
                D, I = self._search(o, Q[i:i + 1], nprobe, max(self.total, 1))
                real = I[0] != NONE
                out.append((D[0][real].copy(), I[0][real].copy()))
            self._cache[k] = out
        return self._cache[k]

    def range(self, Q, nprobe, radius, allow=None):
        return cut(self.full(Q, nprobe, allow), radius)

    def exhaustive(self, Q, k):
        X, ids = self.rows()
        Q = f32(Q).reshape(-1, self.dim)
        if self.metric != 3:
            return exhaustive_ref(self.om, Q, X, ids, k)
        D, I = exhaustive_ref(1, unit_rows_ref(Q), X, ids, k)  # (the stored rows are unit rows already)
        return cos_map(D, I), I

    def fetch(self, ids):
        ids = u64(ids)
        first = self._cache.get("first")
        if first is None:
            first = {}
            for v, i in self.lists:
                for p, x in enumerate(i.tolist()):
                    first.setdefault(x, v[p])
            self._cache["first"] = first
        V = np.zeros((len(ids), self.dim), np.float32)
        F = np.zeros(len(ids), np.uint8)
        for j, x in enumerate(ids.tolist()):
            row = first.get(x)
            if row is not None:
                V[j], F[j] = row, 1
        return V, F

    def search_ids(self, ids, nprobe, k):
        V, F = self.fetch(ids)
        D = np.full((len(F), k), FMAX, np.float32)
        I = np.full((len(F), k), NONE, np.uint64)
        if F.any():
            D[F == 1], I[F == 1] = self.search(V[F == 1], nprobe, k)
        return D, I, F

    def probed_rows(self, Q, nprobe):
        """The rows of the lists each query probes, summed over the queries."""
        Q, o, s = self.prep(Q), self._oracle(), self.sizes()
        return sum(sum(s[int(l)] for l in o.select_nprobe(q, min(nprobe, self.nlist))) for q in Q)


# ---- the fixture ----
def fixture(dim):
    """(X, Q, ids, C) of the scenarios, computed once per dimension and never changed."""
    if dim not in _fx:
        X, Q, ids = oracle.reference_test_data(N, NQ, dim, seed=7000 + dim)
        ids = ids * 7 + 3
        assert int(ids[-1]) < FRESH0
        C = np.ascontiguousarray(X[:: N // NLIST][:NLIST])
        for a in (X, Q, ids, C):
            a.setflags(write=False)
        _fx[dim] = (X, Q, ids, C)
    return _fx[dim]


def start(dim, metric):
    X, Q, ids, C = fixture(dim)
    m = Model(dim, NLIST, metric, C)
    m.add(X, ids)
    return m


class Source:
    """Seeded rows and never-used ids for a scenario."""

    def __init__(self, dim, seed):
        self.dim, self.r, self.next_id = dim, np.random.RandomState(seed), FRESH0 + 100000 * seed

    def rows(self, n):
        return self.r.randn(n, self.dim).astype(np.float32)

    def ids(self, n):
        out = np.arange(self.next_id, self.next_id + n, dtype=np.uint64)
        self.next_id += n
        return out

    def rows_for(self, m, l, n):
        """n rows that add() assigns to list l: rows near its centroid, kept if the model says so."""
        V = (m.C[l][None, :] + np.float32(0.1) * self.rows(4 * n + 16)).astype(np.float32)
        V = V[m.assign(V) == l]
        assert len(V) >= n, f"only {len(V)} of {n} rows for list {l}"
        return np.ascontiguousarray(V[:n])


def step(name, *ops):
    return name, list(ops)


# ---- the scripted scenario ----
def scripted(m, dim):
    """Ten steps, each built from the model's own lists so that its edge holds by construction
    (asserted on the model once the driver has applied the step)."""
    src = Source(dim, 1)
    s0 = m.sizes()
    blocks0 = blocks(s0)
    order = sorted(range(NLIST), key=lambda l: s0[l])
    E, A, B, H = order[0], order[1], order[2], order[-1]  # emptied, to 64, to 1, the largest
    assert s0[E] > 0 and s0[A] > 65 and s0[B] > 2 and len({E, A, B, H}) == 4, f"start: {s0}"

    def at(n):
        return f"step {n}: last {m.last}, sizes {m.sizes()}"

    # 1. a list becomes empty
    yield step("1 empty a list", ("remove", m.lists[E][1].copy()))
    assert m.last == s0[E] and m.sizes()[E] == 0, at(1)

    # 2. 65 -> 64 rows (two blocks to one), and down to one row
    yield step("2a trim to 65 and 2", ("remove", np.concatenate([m.lists[A][1][65:], m.lists[B][1][2:]])))
    assert m.sizes()[A] == 65 and m.sizes()[B] == 2, at("2a")
    yield step("2b 65 to 64, 2 to 1", ("remove", np.array([m.lists[A][1][64], m.lists[B][1][1]], np.uint64)))
    assert m.last == 2 and m.sizes()[A] == 64 and m.sizes()[B] == 1 and m.sizes()[E] == 0, at("2b")

    # 3. ids that match nothing
    before = m.sizes()
    yield step("3 remove nothing", ("remove", ABSENT))
    assert m.last == 0 and m.sizes() == before, at(3)

    # 4. 64 -> 65, rows into the emptied list, a one-row list grows over a block boundary
    V = np.concatenate([src.rows_for(m, A, 1), src.rows_for(m, E, 70), src.rows_for(m, B, 70)])
    p = src.r.permutation(len(V))
    yield step("4 add at the edges", ("add", V[p], src.ids(len(V))[p]))
    assert (m.sizes()[A], m.sizes()[E], m.sizes()[B]) == (65, 70, 71), at(4)

    # 5. replace only: rows of the largest list move to another list
    before, total = m.sizes(), m.total
    req = m.lists[H][1][::2][:100].copy()
    yield step("5 upsert replace-only", ("upsert", src.rows_for(m, A, 100), req))
    assert m.last == (100, 100) and m.total == total, at(5)
    assert m.sizes()[H] == before[H] - 100 and m.sizes()[A] == before[A] + 100, at(5)

    # 6. replaces and inserts, ids repeated inside the request
    stored = src.r.permutation(np.unique(m.stored_ids()))[:60]
    fresh = src.ids(30)
    req = np.concatenate([stored, fresh, stored[:10], fresh[:5]])
    req = req[src.r.permutation(len(req))]
    total = m.total
    yield step("6 upsert with repeats", ("upsert", src.rows(len(req)), req))
    assert m.last == (60, 90) and m.total == total + 30, at(6)

    # 7. far fewer blocks, the other format, more blocks than ever, the first format
    stored = np.unique(m.stored_ids())
    gone = src.r.permutation(stored)[:len(stored) * 6 // 10]
    yield step("7a remove 60 %, toggle", ("remove", gone), ("toggle",))
    assert blocks(m.sizes()) < blocks0 * 6 // 10, at("7a")
    n = len(gone) + 700
    yield step("7b add back", ("add", src.rows(n), src.ids(n)))
    assert blocks(m.sizes()) > blocks0, at("7b")
    yield step("7c toggle", ("toggle",))

    # 8. twenty ids stored twice (two of them twice in one list); one removed: both copies go
    where = {int(i): l for l in range(NLIST) for i in m.lists[l][1]}
    again = src.r.permutation(np.unique(m.stored_ids()))[:20]
    lists = np.array([(where[int(i)] + 1) % NLIST for i in again], np.uint32)
    lists[:2] = [where[int(i)] for i in again[:2]]
    total = m.total
    yield step("8a store 20 ids twice", ("add_to_lists", src.rows(20), again, lists))
    assert m.total == total + 20 and len(m.twice()) == 20, at("8a")
    yield step("8b remove a twice-stored id", ("remove", again[5:6]))
    assert m.last == 2 and len(m.twice()) == 19, at("8b")

    # 9. new centroids on the populated index
    before = m.sizes()
    yield step("9 perturb the centroids", ("centroids", (m.C + np.float32(0.05) * src.rows(NLIST)).astype(np.float32)))
    assert m.sizes() == before, at(9)

    # 10. through a file into a fresh handle, and on
    yield step("10a save and load", ("saveload",))
    assert m.sizes() == before, at("10a")
    stored = np.unique(m.stored_ids())
    yield step("10b remove after load", ("remove", src.r.permutation(stored)[:len(stored) // 20]))
    assert m.last >= len(stored) // 20, at("10b")


# (dim, metric) -> the list sizes at the start and after every scripted step
SCRIPT_STEPS = ["start", "1", "2a", "2b", "3", "4", "5", "6", "7a", "7b", "7c", "8a", "8b", "9", "10a", "10b"]
SCRIPT_SIZES = {
    (30, 0): [
        [167, 270, 499, 122, 251, 153, 699, 339],
        [167, 270, 499, 0, 251, 153, 699, 339],
        [2, 270, 499, 0, 251, 65, 699, 339],
        [1, 270, 499, 0, 251, 64, 699, 339],
        [1, 270, 499, 0, 251, 64, 699, 339],
        [71, 270, 499, 70, 251, 65, 699, 339],
        [71, 270, 499, 70, 251, 165, 599, 339],
        [78, 277, 500, 78, 251, 166, 604, 340],
        [30, 96, 195, 34, 103, 56, 257, 147],
        [161, 347, 586, 157, 299, 166, 858, 420],
        [161, 347, 586, 157, 299, 166, 858, 420],
        [164, 348, 590, 162, 301, 167, 860, 422],
        [164, 348, 589, 161, 301, 167, 860, 422],
        [164, 348, 589, 161, 301, 167, 860, 422],
        [164, 348, 589, 161, 301, 167, 860, 422],
        [154, 328, 552, 152, 288, 158, 826, 403],
    ],
    (30, 3): [
        [335, 291, 280, 329, 359, 317, 236, 353],
        [335, 291, 280, 329, 359, 317, 0, 353],
        [335, 2, 65, 329, 359, 317, 0, 353],
        [335, 1, 64, 329, 359, 317, 0, 353],
        [335, 1, 64, 329, 359, 317, 0, 353],
        [335, 71, 65, 329, 359, 317, 70, 353],
        [335, 71, 165, 329, 259, 317, 70, 353],
        [334, 79, 167, 334, 263, 313, 79, 360],
        [131, 31, 62, 112, 115, 148, 30, 143],
        [356, 294, 240, 358, 392, 356, 210, 423],
        [356, 294, 240, 358, 392, 356, 210, 423],
        [359, 298, 241, 358, 397, 361, 211, 424],
        [359, 298, 241, 357, 396, 361, 211, 424],
        [359, 298, 241, 357, 396, 361, 211, 424],
        [359, 298, 241, 357, 396, 361, 211, 424],
        [344, 279, 227, 339, 376, 345, 201, 403],
    ],
    (200, 1): [
        [336, 233, 328, 340, 251, 359, 338, 315],
        [336, 0, 328, 340, 251, 359, 338, 315],
        [336, 0, 328, 340, 65, 359, 338, 2],
        [336, 0, 328, 340, 64, 359, 338, 1],
        [336, 0, 328, 340, 64, 359, 338, 1],
        [336, 70, 328, 340, 65, 359, 338, 71],
        [336, 70, 328, 340, 165, 259, 338, 71],
        [333, 76, 328, 342, 164, 264, 346, 84],
        [131, 37, 123, 141, 66, 115, 132, 30],
        [428, 215, 375, 366, 223, 349, 393, 288],
        [428, 215, 375, 366, 223, 349, 393, 288],
        [428, 220, 377, 368, 225, 349, 399, 291],
        [428, 220, 377, 368, 225, 348, 398, 291],
        [428, 220, 377, 368, 225, 348, 398, 291],
        [428, 220, 377, 368, 225, 348, 398, 291],
        [409, 207, 361, 344, 213, 331, 383, 274],
    ],
}


# ---- the seeded walk ----
WALK_STEPS = 10
WALK_OPS = ("remove", "add", "add_to_lists", "upsert", "toggle", "centroids")


def walk_ops(seed):
    """The walk's operations: every one of WALK_OPS once, in a seeded order, then seeded draws."""
    r = np.random.RandomState(1000 + seed)
    first = [WALK_OPS[i] for i in r.permutation(len(WALK_OPS))]
    return first + [WALK_OPS[r.randint(len(WALK_OPS))] for _ in range(WALK_STEPS - len(WALK_OPS))]


def walk(m, dim, seed):
    src = Source(dim, 10 + seed)
    r = src.r
    for i, op in enumerate(walk_ops(seed)):
        name = f"seed {seed} step {i}: {op}"
        stored = np.unique(m.stored_ids())
        if op == "remove":  # 1 % .. 50 % of the stored ids, absent ones between them
            n = max(1, int(len(stored) * r.uniform(0.01, 0.5)))
            req = np.concatenate([r.permutation(stored)[:n], ABSENT])
            yield step(name, ("remove", req[r.permutation(len(req))]))
            assert m.last >= n, f"{name}: removed {m.last} of {n}"
        elif op == "add":
            n = int(r.randint(50, 400))
            yield step(name, ("add", src.rows(n), src.ids(n)))
        elif op == "add_to_lists":  # a quarter of the ids are stored already
            n = int(r.randint(20, 200))
            ids = np.concatenate([r.permutation(stored)[:n // 4], src.ids(n - n // 4)])
            yield step(name, ("add_to_lists", src.rows(n), ids, r.randint(0, NLIST, n).astype(np.uint32)))
        elif op == "upsert":  # 0 % .. 100 % of its ids stored, a tenth of the request repeats
            n = int(r.randint(50, 300))
            ns = min(len(stored), int(n * r.uniform(0.0, 1.0)))
            req = np.concatenate([r.permutation(stored)[:ns], src.ids(n - ns)])
            req = np.concatenate([req, req[r.randint(0, n, n // 10)]])
            req = req[r.permutation(len(req))]
            yield step(name, ("upsert", src.rows(len(req)), req))
            assert m.last[1] == n, f"{name}: inserted {m.last} of {n}"
        elif op == "toggle":
            yield step(name, ("toggle",))
        else:
            yield step(name, ("centroids", (m.C + np.float32(0.05) * src.rows(NLIST)).astype(np.float32)))
        assert m.total > 0, name


def apply(m, op):
    """One op of a step on the model; returns what the mutation returned."""
    kind, args = op[0], op[1:]
    if kind == "remove":
        return m.remove(*args)
    if kind == "add":
        return m.add(*args)
    if kind == "add_to_lists":
        return m.add_to_lists(*args)
    if kind == "upsert":
        return m.upsert(*args)
    if kind == "centroids":
        return m.set_centroids(*args)
    assert kind in ("toggle", "saveload"), kind
    return None
