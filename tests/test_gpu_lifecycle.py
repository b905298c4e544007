"""GPU: one handle through its whole life against a CPU model of it (lifecycle_model.py): after
every mutation every read route is compared with the model, ids equal and distance bits equal, no
tolerance anywhere. The per-feature files test each route on a screen built once over a fresh
fixture; here the screen is rebuilt after removes, upserts, adds, a format change and new
centroids, and the four screened side routes (range_search, search_prepared,
search_prepared_multi, search_exhaustive with screen=True) must be served by that rebuilt screen.

The checkpoint after a step:
  stale  (before any plain search) totals, list sizes, every list's ids and row bits, fetch_ids on
         stored, absent, twice-stored and just-removed ids; filters of the previous checkpoint are
         stale and refused (-5) by all six prepared calls if rows moved, live and right (exact
         and screened) if not; fresh filters (exclude ~50 %, include ~2 %, include one list,
         a & b, a.andnot(b)) allow what the model counts; each screened side route equals its
         exact twin and the model, and its record says the exact path served.
  search one plain search (nprobe 3, k 10) equals the model; screen_shadow is the format asked for.
  live   the fresh filters are not stale; search at (3, 10), (8, 10), (2, 1024), search_filtered,
         search_ids, and, exact and screened, search_prepared at k 1, 10, 64, search_prepared_multi
         (40 queries, 5 filters, filter_of shuffled), range_search and range_search_prepared at
         the median radius, +inf and below every distance, search_exhaustive at k 10 and 64. The
         screened calls get a reserve that cannot overflow and their records must say that the
         screen served everything. The plain searches at k 10 must have bounded blocks through the
         screen (profile_read's bounded_blocks under option bounded_stats); the search at k 1024
         (the exact scan's k), search_filtered and search_ids have no such record and are only
         compared with the model.
set_option("screen_i8", ...) rebuilds the screen at once, so after a step that ends in a format
toggle (and after a remove that matched nothing) the screen is live already: the stale phase then
requires the screen, not the exact path, to have served.

test_scripted: a checkpoint at the start and after each of the 15 steps. List sizes after each
step (lists 0..7; rows, arena blocks), pinned on the CPU by test_lifecycle_model.py.
dim 30 L2:
    start                     167 270 499 122 251 153 699 339   2500 42
    1   empty a list          167 270 499   0 251 153 699 339   2378 40
    2a  trim to 65 and 2        2 270 499   0 251  65 699 339   2125 37
    2b  65 -> 64, 2 -> 1        1 270 499   0 251  64 699 339   2123 36
    3   remove nothing        (unchanged)
    4   add at the edges       71 270 499  70 251  65 699 339   2264 40
    5   upsert, replace only   71 270 499  70 251 165 599 339   2264 40
    6   upsert with repeats    78 277 500  78 251 166 604 340   2294 40
    7a  remove 60 %, toggle    30  96 195  34 103  56 257 147    918 19
    7b  add back              161 347 586 157 299 166 858 420   2994 51
    7c  toggle                (unchanged)
    8a  20 ids stored twice   164 348 590 162 301 167 860 422   3014 51
    8b  remove one of them    164 348 589 161 301 167 860 422   3012 51
    9   new centroids         (unchanged)
    10a save, load            (unchanged)
    10b remove after load     154 328 552 152 288 158 826 403   2861 49
dim 30 CosineDistance:
    start                     335 291 280 329 359 317 236 353   2500 43
    1   empty a list          335 291 280 329 359 317   0 353   2264 39
    2a  trim to 65 and 2      335   2  65 329 359 317   0 353   1760 32
    2b  65 -> 64, 2 -> 1      335   1  64 329 359 317   0 353   1758 31
    3   remove nothing        (unchanged)
    4   add at the edges      335  71  65 329 359 317  70 353   1899 35
    5   upsert, replace only  335  71 165 329 259 317  70 353   1899 35
    6   upsert with repeats   334  79 167 334 263 313  79 360   1929 35
    7a  remove 60 %, toggle   131  31  62 112 115 148  30 143    772 16
    7b  add back              356 294 240 358 392 356 210 423   2629 45
    7c  toggle                (unchanged)
    8a  20 ids stored twice   359 298 241 358 397 361 211 424   2649 45
    8b  remove one of them    359 298 241 357 396 361 211 424   2647 45
    9   new centroids         (unchanged)
    10a save, load            (unchanged)
    10b remove after load     344 279 227 339 376 345 201 403   2514 44
dim 200 InnerProduct:
    start                     336 233 328 340 251 359 338 315   2500 43
    1   empty a list          336   0 328 340 251 359 338 315   2267 39
    2a  trim to 65 and 2      336   0 328 340  65 359 338   2   1768 33
    2b  65 -> 64, 2 -> 1      336   0 328 340  64 359 338   1   1766 32
    3   remove nothing        (unchanged)
    4   add at the edges      336  70 328 340  65 359 338  71   1907 36
    5   upsert, replace only  336  70 328 340 165 259 338  71   1907 36
    6   upsert with repeats   333  76 328 342 164 264 346  84   1937 36
    7a  remove 60 %, toggle   131  37 123 141  66 115 132  30    775 17
    7b  add back              428 215 375 366 223 349 393 288   2637 45
    7c  toggle                (unchanged)
    8a  20 ids stored twice   428 220 377 368 225 349 399 291   2657 45
    8b  remove one of them    428 220 377 368 225 348 398 291   2655 45
    9   new centroids         (unchanged)
    10a save, load            (unchanged)
    10b remove after load     409 207 361 344 213 331 383 274   2522 44

test_walk: every operation once in a seeded order, then four seeded draws (lifecycle_model.walk_ops).

Wall time per case on the MI355X (pytest --durations=0, one run, the first case carries the
library's start-up): test_scripted dim 30 L2 3.4 s (int8, first) and 1.9 s (bf16), dim 30
CosineDistance 1.5 s and 1.5 s, dim 200 InnerProduct 2.4 s and 2.3 s; test_walk L2 1.1 s and
1.4 s, CosineDistance 0.9 s and 1.2 s; all ten 18 s.
"""
import numpy as np
import pytest

import lifecycle_model as lm
from conftest import load_vdb
from lifecycle_model import ABSENT, NLIST, NQ
from test_gpu_upsert import bits

vdb = load_vdb()
pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)
STATE = -5
SEARCHES = ((3, 10), (NLIST, 10), (2, 1024))
NP = 3  # nprobe of every filtered and range call


def same(got, want, what):
    assert got[0].shape == want[0].shape and got[1].dtype == np.uint64 and got[0].dtype == np.float32, what
    bad = np.argwhere(got[1] != want[1])
    assert bad.size == 0, f"{what}: ids differ at {bad[:3].tolist()}: {got[1][tuple(bad[0])]} model {want[1][tuple(bad[0])]}"
    badd = np.argwhere(bits(got[0]) != bits(want[0]))
    assert badd.size == 0, f"{what}: distance bits differ at {badd[:3].tolist()}"


def same_range(got, want, what):
    assert got[0].tolist() == want[0].tolist(), f"{what}: lims differ"
    same((got[1], got[2]), (want[1], want[2]), what)


class Run:
    """The handle, the model, and what the next checkpoint must expect."""

    def __init__(self, dim, metric, i8, tmp_path):
        X, Q, ids, C = lm.fixture(dim)
        self.dim, self.metric, self.i8, self.Q, self.tmp = dim, metric, i8, Q, tmp_path
        self.m = lm.Model(dim, NLIST, metric, C)
        self.g = self.handle()
        self.g.centroids = C
        self.m.add(X, ids)
        self.g.add(X, ids)
        self.live = False  # a live screen describes the lists and centroids
        self.moved = True  # rows may have moved since the last checkpoint's filters were prepared
        self.gone = np.zeros(0, np.uint64)  # ids removed since the last checkpoint
        self.filters = None  # the last checkpoint's {name: (Filter, spec)}
        self.rng = np.random.RandomState(99)

    def handle(self):
        g = vdb.IVFFlatIndex(vdb.IVFFlatIndex.Config(self.dim, NLIST, vdb.Metric(self.metric)))
        g.set_option("screen_i8", self.i8)
        g.set_option("screen_floor_ppm", 0)  # the screen always serves
        return g

    def shadow(self):
        return self.g.profile_read()["screen_shadow"]

    def apply(self, op, what):
        g, kind = self.g, op[0]
        want = lm.apply(self.m, op)
        if kind == "remove":
            shadow = self.shadow()
            got = g.remove_ids(op[1])
            assert got == want, f"{what}: remove_ids returned {got}, model {want}"
            if got:
                self.live, self.moved = False, True
                self.gone = np.concatenate([self.gone, lm.u64(op[1])])
            else:  # nothing matched: the handle, its screen and its filters are untouched
                assert self.shadow() == shadow, what
        elif kind == "add":
            g.add(op[1], op[2])
            self.live, self.moved = False, True
        elif kind == "add_to_lists":
            g.add_to_lists(op[1], op[2], op[3])
            self.live, self.moved = False, True
        elif kind == "upsert":
            got = g.upsert(op[1], op[2])
            assert got == want, f"{what}: upsert returned {got}, model {want}"
            self.live, self.moved = False, True
        elif kind == "centroids":
            g.centroids = op[1]
            assert np.array_equal(bits(g.centroids), bits(self.m.C)), what
            self.live = False
        elif kind == "toggle":  # (set_option builds the screen in the new format at once)
            self.i8 ^= 1
            g.set_option("screen_i8", self.i8)
            self.live = True
            assert self.shadow() == (2 if self.i8 else 1), what
        else:
            assert kind == "saveload"
            path = str(self.tmp / "lifecycle.ivf")
            g.save(path)
            self.g = self.handle()
            self.g.load(path)
            assert np.array_equal(bits(self.g.centroids), bits(self.m.C)), what
            self.live, self.moved, self.filters = False, True, None


# ---- the checkpoint ----
def check_state(run, what):
    g, m = run.g, run.m
    assert g.get_total_vectors() == m.total, what
    assert g.list_sizes().tolist() == m.sizes(), what
    for l in range(NLIST):
        gv, gi = g.get_list(l)
        mv, mi = m.lists[l]
        assert np.array_equal(gi, mi), f"{what}: list {l}: ids or their order differ"
        assert np.array_equal(bits(gv), bits(mv)), f"{what}: list {l}: row bits differ"


def id_request(run):
    """Stored, absent, twice-stored and just-removed ids, mixed."""
    stored = np.unique(run.m.stored_ids())
    req = np.concatenate([run.rng.permutation(stored)[:24], ABSENT, run.m.twice()[:8], run.gone[:8]])
    return req[run.rng.permutation(len(req))]


def check_fetch(run, req, what):
    V, F = run.g.fetch_ids(req)
    Vm, Fm = run.m.fetch(req)
    assert np.array_equal(F, Fm), f"{what}: fetch_ids: found differs"
    assert np.array_equal(bits(V), bits(Vm)), f"{what}: fetch_ids: row bits differ"
    if len(run.gone):
        gone = np.isin(req, run.gone) & ~np.isin(req, run.m.stored_ids())
        assert not F[gone].any(), f"{what}: fetch_ids found a removed id"


def refused(call, what):
    with pytest.raises(vdb.VdbError) as e:
        call()
    assert e.value.code == STATE, f"{what}: a stale filter was refused with {e.value.code}"


def check_old_filters(run, what):
    if run.filters is None:
        return
    g, Q = run.g, run.Q
    flts = [f for f, _ in run.filters.values()]
    fo = np.arange(NQ, dtype=np.uint32) % len(flts)
    if run.moved:
        assert all(f.stale for f in flts), f"{what}: a filter outlived moved rows"
        f = flts[0]
        for screen in (False, True):
            refused(lambda: g.search_prepared(Q, f, nprobe=NP, k=10, screen=screen), what)
            refused(lambda: g.search_prepared_multi(Q, flts, fo, nprobe=NP, k=10, screen=screen), what)
            refused(lambda: g.range_search_prepared(Q, f, 1.0, nprobe=NP, screen=screen), what)
    else:
        assert not any(f.stale for f in flts), f"{what}: a filter went stale though no row moved"
        room = max(1, run.m.probed_rows(Q, NP))
        for name, (f, spec) in run.filters.items():
            want = run.m.search_allowed(Q, NP, 10, *spec)
            same(g.search_prepared(Q, f, nprobe=NP, k=10), want, f"{what}: kept filter {name}")
            same(g.search_prepared(Q, f, nprobe=NP, k=10, screen=True, reserve=room), want, f"{what}: kept filter {name} screened")
            served(g.filter_screen_last_timing(), run.live, f"{what}: kept filter {name}")


def fresh_filters(run, what):
    """{name: (Filter, (ids, include) for the model)}: three prepared, two combined."""
    g, m, r = run.g, run.m, run.rng
    stored = np.unique(m.stored_ids())
    big = int(np.argmax(m.sizes()))
    spec = {"excl": (np.concatenate([r.permutation(stored)[:len(stored) // 2], ABSENT]), False),
            "inc2": (r.permutation(stored)[:max(1, len(stored) // 50)], True),
            "list": (m.lists[big][1].copy(), True)}
    out = {n: (g.prepare_filter(ids, include=inc), (ids, inc)) for n, (ids, inc) in spec.items()}
    allowed = {n: m.allowed_ids(*s) for n, s in spec.items()}
    out["and"] = (out["excl"][0] & out["list"][0], (np.intersect1d(allowed["excl"], allowed["list"]), True))
    out["andnot"] = (out["excl"][0].andnot(out["inc2"][0]), (np.setdiff1d(allowed["excl"], allowed["inc2"]), True))
    for n, (f, s) in out.items():
        assert f.allowed == m.allowed_count(*s), f"{what}: filter {n} allows {f.allowed}, model {m.allowed_count(*s)}"
        assert not f.stale, f"{what}: filter {n} is stale as prepared"
    assert 0 < out["and"][0].allowed < out["list"][0].allowed, f"{what}: a & b allows {out['and'][0].allowed}"
    return out


def served(st, screen, what, tiles=False):
    """The screened call's record: the screen served everything, or the exact path did."""
    if tiles:
        ok = (st["exact_tiles"] == 0 and st["screened_tiles"] == 2) if screen else (st["screened_tiles"] == 0 and st["exact_tiles"] > 0)
    else:
        ok = (st["exact_batches"] == 0 and st["screened_batches"] > 0) if screen else (st["screened_batches"] == 0 and st["exact_batches"] > 0)
    assert ok, f"{what}: expected the {'screen' if screen else 'exact path'} to serve: {st}"


def check_side_routes(run, flts, screen, what, full):
    """The four screened side routes, exact and with screen=True, against the model. `screen`:
    whether the screen must have served. full: every k and radius of the live phase."""
    g, m, Q = run.g, run.m, run.Q
    room = max(1, m.probed_rows(Q, NP))  # every probed (query, row) pair: no candidate buffer overflows
    names = list(flts)
    # search_prepared
    for k in ((1, 10, 64) if full else (10,)):
        for n in (names if full and k == 10 else ["excl"]):
            f, spec = flts[n]
            w = f"{what}: search_prepared {n} k {k}"
            want = m.search_allowed(Q, NP, k, *spec)
            same(g.search_prepared(Q, f, nprobe=NP, k=k), want, w)
            same(g.search_prepared(Q, f, nprobe=NP, k=k, screen=True, reserve=room), want, w + " screened")
            served(g.filter_screen_last_timing(), screen, w)
    # search_prepared_multi: 40 queries under the 5 filters, shuffled
    fo = run.rng.permutation(np.arange(NQ, dtype=np.uint32) % len(names)).astype(np.uint32)
    tab = [flts[n][0] for n in names]
    want = m.search_multi(Q, NP, 10, [flts[n][1] for n in names], fo)
    w = f"{what}: search_prepared_multi"
    same(g.search_prepared_multi(Q, tab, fo, nprobe=NP, k=10), want, w)
    same(g.search_prepared_multi(Q, tab, fo, nprobe=NP, k=10, screen=True, reserve=room), want, w + " screened")
    served(g.filter_screen_last_timing(), screen, w)
    # range_search and range_search_prepared
    allD = np.concatenate([D for D, _ in m.full(Q, NP)])
    radii = {"median": np.float32(np.median(allD))}
    if full:
        radii.update({"inf": INF, "below": np.nextafter(allD.min(), -INF, dtype=np.float32)})
    f, spec = flts["excl"]
    for rn, r in radii.items():
        w = f"{what}: range_search {rn}"
        want = m.range(Q, NP, r)
        same_range(g.range_search(Q, r, nprobe=NP), want, w)
        same_range(g.range_search(Q, r, nprobe=NP, screen=True, reserve=room), want, w + " screened")
        served(g.range_screen_last_timing(), screen, w)
        if rn == "below":
            assert want[1].size == 0, f"{w}: the model finds rows below every distance"
        if rn == "inf":
            assert want[1].size > 0, f"{w}: the model finds nothing"
        w = f"{what}: range_search_prepared {rn}"
        want = m.range(Q, NP, r, spec)
        same_range(g.range_search_prepared(Q, f, r, nprobe=NP), want, w)
        same_range(g.range_search_prepared(Q, f, r, nprobe=NP, screen=True, reserve=room), want, w + " screened")
        served(g.range_screen_last_timing(), screen, w)
    # search_exhaustive
    for k in ((10, 64) if full else (10,)):
        w = f"{what}: search_exhaustive k {k}"
        want = m.exhaustive(Q, k)
        same(g.search_exhaustive(Q, k), want, w)
        same(g.search_exhaustive(Q, k, screen=True, reserve=m.total), want, w + " screened")
        st = g.exhaustive_screen_last_timing()
        served(st, screen, w, tiles=True)
        if screen:
            assert st["rows_bounded"] == NQ * m.total, f"{w}: {st}"


def checkpoint(run, name):
    g, m, Q = run.g, run.m, run.Q
    fmt = 2 if run.i8 else 1
    # ---- stale: before any plain search ----
    what = f"{name} [stale]"
    check_state(run, what)
    req = id_request(run)
    check_fetch(run, req, what)
    check_old_filters(run, what)
    flts = fresh_filters(run, what)
    if run.live:
        assert run.shadow() == fmt, what
    check_side_routes(run, flts, run.live, what, full=False)
    # ---- one plain search builds the screen ----
    what = f"{name} [search]"
    same(g.search(Q, nprobe=3, k=10), m.search(Q, 3, 10), what)
    assert run.shadow() == fmt, f"{what}: screen_shadow {run.shadow()}, asked for {fmt}"
    # ---- live ----
    what = f"{name} [live]"
    assert not any(f.stale for f, _ in flts.values()), f"{what}: the rebuild made a filter stale"
    for nprobe, k in SEARCHES:
        g.set_option("bounded_stats", 1)  # (statistics only: counts the blocks the screened scan bounds)
        g.profile_reset()
        got = g.search(Q, nprobe=nprobe, k=k)
        p = g.profile_read()
        g.set_option("bounded_stats", 0)
        same(got, m.search(Q, nprobe, k), f"{what}: search {nprobe}, {k}")
        if k <= 64:  # (k 1024 is the exact scan's; search_filtered and search_ids are compared only)
            assert p["bounded_blocks"] > 0, f"{what}: search {nprobe}, {k}: the screen did not serve: {p}"
    ids, inc = flts["excl"][1]
    same(g.search_filtered(Q, ids=ids, include=inc, nprobe=NP, k=10), m.search_allowed(Q, NP, 10, ids, inc),
         f"{what}: search_filtered")
    check_side_routes(run, flts, True, what, full=True)
    D, I, F = g.search_ids(req, nprobe=3, k=10)
    Dm, Im, Fm = m.search_ids(req, 3, 10)
    assert np.array_equal(F, Fm), f"{what}: search_ids: found differs"
    same((D, I), (Dm, Im), f"{what}: search_ids")
    check_state(run, what)  # (reads leave the lists as they were, now from the row-major copy)
    assert run.shadow() == fmt, what
    run.live, run.moved, run.filters, run.gone = True, False, flts, np.zeros(0, np.uint64)


def drive(run, steps, sizes=None):
    checkpoint(run, "start")
    for n, (name, ops) in enumerate(steps, 1):
        for op in ops:
            run.apply(op, name)
        assert run.g.list_sizes().tolist() == run.m.sizes(), name
        if sizes is not None:
            assert run.m.sizes() == sizes[n], f"{name}: the step missed its edge: {run.m.sizes()}"
        checkpoint(run, name)
    return n


@pytest.mark.parametrize("i8", [1, 0])
@pytest.mark.parametrize("dim,metric", [(30, 0), (30, 3), (200, 1)])
def test_scripted(dim, metric, i8, tmp_path):
    run = Run(dim, metric, i8, tmp_path)
    sizes = lm.SCRIPT_SIZES[(dim, metric)]
    assert run.m.sizes() == sizes[0], f"start: {run.m.sizes()}"
    steps = drive(run, lm.scripted(run.m, dim), sizes)
    assert steps == len(sizes) - 1, f"{steps} steps ran"


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("dim,metric", [(30, 0), (30, 3)])
def test_walk(dim, metric, seed, tmp_path):
    run = Run(dim, metric, 1, tmp_path)
    steps = drive(run, lm.walk(run.m, dim, seed))
    assert steps == lm.WALK_STEPS, f"seed {seed}: {steps} steps ran"
