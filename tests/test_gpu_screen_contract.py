"""GPU check of the deferred screened scan's contract (screen.hip, screen_post.hip) on a
snapshot of one batch's buffers (IVFFlatIndex.screen_snapshot), clause by clause
(screen_ref.check_snapshot): the shadow and the norms the build wrote, the pair rows, every
collected lower bound, the well-formedness of every reserved candidate entry (the host-side
range check of the slots), the required and the allowed candidate sets, the thresholds and the
select chain. The end-to-end parity tests cannot see a collect that stopped pruning or wrote a
wrong slot that happened not to matter; this one names the promise that broke.

One fixture (screen_ref.contract_fixture): a hub list of 31 full blocks and one of 5 vectors,
lists of 64, 65, 1 and 0 vectors, 40 queries probing every list: items of 16 + 16 + 8 queries at
screen_group 16 and of 32 + 8 at 32. The dims make every instantiation launch_screen_collect can
pick run once per metric (KD = 1, 2, 4, 6 int8; 2, 4, 8 bf16)."""
import numpy as np
import pytest

import screen_ref as sr
from conftest import load_vdb
from test_gpu_bounded import assert_same, lists_pair

vdb = load_vdb()
pytestmark = pytest.mark.gpu

NPROBE = 5
CASES = [(1, 64), (1, 100), (1, 256), (1, 384), (0, 64), (0, 128), (0, 256)]  # (screen_i8, D)
# (screen_group, k, seg_vectors): every k and both segment sizes at both item widths
RUNS = [(16, 10, 0), (16, 1, 64), (16, 64, 64), (32, 10, 64), (32, 1, 0), (32, 64, 0)]


def handle(fx, metric, i8):
    g, o = lists_pair(fx["X"], fx["ids"], fx["assign"], fx["C"], metric)
    g.set_option("screen_i8", i8)
    g.set_option("screen_floor_ppm", 0)
    g.set_batch(64)
    return g, o


def run(g, fx, k, group=16, seg=0):
    g.set_option("screen_group", group)
    if getattr(g, "_seg", None) != seg:  # (a change rebuilds the directory and the shadow)
        g.set_option("seg_vectors", seg)
        g._seg = seg
    D, I = g.search(fx["Q"], nprobe=NPROBE, k=k)
    return D, I, g.screen_snapshot()


def violations(snap, fx, metric, **kw):
    return sr.check_snapshot(snap, fx["lists"], fx["C"], fx["Q"], metric, **kw)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("i8,dim", CASES)
def test_contract_holds(metric, i8, dim):
    fx = sr.contract_fixture(dim, seed=dim + metric)
    g, o = handle(fx, metric, i8)
    ref = {k: o.search(fx["Q"], NPROBE, k) for k in (1, 10, 64)}
    tight = 0.0
    for group, k, seg in RUNS:
        D, I, snap = run(g, fx, k, group, seg)
        assert (snap["i8"], snap["wide_q"], snap["k"], snap["B"], snap["P"]) == (i8, group, k, 40, NPROBE)
        assert snap["dp"] == (dim + 63) // 64 * 64 and (seg == 0 or snap["seg_blocks"] == 1)
        st = {}
        V = violations(snap, fx, metric, stats=st)
        assert V == [], (group, k, seg, V[:6])
        assert not snap["ovf"].any() and snap["counters"][sr.CTR_OVF] == 0
        assert_same(D, I, *ref[k])
        tight = max(tight, st["tight"])
    print("screen bound tightness (d_ref - lb) / (2 del), worst: %s D=%d metric=%d: %.4f" %
          ("int8" if i8 else "bf16", dim, metric, tight))


def test_snapshot_does_not_depend_on_the_recheck_and_changes_nothing():
    fx = sr.contract_fixture(64, seed=5)
    g, o = handle(fx, 0, 1)
    snaps = []
    for r2 in (1, 0):
        g.set_option("screen_recheck2", r2)
        D, I, snap = run(g, fx, 10)
        assert violations(snap, fx, 0) == []
        assert_same(D, I, *o.search(fx["Q"], NPROBE, 10))
        snaps.append(snap)
    nv = int(snaps[0]["counters"][sr.CTR_VALID])  # (sorted pairs past the valid ones are never written)
    assert nv == 160 and np.array_equal(snaps[0]["sorted_pair"][:nv], snaps[1]["sorted_pair"][:nv])
    for name in ("probes", "pst", "qscale", "qres", "block_off", "count", "meta", "sscale", "shadow"):
        assert np.array_equal(snaps[0][name].view(np.uint8), snaps[1][name].view(np.uint8)), name
    g.set_option("screen_recheck2", 1)
    # a snapshot between two searches: the second one's results and counters are what they are without it
    ints = [f for f, t in vdb.Profile._fields_ if "int" in t.__name__]
    out = []
    for take in (False, True):
        g.search(fx["Q"], nprobe=NPROBE, k=10)
        if take:
            g.screen_snapshot()
        g.profile_reset()
        D, I = g.search(fx["Q"], nprobe=NPROBE, k=10)
        p = g.profile_read()
        out.append((D, I, {f: p[f] for f in ints}))
    assert_same(out[0][0], out[0][1], out[1][0], out[1][1])
    assert out[0][2] == out[1][2]


def test_other_routes_are_refused():
    fx = sr.contract_fixture(64, seed=6, hub_blocks=3)
    g, o = handle(fx, 0, 1)
    g.set_option("screen", 0)
    g.search(fx["Q"], nprobe=NPROBE, k=10)
    with pytest.raises(Exception, match="deferred screened route"):
        g.screen_snapshot()
    g.set_option("screen", 1)
    g.search(fx["Q"], nprobe=NPROBE, k=10)
    assert g.screen_snapshot()["B"] == 40


@pytest.mark.parametrize("metric", [0, 1])
def test_special_rows(metric):
    """A zero vector, a vector equal to its centroid (scale 0), a 3e38 entry, a +inf entry and a
    1e-41 row in the hub list, and an all-zero query. The non-finite rows have no finite bound:
    they are candidates of every pair that probes the list. (IP: the zero query against the +inf
    row is 0 x inf, a NaN distance, where the reference's ranking is undefined: that
    query is in the batch and in the contract check, but its results are not compared.)"""
    fx = sr.contract_fixture(100, seed=21, special=True)
    g, o = handle(fx, metric, 1)
    D, I, snap = run(g, fx, 10)
    V = violations(snap, fx, metric)
    assert V == [], V[:6]
    assert not snap["ovf"].any() and snap["counters"][sr.CTR_OVF] == 0
    n0 = len(fx["lists"][0])
    base = int(snap["block_off"][0]) * 64
    cand = snap["cand"]
    real = cand[cand[:, 0] != sr.NOID]
    nv = int(snap["counters"][sr.CTR_VALID])
    hub_pairs = [s for s in range(nv) if snap["probes"][(snap["sorted_pair"][s] >> 16) * NPROBE + (snap["sorted_pair"][s] & 0xFFFF)] == 0]
    assert len(hub_pairs) == 40
    for s in hub_pairs:
        slots = set(real[real[:, 0] == s][:, 1].tolist())
        assert base + n0 - 3 in slots and base + n0 - 2 in slots, s  # (the 3e38 and the +inf rows)
    keep = np.ones(40, bool)
    if metric == 1:
        keep[7] = False
    Dr, Ir = o.search(fx["Q"][keep], NPROBE, 10)
    assert_same(D[keep], I[keep], Dr, Ir)


@pytest.mark.parametrize("metric", [0, 1])
def test_ties_at_the_kth_distance(metric):
    fx = sr.contract_fixture(64, seed=31, ties=True)
    g, o = handle(fx, metric, 1)
    D, I, snap = run(g, fx, 10)
    V = violations(snap, fx, metric)
    assert V == [], V[:6]
    assert not snap["ovf"].any() and snap["counters"][sr.CTR_OVF] == 0
    assert_same(D, I, *o.search(fx["Q"], NPROBE, 10))
    if metric == 0:  # (L2: the copies are every query's nearest hub vectors, so all 200 tie at the k-th)
        base = int(snap["block_off"][0]) * 64
        copies = set(range(base + 100, base + 300))
        nv = int(snap["counters"][sr.CTR_VALID])
        n = 0
        for s in range(nv):
            pr = int(snap["sorted_pair"][s])
            if snap["probes"][(pr >> 16) * NPROBE + (pr & 0xFFFF)] != 0:
                continue
            d = sr.ref_dist(fx["Q"][pr >> 16], fx["lists"][0], 0)
            if np.sort(d)[9] != d[100]:
                continue
            o_, c_ = int(snap["soff"][s]), int(snap["scnt"][s])
            assert copies <= set(snap["surv"][o_:o_ + c_, 0].tolist()), s
            n += 1
        assert n > 0


@pytest.mark.parametrize("metric", [0, 1])
def test_overflow(metric):
    """screen_cand_cap = 1024 at k = 64: the buffer overflows. The marked pairs are recomputed
    exactly over their lists; every unmarked pair keeps the whole contract; nothing is written at
    or past the capacity (the slot's allocation beyond it, left by earlier batches with room,
    is unchanged)."""
    fx = sr.contract_fixture(64, seed=41)
    g, o = handle(fx, metric, 1)
    tails = {}
    for _ in range(8):  # (until every workspace slot has served a batch with room)
        D, I, snap = run(g, fx, 64)
        if snap["slot"] in tails:
            break
        assert snap["cand_alloc"] >= snap["counters"][sr.CTR_CAND] > 1024
        tails[snap["slot"]] = g.screen_snapshot_raw("cand_alloc", np.uint32).reshape(-1, 4)
    else:
        pytest.fail("the workspace slots never repeated")
    g.set_option("screen_cand_cap", 1024)
    D, I, snap = run(g, fx, 64)
    ctr = snap["counters"]
    assert snap["cand_cap"] == 1024 and ctr[sr.CTR_OVF] == 1 and snap["ovf"].any()
    assert len(snap["cand"]) == 1024
    after = g.screen_snapshot_raw("cand_alloc", np.uint32).reshape(-1, 4)
    before = tails[snap["slot"]]
    assert len(after) == len(before) and np.array_equal(after[1024:], before[1024:])
    assert ctr[sr.CTR_REAL] >= (snap["cand"][:, 0] != sr.NOID).sum()
    V = violations(snap, fx, metric, allow_overflow=True)
    assert V == [], V[:6]
    assert_same(D, I, *o.search(fx["Q"], NPROBE, 64))
