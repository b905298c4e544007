"""CPU self-test of the screened scan's contract checker (screen_ref.check_snapshot): the
sequential numpy model of the chain (screen_ref.model_snapshot) satisfies every clause at the
GPU test's fixture, for both shadow formats and metrics, and each fault planted into a copy of a
model snapshot is named by its own clause. This is the proof, without a GPU, that
test_gpu_screen_contract.py fails on a subtly wrong kernel."""
import copy

import numpy as np
import pytest

import screen_ref as sr

DIM, K = 64, 10
_cache = {}


def fixture():
    if "fx" not in _cache:
        _cache["fx"] = sr.contract_fixture(DIM, seed=11, hub_blocks=9)
    return _cache["fx"]


def model(metric, i8):
    key = (metric, i8)
    if key not in _cache:
        fx = fixture()
        _cache[key] = sr.model_snapshot(fx["lists"], fx["C"], fx["Q"], metric, K, i8, seg_blocks=8)
    return _cache[key]


def check(snap, metric=0):
    fx = fixture()
    return sr.check_snapshot(snap, fx["lists"], fx["C"], fx["Q"], metric)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("i8", [True, False])
def test_model_satisfies_the_contract(metric, i8):
    snap = model(metric, i8)
    assert snap["counters"][sr.CTR_REAL] > 0 and snap["counters"][sr.CTR_SURV] > 0
    # (the model prunes: far fewer candidates than (query, vector) pairs)
    assert snap["counters"][sr.CTR_REAL] < 0.5 * 40 * sum(len(x) for x in fixture()["lists"])
    st = {}
    fx = fixture()
    assert sr.check_snapshot(snap, fx["lists"], fx["C"], fx["Q"], metric, stats=st) == []
    assert 0.0 < st["tight"] <= 1.0


def test_layout_round_trip():
    r = np.random.default_rng(3)
    codes = r.integers(-127, 128, (128, 128)).astype(np.int8)
    assert np.array_equal(sr.decode_shadow(sr.encode_shadow(codes, True), 2, 128, True), codes)
    # lane l of k-step s, tile vt holds vector 16 vt + (l & 15), dims 64 s + 16 (l >> 4) ..
    raw = sr.encode_shadow(codes, True).view(np.int8).reshape(2, 2, 4, 64, 16)
    assert np.array_equal(raw[1, 1, 2, 37], codes[64 + 16 * 2 + (37 & 15), 64 + 16 * (37 >> 4):][:16])
    vals = sr.bf16(r.standard_normal((64, 64)).astype(np.float32))
    assert np.array_equal(sr.decode_shadow(sr.encode_shadow(vals, False), 1, 64, False), vals)
    rawb = sr.encode_shadow(vals, False).view(np.uint16).reshape(1, 2, 4, 64, 8)
    want = vals[16 * 3 + (21 & 15), 32 + 8 * (21 >> 4):][:8]
    assert np.array_equal((rawb[0, 1, 3, 21].astype(np.uint32) << 16).view(np.float32), want)
    f = np.array([-np.inf, -1.0, -0.0, 0.0, 1e-40, 2.5, np.inf], np.float32)
    assert np.array_equal(sr.ord_dec(sr.ord_enc(f)).view(np.uint32), f.view(np.uint32))
    assert (np.diff(sr.ord_enc(f).astype(np.int64)) >= 0).all() and sr.ord_enc(np.float32(np.inf)) == 0xFF800000


# ---- planted faults (int8, L2: bounds compare bit for bit) -----------------------------------
def pair_truth(s, sp):
    """(list, its first slot, d_ref of its vectors) of sorted pair sp."""
    fx = fixture()
    pr = int(s["sorted_pair"][sp])
    q, p = pr >> 16, pr & 0xFFFF
    l = int(s["probes"][q * s["P"] + p])
    return l, int(s["block_off"][l]) * 64, sr.ref_dist(sr.pad_dp(fx["Q"], s["dp"])[q], sr.pad_dp(fx["lists"][l], s["dp"]), 0)


def entry_of(s, sp, slot):
    return int(np.flatnonzero((s["cand"][:, 0] == sp) & (s["cand"][:, 1] == slot))[0])


def first_pad(s):
    return int(np.flatnonzero(s["cand"][:, 0] == sr.NOID)[0])


def restated_lb(s, sp):
    pr = int(s["sorted_pair"][sp])
    i = (pr >> 16) * s["P"] + (pr & 0xFFFF)
    l = int(s["probes"][i])
    sl = slice(int(s["block_off"][l]) * 64, int(s["block_off"][l]) * 64 + int(s["count"][l]))
    rows = sr.decode_shadow(s["shadow"], s["blocks"], s["dp"], True)
    qres = sr.decode_qres(s["qres"], s["B"] * s["P"], s["dp"], True)
    return sr.pair_bounds(qres[i], s["qscale"][i], s["pst"][i], rows[sl], s["sscale"][sl], s["meta"][sl], s["dp"], 0, True)[0]


def f_required_removed(s):
    l, o, d = pair_truth(s, 0)
    s["cand"][entry_of(s, 0, o + int(np.argmin(d)))] = (sr.NOID, 0, 0, sr.NOID)


def f_lb_one_ulp(s):
    j = int(np.flatnonzero((s["cand"][:, 0] != sr.NOID) & (s["cand"][:, 2].view(np.float32) > 0))[0])
    s["cand"][j, 2] += 1


def f_duplicate(s):
    s["cand"][first_pad(s)] = s["cand"][0]


def f_slot_past_list(s):
    l, o, d = pair_truth(s, 0)
    s["cand"][entry_of(s, 0, o + int(np.argmin(d))), 1] = o + len(d)


def f_garbage_entry(s):
    s["cand"][first_pad(s)] = (0x12345678, 7, 9, 3)


def f_real_off_by_one(s):
    s["counters"][sr.CTR_REAL] += 1


def f_admitted_above_u(s):
    l, o, d = pair_truth(s, 0)
    lb = restated_lb(s, 0)
    have = set(s["cand"][s["cand"][:, 0] == 0][:, 1].tolist())
    out = [i for i in range(len(d)) if o + i not in have and i >= 64]
    i = min(out, key=lambda i: lb[i])  # (the pruned vector nearest its threshold)
    s["cand"][first_pad(s)] = (0, o + i, lb[i:i + 1].view(np.uint32)[0], sr.NOID)
    s["counters"][sr.CTR_REAL] += 1


def f_thr_too_low(s):
    l, o, d = pair_truth(s, 0)
    s["thr"][0] = sr.ord_enc(np.nextafter(np.sort(d)[K - 1], np.float32(-np.inf)))


def f_ublist_unsorted(s):
    row = s["ublist"][0, 0]
    assert row[0] != row[K - 1]
    row[0], row[K - 1] = row[K - 1], row[0]


def f_survivor_dropped(s):
    a = int(s["soff"][0])
    s["surv"][a] = s["surv"][a + 1]


def f_survivor_wrong_run(s):
    a, b = int(s["soff"][0]), int(s["soff"][1])
    s["surv"][[a, b]] = s["surv"][[b, a]]


def f_soff_shifted(s):
    s["soff"][1:] += 1


def f_meta_z_low(s):
    s["meta"][5, 2] *= np.float32(0.5)


def f_code_flipped(s):
    rows = sr.decode_shadow(s["shadow"], s["blocks"], s["dp"], True).copy()
    d = int(np.argmax(np.abs(rows[5].astype(int))))
    rows[5, d] = -rows[5, d]
    s["shadow"] = sr.encode_shadow(rows, True)


FAULTS = [
    (f_required_removed, "5.required"), (f_lb_one_ulp, "3.bounds"), (f_duplicate, "4.entries"),
    (f_slot_past_list, "4.entries"), (f_garbage_entry, "4.entries"), (f_real_off_by_one, "4.entries"),
    (f_admitted_above_u, "6.allowed"), (f_thr_too_low, "7.thresholds"), (f_ublist_unsorted, "7.thresholds"),
    (f_survivor_dropped, "8.select"), (f_survivor_wrong_run, "8.select"), (f_soff_shifted, "8.select"),
    (f_meta_z_low, "1.build"), (f_code_flipped, "1.build"),
]
# (faults whose only consequence is their own clause: the checker must name nothing else)
ALONE = {f_lb_one_ulp, f_real_off_by_one, f_ublist_unsorted, f_duplicate, f_garbage_entry}


@pytest.mark.parametrize("fault,clause", FAULTS, ids=[f.__name__[2:] for f, _ in FAULTS])
def test_planted_fault_is_named_by_its_clause(fault, clause):
    s = copy.deepcopy(model(0, True))
    fault(s)
    V = check(s)
    assert any(v.startswith(clause) for v in V), V
    if fault in ALONE:
        assert all(v.startswith(clause) for v in V), V
