"""CPU test of the coarse contract's restatement (coarse_ref.py) on a numpy stand-in for the
kernels: numpy's fp32 matmul in place of the MFMA sum, the bound and the selection written out in
fp32 as the kernels write them. The stand-in must pass every clause in every regime, and the
restatement must catch a stand-in that is subtly wrong (a halved coefficient, a neighbour's norm,
a lost half of the sum, a selection by the wrong threshold)."""
import numpy as np
import pytest

import coarse_ref as cr

F = np.float32
DIM, NLIST, N, P = 80, 333, 17, 8


def stand_in(metric, dp, Q, C, P, k_coef=4.0, q_norm_shift=0, drop_half=False, tau_rank=None):
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        qn = (Q * Q).sum(axis=1, dtype=F)
        cn = (C * C).sum(axis=1, dtype=F)
        if q_norm_shift:
            qn = qn[np.arange(len(qn)) ^ 1]  # (an even number of rows) the neighbouring row's norm
        h = Q.shape[1] // 2
        dot = (Q[:, :h] @ C[:, :h].T) if drop_half else (Q @ C.T)
        K = F(k_coef) * F(dp + 4) * F(5.9604645e-8)
        qa, ca = np.sqrt(qn)[:, None], np.sqrt(cn)[None, :]
        if metric == cr.L2:
            ap = (qn[:, None] + cn[None, :]) - F(2) * dot
            dl = K * ((qa + ca) * (qa + ca)) + F(1e-30)
        else:
            ap = -dot
            dl = K * (qa * ca) + F(1e-30)
        ap, dl = ap.astype(F), dl.astype(F)
        if tau_rank is None:
            mask = cr.cand_ref(ap, dl, P)
        else:  # the threshold from the wrong rank of the sorted upper bounds
            tau = np.sort(cr.upper(ap, dl), axis=1)[:, tau_rank]
            mask = ~((ap - dl) > tau[:, None])
    cand = np.full(ap.shape, cr.NONE, np.uint32)
    d = cr.d_seq(metric, Q, C)
    probes = np.empty((len(Q), P), np.uint32)
    for i in range(len(Q)):
        ids = np.flatnonzero(mask[i])[::-1]  # (any order)
        cand[i, :len(ids)] = ids
        dd = cr.nan_last(d[i, ids])
        probes[i] = ids[np.lexsort((ids, dd))][:P]
    return ap, dl, cand, probes, d


def run_checks(metric, dp, Q, C, nan_rows, ap, dl, cand, probes, d):
    snap = {"approx": ap, "delta": dl, "cand": cand, "probes": probes, "assign": cr.assign_ref(d)}
    return cr.violations(metric, dp, Q, C, d, snap, P, nan_rows)


def clauses(V):
    return sorted({v.split(":")[0] for v in V})


@pytest.mark.parametrize("metric", [cr.L2, cr.IP])
@pytest.mark.parametrize("name", cr.REGIMES)
def test_stand_in_meets_every_clause(metric, name):
    C, Q, nan_rows = cr.regime(name, *cr.base(DIM, NLIST, N, seed=3))
    dp = cr.padded_dim(DIM)
    assert run_checks(metric, dp, Q, C, nan_rows, *stand_in(metric, dp, Q, C, P)) == []


@pytest.mark.parametrize("metric", [cr.L2, cr.IP])
def test_wrong_stand_ins_are_caught(metric):
    dp = cr.padded_dim(DIM)
    C, Q, nan_rows = cr.regime("mixed", *cr.base(DIM, NLIST, N + 1, seed=3))

    def run(**kw):
        return clauses(run_checks(metric, dp, Q, C, nan_rows, *stand_in(metric, dp, Q, C, P, **kw)))

    assert run(k_coef=2.0) == ["clause 2 (bound shrunk)"]
    assert run(k_coef=4.001) == ["clause 2 (bound loosened)"]
    assert "clause 2 (bound shrunk)" in run(q_norm_shift=1)
    C, Q, nan_rows = cr.regime("plain", *cr.base(DIM, NLIST, N, seed=3))
    assert "clause 1 (sound)" in run(drop_half=True)  # (and the probes it then loses: clause 4)
    assert "clause 3 (candidates)" in run(tau_rank=0)
    assert run(q_norm_shift=0) == []


def test_restated_selection_edges():
    inf, nan = F(np.inf), F(np.nan)
    d = np.array([[nan, 2, inf, 2, 1], [nan, nan, nan, nan, nan], [inf, inf, inf, inf, inf]], F)
    assert cr.probes_ref(d, 5).tolist() == [[4, 1, 3, 0, 2], [0, 1, 2, 3, 4], [0, 1, 2, 3, 4]]
    assert cr.assign_ref(d).tolist() == [4, 0, 0]
    # tau, one register: the P-th smallest of the minima by list % 256, not of all upper bounds
    ap = np.full((1, 600), 10, F)
    ap[0, 3], ap[0, 259], ap[0, 515], ap[0, 7] = 1, 2, 3, 5
    dl = np.zeros((1, 600), F)
    assert cr.tau_ref(ap, dl, 1)[0] == 1 and cr.tau_ref(ap, dl, 2)[0] == 5 and cr.tau_ref(ap, dl, 3)[0] == 10
    assert cr.tau_ref(ap, dl, 65)[0] == 10 and cr.tau_ref(ap, dl[:, :600], 600)[0] == 10
    assert cr.cand_ref(ap, dl, 2)[0].sum() == 4
    # a malformed candidate row is named
    cand = np.full((1, 6), cr.NONE, np.uint32)
    cand[0, :3] = [2, 4, 2]
    with pytest.raises(AssertionError, match="listed twice"):
        cr.cand_sets(cand, 6)
    cand[0, :3] = [2, 6, 1]
    with pytest.raises(AssertionError, match=">= nlist"):
        cr.cand_sets(cand, 6)
    cand[0, :4] = [2, cr.NONE, 1, cr.NONE]
    with pytest.raises(AssertionError, match="after the end mark"):
        cr.cand_sets(cand, 6)
