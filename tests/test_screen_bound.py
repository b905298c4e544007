"""CPU check of the screened scan's distance bound (screen.hip).

The screen computes approx = |a|^2 + |b|^2 - 2 <a', b'> (L2; a = q - c, b = x - c, primes =
bf16 rounding) from fp32 norms and an f32 accumulation of exact bf16 products, and prunes a
pair only when approx - delta exceeds a threshold. Exactness rests on |d_ref - approx| <= delta
for the reference's own fp32 distance d_ref (ivf_flat_index.cpp:352-362: diff = q - x rounded,
diff * diff rounded, acc + term rounded, d = 0..D-1). This test restates the kernel's arithmetic
in numpy float32 (bf16 round-to-nearest-even with subnormals flushed, norms from float64 sums
rounded as the kernel rounds them, the accumulation in two different orders) and checks the
bound on random and adversarial data: iid Gaussian, tight clusters far from the origin, mixed
magnitudes, vectors right at the centroid, and IP.
"""
import numpy as np
import pytest

from screen_ref import (U, bf16, bounds_from_dot, build_restated, f32_dot, pairs_restated, pair_bounds, ref_dist,  # noqa: F401
                        ru, screen_bound)


CASES = {
    "iid": lambda r, d: (r.standard_normal(d), 0.2 * r.standard_normal(d), r.standard_normal((400, d))),
    "clustered": lambda r, d: (
        (c := 30.0 * np.ones(d) / np.sqrt(d) + r.standard_normal(d)) + 0.05 * r.standard_normal(d),
        c, c + 0.05 * r.standard_normal((400, d))),
    "far_ball_centroid_at_origin": lambda r, d: (
        (c := 100.0 * np.ones(d) / np.sqrt(d)) + 0.01 * r.standard_normal(d), 0.0 * c,
        c + 0.01 * r.standard_normal((400, d))),
    "mixed_scales": lambda r, d: (
        r.standard_normal(d) * np.exp(r.uniform(-20, 20, d)), r.standard_normal(d),
        r.standard_normal((400, d)) * np.exp(r.uniform(-20, 20, (400, d)))),
    "at_centroid": lambda r, d: ((c := r.standard_normal(d)), c, np.repeat(c[None], 400, 0)),
    "tiny": lambda r, d: (1e-20 * r.standard_normal(d), 1e-20 * r.standard_normal(d),
                          1e-20 * r.standard_normal((400, d))),
}


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("dim", [64, 768])
def test_screen_bound_holds(metric, case, dim):
    r = np.random.default_rng(dim + 7 * metric + sum(map(ord, case)))
    for _ in range(3):
        q, c, X = (np.asarray(v, np.float32) for v in CASES[case](r, dim))
        d = ref_dist(q, X, metric)
        for order in ("seq", "pairwise"):
            approx, dl = screen_bound(q, c, X, metric, order)
            lo = (approx - dl).astype(np.float32)
            hi = (approx + dl).astype(np.float32)
            bad = ~((lo <= d) & (d <= hi))
            assert not bad.any(), (case, order, float(d[bad][0]), float(approx[bad][0]), float(dl[bad][0]))


def test_screen_bound_is_tight_on_iid_768():
    """The bound is a small fraction of the distance spread on the headline's data (the
    reason the screen prunes): iid N(0,1), |a|, |b| ~ 28, distances spread by ~68."""
    r = np.random.default_rng(5)
    q, c, X = (np.asarray(v, np.float32) for v in CASES["iid"](r, 768))
    d = ref_dist(q, X, 0)
    approx, dl = screen_bound(q, c, X, 0, "seq")
    assert float(np.max(dl)) < 0.15 * float(np.std(d))
    assert float(np.max(np.abs(approx - d))) < float(np.min(dl))


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("dim", [64, 768])
def test_screen_bound_holds_int8(metric, case, dim):
    """The int8 shadow's bound (the default shadow on iid data): scale and codes as
    ivf_screen_build_i8 / ivf_screen_pairs_i8 make them, the integer dot exact, the epilogue one
    rounded fp32 operation at a time (screen_ref.pair_bounds): lb <= d_ref <= ub."""
    r = np.random.default_rng(dim + 7 * metric + sum(map(ord, case)) + 1000)
    for _ in range(3):
        q, c, X = (np.asarray(v, np.float32) for v in CASES[case](r, dim))
        d = ref_dist(q, X, metric)
        rows, sscale, meta = build_restated(X, c, True)
        arow, asc, ps = pairs_restated(q, c, metric, True)
        assert np.abs(rows.astype(int)).max() <= 127 and np.abs(arow.astype(int)).max() <= 127
        lo, hi, dl, tol = pair_bounds(arow, asc, ps, rows, sscale, meta, dim, metric, True)
        assert not tol.any()
        bad = ~((lo <= d) & (d <= hi))
        assert not bad.any(), (case, float(d[bad][0]), float(lo[bad][0]), float(hi[bad][0]))
