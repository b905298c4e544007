"""numpy restatement of Metric.CosineDistance's unit(row) (include/vdb_ivf.h), bit for bit, and
of its distance mapping. Shared by the cosine tests; no GPU, no package import."""
import numpy as np

NONE = np.iinfo(np.uint64).max


def unit_rows_ref(X):
    """unit(row) of every row of X: element i belongs to lane (i // 4) % 64; a lane adds the
    squares of its elements in ascending i (fp32 product, then fp32 sum); the 64 partials combine
    by p[l] += p[l + s], s = 32 .. 1; norm = sqrt; a finite norm > 0 divides the row, any other
    leaves it as it is."""
    X = np.ascontiguousarray(X, np.float32)
    n, d = X.shape
    dp = (d + 255) // 256 * 256
    P = np.zeros((n, dp), np.float32)
    P[:, :d] = X
    P = P.reshape(n, dp // 256, 64, 4)
    p = np.zeros((n, 64), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(dp // 256):
            for e in range(4):
                t = P[:, c, :, e]
                p = p + t * t
        s = 32
        while s:
            p = p[:, :s] + p[:, s:2 * s]
            s //= 2
        nrm = np.sqrt(p[:, 0])
    ok = np.isfinite(nrm) & (nrm > 0)
    out = X.copy()
    out[ok] = X[ok] / nrm[ok, None]
    return out


def cos_map(D, I):
    """An inner-product result's distances as CosineDistance reports them: 1.0f + d where the
    slot is filled."""
    D = np.ascontiguousarray(D, np.float32).copy()
    f = np.asarray(I) != NONE
    D[f] = np.float32(1) + D[f]
    return D
