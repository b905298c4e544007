"""numpy restatement of the coarse step's contract (kernels.hip: ivf_coarse_mfma, ivf_coarse_mfma2x2,
ivf_select_rerank, ivf_assign_rerank), clause by clause. No GPU, no package import.

The kernels promise, with u = 2^-24 and dp the padded dimension:
  |approx - exact| <= delta,  delta = 4 (dp + 4) u (|q| + |c|)^2 + 1e-30   (L2)
                              delta = 4 (dp + 4) u |q| |c| + 1e-30         (inner product)
where exact is the reference's sequential fp32 sum (oracle.np_ref.distances; zero pads do not
change it). The selection keeps every list whose lower bound fl(approx - delta) is not above tau,
the P-th smallest upper bound fl(approx + delta) as the kernel finds it, recomputes those exactly
and orders them by (distance, list), NaN last.

check_* raise AssertionError naming the clause, the row and the list."""
import numpy as np

from oracle import np_ref

L2, IP = 0, 1
U = 2.0 ** -24
FLOOR = 1e-30                      # the kernels' additive floor (1e-30f)
TERM_LO, TERM_HI = 2.0 ** -90, 2.0 ** 120   # where clause 2 pins delta to the stated bound
NONE = np.uint32(0xFFFFFFFF)

REGIMES = ("plain", "offset", "tiny", "huge", "mixed", "special")


def padded_dim(dim):
    return (dim + 63) // 64 * 64


def base(dim, nlist, n, seed):
    """The N(0,1) centroids and rows every regime starts from."""
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((nlist, dim)).astype(np.float32)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    return C, X


def regime(name, C, X):
    """(centroids, rows, nan_rows) of one regime, from the base. nan_rows: the rows holding a NaN."""
    C, X = C.copy(), X.copy()
    nan_rows = np.zeros(len(X), bool)
    with np.errstate(over="ignore"):
        if name == "offset":          # a common offset: the L2 expansion cancels
            C += np.float32(64.0)
            X += np.float32(64.0)
        elif name == "tiny":          # squares underflow below the 1e-30 floor
            C *= np.float32(2.0 ** -70)
            X *= np.float32(2.0 ** -70)
        elif name == "huge":          # norms overflow to inf
            C *= np.float32(2.0 ** 62)
            X *= np.float32(2.0 ** 62)
        elif name == "mixed":         # norms 2^40 apart inside one MFMA tile, in both operands
            X[0::2] *= np.float32(2.0 ** 20)
            X[1::2] *= np.float32(2.0 ** -20)
            C[0::3] *= np.float32(2.0 ** 20)
        elif name == "special":
            n, nl = len(X), len(C)
            X[0 % n] = 0.0
            if n > 1:
                X[1, X.shape[1] // 2] = np.nan
                nan_rows[1] = True
            if n > 2:
                X[2, 3] = np.inf
            if nl > 7:
                C[5] = 0.0
                C[nl - 1] = C[2]                                          # exact duplicates, far apart in id
                C[7] = C[6]
                C[7, 1:2] = (C[7, 1:2].view(np.int32) + 1).view(np.float32)   # 1 ulp from centroid 6
            if n > 4 and nl > 7:
                X[3] = C[2]     # a row on the duplicated pair: an exact tie at distance 0 (L2)
                X[4] = C[6]     # a row on the 1-ulp pair
        elif name != "plain":
            raise ValueError(name)
    return C, X, nan_rows


def d_seq(metric, Q, C):
    """The reference's sequential fp32 distances [n, nlist]."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return np_ref.distances(metric, Q, C)


def bound_term(metric, Q, C):
    """(|q| + |c|)^2 (L2) or |q| |c| (inner product) in float64 from float64 norms of the fp32 inputs."""
    with np.errstate(over="ignore", invalid="ignore"):
        qn = np.sqrt((np.asarray(Q, np.float64) ** 2).sum(axis=1))[:, None]
        cn = np.sqrt((np.asarray(C, np.float64) ** 2).sum(axis=1))[None, :]
        return (qn + cn) ** 2 if metric == L2 else qn * cn


def delta_ref(metric, dp, Q, C):
    with np.errstate(over="ignore", invalid="ignore"):
        return 4.0 * (dp + 4) * U * bound_term(metric, Q, C) + FLOOR


def upper(ap, dl):
    """fl(approx + delta) in fp32, NaN -> +inf (nan_last)."""
    with np.errstate(over="ignore", invalid="ignore"):
        ub = ap.astype(np.float32) + dl.astype(np.float32)
    return np.where(np.isnan(ub), np.float32(np.inf), ub)


def tau_ref(ap, dl, P):
    """tau per row as ivf_select_rerank finds it from its own approx and delta. P <= 64 (one
    register): the P-th smallest of the block's 256 lane minima, lane slot = list % 256 (a lane of
    wave w reads lists r0 + 256 j + lane with r0 = 64 w mod 256). P > 64: the P-th smallest upper
    bound."""
    ub = upper(ap, dl)
    n, nlist = ub.shape
    assert 1 <= P <= nlist
    if P <= 64:
        pad = np.full((n, (nlist + 255) // 256 * 256), np.inf, np.float32)
        pad[:, :nlist] = ub
        ub = pad.reshape(n, -1, 256).min(axis=1)
    return np.sort(ub, axis=1)[:, P - 1]


def cand_ref(ap, dl, P):
    """The candidate mask [n, nlist]: not (fl(approx - delta) > tau)."""
    tau = tau_ref(ap, dl, P)
    with np.errstate(over="ignore", invalid="ignore"):
        lb = ap.astype(np.float32) - dl.astype(np.float32)
        return ~(lb > tau[:, None])


def nan_last(d):
    return np.where(np.isnan(d), np.float32(np.inf), d)


def probes_ref(d, P):
    """select_nprobe per row of the distance matrix: ascending (distance, list), NaN ordered last
    (as +inf, so among lists without a number the lowest id goes first)."""
    d = nan_last(d)
    ids = np.arange(d.shape[1])
    return np.stack([np.lexsort((ids, row))[:P] for row in d]).astype(np.uint32)


def assign_ref(d):
    """assign per row: the first index of the minimum, NaN ordered last; a row without a finite
    distance goes to list 0."""
    return np.argmin(nan_last(d), axis=1).astype(np.uint32)


def cand_sets(cand, nlist):
    """Clause 3's form: row i = distinct lists < nlist, then NONE to the end. Returns the mask."""
    n = cand.shape[0]
    mask = np.zeros((n, nlist), bool)
    for i in range(n):
        row = cand[i]
        m = int(np.argmax(row == NONE)) if (row == NONE).any() else nlist
        assert (row[m:] == NONE).all(), f"clause 3 (form): row {i}: an entry after the end mark at {m}"
        head = row[:m]
        big = np.flatnonzero(head >= nlist)
        assert big.size == 0, f"clause 3 (form): row {i}: entry {big[:1]} is list {head[big[:1]]} >= nlist {nlist}"
        uq, cnt = np.unique(head, return_counts=True)
        assert (cnt == 1).all(), f"clause 3 (form): row {i}: list {int(uq[cnt > 1][0])} is listed twice"
        mask[i, head] = True
    return mask


def _first(bad):
    i, c = np.argwhere(bad)[0]
    return int(i), int(c)


def check_sound(ap, dl, dseq, cand_mask=None):
    """Clause 1. Returns the worst |approx - d_seq| / delta over the finite pairs."""
    fin = np.isfinite(ap) & np.isfinite(dl) & np.isfinite(dseq)
    a, d, e = ap.astype(np.float64), dl.astype(np.float64), dseq.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(a - e)
        bad = fin & ~(err <= d)
    if bad.any():
        i, c = _first(bad)
        raise AssertionError(f"clause 1 (sound): row {i} list {c}: |approx {ap[i, c]!r} - exact {dseq[i, c]!r}| = "
                             f"{err[i, c]!r} > delta {dl[i, c]!r} ({int(bad.sum())} pairs)")
    neg = np.isfinite(dl) & (dl < 0)
    if neg.any():
        i, c = _first(neg)
        raise AssertionError(f"clause 1 (sound): row {i} list {c}: delta {dl[i, c]!r} is negative")
    if cand_mask is not None:
        bad = ~(np.isfinite(ap) & np.isfinite(dl)) & ~cand_mask
        if bad.any():
            i, c = _first(bad)
            raise AssertionError(f"clause 1 (sound): row {i} list {c}: approx {ap[i, c]!r} delta {dl[i, c]!r} not "
                                 f"finite, yet the list is no candidate")
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.where(fin & (d > 0), err / d, 0.0), initial=0.0))


def check_bound(metric, dp, Q, C, dl):
    """Clause 2: delta is the stated bound to within eps = (dp + 32) u where the norm term is in
    [2^-90, 2^120] (each fp32 norm carries at most (dp / 4 + 3) u, the sqrt, the square and the two
    multiplies a few u), and the floor alone below it. Returns how many pairs were pinned."""
    term = bound_term(metric, Q, C)
    ref = 4.0 * (dp + 4) * U * term + FLOOR
    eps = (dp + 32) * U
    d = dl.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        mid = (term >= TERM_LO) & (term <= TERM_HI)
        lo = term < TERM_LO
        bad = mid & ~(d >= ref * (1 - eps))
        if bad.any():
            i, c = _first(bad)
            raise AssertionError(f"clause 2 (bound shrunk): row {i} list {c}: delta {dl[i, c]!r} < stated "
                                 f"{ref[i, c]!r} (ratio {d[i, c] / ref[i, c]:.6f}, {int(bad.sum())} pairs)")
        bad = mid & ~(d <= ref * (1 + eps))
        if bad.any():
            i, c = _first(bad)
            raise AssertionError(f"clause 2 (bound loosened): row {i} list {c}: delta {dl[i, c]!r} > stated "
                                 f"{ref[i, c]!r} (ratio {d[i, c] / ref[i, c]:.6f}, {int(bad.sum())} pairs)")
        bad = lo & ~((d >= FLOOR * (1 - 2.0 ** -20)) & (d <= 2 * FLOOR))
        if bad.any():
            i, c = _first(bad)
            raise AssertionError(f"clause 2 (floor): row {i} list {c}: delta {dl[i, c]!r} outside "
                                 f"[1e-30 (1 - 2^-20), 2e-30] for a norm term {term[i, c]!r}")
    return int(mid.sum())


def check_candidates(ap, dl, cand, P):
    """Clause 3: cand's rows are well formed and are exactly the restated set. Returns the mask."""
    nlist = ap.shape[1]
    got = cand_sets(cand, nlist)
    want = cand_ref(ap, dl, P)
    bad = got != want
    if bad.any():
        i, c = _first(bad)
        raise AssertionError(f"clause 3 (candidates): row {i} list {c}: {'extra' if got[i, c] else 'missing'} "
                             f"(approx {ap[i, c]!r} delta {dl[i, c]!r} tau {tau_ref(ap, dl, P)[i]!r}; kernel "
                             f"{int(got[i].sum())} restated {int(want[i].sum())} candidates)")
    return got


def check_probes(probes, dseq, P, skip_rows=None):
    """Clause 4, the search's half: the oracle's probes, order included, except for skip_rows."""
    want = probes_ref(dseq, P)
    bad = probes != want
    if skip_rows is not None:
        bad[skip_rows] = False
    if bad.any():
        i, j = _first(bad)
        raise AssertionError(f"clause 4 (probes): row {i} rank {j}: list {int(probes[i, j])}, the reference has "
                             f"{int(want[i, j])} ({int(bad.any(axis=1).sum())} rows differ)")


def violations(metric, dp, Q, C, dseq, snap, P=0, nan_rows=None, stats=None):
    """Every clause on one snapshot ({"approx", "delta"} and, where taken, "cand", "probes", "assign"):
    the list of the clauses' messages, empty when the contract holds. A clause is checked whatever
    the others found. stats (a dict) receives "use", the worst |approx - d_seq| / delta, "pinned",
    the pairs clause 2 pinned to the stated bound, and "ncand", the candidates per row."""
    out = []
    stats = {} if stats is None else stats
    ap, dl = snap["approx"], snap["delta"]
    mask = None

    def clause(f, *a):
        try:
            return f(*a)
        except AssertionError as e:
            out.append(str(e))
            return None

    if "cand" in snap:
        mask = clause(check_candidates, ap, dl, snap["cand"], P)
        if mask is None:  # (malformed or wrong: clause 1 still reads what the rows list)
            mask = np.zeros(ap.shape, bool)
            for i, row in enumerate(snap["cand"]):
                mask[i, row[row < ap.shape[1]]] = True
        stats["ncand"] = mask.sum(axis=1)
    stats["use"] = clause(check_sound, ap, dl, dseq, mask)
    stats["pinned"] = clause(check_bound, metric, dp, Q, C, dl)
    if "probes" in snap:
        clause(check_probes, snap["probes"], dseq, P, nan_rows)
    if "assign" in snap:
        clause(check_assign, snap["assign"], dseq)
    return out


def check_assign(assign, dseq):
    """Clause 4, the add's half."""
    want = assign_ref(dseq)
    bad = assign != want
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"clause 4 (assign): row {i}: list {int(assign[i])}, the reference has {int(want[i])} "
                             f"({int(bad.sum())} rows differ)")
