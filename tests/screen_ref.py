"""numpy restatement of the screened scan (screen.hip, screen_post.hip) and
the checker of its contract on a snapshot of a batch's buffers (IVFFlatIndex.screen_snapshot).
Shared by test_screen_bound.py, test_screen_contract.py and test_gpu_screen_contract.py; no
GPU, no package import.

The deferred screened scan promises, per (query, probed list) pair:
 1. build    the shadow b' and the per-slot norms satisfy what the bound's proof needs;
 2. pairs    the same for the A rows a' and the per-pair norms;
 3. bounds   every collected lower bound is the bound of its (pair, slot) and is a lower bound;
 4. entries  every reserved candidate entry is a sentinel or names a slot of the probed list, once;
 5. required every vector that can be in the list's top-k is collected and survives;
 6. allowed  nothing is collected that the thresholds the wave must know would have pruned;
 7. thresholds every shared threshold is valid and the final one is the k-th of the dumped lists;
 8. select   filter, offsets and scatter are exact given the collect's output.
check_snapshot returns one string per violation, each starting with the clause's tag
("1.build", .., "8.select").

Rounding model. int8: the integer dot product is exact and every later operation of
collect_segment is one rounded fp32 operation (the file is built with contraction off), so the
restated lower and upper bounds equal the kernel's bit for bit. bf16: the MFMA's accumulation
order is not restated; with u = 2^-24, any order of dp fp32 additions of the exact products is
within  eps = gamma_dp * sum |a'_i b'_i|,  gamma_dp = dp u / (1 - dp u)  (Higham, Accuracy and
Stability, §4.2) of the float64 dot, plus u |dot| for rounding the float64 dot to the fp32 value
the restatement feeds in. Propagation to the bounds:
   L2  approx = fl(s - 2 dot):  |d approx| <= e_a = 2 eps (1 + 2u) + 2u |approx|
   IP  approx = -fl(c + dot):   |d approx| <= e_a =   eps (1 + 2u) + 2u |approx|
 (two evaluations whose unrounded values differ by x differ by at most x plus one rounding each).
 del depends on approx only through |approx| in the cu and cr terms:
   L2  rest = .. + cu (.. + |approx|),  del = rest + cr (|approx| + rest)
       d del / d|approx| = cu + cr (1 + cu)
   IP  del = .. + cu (.. + |approx|):   d del / d|approx| = cu
 times the final 1.001, plus the roundings of del's own ~16 operations (16u del):
   e_d = 1.001 g e_a + 16u del,   g = cu + cr (1 + cu) (L2) or cu (IP)
 and  |d lb|, |d ub| <= tol = e_a + e_d + 2u (|approx| + del)  for the last subtraction / addition.
"""
import numpy as np

U = 2.0 ** -24
HUGE = 2.0 ** 50
NOID = 0xFFFFFFFF
CTR_VALID, CTR_CAND, CTR_SURV, CTR_PAIRS, CTR_OVF, CTR_REAL = 8, 9, 10, 11, 12, 13
N_COUNTERS = 16
_F = np.float32
_IGN = dict(over="ignore", invalid="ignore", divide="ignore", under="ignore")


# ---------------------------------------------------------------- shared with test_screen_bound
def bf16(x):
    """Nearest bf16 (ties to even), +0 for |x| < 2^-126, as screen.hip's bf16_bits."""
    x = np.asarray(x, np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    ex = b & 0x7F800000
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    r = np.where(ex == 0, 0, r)
    return r.astype(np.uint32).view(np.float32)


def ru(v):
    """float(v) rounded up, v >= 0 (the kernel's __double2float_ru(sqrt(..) * (1 + 2^-30)))."""
    v = np.asarray(v, np.float64) * (1.0 + 2.0 ** -30)
    f = v.astype(np.float32)
    return np.where(f.astype(np.float64) < v, np.nextafter(f, np.float32(np.inf)), f)


def ref_dist(q, x, metric):
    """The reference's sequential fp32 sum (one row of x per query q)."""
    q = q.astype(np.float32)
    x = x.astype(np.float32)
    if metric == 0:
        t = (q[None, :] - x) ** 2          # each op rounds in float32
    else:
        t = q[None, :] * x
    s = np.cumsum(t, axis=1, dtype=np.float32)[:, -1]
    return s if metric == 0 else -s


def f32_dot(a, b, order):
    """f32 accumulation of exact bf16 products (sequential or pairwise order)."""
    p = (a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)  # exact in f32
    if order == "seq":
        return np.cumsum(p, axis=-1, dtype=np.float32)[..., -1]
    while p.shape[-1] > 1:
        if p.shape[-1] % 2:
            p = np.concatenate([p, np.zeros(p.shape[:-1] + (1,), np.float32)], axis=-1)
        p = (p[..., 0::2] + p[..., 1::2]).astype(np.float32)
    return p[..., 0]


def screen_bound(q, c, X, metric, order):
    dp = q.shape[0]
    cm = np.float32((4 * dp + 16) * float.fromhex("0x1.02p-24"))
    cr = np.float32((dp + 2) * float.fromhex("0x1.02p-24"))
    cu = np.float32(float.fromhex("0x1.02p-23"))
    # per vector (ivf_screen_build): b = x - c in double, b' = bf16(float(b))
    bd = X.astype(np.float64) - c.astype(np.float64)
    bq = bf16(bd.astype(np.float32))
    B2 = (bd * bd).sum(1).astype(np.float32)
    Bn = ru(np.sqrt((bd * bd).sum(1)))
    E = ru(np.sqrt(((bd - bq.astype(np.float64)) ** 2).sum(1)))
    Xn = ru(np.sqrt((X.astype(np.float64) ** 2).sum(1)))
    # per pair (ivf_screen_pairs): L2 a = q - c, IP a = q
    ad = q.astype(np.float64) - (c.astype(np.float64) if metric == 0 else 0.0)
    aq = bf16(ad.astype(np.float32))
    A2 = np.float32((ad * ad).sum())
    An = ru(np.sqrt((ad * ad).sum()))
    F = ru(np.sqrt(((ad - aq.astype(np.float64)) ** 2).sum()))
    qc = np.float32((q.astype(np.float64) * c.astype(np.float64)).sum())
    Cn = ru(np.sqrt((c.astype(np.float64) ** 2).sum()))
    dot = f32_dot(np.broadcast_to(aq, bq.shape), bq, order)
    an, bn = np.float32(An + F), (Bn + E).astype(np.float32)
    cs = (an * E + F * bn + F * E).astype(np.float32)
    if metric == 0:
        approx = ((A2 + B2).astype(np.float32) - np.float32(2) * dot).astype(np.float32)
        rest = (np.float32(2) * (cs + cm * (an * bn)) + cu * (A2 + B2 + np.abs(approx))).astype(np.float32)
        dl = (rest + cr * (np.abs(approx) + rest)).astype(np.float32)
    else:
        qn = np.float32(An)  # (IP: An = |q|)
        approx = (-(qc + dot)).astype(np.float32)
        dl = (cs + cm * (an * bn) + cr * (qn * Xn) + cu * (qn * Cn + an * bn + np.abs(approx))).astype(np.float32)
    dl = (dl * np.float32(1.001) + np.float32(1e-30)).astype(np.float32)
    return approx, dl


# ---------------------------------------------------------------- encodings and layouts
def ord_dec(u):
    """scan_common.hpp ord_dec: the shared thresholds' order-preserving encoding back to float."""
    u = np.asarray(u, np.uint32)
    return np.where(u & 0x80000000, u & 0x7FFFFFFF, ~u).astype(np.uint32).view(np.float32)


def ord_enc(f):
    b = np.asarray(f, np.float32).view(np.uint32)
    return np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)


def pad_dp(X, dp):
    X = np.asarray(X, np.float32).reshape(-1, np.shape(X)[-1])
    out = np.zeros((X.shape[0], dp), np.float32)
    out[:, :X.shape[1]] = X
    return out


def decode_shadow(raw, blocks, dp, i8):
    """The shadow's rows [blocks * 64][dp] from its MFMA B-operand order. int8
    (ivf_screen_build_i8): [block][k-step s][vt][lane l][16 x i8], lane l = vector 16 vt + (l & 15),
    dims 64 s + 16 (l >> 4) .. + 16. bf16 (ivf_screen_build): [block][s][vt][l][8 x bf16], dims
    32 s + 8 (l >> 4) .. + 8. Returns int8 codes, or the bf16 values as float32."""
    e = 16 if i8 else 8
    ks = dp // (4 * e)
    a = np.frombuffer(np.ascontiguousarray(raw).tobytes(), np.int8 if i8 else np.uint16)
    a = a[:blocks * 64 * dp].reshape(blocks, ks, 4, 4, 16, e)          # block, s, vt, h, vv, elem
    a = a.transpose(0, 2, 4, 1, 3, 5).reshape(blocks * 64, dp)        # block, vt, vv | s, h, elem
    if i8:
        return np.ascontiguousarray(a)
    return (a.astype(np.uint32) << 16).view(np.float32)


def encode_shadow(rows, i8):
    """decode_shadow's inverse (rows: int8 codes or bf16-representable float32) as raw bytes."""
    n, dp = rows.shape
    e = 16 if i8 else 8
    ks = dp // (4 * e)
    a = rows if i8 else (np.ascontiguousarray(rows, np.float32).view(np.uint32) >> 16).astype(np.uint16)
    a = a.reshape(n // 64, 4, 16, ks, 4, e).transpose(0, 3, 1, 4, 2, 5)
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy()


def decode_qres(raw, BP, dp, i8):
    """The pairs' A rows [B P][dp] (row-major): int8 codes, or bf16 values as float32."""
    a = np.frombuffer(np.ascontiguousarray(raw).tobytes(), np.int8 if i8 else np.uint16)[:BP * dp].reshape(BP, dp)
    return np.ascontiguousarray(a) if i8 else (a.astype(np.uint32) << 16).view(np.float32)


def encode_qres(rows, i8):
    a = rows if i8 else (np.ascontiguousarray(rows, np.float32).view(np.uint32) >> 16).astype(np.uint16)
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy()


# ---------------------------------------------------------------- build and pairs restated
def _i8_scale(mx):
    mx = _F(mx) if np.ndim(mx) == 0 else mx.astype(_F)
    with np.errstate(**_IGN):
        s = (mx * (_F(1.0) / _F(127.0))).astype(_F) * (_F(1.0) + _F(2.0 ** -20))
    return np.where(mx > 0, s, _F(0)).astype(_F)


def _quantize(r32, sc):
    """i8_q: rint(r * (1 / s)) clamped to [-127, 127] (fp32 operations); s = 0: all zero."""
    with np.errstate(**_IGN):
        inv = np.where(sc > 0, _F(1.0) / sc, _F(0)).astype(_F)
        v = np.rint((r32 * inv[..., None]).astype(_F))
    return np.clip(np.nan_to_num(v, nan=0.0, posinf=127.0, neginf=-127.0), -127, 127).astype(np.int8)


def _is_huge(*arrs):
    h = False
    for a in arrs:
        with np.errstate(**_IGN):
            h = h | ~(np.abs(a) <= HUGE).all(axis=-1)
    return h


def build_restated(X, c, i8):
    """ivf_screen_build(_i8) of the rows X (padded to dp) of one list with centroid c: the shadow
    rows (int8 codes or bf16 floats), sscale (zeros for bf16) and meta [n][4]."""
    X64, c64 = X.astype(np.float64), c.astype(np.float64)
    with np.errstate(**_IGN):
        bd = X64 - c64
        b32 = bd.astype(_F)
        huge = _is_huge(bd, X64)
        if i8:
            sc = np.where(huge, _F(0), _i8_scale(np.abs(b32).max(axis=1, initial=0))).astype(_F)
            sh = _quantize(b32, sc)
            bq = sc.astype(np.float64)[:, None] * sh
        else:
            sc = np.zeros(len(X), _F)
            sh = bf16(b32)
            bq = sh.astype(np.float64)
        b2, x2, e2 = (bd * bd).sum(1), (X64 * X64).sum(1), ((bd - bq) ** 2).sum(1)
        meta = np.stack([b2.astype(_F), ru(np.sqrt(b2)), ru(np.sqrt(e2)), ru(np.sqrt(x2))], 1).astype(_F)
    meta[huge] = np.inf
    return sh, sc, meta


def pairs_restated(q, c, metric, i8):
    """ivf_screen_pairs(_i8) of one pair: the A row, its scale and pst."""
    q64, c64 = q.astype(np.float64), c.astype(np.float64)
    with np.errstate(**_IGN):
        ad = q64 - c64 if metric == 0 else q64
        a32 = ad.astype(_F)
        huge = bool(_is_huge(ad[None], q64[None], c64[None])[0])
        if i8:
            sc = _F(0) if huge else _i8_scale(np.abs(a32).max(initial=0))[()]
            row = _quantize(a32[None], np.array([sc], _F))[0]
            aq = np.float64(sc) * row
        else:
            sc = _F(0)
            row = bf16(a32)
            aq = row.astype(np.float64)
        a2, f2, c2, qc = (ad * ad).sum(), ((ad - aq) ** 2).sum(), (c64 * c64).sum(), (q64 * c64).sum()
        if metric == 0:
            pst = np.array([_F(a2), ru(np.sqrt(a2)), ru(np.sqrt(f2)), 0.0], _F)
        else:
            pst = np.array([_F(qc), ru(np.sqrt(a2)), ru(np.sqrt(f2)), ru(np.sqrt(c2))], _F)
    if huge:
        pst[:] = np.inf
    return row, sc, pst


# ---------------------------------------------------------------- the bound restated
def bounds_from_dot(dot, ps, mt, dp, metric):
    """collect_segment's epilogue from the fp32 dot: (approx, del, lb, ub), one rounded fp32
    operation each, in the kernel's order. ps: pst of the pair [4]; mt: meta of the slots [n][4]."""
    cm = _F(4 * dp + 16) * _F(float.fromhex("0x1.02p-24"))
    cr = _F(dp + 2) * _F(float.fromhex("0x1.02p-24"))
    cu = _F(float.fromhex("0x1.02p-23"))
    dot = np.asarray(dot, _F)
    mt = np.asarray(mt, _F)
    px, py, pz, pw = (_F(v) for v in ps)
    mx, my, mz, mw = mt[:, 0], mt[:, 1], mt[:, 2], mt[:, 3]
    two = _F(2)
    with np.errstate(**_IGN):
        approx = (px + mx) - two * dot if metric == 0 else -(px + dot)
        an, bn = py + pz, my + mz
        cs = (an * mz + pz * bn) + pz * mz
        if metric == 0:
            rest = two * (cs + cm * (an * bn)) + cu * ((px + mx) + np.abs(approx))
            dl = rest + cr * (np.abs(approx) + rest)
        else:
            dl = ((cs + cm * (an * bn)) + cr * (py * mw)) + cu * ((py * pw + an * bn) + np.abs(approx))
        dl = dl * _F(1.001) + _F(1e-30)
        lb, ub = approx - dl, approx + dl
    assert approx.dtype == _F and dl.dtype == _F and lb.dtype == _F
    return approx, dl, lb, ub


def pair_bounds(arow, asc, ps, brows, bsc, mt, dp, metric, i8):
    """Restated (lb, ub, del, tol) of one pair against the slots of its list. int8: exact (tol 0):
    dot = float(integer dot) * (s_a * s_b). bf16: from the float64 dot of the decoded rows, tol per
    the module docstring."""
    if i8:
        acc = brows.astype(np.int64) @ arow.astype(np.int64)
        with np.errstate(**_IGN):
            dot = acc.astype(_F) * (_F(asc) * np.asarray(bsc, _F))
        approx, dl, lb, ub = bounds_from_dot(dot, ps, mt, dp, metric)
        return lb, ub, dl, np.zeros(len(lb))
    with np.errstate(**_IGN):
        prod = brows.astype(np.float64) * arow.astype(np.float64)[None, :]
        d64, sabs = prod.sum(1), np.abs(prod).sum(1)
    approx, dl, lb, ub = bounds_from_dot(d64.astype(_F), ps, mt, dp, metric)
    gam = dp * U / (1.0 - dp * U)
    eps = gam * sabs + U * np.abs(d64)
    cr = (dp + 2) * float.fromhex("0x1.02p-24")
    cu = float.fromhex("0x1.02p-23")
    a, d = np.abs(approx.astype(np.float64)), dl.astype(np.float64)
    with np.errstate(**_IGN):
        e_a = (2.0 if metric == 0 else 1.0) * eps * (1 + 2 * U) + 2 * U * a
        g = cu + cr * (1 + cu) if metric == 0 else cu
        tol = e_a + (1.001 * g * e_a + 16 * U * d) + 2 * U * (a + d)
    return lb, ub, dl, tol


def _kth(v, k):
    """k-th smallest of v (NaN: +inf), +inf when fewer than k."""
    v = np.where(np.isnan(v), np.inf, v)
    return np.partition(v, k - 1)[k - 1] if len(v) >= k else np.float64(np.inf)


def _ulp_close(a, v64):
    a = np.asarray(a, _F)
    with np.errstate(**_IGN):
        r = np.asarray(v64, np.float64).astype(_F)
        return (a == r) | (np.abs(a.astype(np.float64) - r.astype(np.float64)) <= np.spacing(np.abs(r)).astype(np.float64))


# ---------------------------------------------------------------- the checker
def check_snapshot(snap, lists, C, Q, metric, allow_overflow=False, stats=None):
    """The violations of the screened scan's contract in `snap` (screen_snapshot's dict, or
    model_snapshot's), empty when it holds. lists[l]: list l's vectors [n_l][dim] in slot order;
    C: centroids [nlist][dim]; Q: the batch's queries [B][dim]. Ground truth: d64 (float64) and
    d_ref (ref_dist, the reference's sequential fp32 sum).

    Clause 1 skips `sscale >= max |x - c| / 127` for rows whose largest residual is below 2^-100:
    the scale's fp32 product is then subnormal and rounds by more than the 2^-20 margin (the
    bound stays valid: |b - b'| is measured from the codes actually stored). Slots past a list's
    count are outside [block_off * 64, + count): clause 4 flags any entry that names one.

    Clause 4's padding. A collect wave pads, at its end, what is left of its current chunk (at most
    chunk - 1 entries: a chunk is opened only for a block that puts at least one candidate in it)
    and the one chunk it may have reserved ahead (the code allows a wave one outstanding
    reservation). With G workgroups of 4 waves: reserved - real <= 4 G (2 chunk - 1).

    Clause 6, why lb <= U(p, s, j) holds on every schedule: a wave's threshold is min(its running
    k-th, shared); both terms only decrease, and the running list holds at least blocks 0..j of
    the segment, because a block is merged whenever one of its upper bounds is below that minimum
    (a skipped block cannot lower the k-th below it). So the threshold at block j is never above
    the k-th smallest upper bound of the segment's blocks 0..j.

    Clause 7, the final threshold: every value a wave publishes during the collect is the k-th of
    its running list at that time, which is never below the k-th of the list it contributes at the
    end, so after tfinal thr equals the k-th smallest of the union of the dumped lists whenever
    every contribution was kept (ubcnt <= ub_lists); with dropped contributions it may be lower
    (a dropped list's published k-th), so only "<= and valid" is asked then.

    allow_overflow: pairs with ovf = 1 are excused from clauses 3 and 5-8; otherwise any overflow
    mark is itself a violation. stats (a dict): 'tight' receives the worst (d_ref - lb) / (2 del)
    over the candidates."""
    V = []
    s = snap
    B, P, k, dp, i8 = s["B"], s["P"], s["k"], s["dp"], bool(s["i8"])
    BP, nlist = B * P, s["nlist"]
    segv = s["seg_blocks"] * 64
    ctr = np.asarray(s["counters"], np.uint32)
    nvalid = int(ctr[CTR_VALID])
    if s["metric"] != metric:
        return ["0.setup metric %d, expected %d" % (s["metric"], metric)]
    Cp, Qp = pad_dp(C, dp), pad_dp(Q, dp)
    off = np.asarray(s["block_off"], np.uint64).astype(np.int64) * 64
    cnt = np.asarray(s["count"], np.uint32).astype(np.int64)
    shadow = decode_shadow(s["shadow"], s["blocks"], dp, i8)
    meta = np.asarray(s["meta"], _F).reshape(-1, 4)
    sscale = np.asarray(s["sscale"], _F) if i8 else np.zeros(len(meta), _F)
    qres = decode_qres(s["qres"], BP, dp, i8)
    pst = np.asarray(s["pst"], _F).reshape(-1, 4)
    qscale = np.asarray(s["qscale"], _F) if i8 else np.zeros(BP, _F)
    probes = np.asarray(s["probes"], np.uint32).astype(np.int64)

    def proof_checks(tag, what, x64, a64, rows, sc, norms, xnorm_col):
        """|a| <= norms.y, |a - a'| <= norms.z, codes and scale (int8), huge -> all inf."""
        with np.errstate(**_IGN):
            huge = _is_huge(a64, x64)
            aq = sc.astype(np.float64)[:, None] * rows if i8 else rows.astype(np.float64)
            an, en = np.sqrt((a64 * a64).sum(1)), np.sqrt(((a64 - aq) ** 2).sum(1))
        ok = ~huge
        bad = huge & ~np.isposinf(norms).all(1)
        if bad.any():
            V.append("%s %s %d: a non-finite or > 2^50 row without all-infinite norms" % (tag, what, np.flatnonzero(bad)[0]))
        for col, val, name in ((1, an, "|a|"), (2, en, "|a - a'|")):
            bad = ok & ~(norms[:, col].astype(np.float64) >= val)
            if bad.any():
                i = np.flatnonzero(bad)[0]
                V.append("%s %s %d: norm %s = %r below the true %r" % (tag, what, i, name, norms[i, col], val[i]))
        if i8:
            if (rows == -128).any():
                V.append("%s %s: an int8 code of -128" % (tag, what))
            with np.errstate(**_IGN):
                mx = np.abs(a64).max(axis=1, initial=0)
            bad = ok & (mx >= 2.0 ** -100) & ~(sc.astype(np.float64) >= mx / 127.0)
            if bad.any():
                i = np.flatnonzero(bad)[0]
                V.append("%s %s %d: scale %r below max / 127 = %r" % (tag, what, i, sc[i], mx[i] / 127.0))
        return ok

    # ---- 1. build
    Xp = []
    for l in range(nlist):
        X = pad_dp(lists[l], dp) if len(lists[l]) else np.zeros((0, dp), _F)
        Xp.append(X)
        if cnt[l] != len(X):
            V.append("1.build list %d holds %d vectors, the test's list %d" % (l, cnt[l], len(X)))
            return V
        if not len(X):
            continue
        sl = slice(off[l], off[l] + cnt[l])
        X64 = X.astype(np.float64)
        with np.errstate(**_IGN):
            bd = X64 - Cp[l].astype(np.float64)
        ok = proof_checks("1.build", "list %d slot" % l, X64, bd, shadow[sl], sscale[sl], meta[sl], 3)
        with np.errstate(**_IGN):
            xn, b2 = np.sqrt((X64 * X64).sum(1)), (bd * bd).sum(1)
        bad = ok & ~(meta[sl, 3].astype(np.float64) >= xn)
        if bad.any():
            V.append("1.build list %d slot %d: |x| norm below the true one" % (l, np.flatnonzero(bad)[0]))
        bad = ok & ~_ulp_close(meta[sl, 0], b2)
        if bad.any():
            i = np.flatnonzero(bad)[0]
            V.append("1.build list %d slot %d: |b|^2 = %r, expected %r" % (l, i, meta[sl][i, 0], _F(b2[i])))

    # ---- 2. pairs
    pq = np.arange(BP) // P
    q64, c64 = Qp[pq].astype(np.float64), Cp[probes].astype(np.float64)
    with np.errstate(**_IGN):
        a64 = q64 - c64 if metric == 0 else q64
        # (a huge centroid also flags the pair)
        hc = _is_huge(c64)
    okp = proof_checks("2.pairs", "pair", np.where(hc[:, None], np.inf, q64), a64, qres, qscale, pst, None)
    with np.errstate(**_IGN):
        want_x = (a64 * a64).sum(1) if metric == 0 else (q64 * c64).sum(1)
        slack = 0.0 if metric == 0 else 1e-13 * (np.abs(q64 * c64)).sum(1)
        r = want_x.astype(_F)
        near = _ulp_close(pst[:, 0], want_x) | (np.abs(pst[:, 0].astype(np.float64) - want_x) <= slack + np.spacing(np.abs(r)))
    bad = okp & ~near
    if bad.any():
        i = np.flatnonzero(bad)[0]
        V.append("2.pairs pair %d: pst.x = %r, expected %r" % (i, pst[i, 0], r[i]))
    if metric == 1:
        bad = okp & ~(pst[:, 3].astype(np.float64) >= np.sqrt((c64 * c64).sum(1)))
        if bad.any():
            V.append("2.pairs pair %d: |c| norm below the true one" % np.flatnonzero(bad)[0])

    # ---- per valid sorted pair: ground truth and restated bounds over its whole list
    spair = np.asarray(s["sorted_pair"], np.uint32).astype(np.int64)
    ovf = np.asarray(s["ovf"], np.uint32)
    if nvalid > BP:
        return V + ["4.entries counters[valid] = %d above B P = %d" % (nvalid, BP)]
    sp_pair = (spair[:nvalid] >> 16) * P + (spair[:nvalid] & 0xFFFF)
    sp_list = probes[np.minimum(sp_pair, BP - 1)]
    if nvalid and (sp_pair >= BP).any():
        return V + ["4.entries a sorted pair outside the batch"]
    T = {}
    for sp in range(nvalid):
        i, l = int(sp_pair[sp]), int(sp_list[sp])
        sl = slice(off[l], off[l] + cnt[l])
        lb, ub, dl, tol = pair_bounds(qres[i], qscale[i], pst[i], shadow[sl], sscale[sl], meta[sl], dp, metric, i8)
        X = Xp[l]
        with np.errstate(**_IGN):
            dref = ref_dist(Qp[i // P], X, metric)
        with np.errstate(**_IGN):
            X64, qq = X.astype(np.float64), Qp[i // P].astype(np.float64)
            d64 = ((qq - X64) ** 2).sum(1) if metric == 0 else -(qq * X64).sum(1)
        T[sp] = dict(l=l, lb=lb, ub=ub, dl=dl, tol=tol, dref=dref, d64=d64)
    if not allow_overflow and (ovf[:nvalid].any() or ctr[CTR_OVF]):
        V.append("4.entries overflow marked (counters[ovf] = %d, %d pairs) with room in the buffer" %
                 (ctr[CTR_OVF], int(ovf[:nvalid].sum())))

    # ---- 4. entries
    cap = s["cand_cap"]
    ncand = int(min(ctr[CTR_CAND], cap))
    cand = np.asarray(s["cand"], np.uint32).reshape(-1, 4)
    if len(cand) < ncand:
        return V + ["4.entries the snapshot holds %d entries of %d reserved" % (len(cand), ncand)]
    cand = cand[:ncand]
    c_sp, c_slot, c_lb, c_w = cand[:, 0].astype(np.int64), cand[:, 1].astype(np.int64), cand[:, 2].view(_F), cand[:, 3]
    sent = cand[:, 0] == NOID
    bad = sent & ((cand[:, 1] != 0) | (cand[:, 2] != 0) | (cand[:, 3] != NOID))
    if bad.any():
        V.append("4.entries entry %d: a sentinel pair with a payload %s" % (np.flatnonzero(bad)[0], cand[bad][0].tolist()))
    real = ~sent
    bad = real & (c_sp >= nvalid)
    if bad.any():
        V.append("4.entries entry %d: sorted pair %d of %d valid (an unwritten entry?)" % (np.flatnonzero(bad)[0], c_sp[bad][0], nvalid))
    good = real & ~bad
    e_l = np.where(good, sp_list[np.minimum(c_sp, max(nvalid - 1, 0))] if nvalid else 0, 0)
    e_idx = c_slot - off[e_l]
    bad = good & ((e_idx < 0) | (e_idx >= cnt[e_l]))
    if bad.any():
        j = np.flatnonzero(bad)[0]
        V.append("4.entries entry %d: slot %d outside list %d's [%d, %d)" % (j, c_slot[j], e_l[j], off[e_l[j]], off[e_l[j]] + cnt[e_l[j]]))
    good &= ~bad
    key = (c_sp << 32) | (c_slot & 0xFFFFFFFF)
    uq, first, n_of = np.unique(key[good], return_index=True, return_counts=True)
    if (n_of > 1).any():
        d = uq[n_of > 1][0]
        V.append("4.entries (pair %d, slot %d) collected %d times" % (d >> 32, d & 0xFFFFFFFF, n_of[n_of > 1][0]))
    nreal = int(real.sum())
    if not ctr[CTR_OVF] and nreal != ctr[CTR_REAL]:
        V.append("4.entries %d real entries, counters[real] = %d" % (nreal, ctr[CTR_REAL]))
    if ctr[CTR_REAL] < nreal:
        V.append("4.entries counters[real] = %d below the %d real entries present" % (ctr[CTR_REAL], nreal))
    if ctr[CTR_CAND] < ctr[CTR_REAL]:
        V.append("4.entries reserved %d below real %d" % (ctr[CTR_CAND], ctr[CTR_REAL]))
    pad_max = 4 * s["grid"] * (2 * s["cand_chunk"] - 1)
    if int(ctr[CTR_CAND]) - int(ctr[CTR_REAL]) > pad_max:
        V.append("4.entries padding %d above 4 x %d workgroups x (2 x %d - 1) = %d" %
                 (int(ctr[CTR_CAND]) - int(ctr[CTR_REAL]), s["grid"], s["cand_chunk"], pad_max))

    # ---- 3. bounds, 6. allowed (per good entry)
    gi = np.flatnonzero(good)
    tight = 0.0
    for sp in np.unique(c_sp[gi]):
        t = T[int(sp)]
        if ovf[sp]:
            continue
        e = gi[c_sp[gi] == sp]
        idx, lbk = e_idx[e], c_lb[e]
        lbr, tol = t["lb"][idx], t["tol"][idx]
        nan_k, nan_r = np.isnan(lbk), np.isnan(lbr)
        if i8:
            bad = (lbk.view(np.uint32) != lbr.view(np.uint32)) & ~(nan_k & nan_r)
        else:
            with np.errstate(**_IGN):
                bad = ~(np.abs(lbk.astype(np.float64) - lbr.astype(np.float64)) <= tol) & ~(nan_k & nan_r) & ~(lbk == lbr)
        if bad.any():
            j = np.flatnonzero(bad)[0]
            V.append("3.bounds pair %d slot %d: lb %r, restated %r (tol %g)" % (sp, c_slot[e[j]], lbk[j], lbr[j], tol[j]))
        with np.errstate(**_IGN):
            bad = ~nan_k & ((lbk > t["dref"][idx]) | (lbk.astype(np.float64) > t["d64"][idx]))
        if bad.any():
            j = np.flatnonzero(bad)[0]
            V.append("3.bounds pair %d slot %d: lb %r above d_ref %r / d64 %r" %
                     (sp, c_slot[e[j]], lbk[j], t["dref"][idx[j]], t["d64"][idx[j]]))
        with np.errstate(**_IGN):
            rt = (t["dref"][idx].astype(np.float64) - lbk) / (2.0 * t["dl"][idx].astype(np.float64))
        if np.isfinite(rt).any():
            tight = max(tight, float(rt[np.isfinite(rt)].max()))
        # allowed: lb <= U(p, seg, block) = k-th smallest (ub + tol) over the segment's blocks 0..j
        ubt = np.where(np.isnan(t["ub"]), np.inf, t["ub"].astype(np.float64) + t["tol"])
        eb = idx // 64
        for b in np.unique(eb):
            lo = (b * 64 // segv) * segv
            Ub = _kth(ubt[lo:min((b + 1) * 64, len(ubt))], k)
            m = eb == b
            with np.errstate(**_IGN):
                bad = m & (lbk.astype(np.float64) - tol > Ub)
            if bad.any():
                j = np.flatnonzero(bad)[0]
                V.append("6.allowed pair %d slot %d: lb %r above U = %r of its segment's blocks so far" %
                         (sp, c_slot[e[j]], lbk[j], Ub))
                break
    if stats is not None:
        stats["tight"] = tight
        stats["real"] = nreal

    # ---- 5. required; 3. the always-candidates (NaN bounds)
    have = set(key[good].tolist())
    scnt = np.asarray(s["scnt"], np.uint32).astype(np.int64)
    soff = np.asarray(s["soff"], np.uint32).astype(np.int64)
    surv = np.asarray(s["surv"], np.uint32).reshape(-1, 2).astype(np.int64)
    nsurv = int(ctr[CTR_SURV])
    runs_ok = len(soff) > nvalid and len(surv) >= nsurv and (soff[:nvalid] + scnt[:nvalid] <= nsurv).all()
    for sp in range(nvalid):
        t = T[sp]
        if ovf[sp]:
            continue
        l, n = t["l"], len(t["dref"])
        if n < k:
            req = np.ones(n, bool)
        else:
            kth = _kth(t["dref"], k)
            with np.errstate(**_IGN):
                req = t["dref"] <= kth
        run = set(surv[soff[sp]:soff[sp] + scnt[sp], 0].tolist()) if runs_ok else set()
        for ii in np.flatnonzero(req):
            slot = int(off[l] + ii)
            if ((sp << 32) | slot) not in have:
                V.append("5.required pair %d slot %d (d_ref %r, within the list's k-th) is not a candidate" % (sp, slot, t["dref"][ii]))
                break
            if slot not in run:
                V.append("5.required pair %d slot %d (d_ref %r, within the list's k-th) did not survive" % (sp, slot, t["dref"][ii]))
                break
        for ii in np.flatnonzero(np.isnan(t["lb"])):
            if ((sp << 32) | int(off[l] + ii)) not in have:
                V.append("3.bounds pair %d slot %d has no finite bound and is not a candidate" % (sp, off[l] + ii))
                break

    # ---- 7. thresholds
    thr = ord_dec(s["thr"])
    thr4 = ord_dec(np.asarray(s["thr4"], np.uint32).reshape(-1, 4))
    ublist = np.asarray(s["ublist"], _F).reshape(BP, s["ub_lists"], k)
    ubcnt = np.asarray(s["ubcnt"], np.uint32).astype(np.int64)
    for sp in range(nvalid):
        t = T[sp]
        if ovf[sp]:
            continue
        n = len(t["dref"])
        ns = (n + segv - 1) // segv
        lo_c = (ns + s["segs_item"] - 1) // s["segs_item"]
        if not (lo_c <= ubcnt[sp] <= ns):
            V.append("7.thresholds pair %d: %d contributions, the plan implies %d .. %d" % (sp, ubcnt[sp], lo_c, ns))
        rows = ublist[sp, :min(ubcnt[sp], s["ub_lists"])]
        with np.errstate(**_IGN):
            asc = rows[:, 1:] >= rows[:, :-1]
            if not asc.all():
                r_ = np.flatnonzero(~asc.all(1))[0]
                V.append("7.thresholds pair %d: contributed list %d is not ascending" % (sp, r_))
        if i8:
            vals = rows[np.isfinite(rows)]
            uv, un = np.unique(vals.view(np.uint32), return_counts=True)
            rv, rn = np.unique(t["ub"][np.isfinite(t["ub"])].view(np.uint32), return_counts=True)
            pos = np.searchsorted(rv, uv)
            inside = (pos < len(rv)) & (rv[np.minimum(pos, len(rv) - 1)] == uv) if len(rv) else np.zeros(len(uv), bool)
            if not inside.all() or (un > rn[pos[inside]] if inside.all() else np.array([True])).any():
                V.append("7.thresholds pair %d: a contributed value is no upper bound of the list's vectors" % sp)

        def valid(th):
            with np.errstate(**_IGN):
                return np.isposinf(th) or int((t["dref"] <= th).sum()) >= k

        if not valid(thr[sp]):
            V.append("7.thresholds pair %d: thr %r has fewer than k vectors at or below it" % (sp, thr[sp]))
        un_k = _kth(rows.reshape(-1).astype(np.float64), k) if rows.size else np.inf
        if thr[sp] > un_k or (ubcnt[sp] <= s["ub_lists"] and thr[sp] != un_k):
            V.append("7.thresholds pair %d: thr %r, the k-th of the dumped lists is %r" % (sp, thr[sp], un_k))
        if np.isfinite(thr4[sp]).all() and not valid(thr4[sp].max()):
            V.append("7.thresholds pair %d: max(thr4) %r has fewer than k vectors at or below it" % (sp, thr4[sp].max()))

    # ---- 8. select
    with np.errstate(**_IGN):
        Tf = np.minimum(thr[:nvalid], thr4[:nvalid].max(axis=1)) if nvalid else np.zeros(0, _F)
        keep = good & (ovf[np.minimum(c_sp, max(nvalid - 1, 0))] == 0 if nvalid else False)
        keep = keep & ~(c_lb > Tf[np.minimum(c_sp, max(nvalid - 1, 0))]) if nvalid else keep
    free = ~np.isin(c_sp, np.flatnonzero(ovf[:nvalid])) | sent  # (entries of overflowed pairs are not judged)
    bad = free & good & ((c_w != NOID) != keep)
    if bad.any():
        j = np.flatnonzero(bad)[0]
        V.append("8.select entry %d (pair %d, lb %r, T %r): kept %s, expected %s" %
                 (j, c_sp[j], c_lb[j], Tf[c_sp[j]] if c_sp[j] < nvalid else None, c_w[j] != NOID, bool(keep[j])))
    if len(soff) <= nvalid or not (soff[:nvalid + 1] == np.concatenate([[0], np.cumsum(scnt[:nvalid])])).all():
        V.append("8.select soff is not the exclusive prefix sum of scnt")
    elif soff[nvalid] != nsurv:
        V.append("8.select soff[nvalid] = %d, counters[surv] = %d" % (soff[nvalid], nsurv))
    for sp in range(nvalid):
        if ovf[sp]:
            continue
        m = keep & (c_sp == sp)
        if scnt[sp] != m.sum() or not np.array_equal(np.sort(c_w[m & (c_w != NOID)]), np.arange(scnt[sp])):
            V.append("8.select pair %d: scnt %d, %d kept entries, ranks no permutation" % (sp, scnt[sp], m.sum()))
            continue
        if not runs_ok:
            V.append("8.select pair %d: its run of surv lies outside the %d survivors" % (sp, nsurv))
            break
        run = surv[soff[sp]:soff[sp] + scnt[sp]]
        if not (run[:, 1] == sp).all() or sorted(run[:, 0].tolist()) != sorted(c_slot[m].tolist()):
            V.append("8.select pair %d: its run of surv does not hold exactly its kept (slot, pair)" % sp)
    return V


# ---------------------------------------------------------------- the model
def model_snapshot(lists, C, Q, metric, k, i8, seg_blocks=8, cand_cap=1 << 20, chunk=128, ub_lists=128):
    """A snapshot of the same format from the restated build, pairs and bounds, on one sequential
    schedule: one wave per list, every query probing every list, segments and blocks in order,
    thresholds from the running k-th upper bound alone. Slow; its only purpose is to test
    check_snapshot."""
    nlist, dim = C.shape
    dp = (dim + 63) // 64 * 64
    B, P = len(Q), nlist
    BP = B * P
    Cp, Qp = pad_dp(C, dp), pad_dp(Q, dp)
    cnt = np.array([len(x) for x in lists], np.int64)
    nb = (cnt + 63) // 64
    boff = np.concatenate([[0], np.cumsum(nb)])[:-1]
    blocks = int(nb.sum())
    rows = np.zeros((blocks * 64, dp), np.int8 if i8 else _F)
    sscale, meta = np.zeros(blocks * 64, _F), np.zeros((blocks * 64, 4), _F)
    for l in range(nlist):
        if cnt[l]:
            sl = slice(boff[l] * 64, boff[l] * 64 + cnt[l])
            rows[sl], sscale[sl], meta[sl] = build_restated(pad_dp(lists[l], dp), Cp[l], i8)
    probes = np.tile(np.arange(P, dtype=np.uint32), B)
    qrows = np.zeros((BP, dp), np.int8 if i8 else _F)
    qscale, pst = np.zeros(BP, _F), np.zeros((BP, 4), _F)
    for i in range(BP):
        qrows[i], qscale[i], pst[i] = pairs_restated(Qp[i // P], Cp[probes[i]], metric, i8)
    order = sorted((int(probes[i]), i) for i in range(BP) if cnt[probes[i]])
    nvalid = len(order)
    sorted_pair = np.zeros(BP, np.uint32)
    thr, thr4 = np.full(BP, np.inf, _F), np.full((BP, 4), np.inf, _F)
    ublist, ubcnt = np.zeros((BP, ub_lists, k), _F), np.zeros(BP, np.uint32)
    ovf, scnt, soff = np.zeros(BP, np.uint32), np.zeros(BP, np.uint32), np.zeros(BP + 1, np.uint32)
    ent = []
    kq = (k + 3) // 4
    for sp, (l, i) in enumerate(order):
        sorted_pair[sp] = ((i // P) << 16) | (i % P)
        sl = slice(boff[l] * 64, boff[l] * 64 + cnt[l])
        lb, ub, _, _ = pair_bounds(qrows[i], qscale[i], pst[i], rows[sl], sscale[sl], meta[sl], dp, metric, i8)
        ubc = np.where(np.isnan(ub), _F(np.inf), ub).astype(_F)
        for b in range(int(nb[l])):
            hi = min((b + 1) * 64, int(cnt[l]))
            th = _kth(ubc[:hi], k)
            for v in range(b * 64, hi):
                if not lb[v] > th:
                    ent.append((sp, boff[l] * 64 + v, lb[v]))
        srt = np.sort(ubc)
        row = np.full(k, np.inf, _F)
        row[:min(k, len(srt))] = srt[:k]
        ublist[sp, 0], ubcnt[sp] = row, 1
        thr[sp] = row[k - 1]
        thr4[sp, 0] = row[kq - 1]
    nreal = len(ent)
    ncand = (nreal + chunk - 1) // chunk * chunk
    cand = np.zeros((ncand, 4), np.uint32)
    cand[:] = (NOID, 0, 0, NOID)
    Tf = np.minimum(thr, thr4.max(1))
    for j, (sp, slot, lbv) in enumerate(ent):
        cand[j] = (sp, slot, np.array(lbv, _F).view(np.uint32), NOID)
        if not lbv > Tf[sp]:
            cand[j, 3] = scnt[sp]
            scnt[sp] += 1
    soff[1:nvalid + 1] = np.cumsum(scnt[:nvalid])
    soff[nvalid + 1:] = soff[nvalid]
    surv = np.zeros((int(soff[nvalid]), 2), np.uint32)
    for e in cand[:nreal]:
        if e[3] != NOID:
            surv[soff[e[0]] + e[3]] = (e[1], e[0])
    ctr = np.zeros(N_COUNTERS, np.uint32)
    ctr[CTR_VALID], ctr[CTR_CAND], ctr[CTR_SURV], ctr[CTR_REAL] = nvalid, ncand, soff[nvalid], nreal
    ns_max = int(max(1, ((cnt + seg_blocks * 64 - 1) // (seg_blocks * 64)).max()))
    return dict(B=B, P=P, k=k, dp=dp, seg_blocks=seg_blocks, segs_item=ns_max, wide_q=16, cand_cap=cand_cap, i8=int(i8),
                metric=metric, grid=1, nlist=nlist, blocks=blocks, ub_lists=ub_lists, cand_chunk=chunk, dim=dim,
                probes=probes, sorted_pair=sorted_pair, counters=ctr, cand=cand, ovf=ovf, thr=ord_enc(thr),
                thr4=ord_enc(thr4), ublist=ublist, ubcnt=ubcnt, scnt=scnt, soff=soff, surv=surv, pst=pst,
                qscale=qscale if i8 else np.zeros(0, _F), qres=encode_qres(qrows, i8),
                block_off=boff.astype(np.uint64), count=cnt.astype(np.uint32), meta=meta,
                sscale=sscale if i8 else np.zeros(0, _F), shadow=encode_shadow(rows, i8))


# ---------------------------------------------------------------- the tests' fixture
def contract_fixture(dim, seed=0, hub_blocks=31, special=False, ties=False, nq=40):
    """Five lists with explicit centroids: a hub of hub_blocks full blocks and one of 5 vectors,
    lists of exactly 64, of 65 and of 1 vector, and an empty one; nq iid queries. special: the hub
    also holds a zero vector, a vector equal to its centroid, a 3e38 entry, a +inf entry and a
    1e-41 row, and query 7 is all zero. ties: hub rows 100..299 are 200 copies of one vector near
    every query. Returns X, ids, assign (list of every row), C, Q and lists (rows per list in slot
    order)."""
    rng = np.random.default_rng(seed)
    sizes = [hub_blocks * 64 + 5, 64, 65, 1, 0]
    C = (2.0 * rng.standard_normal((5, dim))).astype(_F)
    C[0] *= 0.05
    lists = [(C[l] + rng.standard_normal((n, dim))).astype(_F) for l, n in enumerate(sizes)]
    Q = rng.standard_normal((nq, dim)).astype(_F)
    if ties:
        lists[0][100:300] = (0.3 * rng.standard_normal(dim)).astype(_F)
    if special:
        sp = rng.standard_normal((5, dim)).astype(_F)
        sp[0] = 0.0
        sp[1] = C[0]
        sp[2, 3] = 3e38
        sp[3, 5] = np.inf
        sp[4] = 1e-41
        lists[0] = np.concatenate([lists[0], sp])
        Q[7] = 0.0
    X = np.concatenate(lists)
    assign = np.concatenate([np.full(len(x), l, np.int64) for l, x in enumerate(lists)])
    ids = rng.permutation(len(X)).astype(np.uint64) + np.uint64(1000)
    return dict(X=X, ids=ids, assign=assign, C=C, Q=Q, lists=lists)
