"""Rounding bounds for the ordinal kernels (csrc/ordinal.hip) against the long-double statement (gpirt_amd/ordinal.py), and the
constructed cases the CPU and GPU tests share.  Nothing here comes from what the device returns.

u = 2^-53 is the unit roundoff of fp64.  The device's term is ll_term_fast, within 2 ulp = 4 u relative of log(1 + e^-a)
(ll_fast.h, tests/test_ll_fast.py); the term is 1-Lipschitz in its argument.  The long-double statement itself carries 2^-64
relative per operation, 2^11 times less: it is covered by the factor 2 on every bound below.

One cell of a slice / beta sum.  The kernel forms g = (F c + V s) + M and a = b - g (or g - b) in fp64:
    |dg| <= u (|F c| + |V s| + |F c + V s| + |g|)  +  TRIG (|F| + |V|),   |da| <= |dg| + u |a|
TRIG = 4 u covers a device cosine / sine 2 ulp off plus NumPy's own 1 ulp (the statement takes NumPy's float64 c and s).  The term
then errs by |da| + 4 u v (v its value), and a sum of T terms through the kernel's trees (at most 2 * 16 sequential additions in
a lane, 6 shuffle levels, 4 levels over the wavefronts: depth <= 42 <= T + 10) by another (T + 10) u sum v.
"""
import numpy as np

from gpirt_amd import ordinal as OR

U = 2.0 ** -53
LD = np.longdouble


def _abs_terms(cat, g, b):
    """The ll values v (long double) and |a| of every term of a column, as two flat arrays."""
    cat = np.asarray(cat)
    bb = np.concatenate([[-np.inf], np.asarray(b, dtype=np.float64), [np.inf]]).astype(LD)
    Cn = bb.size - 1
    vs, as_ = [], []
    for c in range(1, Cn + 1):
        sel = cat == c
        if not sel.any():
            continue
        if c < Cn:
            a = bb[c] - g[sel]
            vs.append(OR.ll(a)); as_.append(np.abs(a))
        if c > 1:
            a = g[sel] - bb[c - 1]
            vs.append(OR.ll(a)); as_.append(np.abs(a))
    if not vs:
        return np.zeros(0, dtype=LD), np.zeros(0, dtype=LD)
    return np.concatenate(vs), np.concatenate(as_)


def sum_bound(cat, F, V, M, b, c=1.0, s=0.0, trig=True):
    """The bound on |device sum - long-double sum| of a column's ll terms at the point g = (F c + V s) + M."""
    cat = np.asarray(cat)
    Fl, Vl, Ml = (np.asarray(x, dtype=np.float64).astype(LD) for x in (F, V, M))
    g = (Fl * LD(c) + Vl * LD(s)) + Ml
    F, V, M = np.abs(Fl), np.abs(Vl), np.abs(Ml)
    obs = cat > 0
    dg = U * (F * abs(c) + V * abs(s) + np.abs(F * abs(c) + V * abs(s)) + np.abs(g) + M) + (4 * U if trig else 0.0) * (F + V)
    nt = np.where((cat > 1) & (cat < len(b) + 1), 2, 1)
    v, a = _abs_terms(cat, g, b)
    T = v.size
    return 2.0 * float((dg[obs] * nt[obs]).sum() + U * a.sum() + 4 * U * v.sum() + (T + 10) * U * v.sum())


def slice_bound(cat, f, nu, mu, b, eps, ll0, log_u):
    """The band of one slice decision ll(f') - (ll(f) + log u): both sums' bounds, log u (2 ulp), the addition."""
    c, s = np.cos(eps), np.sin(eps)
    return (sum_bound(cat, f, nu, mu, b, c, s) + sum_bound(cat, f, np.zeros_like(np.asarray(f, dtype=np.float64)), mu, b, 1.0, 0.0, trig=False)
            + 8 * U * (abs(float(ll0)) + abs(float(log_u))))


def theta_bound(cat, fstar, B):
    """Per entry of logpost (N x n): the observed items times the term's error (4 u v + u |a|: f* is given, only b - f* rounds),
    plus the GEMM's summation bound (K + 2) u sum |terms| at K = C m (any order of a K-term fp64 dot product)."""
    cat = np.asarray(cat)
    fs = np.asarray(fstar, dtype=np.float64).astype(LD)
    B = np.asarray(B, dtype=np.float64)
    N, m = fs.shape
    Cn = B.shape[1] + 1
    Kdim = Cn * m
    out = np.zeros((N, cat.shape[0]), dtype=LD)
    for j in range(m):
        for c in range(1, Cn + 1):
            who = cat[:, j] == c
            if not who.any():
                continue
            v, a = np.zeros(N, dtype=LD), np.zeros(N, dtype=LD)
            if c < Cn:
                x = LD(B[j, c - 1]) - fs[:, j]; v = v + OR.ll(x); a = a + np.abs(x)
            if c > 1:
                x = fs[:, j] - LD(B[j, c - 2]); v = v + OR.ll(x); a = a + np.abs(x)
            out[:, who] += ((5 + Kdim + 2) * U * v + U * a)[:, None]
    return 2.0 * out


def beta_bound(cat, f, theta, b0, b1, b1p, b, r_parts):
    """The band of the slope's decision r - log u: two sums at mu = b0 + theta b1 (two roundings in mu: u (|theta b1| + |mu|)),
    the priors and log u (a few ulp of each magnitude)."""
    th = np.asarray(theta, dtype=np.float64)
    z = np.zeros_like(th)
    tot = 0.0
    for bb in (b1, b1p):
        mu = b0 + th * bb
        tot += sum_bound(cat, f, z, mu, b, 1.0, 0.0, trig=False) + 2.0 * U * float(((np.abs(th * bb) + np.abs(mu)) * 2)[np.asarray(cat) > 0].sum())
    return tot + 16 * U * sum(abs(float(x)) for x in r_parts)


def lp_bound(cat, g, t, log_prior, K, c, a, W):
    """Per slot of a threshold update's masses: the cells' terms (|da| = u (|g| + |t_q - g|): g = f + mu and the difference
    round), their sum, log_prior - S, and the two w terms (log1p and exp within 2 ulp each, d = t_q - t_left exact to u |d|:
    |dw| <= 4 u |w| + (u d + 4 u e^-d) / (1 - e^-d)), times N_c, plus the additions."""
    cat = np.asarray(cat)
    t = np.asarray(t, dtype=np.float64)
    gg = np.asarray(g, dtype=np.float64).astype(LD)
    K = [int(x) for x in np.asarray(K).reshape(-1)]
    P = t.size
    left = K[c - 2] if c >= 2 else -1
    right = K[c] if c <= len(K) - 1 else P
    lo, hi = OR.candidates(a, W, left, right, P)
    out = np.zeros(int(W))
    lower, upper = gg[cat == c], gg[cat == c + 1]
    for q in range(lo, hi + 1):
        a1, a2 = LD(t[q]) - lower, upper - LD(t[q])
        v = np.concatenate([OR.ll(a1), OR.ll(a2)])
        aa = np.concatenate([np.abs(a1), np.abs(a2)])
        gabs = np.concatenate([np.abs(lower), np.abs(upper)])
        T = v.size
        e = U * (gabs.sum() + aa.sum()) + (4 + T + 10) * U * v.sum()
        tot = abs(float(log_prior[q])) + float(v.sum())
        for nb, d in ((lower.size, t[q] - t[left] if left >= 0 else None), (upper.size, t[right] - t[q] if right < P else None)):
            if d is None:
                continue
            wv = abs(float(OR.w(LD(d))))
            e += nb * (4 * U * wv + (U * d + 4 * U * np.exp(-d)) / (1.0 - np.exp(-d)) + U * wv)
            tot += nb * wv
        out[q - a] = 2.0 * float(e + 3 * U * tot)
    return out


# ---------------------------------------------------------------------------------------------------- the cases ------
def make_case(n, m, C, seed, na=0.1):
    """cat (n x m) with about `na` missing cells, one item with a category nobody chose (the last item never uses category 2 --
    for C = 2 that item never uses category 1 above row 0), one item whose every answer is the same category (item 0: all
    category C), one respondent with no answer (row 1), and random ordered thresholds on the default grid."""
    rng = np.random.default_rng(seed)
    cat = rng.integers(1, C + 1, size=(n, m)).astype(np.int8)
    cat[rng.random((n, m)) < na] = 0
    cat[:, 0] = np.where(cat[:, 0] > 0, C, 0)
    last = cat[:, m - 1]
    last[last == min(2, C)] = 1 if C > 2 else 2
    if C == 2:
        last[0] = 1
    cat[1, :] = 0
    t = OR.grid()
    K = np.sort(np.stack([rng.choice(np.arange(60, 181), C - 1, replace=False) for _ in range(m)]), axis=1).astype(np.int32)
    return np.asfortranarray(cat), t, K


def theta_start(n, seed):
    rng = np.random.default_rng(seed + 1000)
    return -5.0 + 0.01 * np.clip(np.rint((rng.standard_normal(n) + 5.0) / 0.01), 0, 1000)


def slice_case(n, m, C, seed):
    """A constructed state for the slice, the theta product and the slope: make_case's categories and thresholds, f of unit
    scale with rows beyond |g - b| = 40 (rows 5, 6) and around exp()'s range 709 (rows 7, 8, item 1 only: such a row under a
    category that contradicts it costs ~700 in log-likelihood), slopes of both signs and mu = theta * slope."""
    cat, t, K = make_case(n, m, C, seed)
    rng = np.random.default_rng(seed + 7)
    f = np.asfortranarray(rng.standard_normal((n, m)))
    f[5, :], f[6, :] = 45.0, -50.0
    if m > 1:
        f[7, 1], f[8, 1] = 705.0, -712.0
    theta = theta_start(n, seed)
    slopes = rng.uniform(0.5, 1.5, m) * np.where(np.arange(m) % 2 == 0, 1.0, -1.0)
    mu = np.asfortranarray(theta[:, None] * slopes[None, :])
    return dict(cat=cat, t=t, K=K, f=f, mu=mu, theta=theta, slopes=slopes)
