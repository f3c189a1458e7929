"""Ordinal (graded) responses: the cumulative-logit model with the thresholds sampled in the chain (library version 139;
include/gpirt_hip.h "ordinal (graded) responses", csrc/ordinal.hip).

With g = f + mu and an item's thresholds b_1 < ... < b_{C-1} (b_0 = -inf, b_C = +inf),

    log P(y = c | g, b) = -ll(b_c - g) [c < C] - ll(g - b_{c-1}) [c > 1] + w(b_c - b_{c-1}) [1 < c < C]
    ll(a) = log(1 + e^-a),   w(d) = log1p(-e^-d)

cat is n x m, 0 = missing, 1 .. C a category.  The sampler is created on `dichotomise(cat)` and turned ordinal by
Sampler.ordinal_enable; `run` is the one-call way in.  The intercept is pinned at 0: location is the thresholds'.

The NumPy statement: `loglik` (the model; float64 as written, or long double), `slice_exact`, `theta_logpost_exact`, `beta_exact`,
`threshold_conditional` (the masses of one threshold update) and `thresholds_exact` (a whole draw_thresholds).  They work in
long double and report the MARGIN of every decision, so that a test can tell a decided decision from one inside the rounding
band (tests/_ordinal_bounds.py derives the band)."""
from __future__ import annotations

import ctypes as ct

import numpy as np

from . import _lib
from ._lib import NGRID, OFIT_CAT_FIELDS, OFIT_PARTS, OFIT_TOTALS, OFIT_UNIT_FIELDS, ST_ORD, ST_ORD_PPC, check

LD = np.longdouble
ST_F_ESS, ST_BETA = 4, 7
TWO_PI = 6.283185307179586476925286766559
_dp = ct.POINTER(ct.c_double)


def _p(a):
    return a.ctypes.data_as(_dp)


# ---------------------------------------------------------------------------------------------------- the contract ---
def grid(hi=6.0, points=241) -> np.ndarray:
    """t_k = hi (2k - (P - 1)) / (P - 1): gpirt_ordinal_grid (long double, rounded once; the centre exactly 0, the ends exact)."""
    out = np.empty(int(points))
    check(_lib.load().gpirt_ordinal_grid(float(hi), int(points), _p(out)))
    return out


def default_log_prior(t) -> np.ndarray:
    """-t^2 / 18: the normal with sd 3 of beta_prior_sds, the expression Sampler.ordinal_enable(log_prior=None) uses."""
    t = np.asarray(t, dtype=np.float64)
    return -(t * t) / 18.0


def categories(cat, C=None) -> int:
    return int(C) if C is not None else int(np.max(cat))


def dichotomise(cat) -> np.ndarray:
    """+1 above the item's median observed category (the lower median), -1 otherwise, NaN where cat = 0: the binary matrix the
    sampler is created on.  While ordinal is on nothing of the chain reads it but its NaN pattern."""
    cat = np.asarray(cat)
    y = np.full(cat.shape, np.nan)
    for j in range(cat.shape[1]):
        col = cat[:, j]
        obs = col > 0
        if not obs.any():
            continue
        srt = np.sort(col[obs])
        med = srt[(srt.size - 1) // 2]
        y[obs, j] = np.where(col[obs] > med, 1.0, -1.0)
    return np.asfortranarray(y)


def init_thresholds(cat, t, C=None) -> np.ndarray:
    """Start indices (m x (C - 1) int32) from the data: the logit of the item's cumulative proportions P(cat <= c), clipped to
    [0.5 / N, 1 - 0.5 / N], snapped to the nearest grid point and spread to distinct, strictly increasing points (forward, then
    backward from the grid's end) -- also where a category is empty."""
    cat = np.asarray(cat)
    t = np.asarray(t, dtype=np.float64)
    Cn, P, m = categories(cat, C), t.size, cat.shape[1]
    if P < Cn - 1:
        raise ValueError("init_thresholds: the grid has fewer points than thresholds")
    K = np.empty((m, Cn - 1), dtype=np.int32)
    for j in range(m):
        col = cat[:, j]
        N = max(int((col > 0).sum()), 1)
        for c in range(1, Cn):
            p = min(max(((col > 0) & (col <= c)).sum() / N, 0.5 / N), 1.0 - 0.5 / N)
            K[j, c - 1] = int(np.argmin(np.abs(t - np.log(p / (1.0 - p)))))
        for c in range(1, Cn - 1):
            K[j, c] = max(K[j, c], K[j, c - 1] + 1)
        for c in range(Cn - 2, -1, -1):
            K[j, c] = min(K[j, c], P - 1 - (Cn - 2 - c))
    return K


def check_args(cat=None, y=None, C=2, hi=6.0, points=241, log_prior=None, K0=None, width=16, options=None) -> None:
    """gpirt_ordinal_check (no device is touched): every refusal of Sampler.ordinal_enable's arguments as a GpirtError that
    names its reason.  y: the sampler's binary matrix (NaN exactly where cat is 0).  options: a gpirt_options or None."""
    c8 = None if cat is None else np.asfortranarray(np.asarray(cat, dtype=np.int64).clip(-128, 127).astype(np.int8))
    n, m = (0, 0) if c8 is None else c8.shape
    yy = None if y is None or c8 is None else np.asfortranarray(np.asarray(y, dtype=np.float64))
    if yy is not None and yy.shape != c8.shape:
        raise ValueError("ordinal: y and cat must have the same shape")
    lp = None if log_prior is None else np.ascontiguousarray(log_prior, dtype=np.float64).reshape(-1)
    if lp is not None and lp.shape != (int(points),):
        raise ValueError(f"ordinal: log_prior must hold points = {int(points)} values")
    k0 = None if K0 is None else np.ascontiguousarray(K0, dtype=np.int32)
    mm = m
    if k0 is not None:
        if k0.ndim != 2 or k0.shape[1] != max(int(C) - 1, 0) or (c8 is not None and k0.shape[0] != m):
            raise ValueError("ordinal: K0 must be m x (C - 1)")
        mm = k0.shape[0]
    check(_lib.load().gpirt_ordinal_check(None if c8 is None else c8.ctypes.data_as(ct.POINTER(ct.c_int8)),
                                          None if yy is None else _p(yy), n, mm, int(C), float(hi), int(points),
                                          None if lp is None else _p(lp),
                                          None if k0 is None else k0.ctypes.data_as(ct.POINTER(ct.c_int32)), int(width),
                                          None if options is None else ct.byref(options)))


def uniforms(seed, t, item, C) -> np.ndarray:
    """The 2 (C - 1) uniforms of item `item` in the t-th draw_thresholds call (t from 1): item_uniform(seed, t, GPIRT_ST_ORD,
    item, 2 (c - 1)) places threshold c's window, (.., 2 (c - 1) + 1) draws it."""
    from .ppc import item_uniform
    return np.asarray(item_uniform(seed, int(t), ST_ORD, np.uint64(item), np.arange(2 * (int(C) - 1), dtype=np.uint64)), dtype=np.float64)


# ------------------------------------------------------------------------------------------------------- NumPy -------
def ll(a):
    """log(1 + e^-a).  float64: as written (src/log-likelihood.cpp: np.log(1 + np.exp(-a)), the oracle's bits); long double:
    max(-a, 0) + log1p(e^-|a|), accurate at every a."""
    a = np.asarray(a)
    if a.dtype == LD:
        return np.maximum(-a, LD(0)) + np.log1p(np.exp(-np.abs(a)))
    with np.errstate(over="ignore"):
        return np.log(1 + np.exp(-a))


def w(d):
    """log1p(-e^-d), d > 0: the normaliser's part of an interior category."""
    return np.log1p(-np.exp(-np.asarray(d)))


def _bounds(b, dtype):
    b = np.asarray(b, dtype=dtype).reshape(-1)
    return np.concatenate([[dtype(-np.inf)], b, [dtype(np.inf)]])


def loglik(cat, g, b, with_w=True, dtype=np.float64) -> np.ndarray:
    """log P(y = cat_i | g_i, b) per cell (0 where cat_i = 0): -ll(b_c - g) if c < C, then -ll(g - b_{c-1}) if c > 1 (in that
    order), then + w(b_c - b_{c-1}) for an interior c (with_w=False: without it, as the slice, theta and beta see the cell).
    b: the item's C - 1 thresholds.  With C = 2 and b = [0] the float64 value is -log(1 + exp(-y g)) bit for bit."""
    cat = np.asarray(cat)
    g = np.asarray(g, dtype=dtype)
    bb = _bounds(b, dtype)
    Cn = bb.size - 1
    out = np.zeros(g.shape, dtype=dtype)
    for c in range(1, Cn + 1):
        sel = cat == c
        if not sel.any():
            continue
        v = np.zeros(int(sel.sum()), dtype=dtype)
        if c < Cn:
            v = -ll(bb[c] - g[sel])
        if c > 1:
            v = v - ll(g[sel] - bb[c - 1])
        if with_w and 1 < c < Cn:
            v = v + w(bb[c] - bb[c - 1])
        out[sel] = v
    return out


def category_logprobs(g, b, dtype=LD) -> np.ndarray:
    """log P(y = c | g, b) for c = 1 .. C: an array of shape (C,) + g.shape."""
    g = np.asarray(g, dtype=dtype)
    Cn = np.asarray(b).size + 1
    return np.stack([loglik(np.full(g.shape, c), g, b, True, dtype) for c in range(1, Cn + 1)])


def n_terms(cat, C) -> int:
    """The ll evaluations of a column: one per observed end-category cell, two per interior one."""
    cat = np.asarray(cat)
    return int((cat > 0).sum() + ((cat > 1) & (cat < int(C))).sum())


def slice_exact(cat, f, nu, mu, b, u, max_trials=100000) -> dict:
    """The elliptical slice of one item in long double, from the uniforms u = item_uniform(seed, iter, GPIRT_ST_F_ESS, item, 0 ..):
    u[0] the level, u[1] the first angle, one more per rejection.  The angles and their brackets are formed in float64 as the
    kernel forms them (the bracket rule of src/draw-f.cpp:33-56).  Returns k (rejections), eps (every trial angle), margins (long
    double ll(f') - log_y of every trial point: > 0 accepts), ll0 and f_new = f cos(eps) + nu sin(eps) in float64."""
    cat = np.asarray(cat)
    f64, nu64 = np.asarray(f, dtype=np.float64), np.asarray(nu, dtype=np.float64)
    fl, nl, ml = f64.astype(LD), nu64.astype(LD), np.asarray(mu, dtype=np.float64).astype(LD)
    ll0 = loglik(cat, fl + ml, b, False, LD).sum()
    log_y = ll0 + np.log(LD(u[0]))
    eps_min, eps_max = 0.0, TWO_PI
    eps = eps_min + (eps_max - eps_min) * float(u[1])
    eps_min = eps - TWO_PI
    k, ui, angles, margins = 0, 2, [], []
    while True:
        c, s = np.cos(eps), np.sin(eps)
        llp = loglik(cat, (fl * LD(c) + nl * LD(s)) + ml, b, False, LD).sum()
        angles.append(eps)
        margins.append(llp - log_y)
        if llp > log_y:
            break
        if np.isnan(llp):
            break
        if eps < 0.0:
            eps_min = eps
        else:
            eps_max = eps
        if eps_min == eps_max:
            eps = eps_min
        else:
            eps = eps_min + (eps_max - eps_min) * float(u[ui])
            ui += 1
        k += 1
        if k >= max_trials:
            break
    return dict(k=k, eps=np.array(angles), margins=np.array(margins, dtype=LD), ll0=ll0, log_y=log_y,
                f_new=f64 * np.cos(eps) + nu64 * np.sin(eps))


def theta_logpost_exact(cat, fstar, B) -> np.ndarray:
    """logpost[k, i] = sum over the items j respondent i answered of (-ll(b_c - f*_kj) [c < C] - ll(f*_kj - b_{c-1}) [c > 1]),
    c = cat_ij, in long double (N x n).  B: m x (C - 1) threshold values.  A non-finite f* under a missing cell is skipped."""
    cat = np.asarray(cat)
    fs = np.asarray(fstar, dtype=np.float64).astype(LD)
    B = np.asarray(B, dtype=np.float64)
    N, m = fs.shape
    Cn = B.shape[1] + 1
    lp = np.zeros((N, cat.shape[0]), dtype=LD)
    for j in range(m):
        for c in range(1, Cn + 1):
            who = cat[:, j] == c
            if who.any():
                col = loglik(np.full(N, c), fs[:, j], B[j], False, LD)
                lp[:, who] += col[:, None]
    return lp


def beta_exact(cat, f, theta, beta1, b, step, pm, ps, u_norm, u_dec, beta0=0.0) -> dict:
    """The slope's MH step of one item in long double (the k = 1 pass of src/draw-beta.cpp under the ordinal likelihood): the
    proposal beta1 + step qnorm(u_norm) in float64 as the kernel forms it, r = prior' + ll' - prior - ll and the margin
    r - log(u_dec) (> 0 accepts)."""
    from .amp import _qnorm
    cat = np.asarray(cat)
    z = float(_qnorm(np.array([float(u_norm)]))[0])
    prop = float(beta1) + float(step) * z
    th = np.asarray(theta, dtype=np.float64)
    fl = np.asarray(f, dtype=np.float64).astype(LD)

    def mean(b1):                     # cv0 + theta * cv1, each operation rounded in float64 as the kernel's
        return (float(beta0) + th * b1).astype(LD)

    def prior(x):
        zz = abs((LD(x) - LD(pm)) / LD(ps))
        return -(LD(0.918938533204672741780329736406) + LD(0.5) * zz * zz + np.log(LD(ps)))
    llp = loglik(cat, fl + mean(prop), b, False, LD).sum()
    llc = loglik(cat, fl + mean(float(beta1)), b, False, LD).sum()
    r = prior(prop) + llp - prior(float(beta1)) - llc
    margin = r - np.log(LD(u_dec))
    return dict(proposal=prop, r=r, margin=margin, accept=bool(margin > 0), ll_prop=llp, ll_cur=llc)


def window(k, u0, W) -> int:
    """The first index a of the window [a, a + W) that u0 places around the current index k: a = k - (int)(u0 W)."""
    return int(k) - min(int(float(u0) * int(W)), int(W) - 1)


def candidates(a, W, left, right, P) -> tuple:
    """(lo, hi): the window's points strictly between the neighbouring indices (left = -1, right = P stand in for the ends) and
    inside the grid.  The set does not depend on the current index."""
    return max(int(a), int(left) + 1, 0), min(int(a) + int(W) - 1, int(right) - 1, int(P) - 1)


def threshold_conditional(cat, g, t, log_prior, K, c, a, W, dtype=LD) -> np.ndarray:
    """The log masses of threshold c's update of one item over the window [a, a + W): W values, -inf outside the candidates.
    K: the item's C - 1 current indices (those left of c already updated).  A single candidate gives 0 at its slot, as the
    kernel reports it.  For candidate q, in csrc/ordinal.hip's order:
        m_q = log_prior[q] - S,  S = sum over the cells with cat = c of ll(t_q - g_i) and with cat = c + 1 of ll(g_i - t_q)
        + N_c w(t_q - t_left) if there is a left neighbour,  + N_{c+1} w(t_right - t_q) if there is a right one."""
    cat = np.asarray(cat)
    t64 = np.asarray(t, dtype=np.float64)
    tt, pr = t64.astype(dtype), np.asarray(log_prior, dtype=np.float64).astype(dtype)
    gg = np.asarray(g, dtype=np.float64).astype(dtype)
    K = [int(x) for x in np.asarray(K).reshape(-1)]
    Cn, P = len(K) + 1, t64.size
    left = K[c - 2] if c >= 2 else -1
    right = K[c] if c <= Cn - 2 else P
    lo, hi = candidates(a, W, left, right, P)
    out = np.full(int(W), -np.inf, dtype=dtype)
    if lo >= hi:
        out[K[c - 1] - a] = 0
        return out
    lower, upper = gg[cat == c], gg[cat == c + 1]
    nc, nc1 = dtype(lower.size), dtype(upper.size)
    for q in range(lo, hi + 1):
        S = ll(tt[q] - lower).sum() + ll(upper - tt[q]).sum()
        mq = pr[q] - S
        if left >= 0:
            mq = mq + nc * w(tt[q] - tt[left])
        if right < P:
            mq = mq + nc1 * w(tt[right] - tt[q])
        out[q - a] = mq
    return out


def grid_draw(lp, u1) -> dict:
    """The draw from a row of log masses: maximum, exp, ascending cumulative sums, the first slot whose cumulative sum exceeds
    u1 * total.  margin: the smallest |cum - u1 total| / total over the slots, the distance of u1 from a step of the CDF."""
    lp = np.asarray(lp)
    cand = np.flatnonzero(lp > -np.inf)
    if not np.all(np.isfinite(lp[cand])) or cand.size == 0:
        return dict(slot=None, failed=True, margin=LD(0))
    e = np.exp(lp[cand] - lp[cand].max())
    cum = np.cumsum(e)
    target = lp.dtype.type(u1) * cum[-1]
    hit = np.flatnonzero(cum > target)
    slot = int(cand[hit[0]]) if hit.size else int(cand[-1])
    return dict(slot=slot, failed=False, margin=np.min(np.abs(cum - target)) / cum[-1], probs=e / cum[-1], slots=cand)


def thresholds_exact(cat, g, t, log_prior, K, seed, call, W=16, item0=0) -> dict:
    """A whole draw_thresholds in long double: every item, c = 1 .. C - 1 in order, each threshold seeing the updated left
    neighbour.  cat, g: n x m; K: m x (C - 1).  Returns index (the new K), window (the a of every update), lp (m x (C - 1) x W),
    margin (of every draw; inf where nothing was drawn), pinned, failed, updates."""
    cat, g = np.asarray(cat), np.asarray(g, dtype=np.float64)
    K = np.array(K, dtype=np.int64)
    m, R = K.shape
    lp = np.full((m, R, int(W)), -np.inf, dtype=LD)
    win = np.zeros((m, R), dtype=np.int64)
    margin = np.full((m, R), np.inf, dtype=LD)
    pinned = failed = updates = 0
    for j in range(m):
        u = uniforms(seed, call, item0 + j, R + 1)
        for c in range(1, R + 1):
            a = window(K[j, c - 1], u[2 * (c - 1)], W)
            win[j, c - 1] = a
            row = threshold_conditional(cat[:, j], g[:, j], t, log_prior, K[j], c, a, W)
            lp[j, c - 1] = row
            lo, hi = candidates(a, W, K[j, c - 2] if c >= 2 else -1, K[j, c] if c <= R - 1 else len(t), len(t))
            if lo >= hi:
                pinned += 1
                continue
            d = grid_draw(row, u[2 * (c - 1) + 1])
            if d["failed"]:
                failed += 1
                break
            K[j, c - 1] = a + d["slot"]
            margin[j, c - 1] = d["margin"]
            updates += 1
    return dict(index=K.astype(np.int32), window=win.astype(np.int32), lp=lp, margin=margin, pinned=pinned, failed=failed,
                updates=updates)


def transition_matrix(cat, g, t, log_prior, K, c, W) -> tuple:
    """The exact transition matrix of threshold c's update over its allowed indices (strictly between the neighbours, on the
    grid) and the full conditional pi on them: T[k, q] = (1 / W) sum over the W placements a = k - W + 1 .. k of the window's
    normalised masses.  pi T = pi is what makes the move leave the posterior invariant."""
    K = [int(x) for x in np.asarray(K).reshape(-1)]
    P = len(t)
    left = K[c - 2] if c >= 2 else -1
    right = K[c] if c <= len(K) - 1 else P
    allowed = np.arange(max(left + 1, 0), min(right - 1, P - 1) + 1)
    full = threshold_conditional(cat, g, t, log_prior, K, c, int(allowed[0]), int(allowed.size) if allowed.size > 1 else 2)[:allowed.size]
    if allowed.size == 1:
        return allowed, np.ones((1, 1), dtype=LD), np.ones(1, dtype=LD)
    pi = np.exp(full - full.max())
    pi = pi / pi.sum()
    T = np.zeros((allowed.size, allowed.size), dtype=LD)
    for ik, k in enumerate(allowed):
        Kk = list(K)
        Kk[c - 1] = int(k)
        for off in range(int(W)):
            a = int(k) - off
            row = threshold_conditional(cat, g, t, log_prior, Kk, c, a, W)
            slots = np.flatnonzero(row > -np.inf)
            p = np.exp(row[slots] - row[slots].max())
            p = p / p.sum()
            T[ik, a + slots - allowed[0]] += p / LD(W)
    return allowed, T, pi


# ------------------------------------------------------------------------------------------------------ summaries ----
def summarise(draws, t, probs=(0.025, 0.25, 0.5, 0.75, 0.975)) -> dict:
    """Recorded threshold indices (... x m x (C - 1), any leading draw and chain axes) on the grid t: thresholds (the values of
    the draws), mean, sd and quantiles per item and threshold over all leading axes."""
    d = np.asarray(draws)
    t = np.asarray(t, dtype=np.float64)
    vals = t[d.clip(0, t.size - 1)]
    flat = vals.reshape(-1, *d.shape[-2:])
    return dict(draws=d, thresholds=vals, mean=flat.mean(axis=0), sd=flat.std(axis=0),
                quantiles=np.quantile(flat, np.asarray(probs), axis=0), probs=np.asarray(probs))


def curves(cum, draws) -> dict:
    """From Sampler.ordinal_get("cum") (m x (C - 1) x 1001 sums of P(y > c | theta_k)) and the number of accumulated draws:
    exceed (the posterior mean of P(y > c | theta)), probs (m x C x 1001: P(y = c | theta) = exceed_{c-1} - exceed_c with
    exceed_0 = 1, exceed_C = 0), expected (m x 1001: the expected score sum_c c P(y = c)) and theta (the grid)."""
    ex = np.asarray(cum, dtype=np.float64) / float(draws)
    m, R, N = ex.shape
    full = np.concatenate([np.ones((m, 1, N)), ex, np.zeros((m, 1, N))], axis=1)
    probs = full[:, :-1] - full[:, 1:]
    expected = (probs * np.arange(1, R + 2)[None, :, None]).sum(axis=1)
    return dict(exceed=ex, probs=probs, expected=expected, theta=-5.0 + 0.01 * np.arange(N))


def make_graded(n, m, C, seed=20240, na_frac=0.1, slopes=None, thresholds=None) -> dict:
    """Graded-response data from known theta (grid points), slopes and ordered thresholds: cat (n x m int8, about na_frac
    missing), theta, slopes, thresholds (m x (C - 1))."""
    rng = np.random.default_rng(seed)
    theta = -5.0 + 0.01 * np.clip(np.rint((rng.standard_normal(n) + 5.0) / 0.01), 0, NGRID - 1)
    a = rng.uniform(0.8, 2.0, m) * rng.choice([-1.0, 1.0], m) if slopes is None else np.asarray(slopes, dtype=np.float64)
    B = np.sort(rng.uniform(-2.0, 2.0, (m, C - 1)), axis=1) if thresholds is None else np.asarray(thresholds, dtype=np.float64)
    g = theta[:, None] * a[None, :]
    exceed = 1.0 / (1.0 + np.exp(-(g[:, :, None] - B[None, :, :])))           # P(y > c)
    u = rng.random((n, m, 1))
    cat = (1 + (u < exceed).sum(axis=2)).astype(np.int8)
    cat[rng.random((n, m)) < na_frac] = 0
    return dict(cat=np.asfortranarray(cat), theta=theta, slopes=a, thresholds=B)


# ------------------------------------------------------------------------------------------------------ model fit ----
# (include/gpirt_hip.h "ordinal model fit", csrc/ordinal_fit.hip; library version 142) pointwise WAIC, per-cell
# category predictions and the first-order posterior predictive check, accumulated on the device one draw at a time.
# `fit_result` finishes the raw accumulators on the host, `fit_combine` pools chains' state blocks, `fit_from_draws` is the NumPy
# statement over stored draws.
FIT_INT_UNIT = OFIT_UNIT_FIELDS[:9]
FIT_U_TOL = 1e-13         # |u - e_c| at or below: the cell's replicate is undecided
FIT_D_TOL = 1e-10         # 0 < |Delta| <= FIT_D_TOL sum_changed (|logP(cat)| + |logP(rep)|): the deviance comparison is undecided


def fit_parts(parts) -> int:
    """The GPIRT_OFIT_* bits of a tuple of part names ("waic", "pred", "ppc"); an int is passed through, None / () / False is 0,
    True is every part."""
    if parts is True:
        return 7
    if parts is None or parts is False:
        return 0
    if isinstance(parts, (int, np.integer)):
        return int(parts)
    bits = 0
    for k in ((parts,) if isinstance(parts, str) else tuple(parts)):
        if k not in OFIT_PARTS:
            raise ValueError(f"ordinal fit: unknown part {k!r}; the parts are {tuple(OFIT_PARTS)}")
        bits |= OFIT_PARTS[k]
    return bits


def fit_array(name, n, m, C) -> np.ndarray:
    """An empty host array of the shape and type the fit block's array `name` has (gpirt_sampler_ordinal_fit_get)."""
    if name == "draws":
        return np.empty(1, dtype=np.int64)
    if name in ("lse", "ll_mean", "ll_m2"):
        return np.empty((n, m), order="F")
    if name == "pred_sum":
        return np.empty((C - 1, m, n)).transpose(0, 2, 1)           # C - 1 planes of column-major n x m
    if name == "rep":
        return np.empty((n, m), dtype=np.int8, order="F")
    if name == "delta":
        return np.empty(m + n + 1)
    if name == "score":
        return np.empty(m + n + 1, dtype=np.int64)
    if name == "counts_rep":
        return np.empty((m, C), dtype=np.int64)
    for pre, size in (("item_", m), ("respondent_", n), ("total_", 1)):
        if name.startswith(pre):
            fld = name[len(pre):]
            return np.empty(size, dtype=np.float64 if fld in ("dev_obs_sum", "dev_rep_sum") else np.uint64)
    if name.startswith("cat_"):
        return np.empty((m, C), dtype=np.uint64)
    return np.empty(0)


def _fit_get_into(entry, first, name, out):
    base = out.base if out.base is not None and name == "pred_sum" else out
    check(entry(*first, name.encode(), ct.c_void_p(base.ctypes.data), base.nbytes))
    return out


def fit_block_header(state) -> dict:
    """The header of a fit state block (a device tensor): n, m, categories, parts, draws, item0, layout version."""
    w = _lib.header_words(state, 8)
    return dict(version=int(w[1]), n=int(w[2]), m=int(w[3]), categories=int(w[4]), parts=int(w[5]), draws=int(w[6]), item0=int(w[7]))


def fit_block_get(handle, state, name) -> np.ndarray:
    """gpirt_ordinal_fit_get: one raw accumulator of a fit state block, one chain's or a pooled one."""
    h = fit_block_header(state)
    out = fit_array(name, h["n"], h["m"], h["categories"])
    return _fit_get_into(_lib.load().gpirt_ordinal_fit_get, (handle.ptr, ct.c_void_p(state.data_ptr())), name, out)


def _fit_totals_dict(t) -> dict:
    out = {k: int(getattr(t, k)) for k in ("n", "m", "categories", "parts", "draws", "n_obs")}
    out.update({k: float(getattr(t, k)) for k in OFIT_TOTALS})
    return out


def fit_block_totals(handle, state) -> dict:
    """gpirt_ordinal_fit_totals of a fit state block."""
    t = _lib.OrdinalFit()
    check(_lib.load().gpirt_ordinal_fit_totals(handle.ptr, ct.c_void_p(state.data_ptr()), ct.byref(t)))
    return _fit_totals_dict(t)


def _exact_var(S, s1, s2):
    """(S sum R^2 - (sum R)^2) / (S (S - 1)): the numerator in exact integers, rounded once"""
    S, s1, s2 = (np.asarray(x).reshape(-1) for x in (S, s1, s2))
    out = np.full(S.size, np.nan)
    for k in range(S.size):
        Sk = int(S[k])
        if Sk >= 2:
            out[k] = float(Sk * int(s2[k]) - int(s1[k]) ** 2) / (float(Sk) * float(Sk - 1))
    return out


def fit_derive_units(d, draws) -> dict:
    """The derived fields of one kind of unit from its raw sums (ppc.derive's conventions): S = draws - nonfinite, NaN where
    S = 0 or the unit has no observed cell; ppp_score = score_ge / S, ppp_score_mid = (score_ge + score_gt) / 2S, rep_score_mean,
    rep_score_var (from the exact integer sums), ppp_dev = dev_ge / S, dev_obs_mean, dev_rep_mean, agree_mean."""
    f = lambda k: np.asarray(d[k]).astype(np.float64)       # noqa: E731
    nobs = np.asarray(d["n_obs"])
    Si = int(draws) - np.asarray(d["nonfinite"]).astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        S = np.where((Si > 0) & (nobs > 0), Si, np.nan).astype(np.float64)
        d["ppp_score"] = f("score_ge") / S
        d["ppp_score_mid"] = (f("score_ge") + f("score_gt")) / (2.0 * S)
        d["rep_score_mean"] = f("rep_score_sum") / S
        d["rep_score_var"] = np.where(nobs > 0, _exact_var(Si, d["rep_score_sum"], d["rep_score_sumsq"]).reshape(nobs.shape), np.nan)
        d["ppp_dev"] = f("dev_ge") / S
        d["dev_obs_mean"] = f("dev_obs_sum") / S
        d["dev_rep_mean"] = f("dev_rep_sum") / S
        d["agree_mean"] = f("agree_sum") / S
    d["draws"] = int(draws)
    return d


def fit_derive_categories(d, item, draws) -> dict:
    """ppp_count = count_ge / S, ppp_count_mid = (count_ge + count_gt) / 2S and rep_count_mean = rep_count_sum / S per (item,
    category), S the item's draws - nonfinite (NaN for an item without an observed cell)."""
    Si = int(draws) - np.asarray(item["nonfinite"]).astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        S = np.where((Si > 0) & (np.asarray(item["n_obs"]) > 0), Si, np.nan).astype(np.float64)[:, None]
        ge, gt = np.asarray(d["count_ge"]).astype(np.float64), np.asarray(d["count_gt"]).astype(np.float64)
        d["ppp_count"] = ge / S
        d["ppp_count_mid"] = (ge + gt) / (2.0 * S)
        d["rep_count_mean"] = np.asarray(d["rep_count_sum"]).astype(np.float64) / S
    return d


def fit_pred(pred_sum, draws, cat=None) -> dict:
    """From the sums of e_c = P(y > c) ((C - 1) x n x m) and the draws, as `curves` does for the grid: exceed (n x m x (C - 1)),
    probs (n x m x C, by difference of the means), expected (the expected category) and, with cat, p_observed (the mean
    probability of the category that was seen; NaN for a missing cell)."""
    ex = np.moveaxis(np.asarray(pred_sum, dtype=np.float64), 0, 2) / float(draws)
    n, m, R = ex.shape
    full = np.concatenate([np.ones((n, m, 1)), ex, np.zeros((n, m, 1))], axis=2)
    probs = full[:, :, :-1] - full[:, :, 1:]
    out = dict(exceed=ex, probs=probs, expected=(probs * np.arange(1, R + 2)[None, None, :]).sum(axis=2))
    if cat is not None:
        cat = np.asarray(cat).astype(np.int64)
        po = np.take_along_axis(probs, np.clip(cat - 1, 0, R)[:, :, None], axis=2)[:, :, 0]
        out["p_observed"] = np.where(cat > 0, po, np.nan)
    return out


def fit_result(get, totals, cat=None) -> dict:
    """The finished fit output from a getter of raw arrays (name -> array) and the totals dict: "waic" (lse, ll_mean, ll_m2, lppd,
    p_waic, elpd per cell; NaN for a missing one), "pred" (`fit_pred`), "item", "respondent" (raw sums and `fit_derive_units`),
    "categories" (`fit_derive_categories`) and "totals" (the WAIC totals and the whole matrix's PPC fields); a part that is not
    enabled is None."""
    parts, S = totals["parts"], totals["draws"]
    out = dict(waic=None, pred=None, item=None, respondent=None, categories=None, totals=dict(totals))
    if parts & OFIT_PARTS["waic"]:
        lse, mean, m2 = get("lse"), get("ll_mean"), get("ll_m2")
        miss = m2 == -1.0
        with np.errstate(invalid="ignore", divide="ignore"):
            lppd = np.where(miss, np.nan, lse - np.log(float(S))) if S >= 1 else np.full(lse.shape, np.nan)
            pw = np.where(miss, np.nan, m2 / float(S - 1)) if S >= 2 else np.full(lse.shape, np.nan)
        out["waic"] = dict(lse=lse, ll_mean=mean, ll_m2=m2, lppd=lppd, p_waic=pw, elpd=lppd - pw)
    if parts & OFIT_PARTS["pred"]:
        out["pred"] = fit_pred(get("pred_sum"), S, cat) if S >= 1 else None
    if parts & OFIT_PARTS["ppc"]:
        for unit in ("item", "respondent"):
            out[unit] = fit_derive_units({k: get(f"{unit}_{k}") for k in OFIT_UNIT_FIELDS}, S)
        tot = fit_derive_units({k: get(f"total_{k}") for k in OFIT_UNIT_FIELDS}, S)
        out["totals"].update({k: (v if isinstance(v, int) else v.reshape(-1)[0].item()) for k, v in tot.items()})
        out["categories"] = fit_derive_categories({k: get(f"cat_{k}") for k in OFIT_CAT_FIELDS}, out["item"], S)
    return out


def fit_combine(handle, states, cat=None) -> dict:
    """gpirt_ordinal_fit_combine over the fit state blocks `states` (device tensors, or Samplers with ordinal_fit_enable on, all on
    handle's device), in chain order: counts added, Chan's formula for the Welford pairs, a logaddexp for lse.  No signs: theta ->
    -theta with the slope leaves f + mu and the thresholds as they are.  Returns `fit_result` of the pooled block and the block
    itself as "state" (a device tensor that `fit_block_get` and `fit_block_totals` read as they read one chain's)."""
    import torch
    tensors, nc, ptrs = _lib.state_ptrs(states, "ordinal_fit_state")
    pooled = torch.empty_like(tensors[0])
    check(_lib.load().gpirt_ordinal_fit_combine(handle.ptr, ptrs, nc, ct.c_void_p(pooled.data_ptr())))
    out = fit_result(lambda name: fit_block_get(handle, pooled, name), fit_block_totals(handle, pooled), cat)
    out["state"] = pooled
    return out


def _fit_terms(g, B):
    """Per threshold c = 1 .. C - 1 (axis 0) of every cell, in float64 and the kernel's operations: e_c = P(y > c),
    up_c = ll(b_c - g), lo_c = ll(g - b_c) with ll(a) = log1p(e^-|a|) + max(-a, 0) from ONE E_c = exp(-|g - b_c|)."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = g[None, :, :] - B.T[:, None, :]
        E = np.exp(-np.abs(d))
        e = np.where(d >= 0, 1.0 / (1.0 + E), E / (1.0 + E))
        l1 = np.log1p(E)
        return e, l1 + np.maximum(d, 0.0), l1 + np.maximum(-d, 0.0)


def _fit_logp(K, up, lo, W):
    """logP(K) per cell (K: n x m categories 1 .. C) in the header's order: -up_K if K < C, then - lo_{K-1} if K > 1, then + w_K for
    an interior K.  W: m x (C + 1), W[j, c] = w(b_c - b_{c-1}) for 1 < c < C and 0 elsewhere."""
    R = up.shape[0]
    Cn = R + 1
    with np.errstate(invalid="ignore"):
        v = np.zeros(K.shape)
        iu = np.clip(K - 1, 0, R - 1)[None]
        il = np.clip(K - 2, 0, R - 1)[None]
        v = np.where(K < Cn, -np.take_along_axis(up, iu, axis=0)[0], v)
        v = np.where(K > 1, v - np.take_along_axis(lo, il, axis=0)[0], v)
        wk = np.take_along_axis(W, np.clip(K, 0, Cn).T, axis=1).T
        v = np.where((K > 1) & (K < Cn), v + wk, v)
    return v


def fit_from_draws(cat, g_draws, threshold_draws, seed, iters, item0=0, stage=ST_ORD_PPC) -> dict:
    """What the device accumulates, from stored draws: cat (n x m; 0 = missing), g_draws (S, n, m) the draws of g = f + mu,
    threshold_draws (S, m, C - 1) the threshold VALUES of each draw, `iters` the S completed-iteration counters.  It follows
    ppc.from_draws' convention: every integer field of "item", "respondent", "totals" and "categories" is a pair (lo, hi) of int64
    arrays -- a cell with |u - e_c| <= 1e-13 for some c may replicate either way, a deviance comparison with such a cell in it, or
    with 0 < |Delta| <= 1e-10 sum_changed (|logP(cat)| + |logP(rep)|), may go either way.  The double fields (dev_obs_sum,
    dev_rep_sum, "pred_sum") are float64 with the undecided cells at rep = 1 + #{c : u < e_c}; "waic" is the long-double reference
    (lse, ll_mean, ll_m2, lppd, p_waic, ll_absmax = max_s |logP_s| per cell and the totals).  "rep": the S replicates (0: missing or non-finite); "undecided"
    counts cells and comparisons, "comparisons" every deviance comparison made."""
    from .ppc import item_uniform
    cat = np.asarray(cat).astype(np.int64)
    g_draws = np.asarray(g_draws, dtype=np.float64)
    B_draws = np.asarray(threshold_draws, dtype=np.float64)
    n, m = cat.shape
    S = g_draws.shape[0]
    R = B_draws.shape[2]
    Cn = R + 1
    iters = [int(x) for x in iters]
    assert g_draws.shape == (S, n, m) and B_draws.shape == (S, m, R) and len(iters) == S
    obs = cat > 0
    units = (("item", 0, m), ("respondent", 1, n), ("totals", None, 1))

    def usum(a, axis):
        return a.sum(axis=axis) if axis is not None else np.array([a.sum()])

    acc = {}
    zi = lambda size: np.zeros(size, dtype=np.int64)      # noqa: E731
    for name, axis, size in units:
        acc[name] = dict(n_obs=usum(obs, axis).astype(np.int64), obs_score=usum(cat, axis).astype(np.int64), nonfinite=zi(size),
                         dev_obs_sum=np.zeros(size), dev_rep_sum=np.zeros(size),
                         **{f"{k}_{b}": zi(size) for k in ("score_ge", "score_gt", "rep_score_sum", "rep_score_sumsq", "agree_sum",
                                                           "dev_ge") for b in ("lo", "hi")})
    obs_count = np.stack([(cat == c).sum(axis=0) for c in range(1, Cn + 1)], axis=1).astype(np.int64)
    kacc = {f"{k}_{b}": np.zeros((m, Cn), dtype=np.int64) for k in ("rep_count_sum", "rep_count_sumsq", "count_ge", "count_gt")
            for b in ("lo", "hi")}
    pred_sum = np.zeros((R, n, m))
    reps = np.zeros((S, n, m), dtype=np.int8)
    lp_ld = np.zeros((S, n, m), dtype=LD)
    und_cells = und_cmp = n_cmp = 0
    items = (np.arange(m, dtype=np.uint64) + np.uint64(item0))[None, :]
    rows = np.arange(n, dtype=np.uint64)[:, None]
    for s in range(S):
        g, B = g_draws[s], B_draws[s]
        W = np.zeros((m, Cn + 1))
        if Cn > 2:
            with np.errstate(divide="ignore"):
                W[:, 2:Cn] = np.log1p(-np.exp(-(B[:, 1:] - B[:, :-1])))
        e, up, lo = _fit_terms(g, B)
        pred_sum += e
        for j in range(m):
            lp_ld[s, :, j] = loglik(cat[:, j], g[:, j].astype(LD), B[j], True, LD)
        with np.errstate(invalid="ignore"):
            bad = obs & ~np.isfinite(g)
            live = obs & ~bad
            u = item_uniform(seed, iters[s], int(stage), items, rows)
            below = u[None] < e
            undc = (np.abs(u[None] - e) <= FIT_U_TOL)
            rep = 1 + below.sum(axis=0)
            rep_lo = 1 + (below & ~undc).sum(axis=0)
            rep_hi = 1 + (below | undc).sum(axis=0)
            und = live & undc.any(axis=0)
            Kc = np.where(obs, cat, 1)
            lpc = _fit_logp(Kc, up, lo, W)
            lpr = _fit_logp(rep, up, lo, W)
            changed = live & (rep != cat)
            d_obs = np.where(live, -2.0 * lpc, 0.0)
            d_rep = np.where(live, -2.0 * np.where(rep == cat, lpc, lpr), 0.0)
            delta = np.where(changed, lpc - lpr, 0.0)
            absd = np.where(changed, np.abs(lpc) + np.abs(lpr), 0.0)
        reps[s] = np.where(live, rep, 0)
        und_cells += int(und.sum())
        agree_lo = live & ~und & (rep == cat)
        agree_hi = live & np.where(und, (rep_lo <= cat) & (cat <= rep_hi), rep == cat)
        nf_item = None
        for name, axis, size in units:
            a = acc[name]
            nf = usum(bad, axis) > 0
            if name == "item":
                nf_item = nf
            on = ~nf & (a["n_obs"] > 0)
            a["nonfinite"] += nf
            nu = usum(und, axis)
            R_lo = usum(np.where(live, rep_lo, 0), axis).astype(np.int64)
            R_hi = usum(np.where(live, rep_hi, 0), axis).astype(np.int64)
            T = a["obs_score"]
            a["rep_score_sum_lo"] += np.where(on, R_lo, 0); a["rep_score_sum_hi"] += np.where(on, R_hi, 0)
            a["rep_score_sumsq_lo"] += np.where(on, R_lo * R_lo, 0); a["rep_score_sumsq_hi"] += np.where(on, R_hi * R_hi, 0)
            a["score_ge_lo"] += on & (R_lo >= T); a["score_ge_hi"] += on & (R_hi >= T)
            a["score_gt_lo"] += on & (R_lo > T); a["score_gt_hi"] += on & (R_hi > T)
            a["agree_sum_lo"] += np.where(on, usum(agree_lo, axis), 0); a["agree_sum_hi"] += np.where(on, usum(agree_hi, axis), 0)
            with np.errstate(invalid="ignore"):
                D = usum(delta, axis)
                open_ = (nu > 0) | ((D != 0) & (np.abs(D) <= FIT_D_TOL * usum(absd, axis)))
                ge = D >= 0
            a["dev_ge_lo"] += on & ~open_ & ge; a["dev_ge_hi"] += on & (open_ | ge)
            und_cmp += int((on & open_).sum())
            n_cmp += int(on.sum())
            with np.errstate(invalid="ignore"):
                a["dev_obs_sum"] += np.where(on, usum(d_obs, axis), 0.0)
                a["dev_rep_sum"] += np.where(on, usum(d_rep, axis), 0.0)
        on_item = (~nf_item & (acc["item"]["n_obs"] > 0))[:, None]
        c_lo = np.stack([(live & ~und & (rep == c)).sum(axis=0) for c in range(1, Cn + 1)], axis=1).astype(np.int64)
        c_hi = c_lo + np.stack([(und & (rep_lo <= c) & (c <= rep_hi)).sum(axis=0) for c in range(1, Cn + 1)], axis=1)
        for b, cnt in (("lo", c_lo), ("hi", c_hi)):
            kacc[f"rep_count_sum_{b}"] += np.where(on_item, cnt, 0)
            kacc[f"rep_count_sumsq_{b}"] += np.where(on_item, cnt * cnt, 0)
            kacc[f"count_ge_{b}"] += on_item & (cnt >= obs_count)
            kacc[f"count_gt_{b}"] += on_item & (cnt > obs_count)
    out = {}
    pair = lambda x: (x.copy(), x.copy())       # noqa: E731
    for name, axis, size in units:
        a = acc[name]
        d = dict(n_obs=pair(a["n_obs"]), obs_score=pair(a["obs_score"]), nonfinite=pair(a["nonfinite"]),
                 dev_obs_sum=a["dev_obs_sum"], dev_rep_sum=a["dev_rep_sum"], draws=S)
        for k in ("score_ge", "score_gt", "rep_score_sum", "rep_score_sumsq", "agree_sum", "dev_ge"):
            d[k] = (a[f"{k}_lo"], a[f"{k}_hi"])
        out[name] = d
    out["categories"] = dict(obs_count=pair(obs_count), **{k: (kacc[f"{k}_lo"], kacc[f"{k}_hi"])
                                                           for k in ("rep_count_sum", "rep_count_sumsq", "count_ge", "count_gt")})
    # the WAIC reference in long double: the logaddexp over the draws, the mean and the sum of squared deviations
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mx = lp_ld.max(axis=0)
        safe = np.where(np.isfinite(mx), mx, LD(0))
        lse = np.where(np.isfinite(mx), safe + np.log(np.exp(lp_ld - safe).sum(axis=0)), lp_ld.sum(axis=0))
        mean = lp_ld.sum(axis=0) / LD(S)
        m2 = ((lp_ld - mean) ** 2).sum(axis=0)
        lppd = lse - np.log(LD(S))
        pw = m2 / LD(S - 1) if S >= 2 else np.full((n, m), np.nan, dtype=LD)
        elpd = lppd - pw
        nobs = int(obs.sum())
        tl, tp = lppd[obs].sum(), pw[obs].sum()
        se = np.sqrt(LD(nobs) * (((elpd[obs] - elpd[obs].mean()) ** 2).sum() / LD(nobs - 1))) if nobs >= 2 else LD(np.nan)
    out["waic"] = dict(lse=lse, ll_mean=mean, ll_m2=m2, lppd=lppd, p_waic=pw, observed=obs, ll_absmax=np.abs(lp_ld).max(axis=0),
                       totals=dict(lppd=tl, p_waic=tp, elpd_waic=tl - tp, waic=LD(-2) * (tl - tp), se_elpd_waic=se, n_obs=nobs, draws=S))
    out["pred_sum"] = pred_sum
    out["rep"] = reps
    out["undecided"] = dict(cells=und_cells, comparisons=und_cmp)
    out["comparisons"] = n_cmp
    return out


# --------------------------------------------------------------------------------------- scoring new respondents ----
# (include/gpirt_hip.h "scoring new respondents under ordinal responses", csrc/ordinal_score.hip; library
# version 144) the theta posterior, the predictive density, the category predictions and the next item of respondents who were not
# in the fit.  `score_from_draws` / `predict_from_draws` are the NumPy statement over stored f* and threshold draws,
# `score_combine` / `score_predict_combine` pool chains' state blocks and finish them with gpirt_amd.score's functions.
SCORE_TAG, SCORE_PREDICT_TAG = 0x5243534F, 0x5250534F          # "OSCR", "OSPR"
SCORE_HELD = 1e300        # the finite value a term of -inf is held at (csrc/ordinal.hip ord_loglik_terms_kernel)


def check_cat_new(cat_new, m=None, C=None) -> np.ndarray:
    """cat_new as an (n_new, m) int8 array; ValueError for a size outside 1..16384, another width than m or (with C) a value
    outside 0 .. C."""
    from .score import SCORE_MAX_N
    c = np.asarray(cat_new)
    if c.ndim == 1:
        c = c[None, :]
    if c.ndim != 2:
        raise ValueError("cat_new must be n_new x m")
    if not 1 <= c.shape[0] <= SCORE_MAX_N:
        raise ValueError(f"n_new = {c.shape[0]} is outside 1..{SCORE_MAX_N}")
    if m is not None and c.shape[1] != int(m):
        raise ValueError(f"cat_new has {c.shape[1]} item columns, the sampler has {int(m)}: cat_new must be coded over the "
                         "sampler's items")
    ci = np.asarray(c, dtype=np.int64)
    if C is not None and not np.all((ci >= 0) & (ci <= int(C))):
        raise ValueError(f"cat_new must lie in 0 .. C = {int(C)} (0 = missing)")
    return ci.clip(-128, 127).astype(np.int8)


def score_product(cat_new, fstar, B) -> np.ndarray:
    """T (1001, n_new) of one f* draw (1001, m) and its thresholds B (m x (C - 1) values): per (k, r) the sum over r's observed
    cells of `theta_logpost_exact`'s terms in long double, rounded once.  A term of -inf (f* = +-inf) is held at -1e300, as the
    device's table holds it; NaN only where r answered an item whose cell is NaN."""
    cat = np.asarray(cat_new)
    fs = np.asarray(fstar, dtype=np.float64).astype(LD)
    B = np.asarray(B, dtype=np.float64)
    N, m = fs.shape
    Cn = B.shape[1] + 1
    T = np.zeros((N, cat.shape[0]), dtype=LD)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(m):
            for c in range(1, Cn + 1):
                who = cat[:, j] == c
                if who.any():
                    col = loglik(np.full(N, c), fs[:, j], B[j], False, LD)
                    col = np.where(col == -np.inf, LD(-SCORE_HELD), col)
                    T[:, who] += col[:, None]
    return T.astype(np.float64)


def score_w(cat_new, B) -> np.ndarray:
    """Wc (n_new): per respondent the sum over the observed cells with 1 < c < C of w(b_c - b_{c-1}), in long double, rounded once."""
    cat = np.asarray(cat_new)
    Bl = np.asarray(B, dtype=np.float64).astype(LD)
    Cn = Bl.shape[1] + 1
    out = np.zeros(cat.shape[0], dtype=LD)
    for c in range(2, Cn):
        wc = w(Bl[:, c - 1] - Bl[:, c - 2])
        out += ((cat == c) * wc[None, :]).sum(axis=1)
    return out.astype(np.float64)


def score_accumulate(cat_new, fstar_draws, threshold_draws, return_products=False, with_w=True) -> dict:
    """One chain's accumulators from its f* draws (S, 1001, m) and threshold VALUES (S, m, C - 1): draws, nonfinite, n_obs (int64),
    lpd_acc, ll_sum, post_sum (n_new, 1001) -- the state block's arrays.  with_w=False leaves Wc out of l (what is wrong
    without it)."""
    from . import score as SC
    cat = check_cat_new(cat_new)
    f = np.asarray(fstar_draws, dtype=np.float64)
    Bd = np.asarray(threshold_draws, dtype=np.float64)
    n = cat.shape[0]
    lp0, lse0 = SC.logprior(), SC.logprior_lse()
    acc = dict(draws=np.zeros(n, dtype=np.int64), nonfinite=np.zeros(n, dtype=np.int64),
               n_obs=(cat != 0).sum(axis=1).astype(np.int64), lpd_acc=np.full(n, -np.inf), ll_sum=np.zeros(n),
               post_sum=np.zeros((n, NGRID)))
    if return_products:
        acc.update(products=[], wc=[])
    for fd, B in zip(f, Bd):
        T = score_product(cat, fd, B)
        Wc = score_w(cat, B) if with_w else np.zeros(n)
        if return_products:
            acc["products"].append(T); acc["wc"].append(Wc)
        lp = lp0[:, None] + T
        ok = np.isfinite(lp).all(axis=0)
        acc["nonfinite"] += ~ok
        for r in np.flatnonzero(ok):
            M = lp[:, r].max()
            e = np.exp(lp[:, r] - M)
            Z = e.sum()
            ell = M + np.log(Z) - lse0 + Wc[r]
            acc["post_sum"][r] += e / Z
            acc["lpd_acc"][r] = np.logaddexp(acc["lpd_acc"][r], ell)
            acc["ll_sum"][r] += ell
            acc["draws"][r] += 1
    return acc


def _chain_axis(fstar_draws, threshold_draws):
    f = np.asarray(fstar_draws, dtype=np.float64)
    Bd = np.asarray(threshold_draws, dtype=np.float64)
    if f.ndim == 3:
        f, Bd = f[None], Bd[None]
    if f.ndim != 4 or f.shape[2] != NGRID or Bd.ndim != 4 or Bd.shape[:2] != f.shape[:2] or Bd.shape[2] != f.shape[3]:
        raise ValueError("fstar_draws must be (C, S, 1001, m) or (S, 1001, m), threshold_draws (C, S, m, C - 1) or (S, m, C - 1)")
    return f, Bd


def score_from_draws(cat_new, fstar_draws, threshold_draws, probs=(0.025, 0.5, 0.975), signs=None, return_products=False,
                     with_w=True) -> dict:
    """What the device accumulates and `score_combine` reports, from stored draws: fstar_draws (chains, S, 1001, m) or (S, 1001, m),
    threshold_draws the threshold VALUES of each draw ((chains,) S, m, C - 1).  Each chain accumulated on its own, pooled and
    finished by gpirt_amd.score.pool and .finish (signs[c] = -1 reverses that chain's grid axis of post_sum).  With
    return_products, "products" and "wc": per chain the list of T and Wc per draw."""
    from . import score as SC
    f, Bd = _chain_axis(fstar_draws, threshold_draws)
    cat = check_cat_new(cat_new, f.shape[3], Bd.shape[3] + 1)
    chains = [score_accumulate(cat, fc, bc, return_products, with_w) for fc, bc in zip(f, Bd)]
    out = SC.finish(SC.pool([{k: v for k, v in c.items() if k != "wc"} for c in chains], signs), probs)
    if return_products:
        out["products"] = [c["products"] for c in chains]
        out["wc"] = [c["wc"] for c in chains]
    return out


def category_tables(fstar, B) -> tuple:
    """(P, Hc) of one f* draw in float64 and the kernel's operations: P (C, 1001, m) with P_c = exp(logP_c), logP_c = -up_c [c < C]
    - lo_{c-1} [c > 1] + w_c [1 < c < C] from ONE E_c = exp(-|f* - b_c|) per threshold (`_fit_terms`), and Hc (1001, m) =
    -sum_c P_c logP_c in ascending c, a term with P_c = 0 left out."""
    g = np.asarray(fstar, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    R = B.shape[1]
    Cn = R + 1
    _, up, lo = _fit_terms(g, B)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        P = np.empty((Cn,) + g.shape)
        H = np.zeros(g.shape)
        for c in range(1, Cn + 1):
            lp = np.zeros(g.shape)
            if c < Cn:
                lp = -up[c - 1]
            if c > 1:
                lp = lp - lo[c - 2]
            if 1 < c < Cn:
                lp = lp + np.log1p(-np.exp(-(B[:, c - 1] - B[:, c - 2])))[None, :]
            P[c - 1] = np.exp(lp)
            H = np.where(P[c - 1] > 0.0, H - P[c - 1] * np.where(P[c - 1] > 0.0, lp, 0.0), H)
    return P, H


def category_entropy(q) -> np.ndarray:
    """h(q) = -sum_c q_c log q_c over axis 0, q_c clamped to <= 1, 0 log 0 = 0, ascending c."""
    q = np.asarray(q, dtype=np.float64)
    h = np.zeros(q.shape[1:])
    with np.errstate(divide="ignore", invalid="ignore"):
        for qc in q:
            qq = np.minimum(qc, 1.0)
            h = np.where(qq > 0.0, h - qq * np.log(np.where(qq > 0.0, qq, 1.0)), h)
    return h


def predict_accumulate(cat_new, fstar_draws, threshold_draws, return_draws=False) -> dict:
    """One chain's prediction accumulators: prob_sum (C, n_new, m), info_sum (n_new, m), pred_draws, pred_skipped.  Per counted
    draw the contractions q_c = W^T P_c and Hbar = W^T Hc run in long double and are rounded once; a draw whose f* holds a NaN is
    skipped whole.  With return_draws, "q", "Hbar", "weights", "products" list them per counted draw."""
    from . import score as SC
    cat = check_cat_new(cat_new)
    f = np.asarray(fstar_draws, dtype=np.float64)
    Bd = np.asarray(threshold_draws, dtype=np.float64)
    n, m = cat.shape
    Cn = Bd.shape[2] + 1
    acc = dict(prob_sum=np.zeros((Cn, n, m)), info_sum=np.zeros((n, m)), pred_draws=0, pred_skipped=0)
    if return_draws:
        acc.update(q=[], Hbar=[], weights=[], products=[])
    for fd, B in zip(f, Bd):
        if np.isnan(fd).any():
            acc["pred_skipped"] += 1
            continue
        T = score_product(cat, fd, B)
        wts = SC.draw_weights(None, None, T)
        P, H = category_tables(fd, B)
        wl = wts.astype(LD).T
        q = np.stack([SC._contract(wl, P[c]) for c in range(Cn)])
        hbar = SC._contract(wl, H)
        acc["prob_sum"] += q
        acc["info_sum"] += category_entropy(q) - hbar
        acc["pred_draws"] += 1
        if return_draws:
            acc["q"].append(q); acc["Hbar"].append(hbar); acc["weights"].append(wts); acc["products"].append(T)
    return acc


def predict_result(acc, cat_new, top=5) -> dict:
    """The finished prediction from (pooled) sums: probs (n_new x m x C) = prob_sum / pred_draws, expected (the mean category, from
    probs), info, and (top not None) next_items / next_info by gpirt_amd.score.next_items over the cells with cat_new = 0; NaN
    without a counted draw.  acc: prob_sum (C, n_new, m), info_sum, and pred_draws / pred_skipped or "counts"."""
    from . import score as SC
    prob_sum, info_sum = np.asarray(acc["prob_sum"]), np.asarray(acc["info_sum"])
    draws, skipped = (acc["counts"] if "counts" in acc else (acc["pred_draws"], acc["pred_skipped"]))
    draws, skipped = int(draws), int(skipped)
    with np.errstate(invalid="ignore", divide="ignore"):
        S = float(draws) if draws > 0 else np.nan
        probs = np.moveaxis(prob_sum, 0, 2) / S
        info = info_sum / S
    out = dict(probs=probs, expected=(probs * np.arange(1, probs.shape[2] + 1)[None, None, :]).sum(axis=2), info=info,
               prob_sum=prob_sum, info_sum=info_sum, pred_draws=draws, pred_skipped=skipped)
    if top is not None:
        y = np.where(np.asarray(cat_new) == 0, np.nan, 1.0)
        out["next_items"], out["next_info"] = SC.next_items(info, y, top)
    return out


def predict_from_draws(cat_new, fstar_draws, threshold_draws, top=5, return_draws=False) -> dict:
    """What the device accumulates and `score_predict_combine` reports, from stored draws (shapes as `score_from_draws`): each chain
    accumulated on its own, the sums and counters added in chain order.  With return_draws, per chain the lists "q" (C, n_new, m),
    "Hbar", "weights" and "products"."""
    from . import score as SC
    top = SC.check_top(top)
    f, Bd = _chain_axis(fstar_draws, threshold_draws)
    cat = check_cat_new(cat_new, f.shape[3], Bd.shape[3] + 1)
    chains = [predict_accumulate(cat, fc, bc, return_draws) for fc, bc in zip(f, Bd)]
    pooled = dict(prob_sum=np.array(chains[0]["prob_sum"]), info_sum=np.array(chains[0]["info_sum"]),
                  pred_draws=sum(c["pred_draws"] for c in chains), pred_skipped=sum(c["pred_skipped"] for c in chains))
    for c in chains[1:]:
        pooled["prob_sum"] = pooled["prob_sum"] + c["prob_sum"]
        pooled["info_sum"] = pooled["info_sum"] + c["info_sum"]
    out = predict_result(pooled, cat, top)
    if return_draws:
        for k in ("q", "Hbar", "weights", "products"):
            out[k] = [c[k] for c in chains]
    return out


def score_state_header(state) -> dict:
    """The header of an ordinal score or predict state block (a device tensor, or a host array of int64 words): tag, version,
    n_new, m, categories, N and, for a predict block, pred_draws and pred_skipped."""
    wd = np.asarray(state[:8]).view(np.int64) if isinstance(state, np.ndarray) else _lib.header_words(state)
    out = dict(tag=int(wd[0]), version=int(wd[1]), n_new=int(wd[2]), m=int(wd[3]), categories=int(wd[4]), N=int(wd[5]))
    if out["tag"] == SCORE_PREDICT_TAG:
        out.update(pred_draws=int(wd[6]), pred_skipped=int(wd[7]))
    return out


def score_block_arrays(words) -> dict:
    """The arrays of a score block on the host (int64 words): draws, nonfinite, n_obs, lpd_acc, ll_sum, post_sum."""
    wd = np.ascontiguousarray(words).view(np.int64)
    n = int(wd[2])
    at = 8
    out = {}
    for k in ("draws", "nonfinite", "n_obs"):
        out[k] = wd[at:at + n].copy(); at += n
    for k in ("lpd_acc", "ll_sum"):
        out[k] = wd[at:at + n].view(np.float64).copy(); at += n
    out["post_sum"] = wd[at:at + n * NGRID].view(np.float64).reshape(n, NGRID).copy()
    return out


def predict_block_arrays(words) -> dict:
    """The arrays of a predict block on the host: answered (bool, n_new x m), prob_sum (C, n_new, m), info_sum (n_new, m), pred_draws,
    pred_skipped."""
    wd = np.ascontiguousarray(words).view(np.int64)
    n, m, Cn = int(wd[2]), int(wd[3]), int(wd[4])
    nm = (n * m + 63) // 64
    bits = np.unpackbits(wd[8:8 + nm].view(np.uint8), bitorder="little")[:n * m]
    at = 8 + nm
    ps = wd[at:at + Cn * n * m].view(np.float64).reshape(Cn, m, n).transpose(0, 2, 1).copy(); at += Cn * n * m
    return dict(answered=bits.reshape(m, n).T.astype(bool), prob_sum=ps,
                info_sum=wd[at:at + n * m].view(np.float64).reshape(m, n).T.copy(), pred_draws=int(wd[6]), pred_skipped=int(wd[7]))


def score_predict_combine(handle, states, top=5, return_state=False) -> dict:
    """gpirt_ordinal_score_predict_combine over the predict state blocks `states` (device tensors, or Samplers with
    ordinal_score_enable(predict=True) on): prob_sum, info_sum and the two counters added in chain order; blocks with another
    n_new, m, C or answered-mask are refused.  Nothing is reflected: probs and info take no sign."""
    from . import score as SC
    top = SC.check_top(top)
    tensors, nc, ptrs = _lib.state_ptrs(states, "ordinal_score_predict_state")
    pooled = np.empty(int(tensors[0].numel()), dtype=np.int64)
    check(_lib.load().gpirt_ordinal_score_predict_combine(handle.ptr, nc, ptrs, ct.c_void_p(pooled.ctypes.data), pooled.nbytes))
    arr = predict_block_arrays(pooled)
    out = predict_result(arr, np.where(arr["answered"], 1, 0), top)
    if return_state:
        out["state"] = pooled
    return out


def score_combine(handle, states, signs=None, probs=(0.025, 0.5, 0.975), top=None, return_state=False) -> dict:
    """gpirt_ordinal_score_combine over the score state blocks `states` (device tensors, or Samplers with ordinal_score_enable on,
    all on handle's device), in chain order: the counters, post_sum and ll_sum added, lpd_acc combined by logaddexp, a chain with
    sign -1 entering with post_sum[r][k] <-> post_sum[r][1000 - k] (signs=None: nothing is reflected; lpd takes no sign).  The
    pooled block is finished by gpirt_amd.score.finish: its keys.  top (1..16): `states` are Samplers with predict on, and
    "predict" holds `score_predict_combine` over their prediction blocks."""
    from . import score as SC
    tensors, nc, ptrs = _lib.state_ptrs(states, "ordinal_score_state")
    sg = (ct.c_int * nc)(*[int(x) for x in signs]) if signs is not None else None
    pooled = np.empty(int(tensors[0].numel()), dtype=np.int64)
    check(_lib.load().gpirt_ordinal_score_combine(handle.ptr, nc, ptrs, sg, ct.c_void_p(pooled.ctypes.data), pooled.nbytes))
    out = SC.finish(score_block_arrays(pooled), probs)
    if top is not None:
        out["predict"] = score_predict_combine(handle, states, top)
    if return_state:
        out["state"] = pooled
    return out


def _score_request(score, m, C):
    """ordinal.run's score= as (cat_new, probs, predict, top), or None"""
    from . import score as SC
    if score is None:
        return None
    req = dict(score) if isinstance(score, dict) else dict(data=score)
    unknown = set(req) - {"data", "probs", "predict", "top"}
    if unknown or "data" not in req:
        raise ValueError(f"ordinal.run: score= takes data, probs, predict and top; got {sorted(req)}")
    predict = bool(req.get("predict", False))
    top = SC.check_top(req.get("top", SC.DEFAULT_TOP))
    return check_cat_new(req["data"], m, C), tuple(req.get("probs", SC.DEFAULT_PROBS)), predict, top


# ------------------------------------------------------------------------------------------------ one call per run ---
def run(cat, sample_iterations, burn_iterations, C=None, chains=1, seed=1, width=16, consistent=False, hi=6.0, points=241,
        log_prior=None, K0=None, theta_init=None, preset="fast", probs=(0.025, 0.25, 0.5, 0.75, 0.975), *, handle=None, fit=None,
        score=None, **sampler_kw) -> dict:
    """`chains` chains of the stage-driven Sampler under the ordinal model, one after the other: per iteration step() then
    draw_thresholds(), per kept draw ordinal_record() and ordinal_accumulate_irf().  Chain c runs with the seed
    chain_seed(seed, c) from gpirtMCMC(chains=...)'s default init; K0=None starts at init_thresholds(cat, grid).

    Returns theta (chains x S x n; S x n for one chain), beta (.. x 2 x m; row 0 is the pinned 0), threshold_draws (indices,
    .. x m x (C - 1)), thresholds (`summarise` over all chains: mean, sd, quantiles per item and threshold, on each chain's own
    latent scale -- chains are not sign-aligned), hist (pooled), curves (`curves` of the pooled accumulators), counters (pinned,
    failed, updates per chain), grid, categories, chains, consistent.  fit=True, or a tuple of parts ("waic", "pred", "ppc"):
    ordinal_fit_accumulate() after every kept draw and "fit", `fit_combine` over the chains (without its "state"); the default
    makes the calls and returns the keys it did before.  score=cat_new, or dict(data=cat_new, probs=, predict=, top=): the new
    respondents cat_new (n_new x m, 0 = missing) are scored after every kept draw, after draw_thresholds
    (ordinal_score_accumulate), and "score" holds `score_combine` over the chains -- with "predict" when asked -- and "signs":
    chain c enters with the sign of the dot product of its theta means with chain 0's (the chains are not aligned otherwise).
    The default makes no new call and returns the keys it returned before."""
    from . import chains as CH
    from .ops import Handle
    from .sampler import Sampler, _options
    cat = np.asfortranarray(np.asarray(cat, dtype=np.int8))
    n, m = cat.shape
    S, B, nc = int(sample_iterations), int(burn_iterations), int(chains)
    if nc < 1 or S < 1 or B < 0:
        raise ValueError("ordinal.run: chains >= 1, sample_iterations >= 1 and burn_iterations >= 0 are needed")
    Cn = categories(cat, C)
    fit_bits = fit_parts(fit)
    sreq = _score_request(score, m, Cn)
    y = dichotomise(cat)
    o = _options(sampler_kw.get("rng", "item"), seed, True, True, None, sampler_kw.get("item0", 0), sampler_kw.get("m_total", 0),
                 sampler_kw.get("kernel_fp32", False), 0)
    check_args(cat, y, Cn, hi, points, log_prior, K0, width, options=o)      # the refusals that need no device, first
    t = grid(hi, points)
    k0 = init_thresholds(cat, t, Cn) if K0 is None else np.ascontiguousarray(K0, dtype=np.int32)
    inits = CH.default_inits(n, nc, seed) if theta_init is None else np.asarray(theta_init, dtype=np.float64).reshape(nc, -1)
    if inits.shape != (nc, n):
        raise ValueError("theta_init must have one value per respondent (and chain)")
    own = handle is None
    h = Handle() if own else handle
    samplers = []
    try:
        th = np.empty((nc, S, n))
        be = np.empty((nc, S, 2, m))
        dr = np.empty((nc, S, m, Cn - 1), dtype=np.int32)
        hist, cum, counters = 0, 0, []
        for c in range(nc):
            s = Sampler(h, y, inits[c], seed=seed if c == 0 else _lib.chain_seed(seed, c), preset=preset, **sampler_kw)
            samplers.append(s)
            s.init()
            s.check()
            s.ordinal_enable(cat, Cn, hi, points, log_prior, k0, width, planned_draws=S)
            if fit_bits:
                s.ordinal_fit_enable(fit_bits)
            if sreq:
                s.ordinal_score_enable(sreq[0], predict=sreq[2], top=sreq[3])
            for it in range(S + B):
                s.step(consistent=consistent)
                s.draw_thresholds()
                if it >= B:
                    s.ordinal_record()
                    s.ordinal_accumulate_irf()
                    if fit_bits:
                        s.ordinal_fit_accumulate()
                    if sreq:
                        s.ordinal_score_accumulate()
                    th[c, it - B] = s.get("theta")
                    be[c, it - B] = s.get("beta")
            s.check()
            dr[c] = s.ordinal_get("draws")
            hist = hist + s.ordinal_get("hist").astype(np.int64)
            cum = cum + s.ordinal_get("cum")
            st = s.ordinal_stats()
            counters.append({k: st[k] for k in ("pinned", "failed", "updates")})
        one = nc == 1
        extra = {}
        if fit_bits:
            extra["fit"] = fit_combine(h, samplers, cat)
            del extra["fit"]["state"]
        if sreq:
            means = th.mean(axis=1)
            signs = [1] + [(-1 if float(means[c] @ means[0]) < 0.0 else 1) for c in range(1, nc)]
            extra["score"] = score_combine(h, samplers, signs, probs=sreq[1], top=sreq[3] if sreq[2] else None)
            extra["score"]["signs"] = signs
        return dict(**extra, theta=th[0] if one else th, beta=be[0] if one else be, threshold_draws=dr[0] if one else dr,
                    thresholds=summarise(dr, t, probs), hist=hist, curves=curves(cum, nc * S), counters=counters, grid=t,
                    categories=Cn, chains=nc, consistent=bool(consistent))
    finally:
        for s in samplers:
            s.close()
        if own:
            h.close()


__all__ = ["grid", "default_log_prior", "dichotomise", "init_thresholds", "check_args", "uniforms", "ll", "w", "loglik",
           "category_logprobs", "n_terms", "slice_exact", "theta_logpost_exact", "beta_exact", "window", "candidates",
           "threshold_conditional", "grid_draw", "thresholds_exact", "transition_matrix", "summarise", "curves", "make_graded", "run",
           "fit_parts", "fit_array", "fit_block_header", "fit_block_get", "fit_block_totals", "fit_derive_units",
           "fit_derive_categories", "fit_pred", "fit_result", "fit_combine", "fit_from_draws", "check_cat_new", "score_product", "score_w",
           "score_accumulate", "score_from_draws", "category_tables", "category_entropy", "predict_accumulate", "predict_result",
           "predict_from_draws", "score_state_header", "score_block_arrays", "predict_block_arrays", "score_combine",
           "score_predict_combine"]
