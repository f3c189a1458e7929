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
from ._lib import NGRID, ST_ORD, check

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


# ------------------------------------------------------------------------------------------------ one call per run ---
def run(cat, sample_iterations, burn_iterations, C=None, chains=1, seed=1, width=16, consistent=False, hi=6.0, points=241,
        log_prior=None, K0=None, theta_init=None, preset="fast", probs=(0.025, 0.25, 0.5, 0.75, 0.975), *, handle=None,
        **sampler_kw) -> dict:
    """`chains` chains of the stage-driven Sampler under the ordinal model, one after the other: per iteration step() then
    draw_thresholds(), per kept draw ordinal_record() and ordinal_accumulate_irf().  Chain c runs with the seed
    chain_seed(seed, c) from gpirtMCMC(chains=...)'s default init; K0=None starts at init_thresholds(cat, grid).

    Returns theta (chains x S x n; S x n for one chain), beta (.. x 2 x m; row 0 is the pinned 0), threshold_draws (indices,
    .. x m x (C - 1)), thresholds (`summarise` over all chains: mean, sd, quantiles per item and threshold, on each chain's own
    latent scale -- chains are not sign-aligned), hist (pooled), curves (`curves` of the pooled accumulators), counters (pinned,
    failed, updates per chain), grid, categories, chains, consistent."""
    from . import chains as CH
    from .ops import Handle
    from .sampler import Sampler, _options
    cat = np.asfortranarray(np.asarray(cat, dtype=np.int8))
    n, m = cat.shape
    S, B, nc = int(sample_iterations), int(burn_iterations), int(chains)
    if nc < 1 or S < 1 or B < 0:
        raise ValueError("ordinal.run: chains >= 1, sample_iterations >= 1 and burn_iterations >= 0 are needed")
    Cn = categories(cat, C)
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
            for it in range(S + B):
                s.step(consistent=consistent)
                s.draw_thresholds()
                if it >= B:
                    s.ordinal_record()
                    s.ordinal_accumulate_irf()
                    th[c, it - B] = s.get("theta")
                    be[c, it - B] = s.get("beta")
            s.check()
            dr[c] = s.ordinal_get("draws")
            hist = hist + s.ordinal_get("hist").astype(np.int64)
            cum = cum + s.ordinal_get("cum")
            st = s.ordinal_stats()
            counters.append({k: st[k] for k in ("pinned", "failed", "updates")})
        one = nc == 1
        return dict(theta=th[0] if one else th, beta=be[0] if one else be, threshold_draws=dr[0] if one else dr,
                    thresholds=summarise(dr, t, probs), hist=hist, curves=curves(cum, nc * S), counters=counters, grid=t,
                    categories=Cn, chains=nc, consistent=bool(consistent))
    finally:
        for s in samplers:
            s.close()
        if own:
            h.close()


__all__ = ["grid", "default_log_prior", "dichotomise", "init_thresholds", "check_args", "uniforms", "ll", "w", "loglik",
           "category_logprobs", "n_terms", "slice_exact", "theta_logpost_exact", "beta_exact", "window", "candidates",
           "threshold_conditional", "grid_draw", "thresholds_exact", "transition_matrix", "summarise", "curves", "make_graded", "run"]
