"""Exact reference of the summary, chain and quantile outputs, written from the formulas of include/gpirt_hip.h
(GPIRT_SUM_* moments and WAIC, GPIRT_SUM_DIAG, gpirt_chains_combine, GPIRT_SUM_THETA_HIST / GPIRT_SUM_IRF_BAND,
gpirt_quantiles) and nothing else.

Every double is an exact rational, so the moments, the split halves, the batch means and the BDA3 / batch-means formulas
are evaluated in exact arithmetic (Python integers over a common power of two, fractions.Fraction); logs, exps, square
roots and Phi^-1 are evaluated in mpmath at PREC bits.  Each result is rounded to fp64 once, at the end.  Where the header
leaves a case open, the formula as written is followed with IEEE rules (x / 0 = +-inf, 0 / 0 = NaN), and q T is the
fp64 product of the probability and the draw count."""
from __future__ import annotations

import math
from bisect import bisect_right
from fractions import Fraction as Fr

import mpmath
import numpy as np

PREC = 160
NGRID = 1001
BINS = 256
NAN = float("nan")
INF = float("inf")


# ------------------------------------------------------------------------------------------------- exact numbers ---
def _ints(xs):
    """finite doubles -> (integers v, e) with x = v / 2**e exactly"""
    rat = [float(x).as_integer_ratio() for x in xs]
    e = max(d.bit_length() - 1 for _, d in rat)
    return [p << (e - (d.bit_length() - 1)) for p, d in rat], e


def _f(x) -> float:
    """an exact Fraction or an mpf -> the nearest fp64"""
    if isinstance(x, Fr):
        return float(x)                                         # correctly rounded
    if not mpmath.isfinite(x):
        return NAN if mpmath.isnan(x) else (INF if x > 0 else -INF)
    return mpmath.libmp.to_float(mpmath.mpf(x)._mpf_, False, mpmath.libmp.round_nearest)      # float(mpf) truncates


def _mp(x: Fr):
    with mpmath.workprec(PREC):
        return mpmath.mpf(x.numerator) / x.denominator


def _sqrt(x: Fr) -> float:
    with mpmath.workprec(PREC):
        return _f(mpmath.sqrt(_mp(x)))


def _div(num: Fr, den: Fr) -> float:
    """num / den under IEEE rules for den = 0"""
    if den != 0:
        return float(num / den)
    return NAN if num == 0 else math.copysign(INF, num)


# ---------------------------------------------------------------------------------------------------- moments -------
def mean_var(xs):
    """exact (mean, variance with ddof 1; None with fewer than two values) of finite doubles, as Fractions"""
    S = len(xs)
    v, e = _ints(xs)
    s1, s2 = sum(v), sum(t * t for t in v)
    mean = Fr(s1, S << e)
    var = Fr(S * s2 - s1 * s1, (S * (S - 1)) << (2 * e)) if S >= 2 else None
    return mean, var


def moments(draws):
    """draws (S, ...) -> fp64 (mean, var) arrays of the exact values (var NaN with S < 2)"""
    x = np.asarray(draws, dtype=np.float64)
    flat = x.reshape(x.shape[0], -1)
    mean, var = np.empty(flat.shape[1]), np.empty(flat.shape[1])
    for j in range(flat.shape[1]):
        m, v = mean_var(flat[:, j].tolist())
        mean[j], var[j] = float(m), (NAN if v is None else float(v))
    return mean.reshape(x.shape[1:]), var.reshape(x.shape[1:])


# ------------------------------------------------------------------------------------------------------- WAIC --------
def _plogis(g):
    return 1 / (1 + mpmath.exp(-g))


def waic_cell(y, gs):
    """One cell over its draws g_s = f_s + mu_s: ll = -log1p(exp(-y g)), lppd = log mean exp(ll), p_waic = var(ll)
    (ddof 1), p_yes = mean plogis(g).  y NaN (missing): lppd and p_waic NaN.  Returns mpf values (p_waic None, S < 2)."""
    S = len(gs)
    with mpmath.workprec(PREC):
        g = [mpmath.mpf(float(x)) for x in gs]
        p_yes = mpmath.fsum(_plogis(x) for x in g) / S
        if y != y:
            return dict(p_yes=p_yes, lppd=None, p_waic=None, missing=True)
        ll = [-mpmath.log1p(mpmath.exp(-float(y) * x)) for x in g]
        lppd = mpmath.log(mpmath.fsum(mpmath.exp(v) for v in ll) / S)
        mu = mpmath.fsum(ll) / S
        pw = mpmath.fsum((v - mu) ** 2 for v in ll) / (S - 1) if S >= 2 else None
    return dict(p_yes=p_yes, lppd=lppd, p_waic=pw, missing=False)


def waic(y, g):
    """y (n, m) with NaN where missing, g (S, n, m): fp64 arrays p_yes, lppd, p_waic and the totals of
    GPIRT_SUM_T_* over the observed cells (mpf values rounded once)."""
    y = np.asarray(y, dtype=np.float64)
    S = g.shape[0]
    out = {k: np.full(y.shape, NAN) for k in ("p_yes", "lppd", "p_waic")}
    el = []
    with mpmath.workprec(PREC):
        lp_sum, pw_sum = mpmath.mpf(0), mpmath.mpf(0)
        for i, j in np.ndindex(*y.shape):
            c = waic_cell(y[i, j], g[:, i, j].tolist())
            out["p_yes"][i, j] = _f(c["p_yes"])
            if c["missing"]:
                continue
            out["lppd"][i, j] = _f(c["lppd"])
            pw = c["p_waic"] if c["p_waic"] is not None else mpmath.nan
            out["p_waic"][i, j] = _f(pw)
            lp_sum += c["lppd"]
            pw_sum += pw
            el.append(c["lppd"] - pw)
        nobs = len(el)
        em = mpmath.fsum(el) / nobs
        ss = mpmath.fsum((e - em) ** 2 for e in el)
        tot = dict(lppd=lp_sum, p_waic=pw_sum, elpd_waic=lp_sum - pw_sum, waic=-2 * (lp_sum - pw_sum),
                   se_elpd_waic=mpmath.sqrt(nobs * ss / (nobs - 1)), n_obs=mpmath.mpf(nobs), draws=mpmath.mpf(S),
                   elpd_mean=em, elpd_ss=ss)
        out["totals"] = {k: _f(v) for k, v in tot.items()}
    return out


# ------------------------------------------------------------------------------------------------------- DIAG --------
def _batch(S):
    b = math.isqrt(S)
    return b, S // b


def diag_value(chains, signs=None):
    """chains: C sequences of S finite doubles (one value of every chain, draw order).  The GPIRT_SUM_DIAG formulas:
    split-R-hat (BDA3) over the 2C halves (draws 1..N and S-N+1..S, N = floor(S/2)), the batch-means ESS and the MCSE of
    the pooled mean.  signs: C values of +-1 multiplying each chain first (the reflection).  Returns fp64 (rhat, ess,
    mcse)."""
    C = len(chains)
    sg = [1] * C if signs is None else [int(s) for s in signs]
    S = len(chains[0])
    allv, e = _ints([x for ch in chains for x in ch])
    xs = [[sg[c] * allv[c * S + d] for d in range(S)] for c in range(C)]      # integers over 2**e
    N = S // 2
    if S < 4:
        rhat = NAN
    else:
        hm, hv = [], []
        for ch in xs:
            for h in (ch[:N], ch[S - N:]):
                s1, s2 = sum(h), sum(t * t for t in h)
                hm.append(Fr(s1, N))
                hv.append(Fr(N * s2 - s1 * s1, N * (N - 1)))
        M = 2 * C
        xbar = sum(hm) / M
        B = Fr(N, M - 1) * sum((m - xbar) ** 2 for m in hm)
        W = sum(hv) / M
        if W > 0:
            rhat = _sqrt(((N - 1) * W / N + B / N) / W)
        else:
            rhat = INF if B > 0 else NAN
    b, a = _batch(S)
    if a < 2 or S < 2:
        return rhat, NAN, NAN
    lam, sig = Fr(0), Fr(0)
    for ch in xs:
        s1, s2 = sum(ch), sum(t * t for t in ch)
        lam += Fr(S * s2 - s1 * s1, S * (S - 1))
        bs = [sum(ch[k * b:(k + 1) * b]) for k in range(a)]                   # batch sums: means bs / b
        t1, t2 = sum(bs), sum(t * t for t in bs)
        sig += Fr(b, a - 1) * Fr(a * t2 - t1 * t1, a * b * b)                   # b / (a-1) sum_k (Ybar_k - Ybar)^2
    scale = Fr(1, 1 << (2 * e))
    lam, sig = lam * scale, sig * scale
    CS = C * S
    ess = _div(CS * lam / C, sig / C)
    mcse = _sqrt(sig / C / CS)
    return rhat, ess, mcse


def diag(draws, signs=None, reflect=None):
    """draws (C, S, ...): per value (rhat, ess, mcse) arrays.  reflect: boolean mask over the value axes of the values a
    reflection negates (default: all, when signs are given)."""
    x = np.asarray(draws, dtype=np.float64)
    C, S = x.shape[:2]
    rest = x.shape[2:]
    flat = x.reshape(C, S, -1)
    rm = np.ones(flat.shape[2], dtype=bool) if reflect is None else np.asarray(reflect).reshape(-1)
    out = np.empty((3, flat.shape[2]))
    for j in range(flat.shape[2]):
        sg = signs if (signs is not None and rm[j]) else None
        out[:, j] = diag_value([flat[c, :, j].tolist() for c in range(C)], sg)
    return tuple(o.reshape(rest) for o in out)


def pooled_moments(draws, signs=None, reflect=None):
    """draws (C, S, ...): the exact mean and variance (ddof 1) over all C S draws, reflected chains negated"""
    x = np.asarray(draws, dtype=np.float64)
    C, S = x.shape[:2]
    if signs is not None:
        sg = np.asarray(signs, dtype=np.float64).reshape((C, 1) + (1,) * (x.ndim - 2))
        rm = np.ones(x.shape[2:], dtype=bool) if reflect is None else np.asarray(reflect)
        x = np.where(rm[None, None], x * sg, x)
    return moments(x.reshape((C * S,) + x.shape[2:]))


def block_scalars(rhat, ess):
    """the per-block scalars: NaN left out of max / min and counted; R-hat > 1.01 counted, +inf included"""
    r = [float(v) for v in np.ravel(rhat)]
    e = [float(v) for v in np.ravel(ess)]
    rr, ee = [v for v in r if v == v], [v for v in e if v == v]
    return dict(max_rhat=max(rr) if rr else NAN, min_ess=min(ee) if ee else NAN,
                n_rhat_high=float(sum(v > 1.01 for v in rr)), n_rhat_nan=float(len(r) - len(rr)),
                n_ess_nan=float(len(e) - len(ee)))


# --------------------------------------------------------------------------------------------- theta quantiles -------
def grid_k(t: float) -> int:
    """the grid index k of a theta draw that is bit for bit -5 + 0.01 k (fp64 arithmetic, k = 0..1000), else -1"""
    v = (t + 5.0) * 100.0
    if not math.isfinite(v):
        return -1
    k = round(v)                                                # half to even, as rint
    return k if 0 <= k <= NGRID - 1 and -5.0 + k * 0.01 == t else -1


def order_rank(q: float, T: int) -> int:
    """max(ceil(q T), 1) with q T the fp64 product"""
    return max(math.ceil(float(q) * T), 1)


def _phi_inv(p):
    return mpmath.sqrt(2) * mpmath.erfinv(2 * p - 1)


def _bda3(groups):
    """BDA3 split-R-hat on M groups of N exact values each (mpf), with the W = 0 rules"""
    M, N = len(groups), len(groups[0])
    means = [mpmath.fsum(g) / N for g in groups]
    vars_ = [mpmath.fsum((v - m) ** 2 for v in g) / (N - 1) for g, m in zip(groups, means)]
    xbar = mpmath.fsum(means) / M
    B = mpmath.mpf(N) / (M - 1) * mpmath.fsum((m - xbar) ** 2 for m in means)
    W = mpmath.fsum(vars_) / M
    if W > 0:
        return _f(mpmath.sqrt(((N - 1) * W / N + B / N) / W))
    return INF if B > 0 else NAN


def rank_rhat(halves):
    """halves: 2C lists of N exact values (integers or Fractions), ranked together with ties averaged,
    z = Phi^-1((r - 3/8) / (T' + 1/4)), BDA3 on z.  NaN for N < 2."""
    N = len(halves[0])
    if N < 2:
        return NAN
    allv = sorted(v for h in halves for v in h)
    Tp = len(allv)
    with mpmath.workprec(PREC):
        z = {}
        i = 0
        while i < Tp:
            j = i
            while j < Tp and allv[j] == allv[i]:
                j += 1
            r = Fr(i + 1 + j, 2)                                  # ranks i+1..j averaged
            z[allv[i]] = _phi_inv(_mp((r - Fr(3, 8)) / (Tp + Fr(1, 4))))
            i = j
        return _bda3([[z[v] for v in h] for h in halves])


def theta_quantities(theta_draws, probs, signs=None):
    """theta_draws (C, S, n) as the sampler writes them.  The pooled T = C S draws (a reflected chain's grid index
    k -> 1000 - k): hist (1001, n), off (n, off-grid draws), q (nprobs, n), median, mode, bulk, tail, rhat (n); NaN for
    every quantity of a respondent with a draw off the grid."""
    th = np.asarray(theta_draws, dtype=np.float64)
    C, S, n = th.shape
    sg = [1] * C if signs is None else [int(s) for s in signs]
    T = C * S
    N = S // 2
    out = dict(hist=np.zeros((NGRID, n)), off=np.zeros(n), q=np.full((len(probs), n), NAN))
    for k in ("median", "mode", "bulk", "tail", "rhat"):
        out[k] = np.full(n, NAN)
    for i in range(n):
        ks = [[grid_k(float(th[c, d, i])) for d in range(S)] for c in range(C)]
        ks = [[(NGRID - 1 - k if sg[c] < 0 and k >= 0 else k) for k in ks[c]] for c in range(C)]
        flat = [k for ch in ks for k in ch]
        for k in flat:
            if k >= 0:
                out["hist"][k, i] += 1
        off = sum(k < 0 for k in flat)
        out["off"][i] = off
        if off:
            continue
        srt = sorted(flat)
        for p, q in enumerate(probs):
            out["q"][p, i] = -5.0 + srt[order_rank(q, T) - 1] * 0.01
        out["median"][i] = -5.0 + srt[order_rank(0.5, T) - 1] * 0.01
        cnt = np.bincount(flat, minlength=NGRID)
        out["mode"][i] = -5.0 + int(np.argmax(cnt)) * 0.01                    # argmax: the lowest on a tie
        s2 = srt[(T + 1) // 2 - 1] + srt[T // 2]                              # R's median, doubled (half-grid units)
        halves = [h for ch in ks for h in (ch[:N], ch[S - N:])]
        bulk = rank_rhat(halves)
        tail = rank_rhat([[abs(2 * k - s2) for k in h] for h in halves])
        out["bulk"][i], out["tail"][i] = bulk, tail
        out["rhat"][i] = NAN if (bulk != bulk or tail != tail) else max(bulk, tail)
    return out


# ------------------------------------------------------------------------------------------------------ IRF band ------
def band_bin(x: float, edges) -> int:
    """the exported-edge rule: #{b : e_b <= x} (-1 for NaN)"""
    return -1 if x != x else bisect_right(edges, x)


def plogis_exact(x: float):
    """plogis(x) as an mpf (x = +-inf: 1 / 0)"""
    if x == INF:
        return mpmath.mpf(1)
    if x == -INF:
        return mpmath.mpf(0)
    with mpmath.workprec(PREC):
        return _plogis(mpmath.mpf(float(x)))


def exact_bin(x: float) -> int:
    """#{b = 1..255 : b / 256 <= plogis(x)} (x = 0: plogis exactly 1/2)"""
    if x == 0:
        return BINS // 2
    with mpmath.workprec(PREC):
        return min(BINS - 1, int(mpmath.floor(BINS * plogis_exact(x))))


def irf_quantities(fstar_draws, probs, signs=None):
    """fstar_draws (C, S, 1001, m): a reflected chain's grid axis reversed, then per pooled cell the NaN count, the mean of
    plogis (NaN with a NaN draw) and the exact order statistics of plogis(f*) (NaN with a NaN draw)."""
    f = np.asarray(fstar_draws, dtype=np.float64)
    C, S = f.shape[:2]
    sg = [1] * C if signs is None else [int(s) for s in signs]
    f = np.stack([f[c][:, ::-1] if sg[c] < 0 else f[c] for c in range(C)])
    T = C * S
    cells = f.shape[2:]
    flat = f.reshape(T, -1)
    nanc = np.isnan(flat).sum(axis=0)
    pm = np.full(flat.shape[1], NAN)
    qs = np.full((len(probs), flat.shape[1]), NAN)
    ranks = [order_rank(q, T) for q in probs]
    with mpmath.workprec(PREC):
        for c in range(flat.shape[1]):
            if nanc[c]:
                continue
            ps = sorted(plogis_exact(float(x)) for x in flat[:, c])
            pm[c] = _f(mpmath.fsum(ps) / T)
            for p, r in enumerate(ranks):
                qs[p, c] = _f(ps[r - 1])
    return dict(nan=nanc.reshape(cells), p_mean=pm.reshape(cells), q=qs.reshape((len(probs),) + cells))
