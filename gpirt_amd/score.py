"""Scoring respondents who were not in the fit: the posterior of their theta and the predictive density of their answers
(include/gpirt_hip.h, "scoring new respondents": gpirt_sampler_score_*, gpirt_score_combine, gpirt_mcmc_score;
csrc/score.hip).

For every counted draw of f* (1001 x m, it carries mu*) and every new respondent r the device forms
T[k, r] = sum over observed cells of -log(1 + exp(-+ f*[k, j])) -- the product draw_theta forms for the respondents of the
chain --, normalises lp[k] = log dnorm(theta*_k) + T[k, r] over the grid and accumulates the weights (post_sum), the log
marginal likelihood l (ll_sum) and its running logaddexp (lpd_acc).  `struct` / `result` wrap the C struct, `combine`
pools chains' state blocks (a chain with sign -1 enters with its grid axis reversed), and `from_draws` is the NumPy
statement of the header over stored f* draws, with T summed in extended precision so that it is the more accurate side.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import NGRID, SCORE_MAX_N, check

DEFAULT_PROBS = (0.025, 0.5, 0.975)
LN_SQRT_2PI = 0.918938533204672741780329736406
HELD = 1e300          # the finite value an overflowed term -log(1 + exp(x)) = -inf is held at (csrc/stages.hip)


# ---------------------------------------------------------------------------------------------------- the contract ---
def grid() -> np.ndarray:
    """theta*_k = -5 + 0.01 k"""
    return -5.0 + np.arange(NGRID, dtype=np.float64) * 0.01


def logprior() -> np.ndarray:
    """log dnorm(theta*_k) as draw_theta adds it: -(log sqrt(2 pi) + 0.5 z^2), z = |theta*_k|"""
    z = np.abs(grid())
    return -(LN_SQRT_2PI + 0.5 * z * z)


def logprior_lse() -> float:
    """logsumexp_k(logprior), summed in extended precision and rounded once"""
    lp = logprior().astype(np.longdouble)
    mx = lp.max()
    return float(mx + np.log(np.exp(lp - mx).sum()))


def check_y_new(y_new, m=None) -> np.ndarray:
    """y_new as an (n_new, m) float64 array; ValueError for a value outside {+1, -1, NaN}, a size outside
    1..16384 or another width than m."""
    y = np.asarray(y_new, dtype=np.float64)
    if y.ndim == 1:
        y = y[None, :]
    if y.ndim != 2:
        raise ValueError("y_new must be n_new x m")
    if not 1 <= y.shape[0] <= SCORE_MAX_N:
        raise ValueError(f"n_new = {y.shape[0]} is outside 1..{SCORE_MAX_N}")
    if m is not None and y.shape[1] != int(m):
        raise ValueError(f"y_new has {y.shape[1]} item columns, the prepared data has {int(m)}: y_new must be coded over "
                         "the sampler's items -- the usual cause is that unanimous items were dropped from the data and "
                         "not from y_new")
    if not np.all((y == 1.0) | (y == -1.0) | np.isnan(y)):
        raise ValueError("y_new must be +1, -1 or NaN (a missing response)")
    return y


# ------------------------------------------------------------------------------------------------------ the device ---
def struct(n_new: int, probs=DEFAULT_PROBS):
    """A gpirt_score asking for every output, and the host arrays behind it (kept alive by the caller)."""
    n = int(n_new)
    pr = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    arrays = dict(probs=pr, grid_post=np.empty((n, NGRID)), theta_mean=np.empty(n), theta_sd=np.empty(n),
                  theta_quantiles=np.empty((pr.size, n)), theta_map=np.empty(n), lpd=np.empty(n), loglik_mean=np.empty(n),
                  post_sum=np.empty((n, NGRID)), lpd_acc=np.empty(n), ll_sum=np.empty(n),
                  n_obs=np.empty(n, dtype=np.int64), draws=np.empty(n, dtype=np.int64),
                  nonfinite=np.empty(n, dtype=np.int64))
    r = _lib.Score()
    for k, a in arrays.items():
        setattr(r, k, a.ctypes.data_as(dict(r._fields_)[k]))
    r.nprobs = pr.size
    return r, arrays


def result(r, arrays) -> dict:
    """The "score" dict of gpirtMCMC(score=...), Sampler.score() and combine()."""
    out = dict(arrays)
    out["lpd_total"] = float(r.lpd_total)
    out["se_lpd_total"] = float(r.se_lpd_total)
    out["theta_grid"] = grid()
    return out


def state_header(state) -> dict:
    """The header of a score state block (a device tensor of int64): n_new, m, version, N."""
    w = state[:8].cpu().numpy().view(np.int64)
    return dict(n_new=int(w[0]), m=int(w[1]), version=int(w[2]), N=int(w[3]))


def combine(handle, states, signs=None, probs=DEFAULT_PROBS) -> dict:
    """gpirt_score_combine over the score state blocks `states` (device tensors, or Samplers with score_enable() on, all
    on handle's device): the counters added, post_sum and ll_sum added and lpd_acc combined by logaddexp in chain order, a
    chain with sign -1 entering with post_sum[r][k] <-> post_sum[r][1000 - k] (signs=None: nothing is reflected)."""
    lib = _lib.load()
    tensors = [s.score_state() if hasattr(s, "score_state") else s for s in states]
    r, arrays = struct(state_header(tensors[0])["n_new"], probs)
    nc = len(tensors)
    ptrs = (C.c_void_p * nc)(*[t.data_ptr() for t in tensors])
    sg = (C.c_int * nc)(*[int(x) for x in signs]) if signs is not None else None
    check(lib.gpirt_score_combine(handle.ptr, nc, ptrs, sg, C.byref(r)))
    return result(r, arrays)


# ------------------------------------------------------------------------------------------------------- NumPy -------
def terms(fstar):
    """(G+, G-) = (-log(1 + exp(-f*)), -log(1 + exp(+f*))), the formula as written in fp64; a term that overflows to -inf is
    held at -1e300, NaN stays NaN."""
    f = np.asarray(fstar, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        gp, gm = -np.log(1.0 + np.exp(-f)), -np.log(1.0 + np.exp(f))
    gp[gp == -np.inf] = -HELD
    gm[gm == -np.inf] = -HELD
    return gp, gm


def product(y_new, fstar) -> np.ndarray:
    """T (1001, n_new) of one f* draw (1001, m): per (k, r) the sum of the observed cells' fp64 terms in extended
    precision (numpy.longdouble), rounded once -- NaN only where r answered an item whose cell is NaN."""
    y = np.asarray(y_new, dtype=np.float64)
    gp, gm = (g.astype(np.longdouble) for g in terms(fstar))
    T = np.zeros((gp.shape[0], y.shape[0]))
    for r in range(y.shape[0]):
        plus, minus = np.flatnonzero(y[r] == 1.0), np.flatnonzero(y[r] == -1.0)
        T[:, r] = (gp[:, plus].sum(axis=1) + gm[:, minus].sum(axis=1)).astype(np.float64)
    return T


def accumulate(y_new, fstar_draws, return_products=False) -> dict:
    """One chain's accumulators from its f* draws (S, 1001, m): draws, nonfinite, n_obs (int64), lpd_acc, ll_sum,
    post_sum (n_new, 1001) -- the state block's arrays."""
    y = check_y_new(y_new)
    f = np.asarray(fstar_draws, dtype=np.float64)
    n = y.shape[0]
    lp0, lse0 = logprior(), logprior_lse()
    acc = dict(draws=np.zeros(n, dtype=np.int64), nonfinite=np.zeros(n, dtype=np.int64),
               n_obs=(~np.isnan(y)).sum(axis=1).astype(np.int64), lpd_acc=np.full(n, -np.inf), ll_sum=np.zeros(n),
               post_sum=np.zeros((n, NGRID)))
    if return_products:
        acc["products"] = []
    for fd in f:
        T = product(y, fd)
        if return_products:
            acc["products"].append(T)
        lp = lp0[:, None] + T
        ok = np.isfinite(lp).all(axis=0)
        acc["nonfinite"] += ~ok
        for r in np.flatnonzero(ok):
            M = lp[:, r].max()
            e = np.exp(lp[:, r] - M)
            Z = e.sum()
            ell = M + np.log(Z) - lse0
            acc["post_sum"][r] += e / Z
            acc["lpd_acc"][r] = np.logaddexp(acc["lpd_acc"][r], ell)
            acc["ll_sum"][r] += ell
            acc["draws"][r] += 1
    return acc


def pool(chains, signs=None) -> dict:
    """The header's pooling of several chains' accumulators (dicts as `accumulate` returns), in chain order."""
    sg = [1] * len(chains) if signs is None else [int(x) for x in signs]
    pooled = None
    for a, s_ in zip(chains, sg):
        post = a["post_sum"][:, ::-1] if s_ < 0 else a["post_sum"]
        if pooled is None:
            pooled = {k: np.array(v) for k, v in a.items() if k != "products"}
            pooled["post_sum"] = np.array(post)
            continue
        if not np.array_equal(pooled["n_obs"], a["n_obs"]):
            raise ValueError("the chains were scored on different y_new")
        pooled["draws"] = pooled["draws"] + a["draws"]
        pooled["nonfinite"] = pooled["nonfinite"] + a["nonfinite"]
        pooled["post_sum"] = pooled["post_sum"] + post
        pooled["ll_sum"] = pooled["ll_sum"] + a["ll_sum"]
        pooled["lpd_acc"] = np.logaddexp(pooled["lpd_acc"], a["lpd_acc"])
    return pooled


def finish(acc, probs=DEFAULT_PROBS) -> dict:
    """The header's finished values from (pooled) accumulators; NaN where draws[r] = 0."""
    pr = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    n = acc["draws"].size
    th = grid()
    with np.errstate(invalid="ignore", divide="ignore"):
        S = np.where(acc["draws"] > 0, acc["draws"], np.nan).astype(np.float64)
        g = acc["post_sum"] / S[:, None]
        mean = (th[None, :] * g).sum(axis=1)
        sd = np.sqrt((((th[None, :] - mean[:, None]) ** 2) * g).sum(axis=1))
        cum = np.cumsum(g, axis=1)
        q = np.empty((pr.size, n))
        for p, v in enumerate(pr):
            q[p] = th[np.minimum((cum < v).sum(axis=1), NGRID - 1)]
        amap = th[np.argmax(np.where(np.isnan(g), -1.0, g), axis=1)]
        lpd = acc["lpd_acc"] - np.log(S)
        ll = acc["ll_sum"] / S
    none = acc["draws"] == 0
    q[:, none] = np.nan
    amap = np.where(none, np.nan, amap)
    out = dict(probs=pr, grid_post=g, theta_mean=mean, theta_sd=sd, theta_quantiles=q, theta_map=amap, lpd=lpd,
               loglik_mean=ll, post_sum=acc["post_sum"], lpd_acc=acc["lpd_acc"], ll_sum=acc["ll_sum"], n_obs=acc["n_obs"],
               draws=acc["draws"], nonfinite=acc["nonfinite"], theta_grid=th)
    out["lpd_total"] = float(lpd.sum())
    out["se_lpd_total"] = float(np.sqrt(n * lpd.var(ddof=1))) if n >= 2 else float("nan")
    return out


def from_draws(y_new, fstar_draws, probs=DEFAULT_PROBS, signs=None, return_products=False) -> dict:
    """What the device accumulates and gpirt_score_combine reports, from stored draws fstar_draws (C, S, 1001, m) (or
    (S, 1001, m): one chain): each chain accumulated on its own, pooled by the header's rules (signs[c] = -1 reverses
    that chain's grid axis of post_sum).  Returns result()'s keys (and, with return_products, "products": per chain the
    list of T per draw)."""
    f = np.asarray(fstar_draws, dtype=np.float64)
    if f.ndim == 3:
        f = f[None]
    if f.ndim != 4 or f.shape[2] != NGRID:
        raise ValueError("fstar_draws must be (C, S, 1001, m) or (S, 1001, m)")
    y = check_y_new(y_new, f.shape[3])
    chains = [accumulate(y, fc, return_products) for fc in f]
    out = finish(pool(chains, signs), probs)
    if return_products:
        out["products"] = [c["products"] for c in chains]
    return out
