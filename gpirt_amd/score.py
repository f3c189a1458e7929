"""Scoring respondents who were not in the fit: the posterior of their theta and the predictive density of their answers
(include/gpirt_hip.h, "scoring new respondents": gpirt_sampler_score_*, gpirt_score_combine, gpirt_run.score;
csrc/score.hip).

For every counted draw of f* (1001 x m, it carries mu*) and every new respondent r the device forms
T[k, r] = sum over observed cells of -log(1 + exp(-+ f*[k, j])) -- the product draw_theta forms for the respondents of the
chain --, normalises lp[k] = log dnorm(theta*_k) + T[k, r] over the grid and accumulates the weights (post_sum), the log
marginal likelihood l (ll_sum) and its running logaddexp (lpd_acc).  `struct` / `result` wrap the C struct, `combine`
pools chains' state blocks (a chain with sign -1 enters with its grid axis reversed), and `from_draws` is the NumPy
statement of the header over stored f* draws, with T summed in extended precision so that it is the more accurate side.

Predicting the UNSEEN answers (include/gpirt_hip.h, "predicting new respondents' unseen answers"; csrc/predict.hip) is an
add-on to the same state: per draw q[r, j] = sum_k w_k plogis(f*[k, j]) and the mutual information g[r, j] between the
unseen answer and theta_r, accumulated into pred_sum and info_sum.  `predict_struct` / `predict_result` wrap
gpirt_score_predict, `predict_combine` pools chains' predict state blocks, and `predict_from_draws` is the NumPy statement:
the weights `accumulate` forms, the two contractions over the grid in extended precision.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import NGRID, PREDICT_MAX_TOP, SCORE_MAX_N, check

DEFAULT_PROBS = (0.025, 0.5, 0.975)
DEFAULT_TOP = 5
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
    w = _lib.header_words(state)
    return dict(n_new=int(w[0]), m=int(w[1]), version=int(w[2]), N=int(w[3]))


def combine(handle, states, signs=None, probs=DEFAULT_PROBS) -> dict:
    """gpirt_score_combine over the score state blocks `states` (device tensors, or Samplers with score_enable() on, all
    on handle's device): the counters added, post_sum and ll_sum added and lpd_acc combined by logaddexp in chain order, a
    chain with sign -1 entering with post_sum[r][k] <-> post_sum[r][1000 - k] (signs=None: nothing is reflected)."""
    lib = _lib.load()
    tensors, nc, ptrs = _lib.state_ptrs(states, "score_state")
    r, arrays = struct(state_header(tensors[0])["n_new"], probs)
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


# ------------------------------------------------------------------------- predicting the unseen answers: the device ---
def check_top(top) -> int:
    """top as an int in 1..16, ValueError otherwise"""
    t = int(top)
    if t != top or not 1 <= t <= PREDICT_MAX_TOP:
        raise ValueError(f"top = {top!r} is outside 1..{PREDICT_MAX_TOP}")
    return t


def predict_struct(n_new: int, m: int, top=DEFAULT_TOP):
    """A gpirt_score_predict asking for every output, and the host arrays behind it (column-major, as y_new is)."""
    n, m, top = int(n_new), int(m), check_top(top)
    arrays = dict(p_yes=np.empty((n, m), order="F"), info=np.empty((n, m), order="F"),
                  next_items=np.empty((n, top), dtype=np.int64, order="F"), next_info=np.empty((n, top), order="F"),
                  pred_sum=np.empty((n, m), order="F"), info_sum=np.empty((n, m), order="F"))
    r = _lib.ScorePredict()
    for k, a in arrays.items():
        setattr(r, k, a.ctypes.data_as(dict(r._fields_)[k]))
    r.top = top
    return r, arrays


def predict_result(r, arrays) -> dict:
    """The "predict" dict of gpirtMCMC(score=dict(..., predict=True)), Sampler.score_predict() and predict_combine()."""
    out = dict(arrays)
    out["pred_draws"] = int(r.pred_draws)
    out["pred_skipped"] = int(r.pred_skipped)
    return out


def predict_state_header(state) -> dict:
    """The header of a predict state block (a device tensor of int64): n_new, m, version, N, pred_draws, pred_skipped."""
    w = _lib.header_words(state)
    return dict(n_new=int(w[0]), m=int(w[1]), version=int(w[2]), N=int(w[3]), pred_draws=int(w[4]), pred_skipped=int(w[5]))


def predict_combine(handle, states, top=DEFAULT_TOP) -> dict:
    """gpirt_score_predict_combine over the predict state blocks `states` (device tensors, or Samplers with
    score_predict_enable() on, all on handle's device): pred_sum, info_sum and the two counters added in chain order;
    blocks with another n_new, m or answered-mask are refused.  Nothing is reflected: both sums run over the whole grid."""
    lib = _lib.load()
    top = check_top(top)
    tensors, nc, ptrs = _lib.state_ptrs(states, "score_predict_state")
    hdr = predict_state_header(tensors[0])
    r, arrays = predict_struct(hdr["n_new"], hdr["m"], top)
    check(lib.gpirt_score_predict_combine(handle.ptr, nc, ptrs, C.byref(r)))
    return predict_result(r, arrays)


# -------------------------------------------------------------------------- predicting the unseen answers: NumPy -------
def plogis_entropy(fstar):
    """(P, H) of the header, the formulas as written in fp64: plogis(f*) and its binary entropy in nats (exactly 0 once
    exp(-|f*|) underflows)."""
    f = np.asarray(fstar, dtype=np.float64)
    a = np.abs(f)
    e = np.exp(-a)
    l, s_ = np.log1p(e), e / (1.0 + e)
    with np.errstate(invalid="ignore"):
        P = np.where(f >= 0.0, 1.0 / (1.0 + e), s_)
        H = np.where(e == 0.0, 0.0, l + np.where(e == 0.0, 0.0, a) * s_)
    return P, H


def binary_entropy(q):
    """h(q) = -(q log q + (1 - q) log1p(-q)), q clamped to [0, 1], 0 log 0 = 0"""
    q = np.clip(np.asarray(q, dtype=np.float64), 0.0, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(q > 0.0, q * np.log(np.where(q > 0.0, q, 1.0)), 0.0)
        b = np.where(q < 1.0, (1.0 - q) * np.log1p(-np.where(q < 1.0, q, 0.0)), 0.0)
    return -(a + b)


def draw_weights(y_new, fstar, T=None) -> np.ndarray:
    """w (1001, n_new) of one NaN-free f* draw: the weights `accumulate` forms, from the long-double `product`"""
    if T is None:
        T = product(y_new, fstar)
    lp = logprior()[:, None] + T
    e = np.exp(lp - lp.max(axis=0)[None, :])
    return e / e.sum(axis=0)[None, :]


def next_items(info, y_new, top=DEFAULT_TOP):
    """(next_items, next_info), both (n_new, top): each respondent's UNANSWERED items by decreasing info, ties to the lowest
    j, an item whose info is NaN never listed; padded with -1 / NaN."""
    top = check_top(top)
    info = np.asarray(info, dtype=np.float64)
    y = np.asarray(y_new, dtype=np.float64)
    n = y.shape[0]
    items = np.full((n, top), -1, dtype=np.int64)
    vals = np.full((n, top), np.nan)
    for r in range(n):
        cand = np.flatnonzero(np.isnan(y[r]) & ~np.isnan(info[r]))
        order = cand[np.argsort(-info[r, cand], kind="stable")][:top]
        items[r, :order.size] = order
        vals[r, :order.size] = info[r, order]
    return items, vals


def _contract(wl, X):
    """wl @ X in numpy.longdouble (no BLAS there: the columns are shared among a few threads; the same bits either way)"""
    X = X.astype(np.longdouble)
    if wl.shape[0] * X.size < 1 << 24:
        return (wl @ X).astype(np.float64)
    from concurrent.futures import ThreadPoolExecutor
    cols = np.array_split(np.arange(X.shape[1]), 16)
    with ThreadPoolExecutor(8) as ex:
        parts = list(ex.map(lambda c: wl @ X[:, c], cols))
    return np.concatenate(parts, axis=1).astype(np.float64)


def predict_accumulate(y_new, fstar_draws, return_draws=False) -> dict:
    """One chain's prediction accumulators from its f* draws (S, 1001, m): pred_sum, info_sum (n_new, m), pred_draws,
    pred_skipped.  Per counted draw the contractions q = W^T P and Hbar = W^T H run in numpy.longdouble and are rounded
    once; with return_draws, "q", "Hbar", "weights" and "products" list them per counted draw."""
    y = check_y_new(y_new)
    f = np.asarray(fstar_draws, dtype=np.float64)
    n, m = y.shape
    acc = dict(pred_sum=np.zeros((n, m)), info_sum=np.zeros((n, m)), pred_draws=0, pred_skipped=0)
    if return_draws:
        acc.update(q=[], Hbar=[], weights=[], products=[])
    for fd in f:
        if np.isnan(fd).any():
            acc["pred_skipped"] += 1
            continue
        T = product(y, fd)
        w = draw_weights(y, fd, T)
        P, H = plogis_entropy(fd)
        wl = w.astype(np.longdouble).T
        q, hbar = _contract(wl, P), _contract(wl, H)
        acc["pred_sum"] += q
        acc["info_sum"] += binary_entropy(q) - hbar
        acc["pred_draws"] += 1
        if return_draws:
            acc["q"].append(q); acc["Hbar"].append(hbar); acc["weights"].append(w); acc["products"].append(T)
    return acc


def predict_from_draws(y_new, fstar_draws, top=DEFAULT_TOP, return_draws=False) -> dict:
    """What the device accumulates and gpirt_score_predict_combine reports, from stored draws fstar_draws (C, S, 1001, m)
    (or (S, 1001, m): one chain): each chain accumulated on its own, the sums and counters added in chain order.  Returns
    predict_result()'s keys (and, with return_draws, per chain the lists "q", "Hbar", "weights" and "products")."""
    top = check_top(top)
    f = np.asarray(fstar_draws, dtype=np.float64)
    if f.ndim == 3:
        f = f[None]
    if f.ndim != 4 or f.shape[2] != NGRID:
        raise ValueError("fstar_draws must be (C, S, 1001, m) or (S, 1001, m)")
    y = check_y_new(y_new, f.shape[3])
    chains = [predict_accumulate(y, fc, return_draws) for fc in f]
    pred_sum, info_sum = np.array(chains[0]["pred_sum"]), np.array(chains[0]["info_sum"])
    for c in chains[1:]:
        pred_sum = pred_sum + c["pred_sum"]
        info_sum = info_sum + c["info_sum"]
    draws = sum(c["pred_draws"] for c in chains)
    with np.errstate(invalid="ignore", divide="ignore"):
        S = float(draws) if draws > 0 else np.nan
        p_yes, info = pred_sum / S, info_sum / S
    items, vals = next_items(info, y, top)
    out = dict(p_yes=p_yes, info=info, next_items=items, next_info=vals, pred_sum=pred_sum, info_sum=info_sum,
               pred_draws=draws, pred_skipped=sum(c["pred_skipped"] for c in chains))
    if return_draws:
        for k in ("q", "Hbar", "weights", "products"):
            out[k] = [c[k] for c in chains]
    return out
