"""PSIS-LOO without stored draws: leave-one-out cross-validation by Pareto-smoothed importance sampling for every observed cell,
its Pareto k diagnostic and the comparison of two models (include/gpirt_hip.h, "PSIS-LOO": gpirt_sampler_loo_*,
gpirt_loo_combine, gpirt_run.loo; csrc/loo.hip).

Per draw the device keeps, per cell, the K = M + 1 largest keys kappa = -y (f + mu) in a min-heap and the sums of the importance
ratios of everything else; at the end one wave per cell sorts the kept keys and fits the generalised Pareto tail.  `struct` /
`result` wrap the C struct, `combine` pools chains' state blocks, `from_draws` is the NumPy statement of the header over fetched
g = f + mu -- selection on the exact keys, every exp, log1p, sum and quotient in long double --, and `compare` is the difference
of two models' elpd_loo with its standard error.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import LOO_KEY_MAX, LOO_MAX_TAIL, LOO_MAX_TOP, LOO_POINTWISE, LOO_RAW, LOO_TOTALS, check

DEFAULT_TOP = 20
_COUNT_TOTALS = ("n_obs", "k_good", "k_bad", "k_very_bad", "unsmoothed", "cells_incomplete")


# ---------------------------------------------------------------------------------------------------- the contract ---
def check_tail(tail):
    """tail=None (the rule) or an integer in 5 .. 1024"""
    if tail is None:
        return None
    if isinstance(tail, bool) or not isinstance(tail, (int, np.integer)) or not 5 <= int(tail) <= LOO_MAX_TAIL:
        raise ValueError(f"loo: tail must be None or an integer in 5 .. {LOO_MAX_TAIL} (got {tail!r})")
    return int(tail)


def check_top(top):
    if isinstance(top, bool) or not isinstance(top, (int, np.integer)) or not 1 <= int(top) <= LOO_MAX_TOP:
        raise ValueError(f"loo: top must be an integer in 1 .. {LOO_MAX_TOP} (got {top!r})")
    return int(top)


def tail_length(T: int, tail=None) -> int:
    """M, the number of tail keys for T pooled draws: min(floor(T / 5), ceil(3 sqrt(T))), or `tail`.  M > 1024 and M >= T are
    ValueErrors that say so."""
    T = int(T)
    if T < 1:
        raise ValueError(f"loo: the planned number of draws must be at least 1 (got {T})")
    tail = check_tail(tail)
    if tail is not None:
        if tail >= T:
            raise ValueError(f"loo: a tail of {tail} keys and the cutoff need more than the {T} planned draws")
        return tail
    M = min(T // 5, math.isqrt(9 * T - 1) + 1)
    if M > LOO_MAX_TAIL:
        raise ValueError(f"loo: {T} planned draws give a tail of {M} keys, more than GPIRT_LOO_MAX_TAIL = {LOO_MAX_TAIL}; "
                         f"pass tail=")
    return M


def parse(loo) -> dict:
    """gpirtMCMC's loo= argument (True or a dict(tail, top)) as a checked dict."""
    if loo is True:
        loo = {}
    if not isinstance(loo, dict):
        raise ValueError("loo must be None, True or a dict(tail=..., top=...)")
    unknown = set(loo) - {"tail", "top"}
    if unknown:
        raise ValueError(f"loo: unknown keys {sorted(unknown)}")
    return dict(tail=check_tail(loo.get("tail")), top=check_top(loo.get("top", DEFAULT_TOP)))


def k_threshold(T: int) -> float:
    return min(1.0 - 1.0 / math.log10(T), 0.7) if T > 1 else float("-inf")


# ------------------------------------------------------------------------------------------------------ the device ---
def _raw_shape(name, n, m, M):
    return (M + 1, m, n) if name == "keys" else (m, n)          # C order: cell (i, j) at i + j n, slot-major keys


def struct(n: int, m: int, M: int, top: int = DEFAULT_TOP, tail=None):
    """A gpirt_loo asking for every array, and the host arrays behind it (kept alive by the caller)."""
    r = _lib.Loo()
    r.tail, r.top = 0 if tail is None else int(tail), check_top(top)
    arrays = {}
    for k, (name, dt) in enumerate(LOO_RAW):
        arrays[name] = np.zeros(_raw_shape(name, n, m, M), dtype=np.dtype(dt))
        r.raw[k] = arrays[name].ctypes.data
    for k, name in enumerate(LOO_POINTWISE):
        arrays["pw_" + name] = np.zeros((m, n))
        r.pointwise[k] = arrays["pw_" + name].ctypes.data
    arrays["item_elpd_loo"], arrays["respondent_elpd_loo"] = np.zeros(m), np.zeros(n)
    arrays["worst_index"], arrays["worst_k"] = np.zeros(r.top, dtype=np.int64), np.zeros(r.top)
    r.item_elpd_loo, r.respondent_elpd_loo = arrays["item_elpd_loo"].ctypes.data, arrays["respondent_elpd_loo"].ctypes.data
    r.worst_index, r.worst_k = arrays["worst_index"].ctypes.data, arrays["worst_k"].ctypes.data
    return r, arrays


def sorted_tail(keys, count):
    """the kept keys of every cell in descending order (K x n x m; NaN where a cell holds fewer than K keys), from the heaps
    (K x n x m) and `count`"""
    keys = np.array(keys, dtype=np.float64)
    K = keys.shape[0]
    held = np.minimum(np.asarray(count), K)
    keys[np.arange(K)[:, None, None] >= held[None]] = -np.inf
    out = -np.sort(-keys, axis=0)
    out[np.isneginf(out)] = np.nan
    return out


def _worst(index, k, n):
    index = np.asarray(index, dtype=np.int64)
    return dict(index=index, row=np.where(index >= 0, index % n, -1), col=np.where(index >= 0, index // n, -1),
                pareto_k=np.asarray(k, dtype=np.float64))


def result(r, arrays) -> dict:
    """The "loo" dict of gpirtMCMC(loo=...), Sampler.loo() and combine(), from a filled gpirt_loo."""
    n, m = int(r.n), int(r.m)
    out = {k: (int(r.totals[i]) if k in _COUNT_TOTALS else float(r.totals[i])) for i, k in enumerate(LOO_TOTALS)}
    out["pointwise"] = {name: arrays["pw_" + name].T for name in LOO_POINTWISE}
    raw = {name: (arrays[name].transpose(0, 2, 1) if name == "keys" else arrays[name].T) for name, _ in LOO_RAW}
    raw["tail"] = sorted_tail(raw["keys"], raw["count"])
    out.update(raw=raw, item_elpd_loo=arrays["item_elpd_loo"], respondent_elpd_loo=arrays["respondent_elpd_loo"],
               worst=_worst(arrays["worst_index"], arrays["worst_k"], n), n=n, m=m, T=int(r.T), M=int(r.M), draws=int(r.draws),
               chains=int(r.chains))
    return out


def state_header(state) -> dict:
    """The header of a LOO state block (a device tensor of int64)."""
    w = _lib.header_words(state, 16)
    return dict(tag=int(w[0]), version=int(w[1]), n=int(w[2]), m=int(w[3]), T=int(w[4]), M=int(w[5]), draws=int(w[6]),
                chains=int(w[7]))


def combine(handle, states, top=DEFAULT_TOP) -> dict:
    """gpirt_loo_combine over the state blocks `states` (device tensors, or Samplers with loo_enable() on, all on handle's
    device): pooled on the device in chain order (no signs: theta -> -theta does not change g), then finished.  States of
    another n, m, T, M or y are refused."""
    lib = _lib.load()
    tensors, nc, ptrs = _lib.state_ptrs(states, "loo_state")
    hdr = state_header(tensors[0])
    if hdr["tag"] != _lib.LOO_TAG:
        raise ValueError("loo.combine: state 0 is not a LOO state block")
    r, arrays = struct(hdr["n"], hdr["m"], hdr["M"], top)
    check(lib.gpirt_loo_combine(handle.ptr, nc, ptrs, C.byref(r)))
    return result(r, arrays)


# ------------------------------------------------------------------------------------------------------- NumPy -------
def totals(pointwise, y, T: int, top=DEFAULT_TOP) -> dict:
    """The totals, the item and respondent sums and the worst cells from the pointwise arrays (n x m) and y: the host's own
    reduction of what the device reduces in its fixed order."""
    top = check_top(top)
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    e, k = np.asarray(pointwise["elpd_loo"], dtype=np.float64), np.asarray(pointwise["pareto_k"], dtype=np.float64)
    fin = ~np.isnan(e)
    N = int(fin.sum())
    thr = k_threshold(T)
    with np.errstate(invalid="ignore", divide="ignore"):
        kk = k[fin]
        se = float(np.sqrt(N * np.var(e[fin], ddof=1))) if N > 1 else float("nan")
        out = dict(elpd_loo=float(e[fin].sum()), se_elpd_loo=se, p_loo=float(np.asarray(pointwise["p_loo"])[fin].sum()),
                   looic=float(-2.0 * e[fin].sum()), se_looic=2.0 * se, n_obs=N, lppd=float(np.asarray(pointwise["lppd"])[fin].sum()),
                   k_threshold=thr, k_good=int((kk <= thr).sum()), k_bad=int(((kk > thr) & (kk <= 1.0)).sum()),
                   k_very_bad=int((kk > 1.0).sum()), unsmoothed=int(np.isnan(kk).sum()),
                   cells_incomplete=int((~np.isnan(y) & ~fin).sum()), elpd_mean=float(e[fin].mean()) if N else float("nan"))
    out["item_elpd_loo"] = np.where(fin, e, 0.0).sum(axis=0)
    out["respondent_elpd_loo"] = np.where(fin, e, 0.0).sum(axis=1)
    kf = k.ravel(order="F")
    have = np.flatnonzero(~np.isnan(kf))
    order = have[np.lexsort((have, -kf[have]))][:top]                 # the largest k first, ties to the lowest index
    idx = np.full(top, -1, dtype=np.int64)
    idx[:order.size] = order
    out["worst"] = _worst(idx, np.where(idx >= 0, kf[np.maximum(idx, 0)], np.nan), n)
    return out


def _fit_cell(kept, es, es2, p_sum, yv, T, M, ld):
    """steps 1 to 6 of the header for one finished cell: kept (K float64 keys, ascending), the evicted sums and p_sum in `ld`"""
    one, half = ld(1), ld(0.5)
    kc, kmax = kept[0], kept[-1]
    with np.errstate(all="ignore"):
        e = np.exp((kept - kmax).astype(ld)) if ld is np.float64 else np.exp(kept.astype(ld) - ld(kmax))
        ec, emk = e[0], np.exp(-ld(kmax))
        x = e[1:] - ec
        smooth = M >= 5 and x[-1] > 0
        k = ld(np.nan)
        if smooth:
            mgrid = 30 + math.isqrt(M)
            xstar = x[(M + 2) // 4 - 1]
            j = np.arange(1, mgrid + 1).astype(ld)
            theta = one / x[-1] + (one - np.sqrt(ld(mgrid) / (j - half))) / (ld(3) * xstar)
            kj = np.log1p(-theta[:, None] * x[None, :]).sum(axis=1) / ld(M)
            lj = ld(M) * (np.log(-theta / kj) - kj - one)
            w = one / np.exp(lj[None, :] - lj[:, None]).sum(axis=1)
            that = (theta * w).sum()
            k0 = np.log1p(-that * x).sum() / ld(M)
            sigma = -k0 / that
            k = (k0 * ld(M) + ld(5)) / (ld(M) + ld(10))
            if not (np.isfinite(k) and np.isfinite(sigma)):
                smooth, k = False, ld(np.nan)
        rho = emk + e[1:]
        wt = rho
        if smooth:
            z = np.arange(1, M + 1).astype(ld)
            q = np.minimum(sigma * np.expm1(-k * np.log1p(-(z - half) / ld(M))) / k + ec, one)
            wt = emk + q
        rc = one + np.exp(ld(kc))
        E, E2 = es + rc, es2 + rc * rc
        W = E * emk + wt.sum()
        elpd = np.log(ld(T - M) + (wt / rho).sum()) - np.log(W) - ld(kmax)
        neff = W * W / ((E2 * emk) * emk + (wt * wt).sum())
        lppd = np.log(p_sum / ld(T))
        pyes = np.exp(elpd) if yv > 0 else one - np.exp(elpd)
    return k, elpd, neff, lppd, lppd - elpd, pyes


def from_draws(y, g_draws, tail=None, top=DEFAULT_TOP, dtype=np.longdouble) -> dict:
    """The NumPy statement of the header.  y: n x m (+1, -1, NaN); g_draws: one chain's g = f + mu (S x n x m) or a sequence of
    chains' (pooled in order; T is the total number of draws).  The K largest keys are selected on the exact float64 keys;
    every exp, log1p, sum and quotient runs in `dtype` (long double) and the pointwise results are returned rounded to float64.
    "raw" holds tail (the kept keys, descending, K x n x m), count, nonfinite and -- in `dtype` -- p_sum, evicted_sum and
    evicted_sumsq, the sums over the very keys that are not kept."""
    ld = np.dtype(dtype).type
    y = np.asarray(y, dtype=np.float64)
    chains = [g_draws] if isinstance(g_draws, np.ndarray) and g_draws.ndim == 3 else list(g_draws)
    g = np.concatenate([np.asarray(ch, dtype=np.float64) for ch in chains], axis=0)
    if g.ndim != 3 or g.shape[1:] != y.shape:
        raise ValueError("from_draws: a chain's g is S x n x m")
    T, (n, m) = g.shape[0], y.shape
    M = tail_length(T, tail)
    K = M + 1
    pw = {name: np.full((n, m), np.nan) for name in LOO_POINTWISE}
    raw = dict(tail=np.full((K, n, m), np.nan), count=np.zeros((n, m), dtype=np.int32), nonfinite=np.zeros((n, m), dtype=np.int32),
               p_sum=np.zeros((n, m), dtype=ld), evicted_sum=np.zeros((n, m), dtype=ld), evicted_sumsq=np.zeros((n, m), dtype=ld))
    for i in range(n):
        for j in range(m):
            if np.isnan(y[i, j]):
                continue
            gc = g[:, i, j]
            key = -(y[i, j] * gc)                                    # exact: the device forms the same double
            with np.errstate(invalid="ignore"):
                ok = np.isfinite(gc) & ~(key > LOO_KEY_MAX)
            ks = np.sort(key[ok])
            cnt = ks.size
            kept, gone = ks[max(cnt - K, 0):], ks[:max(cnt - K, 0)]
            r = ld(1) + np.exp(gone.astype(ld))
            raw["count"][i, j], raw["nonfinite"][i, j] = cnt, T - cnt
            raw["evicted_sum"][i, j], raw["evicted_sumsq"][i, j] = r.sum(), (r * r).sum()
            raw["p_sum"][i, j] = (ld(1) / (ld(1) + np.exp(ks.astype(ld)))).sum()
            raw["tail"][:kept.size, i, j] = kept[::-1]
            if cnt != T:
                continue
            vals = _fit_cell(kept, raw["evicted_sum"][i, j], raw["evicted_sumsq"][i, j], raw["p_sum"][i, j], y[i, j], T, M, ld)
            for name, v in zip(LOO_POINTWISE, vals):
                pw[name][i, j] = np.float64(v)
    out = totals(pw, y, T, top)
    out.update(pointwise=pw, raw=raw, n=n, m=m, T=T, M=M, draws=T, chains=len(chains))
    return out


def compare(a, b) -> dict:
    """elpd_loo(a) - elpd_loo(b) with its standard error, from two results (or their pointwise elpd_loo arrays) over the same
    data: elpd_diff, se_diff = sqrt(N var of the pointwise differences) (ddof 1) and n_obs.  Raises a ValueError that says so
    when the finished cells of the two differ."""
    pa, pb = (np.asarray(x["pointwise"]["elpd_loo"] if isinstance(x, dict) else x, dtype=np.float64) for x in (a, b))
    if pa.shape != pb.shape:
        raise ValueError(f"loo.compare: the pointwise arrays have different shapes, {pa.shape} and {pb.shape}")
    fa, fb = ~np.isnan(pa), ~np.isnan(pb)
    if not np.array_equal(fa, fb):
        raise ValueError(f"loo.compare: the finished cells differ ({int((fa != fb).sum())} cells are finished in one result "
                         f"only); compare models over the same observed cells")
    d = pa[fa] - pb[fa]
    N = int(d.size)
    se = float(np.sqrt(N * np.var(d, ddof=1))) if N > 1 else float("nan")
    return dict(elpd_diff=float(d.sum()), se_diff=se, n_obs=N)
