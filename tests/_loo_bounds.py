"""Bounds for the PSIS-LOO GPU tests (tests/test_gpu_loo.py), from the NumPy statement alone: the code under test is not involved.

For each case the statement (gpirt_amd.loo.from_draws) runs once in long double -- the reference -- and once in plain float64.
The float64 run makes the same roundings a correct fp64 implementation must make (the subtraction kappa - kmax, exp, log1p, the
sums over the tail, the softmax over the grid), so its largest distance from the reference over the case's cells measures how
ill-conditioned the case is for the quantity; a single cell's distance can be 0 by luck and says nothing.  The device may differ
from the reference, per cell, by
    16 x (the float64 run's largest difference over the case's cells) + 64 eps |value|:
the margin covers another exp / log1p (each within a few ulp) and another fixed summation order.
The sums kept per draw (evicted_sum, evicted_sumsq, p_sum) are sums of T positive terms, each term within 1.5 eps (r) or 3.5 eps
(r^2, 1 / r) of its exact value and every addition within eps / 2 of the partial sum: (T + 8) eps relative covers them.
"""
import functools

import numpy as np

from gpirt_amd import loo as LO

EPS = np.finfo(np.float64).eps
QUANTITIES = ("pareto_k", "elpd_loo", "n_eff", "loo_p_yes")

_CASES = {}


def register(name, y, chains, tail=None, top=20):
    """a case by name: y (n x m) and the chains' g = f + mu (each S x n x m); the references are computed on first use, once"""
    _CASES[name] = (y, chains, tail, top)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(long double result, float64 result) of from_draws for the registered case"""
    y, chains, tail, top = _CASES[name]
    return LO.from_draws(y, chains, tail=tail, top=top), LO.from_draws(y, chains, tail=tail, top=top, dtype=np.float64)


def pointwise_bound(name, quantity):
    """the per-cell bound of `quantity` for the case (NaN where the reference is NaN)"""
    want, f64 = reference(name)
    w, f = want["pointwise"][quantity], f64["pointwise"][quantity]
    assert np.array_equal(np.isnan(w), np.isnan(f)), (name, quantity)
    ok = ~np.isnan(w)
    spread = float(np.abs(f[ok] - w[ok]).max()) if ok.any() else 0.0
    return 16.0 * spread + 64.0 * EPS * np.abs(w)


def check_pointwise(name, got):
    """every quantity of the device's pointwise arrays inside its bound, NaN exactly where the reference has it; returns the
    largest used fraction of a bound per quantity"""
    want, _ = reference(name)
    used = {}
    for q in QUANTITIES:
        w, g = want["pointwise"][q], np.asarray(got["pointwise"][q])
        assert np.array_equal(np.isnan(g), np.isnan(w)), (name, q, "NaN positions")
        ok = ~np.isnan(w)
        if not ok.any():
            used[q] = 0.0
            continue
        b = pointwise_bound(name, q)[ok]
        frac = np.abs(g[ok] - w[ok]) / np.maximum(b, 1e-300)
        used[q] = float(frac.max())
        print(f"MEASURED {name} {q}: used {used[q]:.3f} of the bound")
    for q in QUANTITIES:
        assert used[q] <= 1.0, (name, q, used[q])
    return used


def check_sums(name, got_raw, T):
    """evicted_sum, evicted_sumsq and p_sum within (T + 8) eps relative of the long-double sums over the same values"""
    want, _ = reference(name)
    worst = 0.0
    for k in ("evicted_sum", "evicted_sumsq", "p_sum"):
        w = want["raw"][k]
        g = np.asarray(got_raw[k]).astype(np.longdouble)
        tol = (T + 8) * EPS * np.abs(w)
        err = np.abs(g - w)
        assert (err <= tol).all(), (name, k, float((err / np.maximum(tol, np.longdouble(1e-300))).max()))
        nz = tol > 0
        if nz.any():
            worst = max(worst, float((err[nz] / tol[nz]).max()))
    print(f"MEASURED {name} evicted sums / p_sum: used {worst:.3f} of (T + 8) eps")
    return worst
