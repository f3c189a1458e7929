"""Shape posteriors of the item response curves without stored draws: monotonicity, peaks, crossings, slopes, information
(include/gpirt_hip.h, "IRF shape posteriors": gpirt_sampler_shape_*, gpirt_shape_combine, gpirt_mcmc_shape; csrc/shape.hip).

The curve of a draw is g = k*^T S^-1 f + mu*, the conditional mean draw_fstar forms (the sampler array "gbar"); the stored f* is
white noise around it.  Per draw and item the device finds, inside the window W = [500 - k_half, 500 + k_half] of the grid, the
argmax and argmin, the largest fall DD and rise DU (and from them, per tolerance, whether the draw is flat, increasing,
decreasing or non-monotone), the crossings of P = 1/2 and the extreme slopes, and over the whole grid the Fisher information.
`struct` / `finish` wrap the C struct, `combine` pools chains' state blocks (reflecting a chain exactly where its sign is
-1), and `from_draws` is the NumPy statement of the header over fetched curves: every integer it returns is what the device
must hold bit for bit; its information sums run in long double.

Arrays indexed [k, j] are returned as 1001 x m (views of the library's item-major storage).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import NGRID, SHAPE_MAX_TOLS, SHAPE_MAX_TOP, SHAPE_RAW, check

DEFAULT_WINDOW = 3.0
DEFAULT_TOLS = (0.0, 0.25, 1.0)
DEFAULT_PROBS = (0.025, 0.5, 0.975)
DEFAULT_TOP = 20
CENTRE = (NGRID - 1) // 2
FLAT, INCREASING, DECREASING, NONMONOTONE = 0, 1, 2, 3
_INT = ("cls", "peak_hist", "valley_hist", "cross_first_hist", "cross_last_hist", "cross_count", "draws", "nonfinite")


# ---------------------------------------------------------------------------------------------------- the contract ---
def check_window(window) -> int:
    """k_half = round(100 window) for a window in [0.01, 5.0] (theta units, half width about 0)"""
    w = float(window)
    if not (0.01 <= w <= 5.0):
        raise ValueError(f"shape: window = {window!r} is outside [0.01, 5.0]")
    return int(round(100.0 * w))


def check_tols(tols):
    t = tuple(float(x) for x in np.atleast_1d(np.asarray(tols, dtype=np.float64)))
    if not 1 <= len(t) <= SHAPE_MAX_TOLS:
        raise ValueError(f"shape: {len(t)} tolerances given, 1..{SHAPE_MAX_TOLS} are taken")
    if any(not (x >= 0.0) or not np.isfinite(x) for x in t):
        raise ValueError("shape: a tolerance must be finite and >= 0 (logits)")
    return t


def check_top(top) -> int:
    if int(top) != top or not 1 <= int(top) <= SHAPE_MAX_TOP:
        raise ValueError(f"shape: top = {top!r} is outside 1..{SHAPE_MAX_TOP}")
    return int(top)


def check_probs(probs):
    p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    if ((p < 0.0) | (p > 1.0) | np.isnan(p)).any():
        raise ValueError("shape: probs must lie in [0, 1]")
    return p


def parse(shape) -> dict:
    """gpirtMCMC's shape= argument (True or a dict(window, tols, probs, top)) as a checked dict with k_half."""
    if shape is not True and not isinstance(shape, dict):
        raise ValueError("shape must be None, False, True or a dict(window=..., tols=..., probs=..., top=...)")
    d = dict(shape) if isinstance(shape, dict) else {}
    unknown = set(d) - {"window", "tols", "probs", "top"}
    if unknown:
        raise ValueError(f"shape: unknown keys {sorted(unknown)}")
    window = d.get("window", DEFAULT_WINDOW)
    return dict(window=float(window), k_half=check_window(window), tols=check_tols(d.get("tols", DEFAULT_TOLS)),
                probs=check_probs(d.get("probs", DEFAULT_PROBS)), top=check_top(d.get("top", DEFAULT_TOP)))


def _raw_shape(name, m):
    return dict(cls=(SHAPE_MAX_TOLS, 4, m), peak_hist=(m, NGRID), valley_hist=(m, NGRID), cross_first_hist=(m, NGRID),
                cross_last_hist=(m, NGRID), cross_count=(4, m), draws=(m,), nonfinite=(m,), slope=(4, m), info_sum=(m, NGRID),
                ti_sum=(NGRID,), ti_sumsq=(NGRID,), rel=(2,))[name]


def _public(name, a, n_tols):
    """the library's storage of raw array `name` as this module returns it: [k, j] arrays as 1001 x m, cls cut to n_tols"""
    if name.endswith("_hist") or name == "info_sum":
        return a.T
    return a[:n_tols] if name == "cls" else a


def grid_weights():
    """the N(0, 1) density on the grid, normalised, in long double from the double theta_k = -5 + 0.01 k"""
    th = (-5.0 + np.arange(NGRID, dtype=np.float64) * 0.01).astype(np.longdouble)
    w = np.exp(-(th * th) / 2)
    return w / w.sum()


# ------------------------------------------------------------------------------------------------------ the device ---
def struct(m: int, k_half=None, tols=None):
    """A gpirt_shape asking for every raw array, and the host arrays behind it (kept alive by the caller).  k_half and tols
    are read by gpirt_mcmc_shape; gpirt_shape_combine ignores them."""
    r = _lib.Shape()
    arrays = {}
    for k, (name, dt) in enumerate(SHAPE_RAW):
        arrays[name] = np.zeros(_raw_shape(name, m), dtype=np.dtype(dt))
        r.raw[k] = arrays[name].ctypes.data
    if k_half is not None:
        r.k_half = int(k_half)
        r.n_tols = len(tols)
        for q, t in enumerate(tols):
            r.tols[q] = t
    return r, arrays


def result(r, arrays, probs=DEFAULT_PROBS, top=DEFAULT_TOP) -> dict:
    """The "shape" dict of gpirtMCMC(shape=...), Sampler.shape() and combine(), from a filled gpirt_shape."""
    n_tols = int(r.n_tols)
    raw = {name: _public(name, arrays[name], n_tols) for name, _ in SHAPE_RAW}
    return finish(raw, int(r.k_half), [float(r.tols[q]) for q in range(n_tols)], probs, top, int(r.info_draws),
                  int(r.info_skipped))


def combine(handle, states, signs=None, probs=DEFAULT_PROBS, top=DEFAULT_TOP) -> dict:
    """gpirt_shape_combine over the shape state blocks `states` (device tensors, or Samplers with shape_enable() on, all on
    handle's device): the integers added, the doubles added in chain order, a chain with sign -1 reflected exactly first
    (signs=None: nothing is reflected)."""
    lib = _lib.load()
    probs, top = check_probs(probs), check_top(top)
    tensors = [s.shape_state() if hasattr(s, "shape_state") else s for s in states]
    m = state_header(tensors[0])["m"]
    r, arrays = struct(m)
    nc = len(tensors)
    ptrs = (C.c_void_p * nc)(*[t.data_ptr() for t in tensors])
    sg = (C.c_int * nc)(*[int(x) for x in signs]) if signs is not None else None
    check(lib.gpirt_shape_combine(handle.ptr, nc, ptrs, sg, C.byref(r)))
    return result(r, arrays, probs, top)


def state_header(state) -> dict:
    """The header of a shape state block (a device tensor of int64): tag, version, n, m, k_half, the tolerances, the counters."""
    w = state[:16].cpu().numpy().view(np.int64)
    n_tols = int(w[5])
    return dict(tag=int(w[0]), version=int(w[1]), n=int(w[2]), m=int(w[3]), k_half=int(w[4]),
                tols=[float(x) for x in w[6:6 + n_tols].view(np.float64)], info_draws=int(w[10]), info_skipped=int(w[11]))


# ------------------------------------------------------------------------------------------------------- finishing ---
def _hist_quantiles(hist, probs, offset):
    """per item the max(1, ceil(q S))-th smallest index of a 1001 x m histogram as theta = -5 + 0.01 (k + offset); NaN where
    the histogram is empty"""
    cum = np.cumsum(hist.astype(np.int64), axis=0)
    S = cum[-1]
    out = np.full((len(probs), hist.shape[1]), np.nan)
    for p, q in enumerate(probs):
        need = np.maximum(np.ceil(q * S.astype(np.float64)), 1.0)
        k = (cum < need[None, :]).sum(axis=0)
        out[p] = np.where(S > 0, -5.0 + 0.01 * (np.minimum(k, NGRID - 1) + offset), np.nan)
    return out


def finish(raw, k_half, tols, probs=DEFAULT_PROBS, top=DEFAULT_TOP, info_draws=0, info_skipped=0) -> dict:
    """The finished outputs from (pooled) raw accumulators in this module's layout; shared by the device path and from_draws."""
    probs, top = check_probs(probs), check_top(top)
    k_lo, k_hi = CENTRE - k_half, CENTRE + k_half
    out = dict(raw)
    out.update(window=k_half / 100.0, k_lo=k_lo, k_hi=k_hi, tols=np.array(tols, dtype=np.float64), probs=probs,
               info_draws=int(info_draws), info_skipped=int(info_skipped))
    with np.errstate(invalid="ignore", divide="ignore"):
        S = raw["draws"].astype(np.float64)
        cls = raw["cls"] / S
        out["p_flat"], out["p_increasing"] = cls[:, FLAT], cls[:, INCREASING]
        out["p_decreasing"], out["p_nonmonotone"] = cls[:, DECREASING], cls[:, NONMONOTONE]
        out["peak_quantiles"] = _hist_quantiles(raw["peak_hist"], probs, 0.0)
        out["valley_quantiles"] = _hist_quantiles(raw["valley_hist"], probs, 0.0)
        out["p_peak_interior"] = raw["peak_hist"][k_lo + 1:k_hi].sum(axis=0) / S
        out["crossings"] = raw["cross_count"] / S
        # a crossing pair (k, k + 1) is reported at its midpoint
        out["difficulty_quantiles"] = _hist_quantiles(raw["cross_first_hist"], probs, 0.5)
        out["slope_max_mean"], out["slope_min_mean"] = raw["slope"][0] / S, raw["slope"][2] / S
        out["slope_max_sd"] = np.sqrt(np.maximum(raw["slope"][1] - raw["slope"][0] ** 2 / S, 0.0) / (S - 1.0))
        out["slope_min_sd"] = np.sqrt(np.maximum(raw["slope"][3] - raw["slope"][2] ** 2 / S, 0.0) / (S - 1.0))
        out["item_info"] = raw["info_sum"] / S[None, :]
        T = np.float64(info_draws)
        out["test_info_mean"] = raw["ti_sum"] / T
        out["test_info_sd"] = np.sqrt(np.maximum(raw["ti_sumsq"] - raw["ti_sum"] ** 2 / T, 0.0) / (T - 1.0))
        out["sem"] = 1.0 / np.sqrt(out["test_info_mean"])
        out["reliability_mean"] = float(raw["rel"][0] / T)
        out["reliability_sd"] = float(np.sqrt(max(raw["rel"][1] - raw["rel"][0] ** 2 / T, 0.0) / (T - 1.0)))
    # the items most often non-monotone at the largest tolerance: decreasing p, ties to the lowest j, NaN never listed
    p = out["p_nonmonotone"][int(np.argmax(out["tols"]))]
    order = [j for j in np.argsort(-np.where(np.isnan(p), -np.inf, p), kind="stable") if not np.isnan(p[j])][:top]
    out["nonmonotone"] = dict(items=np.array(order, dtype=np.int64), p=p[order] if order else np.empty(0))
    return out


# ------------------------------------------------------------------------------------------------------- NumPy -------
def zeros(m: int, n_tols: int) -> dict:
    """empty accumulators in this module's layout (the doubles of the information in long double)"""
    ld = np.longdouble
    return dict(cls=np.zeros((n_tols, 4, m), dtype=np.uint32), peak_hist=np.zeros((NGRID, m), dtype=np.uint32),
                valley_hist=np.zeros((NGRID, m), dtype=np.uint32), cross_first_hist=np.zeros((NGRID, m), dtype=np.uint32),
                cross_last_hist=np.zeros((NGRID, m), dtype=np.uint32), cross_count=np.zeros((4, m), dtype=np.uint32),
                draws=np.zeros(m, dtype=np.uint32), nonfinite=np.zeros(m, dtype=np.uint32), slope=np.zeros((4, m)),
                info_sum=np.zeros((NGRID, m), dtype=ld), ti_sum=np.zeros(NGRID, dtype=ld), ti_sumsq=np.zeros(NGRID, dtype=ld),
                rel=np.zeros(2, dtype=ld), info_draws=0, info_skipped=0)


def draw_info(g):
    """I[k, j] of one curve draw g (1001 x m, finite) in long double: (e / ((1 + e)(1 + e))) g'^2, e = exp(-|g|),
    g' = (g[k + 1] - g[k - 1]) / 0.02, one-sided (/ 0.01) at the two ends"""
    gl = np.asarray(g, dtype=np.float64).astype(np.longdouble)
    gp = np.empty_like(gl)
    gp[1:-1] = (gl[2:] - gl[:-2]) / np.longdouble(np.float64(0.02))
    gp[0] = (gl[1] - gl[0]) / np.longdouble(np.float64(0.01))
    gp[-1] = (gl[-1] - gl[-2]) / np.longdouble(np.float64(0.01))
    e = np.exp(-np.abs(gl))
    return (e / ((1 + e) * (1 + e))) * (gp * gp)


def accumulate(acc, g, k_half, tols):
    """Add one curve draw g (1001 x m, float64) to the accumulators `acc`: the header's rules, one statement each."""
    g = np.asarray(g, dtype=np.float64)
    k_lo, k_hi = CENTRE - k_half, CENTRE + k_half
    ok = np.isfinite(g).all(axis=0)                      # an item with ANY non-finite g is skipped, inside W or not
    acc["nonfinite"] += (~ok).astype(np.uint32)
    acc["draws"] += ok.astype(np.uint32)
    cols = np.flatnonzero(ok)
    if cols.size:
        W = g[k_lo:k_hi + 1][:, cols]
        acc["peak_hist"][k_lo + np.argmax(W, axis=0), cols] += 1          # first occurrence: the lowest k on ties
        acc["valley_hist"][k_lo + np.argmin(W, axis=0), cols] += 1
        DD = (np.maximum.accumulate(W, axis=0) - W).max(axis=0)
        DU = (W - np.minimum.accumulate(W, axis=0)).max(axis=0)
        for t, tol in enumerate(tols):
            c = np.where(DD <= tol, np.where(DU <= tol, FLAT, INCREASING), np.where(DU <= tol, DECREASING, NONMONOTONE))
            acc["cls"][t, c, cols] += 1
        sg = W >= 0.0
        x = sg[:-1] != sg[1:]
        cnt = x.sum(axis=0)
        acc["cross_count"][np.minimum(cnt, 3), cols] += 1
        has = cnt >= 1
        acc["cross_first_hist"][k_lo + np.argmax(x, axis=0)[has], cols[has]] += 1
        acc["cross_last_hist"][k_lo + x.shape[0] - 1 - np.argmax(x[::-1], axis=0)[has], cols[has]] += 1
        d = W[1:] - W[:-1]
        smax, smin = d.max(axis=0) / 0.01, d.min(axis=0) / 0.01
        acc["slope"][0, cols] += smax
        acc["slope"][1, cols] += smax * smax
        acc["slope"][2, cols] += smin
        acc["slope"][3, cols] += smin * smin
        I = draw_info(g[:, cols])
        acc["info_sum"][:, cols] += I
    if not ok.all():
        acc["info_skipped"] += 1
        return
    acc["info_draws"] += 1
    TI = I.sum(axis=1)
    acc["ti_sum"] += TI
    acc["ti_sumsq"] += TI * TI
    rho = (grid_weights() * (TI / (TI + 1))).sum()
    acc["rel"] += np.array([rho, rho * rho])


def reflect(acc) -> dict:
    """theta -> -theta on the accumulators (exact: W is symmetric).  The argmax tie rule was applied before."""
    out = dict(acc)
    for k in ("peak_hist", "valley_hist", "info_sum", "ti_sum", "ti_sumsq"):
        out[k] = acc[k][::-1].copy()
    for a, b in (("cross_first_hist", "cross_last_hist"), ("cross_last_hist", "cross_first_hist")):
        h = acc[b].copy()
        h[:NGRID - 1] = acc[b][NGRID - 2::-1]            # pair index k -> 999 - k
        out[a] = h
    out["cls"] = acc["cls"][:, [FLAT, DECREASING, INCREASING, NONMONOTONE]].copy()
    s = acc["slope"]
    out["slope"] = np.stack([-s[2], s[3], -s[0], s[1]])
    return out


def add(a, b) -> dict:
    """a + b, accumulator by accumulator (chains pooled in order)"""
    return {k: a[k] + b[k] for k in a}


def from_draws(gbar_draws, window=DEFAULT_WINDOW, tols=DEFAULT_TOLS, probs=DEFAULT_PROBS, top=DEFAULT_TOP, signs=None) -> dict:
    """The NumPy statement of the header over fetched curves.  gbar_draws: one chain's curves (S x 1001 x m) or a sequence
    of chains' curves; signs: per chain, -1 reflects that chain's accumulators before pooling.  The integers are what the
    device must hold bit for bit; the information's sums run in long double and are returned rounded to float64."""
    k_half, tols = check_window(window), check_tols(tols)
    chains = [gbar_draws] if isinstance(gbar_draws, np.ndarray) and gbar_draws.ndim == 3 else list(gbar_draws)
    if signs is None:
        signs = [1] * len(chains)
    if len(signs) != len(chains) or any(s not in (1, -1) for s in signs):
        raise ValueError("from_draws: signs must give +1 or -1 per chain")
    pooled = None
    for ch, sg in zip(chains, signs):
        ch = np.asarray(ch, dtype=np.float64)
        if ch.ndim != 3 or ch.shape[1] != NGRID:
            raise ValueError("from_draws: a chain's curves are S x 1001 x m")
        acc = zeros(ch.shape[2], len(tols))
        for g in ch:
            accumulate(acc, g, k_half, tols)
        if sg < 0:
            acc = reflect(acc)
        pooled = acc if pooled is None else add(pooled, acc)
    raw = {k: (np.asarray(v, dtype=np.float64) if isinstance(v, np.ndarray) and v.dtype == np.longdouble else v)
           for k, v in pooled.items() if k not in ("info_draws", "info_skipped")}
    return finish(raw, k_half, tols, probs, top, pooled["info_draws"], pooled["info_skipped"])
