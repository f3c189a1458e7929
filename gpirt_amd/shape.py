"""Shape posteriors of the item response curves without stored draws: monotonicity, peaks, crossings, slopes, information
(include/gpirt_hip.h, "IRF shape posteriors": gpirt_sampler_shape_*, gpirt_shape_combine, gpirt_run.shape; csrc/shape.hip),
and on top of them the item-pair order posteriors (gpirt_sampler_shape_order_*, csrc/order.hip; the order_* functions below).

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
from ._lib import NGRID, ORDER_MAX_M, ORDER_MAX_TOP, ORDER_RAW, SHAPE_MAX_TOLS, SHAPE_MAX_TOP, SHAPE_RAW, check

DEFAULT_WINDOW = 3.0
DEFAULT_TOLS = (0.0, 0.25, 1.0)
DEFAULT_PROBS = (0.025, 0.5, 0.975)
DEFAULT_TOP = 20
DEFAULT_ORDER_TOP = 20
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


def check_order_top(top) -> int:
    if isinstance(top, bool) or int(top) != top or not 1 <= int(top) <= ORDER_MAX_TOP:
        raise ValueError(f"shape: order_top = {top!r} is outside 1..{ORDER_MAX_TOP}")
    return int(top)


def check_order_m(m) -> int:
    if not 2 <= int(m) <= ORDER_MAX_M:
        raise ValueError(f"shape: the order posteriors take 2..{ORDER_MAX_M} items, m = {m}")
    return int(m)


def check_probs(probs):
    p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    if ((p < 0.0) | (p > 1.0) | np.isnan(p)).any():
        raise ValueError("shape: probs must lie in [0, 1]")
    return p


def parse(shape) -> dict:
    """gpirtMCMC's shape= argument (True or a dict(window, tols, probs, top, order, order_top)) as a checked dict with k_half."""
    if shape is not True and not isinstance(shape, dict):
        raise ValueError("shape must be None, False, True or a dict(window=..., tols=..., probs=..., top=..., order=..., "
                         "order_top=...)")
    d = dict(shape) if isinstance(shape, dict) else {}
    unknown = set(d) - {"window", "tols", "probs", "top", "order", "order_top"}
    if unknown:
        raise ValueError(f"shape: unknown keys {sorted(unknown)}")
    window = d.get("window", DEFAULT_WINDOW)
    order = d.get("order", False)
    if order not in (True, False):
        raise ValueError(f"shape: order = {order!r} must be True or False")
    return dict(window=float(window), k_half=check_window(window), tols=check_tols(d.get("tols", DEFAULT_TOLS)),
                probs=check_probs(d.get("probs", DEFAULT_PROBS)), top=check_top(d.get("top", DEFAULT_TOP)),
                order=bool(order), order_top=check_order_top(d.get("order_top", DEFAULT_ORDER_TOP)))


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
    are read by gpirt_mcmc_run; gpirt_shape_combine ignores them."""
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
    tensors, nc, ptrs = _lib.state_ptrs(states, "shape_state")
    m = state_header(tensors[0])["m"]
    r, arrays = struct(m)
    sg = (C.c_int * nc)(*[int(x) for x in signs]) if signs is not None else None
    check(lib.gpirt_shape_combine(handle.ptr, nc, ptrs, sg, C.byref(r)))
    return result(r, arrays, probs, top)


def state_header(state) -> dict:
    """The header of a shape state block (a device tensor of int64): tag, version, n, m, k_half, the tolerances, the counters."""
    w = _lib.header_words(state, 16)
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


# ---------------------------------------------------------------------------- item-pair order posteriors (order.hip) ---
def _order_raw_shape(name, m, n_tols):
    """the library's storage of the order block's raw array `name` (set_counts keeps all SHAPE_MAX_TOLS slots)"""
    return dict(above=(n_tols, m, m), cross=(n_tols, m, m), easier=(m, m), depth_sum=(m, m), easiness=(2, m),
                set_counts=(3, SHAPE_MAX_TOLS))[name]


def order_state_bytes(m: int, n_tols: int) -> int:
    """the size of an order state block by the layout: 16 int64, then the arrays, each padded to 16 bytes"""
    at = 16 * 8
    for name, dt in ORDER_RAW:
        at += (int(np.prod(_order_raw_shape(name, m, n_tols))) * np.dtype(dt).itemsize + 15) // 16 * 16
    return at


def order_struct(m: int, n_tols: int, top=DEFAULT_ORDER_TOP):
    """A gpirt_shape_order asking for every raw array and the worst pairs, and the host arrays behind it."""
    r = _lib.ShapeOrder()
    r.top = check_order_top(top)
    arrays = {}
    for k, (name, dt) in enumerate(ORDER_RAW):
        arrays[name] = np.zeros(_order_raw_shape(name, m, n_tols), dtype=np.dtype(dt))
        r.raw[k] = arrays[name].ctypes.data
    arrays["worst_a"] = np.full(r.top, -1, dtype=np.int64)
    arrays["worst_b"] = np.full(r.top, -1, dtype=np.int64)
    r.worst_a, r.worst_b = arrays["worst_a"].ctypes.data, arrays["worst_b"].ctypes.data
    return r, arrays


def order_result(r, arrays) -> dict:
    """The "order" dict from a filled gpirt_shape_order (the worst pairs are the library's)."""
    n_tols, nw = int(r.n_tols), int(r.n_worst)
    raw = {name: arrays[name] for name, _ in ORDER_RAW}
    raw["set_counts"] = raw["set_counts"][:, :n_tols]
    worst = np.stack([arrays["worst_a"][:nw], arrays["worst_b"][:nw]], axis=1)
    return order_finish(raw, int(r.k_half), [float(r.tols[q]) for q in range(n_tols)], int(r.top), int(r.draws), int(r.skipped),
                        worst=worst)


def order_combine(handle, states, top=DEFAULT_ORDER_TOP) -> dict:
    """gpirt_shape_order_combine over the order state blocks `states` (device tensors, or Samplers with shape_order_enable()
    on): the integers added, the doubles added in chain order.  No signs: theta -> -theta changes nothing in this block."""
    lib = _lib.load()
    top = check_order_top(top)
    tensors, nc, ptrs = _lib.state_ptrs(states, "shape_order_state")
    hd = order_state_header(tensors[0])
    r, arrays = order_struct(hd["m"], len(hd["tols"]), top)
    check(lib.gpirt_shape_order_combine(handle.ptr, nc, ptrs, C.byref(r)))
    return order_result(r, arrays)


def order_state_header(state) -> dict:
    """The header of an order state block (a device tensor of int64): tag, version, n, m, k_half, the tolerances, the counters."""
    w = _lib.header_words(state, 16)
    n_tols = int(w[5])
    return dict(tag=int(w[0]), version=int(w[1]), n=int(w[2]), m=int(w[3]), k_half=int(w[4]),
                tols=[float(x) for x in w[6:6 + n_tols].view(np.float64)], draws=int(w[10]), skipped=int(w[11]))


def order_worst(cross_t, top):
    """the `top` pairs a < b with the largest count in cross_t (m x m), ties to the lowest (a, b): an array of (a, b) rows"""
    m = cross_t.shape[0]
    a, b = np.triu_indices(m, 1)                          # in (a, b) order
    pick = np.argsort(-cross_t[a, b].astype(np.int64), kind="stable")[:top]
    return np.stack([a[pick], b[pick]], axis=1).astype(np.int64)


def order_finish(raw, k_half, tols, top=DEFAULT_ORDER_TOP, draws=0, skipped=0, worst=None) -> dict:
    """The finished outputs from (pooled) raw order accumulators; shared by the device path and order_from_draws."""
    top = check_order_top(top)
    tols = np.array(tols, dtype=np.float64)
    out = dict(raw)
    m = raw["easier"].shape[0]
    out.update(window=k_half / 100.0, k_lo=CENTRE - k_half, k_hi=CENTRE + k_half, tols=tols, draws=int(draws), skipped=int(skipped))
    eye = np.eye(m, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        S = np.float64(draws)
        nan_diag = lambda x: np.where(eye, np.nan, x)                          # noqa: E731
        out["p_above"] = nan_diag(raw["above"] / S)
        out["p_cross"] = nan_diag(raw["cross"] / S)
        # (b above a) is above[t, b, a]: what is left of the draws is tied
        tied = np.int64(draws) - raw["above"].astype(np.int64) - raw["above"].astype(np.int64).transpose(0, 2, 1) - raw["cross"]
        out["p_tied"] = nan_diag(tied / S)
        out["p_easier"] = nan_diag(raw["easier"] / S)
        out["depth_mean"] = nan_diag(raw["depth_sum"] / S)
        out["easiness_mean"] = raw["easiness"][0] / S
        out["easiness_sd"] = np.sqrt(np.maximum(raw["easiness"][1] - raw["easiness"][0] ** 2 / S, 0.0) / (S - 1.0))
        # a mean rank is linear in the indicators: 1 + the expected number of items easier than j
        out["rank_mean"] = 1.0 + raw["easier"].astype(np.float64).sum(axis=0) / S
        out["order"] = np.argsort(np.where(np.isnan(out["rank_mean"]), np.inf, out["rank_mean"]), kind="stable").astype(np.int64)
        out["cross_items_mean"] = raw["cross"].astype(np.float64).sum(axis=2) / S
        sc = raw["set_counts"].astype(np.float64)
        out["p_iio"] = sc[0] / S
        out["cross_pairs_mean"] = sc[1] / S
        out["cross_pairs_sd"] = np.sqrt(np.maximum(sc[2] - sc[1] ** 2 / S, 0.0) / (S - 1.0))
        qmax = int(np.argmax(tols))
        if worst is None:
            worst = order_worst(raw["cross"][qmax], top)
        wa, wb = worst[:, 0], worst[:, 1]
        out["worst"] = dict(pairs=worst, p_cross=raw["cross"][qmax][wa, wb] / S, depth_mean=raw["depth_sum"][wa, wb] / S)
    return out


def order_ranks_from_easiness(e_draws):
    """easier[a, b] = #{draws with e_a > e_b} from the draws' easiness (S x m), as uint32"""
    e = np.asarray(e_draws)
    if e.ndim != 2:
        raise ValueError("order_ranks_from_easiness: e_draws is S x m")
    out = np.zeros((e.shape[1], e.shape[1]), dtype=np.uint32)
    for row in e:
        out += (row[:, None] > row[None, :]).astype(np.uint32)
    return out


def order_draw_easiness(g):
    """e_j of one curve draw g (1001 x m, finite) in long double: sum over the whole grid of w_k / (1 + exp(-g[k, j]))"""
    gl = np.asarray(g, dtype=np.float64).astype(np.longdouble)
    with np.errstate(over="ignore"):
        return (grid_weights()[:, None] / (1 + np.exp(-gl))).sum(axis=0)


def order_draw_u(g, k_half):
    """U[a, b] = max over k in W of fl(g[k, a] - g[k, b]) of one curve draw g (1001 x m), in fp64"""
    W = np.asarray(g, dtype=np.float64)[CENTRE - k_half:CENTRE + k_half + 1]
    m = W.shape[1]
    U = np.empty((m, m))
    with np.errstate(over="ignore"):
        for a in range(m):
            U[a] = (W[:, a:a + 1] - W).max(axis=0)
    return U


def order_from_draws(gbar_draws, window=DEFAULT_WINDOW, tols=DEFAULT_TOLS, top=DEFAULT_ORDER_TOP) -> dict:
    """The NumPy statement of the header's order block over fetched curves.  gbar_draws: one chain's curves (S x 1001 x m) or a
    sequence of chains' curves (each accumulated on its own, then added in chain order, as gpirt_shape_order_combine does).
    Everything about U is fp64 and is what the device must hold bit for bit; e runs in long double ("e_draws", the counted
    draws' e in order, S x m, with easier decided on it; easiness rounded to float64 at the end).  "u" is the last counted
    draw's U (the diagonal 0), "ncross" its crossing pairs per tolerance."""
    k_half, tols, top = check_window(window), check_tols(tols), check_order_top(top)
    chains = [gbar_draws] if isinstance(gbar_draws, np.ndarray) and gbar_draws.ndim == 3 else list(gbar_draws)
    m = check_order_m(np.asarray(chains[0]).shape[2])
    nt = len(tols)
    off = ~np.eye(m, dtype=bool)
    upper = np.triu(np.ones((m, m), dtype=bool), 1)
    pooled, e_draws = None, []
    u = np.zeros((m, m))
    ncross = np.zeros(nt, dtype=np.int64)
    draws = skipped = 0
    for ch in chains:
        ch = np.asarray(ch, dtype=np.float64)
        if ch.ndim != 3 or ch.shape[1] != NGRID or ch.shape[2] != m:
            raise ValueError("order_from_draws: a chain's curves are S x 1001 x m")
        acc = dict(above=np.zeros((nt, m, m), dtype=np.uint32), cross=np.zeros((nt, m, m), dtype=np.uint32),
                   easier=np.zeros((m, m), dtype=np.uint32), depth_sum=np.zeros((m, m)),
                   easiness=np.zeros((2, m), dtype=np.longdouble), set_counts=np.zeros((3, nt), dtype=np.uint64))
        for g in ch:
            if not np.isfinite(g).all():                 # any item, anywhere on the grid: the draw is skipped whole
                skipped += 1
                continue
            draws += 1
            U = order_draw_u(g, k_half)
            L = -U.T                                     # the minimum over W of g_a - g_b
            for q, t in enumerate(tols):
                hi, lo = (U > t) & off, (L < -t) & off
                x = hi & lo
                acc["cross"][q] += x.astype(np.uint32)
                acc["above"][q] += (hi & ~lo).astype(np.uint32)
                nc = int((x & upper).sum())
                ncross[q] = nc
                acc["set_counts"][:, q] += np.array([nc == 0, nc, nc * nc], dtype=np.uint64)
            acc["depth_sum"] += np.where(off, np.minimum(np.maximum(U, 0.0), np.maximum(-L, 0.0)), 0.0)
            u = np.where(off, U, 0.0)
            e = order_draw_easiness(g)
            e_draws.append(e)
            acc["easier"] += order_ranks_from_easiness(e[None, :])
            acc["easiness"] += np.stack([e, e * e])
        pooled = acc if pooled is None else {k: pooled[k] + acc[k] for k in acc}
    pooled["easiness"] = np.asarray(pooled["easiness"], dtype=np.float64)
    out = order_finish(pooled, k_half, tols, top, draws, skipped)
    out.update(u=u, ncross=ncross, e_draws=np.array(e_draws, dtype=np.longdouble).reshape(len(e_draws), m))
    return out
