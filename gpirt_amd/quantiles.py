"""Quantiles of long chains without their draws (include/gpirt_hip.h GPIRT_SUM_THETA_HIST, GPIRT_SUM_IRF_BAND,
gpirt_summary_quantiles, gpirt_run.quantiles).

Every theta draw is a point of the fixed grid theta* = -5 + 0.01 k, k = 0..1000, so a count per (respondent, grid point)
is the exact posterior of theta in n x 1001 counts however long the chain: exact quantiles, the median, the mode, exact
pooling over chains (an integer sum; the reflection theta -> -theta reverses the grid index) and -- from the counts of
DIAG's two halves -- the rank-normalised split-R-hat of Vehtari et al. (2021), bulk and tail, exactly.  The rank-normalised
bulk-ESS and tail-ESS are not offered: the ranks are not known until the end of the chain.  The autocorrelation ESS of the values
themselves is (gpirt_amd.acf).

f* is not on a grid; each cell (grid point k, item j) keeps a histogram of 256 bins that cut the probability scale evenly
(edges e_b = logit(b / 256) on the f* scale, gpirt_irf_band_edges) and the sum of plogis(f*).  A band quantile is
interpolated inside the bin that holds the order statistic, so it is within 1/256 of the exact sample quantile of
plogis(f*).

`from_states` runs the device extraction on state blocks (Sampler.summary_state()).  `from_draws` is the NumPy reference
over stored draws (scipy.stats.rankdata, scipy.special.ndtri) and `from_histograms` computes the same from the histograms
alone by the histogram algebra: two independent routes that the tests hold against each other.
ShardedSampler is not covered: item shards would need their f* bands gathered.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import NGRID, check

BINS = _lib.IRF_BINS
_dp = C.POINTER(C.c_double)


def _ptr(a):
    return a.ctypes.data_as(_dp)


def band_edges() -> np.ndarray:
    """The 255 edges e_b = logit(b / 256), b = 1..255, as the library computes them (gpirt_irf_band_edges)."""
    e = np.empty(BINS - 1)
    check(_lib.load().gpirt_irf_band_edges(_ptr(e)))
    return e


def plogis(x):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def ranks(probs, T: int) -> np.ndarray:
    """max(ceil(q T), 1): the 1-based order statistic of quantile q over T draws."""
    return np.maximum(np.ceil(np.asarray(probs, dtype=np.float64) * T), 1).astype(np.int64)


# ------------------------------------------------------------------------------------------------------ the device ---
def quantiles_struct(probs, n: int, m: int, chains: int, theta=True, rhat=True, irf=True):
    """A gpirt_quantiles with host arrays for the outputs asked for, and those arrays (kept alive by the caller)."""
    q = _lib.Quantiles()
    pr = np.ascontiguousarray(np.asarray(probs, dtype=np.float64).ravel())
    arrays = {"probs": pr}
    q.nprobs = pr.size
    q.probs = _ptr(pr)
    shapes = {}
    if theta:
        shapes.update(theta_q=(pr.size, n), theta_median=(n,), theta_mode=(n,), theta_hist=(NGRID, n))
    if rhat:
        shapes.update(theta_rhat_bulk=(n,), theta_rhat_tail=(n,), theta_rhat=(n,))
    if irf:
        shapes.update(irf_q=(pr.size, NGRID, m), irf_p_mean=(NGRID, m))
    for k, shp in shapes.items():
        a = np.empty(shp, order="F")
        arrays[k] = a
        if a.size:
            setattr(q, k, _ptr(a))
    refl = np.zeros(chains, dtype=np.int32)
    q.reflected = refl.ctypes.data_as(C.POINTER(C.c_int))
    arrays["reflected"] = refl
    return q, arrays


def quantiles_result(q, arrays) -> dict:
    """The "quantiles" dict of gpirtMCMC(quantiles=...) and from_states: probs, theta (len(probs) x n), theta_median,
    theta_mode, theta_hist, theta_rhat (bulk / tail / max), irf (len(probs) x 1001 x m), irf_p_mean, reflected, scalars
    (the entries whose part the states lack are left out)."""
    out = dict(probs=arrays["probs"].copy())
    ren = dict(theta_q="theta", irf_q="irf")
    for k, v in arrays.items():
        if k not in ("probs", "reflected", "theta_rhat_bulk", "theta_rhat_tail", "theta_rhat"):
            out[ren.get(k, k)] = v
    if "theta_rhat" in arrays:
        out["theta_rhat"] = dict(bulk=arrays["theta_rhat_bulk"], tail=arrays["theta_rhat_tail"], max=arrays["theta_rhat"])
    out["reflected"] = arrays["reflected"].astype(bool)
    out["scalars"] = {k: float(q.scalars[i]) for i, k in enumerate(_lib.QNT_SCALARS)}
    return out


def from_states(handle, states, probs, signs=None, align=True) -> dict:
    """gpirt_summary_quantiles over the state blocks `states` (device tensors, or Samplers with summaries on, all on
    handle's device): every output the states' parts allow.  The reflection is chains.combine's for the same arguments."""
    from .chains import state_header
    lib = _lib.load()
    tensors, nc, ptrs = _lib.state_ptrs(states, "summary_state")
    hdr = state_header(tensors[0])
    n, m, parts = hdr["n"], hdr["m"], hdr["parts"]
    th = bool(parts & _lib.SUM_THETA_HIST)
    q, arrays = quantiles_struct(probs, n, m, len(tensors), theta=th, rhat=th and bool(parts & _lib.SUM_DIAG),
                                 irf=bool(parts & _lib.SUM_IRF_BAND))
    sg = (C.c_int * nc)(*[int(x) for x in signs]) if signs is not None else None
    check(lib.gpirt_summary_quantiles(handle.ptr, nc, ptrs, sg, int(bool(align)), C.byref(q)))
    return quantiles_result(q, arrays)


# ------------------------------------------------------------------------------------------------------- NumPy -------
def grid_index(theta):
    """k = rint((theta + 5) 100) where theta is bit for bit -5 + 0.01 k, else -1 (NaN included)."""
    t = np.asarray(theta, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        k = np.rint((t + 5.0) * 100.0)
        on = (k >= 0) & (k <= NGRID - 1) & (-5.0 + k * 0.01 == t)
    return np.where(on, k, -1).astype(np.int64)


def _grid(k):
    return -5.0 + np.asarray(k).astype(np.float64) * 0.01


def _count(k):
    """k (s, n) grid indices (-1: off the grid) -> (1001, n) counts"""
    n = k.shape[1]
    idx = (k * n + np.arange(n)[None, :])[k >= 0]
    return np.bincount(idx, minlength=NGRID * n).reshape(NGRID, n)


def histograms(theta_draws, fstar_draws=None, edges=None) -> dict:
    """Per chain, what the device accumulates, in NumPy: theta_draws (C, S, n), fstar_draws (C, S, 1001, m) or None.
    Returns theta_hist, theta_hist_h1, theta_hist_h2 (C, 1001, n; the halves are DIAG's, draws 1..floor(S/2) and the last
    floor(S/2)), theta_off_grid (C, n) and, with f*, irf_band (C, 256, 1001, m), irf_nan and irf_psum (C, 1001, m)."""
    th = np.asarray(theta_draws, dtype=np.float64)
    C_, S, n = th.shape
    k = grid_index(th)
    hN = S // 2
    out = dict(theta_hist=np.stack([_count(k[c]) for c in range(C_)]),
               theta_hist_h1=np.stack([_count(k[c, :hN]) for c in range(C_)]),
               theta_hist_h2=np.stack([_count(k[c, S - hN:]) for c in range(C_)]),
               theta_off_grid=(k < 0).sum(axis=1))
    if fstar_draws is not None:
        f = np.asarray(fstar_draws, dtype=np.float64)
        e = band_edges() if edges is None else np.asarray(edges, dtype=np.float64)
        cells = int(np.prod(f.shape[2:]))
        band = []
        for c in range(C_):
            x = f[c].reshape(S, cells)
            ok = ~np.isnan(x)
            b = np.searchsorted(e, np.where(ok, x, 0.0), side="right")            # #{e_b <= x}
            idx = (b * cells + np.arange(cells)[None, :])[ok]
            band.append(np.bincount(idx, minlength=BINS * cells).reshape((BINS,) + f.shape[2:]))
        out.update(irf_band=np.stack(band), irf_nan=np.isnan(f).sum(axis=1), irf_psum=plogis(f).sum(axis=1))
    return out


def _rank_rhat_draws(v, S):
    """Rank-normalised split-R-hat of integer-valued draws v (C, S, n): the 2C halves' draws ranked with ties averaged
    (scipy.stats.rankdata), z = ndtri((r - 3/8) / (T' + 1/4)), BDA3 on z."""
    from scipy.special import ndtri
    from scipy.stats import rankdata
    from .chains import _split_rhat
    C_, _, n = v.shape
    hN = S // 2
    if hN < 2:
        return np.full(n, np.nan)
    halves = np.concatenate([v[:, :hN], v[:, S - hN:]], axis=0)                  # (2C, hN, n)
    flat = halves.reshape(2 * C_ * hN, n).astype(np.float64)
    r = rankdata(flat, method="average", axis=0)
    z = ndtri((r - 0.375) / (flat.shape[0] + 0.25)).reshape(halves.shape)
    return _split_rhat(z.mean(axis=1), z.var(axis=1, ddof=1), hN)


def _rhat_max(bulk, tail):
    return dict(bulk=bulk, tail=tail, max=np.where(np.isnan(bulk) | np.isnan(tail), np.nan, np.fmax(bulk, tail)))


def _band_quantiles(band, nanc, pr, T):
    """band (256, ...) pooled counts: for t = q T the first bin with a draw whose cumulative count is >= t, then
    (b + (t - cum_(b-1)) / count_b) / 256; NaN for a cell with a NaN draw."""
    cnt = band.astype(np.float64)
    cum = np.cumsum(cnt, axis=0)
    out = np.full((pr.size,) + band.shape[1:], np.nan)
    for p, q in enumerate(pr):
        t = q * T
        ok = (cnt > 0) & (cum >= t)
        b = ok.argmax(axis=0)
        cb = np.take_along_axis(cnt, b[None], axis=0)[0]
        prev = np.take_along_axis(cum, b[None], axis=0)[0] - cb
        with np.errstate(invalid="ignore", divide="ignore"):
            v = (b.astype(np.float64) + (t - prev) / cb) / float(BINS)
        out[p] = np.where(ok.any(axis=0) & (nanc == 0), v, np.nan)
    return out


def from_draws(theta_draws, fstar_draws, probs, signs=None, edges=None) -> dict:
    """What gpirt_summary_quantiles returns, from stored draws: theta_draws (C, S, n), fstar_draws (C, S, 1001, m) or None;
    signs (C values of +-1) reflect a chain: its grid index k -> 1000 - k, for theta and f*'s grid axis.  The theta
    quantiles are order statistics of the pooled draws; the R-hat is computed on the grid index (the tail's fold
    |2k - (k_lo + k_hi)| in integer half-grid units, so mirror ties are exact); NaN for a respondent with a draw off the
    grid.  irf is the band interpolation, irf_exact the exact ceil(q T)-th smallest plogis(f*)."""
    th = np.asarray(theta_draws, dtype=np.float64)
    C_, S, n = th.shape
    sg = np.ones(C_) if signs is None else np.asarray(signs, dtype=np.float64)
    pr = np.asarray(probs, dtype=np.float64).ravel()
    T = C_ * S
    k0 = grid_index(th)
    bad = (k0 < 0).any(axis=(0, 1))
    k = np.where(k0 < 0, -1, np.where(sg[:, None, None] < 0, NGRID - 1 - k0, k0))
    kf = np.where(bad[None, None, :], 0, k)                                      # off-grid respondents: masked below
    srt = np.sort(kf.reshape(T, n), axis=0)
    rk = ranks(pr, T)
    out = dict(probs=pr.copy())
    out["theta"] = np.where(bad[None, :], np.nan, _grid(srt[rk - 1]))
    out["theta_median"] = np.where(bad, np.nan, _grid(srt[ranks([0.5], T)[0] - 1]))
    hist = _count(k.reshape(T, n))
    out["theta_hist"] = hist.astype(np.float64)
    out["theta_mode"] = np.where(bad, np.nan, _grid(hist.argmax(axis=0)))
    s2 = srt[(T + 1) // 2 - 1] + srt[T // 2]                                      # k_lo + k_hi: R's median, doubled
    bulk = np.where(bad, np.nan, _rank_rhat_draws(kf, S))
    tail = np.where(bad, np.nan, _rank_rhat_draws(np.abs(2 * kf - s2[None, None, :]), S))
    out["theta_rhat"] = _rhat_max(bulk, tail)
    if fstar_draws is not None:
        f = np.asarray(fstar_draws, dtype=np.float64)
        f = np.where(sg[:, None, None, None] < 0, f[:, :, ::-1, :], f)
        p = plogis(f).reshape((T,) + f.shape[2:])
        nanc = np.isnan(f).reshape(p.shape).sum(axis=0)
        out["irf_p_mean"] = p.sum(axis=0) / T
        out["irf_exact"] = np.where(nanc[None] > 0, np.nan, np.sort(p, axis=0)[rk - 1])
        h = histograms(np.zeros((C_, S, 1)), f, edges)
        out["irf"] = _band_quantiles(h["irf_band"].sum(axis=0), nanc, pr, T)
    return out


def _rank_rhat_hist(halves, hN):
    """halves (2C, K, n): counts over an ordered integer variable.  The rank-normalised split-R-hat by the histogram
    algebra: average ranks r_k = cum_(k-1) + (count_k + 1) / 2 of the pooled halves, z_k = Phi^-1((r_k - 3/8) /
    (T' + 1/4)), each half's mean and variance (ddof 1) from its counts, BDA3 on those."""
    from scipy.special import ndtri
    from .chains import _split_rhat
    n = halves.shape[2]
    if hN < 2:
        return np.full(n, np.nan)
    h = halves.astype(np.float64)
    sc = h.sum(axis=0)                                                            # (K, n)
    cum = np.cumsum(sc, axis=0)
    Tp = float(halves.shape[0] * hN)
    r = cum - sc + (sc + 1.0) * 0.5
    z = np.where(sc > 0, ndtri((r - 0.375) / (Tp + 0.25)), 0.0)
    means = (h * z[None]).sum(axis=1) / hN
    var = (h * (z[None] - means[:, None]) ** 2).sum(axis=1) / (hN - 1)
    return _split_rhat(means, var, hN)


def _fold(h, s2):
    """h (M, 1001, n) grid counts -> counts over the folded distance d = 2t + (s2 & 1) (half-grid units) from s2 / 2,
    t = 0..1000: grid points (s2 + d) / 2 and (s2 - d) / 2, one point at d = 0."""
    t = np.arange(NGRID)[:, None]
    kp = (s2[None, :] + 1) // 2 + t
    km = s2[None, :] // 2 - t
    cols = np.arange(h.shape[-1])[None, :]
    up = np.where(kp < NGRID, h[:, np.minimum(kp, NGRID - 1), cols], 0)
    dn = np.where((km >= 0) & (km != kp), h[:, np.maximum(km, 0), cols], 0)
    return up + dn


def from_histograms(*, draws, probs, signs=None, theta_hist=None, theta_hist_h1=None, theta_hist_h2=None,
                    theta_off_grid=None, irf_band=None, irf_nan=None, irf_psum=None) -> dict:
    """What gpirt_summary_quantiles returns, from the per-chain histograms alone (as `histograms` returns them, each
    (C, ...)), `draws` = S per chain.  The halves give the R-hat (None: no R-hat)."""
    pr = np.asarray(probs, dtype=np.float64).ravel()
    C_ = np.asarray(theta_hist if theta_hist is not None else irf_band).shape[0]
    sg = np.ones(C_) if signs is None else np.asarray(signs, dtype=np.float64)
    S = int(draws)
    T = C_ * S
    rk = ranks(pr, T)
    out = dict(probs=pr.copy())

    def refl(h, axis):                                  # chain-wise: the grid axis of a reflected chain reversed
        h = np.asarray(h)
        return np.stack([np.flip(h[c], axis=axis) if sg[c] < 0 else h[c] for c in range(C_)]).astype(np.int64)

    if theta_hist is not None:
        hist = refl(theta_hist, 0).sum(axis=0)                                      # (1001, n)
        bad = np.asarray(theta_off_grid).sum(axis=0) > 0
        cum = np.cumsum(hist, axis=0)

        def order_stat(r):                                                          # the grid point of rank r
            return (cum >= r).argmax(axis=0)

        out["theta"] = np.stack([np.where(bad, np.nan, _grid(order_stat(r))) for r in rk]).reshape(pr.size, -1)
        out["theta_median"] = np.where(bad, np.nan, _grid(order_stat(ranks([0.5], T)[0])))
        out["theta_mode"] = np.where(bad, np.nan, _grid(hist.argmax(axis=0)))
        out["theta_hist"] = hist.astype(np.float64)
        if theta_hist_h1 is not None:
            hN = S // 2
            halves = np.concatenate([refl(theta_hist_h1, 0), refl(theta_hist_h2, 0)])      # (2C, 1001, n)
            bulk = _rank_rhat_hist(halves, hN)
            s2 = order_stat((T + 1) // 2) + order_stat(T // 2 + 1)
            tail = _rank_rhat_hist(_fold(halves, s2), hN)
            out["theta_rhat"] = _rhat_max(np.where(bad, np.nan, bulk), np.where(bad, np.nan, tail))
    if irf_band is not None:
        band = refl(irf_band, 1).sum(axis=0)                                        # (256, 1001, m)
        nanc = refl(irf_nan, 0).sum(axis=0)
        out["irf"] = _band_quantiles(band, nanc, pr, T)
        ps = np.stack([np.flip(irf_psum[c], axis=0) if sg[c] < 0 else irf_psum[c] for c in range(C_)])
        out["irf_p_mean"] = ps.sum(axis=0) / T
    return out
