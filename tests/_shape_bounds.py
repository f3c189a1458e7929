"""Bounds for comparing the device's shape accumulators with gpirt_amd.shape.from_draws, derived from each case's curves.

The integers (cls, the four histograms, cross_count, draws, nonfinite, info_draws, info_skipped) are compared bit for bit:
every decision behind them is an fp64 comparison of max / min / one subtraction on the same g.  The doubles differ by rounding
alone, and the bounds come from the operation counts and the precision of the format (EPS = 2^-52 = 1 ulp relative), never
from what the device gives.  First order, each count rounded up:
  slope sums  max d / 0.01 and its square are the same correctly rounded operations on both sides and are added in draw order on
              both: only a different association could differ, S EPS of the sum of the absolute terms
  I[k, j]     e = exp(-|g|) within 2 ulp: 2 EPS; 1 + e: 1.5 EPS (e / (1 + e) <= 1/2); its square 3.5;
              e / (1 + e)^2: 6; g' = one subtraction and one division: 1, g'^2: 2.5; the product: 9 EPS.  The reference runs in
              long double (2^-64 per operation) and is rounded to fp64 once: 0.5.  With slack for the second order: 11 EPS I,
              plus 8 denormal steps times (g'^2 + 1) where e itself is denormal (|g| > 708)
  info_sum    the draws' bounds added, plus S EPS of the sum for the S additions                    -> (11 + S) EPS sum I
  TI[k]       m additions in ascending j: (11 + m) EPS TI;  ti_sum: (11 + m + S) EPS sum TI;
              ti_sumsq: TI^2 is 2 (11 + m) + 1, so (23 + 2 m + S) EPS sum TI^2
  w_k         theta^2 rounded once (an absolute 12.5 EPS, 6.25 after the exact halving), the host's exp 1 ulp: 7.25 EPS; the sum
              of 1001 positive terms 500.5 more, the division 0.5 and w's own 7.25: 520 EPS
  rho         TI / (TI + 1): 2 (11 + m) + 1; times w: 520.5; the 1001 terms added in any order: 501  -> (1050 + 2 m) EPS rho
  rel         sum rho: (1050 + 2 m + S) EPS; sum rho^2: (2101 + 4 m + S) EPS
"""
import numpy as np

from gpirt_amd import shape as SH

EPS = float(np.finfo(np.float64).eps)
TINY = 8.0 * 2.0 ** -1074
INT_KEYS = ("cls", "peak_hist", "valley_hist", "cross_first_hist", "cross_last_hist", "cross_count", "draws", "nonfinite",
            "info_draws", "info_skipped")
DOUBLE_KEYS = ("slope", "info_sum", "ti_sum", "ti_sumsq", "rel")


def bounds(curves, window):
    """name -> bound array (gpirt_amd.shape's layout) for one chain's curves (S x 1001 x m)"""
    curves = np.asarray(curves, dtype=np.float64)
    S, N, m = curves.shape
    k_half = SH.check_window(window)
    k_lo, k_hi = SH.CENTRE - k_half, SH.CENTRE + k_half
    slope_abs = np.zeros((4, m))
    info = np.zeros((N, m), dtype=np.longdouble)
    tiny = np.zeros((N, m))
    ti = np.zeros(N, dtype=np.longdouble)
    ti2 = np.zeros(N, dtype=np.longdouble)
    rho1 = rho2 = np.longdouble(0)
    w = SH.grid_weights()
    for g in curves:
        ok = np.isfinite(g).all(axis=0)
        cols = np.flatnonzero(ok)
        if cols.size:
            d = np.diff(g[k_lo:k_hi + 1][:, cols], axis=0)
            smax, smin = np.abs(d.max(axis=0) / 0.01), np.abs(d.min(axis=0) / 0.01)
            slope_abs[:, cols] += np.stack([smax, smax * smax, smin, smin * smin])
            I = SH.draw_info(g[:, cols])
            info[:, cols] += I
            gp = np.gradient(g[:, cols], 0.01, axis=0)
            tiny[:, cols] += TINY * (gp * gp + 1.0)
        if ok.all():
            TI = I.sum(axis=1)
            ti += TI
            ti2 += TI * TI
            rho = (w * (TI / (TI + 1))).sum()
            rho1, rho2 = rho1 + rho, rho2 + rho * rho
    f = lambda x: np.asarray(x, dtype=np.float64)                      # noqa: E731
    return dict(slope=S * EPS * slope_abs, info_sum=(11 + S) * EPS * f(info) + tiny,
                ti_sum=(11 + m + S) * EPS * f(ti) + tiny.sum(axis=1), ti_sumsq=(23 + 2 * m + S) * EPS * f(ti2) + tiny.sum(axis=1),
                rel=np.array([(1050 + 2 * m + S) * EPS * float(rho1), (2101 + 4 * m + S) * EPS * float(rho2)]))


def check(got, want, curves=None, window=None, label=""):
    """got: the device's dict (Sampler.shape() / shape.combine / gpirtMCMC's "shape"); want: from_draws over the same curves.
    The integers bit for bit; with `curves` (one chain) the doubles within bounds(curves, window), observed / bound printed."""
    for k in INT_KEYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and np.array_equal(a, b), (label, k, int((a != b).sum()) if a.shape == b.shape else "shape")
    if curves is None:
        return
    bd = bounds(curves, window)
    for k in DOUBLE_KEYS:
        a, b = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        assert a.shape == b.shape == bd[k].shape, (label, k)
        assert np.isfinite(a).all(), (label, k, "non-finite")
        gap = np.abs(a - b)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = float(np.max(np.where(bd[k] > 0, gap / bd[k], np.where(gap > 0, np.inf, 0.0))))
        print(f"MEASURED {label} {k}: observed / bound = {ratio:.3g} (largest gap {float(gap.max()):.3e}, "
              f"largest bound {float(bd[k].max()):.3e})")
        assert (gap <= bd[k]).all(), f"{label} {k}: observed / bound = {ratio:.3g}"
