"""Bounds for comparing the device's theta-binned item fit with gpirt_amd.ppc.bins_from_rep, derived from the inputs.

The integers (bins, N, T, R, every count) are compared bit for bit.  The doubles differ by rounding alone, and the bounds come
from the precision of the format (gpirt_amd.ppc.bins_bounds), never from what the device gives:
  p, q        exp within 1 ulp, 1 + e and the division rounded once each: within 4 eps of the true value, so the device's
              and NumPy's within 8 eps of each other; p q within 20 eps
  E, V        a sum of N positive terms in any fixed order: N eps of the sum on top     ->  dE = (8 + N) eps E, dV = (20 + N) eps V
  z, X2 term  (C - E) / sqrt(V) and (C - E)^2 / V through d(C - E) = dE + eps |C - E|, first order, 1 % on top
  X2          the bins' bounds added, plus B eps X2 for the sum over the bins
  sums over the draws   the draws' bounds added, plus (S + 1) eps of the sum of the absolute terms
The reference sums E, V and X2 in np.longdouble, whose own error (2^-64 per operation) is far below every bound above.
A chi-square decision is compared only through the reference's bracket: an (item, draw) is undecided when |X2(R) - X2(T)| is
at most the sum of the two bounds; an integer tie is decided."""
import numpy as np

from gpirt_amd import ppc as P

INT_KEYS = ("sum_n", "sum_t", "sum_r", "cell_ge", "cell_gt", "cell_empty", "occ_sum")
DOUBLE_KEYS = ("sum_e", "sum_z", "chi_obs_sum", "chi_rep_sum")
MAX_UNDECIDED = 0.01


def check_tables(got, last, label=""):
    """got: the device's bin, tN, tT, tR, tE, tV of one draw; last: bins_from_rep(...)["last"] of that draw alone"""
    for k in ("bin", "tN", "tT", "tR"):
        assert got[k].dtype == last[k].dtype and np.array_equal(got[k], last[k]), (label, k)
    gE, gV = np.abs(got["tE"] - last["tE"]), np.abs(got["tV"] - last["tV"])
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"MEASURED {label}: tE gap / bound {np.nanmax(np.where(last['dE'] > 0, gE / last['dE'], 0.0)):.3f} "
              f"(bound up to {last['dE'].max():.2e}), tV gap / bound {np.nanmax(np.where(last['dV'] > 0, gV / last['dV'], 0.0)):.3f}")
    assert (gE <= last["dE"]).all(), (label, "tE", float(gE.max()))
    assert (gV <= last["dV"]).all(), (label, "tV", float(gV.max()))
    empty = last["tN"] == 0
    assert not got["tE"][empty].any() and not got["tV"][empty].any()


def check_accumulators(got, want, label=""):
    """got: bins_result's dict from the device; want: bins_from_rep's over the same draws"""
    for k in INT_KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (label, k)
    for k in ("n", "m", "B", "bin_draws", "bin_skipped"):
        assert got[k] == want[k], (label, k)
    assert np.array_equal(got["cuts"], want["cuts"])
    share = want["undecided"] / max(want["decisions"], 1)
    worst = {}
    for k in DOUBLE_KEYS:
        gap = np.abs(got[k] - want[k])
        with np.errstate(invalid="ignore", divide="ignore"):
            worst[k] = float(np.nanmax(np.where(want["bounds"][k] > 0, gap / want["bounds"][k], 0.0))) if gap.size else 0.0
    inside = {k: bool(((want[k][0] <= got[k]) & (got[k] <= want[k][1])).all()) for k in ("chi_ge", "chi_gt")}
    print(f"MEASURED {label}: undecided {want['undecided']}/{want['decisions']}; gap / bound " +
          ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f"; brackets hold {inside}")
    assert share <= MAX_UNDECIDED, f"{label}: {share:.3%} of the chi-square decisions are undecided on the reference"
    for k in DOUBLE_KEYS:
        assert (np.abs(got[k] - want[k]) <= want["bounds"][k]).all(), (label, k, worst[k])
    for k in ("chi_ge", "chi_gt"):
        assert got[k].dtype == np.uint32 and inside[k], (label, k)
    # the finished arrays are the header's quotients of the device's own raw arrays, bit for bit
    S = got["bin_draws"]
    with np.errstate(invalid="ignore", divide="ignore"):
        sN = np.where(got["sum_n"] > 0, got["sum_n"], np.nan).astype(np.float64)
        Sc = S - got["cell_empty"].astype(np.int64)
        Sc = np.where(Sc > 0, Sc, np.nan).astype(np.float64)
        Sd = float(S) if S > 0 else np.nan
        fin = dict(obs_rate=got["sum_t"] / sN, rep_rate=got["sum_r"] / sN, exp_rate=got["sum_e"] / sN, z_mean=got["sum_z"] / Sc,
                   ppp_cell=got["cell_ge"] / Sc, ppp_cell_mid=(got["cell_ge"].astype(np.float64) + got["cell_gt"]) / (2.0 * Sc),
                   n_mean=got["sum_n"] / Sd, ppp_chi2=got["chi_ge"] / Sd,
                   ppp_chi2_mid=(got["chi_ge"].astype(np.float64) + got["chi_gt"]) / (2.0 * Sd),
                   chi2_obs_mean=got["chi_obs_sum"] / Sd, chi2_rep_mean=got["chi_rep_sum"] / Sd, occupancy=got["occ_sum"] / Sd)
    for k, v in fin.items():
        assert np.array_equal(got[k], v, equal_nan=True), (label, k)
    assert np.array_equal(got["bin_lo"], want["bin_lo"]) and np.array_equal(got["bin_hi"], want["bin_hi"])
    w = P.bins_worst(got["ppp_chi2_mid"], got["chi2_obs_mean"], len(got["worst"]["items"]))
    for k in ("items", "ppp_chi2_mid", "chi2_obs_mean"):
        assert np.array_equal(got["worst"][k], w[k], equal_nan=True), (label, "worst", k)


def same_result(a, b, label=""):
    """two device results bit for bit"""
    for k in INT_KEYS + DOUBLE_KEYS + ("chi_ge", "chi_gt", "obs_rate", "z_mean", "ppp_chi2_mid", "occupancy", "cuts"):
        assert np.array_equal(a[k], b[k], equal_nan=True), (label, k)
    for k in ("n", "m", "B", "bin_draws", "bin_skipped"):
        assert a[k] == b[k], (label, k)
    for k in ("items", "ppp_chi2_mid", "chi2_obs_mean"):
        assert np.array_equal(a["worst"][k], b["worst"][k], equal_nan=True), (label, "worst", k)
