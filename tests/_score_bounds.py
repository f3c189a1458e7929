"""Bounds for comparing the device's scores of new respondents with gpirt_amd.score.from_draws, derived from the inputs.

Every term -log(1 + exp(.)) is <= 0, so sum_j |term_kj| = |T[k, r]| and
    delta = 2 m eps max_{k, r} |T[k, r]|
bounds both product forms against the exact sum of the fp64 terms: the fixed-point form rounds each term once to 2^-54 of
its row's range (m 2^-54 range in all), the fp64 GEMM commits at most m eps sum |terms|.  A term the product holds at
-1e300 (the formula as written overflowed) is left out of the maximum: it is the same constant on both sides, and whatever
is added to it is absorbed identically (|x| < 1e284 vanishes in fp64), so it contributes no difference -- leaving it in
would only make the bound vacuous.

With rho = 2 delta + 2 * 1001 * eps (two log-posteriors enter a weight: lp[k] and the normaliser; 1001 eps for the exp,
the sum over the grid and the division, twice for the two sides):
  grid_post                |got - want| <= rho want + 1e-300
  lpd, loglik_mean         |got - want| <= delta + 2 * 1001 eps (1 + |want|)
  theta_mean               sum_k |theta_k| |d grid_post[k]| + the sum's own rounding <= (rho + 1001 eps) sum_k |theta_k| want[k]
  theta_sd                 var = sum (theta_k - mean)^2 g[k]:  d var <= (rho + 1001 eps) var + 2 d mean sum |theta_k - mean| g[k]
                           + d mean^2, and |sqrt(a) - sqrt(b)| <= sqrt(var + d var) - sqrt(max(var - d var, 0)) (+ 4 eps sd)
  theta_quantiles          compared where no cumulative sum of the reference is within rho cum + 1001 eps of q
  theta_map                compared where the runner-up is further than rho top below the top
"""
import numpy as np

EPS = np.finfo(np.float64).eps
N = 1001
HELD_FROM = 1e299


def delta_of(products, m):
    """delta from the reference's products (a list of (1001, n_new) arrays), non-finite and held entries left out"""
    big = 0.0
    for T in products:
        a = np.abs(T[np.isfinite(T)])
        a = a[a < HELD_FROM]
        if a.size:
            big = max(big, float(a.max()))
    return 2.0 * m * EPS * big


def compare(got, want, delta, label=""):
    """Asserts every bound above; prints MEASURED with the largest gap of each kind.  Returns the share of quantile cells
    left out."""
    rho = 2.0 * delta + 2.0 * N * EPS
    th = -5.0 + np.arange(N) * 0.01
    ints_equal = all(np.array_equal(got[k], want[k]) for k in ("draws", "nonfinite", "n_obs"))
    live = want["draws"] > 0
    for k in ("grid_post", "theta_mean", "theta_sd", "theta_map", "lpd", "loglik_mean"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), f"{label} {k}: NaN pattern"
    g, w = got["grid_post"][live], want["grid_post"][live]
    gap_post = np.abs(g - w)
    tol_post = rho * w + 1e-300
    rel_post = float((gap_post / (w + 1e-300)).max()) if live.any() else 0.0
    gaps = {}
    for k in ("lpd", "loglik_mean"):
        d = np.abs(got[k][live] - want[k][live])
        gaps[k] = float(d.max()) if live.any() else 0.0
        tol = delta + 2.0 * N * EPS * (1.0 + np.abs(want[k][live]))
    mean_w = want["theta_mean"][live]
    tol_mean = (rho + N * EPS) * (np.abs(th)[None, :] * w).sum(axis=1) + 4.0 * EPS
    gap_mean = np.abs(got["theta_mean"][live] - mean_w)
    var_w = ((th[None, :] - mean_w[:, None]) ** 2 * w).sum(axis=1)
    dvar = (rho + N * EPS) * var_w + 2.0 * tol_mean * (np.abs(th[None, :] - mean_w[:, None]) * w).sum(axis=1) + tol_mean ** 2
    tol_sd = np.sqrt(var_w + dvar) - np.sqrt(np.maximum(var_w - dvar, 0.0)) + 4.0 * EPS * np.sqrt(var_w)
    gap_sd = np.abs(got["theta_sd"][live] - want["theta_sd"][live])
    # quantiles: only where the reference's cumulative sum is clear of q
    cum = np.cumsum(w, axis=1)
    probs = np.asarray(want["probs"])
    left_out = total = wrong_q = 0
    for p, q in enumerate(probs):
        clear = (np.abs(cum - q) > rho * cum + N * EPS).all(axis=1)
        total += clear.size
        left_out += int((~clear).sum())
        wrong_q += int((got["theta_quantiles"][p][live][clear] != want["theta_quantiles"][p][live][clear]).sum())
    share = left_out / max(total, 1)
    srt = np.sort(w, axis=1)
    clear_map = srt[:, -1] - srt[:, -2] > rho * srt[:, -1]
    wrong_map = int((got["theta_map"][live][clear_map] != want["theta_map"][live][clear_map]).sum())
    print(f"MEASURED {label}: delta {delta:.3e} rho {rho:.3e}; grid_post rel gap {rel_post:.3e}; lpd gap {gaps['lpd']:.3e}; "
          f"loglik_mean gap {gaps['loglik_mean']:.3e}; theta_mean gap {float(gap_mean.max()) if live.any() else 0.0:.3e}; "
          f"theta_sd gap {float(gap_sd.max()) if live.any() else 0.0:.3e}; quantile cells left out {left_out}/{total}, "
          f"wrong {wrong_q}; map wrong {wrong_map}; integers bit-equal {ints_equal}")
    assert ints_equal, f"{label}: draws / nonfinite / n_obs differ"
    assert (gap_post <= tol_post).all(), f"{label} grid_post: rel gap {rel_post:.3e} > rho {rho:.3e}"
    for k in ("lpd", "loglik_mean"):
        d = np.abs(got[k][live] - want[k][live])
        tol = delta + 2.0 * N * EPS * (1.0 + np.abs(want[k][live]))
        assert (d <= tol).all(), f"{label} {k}: gap {float(d.max()):.3e}"
    assert (gap_mean <= tol_mean).all(), f"{label} theta_mean: gap {float(gap_mean.max()):.3e}"
    assert (gap_sd <= tol_sd).all(), f"{label} theta_sd: gap {float(gap_sd.max()):.3e}"
    assert wrong_q == 0 and wrong_map == 0, f"{label}: {wrong_q} quantiles / {wrong_map} maps differ where the reference is clear"
    assert share <= 0.01, f"{label}: {share:.3%} of the quantile cells are too close to q to compare"
    return share
