"""Bounds for comparing the device's scores and category predictions of new respondents under ordinal responses
(csrc/ordinal_score.hip) with gpirt_amd.ordinal.score_from_draws / predict_from_draws, and the cases the tests share.  Nothing here
comes from what the device returns.

The product.  _score_bounds' scalar delta = 2 m eps max|T| is replaced by the per-entry bound of the one-hot fp64 product,
_ordinal_bounds.theta_bound(cat_new, fstar, B) (the term's 4 u v + u |a| and the GEMM's (K + 2) u sum |terms| at K = C m, doubled);
_score_bounds.compare takes one number, so delta is that bound's largest entry over the draws.  Entries the table holds at -1e300
and non-finite ones are left out, as _score_bounds.delta_of leaves them out: the same constant on both sides.

The w term.  Wc[r] is a sum of at most m values log1p(-exp(-d)), each within 4 u of its magnitude (the device's exp and log1p, 2
ulp each), summed in ascending j: 4 u |Wc| + m u |Wc| (every w is <= 0, so sum |w| = |Wc|).  It enters l alone; compare's one
delta carries it too, which widens the grid's bound by a part in 10^3 of delta.

Downstream everything follows _score_bounds.compare.  For the predictions _predict_bounds.compare is restated for C categories:
    c = rho + (C + 2) * 1001 * eps
(1001 eps each for the C category functions and the entropy table, the contraction, and the other side's), every term of
q_c = sum_k w_k P_c[k, j] and Hbar = sum_k w_k Hc[k, j] is >= 0, so
  probs        |got - want| <= c want + 1e-300
  info         |d info| <= c (h(q) + Hbar + sum_c q_c |1 + log q_c|) per draw (dh / dq_c = -(1 + log q_c): the slope term summed
               over the categories), averaged over the counted draws, plus 8 eps
  expected     sum_c c |d probs_c| + C eps
  next_items   compared only for respondents whose compared ranks (the reference's first top + 1 unanswered items) are separated by
               more than twice the largest info bound among them; the share left out is capped at 1 % of the respondents, or at
               one respondent where n_new < 100
  integers     pred_draws and pred_skipped equal
"""
import numpy as np

import _ordinal_bounds as OB
from _score_bounds import EPS, N, compare as score_compare

from gpirt_amd import ordinal as OR

U = OB.U
HELD_FROM = 1e299


def delta_of(cat_new, fstar_draws, B_draws, products, wcs):
    """delta over one chain's draws: the largest finite entry of theta_bound where the product is finite and not held, plus the
    largest w-term bound"""
    cat = np.asarray(cat_new)
    m = cat.shape[1]
    big = 0.0
    for f, B, T, wc in zip(fstar_draws, B_draws, products, wcs):
        with np.errstate(invalid="ignore", over="ignore"):
            b = np.asarray(OB.theta_bound(cat, f, B), dtype=np.float64)
        ok = np.isfinite(T) & (np.abs(T) < HELD_FROM) & np.isfinite(b)
        if ok.any():
            big = max(big, float(b[ok].max()))
    wmax = max([float(np.abs(wc).max()) for wc in wcs] + [0.0])
    return big + (4.0 + m) * U * wmax


def compare_score(got, want, delta, label=""):
    return score_compare(got, want, delta, label)


def info_bound(want, c):
    tot, cnt = 0.0, 0
    for qs, hs in zip(want["q"], want["Hbar"]):
        for q, hbar in zip(qs, hs):
            with np.errstate(divide="ignore", invalid="ignore"):
                slope = np.where(q > 0.0, q * np.abs(1.0 + np.log(np.where(q > 0.0, q, 1.0))), 0.0).sum(axis=0)
            tot = tot + OR.category_entropy(q) + hbar + slope
            cnt += 1
    return c * tot / max(cnt, 1) + 8.0 * EPS


def compare_predict(got, want, delta, cat_new, label="", cap=True):
    """Asserts every bound above; prints MEASURED.  want: predict_from_draws(..., return_draws=True).  Returns (respondents left
    out, smallest compared-rank gap, largest info bound)."""
    cat = np.asarray(cat_new)
    n, m = cat.shape
    C = want["probs"].shape[2]
    rho = 2.0 * delta + 2.0 * N * EPS
    c = rho + (C + 2.0) * N * EPS
    ints_equal = got["pred_draws"] == want["pred_draws"] and got["pred_skipped"] == want["pred_skipped"]
    for k in ("probs", "info", "expected", "next_info"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), f"{label} {k}: NaN pattern"
    top = want["next_items"].shape[1]
    assert got["next_items"].shape == want["next_items"].shape
    if want["pred_draws"] == 0:
        assert ints_equal and (got["next_items"] == -1).all()
        return 0, np.inf, 0.0
    gap_p = np.abs(got["probs"] - want["probs"])
    tol_p = c * want["probs"] + 1e-300
    tol_e = (np.arange(1, C + 1)[None, None, :] * tol_p).sum(axis=2) + C * EPS
    gap_e = np.abs(got["expected"] - want["expected"])
    tol_i = info_bound(want, c)
    gap_i = np.abs(got["info"] - want["info"])
    left_out = wrong = 0
    min_gap = np.inf
    for r in range(n):
        cand = np.flatnonzero(cat[r] == 0)
        order = cand[np.argsort(-want["info"][r, cand], kind="stable")][:top + 1]
        if order.size >= 2:
            gaps = -np.diff(want["info"][r, order])
            min_gap = min(min_gap, float(gaps.min()))
            if not (gaps > 2.0 * tol_i[r, order].max()).all():
                left_out += 1
                continue
        ok = np.array_equal(got["next_items"][r], want["next_items"][r])
        k = min(order.size, top)
        ok = ok and (np.abs(got["next_info"][r, :k] - want["next_info"][r, :k]) <= tol_i[r, order[:k]]).all()
        wrong += 0 if ok else 1
    rel_p = float((gap_p / (want["probs"] + 1e-300)).max())
    print(f"MEASURED {label}: delta {delta:.3e} c {c:.3e}; probs rel gap {rel_p:.3e}; info gap {float(gap_i.max()):.3e} (bound "
          f"{float(tol_i.min()):.3e} .. {float(tol_i.max()):.3e}); expected gap {float(gap_e.max()):.3e}; next_items left out {left_out}/{n}, "
          f"wrong {wrong}, smallest compared-rank gap {min_gap:.3e}; integers bit-equal {ints_equal}")
    assert ints_equal, f"{label}: pred_draws / pred_skipped differ"
    assert (gap_p <= tol_p).all(), f"{label} probs: rel gap {rel_p:.3e} > c {c:.3e}"
    assert (gap_i <= tol_i).all(), f"{label} info: gap {float((gap_i - tol_i).max()):.3e} beyond the bound"
    assert (gap_e <= tol_e).all(), f"{label} expected"
    assert wrong == 0, f"{label}: next_items / next_info of {wrong} respondents differ where the reference is clear"
    if cap:
        allowed = 1 if n < 100 else int(0.01 * n)
        assert left_out <= allowed, f"{label}: {left_out} of {n} respondents have compared ranks too close to compare"
    return left_out, min_gap, float(tol_i.max())


# ---------------------------------------------------------------------------------------------------- the cases ------
def make_new(n_new, m, C, seed, na=0.3):
    """cat_new (n_new x m int8): about `na` missing, respondent 0 answers category 1 alone and (n_new > 2) respondent 1 category C
    alone (no w term), the LAST respondent has no answers."""
    rng = np.random.default_rng(seed + 31)
    cat = rng.integers(1, C + 1, size=(n_new, m)).astype(np.int8)
    cat[rng.random((n_new, m)) < na] = 0
    if n_new > 2:
        cat[0] = np.where(cat[0] > 0, 1, 0)
        cat[1] = np.where(cat[1] > 0, C, 0)
    cat[n_new - 1] = 0
    return np.asfortranarray(cat)
