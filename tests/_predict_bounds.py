"""Bounds for comparing the device's predictions for new respondents with gpirt_amd.score.predict_from_draws, derived from
each case's inputs in the manner of tests/_score_bounds.py.

With delta and rho as _score_bounds defines them from the reference's products (rho bounds a weight's relative error on
both sides together), let
    c = rho + 3 * 1001 * eps
(1001 eps each for the cell function P or H, the contraction over the grid, and the other side's same two).  Every term of
q = sum_k w_k P[k, j] and Hbar = sum_k w_k H[k, j] is >= 0, so both carry the relative error c:
  p_yes        |got - want| <= c want + 1e-300
  info         g = h(q) - Hbar with h'(q) = log((1 - q) / q):  |d g| <= c (h(q) + Hbar + q |log((1 - q) / q)|) per draw; the
               bound is that expression averaged over the counted draws, plus 8 eps for the sum and the division
  next_items   compared only for respondents whose compared ranks -- the reference's first top + 1 unanswered items, so the
               cut after the list is covered too -- are separated by more than twice the largest info bound among them;
               the share of respondents left out is capped at 1 % (callers of constructed ties switch the cap off)
  integers     pred_draws and pred_skipped must be equal
"""
import numpy as np

from _score_bounds import EPS, N, delta_of

from gpirt_amd import score as SC


def delta_from(want, m):
    """delta over every chain's per-draw products of a predict_from_draws(..., return_draws=True) result"""
    return max([delta_of(p, m) for p in want["products"] if p] + [0.0])


def info_bound(want, c):
    """(n_new, m): c times the per-draw expression averaged over the counted draws, plus 8 eps"""
    tot, cnt = 0.0, 0
    for qs, hs in zip(want["q"], want["Hbar"]):
        for q, hbar in zip(qs, hs):
            with np.errstate(divide="ignore", invalid="ignore"):
                slope = np.where((q > 0.0) & (q < 1.0), q * np.abs(np.log((1.0 - q) / q)), np.where(q >= 1.0, np.inf, 0.0))
            tot = tot + SC.binary_entropy(q) + hbar + slope
            cnt += 1
    return c * tot / max(cnt, 1) + 8.0 * EPS


def compare(got, want, delta, y_new, label="", cap=True):
    """Asserts every bound above; prints MEASURED with the largest gap of each kind.  want: predict_from_draws(...,
    return_draws=True).  Returns the share of respondents whose next_items were left out."""
    rho = 2.0 * delta + 2.0 * N * EPS
    c = rho + 3.0 * N * EPS
    y = np.asarray(y_new, dtype=np.float64)
    ints_equal = got["pred_draws"] == want["pred_draws"] and got["pred_skipped"] == want["pred_skipped"]
    for k in ("p_yes", "info", "next_info"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), f"{label} {k}: NaN pattern"
    top = want["next_items"].shape[1]
    assert got["next_items"].shape == want["next_items"].shape
    if want["pred_draws"] == 0:
        print(f"MEASURED {label}: no counted draw; integers bit-equal {ints_equal}")
        assert ints_equal and (got["next_items"] == -1).all()
        return 0.0
    gap_p = np.abs(got["p_yes"] - want["p_yes"])
    tol_p = c * want["p_yes"] + 1e-300
    tol_i = info_bound(want, c)
    gap_i = np.abs(got["info"] - want["info"])
    finite = np.isfinite(tol_i)
    left_out = wrong = 0
    min_gap = np.inf
    for r in range(y.shape[0]):
        cand = np.flatnonzero(np.isnan(y[r]))
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
    share = left_out / y.shape[0]
    rel_p = float((gap_p / (want["p_yes"] + 1e-300)).max())
    print(f"MEASURED {label}: delta {delta:.3e} c {c:.3e}; p_yes rel gap {rel_p:.3e}; info gap {float(gap_i[finite].max()):.3e} "
          f"(bound {float(tol_i[finite].min()):.3e} .. {float(tol_i[finite].max()):.3e}); next_items left out {left_out}/"
          f"{y.shape[0]}, wrong {wrong}, smallest compared-rank gap {min_gap:.3e}; integers bit-equal {ints_equal}")
    assert ints_equal, f"{label}: pred_draws / pred_skipped differ"
    assert (gap_p <= tol_p).all(), f"{label} p_yes: rel gap {rel_p:.3e} > c {c:.3e}"
    assert (gap_i <= tol_i).all(), f"{label} info: gap {float((gap_i - tol_i).max()):.3e} beyond the bound"
    assert wrong == 0, f"{label}: next_items / next_info of {wrong} respondents differ where the reference is clear"
    if cap:
        assert share <= 0.01, f"{label}: {share:.3%} of the respondents have compared ranks too close to compare"
    return share
