"""Bounds for comparing the device's sum-score accumulators (csrc/sumscore.hip) with gpirt_amd.sumscore.from_draws, counted
from the operations of the header's statement -- never from what the device gives.  eps = 2^-52; one rounding is eps / 2.

  p, q        exp within 1 ulp (eps), the sum 1 + e (eps / 2 on a sum whose terms are positive, the error of e not magnified:
              e / (1 + e) <= 1) and the division (eps / 2): C_PQ = 2 eps, taken as 2.5 for the second-order terms.
  one step    A[s] <- A[s] q + A[s - 1] p: every term carries its factor's error (C_PQ), one product (eps / 2) and one sum
              (eps / 2) further: C_STEP = C_PQ + 1 = 3.5 eps a step, and nothing cancels (every term is >= 0).
  A           every term of A[k, s] went through M steps: relative C_STEP M eps, plus the floor (M + 1) 2^-1021 for what went
              through a subnormal on the way (the header says why that is all).
  joint_sum   w_k A (eps / 2) and D additions of positive numbers (at most D eps / 2, taken as D eps), the floor D times.
  pi          1001 products and 1001 additions of positive numbers: (1 + 1001) eps / 2 more than A; pi_sum adds D eps,
              pi_sumsq squares (twice the relative error, one product) and adds.
  T, V        T = sum p: C_PQ + M / 2; V = sum p q: 2 C_PQ + 1 / 2 + M / 2; their sums over draws add D eps, the squares double.
  rho         a = sum w V, b = sum w (V + T T), c = sum w T each with its terms' error and (1 + 1001) eps / 2 of its own; the
              denominator b - c c CANCELS, so its absolute error is carried as such and rho's bound is worked out per draw
              from the reference's (a, b, c); a draw whose denominator is not clear of its own error has no bound (inf).
Every relative bound gets one eps more for the reference's own rounding to float64, and the factor SLACK = 1.01 for what is
of second order in M eps (M <= 4096: M eps < 1e-12).
"""
import numpy as np

EPS = 2.0 ** -52
FLOOR = 2.0 ** -1021
C_PQ = 2.5
C_STEP = C_PQ + 1.0
SLACK = 1.01
N = 1001
SUM_KEYS = ("joint_sum", "pi_sum", "pi_sumsq", "tcc_sum", "tcc_sumsq", "var_sum", "last", "last_pi")


def rel_A(M):
    return SLACK * C_STEP * M * EPS + EPS


def bounds(want, D=None):
    """per-cell bounds for the raw arrays of `want` (from_draws' dict; D counted draws)"""
    M = int(want["M"])
    D = int(want["draws"]) if D is None else D
    rA = rel_A(M)
    fl = (M + 1) * FLOOR
    r_pi = rA + SLACK * (1 + N) * 0.5 * EPS
    r_T = SLACK * (C_PQ + 0.5 * M) * EPS + EPS
    r_V = SLACK * (2 * C_PQ + 0.5 + 0.5 * M) * EPS + EPS
    b = dict(last=rA * want["last"] + fl, last_pi=r_pi * want["last_pi"] + fl,
             joint_sum=(rA + (0.5 + D) * EPS) * want["joint_sum"] + D * fl,
             pi_sum=(r_pi + D * EPS) * want["pi_sum"] + D * fl,
             pi_sumsq=(2 * r_pi + (1 + D) * EPS) * want["pi_sumsq"] + 2 * D * fl,
             tcc_sum=(r_T + D * EPS) * want["tcc_sum"] + D * fl,
             tcc_sumsq=(2 * r_T + (1 + D) * EPS) * want["tcc_sumsq"] + 2 * D * fl,
             var_sum=(r_V + D * EPS) * want["var_sum"] + D * fl)
    # the reliability, per draw
    own = SLACK * (1 + N) * 0.5 * EPS
    e_a, e_b, e_c = r_V + own, max(r_V, 2 * r_T + 0.5 * EPS) + 0.5 * EPS + own, r_T + own
    d0 = d1 = 0.0
    s0 = s1 = 0.0
    for a, bb, c in np.asarray(want.get("rel_terms", np.empty((0, 3)))).reshape(-1, 3):
        den = bb - c * c
        dden = e_b * bb + (2 * e_c + 0.5 * EPS) * c * c + 0.5 * EPS * abs(den)
        if not den > 2.0 * dden:
            d0 = d1 = np.inf
            break
        ratio = a / den
        drho = SLACK * ratio * (e_a + dden / (den - dden) + 0.5 * EPS) + 0.5 * EPS * max(1.0, abs(1.0 - ratio))
        rho = 1.0 - ratio
        d0 += drho
        d1 += 2 * abs(rho) * drho + drho * drho + 0.5 * EPS * rho * rho
        s0 += abs(rho)
        s1 += rho * rho
    b["rel"] = np.array([d0 + D * EPS * s0, d1 + D * EPS * s1])
    return b


def check(got, want, label="", D=None, need_rel=True):
    """Asserts every bound; prints MEASURED with the largest share of its bound that each array used.  Returns that share over
    all arrays.  The reliability's sums and counters are compared whenever every draw's denominator is clear of its own error;
    a case in which one is not must say so (need_rel=False), else it fails: no case passes without them by accident."""
    bd = bounds(want, D)
    assert np.isfinite(bd["rel"]).all() or not need_rel, f"{label}: a draw's denominator is not clear of its error: rel cannot be compared"
    assert np.array_equal(got["mask"], want["mask"]) and np.array_equal(got["w"], want["w"]), f"{label}: mask or w differ"
    for k in ("draws", "skipped", "M"):
        assert got[k] == want[k], f"{label} {k}: {got[k]} != {want[k]}"
    shares = {}
    keys = SUM_KEYS + (("rel",) if np.isfinite(bd["rel"]).all() else ())
    if "rel" in keys:
        assert (got["rel_draws"], got["rel_skipped"]) == (want["rel_draws"], want["rel_skipped"]), f"{label}: rel counters"
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and not np.isnan(g).any(), f"{label} {k}: shape or NaN"
        gap = np.abs(g - w)
        with np.errstate(invalid="ignore", divide="ignore"):
            share = np.where(gap > 0, gap / bd[k], 0.0)
        shares[k] = float(share.max())
    print(f"MEASURED {label}: M {want['M']} draws {want['draws']}; share of the bound used: " +
          ", ".join(f"{k} {v:.3f}" for k, v in shares.items()) + ("" if "rel" in keys else "; rel not comparable (denominator)"))
    for k, v in shares.items():
        assert v <= 1.0, f"{label} {k}: {v:.3g} times its bound"
    return max(shares.values())
