"""Bounds for comparing the device's equating accumulators (csrc/equate.hip) with gpirt_amd.equate.from_draws, counted from the
operations of the header's statement in the manner of tests/_sumscore_bounds.py (whose constants these are) -- never from what
the device gives.  eps = 2^-52; one rounding is eps / 2.

  A_X, A_Y    rel_A(M) of the form's M steps, plus the floor (M + 1) 2^-1021 (the sum-score bounds).
  J           a term (w_k A_X) A_Y carries rel_A(M_X) + rel_A(M_Y), the rounding of w_k A_X and of the product (eps / 2 each; the
              matrix core fuses the product, which is no worse); 1001 non-negative terms added in ANY order lose at most
              (1001 - 1) eps / 2 of their sum: (1 + 1001) eps / 2 in all.  The floor: both factors' floors (the other factor and
              sum_k w_k are <= 1) and 1001 products that may underflow.  joint_sum adds D eps and D floors.
  pi          the sum-score bound: rel_A(M) + (1 + 1001) eps / 2; pi_sum adds D eps, pi_sumsq doubles and adds.
  F           s + 1 non-negative terms added in ascending score: the terms' r_pi and at most M eps / 2 of the sum.
  P           F_A[s - 1] + pi_A[s] / 2: both terms' errors and one more sum, relative to P: r_pi + (M_A + 1) eps / 2.
  e           (t* - 1/2) + (P - F_B[t* - 1]) / pi_B[t*].  As a function of P, e is continuous, piecewise linear and increasing with
              slope 1 / pi_B[t] on segment t (a segment is 1 high whatever its width), and the device's F_B, pi_B are a
              perturbed copy of the reference's.  With d = dP + dF_B, every segment that [P - d, P + d] touches can be the
              device's t*; the steepest of them bounds the error: d / min pi_B.  This is ill-conditioned where pi_B is tiny,
              and a touched segment without any mass has no bound (inf).  On top come pi_B's own r_pi and the division (on a
              quotient <= 1) and the two sums (eps / 2 of |e| + 1).
  r           a = sum w T, b = sum w (V + T T), c = sum w T_X T_Y with their terms' errors (the sum-score bounds' r_T, r_V)
              and (1 + 1001) eps / 2 of their own; c - a_X a_Y and b - a a CANCEL, so their absolute errors are carried as such
              and r's bound is worked out per draw from the reference's corr_terms; a draw whose variance is not clear of its own
              error has no bound (inf).
Every relative bound gets one eps more for the reference's own rounding to float64 and the factor SLACK for the second order.
A cell whose bound on e exceeds E_KEEP = 1e-6 score points is left out of the comparison of e; `keep_conditions` asserts, from
the reference alone, that no cell with 0.01 <= F[s] <= 0.99 is left out.
"""
import numpy as np

from _sumscore_bounds import C_PQ, EPS, FLOOR, N, SLACK, rel_A

E_KEEP = 1e-6
TINY = 2.0 ** -1074
RAW = ("joint_sum", "pix_sum", "pix_sumsq", "piy_sum", "piy_sumsq", "eyx_sum", "eyx_sumsq", "exy_sum", "exy_sumsq", "corr",
       "corr_terms", "mask_x", "mask_y", "w", "last_joint", "last_pix", "last_piy", "last_eyx", "last_exy")
OWN = SLACK * (1 + N) * 0.5 * EPS


def r_pi(M):
    return rel_A(M) + OWN


def rel_J(Mx, My):
    return rel_A(Mx) + rel_A(My) + OWN


def floor_J(Mx, My):
    return (Mx + My + 2) * FLOOR + N * TINY


def e_bound(pi_a, pi_b):
    """(bound, risky) per score of form A for its equivalent on B's scale, from the reference's pi alone; risky counts the
    cells whose [P - d, P + d] reaches the top of F_B (whether such a cell is clamped is a matter of rounding)"""
    Ma, Mb = pi_a.size - 1, pi_b.size - 1
    Fa, Fb = np.cumsum(pi_a), np.cumsum(pi_b)
    P = np.concatenate([[0.0], Fa[:-1]]) + 0.5 * pi_a
    dP = (r_pi(Ma) + SLACK * 0.5 * (Ma + 1) * EPS) * P + (Ma + 1) * (Ma + 1) * FLOOR
    dF = (r_pi(Mb) + SLACK * 0.5 * Mb * EPS) * Fb + (Mb + 1) * (Mb + 1) * FLOOR
    out = np.empty(Ma + 1)
    risky = 0
    for s in range(Ma + 1):
        t0 = min(int(np.searchsorted(Fb, P[s], side="right")), Mb)
        d = dP[s] + dF[min(t0 + 1, Mb)]
        lo = min(int(np.searchsorted(Fb, P[s] - d, side="right")), Mb)
        hi = int(np.searchsorted(Fb, P[s] + d, side="right"))
        if hi > Mb:
            risky += 1
            hi = Mb
        pmin = pi_b[lo:hi + 1].min()
        e_abs = Mb + 1.5
        out[s] = SLACK * (d / pmin + r_pi(Mb) + EPS + EPS * e_abs) if pmin > 0.0 else np.inf
    return out, risky


def r_bound(terms, Mx, My):
    """the bound on one draw's correlation from its five sums (a_X, b_X, a_Y, b_Y, c); inf where a variance is not clear"""
    ax, bx, ay, by, c = (float(v) for v in terms)
    rT = lambda M: SLACK * (C_PQ + 0.5 * M) * EPS + EPS                         # noqa: E731
    rV = lambda M: SLACK * (2 * C_PQ + 0.5 + 0.5 * M) * EPS + EPS               # noqa: E731
    e_ax, e_ay = rT(Mx) + OWN, rT(My) + OWN
    e_bx = max(rV(Mx), 2 * rT(Mx) + 0.5 * EPS) + 0.5 * EPS + OWN
    e_by = max(rV(My), 2 * rT(My) + 0.5 * EPS) + 0.5 * EPS + OWN
    e_c = rT(Mx) + rT(My) + EPS + OWN
    vx, vy, num = bx - ax * ax, by - ay * ay, c - ax * ay
    dvx = e_bx * bx + (2 * e_ax + 0.5 * EPS) * ax * ax + 0.5 * EPS * abs(vx)
    dvy = e_by * by + (2 * e_ay + 0.5 * EPS) * ay * ay + 0.5 * EPS * abs(vy)
    if not (vx > 2.0 * dvx and vy > 2.0 * dvy):
        return np.inf, np.nan
    dnum = e_c * c + (e_ax + e_ay + 0.5 * EPS) * abs(ax * ay) + 0.5 * EPS * abs(num)
    den = np.sqrt(vx * vy)
    r = num / den
    rel_den = 0.5 * (dvx / (vx - dvx) + dvy / (vy - dvy) + 0.5 * EPS) + EPS
    return SLACK * (dnum / den + abs(r) * (rel_den + EPS)) + EPS * abs(r), r


def bounds(want, singles):
    """per-cell bounds for the raw arrays of `want` (from_draws of all draws); singles: from_draws of each COUNTED draw alone,
    in order (their last_* arrays are that draw's values)"""
    Mx, My, D = int(want["Mx"]), int(want["My"]), int(want["draws"])
    assert len(singles) == D
    rJ, fJ = rel_J(Mx, My), floor_J(Mx, My)
    b = dict(last_joint=rJ * want["last_joint"] + fJ, joint_sum=(rJ + D * EPS) * want["joint_sum"] + D * fJ)
    for f, M in (("x", Mx), ("y", My)):
        fl = (M + 1) * FLOOR
        b[f"last_pi{f}"] = r_pi(M) * want[f"last_pi{f}"] + fl
        b[f"pi{f}_sum"] = (r_pi(M) + D * EPS) * want[f"pi{f}_sum"] + D * fl
        b[f"pi{f}_sumsq"] = (2 * r_pi(M) + (1 + D) * EPS) * want[f"pi{f}_sumsq"] + 2 * D * fl
    risky = 0
    for key, a, bb in (("eyx", "last_pix", "last_piy"), ("exy", "last_piy", "last_pix")):
        s0 = s1 = a0 = a1 = 0.0
        last = None
        for one in singles:
            last, rk = e_bound(one[a], one[bb])
            e = np.abs(one[f"last_{key}"])
            risky += rk
            with np.errstate(invalid="ignore"):
                s0 = s0 + last
                s1 = s1 + 2 * e * last + last * last + 0.5 * EPS * e * e
            a0, a1 = a0 + e, a1 + e * e
        b[f"last_{key}"] = last
        b[f"{key}_sum"] = s0 + D * EPS * a0
        b[f"{key}_sumsq"] = s1 + D * EPS * a1
        b[f"{key}_keep"] = np.isfinite(s0) & (s0 <= E_KEEP) if D else np.zeros(0, dtype=bool)
        b[f"last_{key}_keep"] = np.isfinite(last) & (last <= E_KEEP)
    b["risky"] = risky
    d0 = d1 = s0 = s1 = 0.0
    for terms in np.asarray(want["corr_terms_all"]).reshape(-1, 5):
        dr, r = r_bound(terms, Mx, My)
        if not np.isfinite(dr):
            d0 = d1 = np.inf
            break
        d0 += dr
        d1 += 2 * abs(r) * dr + dr * dr + 0.5 * EPS * r * r
        s0 += abs(r)
        s1 += r * r
    b["corr"] = np.array([d0 + D * EPS * s0, d1 + D * EPS * s1])
    return b


def decision_tol(want):
    """(agreement, kappa): absolute tolerances per cut for the decision consistency from the pooled joint.  Every cell of
    joint_sum carries rel_J + D eps; a sum of non-negative cells over the total (itself such a sum) carries twice that plus the
    additions: delta.  agreement is two such sums (2 delta); p_X and p_Y carry delta each, so chance agreement p_e = p_X p_Y +
    (1 - p_X)(1 - p_Y) carries 4 delta.  kappa = (agreement - p_e) / (1 - p_e) CANCELS in its numerator, so the absolute errors
    are carried as such: (6 delta + |kappa| 4 delta) / (1 - p_e - 4 delta); a denominator not clear of its error has no bound."""
    Mx, My, D = int(want["Mx"]), int(want["My"]), int(want["draws"])
    delta = SLACK * 2.0 * (rel_J(Mx, My) + D * EPS + (Mx + 1) * (My + 1) * EPS) + EPS
    J = np.asarray(want["joint_sum"], dtype=np.float64)
    tot = J.sum()
    agree, kappa = [], []
    for (cx, cy), k in zip(np.asarray(want["cuts"]).reshape(-1, 2), np.asarray(want["kappa"]).reshape(-1)):
        px, py = J[cx:, :].sum() / tot, J[:, cy:].sum() / tot
        den = 1.0 - (px * py + (1.0 - px) * (1.0 - py))
        agree.append(2.0 * delta)
        kappa.append((6.0 + 4.0 * abs(k)) * delta / (den - 4.0 * delta) + EPS * abs(k) if den > 8.0 * delta else np.inf)
    return np.array(agree), np.array(kappa)


def keep_conditions(singles, quarter=True, label=""):
    """From the reference alone, before the device is looked at: every score with 0.01 <= F[s] <= 0.99 is kept, and (small-form
    cases) at most a quarter of the cells are left out.  Returns the share of cells left out."""
    out = cells = 0
    for one in singles:
        for a, bb in (("last_pix", "last_piy"), ("last_piy", "last_pix")):
            bd, _ = e_bound(one[a], one[bb])
            F = np.cumsum(one[a])
            kept = np.isfinite(bd) & (bd <= E_KEEP)
            assert kept[(F >= 0.01) & (F <= 0.99)].all(), f"{label}: a score in the body of the distribution has no usable bound"
            out += int((~kept).sum())
            cells += kept.size
    share = out / max(cells, 1)
    if quarter:
        assert share <= 0.25, f"{label}: {share:.3f} of the equating cells are left out"
    return share


def check(got, want, singles, label="", need_corr=True, quarter=True):
    """Asserts the keep conditions (from the reference alone), then every bound; prints MEASURED with the largest share of its
    bound that each array used and the share of equating cells left out.  Returns the largest share."""
    left_out = keep_conditions(singles, quarter, label)
    bd = bounds(want, singles)
    corr_ok = bool(np.isfinite(bd["corr"]).all())
    assert corr_ok or not need_corr, f"{label}: a draw's variance is not clear of its error: corr cannot be compared"
    for k in ("mask_x", "mask_y", "w"):
        assert np.array_equal(got[k], want[k]), f"{label}: {k} differs"
    for k in ("draws", "skipped", "Mx", "My"):
        assert got[k] == want[k], f"{label} {k}: {got[k]} != {want[k]}"
    if bd["risky"] == 0:
        assert got["eq_clamped"] == want["eq_clamped"], f"{label}: eq_clamped {got['eq_clamped']} != {want['eq_clamped']}"
    keys = ["joint_sum", "last_joint", "pix_sum", "pix_sumsq", "piy_sum", "piy_sumsq", "last_pix", "last_piy", "eyx_sum", "eyx_sumsq",
            "exy_sum", "exy_sumsq", "last_eyx", "last_exy"]
    if corr_ok:
        keys.append("corr")
        assert (got["corr_draws"], got["corr_skipped"]) == (want["corr_draws"], want["corr_skipped"]), f"{label}: corr counters"
    shares = {}
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and not np.isnan(g).any(), f"{label} {k}: shape or NaN"
        gap, bound = np.abs(g - w), bd[k]
        if k[-3:] in ("eyx", "exy") or k[:3] in ("eyx", "exy"):
            keep = bd[("last_" if k.startswith("last_") else "") + k.replace("last_", "")[:3] + "_keep"]
            gap, bound = gap[keep], bound[keep]
        with np.errstate(invalid="ignore", divide="ignore"):
            share = np.where(gap > 0, gap / bound, 0.0)
        shares[k] = float(share.max()) if share.size else 0.0
    print(f"MEASURED {label}: M_X {want['Mx']} M_Y {want['My']} draws {want['draws']}; equating cells left out {left_out:.3f}; "
          f"share of the bound used: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()) +
          ("" if corr_ok else "; corr not comparable (variance)"))
    for k, v in shares.items():
        assert v <= 1.0, f"{label} {k}: {v:.3g} times its bound"
    return max(shares.values())
