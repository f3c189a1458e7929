"""Helpers of tests/test_pop_cpu.py and tests/test_gpu_pop.py: the population prior for theta (include/gpirt_hip.h, "a population
prior for theta"; csrc/pop.hip, gpirt_amd/pop.py).

theta_exact_table is tests/_stage_exact.py theta_exact -- draw_theta in long double with the bound of the device's rounding --
with row codes[i] of a prior table in place of the built-in N(0, 1).  A table entry is an exact fp64 input, so where theta_exact
carries 3 u |prior| + 2^-50 |theta*_k| for the prior's own roundings this carries nothing: the addition's one rounding, u |P_k|,
is all the prior adds.  hyper_draw is the long-double decision and the bound for the CDF of draw_pop's two draws, written here
on its own (a loop over the points) so that gpirt_amd.pop.grid_draw_exact is checked against it.  Below them the constructed
cases that both test files share.
"""
import numpy as np

import _stage_exact as X

LD = X.LD
NGRID = X.NGRID
U53, U51 = 2.0 ** -53, 2.0 ** -51


# ------------------------------------------------------------------------------------------- theta under a table ---
def theta_exact_table(y, fstar, u, stabilise, codes, table, product="fixed"):
    """theta_exact (tests/_stage_exact.py) with P[k] = table[codes[i], k] + logpost[k, i].  Same returns.  THE BOUND in the log
    domain: the terms and the product as there (lp_bound), then u |P_k| for the addition, then u |P_k - max| (stabilise); a
    table entry carries no error.  Everything behind that -- exp, the 256 x 4 scan, :25 -- as there."""
    F = np.asarray(fstar, dtype=np.float64)
    Y = np.asarray(y, dtype=np.float64)
    us = np.asarray(u, dtype=np.float64)
    tab = np.asarray(table, dtype=np.float64)
    cd = np.asarray(codes, dtype=np.int64)
    N, m = F.shape
    n = Y.shape[0]
    assert N == NGRID and Y.shape[1] == m and us.shape == (n,) and cd.shape == (n,) and tab.shape[1] == N and np.isfinite(tab).all()
    if product == "fixed" and X.theta_hands_over(F):
        product = "gemm"
    FL = F.astype(LD)
    with np.errstate(over="ignore", invalid="ignore"):
        gp, gm = -np.log1p(np.exp(-FL)), -np.log1p(np.exp(FL))
        gp[-F > X.EXP_OVERFLOW] = -np.inf
        gm[F > X.EXP_OVERFLOW] = -np.inf
    sp, ap, ip, npn = X._masked_product(gp, Y == 1.0)
    sm, am, im, nmn = X._masked_product(gm, Y == -1.0)
    lp = sp + sm
    lp[(ip + im) > 0] = -np.inf
    lp[(npn + nmn) > 0] = np.nan
    sum_abs = ap + am
    n_obs = ((Y == 1.0) | (Y == -1.0)).sum(axis=1).astype(np.float64)
    term_err = X.U51 * sum_abs + X.U50 * n_obs[None, :]
    with np.errstate(invalid="ignore"):
        lp_abs = np.where(np.isfinite(lp), np.abs(lp), LD(0)).astype(np.float64)
    if product == "fixed":
        e_k = np.floor(np.log2(np.abs(F).max(axis=1) + np.log(2.0))) + 1
        prod_err = n_obs[None, :] * 2.0 ** (e_k - 55)[:, None] + np.spacing(lp_abs)
    else:
        assert product == "gemm"
        prod_err = 1.01 * (2 * m) * U53 * sum_abs
    h = X.SCAN_DEPTH
    lp_bound = prod_err + term_err
    P = tab[cd].T.astype(LD) + lp                                          # N x n
    fin = np.isfinite(P)
    Pabs = np.where(fin, np.abs(P), LD(0)).astype(np.float64)
    eps = lp_bound + U53 * Pabs
    if stabilise:
        with np.errstate(invalid="ignore"):
            mx = np.where(np.isnan(P), LD(-np.inf), P).max(axis=0)
            P = P - mx[None, :]
        eps = eps + U53 * np.where(np.isfinite(P), np.abs(P), LD(0)).astype(np.float64)
    eps = np.where(fin, eps, 0.0)
    with np.errstate(under="ignore", invalid="ignore"):
        e = np.exp(P)
        e[P < X.EXP_UNDERFLOW] = 0
    near_flush = (np.abs(np.where(np.isfinite(P), P, LD(0)).astype(np.float64) - X.EXP_UNDERFLOW) < 1e-6).any(axis=0)
    rho = np.where(eps < 0.01, 1.01 * eps + U51, np.inf)
    with np.errstate(invalid="ignore"):
        re = np.where(e == 0, LD(0), rho.astype(LD) * e)
    C = np.cumsum(e, axis=0)
    e_tail = e.copy()
    e_tail[0] = 0
    T = np.cumsum(e_tail, axis=0)
    with np.errstate(invalid="ignore"):
        E = (np.cumsum(re, axis=0) + 1.01 * h * U53 * C).astype(np.float64) + (np.arange(1, N + 1, dtype=np.float64) * 2.0 ** -1074)[:, None]
    index = np.full(n, -1, dtype=np.int64)
    margin = np.full(n, np.inf)
    bound = np.zeros(n)
    undecided = np.zeros(n, dtype=bool)
    for i in range(n):
        bad = np.flatnonzero(np.isnan(C[:, i]))
        L = (bad[0] if bad.size else N) - 1
        if L < 0:
            continue
        TL, e0 = T[L, i], e[0, i]
        if TL == 0:
            undecided[i] = bool(near_flush[i])
            continue
        rmax = float(rho[:L + 1, i][e[:L + 1, i] > 0].max())
        if 1.01 * (1 + rmax) * TL < LD(2.0 ** -54) * e0:
            continue
        c = T[:L + 1, i] / TL
        k = int(np.argmax(c > us[i]))
        index[i] = k
        E0, EL = E[0, i], E[L, i]
        rel = (EL + E0) / float(TL)
        if not rel < 0.01:
            margin[i], bound[i], undecided[i] = 0.0, np.inf, True
            continue
        rows = np.array([k, k - 1])
        b = 1.02 * ((E[rows, i] + E0) + c[rows].astype(np.float64) * (EL + E0)) / float(TL) + 4 * U53
        margin[i] = float(np.abs(c[rows] - LD(us[i])).min())
        bound[i] = float(b.max())
        undecided[i] = bool(margin[i] < bound[i])
    return dict(index=index, logpost=lp, lp_bound=lp_bound, margin=margin, bound=bound, undecided=undecided,
                degenerate=int((index < 0).sum()), product=product)


# ------------------------------------------------------------------------------------------- the hyper-draw's CDF ---
def hyper_draw(lp, u):
    """The index draw_pop takes from the fp64 row lp against u, point by point in long double, with the bound of the device's
    rounding at the two rows that decide (the derivation: gpirt_amd.pop.grid_draw_exact's docstring; per point the error of
    lp - max is 2^-53 |x|, exp's 2 ulp plus that, 12 additions at most on the way through the 256 x 4 scan, three roundings in
    the quotient).  Returns (index, margin, bound); index -1 where C_last = C_0."""
    x = [LD(v) for v in np.asarray(lp, dtype=np.float64)]
    mx = max(x)
    e, re = [], []
    for v in x:
        d = v - mx
        ev = LD(0) if d < X.EXP_UNDERFLOW else np.exp(d)
        e.append(ev)
        re.append(LD(0) if ev == 0 else LD(1.01 * U53 * float(abs(d)) + U51) * ev)
    C, T, E = [], [], []
    c = t = r = LD(0)
    for k, (ev, rv) in enumerate(zip(e, re)):
        c += ev
        t += ev if k else LD(0)
        r += rv
        C.append(c)
        T.append(t)
        E.append(float(r + LD(1.01 * 12 * U53) * c) + (k + 1) * 2.0 ** -1074)
    TL = T[-1]
    if TL == 0:
        return -1, np.inf, 0.0
    cdf = [tk / TL for tk in T]
    k = next(i for i, v in enumerate(cdf) if v > LD(u))
    rows = (k, k - 1)                                                     # (k >= 1: cdf[0] = 0 is never above u)
    b = max(1.02 * ((E[j] + E[0]) + float(cdf[j]) * (E[-1] + E[0])) / float(TL) + 4 * U53 for j in rows)
    margin = min(float(abs(cdf[j] - LD(u))) for j in rows)
    return k, margin, b


# ---------------------------------------------------------------------------------------------- constructed cases ---
THETA_SEED, THETA_IT, THETA_M = 23, 4, 6
# (n, G): n = 1 allows one group alone (every group has a member)
THETA_SHAPES = ((1, 1), (65, 1), (65, 2), (65, 8), (257, 1), (257, 2), (257, 8))
ROWS_BY_G = {1: {1: ("shifted",), 65: ("flat",), 257: ("two_point",)},
             2: {65: ("shifted", "narrow"), 257: ("flat", "two_point")},
             8: {65: ("shifted", "narrow", "flat", "two_point", "default", "mixture", "wide", "shifted"),
                 257: ("shifted", "narrow", "flat", "two_point", "default", "mixture", "wide", "shifted")}}


def prior_row(kind):
    from gpirt_amd import pop as PO
    if kind == "shifted":
        return PO.normal_table(1.25, 0.8)[0]
    if kind == "narrow":
        return PO.normal_table(4.9, 0.05)[0]                               # sd 0.05 at mu = 4.9: the mass on the last rows
    if kind == "wide":
        return PO.normal_table(-0.7, 2.5)[0]
    if kind == "flat":
        return np.zeros(NGRID)
    if kind == "default":
        return PO.default_row()
    if kind == "two_point":
        r = np.full(NGRID, -1e300)                                         # every other entry -1e300
        r[310], r[655] = 0.0, -0.4
        return r
    assert kind == "mixture"
    a, b = PO.normal_table(-1.5, 0.4)[0].astype(LD), PO.normal_table(1.0, 0.6)[0].astype(LD)
    return np.log(0.3 * np.exp(a) + 0.7 * np.exp(b)).astype(np.float64)


def theta_case(n, G):
    """y (n x 6), fstar (1001 x 6: modest slopes, so that no posterior is a point), codes (the last group has ONE member where
    G > 1), the table, the uniforms of (THETA_SEED, THETA_IT)"""
    rng = np.random.default_rng(1000 * n + G)
    m = THETA_M
    t = X.grid()
    fstar = rng.uniform(-1.0, 1.0, m)[None, :] + rng.uniform(0.3, 1.2, m)[None, :] * t[:, None] + 0.3 * np.sin(t[:, None] * rng.uniform(0.5, 2.0, m)[None, :])
    y = np.where(rng.random((n, m)) < 0.5, 1.0, -1.0)
    y[rng.random((n, m)) < 0.1] = np.nan
    if G == 1:
        codes = np.zeros(n, dtype=np.int32)
    else:
        codes = (np.arange(n) % (G - 1)).astype(np.int32)
        codes[n // 2] = G - 1                                              # a group with one member
    kinds = ROWS_BY_G[G][n]
    table = np.array([prior_row(k) for k in kinds])
    return dict(y=np.asfortranarray(y), fstar=np.asfortranarray(fstar), codes=codes, table=table, kinds=kinds,
                u=X.theta_uniforms(THETA_SEED, THETA_IT, n))


# the update from a constructed theta: (n, G, P_mu, P_sd); every value of the issue's lists appears, the edges 255 | 256 | 257 of
# the 256 x 4 layout together.  n = 1 with G >= 2 cannot be (every group has a member): n = 2 stands for it, group 1 of one member.
UPDATE_CASES = ((2, 2, 2, 3), (63, 2, 3, 2), (64, 8, 255, 257), (65, 2, 256, 256), (255, 8, 257, 255), (256, 2, 1024, 2),
                (257, 8, 2, 1024), (1025, 8, 256, 255))
UPDATE_SEED = 31
MU_HI, SD_LO, SD_HI = 2.5, 0.25, 4.0


def update_case(n, G, P_mu, P_sd):
    """theta on the grid per group (group g about 0.4 g - 1 with sd 0.5 + 0.1 g), the codes, the start indices.  On a mu grid
    of two points the draw can only take index 1 (index 0 is never drawn), and it fails where that point's mass underflows
    against index 0's: the groups are moved up by 1.5 there, so that every draw of every case is an update."""
    rng = np.random.default_rng(7 * n + G)
    codes = (np.arange(n) % G).astype(np.int32)
    z = rng.standard_normal(n)
    th = (0.4 * codes - 1.0 + (1.5 if P_mu == 2 else 0.0)) + (0.5 + 0.1 * codes) * z
    k = np.clip(np.rint((th + 5.0) * 100.0), 0, 1000)
    theta = -5.0 + k * 0.01
    a0 = (np.arange(G) * 7 + 1) % P_mu
    b0 = (np.arange(G) * 5 + 1) % P_sd
    return dict(theta=theta, codes=codes, a0=a0.astype(np.int32), b0=b0.astype(np.int32), n=n, G=G, P_mu=P_mu, P_sd=P_sd)


FROZEN = dict(n=300, G=3, P=33, calls=4000, seed=5, mu_hi=2.0, sd_lo=0.3, sd_hi=3.0)


def frozen_case():
    c = FROZEN
    rng = np.random.default_rng(99)
    codes = (np.arange(c["n"]) % c["G"]).astype(np.int32)
    th = 0.5 * codes + (0.8 + 0.2 * codes) * rng.standard_normal(c["n"])
    theta = -5.0 + np.clip(np.rint((th + 5.0) * 100.0), 0, 1000) * 0.01
    return dict(theta=theta, codes=codes)
