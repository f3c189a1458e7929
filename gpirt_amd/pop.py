"""A population prior for theta: group means and sds, fixed or sampled in the chain (include/gpirt_hip.h, "a population prior
for theta": gpirt_pop_check, gpirt_sampler_pop_*, gpirt_sampler_draw_pop; csrc/pop.hip, csrc/stages.hip, csrc/sampler.hip).

Respondent i carries a group code g_i in 0 .. G - 1 (parties, cohorts, treatment arms) and group g's prior is a mass on the
theta grid t_k = -5 + 0.01 k, row g of a G x 1001 table of log masses that draw_theta adds in place of the reference's N(0, 1):
the multiple-group IRT model (Bock & Zimowski 1997).  Fixed (Sampler.pop_set), any finite table is allowed.  Sampled
(Sampler.pop_enable), group 0 is the anchor -- its fixed row is what identifies location and scale -- and every other group has
(mu_g, sd_g) on two grids, updated by exact Gibbs on the grids from the group's integer sufficient statistics (Sampler.draw_pop:
two launches, no host read).  score, predict, sumscore and shape's reliability weights keep reading N(0, 1), group 0's default
population.

`run` is the one-call way in.  `step_exact` is the NumPy statement of one draw_pop: its lp rows are the device's bits, the CDF
and the decision are long double with a margin and a bound per draw.  `conditional` gives the exact joint masses of (a, b) for
a frozen theta: the stationary distribution of the update.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import NGRID, ST_POP, check

LD = np.longdouble
CENTRE = (NGRID - 1) // 2
U53, U51 = 2.0 ** -53, 2.0 ** -51
SCAN_DEPTH = 3 + 8 + 1            # csrc/pop.hip pop_grid_draw: 3 additions inside a thread, 8 scan levels, 1 base addition
EXP_UNDERFLOW = -745.1332191019412

_dp = C.POINTER(C.c_double)


def _p(a):
    return a.ctypes.data_as(_dp)


# ---------------------------------------------------------------------------------------------------- the contract ---
def theta_grid() -> np.ndarray:
    """t_k = -5.0 + k * 0.01, each product and sum rounded on its own: the device's grid values"""
    return -5.0 + np.arange(NGRID, dtype=np.float64) * 0.01


def default_row() -> np.ndarray:
    """The N(0, 1) row, -(ln sqrt(2 pi) + 0.5 z z) with z = |t_k|, as theta_sample_kernel forms the built-in prior: a sampler
    whose rows are all this row draws the bits of a sampler without a population prior (gpirt_pop_default_row)."""
    out = np.empty(NGRID)
    check(_lib.load().gpirt_pop_default_row(_p(out)))
    return out


def normal_table(mu, sd) -> np.ndarray:
    """G x 1001: row g = -(0.5 z z), z = (t_k - mu_g) / sd_g, every operation one fp64 rounding -- the expression by which
    draw_pop rebuilds a group's row (gpirt_pop_normal_row).  Unnormalised; the constant cancels in draw_theta."""
    mu = np.atleast_1d(np.asarray(mu, dtype=np.float64))
    sd = np.broadcast_to(np.asarray(sd, dtype=np.float64), mu.shape)
    if not (np.isfinite(mu).all() and np.isfinite(sd).all() and (sd > 0).all()):
        raise ValueError("normal_table: finite mu and sd > 0 are needed")
    t = theta_grid()
    z = (t[None, :] - mu[:, None]) / sd[:, None]
    return -((0.5 * z) * z)


def grids(mu_hi=3.0, points_mu=121, sd_lo=0.2, sd_hi=5.0, points_sd=65) -> tuple:
    """(mu_grid, sd_grid) as the library keeps them (gpirt_pop_grids): mu linear on [-mu_hi, mu_hi], antisymmetric bit for bit,
    sd logarithmic on [sd_lo, sd_hi] by gpirt_ell_grid's rule with exact end points.  GpirtError names what is out of range."""
    Pm, Ps = int(points_mu), int(points_sd)
    mu, sd = np.empty(max(Pm, 1)), np.empty(max(Ps, 1))
    check(_lib.load().gpirt_pop_grids(float(mu_hi), Pm, float(sd_lo), float(sd_hi), Ps, _p(mu), _p(sd)))
    return mu, sd


def lse_table(mu_grid, sd_grid) -> np.ndarray:
    """lse[a, b] = log sum_k exp(-(t_k - mu_a)^2 / (2 sd_b^2)), the theta grid's normaliser of a normal row: long double on the
    host, k ascending, rounded once (gpirt_pop_lse: the table a sampler holds under "lse")."""
    mu = np.ascontiguousarray(mu_grid, dtype=np.float64)
    sd = np.ascontiguousarray(sd_grid, dtype=np.float64)
    out = np.empty((mu.shape[0], sd.shape[0]))
    check(_lib.load().gpirt_pop_lse(_p(mu), mu.shape[0], _p(sd), sd.shape[0], _p(out)))
    return out


def check_args(codes=None, groups=1, log_prior=None, sampled=False, mu_hi=3.0, points_mu=121, sd_lo=0.2, sd_hi=5.0, points_sd=65,
               log_hyper_mu=None, log_hyper_sd=None, a0=None, b0=None, options=None) -> None:
    """gpirt_pop_check (no device is touched): every refusal of Sampler.pop_set's (sampled=False) and Sampler.pop_enable's
    (sampled=True) arguments as a GpirtError that names its reason.  options: a gpirt_options (_lib.Options) or None."""
    G = int(groups)
    cd = None if codes is None else np.ascontiguousarray(codes, dtype=np.int32).reshape(-1)
    lp = None if log_prior is None else np.ascontiguousarray(np.atleast_2d(log_prior), dtype=np.float64)
    if lp is not None and lp.shape[1] != NGRID:
        raise ValueError(f"pop: log_prior must have {NGRID} columns")
    Pm, Ps = int(points_mu), int(points_sd)
    hm = None if log_hyper_mu is None else np.ascontiguousarray(log_hyper_mu, dtype=np.float64)
    hs = None if log_hyper_sd is None else np.ascontiguousarray(log_hyper_sd, dtype=np.float64)
    if hm is not None and hm.shape != (Pm,):
        raise ValueError(f"pop: log_hyper_mu must hold points_mu = {Pm} values")
    if hs is not None and hs.shape != (Ps,):
        raise ValueError(f"pop: log_hyper_sd must hold points_sd = {Ps} values")
    ints = lambda v: None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.int32), (max(G, 1),)))  # noqa: E731
    ia, ib = ints(a0), ints(b0)
    ip = lambda v: None if v is None else v.ctypes.data_as(C.POINTER(C.c_int))              # noqa: E731
    check(_lib.load().gpirt_pop_check(None if cd is None else cd.ctypes.data_as(C.POINTER(C.c_int32)), 0 if cd is None else cd.shape[0],
                                      G, None if lp is None else _p(lp), 0 if lp is None else lp.shape[0], int(bool(sampled)),
                                      float(mu_hi), Pm, float(sd_lo), float(sd_hi), Ps, None if hm is None else _p(hm),
                                      None if hs is None else _p(hs), ip(ia), ip(ib),
                                      None if options is None else C.byref(options)))


def uniforms(seed, t, group) -> tuple:
    """(u0, u1) of group `group` in the t-th draw_pop call on a sampler (t counted from 1): item_uniform(seed, t, GPIRT_ST_POP,
    group, 0 / 1), mu's and sd's.  group may be an array: two arrays come back."""
    from .ppc import item_uniform
    g = np.asarray(group, dtype=np.uint64)
    u = item_uniform(seed, int(t), ST_POP, g[..., None], np.arange(2, dtype=np.uint64))
    if g.ndim == 0:
        return float(u[0]), float(u[1])
    return u[..., 0], u[..., 1]


# ------------------------------------------------------------------------------------------------------- NumPy -------
def grid_index(theta) -> np.ndarray:
    """k where theta is bit for bit -5 + 0.01 k, else -1 (csrc/kernels.h grid_index)"""
    t = np.asarray(theta, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        k = np.rint((t + 5.0) * 100.0)
        ok = (k >= 0) & (k <= NGRID - 1) & (-5.0 + k * 0.01 == t)
    return np.where(ok, k, -1).astype(np.int64)


def stats_exact(theta, codes, G) -> dict:
    """The groups' sufficient statistics as draw_pop forms them, exact integers: n (members on the grid), S1 = sum (k_i - 500),
    S2 = sum (k_i - 500)^2 and off_grid (members whose theta is no grid point), G values each (int64)."""
    k = grid_index(theta)
    cd = np.asarray(codes, dtype=np.int64)
    n, S1, S2, off = (np.zeros(int(G), dtype=np.int64) for _ in range(4))
    for g in range(int(G)):
        mem = cd == g
        on = mem & (k >= 0)
        d = k[on] - CENTRE
        n[g], S1[g], S2[g], off[g] = int(on.sum()), int(d.sum()), int((d * d).sum()), int((mem & (k < 0)).sum())
    return dict(n=n, S1=S1, S2=S2, off_grid=off)


def _quad(n, S1, S2, m):
    """Q = (A - B) + C of the header, fp64, every operation rounded on its own; m may be an array"""
    c = 0.01
    fn, f1, f2 = np.float64(n), np.float64(S1), np.float64(S2)
    A = (f2 * c) * c
    B = ((2.0 * m) * f1) * c
    Cc = (fn * m) * m
    return (A - B) + Cc


def lp_mu_row(n, S1, S2, mu_grid, sd_b, lse_col, log_hyper_mu) -> np.ndarray:
    """lp[a] of step 2 in fp64, the header's order: the device's bits"""
    den = 2.0 * (np.float64(sd_b) * np.float64(sd_b))
    return (log_hyper_mu - _quad(n, S1, S2, mu_grid) / den) - np.float64(n) * lse_col


def lp_sd_row(n, S1, S2, mu_a, sd_grid, lse_row, log_hyper_sd) -> np.ndarray:
    """lp[b] of step 3 in fp64, the header's order: the device's bits"""
    den = 2.0 * (sd_grid * sd_grid)
    return (log_hyper_sd - _quad(n, S1, S2, np.float64(mu_a)) / den) - np.float64(n) * lse_row


def grid_draw_exact(lp, u) -> dict:
    """The draw of an index from the fp64 row lp against the uniform u, in long double: subtract the maximum, exp (fp64's range:
    0 below 2^-1075), cumulative sum, cdf_k = (C_k - C_0) / (C_last - C_0), the first k with cdf_k > u (so k = 0 is never
    drawn).  index = -1 where C_last = C_0.  margin = min(|cdf_k - u|, |cdf_{k-1} - u|); bound on |device cdf - cdf| at those two
    rows, derived as tests/_stage_exact.py theta_exact derives draw_theta's: lp - max is one rounding (2^-53 |x|), exp is within
    2 ulp plus its argument's error as a relative one (rho_k), every term passes through at most 12 additions of the 256 x 4
    scan, and the quotient is three roundings:
        |d cdf_k| <= 1.02 ((E_k + E_0) + cdf_k (E_L + E_0)) / T_L + 4 * 2^-53,   E_k = sum_{j<=k} (rho_j e_j + 2^-1074) + 1.01 * 12 * 2^-53 C_k
    decided = margin >= bound."""
    x = np.asarray(lp, dtype=np.float64)
    P = x.shape[0]
    d = x.astype(LD) - LD(x.max())
    eps = U53 * np.abs(d).astype(np.float64)
    with np.errstate(under="ignore"):
        e = np.exp(d)
    e[d < EXP_UNDERFLOW] = 0
    rho = 1.01 * eps + U51
    re = np.where(e == 0, LD(0), rho.astype(LD) * e)
    Cs = np.cumsum(e)
    et = e.copy()
    et[0] = 0
    T = np.cumsum(et)
    E = (np.cumsum(re) + 1.01 * SCAN_DEPTH * U53 * Cs).astype(np.float64) + np.arange(1, P + 1, dtype=np.float64) * 2.0 ** -1074
    TL = T[-1]
    if TL == 0:
        return dict(index=-1, margin=np.inf, bound=0.0, decided=True, cdf=np.full(P, LD("nan")))
    cdf = T / TL
    k = int(np.argmax(cdf > LD(u)))
    rows = np.array([k, k - 1])
    b = 1.02 * ((E[rows] + E[0]) + cdf[rows].astype(np.float64) * (E[-1] + E[0])) / float(TL) + 4 * U53
    margin = float(np.abs(cdf[rows] - LD(u)).min())
    bound = float(b.max())
    return dict(index=k, margin=margin, bound=bound, decided=bool(margin >= bound), cdf=cdf)


def step_exact(theta, codes, index, seed, t, mu_grid, sd_grid, lse, log_hyper_mu=None, log_hyper_sd=None, log_prior=None) -> dict:
    """One draw_pop as the header states it.  theta (n), codes (n), index (G x 2: the (a, b) in front of the call, row 0 not
    read), the sampler's seed, t the count of draw_pop calls including this one, the grids and lse as the sampler holds them,
    the hyperprior masses (None: zeros), log_prior (G x 1001: the table in front of the call, or None).
    Returns dict(stats: stats_exact's, status (G of "anchor", "updated", "skipped", "failed"), index (G x 2 afterwards), lp_mu
    (G x P_mu) and lp_sd (G x P_sd) -- fp64, the device's bits; rows of groups that were not updated are NaN --, u0, u1, decided
    (G x 2 bool), margin, bound (G x 2), log_prior (the table afterwards, when one was given)).  The sd draw conditions on the mu
    index found here: where mu's draw is undecided, sd's says nothing."""
    mu_grid = np.asarray(mu_grid, dtype=np.float64)
    sd_grid = np.asarray(sd_grid, dtype=np.float64)
    lse = np.asarray(lse, dtype=np.float64)
    Pm, Ps = mu_grid.shape[0], sd_grid.shape[0]
    idx = np.array(index, dtype=np.int64).reshape(-1, 2).copy()
    G = idx.shape[0]
    hm = np.zeros(Pm) if log_hyper_mu is None else np.asarray(log_hyper_mu, dtype=np.float64)
    hs = np.zeros(Ps) if log_hyper_sd is None else np.asarray(log_hyper_sd, dtype=np.float64)
    st = stats_exact(theta, codes, G)
    u0, u1 = uniforms(seed, t, np.arange(G, dtype=np.uint64))
    lpm, lps = np.full((G, Pm), np.nan), np.full((G, Ps), np.nan)
    decided = np.ones((G, 2), dtype=bool)
    margin, bound = np.full((G, 2), np.inf), np.zeros((G, 2))
    table = None if log_prior is None else np.array(log_prior, dtype=np.float64)
    status = ["anchor"]
    for g in range(1, G):
        if st["off_grid"][g]:
            status.append("skipped")
            continue
        n, S1, S2 = int(st["n"][g]), int(st["S1"][g]), int(st["S2"][g])
        lpm[g] = lp_mu_row(n, S1, S2, mu_grid, sd_grid[idx[g, 1]], lse[:, idx[g, 1]], hm)
        da = grid_draw_exact(lpm[g], u0[g])
        decided[g, 0], margin[g, 0], bound[g, 0] = da["decided"], da["margin"], da["bound"]
        if da["index"] < 0:
            status.append("failed")
            continue
        a = da["index"]
        lps[g] = lp_sd_row(n, S1, S2, mu_grid[a], sd_grid, lse[a, :], hs)
        db = grid_draw_exact(lps[g], u1[g])
        decided[g, 1], margin[g, 1], bound[g, 1] = db["decided"], db["margin"], db["bound"]
        if db["index"] < 0:
            status.append("failed")
            continue
        idx[g] = (a, db["index"])
        status.append("updated")
        if table is not None:
            table[g] = normal_table(mu_grid[a], sd_grid[db["index"]])[0]
    return dict(stats=st, status=status, index=idx, lp_mu=lpm, lp_sd=lps, u0=u0, u1=u1, decided=decided, margin=margin, bound=bound,
                log_prior=table)


def conditional(n, S1, S2, mu_grid, sd_grid, lse, log_hyper_mu=None, log_hyper_sd=None) -> np.ndarray:
    """The exact joint masses p(a, b | theta) of one group on the grids (P_mu x P_sd, long double, summing to 1) from its
    statistics: log p = log_hyper_mu[a] + log_hyper_sd[b] - Q_a / (2 sd_b^2) - n lse[a, b] with Q_a = S2 c^2 - 2 mu_a S1 c + n mu_a^2,
    c = 0.01, in long double from the fp64 tables.  Index 0 of either grid carries mass 0: the update's rule, the first index
    whose (C - C_0) / (C_last - C_0) exceeds u, never draws it (as draw_theta never draws the first theta point).  For a frozen
    theta this is the stationary distribution of draw_pop's alternation."""
    mu = np.asarray(mu_grid, dtype=np.float64).astype(LD)
    sd = np.asarray(sd_grid, dtype=np.float64).astype(LD)
    hm = np.zeros(mu.shape[0], dtype=LD) if log_hyper_mu is None else np.asarray(log_hyper_mu, dtype=np.float64).astype(LD)
    hs = np.zeros(sd.shape[0], dtype=LD) if log_hyper_sd is None else np.asarray(log_hyper_sd, dtype=np.float64).astype(LD)
    c = LD("0.01")
    Q = LD(int(S2)) * c * c - 2 * mu * LD(int(S1)) * c + LD(int(n)) * mu * mu
    lw = hm[:, None] + hs[None, :] - Q[:, None] / (2 * sd * sd)[None, :] - LD(int(n)) * np.asarray(lse, dtype=np.float64).astype(LD)
    lw[0, :] = -np.inf
    lw[:, 0] = -np.inf
    w = np.exp(lw - lw.max())
    return w / w.sum()


# ------------------------------------------------------------------------------------------------------- summaries ---
def summarise(draws, hist_mu, hist_sd, mu_grid, sd_grid, signs=None, probs=(0.025, 0.25, 0.5, 0.75, 0.975)) -> dict:
    """Exact summaries per group from the histograms.  draws: chains x S x G x 2 (or S x G x 2) recorded indices; hist_mu: chains
    x P_mu x G (or P_mu x G) counts, hist_sd likewise; signs: None, or one +1 / -1 per chain -- a chain with -1 (one that
    `diagnostics["reflected"]` of gpirt_amd.chains.combine reports) enters with its mu axis reversed, a -> P_mu - 1 - a, which is
    mu -> -mu bit for bit on the antisymmetric grid.  Returns hist_mu, hist_sd (pooled), draws (aligned), and per group mean,
    sd and quantiles of mu and of sd (mu_mean, mu_sd, mu_quantiles, sd_mean, sd_sd, sd_quantiles; group 0, the anchor, is NaN)."""
    mu_grid = np.asarray(mu_grid, dtype=np.float64)
    sd_grid = np.asarray(sd_grid, dtype=np.float64)
    d = np.array(draws, dtype=np.int64)
    hm, hs = np.array(hist_mu, dtype=np.int64), np.array(hist_sd, dtype=np.int64)
    if d.ndim == 3:
        d, hm, hs = d[None], hm[None], hs[None]
    nc, Pm = d.shape[0], mu_grid.shape[0]
    sg = np.ones(nc, dtype=np.int64) if signs is None else np.asarray(signs, dtype=np.int64).reshape(nc)
    for c in range(nc):
        if sg[c] < 0:
            hm[c] = hm[c, ::-1]
            a = d[c, :, :, 0]
            d[c, :, :, 0] = np.where(a >= 0, Pm - 1 - a, a)
    hm, hs = hm.sum(axis=0), hs.sum(axis=0)

    def moments(hist, grid):
        total = hist.sum(axis=0)
        with np.errstate(all="ignore"):
            w = hist.astype(LD) / total.astype(LD)[None, :]
            mean = (w * grid.astype(LD)[:, None]).sum(axis=0)
            var = (w * (grid.astype(LD)[:, None] - mean[None, :]) ** 2).sum(axis=0)
        cum = np.cumsum(hist, axis=0)
        qs = {}
        for p in probs:
            need = np.ceil(float(p) * total)
            pos = np.array([int(np.searchsorted(cum[:, g], need[g], side="left")) for g in range(hist.shape[1])])
            qs[float(p)] = np.where(total > 0, grid[pos.clip(0, grid.shape[0] - 1)], np.nan)
        return mean.astype(np.float64), np.sqrt(var).astype(np.float64), qs

    mm, ms, mq = moments(hm, mu_grid)
    sm, ss, sq = moments(hs, sd_grid)
    return dict(hist_mu=hm, hist_sd=hs, draws=d if np.ndim(draws) == 4 else d[0], mu_mean=mm, mu_sd=ms, mu_quantiles=mq, sd_mean=sm,
                sd_sd=ss, sd_quantiles=sq)


# ------------------------------------------------------------------------------------------------ synthetic groups ---
def make_grouped(n, m, codes, mu, sd, seed=20240, na_frac=0.05):
    """gpirt_amd.synthetic.make_responses with theta_i ~ N(mu[g_i], sd[g_i]^2): returns (y, theta_init, theta_true).  theta_init
    is a standard normal snapped to the grid, as there."""
    rng = np.random.default_rng(seed)
    cd = np.asarray(codes, dtype=np.int64)
    theta_true = np.asarray(mu, dtype=np.float64)[cd] + np.asarray(sd, dtype=np.float64)[cd] * rng.standard_normal(n)
    a = rng.uniform(-2.0, 2.0, m)
    b = rng.uniform(0.5, 3.0, m)
    y = np.empty((n, m), order="F")
    for j in range(m):
        while True:
            p = 1.0 / (1.0 + np.exp(-(a[j] + b[j] * theta_true)))
            col = np.where(rng.random(n) < p, 1.0, -1.0)
            col[rng.random(n) < na_frac] = np.nan
            if len(np.unique(col[~np.isnan(col)])) == 2:
                break
            a[j] = rng.uniform(-2.0, 2.0)
        y[:, j] = col
    k = np.clip(np.rint((rng.standard_normal(n) + 5.0) / 0.01), 0, 1000)
    return y, -5.0 + k * 0.01, theta_true


# ------------------------------------------------------------------------------------------------ one call per run ---
def run(y, sample_iterations, burn_iterations, groups=None, chains=1, seed=1, mu_hi=3.0, points_mu=121, sd_lo=0.2, sd_hi=5.0,
        points_sd=65, log_hyper_mu=None, log_hyper_sd=None, anchor_row=None, a0=None, b0=None, fixed=None, align=True,
        theta_init=None, preset="fast", *, handle=None, consistent=False, **sampler_kw) -> dict:
    """`chains` chains of the stage-driven Sampler, one after the other, each with a population prior over the groups `groups`
    (one code per respondent in 0 .. G - 1): per iteration step() then draw_pop(), and per kept draw pop_record().  Chain c runs
    with the seed chain_seed(seed, c) from gpirtMCMC(chains=...)'s default init.

    fixed: a G x 1001 table -- the chains run with Sampler.pop_set(groups, fixed) and no update; res["pop"] then holds
    mode="fixed" alone.

    Returns theta (chains x S x n; S x n for one chain), group_theta_mean (chains x S x G: the mean of each group's theta per
    kept draw), diagnostics and reflected (gpirt_amd.chains.combine's, align as there), consistent, chains, and pop: mode
    ("sampled"), draws (chains x S x G x 2, a reflected chain's mu indices mirrored; S x G x 2 for one chain), mu and sd
    (mu_grid[a], sd_grid[b] of the draws; NaN for the anchor), hist_mu (P_mu x G), hist_sd (P_sd x G) pooled over the chains,
    mu_mean, mu_sd, mu_quantiles, sd_mean, sd_sd, sd_quantiles per group (`summarise`), counts per chain (4 x G), off_grid (the
    last call's, per chain), mu_grid, sd_grid.

    consistent=True: every iteration is Sampler.step(consistent=True) (gpirt_amd.consistent)."""
    from . import chains as CH
    from .ops import Handle
    from .sampler import Sampler, _options
    y = np.asfortranarray(np.asarray(y, dtype=np.float64))
    n = y.shape[0]
    S, B, nc = int(sample_iterations), int(burn_iterations), int(chains)
    if nc < 1 or S < 1 or B < 0:
        raise ValueError("pop.run: chains >= 1, sample_iterations >= 1 and burn_iterations >= 0 are needed")
    if groups is None:
        raise ValueError("pop.run: groups (one code per respondent) is needed")
    codes = np.ascontiguousarray(groups, dtype=np.int32).reshape(-1)
    if codes.shape != (n,):
        raise ValueError(f"pop.run: groups must hold n = {n} codes")
    G = int(codes.max()) + 1
    sampled = fixed is None
    # the refusals that need no device, before anything is created: they name their reason (gpirt_pop_check)
    o = _options(sampler_kw.get("rng", "item"), seed, True, True, None, sampler_kw.get("item0", 0), sampler_kw.get("m_total", 0),
                 sampler_kw.get("kernel_fp32", False), 0)
    if sampled:
        check_args(codes, G, anchor_row, True, mu_hi, points_mu, sd_lo, sd_hi, points_sd, log_hyper_mu, log_hyper_sd, a0, b0, options=o)
        mu_grid, sd_grid = grids(mu_hi, points_mu, sd_lo, sd_hi, points_sd)
    else:
        check_args(codes, G, fixed, False, options=o)
    inits = CH.default_inits(n, nc, seed) if theta_init is None else np.asarray(theta_init, dtype=np.float64).reshape(nc, -1)
    if inits.shape != (nc, n):
        raise ValueError("theta_init must have one value per respondent (and chain)")
    own = handle is None
    h = Handle() if own else handle
    samplers = []
    try:
        th = np.empty((nc, S, n))
        gm = np.empty((nc, S, G))
        draws = np.empty((nc, S, G, 2), dtype=np.int32)
        hms, hss, counts, offs = [], [], [], []
        for c in range(nc):
            s = Sampler(h, y, inits[c], seed=seed if c == 0 else _lib.chain_seed(seed, c), preset=preset, **sampler_kw)
            samplers.append(s)
            s.init()
            s.check()
            if sampled:
                s.pop_enable(codes, G, anchor_row, mu_hi, points_mu, sd_lo, sd_hi, points_sd, log_hyper_mu, log_hyper_sd, a0, b0,
                             planned_draws=S)
            else:
                s.pop_set(codes, fixed)
            s.summary_enable(_lib.SUM_THETA_BETA | _lib.SUM_DIAG, planned_draws=S)
            for it in range(S + B):
                s.step(consistent=consistent)
                if sampled:
                    s.draw_pop()
                if it >= B:
                    s.accumulate_irf()
                    s.summary_accumulate()
                    t = s.get("theta")
                    th[c, it - B] = t
                    gm[c, it - B] = [t[codes == g].mean() for g in range(G)]
                    if sampled:
                        s.pop_record()
            s.check()
            if sampled:
                draws[c] = s.pop_get("draws")
                hms.append(s.pop_get("hist_mu"))
                hss.append(s.pop_get("hist_sd"))
                counts.append(s.pop_get("counts"))
                offs.append(s.pop_get("off_grid"))
        pooled = CH.combine(h, samplers, align=align)
        refl = pooled["diagnostics"]["reflected"]
        if sampled:
            pop = summarise(draws, np.array(hms), np.array(hss), mu_grid, sd_grid, signs=[-1 if r else 1 for r in refl])
            d = pop["draws"]
            with np.errstate(invalid="ignore"):
                pop["mu"] = np.where(d[..., 0] >= 0, mu_grid[d[..., 0].clip(0)], np.nan)
                pop["sd"] = np.where(d[..., 1] >= 0, sd_grid[d[..., 1].clip(0)], np.nan)
            if nc == 1:
                pop.update(draws=d[0], mu=pop["mu"][0], sd=pop["sd"][0])
            pop.update(mode="sampled", counts=np.array(counts), off_grid=np.array(offs), mu_grid=mu_grid, sd_grid=sd_grid)
        else:
            pop = dict(mode="fixed")
        return dict(theta=th if nc > 1 else th[0], group_theta_mean=gm if nc > 1 else gm[0], diagnostics=pooled["diagnostics"],
                    reflected=refl, consistent=bool(consistent), chains=nc, groups=G, pop=pop)
    finally:
        for s in samplers:
            s.close()
        if own:
            h.close()


__all__ = ["theta_grid", "default_row", "normal_table", "grids", "lse_table", "check_args", "uniforms", "grid_index", "stats_exact",
           "lp_mu_row", "lp_sd_row", "grid_draw_exact", "step_exact", "conditional", "summarise", "make_grouped", "run"]
