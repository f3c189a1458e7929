"""Constructed states, derived error bounds and the NumPy chains for the tests of the collapsed scale and shift move
(include/gpirt_hip.h "a collapsed scale and shift move", csrc/scale.hip, gpirt_amd.scale).  Imported by tests/test_scale_cpu.py and
tests/test_gpu_scale.py; no GPU is needed here.

THE BOUNDS, from the header's order of operations, with u = 2^-53 (one rounding is at most u relative), the device library's
exp and log taken as within 1 ulp = 2 u relative (the ROCm device library documents 1 ulp for both in fp64), and every bound
multiplied by 1.01 for the second-order terms.  The reference is gpirt_amd.scale.step_exact: long double (u_L = 2^-64 and
below this file's interest) from the same fp64 logpost, prior rows and coefficients.

  lz_i.  w_k = exp(P_k - lz) are the masses, sum_k w_k = 1.
    P_k = fl(pr_k + lp_k)                one rounding: u |P_k|, which moves lz by at most sum_k w_k u |P_k|
    x_k = fl(P_k - M)                    u |x_k|; e_k = exp(x_k) within 2 u: relative (|x_k| + 2) u on each term, so
                                         sum_k w_k (|x_k| + 2) u on log S
    S                                    three additions in the thread and eight levels of the tree: every term passes at most
                                         eleven additions of positive numbers, relative 11 u on S, so 11 u on log S
    log(S)                               S lies in [1, N - 1] (the largest term is exp(0) = 1): 2 u log(S)
    lz = fl(M + log S)                   u |lz|
    E_lz = 1.01 u (sum_k w_k (|P_k| + |x_k|) + 13 + 2 log S + |lz|)
  dlz_i = fl(lz' - lz):                  E_dlz = E_lz + E_lz' + u |dlz|
  D = sum_i dlz_i:                       row order, ceil(n / 256) additions in the thread and eight in the tree:
                                         E_D = sum_i E_dlz_i + 1.01 (ceil(n / 256) + 8) u sum_i |dlz_i|
  ldn(x; pm, ps) = -(c + 0.5 z^2 + log ps), z = |(x - pm) / ps|:  z within 2 u, 0.5 z^2 within 5 u (0.5 z^2), log ps within
                                         2 u |log ps|, the two additions u (c + 0.5 z^2) and u |ldn|:
                                         E_ldn = 1.01 u (3.5 z^2 + 3 |log ps| + 2 c)
  q_j = fl(ldn' - ldn):                  E_q = E_ldn' + E_ldn + u |q_j|;  Q in ascending j: E_Q = sum_j E_q + 1.01 (m - 1) u sum_j |q_j|
  J = fl(m step):                        E_J = u |J| (0 for the shift)
  log r = fl(fl(D + Q) - J):             E_r = E_D + E_Q + E_J + 1.01 u (|D + Q| + |log r|)
  log u:                                 E_u = 2.02 u |log u|
A decision is safe when |log u - log r| >= MARGIN (E_r + E_u); the constructed cases are held to that here on the CPU.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SLACK = 1.01
MARGIN = 100.0
NS = (2, 255, 256, 257, 1025)
MS = (1, 5, 33)
SEED = 20261
WIDTH = {"scale": 0.03, "shift": 0.05}
LN_SQRT_2PI = 0.918938533204672741780329736406


# ------------------------------------------------------------------------------------------------ constructed states ---
def pop_table():
    """a two-group table of log masses on the grid: N(-0.5, 0.8^2) and N(0.7, 1.2^2), normalised over all N points"""
    from gpirt_amd import scale as SC
    rows = []
    for mu, sd in ((-0.5, 0.8), (0.7, 1.2)):
        lp = -0.5 * ((SC.GRID - mu) / sd) ** 2
        rows.append(lp - np.log(np.exp(lp).sum()))
    return np.ascontiguousarray(np.stack(rows))


def state(n, m, seed=SEED):
    """theta on the grid with both end points, answers of +1 / -1 with a tenth missing (every respondent keeps an answer), beta,
    a smooth hstar, and mu_star, mu and fstar in the library's expressions and bits; priors off centre"""
    from gpirt_amd import scale as SC
    rng = np.random.default_rng(seed + 37 * n + m)
    idx = np.clip(np.round(500 + 100 * rng.standard_normal(n)).astype(int), 0, 1000)
    idx[0], idx[-1] = 0, 1000
    theta = SC.GRID[idx].copy()
    b0, b1 = rng.uniform(-1, 1, m), rng.uniform(0.6, 1.6, m)
    beta = np.asfortranarray(np.stack([b0, b1]))
    hstar = np.asfortranarray(0.5 * np.sin(SC.GRID[:, None] * rng.uniform(0.5, 1.5, m)[None, :] + rng.uniform(0, 6, m)[None, :]))
    eta = b0[None, :] + b1[None, :] * theta[:, None] + hstar[idx]
    y = np.where(rng.random((n, m)) < 1 / (1 + np.exp(-eta)), 1.0, -1.0)
    miss = rng.random((n, m)) < 0.1
    miss[np.arange(n), rng.integers(0, m, n)] = False
    y[miss] = np.nan
    mu_star = np.asfortranarray(b0[None, :] + SC.GRID[:, None] * b1[None, :])
    mu = np.asfortranarray(b0[None, :] + theta[:, None] * b1[None, :])
    fstar = np.asfortranarray(hstar + mu_star)
    pm = np.asfortranarray(np.stack([np.full(m, 0.2), np.full(m, 1.0)]))
    ps = np.asfortranarray(np.stack([np.full(m, 1.5), np.full(m, 0.8)]))
    codes = (np.arange(n) % 2).astype(np.int32)
    return dict(n=n, m=m, theta=theta, y=np.asfortranarray(y), beta=beta, hstar=hstar, mu_star=mu_star, mu=mu, fstar=fstar, pm=pm, ps=ps,
                codes=codes, seed=seed)


def loglik_grid64(y, fstar):
    """logpost (N x n) in fp64 by two products, for the margin check and the chains (gpirt_amd.scale.loglik_grid is the long-double
    one): G+ = -log(1 + exp(-f*)), G- = -log(1 + exp(f*)), logpost = G+ Y+^T + G- Y-^T"""
    f = np.asarray(fstar, dtype=np.float64)
    gp = -(np.maximum(-f, 0) + np.log1p(np.exp(-np.abs(f))))
    gm = -(np.maximum(f, 0) + np.log1p(np.exp(-np.abs(f))))
    return gp @ (y == 1.0).astype(np.float64).T + gm @ (y == -1.0).astype(np.float64).T


def lprior_rows(c, pop):
    from gpirt_amd import scale as SC
    return pop_table()[c["codes"]] if pop else SC.default_lprior()


# ------------------------------------------------------------------------------------------------------- the bounds ---
def lz_bound(logpost, lprior, lz):
    """E_lz (n) for fp64 logpost (N x n), the prior rows (N or n x N) and the long-double lz"""
    lp = np.asarray(logpost, dtype=np.float64)
    N, n = lp.shape
    pr = np.asarray(lprior, dtype=np.float64)
    pr = np.broadcast_to(pr, (n, N)) if pr.ndim == 1 else pr
    P = (pr.T + lp)[1:].astype(LD)
    lzL = np.asarray(lz, dtype=LD)
    M = P.max(axis=0)
    w = np.exp(P - lzL[None, :])
    logS = (lzL - M).astype(np.float64)
    first = (w * (np.abs(P) + np.abs(P - M[None, :]))).sum(axis=0).astype(np.float64)
    return SLACK * U * (first + 13.0 + 2.0 * logS + np.abs(lzL.astype(np.float64)))


def ldn_bound(x, pm, ps):
    z = np.abs((np.asarray(x, dtype=np.float64) - pm) / ps)
    return SLACK * U * (3.5 * z * z + 3.0 * np.abs(np.log(ps)) + 2.0 * LN_SQRT_2PI)


def decision_bounds(ex, logpost, logpost_prop, lprior, beta, beta_prop, pm, ps, kind) -> dict:
    """E_lz, E_lz', E_dlz (n), E_D, E_Q, E_r, E_u for the statement `ex` (gpirt_amd.scale.step_exact's dict)"""
    n = ex["lz"].size
    q = 1 if kind in ("scale", 0) else 0
    b, bp = np.asarray(beta, dtype=np.float64).reshape(2, -1), np.asarray(beta_prop, dtype=np.float64).reshape(2, -1)
    m = b.shape[1]
    pm, ps = np.asarray(pm, dtype=np.float64).reshape(2, m), np.asarray(ps, dtype=np.float64).reshape(2, m)
    e_lz, e_lzp = lz_bound(logpost, lprior, ex["lz"]), lz_bound(logpost_prop, lprior, ex["lz_prop"])
    dlz = np.abs(ex["dlz"].astype(np.float64))
    e_dlz = e_lz + e_lzp + U * dlz
    e_D = float(e_dlz.sum() + SLACK * (-(-n // 256) + 8) * U * dlz.sum())
    from gpirt_amd import scale as SC
    qj = np.abs((SC.ldn(bp[q].astype(LD), pm[q].astype(LD), ps[q].astype(LD)) - SC.ldn(b[q].astype(LD), pm[q].astype(LD), ps[q].astype(LD))).astype(np.float64))
    e_q = ldn_bound(bp[q], pm[q], ps[q]) + ldn_bound(b[q], pm[q], ps[q]) + U * qj
    e_Q = float(e_q.sum() + SLACK * (m - 1) * U * qj.sum())
    e_J = U * abs(float(ex["J"]))
    e_r = e_D + e_Q + e_J + SLACK * U * (abs(float(ex["D"] + ex["Q"])) + abs(float(ex["log_r"])))
    e_u = 2.0 * SLACK * U * abs(float(ex["log_u"]))
    return dict(lz=e_lz, lz_prop=e_lzp, dlz=e_dlz, D=e_D, Q=e_Q, log_r=e_r, log_u=e_u)


def case_on_cpu(n, m, kind, pop, t=1, seed=SEED):
    """the constructed case's statement evaluated here (fp64 logposts by loglik_grid64): (state, proposal, statement, bounds, u)"""
    from gpirt_amd import scale as SC
    c = state(n, m, seed)
    z, u = SC.normals(seed, t, kind)
    pr = SC.proposal(c["beta"], kind, WIDTH[kind], z)
    f2 = SC.curve(c["fstar"], c["mu_star"], pr["mu"])
    lp, lp2 = loglik_grid64(c["y"], c["fstar"]), loglik_grid64(c["y"], f2)
    rows = lprior_rows(c, pop)
    ex = SC.step_exact(lp, lp2, c["beta"], pr["beta"], c["pm"], c["ps"], kind, pr["step"], u, lprior=rows)
    bd = decision_bounds(ex, lp, lp2, rows, c["beta"], pr["beta"], c["pm"], c["ps"], kind)
    return c, pr, ex, bd, u


# ------------------------------------------------------------------------------- prior invariance: the NumPy chain ---
PI_M, PI_REPS, PI_CALLS, PI_SDS = 64, 300, 40, 5.0
PI_PM, PI_PS = (0.5, 1.0), (0.5, 0.15)
PI_W = (0.04, 0.08)


def pi_priors(m=PI_M):
    pm = np.asfortranarray(np.stack([np.full(m, PI_PM[0]), np.full(m, PI_PM[1])]))
    ps = np.asfortranarray(np.stack([np.full(m, PI_PS[0]), np.full(m, PI_PS[1])]))
    return pm, ps


def pi_zscores(finals, pm, ps):
    """finals (R x 2 x m): the coefficients at the end of R independent replicates that started from the prior.  If the move
    leaves the prior invariant every final kappa = (beta - pm) / ps is an independent N(0, 1) draw, so over the R m values per
    coefficient: the mean (variance 1 / (R m)), the mean of kappa^2 - 1 (variance 2 / (R m)), and the mean of kappa_0 kappa_1
    (variance 1 / (R m)) -- five z-scores."""
    k = (np.asarray(finals) - pm[None]) / ps[None]
    R, _, m = k.shape
    cnt = R * m
    return np.array([k[:, 0].mean() * np.sqrt(cnt), k[:, 1].mean() * np.sqrt(cnt), (k[:, 0] ** 2 - 1).mean() * np.sqrt(cnt / 2),
                     (k[:, 1] ** 2 - 1).mean() * np.sqrt(cnt / 2), (k[:, 0] * k[:, 1]).mean() * np.sqrt(cnt)])


def pi_chain(variant="right", reps=PI_REPS, calls=PI_CALLS, m=PI_M, seed=5):
    """R replicates of `calls` alternating scale / shift calls with every answer missing (dlz = 0: the prior and the Jacobian
    decide), each from a fresh draw of the prior; variant "no_jacobian" leaves out -m eps, "shift_reversed" moves the intercepts
    by -b1 delta while the ratio is the stated move's.  Returns (finals, accepted share)."""
    from gpirt_amd import scale as SC
    rng = np.random.default_rng(seed)
    pm, ps = pi_priors(m)
    finals, acc = np.empty((reps, 2, m)), 0
    for r in range(reps):
        b = pm + ps * rng.standard_normal((2, m))
        for t in range(calls):
            kind = t % 2
            z, u = rng.standard_normal(), rng.random()
            pr = SC.proposal(b, kind, PI_W[kind], z)
            q = 1 if kind == 0 else 0
            Q = float((SC.ldn(pr["beta"][q], pm[q], ps[q]) - SC.ldn(b[q], pm[q], ps[q])).sum())
            J = 0.0 if variant == "no_jacobian" else pr["jacobian"]
            if np.log(u) < Q + J:
                acc += 1
                if variant == "shift_reversed" and kind == 1:
                    b = b.copy()
                    b[0] = b[0] - b[1] * pr["step"]
                else:
                    b = pr["beta"]
        finals[r] = b
    return finals, acc / (reps * calls)


# ---------------------------------------------------------------------------- the collapsed target: chain, quadrature ---
CT_N, CT_M, CT_MOVES = 40, 4, 20000
CT_W = {"scale": 0.25, "shift": 0.3}


def ct_state():
    c = state(CT_N, CT_M, seed=77)
    return c


def ct_chain(kind, moves=CT_MOVES, seed=3):
    """`moves` calls of one kind on the statement with hstar and y fixed (fp64 logposts): the accumulated step after every call"""
    from gpirt_amd import scale as SC
    c = ct_state()
    rng = np.random.default_rng(seed)
    rows = SC.default_lprior()
    beta, x = c["beta"].copy(), 0.0
    mu_star = c["mu_star"]
    lp = loglik_grid64(c["y"], c["hstar"] + mu_star)
    lz = SC.log_normalisers(lp, rows, order="device")
    out, acc = np.empty(moves), 0
    q = 1 if kind == "scale" else 0
    for t in range(moves):
        z, u = rng.standard_normal(), rng.random()
        pr = SC.proposal(beta, kind, CT_W[kind], z)
        lz2 = SC.log_normalisers(loglik_grid64(c["y"], c["hstar"] + pr["mu"]), rows, order="device")
        Q = float((SC.ldn(pr["beta"][q], c["pm"][q], c["ps"][q]) - SC.ldn(beta[q], c["pm"][q], c["ps"][q])).sum())
        if np.log(u) < float((lz2 - lz).sum()) + Q + pr["jacobian"]:
            beta, lz, x, acc = pr["beta"], lz2, x + pr["step"], acc + 1
        out[t] = x
    return out, acc / moves


def ct_quadrature(kind, lo=-1.5, hi=1.5, points=601):
    """mean and variance of the accumulated step under gpirt_amd.scale.collapsed_density by the trapezoid rule on [lo, hi]"""
    from gpirt_amd import scale as SC
    c = ct_state()
    xs = np.linspace(lo, hi, points)
    ld = np.array([SC.collapsed_density(x, kind, c["hstar"], c["beta"], c["y"], c["pm"], c["ps"]) for x in xs])
    w = np.exp(ld - ld.max())
    w[0] *= 0.5
    w[-1] *= 0.5
    w /= w.sum()
    mean = float((w * xs).sum())
    return mean, float((w * (xs - mean) ** 2).sum()), float(w[0] + w[-1])


def mcse(x, batches=50):
    """batch-means standard errors of the mean and of the variance of a series"""
    x = np.asarray(x, dtype=np.float64)
    L = x.size // batches
    b = x[:L * batches].reshape(batches, L)
    mu = x.mean()
    return float(b.mean(axis=1).std(ddof=1) / np.sqrt(batches)), float(((b - mu) ** 2).mean(axis=1).std(ddof=1) / np.sqrt(batches))
