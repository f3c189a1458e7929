"""Derived bounds and the shared constructed cases of the length-scale tests (tests/test_ell_cpu.py, tests/test_gpu_ell.py).

DEVICE AGAINST gpirt_amd.ell.step_exact, ONE UPDATE FROM THE SAME f.  u = 2^-53.  Both sides factor S_k = K(theta, theta;
ell_k) + 0.001 I in fp64 (the device's blocked factorisation, NumPy's LAPACK call); everything after that is fp64 on the device
and long double in the reference.  For a computed Cholesky factor L + dL of S, (L + dL)(L + dL)^T = S + dS with
|dS| <= (n + 1) u |L| |L^T| (Higham, Accuracy and Stability, thm 10.3), so ||dS||_F <= (n + 1) u ||L||_F^2 = (n + 1) u tr(S); the
entries of S themselves differ between the two builds by a few u each (tests/_kernel_exact.py), n times less in this norm.  To
first order L^-1 dL is the lower part of L^-1 dS L^-T, hence
    ||L^-1 dL||_F <= ||dS||_F / lmin(S) <= (n + 1) u tr(S) / lmin(S) =: A(S)                    per factor, 2 A between the two.
nu = L^-1 f:       nu_dev - nu_ref = -L^-1 (L_dev - L_ref) nu + the solve's own rounding (n u kF ||nu||, kF = ||L||_F ||L^-1||_2 =
                   sqrt(tr(S) / lmin(S)), a substitution's backward error)
                   ||d nu_j||_2 <= (2 A(S_k) + n u kF_k) ||nu_j||_2 =: e_nu_j
f' = L' nu:        ||d f'_j||_2 <= ||L'||_2 e_nu_j + ||L'||_2 2 A(S_k') ||nu_j||_2 + n u ||L'||_F ||nu_j||_2 =: e_fp_j
                   (the solve's error through the product, the two factors' difference, the product's own rounding)
delta_j:           t(a) = log(1 + exp(-a)) is 1-Lipschitz, so the change of f' moves delta_j by at most ||d f'_j||_1 <= sqrt(n)
                   e_fp_j; the terms themselves: the argument y (f + mu) carries 2 u |a|, ll_term_fast 2 ulp of t (csrc/ll_fast.h),
                   the difference one more rounding, the 256 + 8 additions of a column (n / 256 + 9) u sum |term|:
                   e_delta_j = sqrt(n) e_fp_j + sum_i [2 u (|a0| + |a1|) + 5 u (t0 + t1)] + (n / 256 + 9) u sum_i |t0 - t1|
dll, log_ratio:    e_dll = sum_j e_delta_j + m u sum_j |delta_j|;  e_ratio = e_dll + 2 u (|dll| + |lp' - lp|)
max-abs figures are held under these 2-norm bounds (||x||_inf <= ||x||_2).

A TRAJECTORY of T updates with no step() in between.  Each side solves with the factor it multiplied by: nu_(t+1) =
L'^-1 fl(L' nu_t) moves nu by the product's and the solve's rounding alone, (2 n + 1) u kF ||nu|| per update and side -- the
difference of the two sides' factors does not accumulate.  So after t updates
    ||nu_dev,t - nu_ref,t||_2 <= e_nu (the first solve) + 2 t (2 n + 1) u kF_max ||nu||_2 =: e_nu(t)
and both f and f' carry e_fp with e_nu(t) in place of e_nu and the worst factor of the grid; delta moves by the two of them.
(The device's solve applies explicit inverses of L's diagonal blocks; that its error obeys the substitution's bound is this
file's assumption -- the measured figures are printed beside the bounds.)

STAGE BY STAGE, GIVEN THE DEVICE'S OWN FACTORS (the sharper layer: what the two factorisations differ by does not enter, so the
bounds are the stages' own rounding and an error of the wrong order in one stage shows).  L and L' are the device's factors
under ell_k and ell_k' (a fresh sampler's factor is bit for bit the proposal's: test_state_after_accept_...), each stage's
reference takes the device's output of the stage before it, in long double:
    nu against L^-1 f:         ||d nu_j||_2 <= n u kF ||nu_j||_2      (a substitution's backward error |dL| <= n u |L|, as above)
    f' against L' nu_dev:      |d f'_ij| <= (n + 2) u sum_k |L'_ik| |nu_kj|      (any order of the n additions, fused or not)
    delta against the terms of (f, f'_dev):   the term and addition errors of e_delta alone, without sqrt(n) e_fp
    dll against sum_j delta_dev_j:   m u sum_j |delta_j|;     log_ratio against dll_dev + (lp' - lp):   2 u (|dll| + |lp' - lp|)

THE CHAIN AGAINST conditional_posterior.  With nu fixed the update is a Metropolis chain on P states with stationary mass p.
The frequency of state k over T updates has variance p_k (1 - p_k) tau / T, tau = T / ESS the chain's integrated
autocorrelation time (gpirt_amd.acf.from_draws on the index series); a 4-sigma band per state holds all P of them together with
probability > 1 - P 6.4e-5, and total variation is half the sum of the deviations:
    TV <= 0.5 sum_k 4 sqrt(p_k (1 - p_k) / ESS).
"""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
SEED = 5                      # the trajectory's seed: chosen so that no update of the 4000 is a near-tie (test_ell_cpu.py asserts it)
P, W, N, M = 17, 2, 40, 3     # the trajectory case of the issue
LO, HI = 0.25, 4.0


def case(n, m, points, seed, family="se", lo=LO, hi=HI, k=None, nan_share=0.05):
    """A constructed state on the grid of theta: theta, beta, mu, f = L_k nu0 (fp64), y (+1 / -1, `nan_share` NaN), the grid,
    the default prior and the starting index k (default: the middle)."""
    from gpirt_amd import ell as E
    rng = np.random.default_rng(seed)
    theta = np.round(rng.standard_normal(n).clip(-4, 4), 2)
    g = E.grid(lo, hi, points)
    lp = E.default_log_prior(g)
    k = points // 2 if k is None else k
    beta = np.stack([rng.normal(0, 1, m), rng.normal(1, 0.3, m)])
    mu = beta[0][None, :] + beta[1][None, :] * theta[:, None]
    L = E.factor(theta, family, g[k])
    f = (L @ rng.standard_normal((n, m)).astype(LD)).astype(np.float64)
    p = 1 / (1 + np.exp(-(f + mu)))
    y = np.where(rng.random((n, m)) < p, 1.0, -1.0)
    y[rng.random((n, m)) < nan_share] = np.nan
    return dict(theta=theta, beta=beta, mu=np.asfortranarray(mu), f=np.asfortranarray(f), y=np.asfortranarray(y), grid=g,
                log_prior=lp, k=k, family=family, n=n, m=m, points=points, seed=seed, lo=lo, hi=hi)


def chain(c, width, updates, seed=None):
    """The NumPy chain from a case: `updates` step_exact calls with no step() in between.  Returns the per-update records
    (status, k, margin = |log_ratio - log u1| or None), the final f, nu of the first solve and the factor cache."""
    from gpirt_amd import ell as E
    seed = c["seed"] if seed is None else seed
    k, f, cache, rec = c["k"], c["f"], {}, []
    nu0 = E.solve_lower(E._factor_of(cache, c["theta"], c["family"], c["grid"], k), f)
    for t in range(1, updates + 1):
        u0, u1 = E.uniforms(seed, t)
        r = E.step_exact(c["theta"], f, c["mu"], c["y"], k, u0, u1, c["grid"], c["log_prior"], width, c["family"], cache)
        k, f = r["k"], r["f"]
        rec.append(dict(status=r["status"], k=k, k_prop=r["k_prop"],
                        margin=abs(float(r["log_ratio"] - r["log_u"])) if "log_ratio" in r else None,
                        dll=float(r["dll"]) if "dll" in r else None))
    return dict(records=rec, f=f, k=k, nu0=nu0, cache=cache)


def factor_constants(theta, family, ell):
    """A(S), kF, ||L||_2, ||L||_F of the reference factor under one length scale"""
    from gpirt_amd import ell as E
    L = E.factor(theta, family, ell).astype(np.float64)
    n = L.shape[0]
    sv = np.linalg.svd(L, compute_uv=False)
    lmin, tr = float(sv[-1]) ** 2, float((L * L).sum())
    return dict(A=(n + 1) * U * tr / lmin, kF=float(np.sqrt(tr / lmin)), L2=float(sv[0]), LF=float(np.sqrt(tr)))


def update_bounds(c, k, kp, ref, steps=0, worst=None):
    """The bounds of the module docstring for the update k -> kp of case c, from the reference's own record `ref` (step_exact's
    dict).  steps > 0: after that many earlier updates of a trajectory, with `worst` = the grid's worst constants (both f and
    f' then carry the drift)."""
    n, m = c["n"], c["m"]
    a, b = factor_constants(c["theta"], c["family"], c["grid"][k]), factor_constants(c["theta"], c["family"], c["grid"][kp])
    nu = np.asarray(ref["nu"], dtype=np.float64)
    nn = np.sqrt((nu * nu).sum(axis=0))                                   # ||nu_j||_2
    e_nu = (2 * a["A"] + n * U * a["kF"]) * nn
    if steps:
        e_nu = (2 * worst["A"] + n * U * worst["kF"]) * nn + 2 * steps * (2 * n + 1) * U * worst["kF"] * nn
        b = worst
    e_fp = b["L2"] * e_nu + b["L2"] * 2 * b["A"] * nn + n * U * b["LF"] * nn
    y = c["y"]
    obs = ~np.isnan(y)
    ys = np.where(obs, y, 0.0)
    from gpirt_amd import ell as E
    f0 = np.asarray(ref["f_in"], dtype=np.float64)
    a0, a1 = ys * (f0 + c["mu"]), ys * (np.asarray(ref["f_prop"], dtype=np.float64) + c["mu"])
    t0, t1 = E.ll_term(a0).astype(np.float64), E.ll_term(a1).astype(np.float64)
    terms = np.where(obs, 2 * U * (np.abs(a0) + np.abs(a1)) + 5 * U * (t0 + t1), 0.0).sum(axis=0)
    adds = (n / 256 + 9) * U * np.where(obs, np.abs(t0 - t1), 0.0).sum(axis=0)
    e_delta = np.sqrt(n) * e_fp * (2 if steps else 1) + terms + adds
    delta = np.asarray(ref["delta"], dtype=np.float64)
    e_dll = float(e_delta.sum() + m * U * np.abs(delta).sum())
    lpd = abs(float(c["log_prior"][kp] - c["log_prior"][k]))
    return dict(nu=e_nu, f_prop=e_fp, delta=e_delta, dll=e_dll, log_ratio=e_dll + 2 * U * (abs(float(ref["dll"])) + lpd))


def stage_bounds(c, L, Lp, dev, k, kp):
    """The stage-by-stage layer of the module docstring: L, Lp the device's factors (n x n fp64) under ell_k and ell_kp, dev the
    device's nu, f_prop, delta and record.  Returns name -> (error, bound) with each stage's reference computed in long double
    from the device's output of the stage before."""
    from gpirt_amd import ell as E
    n, m = c["n"], c["m"]
    Ld, Lpd = np.tril(L).astype(LD), np.tril(Lp).astype(LD)
    sv = np.linalg.svd(np.tril(L), compute_uv=False)
    kF = float(np.sqrt((np.tril(L) ** 2).sum()) / sv[-1])
    nu, fp, delta, rec = (np.asarray(dev[k_]) for k_ in ("nu", "f_prop", "delta", "record"))
    out = {}
    nu_ref = E.solve_lower(Ld, c["f"])
    e = np.sqrt((((nu.astype(LD) - nu_ref).astype(np.float64)) ** 2).sum(axis=0))
    out["nu"] = (e, n * U * kF * np.sqrt((nu ** 2).sum(axis=0)))
    out["f_prop"] = (np.abs(fp.astype(LD) - Lpd @ nu.astype(LD)).astype(np.float64), (n + 2) * U * (np.abs(np.tril(Lp)) @ np.abs(nu)))
    y = c["y"]
    obs = ~np.isnan(y)
    ys = np.where(obs, y, 0.0)
    a0, a1 = ys * (c["f"] + c["mu"]), ys * (fp + c["mu"])
    t0, t1 = E.ll_term(a0), E.ll_term(a1)
    d_ref = np.where(obs, t0 - t1, LD(0)).sum(axis=0)
    t0, t1 = t0.astype(np.float64), t1.astype(np.float64)
    tol = np.where(obs, 2 * U * (np.abs(a0) + np.abs(a1)) + 5 * U * (t0 + t1), 0.0).sum(axis=0) + \
        (n / 256 + 9) * U * np.where(obs, np.abs(t0 - t1), 0.0).sum(axis=0)
    out["delta"] = (np.abs(delta.astype(LD) - d_ref).astype(np.float64), tol)
    out["dll"] = (abs(float(LD(rec[0]) - delta.astype(LD).sum())), m * U * float(np.abs(delta).sum()))
    lpd = LD(c["log_prior"][kp]) - LD(c["log_prior"][k])
    out["log_ratio"] = (abs(float(LD(rec[1]) - (LD(rec[0]) + lpd))), 2 * U * (abs(float(rec[0])) + abs(float(lpd))))
    return out


def worst_constants(c):
    """the largest A, kF, ||L||_2 and ||L||_F over the grid of case c"""
    cs = [factor_constants(c["theta"], c["family"], e) for e in c["grid"]]
    return {k: max(x[k] for x in cs) for k in ("A", "kF", "L2", "LF")}


def trajectory_ratio_bound(c, nu0, updates):
    """the largest device-versus-reference error of log_ratio any update of a `updates`-long trajectory of case c can carry: the
    update bound with the grid's worst constants and the drift of all `updates` steps, the term errors at |a| <= 40, t <= 40"""
    n, m = c["n"], c["m"]
    w = worst_constants(c)
    nn = np.sqrt((np.asarray(nu0, dtype=np.float64) ** 2).sum(axis=0)) * (1 + 1e-6)
    e_nu = (2 * w["A"] + n * U * w["kF"]) * nn + 2 * updates * (2 * n + 1) * U * w["kF"] * nn
    e_fp = w["L2"] * e_nu + w["L2"] * 2 * w["A"] * nn + n * U * w["LF"] * nn
    terms = n * (2 * U * 80 + 5 * U * 80) + (n / 256 + 9) * U * n * 40
    e_dll = float((2 * np.sqrt(n) * e_fp + terms).sum()) + m * U * m * n * 40
    return e_dll + 2 * U * (m * n * 40 + 10), e_fp


def tv_bound(p, ess):
    p = np.asarray(p, dtype=np.float64)
    return float(0.5 * (4 * np.sqrt(p * (1 - p) / ess)).sum())


def index_ess(ks):
    """ESS of an index series by gpirt_amd.acf.from_draws: the indices enter as grid values of theta (-5 + 0.01 k), which the
    header's integer sums take exactly"""
    from gpirt_amd import acf as AC
    ks = np.asarray(ks, dtype=np.int64)
    r = AC.from_draws((-5.0 + 0.01 * ks).reshape(-1, 1), None, None, np.ones((1, 1)), max_lag=min(len(ks) // 2 - 1, 256))
    return float(r["ess"][0])
