"""Derived bounds, the constructed cases and the prior-invariance chain of the centred amplitude update's tests
(tests/test_amp_centred_cpu.py, tests/test_gpu_amp_centred.py).

DEVICE AGAINST gpirt_amd.amp.centred_exact_coef (long double), u = 2^-53.  The statement's own rounding is 2^-64 and is not
counted.  V is fp64 on both sides by the same barycentric formula, q_k = w_k / (theta - c_k), V_k = q_k / sum q, whose sum the
device adds in another order than NumPy: with L_i = sum_k |V_ik| (the Lebesgue function at theta_i) either V_ik is within
u (4 + 66 L_i) |V_ik| of the exact quotient, so the two differ by at most e_V[i, k] = 2 u (4 + 66 L_i) |V_ik|.
    T = V^T f       n products added in some order (split-K parts, then the parts): (n + 2) u sum_i |V_ik| |f_ij|, and V's
                    difference: e_T[k, j] = sum_i ((n + 2) u |V_ik| + e_V[i, k]) |f_ij|.
    A = R R^T       A = F^T (V^T V) F + eps I.  The device's Gram sum (n terms), the two 64-term products, the Cholesky
                    factorisation (64 + 1) u and each substitution (64 u) are backward stable: together they act as a relative
                    perturbation of A of at most eps_A = 8 (n + 448 + 140 max_i L_i) u in norm -- the sums counted once each (n,
                    2 x 64, 65, 3 x 64 = 385 + n, rounded up to 448 + n), V's difference twice (2 x 70 L), a factor 8 for
                    |Phi|^T |Phi| against Phi^T Phi in norm and the 64 x 64 Frobenius norms.
                    With E = R^-1 dA R^-T, |E| <= kappa eps_A (kappa = cond_2 A), the perturbed factor is R G with G the factor of
                    I + E, |G - I|_F <= |E|_F <= 8 |E|_2.  So any vector R^-1 b moves by at most rho |R^-1 b| and any R^-T w by at
                    most |R^-1|_2 rho |w|, rho = 8 kappa eps_A, and |R^-1|_2 <= eps^-1/2 = 31.63 (A >= eps I).
    t = R^-1 F^T T  e_t = rho |t|_2 + 31.63 (|F|_2 |e_T[:, j]|_2 + 66 u | |F|^T |T_j| |_2)                      (2-norm, per item)
    w = t + sd z    z is the same bits (checked apart), sd z two fp64 products on both sides: e_w = e_t + 4 u (|t|_2 + |sd z|_2)
    xi = R^-T w     = A^-1 b + sd R^-T z with b = F^T T.  The first part is a solve with A, perturbed relatively by rho at most, and
                    takes b's error through |A^-1|_2 <= 1 / eps; the second moves by |R^-1|_2 rho |sd z|_2 <= 31.63 sqrt(eps) a_j
                    rho |z|_2 = a_j rho |z|_2; the substitution itself adds 66 u sqrt(kappa) |xi|_2:
                    e_xi = rho |A^-1 b|_2 + e_b / eps + a_j rho |z|_2 + 66 u sqrt(kappa) |xi|_2,
                    e_b = |F|_2 |e_T[:, j]|_2 + 66 u | |F|^T |T_j| |_2
    Q = |xi_live|^2 e_Q = 2 |xi|_2 e_xi + e_xi^2 + 66 u Q
    g = F xi        as Xh^T w on the device: e_g = |F|_2 (e_xi + rho |xi|_2) + 66 u | |F| |xi| |_2
    H = V g         e_H[i, j] = |V_i|_2 e_g[j] + sum_k (e_V[i, k] + 66 u |V_ik|) |g_kj|
At n = 1025: eps_A = 2e-12, kappa = 1e5, rho = 1e-5 and e_H a few thousandths -- the price of norm-wise worst cases: wide against what a correct kernel shows and narrow against a wrong one (a missing noise term, a wrong
triangle or a transposed factor move these quantities by order one).  The tests print the used fraction.

GIVEN THE DEVICE'S H AND Q the rest is gpirt_amd.amp.centred_exact_update's own bounds (its docstring): the draw is decided
where the cut u0 C_last clears the two neighbouring sums by their bounds, c and f' are bit for bit, dll carries
tests/_amp_bounds.py's e_dll and the decision is decided where |log u1 - dll| > e_dll + 2 u |log u1|.

PRIOR INVARIANCE.  With every answer missing the likelihood is constant, draw_f is an exact draw-preserving rotation under the
prior and the centred update must leave p(a) = the prior's mass on the grid invariant.  64 items are independent chains; every
5th index after round 200 of 2000 is kept (23040 draws), the 65-point grid is cut into 8 cells by linspace(0, 65, 9) and every
cell count must lie within 5 binomial standard deviations sqrt(N p (1 - p)) of N p.  The thinned draws are not independent; the
5 sds are the issue's margin for that, and the prototype measured z within -0.9 .. 2.4 where an exponent r - 1 in place of r gave
44 and a missing augmentation noise 1248.
"""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
RINV = 31.63                      # eps^-1/2 rounded up: |R^-1|_2 <= it
NS = [2, 63, 64, 65, 255, 256, 257, 1025]
MS = [1, 5]
SEED = 5                          # the constructed cases' sampler seed (tests/test_amp_centred_cpu.py asserts that the statement
                                  # alone leaves at most 2 % of the items undecided at every shape)
P = 33
LO, HI = 0.25, 4.0

# the prior-invariance configuration of the issue
PI_N, PI_M, PI_P, PI_LO, PI_HI = 64, 64, 65, 0.25, 4.0
PI_ROUNDS, PI_BURN, PI_THIN, PI_CELLS, PI_SDS = 2000, 200, 5, 8, 5.0


def case(n, m, seed=None):
    """A constructed state at n x m: on-grid theta with repeated values and both end points, beta, mu, amplitudes spread over
    the grid (indices from one end to the other), f = a_k L z + a nugget-free smooth curve, y of +1 / -1 with 5 % NaN."""
    from gpirt_amd import amp as A, ell as E
    rng = np.random.default_rng(1000 + 7 * n + m if seed is None else seed)
    theta = np.round(rng.standard_normal(n).clip(-4, 4), 2)
    theta[0] = -5.0
    theta[-1] = 5.0
    if n >= 4:
        theta[2] = theta[1]                                        # a repeated value
    g = A.grid(LO, HI, P)
    lp = A.default_log_prior(g)
    k = np.round(np.linspace(0, P - 1, m + 2)[1:-1]).astype(np.int64) if m > 1 else np.array([P // 3])
    beta = np.stack([rng.normal(0, 1, m), rng.normal(1, 0.3, m)])
    mu = beta[0][None, :] + beta[1][None, :] * theta[:, None]
    L = E.factor(theta, "se", 1.0).astype(np.float64)
    f = (L @ rng.standard_normal((n, m))) * g[k][None, :]
    pr = 1 / (1 + np.exp(-(f + mu)))
    y = np.where(rng.random((n, m)) < pr, 1.0, -1.0)
    y[rng.random((n, m)) < 0.05] = np.nan
    return dict(theta=theta, beta=beta, mu=np.asfortranarray(mu), f=np.asfortranarray(f), y=np.asfortranarray(y), grid=g,
                log_prior=lp, k=k, n=n, m=m, points=P, lo=LO, hi=HI)


def coef_bounds(ref, f, a, eps=1.0e-3):
    """dict(T (64 x m), t, w, xi, Q, g (m each, 2-norm over the coordinates but Q), H (n x m), rho) of the module docstring for a
    centred_exact_coef result `ref` on the state f (n x m fp64) with amplitudes a (m)"""
    V, F = ref["V"], ref["F"]
    f = np.abs(np.asarray(f, dtype=np.float64))
    n, m = f.shape
    aV = np.abs(V)
    leb = aV.sum(axis=1)
    e_V = 2 * U * (4 + 66 * leb)[:, None] * aV
    e_T = ((n + 2) * U * aV + e_V).T @ f
    eps_A = 8 * (n + 448 + 140 * leb.max()) * U
    kappa = ref["cond"]
    rho = 8 * kappa * eps_A
    nF = np.linalg.norm(F, 2)
    nrm = lambda x: np.linalg.norm(np.asarray(x, dtype=np.float64), axis=0)             # noqa: E731
    T = np.abs(np.asarray(ref["T"], dtype=np.float64))
    e_b = nF * nrm(e_T) + 66 * U * nrm(np.abs(F).T @ T)
    e_t = rho * nrm(ref["t"]) + RINV * e_b
    sdz = np.asarray(ref["w"] - ref["t"], dtype=np.float64)
    e_w = e_t + 4 * U * (nrm(ref["t"]) + nrm(sdz))
    from gpirt_amd.amp import _solve_lower
    xi_mean = _solve_lower(ref["R"], ref["t"], transposed=True)                           # A^-1 b
    e_xi = (rho * nrm(xi_mean) + e_b / eps + np.asarray(a, dtype=np.float64) * rho * nrm(ref["z"])
            + 66 * U * np.sqrt(kappa) * nrm(ref["xi"]))
    Q = np.asarray(ref["Q"], dtype=np.float64)
    e_Q = 2 * nrm(ref["xi"]) * e_xi + e_xi ** 2 + 66 * U * Q
    axi = np.abs(np.asarray(ref["xi"], dtype=np.float64))
    e_g = nF * (e_xi + rho * nrm(ref["xi"])) + 66 * U * nrm(np.abs(F) @ axi)
    ag = np.abs(np.asarray(ref["g"], dtype=np.float64))
    e_H = np.linalg.norm(V, axis=1)[:, None] * e_g[None, :] + (e_V + 66 * U * aV) @ ag
    return dict(T=e_T, t=e_t, w=e_w, xi=e_xi, Q=e_Q, g=e_g, H=e_H, rho=rho)


# ------------------------------------------------------------------------------------------- prior invariance -------
def pi_setup():
    """(theta, grid, log_prior, cell edges, the prior's mass per cell) of the prior-invariance chain"""
    from gpirt_amd import amp as A
    rng = np.random.default_rng(11)
    theta = np.round(rng.standard_normal(PI_N).clip(-4, 4), 2)
    g = A.grid(PI_LO, PI_HI, PI_P)
    lp = -(np.log(g) ** 2) / 0.5
    edges = np.linspace(0, PI_P, PI_CELLS + 1)
    w = np.exp(lp - lp.max())
    w /= w.sum()
    mass = np.histogram(np.arange(PI_P), bins=edges, weights=w)[0]
    return theta, g, lp, edges, mass


def pi_zscores(kept, edges, mass):
    """z per cell: (count - N p) / sqrt(N p (1 - p)) for the kept indices (any shape)"""
    kept = np.asarray(kept).ravel()
    N = kept.size
    cnt = np.histogram(kept, bins=edges)[0]
    return (cnt - N * mass) / np.sqrt(N * mass * (1 - mass))


def pi_chain_numpy(seed=3, exponent_shift=0, noise=True):
    """The chain in NumPy (fp64, NumPy's own generator): PI_ROUNDS rounds of {draw_f under a constant likelihood, the centred
    update of every item}, the kept indices (kept x PI_M).  exponent_shift and noise=False are the two wrong variants the issue
    names: r + shift in the proposal, and no augmentation noise."""
    from gpirt_amd import amp as A, fstar_free as FF
    theta, g, lp, edges, mass = pi_setup()
    rng = np.random.default_rng(seed)
    n, m, eps = PI_N, PI_M, 1.0e-3
    V = FF.basis(theta)
    F, live, r = A.centred_factor()
    Phi = V @ F
    S = Phi @ Phi.T + eps * np.eye(n)
    L = np.linalg.cholesky(S)
    R = np.linalg.cholesky(Phi.T @ Phi + eps * np.eye(64))
    Rinv = np.linalg.inv(R)
    ln_a, h2 = A.centred_tables(g)
    k = np.full(m, PI_P // 2)
    f = (L @ rng.standard_normal((n, m))) * g[k][None, :]
    kept = []
    for rnd in range(PI_ROUNDS):
        ang = rng.uniform(0, 2 * np.pi, m)                          # the slice accepts its first point: the likelihood is flat
        nu = (L @ rng.standard_normal((n, m))) * g[k][None, :]
        f = f * np.cos(ang)[None, :] + nu * np.sin(ang)[None, :]
        w = Rinv @ (Phi.T @ f)
        if noise:
            w = w + (g[k] * np.sqrt(eps))[None, :] * rng.standard_normal((64, m))
        xi = Rinv.T @ w
        Q = (xi[live] ** 2).sum(axis=0)
        h = Phi @ xi
        lq = lp[:, None] - (r + exponent_shift) * ln_a[:, None] - Q[None, :] * h2[:, None]
        C = np.cumsum(np.exp(lq - lq.max(axis=0)), axis=0)
        kp = (C > (rng.random(m) * C[-1])[None, :]).argmax(axis=0)
        f = h + (g[kp] / g[k])[None, :] * (f - h)                   # every answer missing: always accepted
        k = kp
        if rnd >= PI_BURN and (rnd - PI_BURN) % PI_THIN == 0:
            kept.append(k.copy())
    return np.array(kept), edges, mass


# ------------------------------------------------------------------------------------------------------ mixing -------
def geyer_ess(x):
    """ESS of one series by Geyer's initial positive sequence: N / (-1 + 2 sum of the pair sums Gamma_k = rho_2k + rho_2k+1 while
    they stay positive), autocorrelations by direct sums; a constant series has ESS 0"""
    x = np.asarray(x, dtype=np.float64)
    N = x.size
    d = x - x.mean()
    v = float(d @ d) / N
    if v == 0.0:
        return 0.0
    tau = -1.0
    for k in range(0, N // 2 - 1):
        pair = (float(d[:N - 2 * k] @ d[2 * k:]) + float(d[:N - 2 * k - 1] @ d[2 * k + 1:])) / (N * v)
        if pair <= 0:
            break
        tau += 2 * pair
    return N / max(tau, 1e-12)


def bumped_responses(n, m, seed=17, bump=1.5):
    """n x m answers of +1 / -1 from 2PL items of which the odd ones carry a bump of `bump` logits (a Gaussian of width 0.7 at
    theta = 0.5): linear items want a small amplitude, bumped ones a large one.  Returns (y, theta_init on the grid)."""
    rng = np.random.default_rng(seed)
    theta = rng.standard_normal(n)
    a, b = rng.uniform(-1, 1, m), rng.uniform(0.8, 2.0, m)
    eta = a[None, :] + b[None, :] * theta[:, None]
    eta[:, 1::2] += bump * np.exp(-0.5 * ((theta[:, None] - 0.5) / 0.7) ** 2)
    y = np.where(rng.random((n, m)) < 1 / (1 + np.exp(-eta)), 1.0, -1.0)
    return np.asfortranarray(y), np.round(np.clip(theta + 0.3 * rng.standard_normal(n), -4, 4), 2)
