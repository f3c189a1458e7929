"""Derived bounds, the constructed states and the prior-invariance chain of the centred beta update's tests
(tests/test_beta_centred_cpu.py, tests/test_gpu_beta_centred.py).  The states are tests/_amp_centred_bounds.case's, by import.

u = 2^-53 is fp64's unit roundoff, u_ld = 2^-64 long double's.  The statement (gpirt_amd.beta) is long double.

B AGAINST THE DENSE FORMULA.  With S1 = K + eps I (the true kernel) and S2 = Phi Phi^T + eps I (the rank-64 form), dS = S2 - S1,
W1 = S1^-1 X and W2 = S2^-1 X the identity S2^-1 - S1^-1 = -S2^-1 dS S1^-1 is exact, so B2 - B1 = -W2^T dS W1 and
    |B2 - B1|[k, l] <= |W2[:, k]|_2 |dS|_2 |W1[:, l]|_2,
every factor computed, |dS|_2 <= |dS|_F.  Both sides are long-double Cholesky solves of matrices with cond <= (n + eps) / eps:
their own forward error is at most 8 n u_ld cond relative (Higham, Accuracy and Stability, theorem 10.4 with the usual constant
rounded up), taken against sqrt(B_kk B_ll).  The prototype saw agreement to about 1e-9 relative; the bound at n = 1025 is of
that size and the test asserts that it stays under 1e-7 of sqrt(B_kk B_ll) (not vacuous).

W, A POSTERIORI.  With r = (Phi Phi^T + eps I) W_dev - X formed in long double from the statement's Phi, W_dev - W = S2^-1 r and
S2 >= eps I, so per column |W_dev[:, k] - W[:, k]|_2 <= |r[:, k]|_2 / eps.  The inequality holds for any W_dev; what it tests is
its size, which the non-vacuity condition caps at 1e-3 of the column's 2-norm: a W that does not solve the system fails that.
The residual itself is formed with n 64-term and 64 n-term long-double sums, error at most (n + 66) u_ld (|Phi| |Phi|^T |W| +
eps |W| + |X|), added to |r|.
    B = X^T W_dev       |B_dev - B|[k, l] <= |X[:, k]|_2 e_W[l] + (n + 2) u sum_i |X_ik| |W_dev[i, l]|  (the device's own sums)

GIVEN THE DEVICE'S W AND B everything else is a handful of operations in a stated order (include/gpirt_hip.h), each within u
relative of its exact result; first-order propagation, every term kept, the total times 1.01 for the second order:
    T      n fma terms and the tree: e_T = (n + 2) u sum_i |W_ik| |f_ij|
    ia, p  a product and a division: 2 u relative each
    Lam    Lam00 = B00 ia + p0: e = 4 u (|B00| ia + p0); Lam10 = B10 ia: 3 u |Lam10|; Lam11 as Lam00
    c00    sqrt: e_L00 / (2 c00) + u c00;  c10 = Lam10 / c00: e_L10 / c00 + |c10| e_c00 / c00 + u |c10|
    piv    = Lam11 - c10 c10: e_L11 + 2 |c10| e_c10 + u c10^2 + u |piv|;  c11: e_piv / (2 c11) + u c11
    b_k    s = B_k0 beta_0 + B_k1 beta_1: 2 u (|B_k0 beta_0| + |B_k1 beta_1|); t = T_k + s: e_T + e_s + u |t|; t ia: 3 u |t ia| +
           ia (e_T + e_s + u |t|); m0 p: 3 u |m0 p|; the sum: u |b|
    y0     = b0 / c00: e_b0 / c00 + |y0| e_c00 / c00 + u |y0|
    y1     = (b1 - c10 y0) / c11: num e = e_b1 + |c10| e_y0 + |y0| e_c10 + u |c10 y0| + u |num|; e_num / c11 + |y1| e_c11 / c11 + u |y1|
    mean1  = y1 / c11: e_y1 / c11 + |mean1| e_c11 / c11 + u |mean1|
    mean0  = (y0 - c10 mean1) / c00: as y1 with (y0, mean1, c00)
    x1, x0 the same two substitutions from z (exact inputs); beta' = mean + x: e_mean + e_x + u |beta'|
Non-vacuity: the bounds on mean and chol are at most 1e-9 of the conditional sd (sqrt of Lam^-1's diagonal).

THE REWRITE is bit for bit given the device's beta': numpy's fp64 +, -, * are the device's.  With mo = beta0 + theta beta1 (the
stored mu's bits) and mu' = beta'0 + theta beta'1 the shift is s = fl(mo - mu') and f' = fl(f + s), so g' - g = f' + mu' - f - mo
is the two roundings alone: at most u |mo - mu'| + u |f'| <= u (|f| + 2 |mu| + 2 |mu'|) (1 + u), inside the 4 u (|f| + |mu| + |mu'|)
the update's issue states (g_cell_bound), in every cell.  Summed over an item's observed cells it bounds the change of the
log-likelihood, whose derivative in g is at most 1.

PRIOR INVARIANCE.  With every answer missing the likelihood is constant and draw_f preserves the prior of f; the move must
leave beta_kj ~ N(m0_k, s0_k^2) independent of f_j ~ N(0, a_j^2 S) invariant.  64 x 64, 2000 rounds, every 5th state after round
200 kept (360 states of 64 items: N = 23040).  36 z-scores: the counts of (beta_k - m0_k) / s0_k and of
u_k = (W^T f_j)_k / (a_j sqrt(B_kk)) (standard normal under the prior, since Var W^T f = a^2 W^T S W = a^2 B) in the 8 normal
octile cells, k = 0, 1, against N / 8 with sd sqrt(N (1/8) (7/8)); and sqrt(N) times the four correlations between the
standardised betas and the u_k.  Every |z| within 5.  `pi_chain_numpy` is the chain in NumPy with the wrong variants: the move
without a_j^2, f not moved, the f-shift reversed.
"""
import numpy as np

import _amp_centred_bounds as CB

U = 2.0 ** -53
U_LD = 2.0 ** -64
LD = np.longdouble
EPS = 1.0e-3
NS, MS, SEED = CB.NS, CB.MS, CB.SEED
DENSE_NS = [2, 3, 64, 257, 1025]
SO = 1.01                          # the second-order allowance on a first-order bound

PI_N, PI_M = CB.PI_N, CB.PI_M
PI_ROUNDS, PI_BURN, PI_THIN, PI_CELLS, PI_SDS = 2000, 200, 5, 8, 5.0
PI_AMPS = (0.5, 1.0, 2.0, 1.0)
PI_MEANS, PI_PSDS = (0.5, 1.0), (0.5, 0.15)
# the standard normal's octiles, qnorm(k / 8) for k = 1 .. 7 (to 17 digits)
OCTILES = np.array([-1.1503493803760079, -0.67448975019608171, -0.31863936396437514, 0.0,
                    0.31863936396437514, 0.67448975019608171, 1.1503493803760079])


def state(n, m, amps):
    """A constructed state at n x m: CB.case(n, m) (theta on the grid with both end points and a repeated value, beta, mu, f, y)
    with prior means and sds that differ by item and row, and the amplitudes: None (off) or "spread" (fixed, geometric over
    0.25 .. 4)."""
    c = CB.case(n, m)
    j = np.arange(m)
    c["pm"] = np.stack([0.3 - 0.1 * j, 0.8 + 0.05 * j]).astype(np.float64)
    c["ps"] = np.stack([3.0 - 0.4 * j, 0.5 + 0.5 * j]).astype(np.float64)
    c["a"] = None if amps is None else (np.array([1.7]) if m == 1 else np.geomspace(0.25, 4.0, m))
    return c


def shared_fp64(theta, F=None):
    """The device's shared part in NumPy fp64 by the same formulas (not its bits): dict(W (n x 2), B (2 x 2)).  For the CPU
    tests' non-vacuity conditions."""
    from gpirt_amd import amp as A, fstar_free as FF
    th = np.asarray(theta, dtype=np.float64)
    V = FF.basis(th)
    if F is None:
        F = A.centred_factor()[0]
    X = np.stack([np.ones_like(th), th], axis=1)
    Phi = V @ F
    R = np.linalg.cholesky(Phi.T @ Phi + EPS * np.eye(64))
    Xh = np.linalg.solve(R, F.T)
    Gx = Xh.T @ (Xh @ (V.T @ X))
    W = (X - V @ Gx) / EPS
    B = np.array([[W[:, 0].sum(), W[:, 0] @ th], [W[:, 0] @ th, W[:, 1] @ th]])
    return dict(W=np.asfortranarray(W), B=B)


def dense_tolerance(theta, sh, dense):
    """(tol (2 x 2), |dS|_F) for centred_shared's B (`sh`) against gpirt_amd.beta.dense_B's (`dense` = its triple)"""
    th = np.asarray(theta, dtype=np.float64).astype(LD)
    n = th.size
    d = th[:, None] - th[None, :]
    dS = sh["Phi"] @ sh["Phi"].T - np.exp(LD(-0.5) * d * d)
    nS = float(np.sqrt((dS * dS).sum()))
    B1, W1, _ = dense
    w2 = np.sqrt((sh["W"] ** 2).sum(axis=0)).astype(np.float64)
    w1 = np.sqrt((W1 ** 2).sum(axis=0)).astype(np.float64)
    bb = np.sqrt(np.abs(np.diag(B1).astype(np.float64)))
    cond = (n + EPS) / EPS
    return np.outer(w2, w1) * nS + 8 * n * U_LD * cond * np.outer(bb, bb), nS


def w_bound(sh, W_dev, theta):
    """e_W (2): the a-posteriori bound on |W_dev[:, k] - sh["W"][:, k]|_2 of the module docstring"""
    th = np.asarray(theta, dtype=np.float64)
    n = th.size
    X = np.stack([np.ones_like(th), th], axis=1).astype(LD)
    Wd = np.asarray(W_dev, dtype=np.float64).astype(LD)
    Phi = sh["Phi"]
    r = Phi @ (Phi.T @ Wd) + LD(EPS) * Wd - X
    aP = np.abs(Phi)
    slop = (n + 66) * U_LD * (aP @ (aP.T @ np.abs(Wd)) + LD(EPS) * np.abs(Wd) + np.abs(X))
    return (np.sqrt((r * r).sum(axis=0)) + np.sqrt((slop * slop).sum(axis=0))).astype(np.float64) / EPS


def b_bound(W_dev, theta, e_W):
    """e_B (2 x 2): |B_dev - sh["B"]|[k, l] of the module docstring"""
    th = np.asarray(theta, dtype=np.float64)
    n = th.size
    X = np.stack([np.ones_like(th), th], axis=1)
    own = (n + 2) * U * (np.abs(X).T @ np.abs(np.asarray(W_dev, dtype=np.float64)))
    e = np.outer(np.linalg.norm(X, axis=0), e_W) + own
    return np.maximum(e, e.T)                  # (the device stores one sum for both off-diagonal entries)


def t_bound(W, f):
    """e_T (2 x m) = (n + 2) u |W|^T |f|"""
    W, f = np.abs(np.asarray(W, dtype=np.float64)), np.abs(np.asarray(f, dtype=np.float64))
    return (W.shape[0] + 2) * U * (W.T @ f)


def update_bounds(ref, B, beta, a, pm, ps, z, e_T):
    """dict(Lam (3 x m: Lam00, Lam10, Lam11), chol (3 x m), mean (2 x m), beta (2 x m), sd (2 x m: the conditional sds)) of the
    module docstring for a gpirt_amd.beta.centred_exact_update result `ref` computed from the device's W and B"""
    B = np.abs(np.asarray(B, dtype=np.float64).reshape(2, 2))
    beta = np.asarray(beta, dtype=np.float64)
    m = beta.shape[1]
    a = np.ones(m) if a is None else np.asarray(a, dtype=np.float64)
    f64 = lambda x: np.abs(np.asarray(x, dtype=np.float64))                              # noqa: E731
    out = dict(Lam=np.empty((3, m)), chol=np.empty((3, m)), mean=np.empty((2, m)), beta=np.empty((2, m)), sd=np.empty((2, m)))
    for j in range(m):
        ia = 1.0 / (a[j] * a[j])
        p = 1.0 / (ps[:, j] * ps[:, j])
        L = f64(ref["Lam"][j])
        c00, c10, c11 = f64(ref["chol"][:, j])
        T = f64(ref["T"][:, j])
        e_L00 = 4 * U * (B[0, 0] * ia + p[0])
        e_L10 = 3 * U * L[1, 0]
        e_L11 = 4 * U * (B[1, 1] * ia + p[1])
        e_c00 = e_L00 / (2 * c00) + U * c00
        e_c10 = e_L10 / c00 + c10 * e_c00 / c00 + U * c10
        piv = c11 * c11
        e_piv = e_L11 + 2 * c10 * e_c10 + U * c10 * c10 + U * piv
        e_c11 = e_piv / (2 * c11) + U * c11
        e_b, b = np.empty(2), np.empty(2)
        for k in range(2):
            s_abs = B[k, 0] * abs(beta[0, j]) + B[k, 1] * abs(beta[1, j])
            e_s = 2 * U * s_abs
            t_abs = T[k] + s_abs
            e_t = e_T[k, j] + e_s + U * t_abs
            prior = abs(pm[k, j]) * p[k]
            b[k] = t_abs * ia + prior
            e_b[k] = 3 * U * t_abs * ia + ia * e_t + 3 * U * prior + U * b[k]
        mean = f64(ref["mean"][:, j])
        # the substitutions, from the exact magnitudes of the statement
        y0 = float(abs(ref["mean"][0, j] * ref["chol"][0, j] + ref["chol"][1, j] * ref["mean"][1, j]))      # c00 mean0 + c10 mean1
        y1 = float(abs(ref["chol"][2, j] * ref["mean"][1, j]))                                              # c11 mean1
        e_y0 = e_b[0] / c00 + y0 * e_c00 / c00 + U * y0
        num1 = y1 * c11
        e_num1 = e_b[1] + c10 * e_y0 + y0 * e_c10 + U * c10 * y0 + U * (num1 + 2 * c10 * y0)
        e_y1 = e_num1 / c11 + y1 * e_c11 / c11 + U * y1
        e_m1 = e_y1 / c11 + mean[1] * e_c11 / c11 + U * mean[1]
        num0 = mean[0] * c00
        e_num0 = e_y0 + c10 * e_m1 + mean[1] * e_c10 + U * c10 * mean[1] + U * (num0 + 2 * c10 * mean[1])
        e_m0 = e_num0 / c00 + mean[0] * e_c00 / c00 + U * mean[0]
        x = f64(ref["beta"][:, j] - ref["mean"][:, j])
        e_x1 = x[1] * e_c11 / c11 + U * x[1]
        numx = x[0] * c00
        e_numx = c10 * e_x1 + x[1] * e_c10 + U * c10 * x[1] + U * (numx + 2 * c10 * x[1])
        e_x0 = e_numx / c00 + x[0] * e_c00 / c00 + U * x[0]
        bn = f64(ref["beta"][:, j])
        out["Lam"][:, j] = SO * np.array([e_L00, e_L10, e_L11])
        out["chol"][:, j] = SO * np.array([e_c00, e_c10, e_c11])
        out["mean"][:, j] = SO * np.array([e_m0, e_m1])
        out["beta"][:, j] = SO * np.array([e_m0 + e_x0 + U * bn[0], e_m1 + e_x1 + U * bn[1]])
        out["sd"][:, j] = np.sqrt(np.abs(np.diag(np.asarray(ref["cov"][j], dtype=np.float64))))
    return out


def g_cell_bound(f, mu, mu_new):
    """4 u (|f| + |mu| + |mu'|) cell by cell"""
    return 4 * U * (np.abs(f) + np.abs(mu) + np.abs(mu_new))


def loglik(g, y):
    """per item: the sum over the observed cells of -log(1 + exp(-y g)) in long double"""
    g, y = np.asarray(g, dtype=LD), np.asarray(y, dtype=np.float64)
    obs = ~np.isnan(y)
    x = np.where(obs, y, 0.0).astype(LD) * g
    t = np.maximum(-x, LD(0)) + np.log1p(np.exp(-np.abs(x)))
    return -np.where(obs, t, LD(0)).sum(axis=0)


# ------------------------------------------------------------------------------------------- prior invariance -------
def pi_theta():
    return CB.pi_setup()[0]


def pi_priors():
    """(amplitudes (m), prior means (2 x m), prior sds (2 x m)) of the prior-invariance configuration"""
    a = np.array([PI_AMPS[j % 4] for j in range(PI_M)])
    pm = np.repeat(np.array(PI_MEANS)[:, None], PI_M, axis=1)
    ps = np.repeat(np.array(PI_PSDS)[:, None], PI_M, axis=1)
    return a, pm, ps


def pi_zscores(betas, us):
    """The 36 z-scores from the kept standardised betas and u (each kept x 2 x m): 4 x 8 cell counts, then 4 correlations."""
    sb = np.asarray(betas, dtype=np.float64).transpose(1, 0, 2).reshape(2, -1)
    su = np.asarray(us, dtype=np.float64).transpose(1, 0, 2).reshape(2, -1)
    N = sb.shape[1]
    p = 1.0 / PI_CELLS
    z = []
    for x in (sb[0], sb[1], su[0], su[1]):
        cnt = np.bincount(np.searchsorted(OCTILES, x), minlength=PI_CELLS)
        z.extend(((cnt - N * p) / np.sqrt(N * p * (1 - p))).tolist())
    for k in range(2):
        for l in range(2):
            z.append(float(np.sqrt(N) * np.corrcoef(sb[k], su[l])[0, 1]))
    return np.array(z)


def pi_chain_numpy(seed=3, variant="ok"):
    """The chain in NumPy (fp64, NumPy's own generator): PI_ROUNDS rounds of {draw_f under a constant likelihood, the centred
    update of every item}; returns (standardised betas, u), each kept x 2 x m, read right after the move.  variant: "ok", or one
    of the wrong moves "no_a2" (the precision without a_j^2), "f_fixed" (f not moved), "reversed" (the f-shift's sign)."""
    from gpirt_amd import amp as A, fstar_free as FF
    theta = pi_theta()
    a, pm, ps = pi_priors()
    rng = np.random.default_rng(seed)
    n, m = PI_N, PI_M
    Phi = FF.basis(theta) @ A.centred_factor()[0]
    S = Phi @ Phi.T + EPS * np.eye(n)
    L = np.linalg.cholesky(S)
    X = np.stack([np.ones(n), theta], axis=1)
    W = np.linalg.solve(S, X)
    B = X.T @ W
    B = (B + B.T) / 2
    ia = np.ones(m) if variant == "no_a2" else 1.0 / (a * a)
    prec = 1.0 / (ps * ps)
    beta = pm + ps * rng.standard_normal((2, m))
    f = (L @ rng.standard_normal((n, m))) * a[None, :]
    kb, ku = [], []
    sB = np.sqrt(np.diag(B))
    for rnd in range(PI_ROUNDS):
        ang = rng.uniform(0, 2 * np.pi, m)                          # the slice accepts its first point: the likelihood is flat
        nu = (L @ rng.standard_normal((n, m))) * a[None, :]
        f = f * np.cos(ang)[None, :] + nu * np.sin(ang)[None, :]
        T = W.T @ f
        z = rng.standard_normal((2, m))
        new = np.empty((2, m))
        for j in range(m):
            Lam = B * ia[j] + np.diag(prec[:, j])
            b = (T[:, j] + B @ beta[:, j]) * ia[j] + pm[:, j] * prec[:, j]
            C = np.linalg.cholesky(Lam)
            new[:, j] = np.linalg.solve(Lam, b) + np.linalg.solve(C.T, z[:, j])
        d = beta - new
        if variant == "reversed":
            f = f - X @ d
        elif variant != "f_fixed":
            f = f + X @ d
        beta = new
        if rnd >= PI_BURN and (rnd - PI_BURN) % PI_THIN == 0:
            kb.append((beta - pm) / ps)
            ku.append((W.T @ f) / (a[None, :] * sB[:, None]))
    return np.array(kb), np.array(ku)
