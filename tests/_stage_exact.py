"""Long-double references of the four stages of an iteration behind the factorisation, and the constructed inputs the GPU
tests feed them (tests/test_gpu_draw_f_constructed.py, tests/test_gpu_fstar_ranks.py,
tests/test_gpu_draw_theta_constructed.py, tests/test_gpu_draw_beta_constructed.py).

  slice_exact        one column of ess(), src/draw-f.cpp:21-60, with a derived bound on the device's rounding
  fstar_rank_exact   draw_fstar through K(theta, theta*) = K(theta, c) V^T at r Chebyshev nodes (r = 0: the full solve)
  item_uniforms / item_normals   the counter-based item RNG restated in NumPy (checked against the oracle's)
  draw_f_cases       the constructed columns of the draw_f test, per order n and scale sigma of L = sigma I
  theta_exact        draw_theta (src/draw-theta.cpp:3-37) per respondent, with a derived bound on the device's CDF
  beta_exact         draw_beta (src/draw-beta.cpp:3-41) for one item, with a derived bound on the device's r
  draw_theta_cases / draw_beta_cases   the constructed respondents and items of the two tests

np.longdouble is the x87 80-bit format (64-bit significand) on the machines this suite runs on; nothing here needs more.
"""
from __future__ import annotations

import functools

import numpy as np

LD = np.longdouble
NGRID = 1001
ST_F_Z, ST_F_ESS, ST_FSTAR = 3, 4, 5
LL_SCREEN_ERR = 4.0e-6                 # csrc/ll_fast.h
EXP_OVERFLOW = 709.782712893384        # exp(x) = +inf in fp64 above this
U53, U52, U51, U50 = 2.0 ** -53, 2.0 ** -52, 2.0 ** -51, 2.0 ** -50


# --------------------------------------------------------------------------------------------- the item RNG --------
def _philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al. 2011) on uint64 arrays that hold 32-bit words"""
    M = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M
        k0 = (k0 + np.uint64(0x9E3779B9)) & M
        k1 = (k1 + np.uint64(0xBB67AE85)) & M
    return c0, c1


def item_uniforms(seed, it, stage, item, index):
    """uniforms in (0, 1) keyed (seed, iteration, stage, item, index): 52 random bits + half an ulp; item and index broadcast"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    o0, o1 = _philox4x32_10(np.asarray(index, dtype=np.uint64), np.asarray(item, dtype=np.uint64), np.uint64(stage),
                            np.uint64(it), seed & 0xFFFFFFFF, seed >> 32)
    v = ((o0 >> np.uint64(6)) << np.uint64(26)) | (o1 >> np.uint64(6))
    return (v.astype(np.float64) + 0.5) * U52


def _horner(r, coef):
    acc = np.full_like(r, coef[0])
    for c in coef[1:]:
        acc = acc * r + c
    return acc


_A = ((2509.0809287301226727, 33430.575583588128105, 67265.770927008700853, 45921.953931549871457, 13731.693765509461125,
       1971.5909503065514427, 133.14166789178437745, 3.387132872796366608),
      (5226.495278852545925, 28729.085735721942674, 39307.89580009271061, 21213.794301586595867, 5394.1960214247511077,
       687.1870074920579083, 42.313330701600911252, 1.0))
_C = ((7.7454501427834140764e-4, 0.0227238449892691845833, 0.24178072517745061177, 1.27045825245236838258,
       3.64784832476320460504, 5.7694972214606914055, 4.6303378461565452959, 1.42343711074968357734),
      (1.05075007164441684324e-9, 5.475938084995344946e-4, 0.0151986665636164571966, 0.14810397642748007459,
       0.68976733498510000455, 1.6763848301838038494, 2.05319162663775882187, 1.0))
_E = ((2.01033439929228813265e-7, 2.71155556874348757815e-5, 0.0012426609473880784386, 0.026532189526576123093,
       0.29656057182850489123, 1.7848265399172913358, 5.4637849111641143699, 6.6579046435011037772),
      (2.04426310338993978564e-15, 1.4215117583164458887e-7, 1.8463183175100546818e-5, 7.868691311456132591e-4,
       0.0148753612908506148525, 0.13692988092273580531, 0.59983220655588793769, 1.0))


def qnorm(p):
    """Wichura's AS 241 (PPND16), the inversion R's qnorm and the library use, for p in (0, 1)"""
    p = np.asarray(p, dtype=np.float64)
    q = p - 0.5
    out = np.empty_like(p)
    mid = np.abs(q) <= 0.425
    r = 0.180625 - q[mid] * q[mid]
    out[mid] = q[mid] * _horner(r, _A[0]) / _horner(r, _A[1])
    t = ~mid
    r = np.sqrt(-np.log(np.where(q[t] < 0, p[t], 1.0 - p[t])))
    near = r <= 5.0
    val = np.empty_like(r)
    val[near] = _horner(r[near] - 1.6, _C[0]) / _horner(r[near] - 1.6, _C[1])
    val[~near] = _horner(r[~near] - 5.0, _E[0]) / _horner(r[~near] - 5.0, _E[1])
    out[t] = np.where(q[t] < 0, -val, val)
    return out


def item_normals(seed, it, stage, items, n_index):
    """(n_index, len(items)): column j holds item items[j]'s normals, index 0 .. n_index - 1"""
    items = np.asarray(items, dtype=np.uint64)
    return qnorm(item_uniforms(seed, it, stage, items[None, :], np.arange(n_index, dtype=np.uint64)[:, None]))


# ----------------------------------------------------------------------------------------------- slice_exact -------
def sum_depth(n):
    """An upper bound on the number of additions any term of a column's sum passes through in the slice kernels
    (csrc/rng_ess.hip): a lane adds at most ceil(n / 256) terms one after the other (8 or 16 in the register kernels), a
    wavefront's shuffle tree adds 6 levels, the wavefronts' partial sums at most 4 more (written as one expression of up to
    sixteen values); 16 covers the last two with room."""
    return -(-int(n) // 256) + 16


def slice_exact(f, y, nu, mu, uniforms, term="exact", max_trials=4000):
    """One column of ess() (src/draw-f.cpp:21-60) in long double.

    uniforms[0] is u of the slice level (:28), uniforms[1] the first angle (:35), one more per rejection (:56) -- nothing is
    consumed once the bracket has closed (eps_min == eps_max: R::runif(a, a) = a).  eps is carried in fp64, the way the
    device carries it; cos, sin, the trial point, the terms and their sums are long double.
    term = "exact":   max(-a, 0) + log1p(exp(-|a|)), what csrc/ll_fast.h approximates to 2 ulp;
    term = "written": log(1 + exp(-a)) as src/log-likelihood.cpp:34 writes it, each term evaluated in fp64 from the fp64
                      argument (+inf for a < -709.78), the terms added in long double.

    Returns a dict: k (rejections), f_new (long double), f_err (a bound per row on |device f' - f_new|, below), and per
    trial t = 0..k: margin[t] = |ll(f'_t) - log_y|, sum_abs[t] = sum of |terms|, bound[t] (below), overflow[t] (written
    form: an observed row of the trial overflows), plus n_band / n_near: the trials whose margin is within
    band = LL_SCREEN_ERR n of the level, and those outside it but within four bands; undecided: the trials with
    margin < bound[t].

    THE BOUND.  The device forms, at a trial with angle eps_t, for every observed row
        a_i = y_i ((f_i c + nu_i s) + mu_i),   c = cos(eps_t), s = sin(eps_t)            (fp64)
    and adds the terms T(a_i).  With u = 2^-53 and against the long-double value of the same expression:
      * eps: every update eps = eps_min + (eps_max - eps_min) U is one fp64 expression of magnitudes <= 2 pi that the
        device may contract into an fma: its value differs by at most one ulp(2 pi) = 2^-50 from NumPy's, and the bracket
        ends are earlier values of eps, so after t updates |d eps| <= (t + 1) 2^-50;
      * cos / sin: the device library's are within 2 ulp, |dc|, |ds| <= 2^-51 (values <= 1; NumPy's long-double
        ones are exact at this scale); together |d(f c + nu s)| <= (|f_i| + |nu_i|) (2^-51 + (t + 1) 2^-50);
      * rounding of (f c + nu s) + mu: two products, two sums, each u relative, fma or not: <= 4 u (|f_i| + |nu_i| + |mu_i|);
        the product with y = +-1 is exact.  Sum of the two: da_i;
      * the term: |T'(a)| <= 1, so the argument contributes da_i; the term's own error is 2 ulp of its value for the
        form of ll_fast.h (tests/test_ll_fast.py) -- 2^-51 |T| -- and for the written form through the library's exp and log
        (1 ulp each, and a 1 + e that may round the other way: 2^-52 absolute through the logarithm) 2^-51 |T| + 2^-50;
        the larger, 2^-51 |T_i| + 2^-50, is used for both;
      * the summation: every partial sum passes through at most h = sum_depth(n) additions, each u relative, so the sum
        is off by at most 1.01 h u sum|T_i|.
    bound(trial) = sum_i (da_i + 2^-51 |T_i| + 2^-50) + 1.01 h u sum|T_i|.  The level log_y = ll(f) + log(u) carries the same
    bound at eps = 0 without the trigonometric part, plus the rounding of the logarithm and of the sum, 2^-51 (|log u| +
    |log_y|).  bound[t] is the sum of the two: a trial whose margin is below it is UNDECIDED -- the device may take either
    branch.  (Written form: a trial with an observed row within 1e-6 of the overflow threshold is undecided too.)
    f_err, for the accepted trial: (|f_i| + |nu_i|) (2^-51 + (k + 1) 2^-50) + 4 u (|f_i| + |nu_i|).
    """
    assert term in ("exact", "written")
    f64, nu64, mu64 = (np.asarray(a, dtype=np.float64) for a in (f, nu, mu))
    y = np.asarray(y, dtype=np.float64)
    n = len(f64)
    obs = np.flatnonzero(~np.isnan(y))
    yo = y[obs]
    fo, no, mo = f64[obs], nu64[obs], mu64[obs]
    foL, noL, moL, yoL = fo.astype(LD), no.astype(LD), mo.astype(LD), yo.astype(LD)
    h = sum_depth(n)
    mag2, mag3 = np.abs(fo) + np.abs(no), np.abs(fo) + np.abs(no) + np.abs(mo)

    def ll_at(eps, t):
        """(ll, sum|T|, bound of the fp64 sum's error, overflow) at angle eps after t updates of eps (t = -1: the current state)"""
        if t < 0:
            aL = yoL * (foL + moL)
            a64 = yo * (fo + mo)
            da = 2 * U53 * (np.abs(fo) + np.abs(mo))
        else:
            cL, sL = np.cos(LD(eps)), np.sin(LD(eps))
            aL = yoL * ((foL * cL + noL * sL) + moL)
            a64 = yo * ((fo * np.cos(eps) + no * np.sin(eps)) + mo)
            da = mag2 * (U51 + (t + 1) * U50) + 4 * U53 * mag3
        edge = False
        if term == "exact":
            T = np.maximum(-aL, LD(0)) + np.log1p(np.exp(-np.abs(aL)))
            over = False
        else:
            with np.errstate(over="ignore"):
                T = np.log(1.0 + np.exp(-a64)).astype(LD)
            over = bool(np.isinf(T).any())
            edge = bool((np.abs(a64 + EXP_OVERFLOW) < 1e-6).any())
        tot = T.sum() if len(T) else LD(0)
        sabs = float(np.abs(T).sum()) if len(T) else 0.0
        bnd = float(da.sum()) + U51 * sabs + U50 * len(T) + 1.01 * h * U53 * sabs if not over else 0.0
        return -tot, sabs, bnd, over, edge

    us = np.asarray(uniforms, dtype=np.float64)
    ll0, _, b0, over0, edge0 = ll_at(0.0, -1)
    log_u = np.log(LD(us[0]))
    log_y = ll0 + log_u
    b_level = b0 + (U51 * (abs(float(log_u)) + abs(float(log_y))) if np.isfinite(log_y) else 0.0)
    two_pi = 2.0 * np.pi
    eps_min, eps_max = 0.0, two_pi
    eps = eps_min + (eps_max - eps_min) * us[1]
    eps_min = eps - two_pi
    ui, k = 2, 0
    band = LL_SCREEN_ERR * n
    margin, sum_abs, bound, overflow, undecided = [], [], [], [], 0
    n_band = n_near = 0
    while True:
        llp, sabs, bt, over, edge = ll_at(eps, k)
        mg = abs(float(llp - log_y)) if (np.isfinite(llp) or np.isfinite(log_y)) else 0.0
        if not np.isfinite(llp) and not np.isfinite(log_y):
            mg = np.inf                                        # -inf > -inf is false under every rounding: a decided rejection
        margin.append(mg); sum_abs.append(sabs); bound.append(bt + b_level); overflow.append(over)
        if mg < bt + b_level or edge or edge0:
            undecided += 1
        if mg <= band:
            n_band += 1
        elif mg <= 4 * band:
            n_near += 1
        if llp > log_y:
            break
        if eps < 0.0:
            eps_min = eps
        else:
            eps_max = eps
        if eps_min == eps_max:
            eps = eps_min
        else:
            eps = eps_min + (eps_max - eps_min) * us[ui]
            ui += 1
        k += 1
        if k >= max_trials:
            raise RuntimeError("slice_exact: no trial point accepted")
    cL, sL = np.cos(LD(eps)), np.sin(LD(eps))
    f_new = f64.astype(LD) * cL + nu64.astype(LD) * sL
    mag = np.abs(f64) + np.abs(nu64)
    f_err = mag * (U51 + (k + 1) * U50) + 4 * U53 * mag
    return dict(k=k, f_new=f_new, f_err=f_err, margin=margin, sum_abs=sum_abs, bound=bound, overflow=overflow,
                n_band=n_band, n_near=n_near, undecided=undecided, eps=eps, band=band)


# -------------------------------------------------------------------------------------------- fstar_rank_exact -----
def grid():
    return -5.0 + np.arange(NGRID, dtype=np.float64) * 0.01


def cheb_nodes(r):
    """5 cos((2k + 1) pi / 2r), k = 0..r-1, rounded to fp64 (what the device evaluates K(theta, c) at), and the long-double
    barycentric weights (-1)^k sin((2k + 1) pi / 2r)"""
    a = (2 * np.arange(r, dtype=LD) + 1) * LD("3.141592653589793238462643383279502884") / (2 * r)
    c = (LD(5) * np.cos(a)).astype(np.float64)
    w = np.where(np.arange(r) % 2 == 1, LD(-1), LD(1)) * np.sin(a)
    return c, w


@functools.lru_cache(maxsize=None)
def cheb_basis(r):
    """(nodes (r,) fp64, V (1001, r) long double): V[j, k] = the k-th Lagrange basis polynomial of the nodes at grid point j,
    in barycentric form (a grid point that IS a node gets the unit row)"""
    c, w = cheb_nodes(r)
    d = grid().astype(LD)[:, None] - c.astype(LD)[None, :]
    hit = d == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = w[None, :] / d
        V = q / q.sum(axis=1, keepdims=True)
    rows = hit.any(axis=1)
    V[rows] = hit[rows].astype(LD)
    return c, V


def se_kernel_ld(x1, x2):
    d = np.asarray(x1, dtype=np.float64).astype(LD)[:, None] - np.asarray(x2, dtype=np.float64).astype(LD)[None, :]
    return np.exp(LD(-0.5) * d * d)


def _forward(L, B):
    """L^-1 B by forward substitution, long double"""
    B = B.copy()
    for i in range(L.shape[0]):
        if i:
            B[i] -= L[i, :i] @ B[:i]
        B[i] /= L[i, i]
    return B


def _backward(L, B):
    """L^-T B by back substitution, long double"""
    B = B.copy()
    for i in range(L.shape[0] - 1, -1, -1):
        if i + 1 < L.shape[0]:
            B[i] -= L[i + 1:, i] @ B[i + 1:]
        B[i] /= L[i, i]
    return B


def interpolation_error(r, theta=None):
    """max |K(theta, c) V^T - K(theta, theta*)| in long double with V rounded to fp64 (what the device holds); theta: every
    seventh grid point by default"""
    c, V = cheb_basis(r)
    th = grid()[::7] if theta is None else theta
    V64 = V.astype(np.float64).astype(LD)
    return float(np.abs(se_kernel_ld(th, c) @ V64.T - se_kernel_ld(th, grid())).max())


def fstar_rank_exact(theta, L, f, mu_star, r, z):
    """draw_fstar (src/draw-fstar.cpp:10-31) in long double through the rank-r form the sampler builds (r = 0: the full
    form, L^-1 k* and its column norms).  L is an input: pass the device's own factor, so that the comparison prices the
    stage and not the factorisation.  V is rounded to fp64 first, as the device holds it.
      U = K(theta, c);  B = L^-1 U;  W = B V^T (n x 1001);  s_j = 1 - sqrt(max(sum_i W_ij^2, 0))     (:19-20)
      mean = V (L^-T B)^T f  (:7, :24-25; WITHOUT mu*, like the sampler's "mean");  f* = mean + mu* + s z   (:27)
    (R::rnorm: s = 0 returns the mean, s < 0 NaN.)  Also returns alpha1 = ||S^-1 f_j||_1 per item, S = L L^T, and
    cond = cond_2(L)^2 = cond_2(S) (fp64 singular values of L) -- what the derived tolerances of the tests use."""
    Ld = np.asarray(L, dtype=np.float64).astype(LD)
    fL = np.asarray(f, dtype=np.float64).astype(LD)
    if r > 0:
        c, V = cheb_basis(r)
        V = V.astype(np.float64).astype(LD)
        B = _forward(Ld, se_kernel_ld(theta, c))
        W = B @ V.T
        Cm = _backward(Ld, B)
        mean = V @ (Cm.T @ fL)
    else:
        W = _forward(Ld, se_kernel_ld(theta, grid()))
        mean = W.T @ _forward(Ld, fL)
    q = (W * W).sum(axis=0)
    s = LD(1) - np.sqrt(np.maximum(q, LD(0)))
    zL, muL = np.asarray(z, dtype=np.float64).astype(LD), np.asarray(mu_star, dtype=np.float64).astype(LD)
    m0 = mean + muL
    fstar = np.where(s[:, None] > 0, m0 + s[:, None] * zL, np.where(s[:, None] == 0, m0, LD("nan")))
    alpha = _backward(Ld, _forward(Ld, fL))
    return dict(s=s, mean=mean, fstar=fstar, q=q, alpha1=np.abs(alpha).sum(axis=0).astype(np.float64),
                cond=float(np.linalg.cond(np.asarray(L, dtype=np.float64), 2) ** 2))


# --------------------------------------------------------------------------------- the constructed draw_f columns ---
ORDERS = (100, 2049, 8193, 16385)      # the smallest order of each size class of launch_ess (csrc/rng_ess.hip)
SIGMAS = (1.0, 50.0, 1.0e3)            # L = sigma I: one launch per order, mode and sigma
SEED = {100: 11, 2049: 23, 8193: 33, 16385: 44}      # chosen so that the conditions of tests/test_stage_exact_cpu.py hold
N_FEW = {100: 0, 2049: 360, 8193: 150, 16385: 12}     # screen-band columns with 1, 2, 3 observed rows (reg-class orders need many)
N_DENSE = 2


def iteration(sigma):
    return 1 + SIGMAS.index(sigma)


@functools.lru_cache(maxsize=None)
def draw_f_cases(n, sigma):
    """(names, f, y, mu) of the launch at order n with L = sigma I: n x m column-major fp64, one column per name.  The item
    RNG's keys are (SEED[n], iteration(sigma), stage, column)."""
    seed, it = SEED[n], iteration(sigma)
    rng = np.random.default_rng(1000 * n + int(sigma))
    theta = np.clip(rng.normal(size=n), -4.9, 4.9)
    cols = []

    def responses(missing=0.05):
        y = np.where(rng.random(n) < 0.5, 1.0, -1.0)
        y[rng.random(n) < missing] = np.nan
        return y

    def add(name, f, y, mu):
        cols.append((name, np.asarray(f, dtype=np.float64), y, np.asarray(mu, dtype=np.float64)))

    def ordinary():
        return rng.normal(size=n), responses(), 0.3 - 0.8 * theta

    if sigma == 1.0:
        add("ordinary", *ordinary())
        # |f + mu| in 30..45, both signs of a = y (f + mu): the written term is exactly 0 above 37, the fast one e^-a
        y = responses()
        g = rng.uniform(30.0, 45.0, size=n) * np.where(rng.random(n) < 0.5, 1.0, -1.0)
        f = rng.normal(size=n)
        add("a_30_45", f, y, g - f)
        for name, lvl in (("mu_300", 300.0), ("mu_700", 700.0)):      # |a| <= 700 + sqrt(f^2 + nu^2) < 709.78
            add(name, rng.normal(size=n), responses(),
                lvl * np.where(rng.random(n) < 0.5, 1.0, -1.0) + rng.uniform(-1.0, 1.0, size=n))
        add("no_observed_row", rng.normal(size=n), np.full(n, np.nan), rng.normal(size=n))
        if n >= 2049:
            for q in range(N_FEW[n]):                                  # the screen band: 1, 2, 3 observed rows of n
                y = np.full(n, np.nan)
                rows = rng.choice(n, size=1 + q % 3, replace=False)
                y[rows] = np.where(rng.random(len(rows)) < 0.5, 1.0, -1.0)
                add(f"band_{1 + q % 3}_rows_{q}", rng.normal(size=n), y, rng.normal(size=n))
            for q in range(N_DENSE):                                   # ... and the dense twin: every row observed
                add(f"band_dense_{q}", rng.normal(size=n), responses(missing=0.0), rng.normal(size=n))
    elif sigma == 50.0:
        add("ordinary_s50", *ordinary())
        add("mu_300_s50", rng.normal(size=n), responses(),
            300.0 * np.where(rng.random(n) < 0.5, 1.0, -1.0) + rng.uniform(-1.0, 1.0, size=n))
        # the CURRENT state beyond the overflow: one observed row with a = -720 exactly, at the row whose nu = 50 z is
        # largest, so that trial points leave the overflow region on part of the ellipse
        f, y, mu = ordinary()
        z = item_normals(seed, it, ST_F_Z, [len(cols)], n)[:, 0]
        i0 = int(np.argmax(np.abs(z)))
        y[i0] = 1.0 if z[i0] > 0 else -1.0
        f[i0] = 0.5
        mu[i0] = -720.0 * y[i0] - 0.5
        add("current_overflow", f, y, mu)
    else:
        add("trial_overflow", *ordinary())                              # current state |a| < 700, nu = 1e3 z
    names = [c[0] for c in cols]
    F, Y, MU = (np.asfortranarray(np.stack([c[i] for c in cols], axis=1)) for i in (1, 2, 3))
    return names, F, Y, MU


def draw_f_reference_with(n, sigma, term, Z):
    """slice_exact for every column of draw_f_cases(n, sigma) with nu = fl(sigma Z): Z as the device drew it (its qnorm goes
    through the device library's log and sqrt and may differ from the restatement's in the last place)"""
    names, F, Y, MU = draw_f_cases(n, sigma)
    seed, it = SEED[n], iteration(sigma)
    m = len(names)
    U = item_uniforms(seed, it, ST_F_ESS, np.arange(m)[None, :], np.arange(4096)[:, None])
    return [slice_exact(F[:, j], Y[:, j], sigma * Z[:, j], MU[:, j], U[:, j], term) for j in range(m)]


@functools.lru_cache(maxsize=None)
def draw_f_reference(n, sigma, term):
    """... with Z from the restated item RNG: what tests/test_stage_exact_cpu.py checks the inputs' conditions on"""
    Z = item_normals(SEED[n], iteration(sigma), ST_F_Z, np.arange(len(draw_f_cases(n, sigma)[0])), n)
    return draw_f_reference_with(n, sigma, term, Z), Z


# ------------------------------------------------------------------------------------------------ theta_exact ------
ST_THETA, ST_BETA = 6, 7               # csrc/common.h, oracle/gpirt_oracle.h
LN_SQRT_2PI = LD("0.918938533204672741780329736406")
EXP_UNDERFLOW = -745.1332191019412     # exp(x) = 0 in fp64 below this (x < log 2^-1075)
TF_MAX = 709.0                         # csrc/theta_fixed.hip: a grid row with |f*| above it hands the product to the fp64 GEMM
SENTINEL = -1e300                      # csrc/stages.hip loglik_terms_kernel: what the device's product holds for -inf
SCAN_DEPTH = 3 + 8 + 1                 # theta_sample_kernel: 3 additions inside a thread, 8 scan levels, 1 base addition


def theta_hands_over(fstar):
    """the fixed-point product leaves the launch to the fp64 GEMM: some |f*| > 709 or not finite"""
    return not bool((np.abs(np.asarray(fstar, dtype=np.float64)) <= TF_MAX).all())


def _masked_product(G, ind):
    """sum over the cells with ind = 1 of G (N x m long double, may hold -inf and NaN) per (row, respondent): the finite
    sum, the sum of |terms|, and the number of -inf and NaN cells seen (0 * inf never formed)"""
    fin = np.isfinite(G)
    Gf = np.where(fin, G, LD(0))
    I = ind.astype(LD)
    I64 = ind.astype(np.float64)
    return (Gf @ I.T, (np.abs(Gf) @ I.T).astype(np.float64), np.isneginf(G).astype(np.float64) @ I64.T,
            np.isnan(G).astype(np.float64) @ I64.T)


def theta_exact(y, fstar, u, stabilise, product="fixed"):
    """draw_theta (src/draw-theta.cpp:3-37) in long double for every respondent: y (n x m, NaN = missing), fstar (1001 x m),
    u (n,) the uniforms of :27.  The terms of ll() (:18, src/log-likelihood.cpp:12-23) are -log1p(exp(-+f*)) in long double,
    -inf where the written fp64 form overflows (-+f* > 709.78) and NaN where f* is; a cell counts only where it is
    observed.  exp (:21) is fp64's in its RANGE: 0 below 2^-1075.  max / min (:23-24) skip NaN the way the oracle's
    comparisons and the device's fmax do: a NaN at row k0 leaves rows < k0 an ordinary CDF that ends in 1.

    Returns a dict: index (n,) the grid row drawn, -1 = degenerate (no row's CDF exceeds u: 0/0, or NaN throughout);
    cdf (1001 x n long double); logpost (1001 x n long double, before the prior) and lp_bound (the product's bound, below);
    margin = min(|cdf[k] - u|, |cdf[k-1] - u|) at the row drawn; bound on |device CDF - cdf| at those two rows;
    undecided = margin < bound (bool per respondent); degenerate = their count.

    product: "fixed" (csrc/theta_fixed.hip; the fp64 GEMM's bound where theta_hands_over(fstar)), "gemm"
    (GPIRT_THETA_FIXED=2), "oracle" (the CPU oracle's sequential fp64 loops: depth m in the product, 1001 in the cumsum).

    THE BOUND, with u = 2^-53, per respondent i and row k, first in the log domain (eps_k, absolute):
      * the terms: the device's fp64 -log(1 + exp(-a)) is within 2^-51 |T| + 2^-50 of T (slice_exact); over the observed
        cells that is 2^-51 sum|T| + 2^-50 n_obs -- the 0/1 operand multiplies everything else by an exact 0;
      * the product: fixed point rounds every term once to 54 bits of its row's range, 2^(e_k - 55) per observed cell,
        e_k = floor(log2(max_j |f*_kj| + log 2)) + 1, adds exactly and rounds the result once (one ulp of |logpost|) -- the
        bound of tests/test_gpu_theta_fixed.py; the GEMM adds 2m products in an order of its own, any of which is within
        1.01 (2m) u sum|T| (depth <= 2m; the correction pass behind it re-sums at most m terms one after the other);
        lp_bound is the sum of this and the terms' part;
      * the prior -(log sqrt(2 pi) + z^2 / 2): three roundings of at most |prior| each, and a grid point that an fma would
        move by an ulp of 5: 3 u |prior| + 2^-50 |theta*_k|;
      * prior + logpost: u |P_k|;  minus the maximum (stabilise): u |P_k - max|.  The maximum is one of the device's own
        P_k; whatever it is off by shifts every row alike and cancels in the quotient of :25.
      Rows at -inf (the device: at or below -1e300, whose exp is exactly 0) and NaN rows carry no error.
    exp: 2 ulp of its own plus its argument's error as a relative one, rho_k = 1.01 eps_k + 2^-51 (eps_k < 0.01, else the
    respondent is undecided), and 2^-1074 absolute where the result is subnormal.
    cumsum as theta_sample_kernel forms it: every term passes through at most h = 12 additions (3 in its thread, 8 scan
    levels, 1 base), so |dC_k| <= E_k = sum_{j<=k} (rho_j e_j + 2^-1074) + 1.01 h u C_k.
    :25, with T_k = C_k - C_0 (summed here without C_0, so that nothing is lost to it) and L the last row that is not NaN:
        |d cdf_k| <= 1.02 ((E_k + E_0) + cdf_k (E_L + E_0)) / T_L + 4 u
    (numerator and denominator each one rounding, the division one; (E_L + E_0) / T_L < 0.01, else undecided).  T_L = 0
    is the degenerate draw; it is decided when every e_k, k >= 1, is exactly 0 or their sum is below a quarter ulp of e_0,
    1.01 (1 + max rho) T_L < 2^-54 e_0: then no order of additions moves C off e_0.  Every figure is near 1e-13 for the
    cases of draw_theta_cases(); the near-ties at 1e-11 rest on that.
    """
    F = np.asarray(fstar, dtype=np.float64)
    Y = np.asarray(y, dtype=np.float64)
    us = np.asarray(u, dtype=np.float64)
    N, m = F.shape
    n = Y.shape[0]
    assert N == NGRID and Y.shape[1] == m and us.shape == (n,)
    assert not (np.abs(np.abs(F[np.isfinite(F)]) - EXP_OVERFLOW) < 1e-6).any(), "an f* at the overflow threshold decides nothing"
    if product == "fixed" and theta_hands_over(F):
        product = "gemm"
    FL = F.astype(LD)
    with np.errstate(over="ignore", invalid="ignore"):
        gp, gm = -np.log1p(np.exp(-FL)), -np.log1p(np.exp(FL))
        gp[-F > EXP_OVERFLOW] = -np.inf
        gm[F > EXP_OVERFLOW] = -np.inf
    sp, ap, ip, npn = _masked_product(gp, Y == 1.0)
    sm, am, im, nmn = _masked_product(gm, Y == -1.0)
    lp = sp + sm
    lp[(ip + im) > 0] = -np.inf
    lp[(npn + nmn) > 0] = np.nan
    sum_abs = ap + am                                                     # N x n
    n_obs = ((Y == 1.0) | (Y == -1.0)).sum(axis=1).astype(np.float64)     # n
    term_err = U51 * sum_abs + U50 * n_obs[None, :]
    with np.errstate(invalid="ignore"):
        lp_abs = np.where(np.isfinite(lp), np.abs(lp), LD(0)).astype(np.float64)
    if product == "fixed":
        e_k = np.floor(np.log2(np.abs(F).max(axis=1) + np.log(2.0))) + 1
        prod_err = n_obs[None, :] * 2.0 ** (e_k - 55)[:, None] + np.spacing(lp_abs)
        h = SCAN_DEPTH
    elif product == "gemm":
        prod_err = 1.01 * (2 * m) * U53 * sum_abs
        h = SCAN_DEPTH
    else:
        assert product == "oracle"
        prod_err = 1.01 * m * U53 * sum_abs
        h = N
    lp_bound = prod_err + term_err
    ts = grid()
    prior = -(LN_SQRT_2PI + LD(0.5) * ts.astype(LD) ** 2)
    P = prior[:, None] + lp
    fin = np.isfinite(P)
    Pabs = np.where(fin, np.abs(P), LD(0)).astype(np.float64)
    eps = lp_bound + (3 * U53 * np.abs(prior).astype(np.float64) + U50 * np.abs(ts))[:, None] + U53 * Pabs
    if stabilise:
        with np.errstate(invalid="ignore"):
            mx = np.where(np.isnan(P), LD(-np.inf), P).max(axis=0)        # -inf: every row -inf or NaN -> P - mx is NaN
            P = P - mx[None, :]
        eps = eps + U53 * np.where(np.isfinite(P), np.abs(P), LD(0)).astype(np.float64)
    eps = np.where(fin, eps, 0.0)
    with np.errstate(under="ignore", invalid="ignore"):
        e = np.exp(P)
        e[P < EXP_UNDERFLOW] = 0
    near_flush = (np.abs(np.where(np.isfinite(P), P, LD(0)).astype(np.float64) - EXP_UNDERFLOW) < 1e-6).any(axis=0)
    rho = np.where(eps < 0.01, 1.01 * eps + U51, np.inf)
    with np.errstate(invalid="ignore"):
        re = np.where(e == 0, LD(0), rho.astype(LD) * e)
    C = np.cumsum(e, axis=0)
    e_tail = e.copy()
    e_tail[0] = 0
    T = np.cumsum(e_tail, axis=0)
    with np.errstate(invalid="ignore"):
        E = (np.cumsum(re, axis=0) + 1.01 * h * U53 * C).astype(np.float64) \
            + (np.arange(1, N + 1, dtype=np.float64) * 2.0 ** -1074)[:, None]
    index = np.full(n, -1, dtype=np.int64)
    margin = np.full(n, np.inf)
    bound = np.zeros(n)
    undecided = np.zeros(n, dtype=bool)
    cdf = np.full((N, n), LD("nan"))
    for i in range(n):
        bad = np.flatnonzero(np.isnan(C[:, i]))
        L = (bad[0] if bad.size else N) - 1
        if L < 0:
            continue                                                      # NaN from row 0 on: degenerate under every rounding
        TL, e0 = T[L, i], e[0, i]
        if TL == 0:
            undecided[i] = bool(near_flush[i])
            continue
        rmax = float(rho[:L + 1, i].max())
        if 1.01 * (1 + rmax) * TL < LD(2.0 ** -54) * e0:
            continue                                                      # absorbed by C_0 in any order of additions
        c = T[:L + 1, i] / TL
        cdf[:L + 1, i] = c
        k = int(np.argmax(c > us[i]))                                     # (c[L] = 1 > u: some row exceeds u)
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
    return dict(index=index, cdf=cdf, logpost=lp, lp_bound=lp_bound, margin=margin, bound=bound, undecided=undecided,
                degenerate=int((index < 0).sum()), product=product)


# ------------------------------------------------------------------------------------------- draw_theta_cases ------
THETA_SEED, THETA_IT = 19, 3           # chosen so that the conditions of tests/test_stage_exact_cpu.py hold
TIE_DELTAS = (1e-6, -1e-6, 1e-9, -1e-9, 1e-11, -1e-11)     # the derived bound is near 1e-13: 1e-11 stands as the issue set it
TIE_ROWS = (300, 700)                  # threads 75 and 175 of theta_sample_kernel: the second step needs the scan's base
ONE_ITEM_N = 130                       # ragged against the product's tiles of 128 respondents and 16 items
DENSE_N, DENSE_M, DENSE_K0, DENSE_J0 = 257, 48, 500, 7
_PATTERN = ("point", "last_row", "row_0", "tie", "tie", "peaked", "flat", "overflow", "tie", "point")


def theta_uniforms(seed, it, n):
    """u of respondent i: (seed, it, ST_THETA, item = respondent, index 0)"""
    return item_uniforms(seed, it, ST_THETA, np.arange(n, dtype=np.uint64), 0)


def _solve_two_point(p, prior1, prior2):
    """(a1, a2): f* at the two rows so that w1 / (w1 + w2) = p for one answer y = +1, w = exp(prior - log1p(exp(-a)))"""
    d = np.log(LD(p) / (1 - LD(p))) - (prior1 - prior2)                  # T(a1) - T(a2), T = -log1p(exp(-a))
    t = -np.log(LD(2)) - abs(d)                                           # the smaller of the two terms; the other is T(0)
    a = float(-np.log(np.expm1(-t)))
    return (a, 0.0) if d <= 0 else (0.0, a)


@functools.lru_cache(maxsize=None)
def draw_theta_cases():
    """name -> dict(y, fstar, kinds, k0): the constructed inputs of draw_theta, all drawn under (THETA_SEED, THETA_IT).

    one_item_finite / one_item_fallback: n = m = 130; respondent i answers +1 to item i alone (a "peaked" one also to item
    i + 1, the column of the "flat" respondent behind it, who answers nothing: one term cannot go below -709.78 without
    overflowing, two can), so column i designs that respondent's posterior.  f* away from the designed rows is -600
    (finite: the fixed-point product runs) or -800 (the written term overflows to -inf: the launch is handed to the fp64
    product).  kinds[i], in the pattern _PATTERN:
      point     point mass at the interior row k0[i] (f* = 30 there): theta = ts[k0] for every u
      last_row  ... at row 1000: theta = +5.0
      row_0     ... at row 0: cdf is 0/0, degenerate with and without stabilisation
      tie       two-point posterior at rows 300 and 700 with w1 / (w1 + w2) = u_i + delta, delta = TIE_DELTAS in turn
      flat      no observed cell: the prior alone
      peaked    log-posterior near -760: exp underflows to 0 without stabilisation (degenerate), an ordinary draw with it
      overflow  f* = -800 on the whole grid under the answer +1 (fallback only; "point" in the finite twin): every row -inf,
                degenerate with and without stabilisation
    dense_*: n = 257, m = 48, 7 % missing, respondent 0 answers nothing; smooth f*; dense_nan_cell has f*[500, 7] = NaN
    (respondents with item 7 missing must not see it), dense_nan_row f*[500, :] = NaN, dense_pm800 one +800 and one -800
    entry (under observed and missing cells alike), dense_overflow_item f*[:, 11] = +800 (whoever answered -1 to item 11
    is degenerate)."""
    ts = grid()
    prior = -(LN_SQRT_2PI + LD(0.5) * ts.astype(LD) ** 2)
    cases = {}
    n = ONE_ITEM_N
    u = theta_uniforms(THETA_SEED, THETA_IT, n)
    for name, out in (("one_item_finite", -600.0), ("one_item_fallback", -800.0)):
        F = np.full((NGRID, n), out, order="F")
        Y = np.full((n, n), np.nan, order="F")
        kinds, k0s, tie = [], np.full(n, -1), 0
        for i in range(n):
            kind = _PATTERN[i % len(_PATTERN)]
            if kind == "overflow" and out == -600.0:
                kind = "point"
            kinds.append(kind)
            if kind != "flat":
                Y[i, i] = 1.0
            if kind in ("point", "last_row", "row_0"):
                k0s[i] = {"point": 1 + (37 * i) % 999, "last_row": NGRID - 1, "row_0": 0}[kind]
                F[k0s[i], i] = 30.0
            elif kind == "tie":
                a1, a2 = _solve_two_point(u[i] + TIE_DELTAS[tie % len(TIE_DELTAS)], prior[TIE_ROWS[0]], prior[TIE_ROWS[1]])
                F[TIE_ROWS[0], i], F[TIE_ROWS[1], i] = a1, a2
                k0s[i] = tie % len(TIE_DELTAS)                            # (for ties: which delta)
                tie += 1
            elif kind == "peaked":
                bump = -380.0 - 0.5 * ((np.arange(NGRID) - (200 + 5 * i)) / 40.0) ** 2
                F[:, i] = bump
                F[:, i + 1] = bump
                Y[i, i + 1] = 1.0
        cases[name] = dict(y=Y, fstar=F, kinds=kinds, k0=k0s)
    n, m = DENSE_N, DENSE_M
    rng = np.random.default_rng(77)
    th = np.clip(rng.normal(size=n), -3, 3)
    b0, b1 = rng.normal(size=m) * 0.7, rng.uniform(0.5, 1.6, size=m) * np.where(rng.random(m) < 0.8, 1.0, -1.0)
    F0 = np.asfortranarray(b0[None, :] + ts[:, None] * b1[None, :] + 0.3 * np.sin(2.0 * ts)[:, None])
    pr = 1.0 / (1.0 + np.exp(-(b0[None, :] + th[:, None] * b1[None, :])))
    Y = np.where(rng.random((n, m)) < pr, 1.0, -1.0)
    Y[rng.random((n, m)) < 0.07] = np.nan
    Y[0, :] = np.nan
    Y[1, DENSE_J0], Y[2, DENSE_J0], Y[3, DENSE_J0] = np.nan, 1.0, -1.0
    Y = np.asfortranarray(Y)

    def dense(name, edit):
        F = F0.copy(order="F")
        edit(F)
        cases[name] = dict(y=Y, fstar=F, kinds=["dense"] * n, k0=np.full(n, -1))

    def _cell(F): F[DENSE_K0, DENSE_J0] = np.nan
    def _row(F): F[DENSE_K0, :] = np.nan
    def _pm(F): F[300, 3], F[650, 5] = 800.0, -800.0
    def _item(F): F[:, 11] = 800.0
    dense("dense_smooth", lambda F: None)
    dense("dense_nan_cell", _cell)
    dense("dense_nan_row", _row)
    dense("dense_pm800", _pm)
    dense("dense_overflow_item", _item)
    return cases


@functools.lru_cache(maxsize=None)
def draw_theta_reference(name, stabilise, product):
    c = draw_theta_cases()[name]
    return theta_exact(c["y"], c["fstar"], theta_uniforms(THETA_SEED, THETA_IT, c["y"].shape[0]), stabilise, product)


# ------------------------------------------------------------------------------------------------- beta_exact ------
def _dnorm_log(x, mu, sd):
    z = np.abs((LD(x) - LD(mu)) / LD(sd))
    return -(LN_SQRT_2PI + LD(0.5) * z * z + np.log(LD(sd)))


def beta_exact(beta, theta, y, f, pm, ps, step, z, u):
    """draw_beta (src/draw-beta.cpp:3-41) for ONE item in long double: beta, pm, ps, step, z, u are pairs (z: the normals at
    index 0 and 2 of the item's sub-stream, u: the uniforms at index 1 and 3), theta, y, f its n rows.  The proposal
    cv + step z (R::rnorm: step = 0 returns cv) is carried in fp64, as are the arguments a_i = y_i (f_i + (b0 + theta_i
    b1)); the terms are the "written" ones of slice_exact -- log(1 + exp(-a)) evaluated in fp64 from the fp64 argument, which
    is what ll_term computes (+inf for a < -709.78) -- added in long double; the priors (R::dnorm, log) and r (:29) are long
    double.

    Returns a dict: beta (the new pair, fp64), accept (2 bools), r, margin = |log u - r| and bound per step, proposal
    (what was proposed), overflow (per step: (proposal's ll is -inf, current's is)), undecided (count).

    THE BOUND on |device r - r| (u = 2^-53):
      * the proposal: mu + sd z contracted into an fma or not differs by one ulp, d = ulp(max(|cv|, |pv|)); once accepted it
        is the current value and its d stays with it.  Through the prior that is d z / sd, through the argument d |x_ik|
        (x_i = (1, theta_i));
      * da_i: b0 + theta_i b1, then f_i + that -- two sums and a product, each u relative, fma or not:
        3 u (|b0| + |theta_i b1| + |f_i|), plus the d's; y = +-1 multiplies exactly;
      * the term: |T'| <= 1 hands da_i on; its own error 2^-51 |T_i| + 2^-50 (slice_exact);
      * the sum: 1.01 h u sum|T_i|, h = sum_depth(n) (a lane adds ceil(n / 256) terms, then 6 shuffle levels and 2 more);
      * the two priors -(log sqrt(2 pi) + z^2 / 2 + log sd): z from a difference and a quotient, squared, halved and added,
        the library's log within an ulp: 8 u (log sqrt(2 pi) + z^2 / 2 + |log sd|) each;
      * r: three additions, 3 u (|pv_prior| + |pv_ll| + |cv_prior| + |cv_ll|);  log u: 2^-51 |log u|.
    DECIDED WITHOUT A MARGIN: step = 0 makes pv = cv, both priors and both sums the same fp64 expressions, r = 0 exactly and
    log u < 0: accepted.  A sum with an overflowing term is -inf under every rounding when no observed a_i is within 1e-6 of
    the threshold (else: undecided): both overflow, r = NaN, rejected; the proposal alone, r = -inf, rejected; the current
    state alone, r = +inf, accepted."""
    th = np.asarray(theta, dtype=np.float64)
    yv, fv = np.asarray(y, dtype=np.float64), np.asarray(f, dtype=np.float64)
    obs = np.flatnonzero(~np.isnan(yv))
    tho, yo, fo = th[obs], yv[obs], fv[obs]
    h = sum_depth(len(th))
    cv = [float(beta[0]), float(beta[1])]
    dcv = [0.0, 0.0]
    x_abs = (np.ones_like(tho), np.abs(tho))

    def ll(b, db):
        a = yo * (fo + (b[0] + tho * b[1]))
        with np.errstate(over="ignore"):
            T = np.log(1.0 + np.exp(-a))
        over = bool(np.isinf(T).any())
        edge = bool((np.abs(a + EXP_OVERFLOW) < 1e-6).any())
        if over:
            return LD(-np.inf), 0.0, True, edge
        sabs = float(T.sum())
        da = 3 * U53 * (abs(b[0]) + np.abs(tho * b[1]) + np.abs(fo)) + db[0] * x_abs[0] + db[1] * x_abs[1]
        err = float(da.sum()) + U51 * sabs + U50 * len(T) + 1.01 * h * U53 * sabs
        return -(T.astype(LD).sum() if len(T) else LD(0)), err, False, edge

    out = dict(accept=[], r=[], margin=[], bound=[], proposal=[], overflow=[], undecided=0)
    for k in range(2):
        s = float(step[k])
        pv = list(cv)
        pv[k] = cv[k] if s == 0.0 else cv[k] + s * float(z[k])
        d = 0.0 if s == 0.0 else float(np.spacing(max(abs(cv[k]), abs(pv[k]))))
        dpv = list(dcv)
        dpv[k] = max(dcv[k], d)
        pvp, cvp = _dnorm_log(pv[k], pm[k], ps[k]), _dnorm_log(cv[k], pm[k], ps[k])
        pll, perr, pover, pedge = ll(pv, dpv)
        cll, cerr, cover, cedge = ll(cv, dcv)
        logu = np.log(LD(float(u[k])))
        out["proposal"].append(pv[k])
        out["overflow"].append((pover, cover))
        if pover or cover:
            r = LD("nan") if (pover and cover) else (LD(-np.inf) if pover else LD(np.inf))
            acc, mg, bd = bool(cover and not pover), np.inf, 0.0
            und = pedge or cedge
        elif s == 0.0:
            r, acc, mg, bd, und = LD(0), True, abs(float(logu)), 0.0, False
        else:
            r = pvp + pll - cvp - cll
            zp, zc = abs(pv[k] - pm[k]) / ps[k], abs(cv[k] - pm[k]) / ps[k]
            lsd = abs(float(np.log(ps[k])))
            bd = (perr + cerr + 8 * U53 * (2 * float(LN_SQRT_2PI) + 0.5 * zp * zp + 0.5 * zc * zc + 2 * lsd)
                  + (dpv[k] * zp + dcv[k] * zc) / ps[k]
                  + 3 * U53 * float(abs(pvp) + abs(pll) + abs(cvp) + abs(cll)) + U51 * abs(float(logu)))
            mg = abs(float(logu - r))
            acc = bool(logu < r)
            und = mg < bd or pedge or cedge
        out["accept"].append(acc); out["r"].append(r); out["margin"].append(mg); out["bound"].append(bd)
        out["undecided"] += int(bool(und))
        if acc:
            cv, dcv = pv, dpv
    out["beta"] = np.array(cv)
    return out


# -------------------------------------------------------------------------------------------- draw_beta_cases ------
BETA_ORDERS = (1, 100, 256, 257, 1000)          # 256 | 257: the edges of draw_beta_kernel's 256-thread strided loop
BETA_SEED = {1: 3, 100: 5, 256: 7, 257: 9, 1000: 13}     # chosen so that the conditions of tests/test_stage_exact_cpu.py hold
BETA_IT = 4
BETA_TIES = (("tie_s0_p6", 0, 1e-6), ("tie_s0_m6", 0, -1e-6), ("tie_s0_p9", 0, 1e-9), ("tie_s0_m9", 0, -1e-9),
             ("tie_s1_p6", 1, 1e-6), ("tie_s1_m6", 1, -1e-6), ("tie_s1_p9", 1, 1e-9), ("tie_s1_m9", 1, -1e-9))


def beta_randoms(seed, it, m):
    """(z, u), each 2 x m: z at index 2k, u at index 2k + 1 of item j's sub-stream"""
    U = item_uniforms(seed, it, ST_BETA, np.arange(m, dtype=np.uint64)[None, :], np.arange(4, dtype=np.uint64)[:, None])
    return qnorm(U[0::2]), U[1::2]


@functools.lru_cache(maxsize=None)
def draw_beta_cases(n):
    """dict(names, beta, theta, y, f, pm, ps, step): one launch at n rows, one column per name, keys (BETA_SEED[n], BETA_IT).
    theta[0] = 5 and (n > 1) theta[1] = -5; both rows are observed in every column but no_observed_row.
      ordinary;  step0_zero, step1_zero, both_zero (r = 0 exactly: accepted);  no_observed_row;  single_observed_row;
      tight_prior (ps = 1e-3, pm two away from beta);
      tie_s<k>_<p|m><6|9>: pm[k] solved (r is linear in it) so that r = log u +- 1e-6 | 1e-9 at step k; the ties at step 1
        stand behind a step 0 forced like accept_then_decide (the 1e-6 pair) and reject_then_decide (the 1e-9 pair), so a
        kept log-likelihood taken from the wrong branch -- an error of |pv_ll - cv_ll| of step 0 in r -- flips one of each pair;
        the last row is observed in every tie column, so a loop that misses it flips one of each pair too;
      accept_then_decide, reject_then_decide: pm[0] solved for r = log u +- 1 at step 0 -- the two branches that hand the
        kept log-likelihood to step 1, which then decides by its own ordinary margin;
      both_overflow: the current state and the proposal overflow (cv0 = -+2000): r = NaN, rejected twice;
      proposal_overflow: step0 = 2000 / |z0| against row 0's answer: r = -inf, rejected;
      current_overflow: cv0 = -+1000 and step0 = 1000 / |z0| bring the proposal back to ~0: r = +inf, accepted;
      proposal_overflow_s1: step1 = 200 / |z1| times theta = +-5 against the answers of rows 0 and 1: rejected."""
    seed, it = BETA_SEED[n], BETA_IT
    rng = np.random.default_rng(500 + n)
    names = (["ordinary", "step0_zero", "step1_zero", "both_zero", "no_observed_row", "single_observed_row", "tight_prior"]
             + [t[0] for t in BETA_TIES] + ["accept_then_decide", "reject_then_decide", "both_overflow", "proposal_overflow",
                                            "current_overflow", "proposal_overflow_s1"])
    m = len(names)
    col = {nm: j for j, nm in enumerate(names)}
    z, u = beta_randoms(seed, it, m)
    theta = np.clip(rng.normal(size=n), -4.9, 4.9)
    theta[0] = 5.0
    if n > 1:
        theta[1] = -5.0
    beta = np.asfortranarray(np.stack([rng.normal(size=m) * 0.5, rng.uniform(0.6, 1.4, size=m)]))
    f = np.asfortranarray(rng.normal(size=(n, m)) * 0.5)
    pr = 1.0 / (1.0 + np.exp(-(f + beta[0][None, :] + theta[:, None] * beta[1][None, :])))
    y = np.where(rng.random((n, m)) < pr, 1.0, -1.0)
    y[rng.random((n, m)) < 0.06] = np.nan
    y[:2, :] = np.where(np.isnan(y[:2, :]), 1.0, y[:2, :])
    pm, ps, step = np.zeros((2, m), order="F"), np.full((2, m), 3.0, order="F"), np.full((2, m), 0.1, order="F")
    step[0, col["step0_zero"]] = step[1, col["step1_zero"]] = 0.0
    step[:, col["both_zero"]] = 0.0
    y[:, col["no_observed_row"]] = np.nan
    j = col["single_observed_row"]
    keep = y[n // 2, j] if not np.isnan(y[n // 2, j]) else 1.0
    y[:, j] = np.nan
    y[n // 2, j] = keep
    j = col["tight_prior"]
    ps[:, j] = 1e-3
    pm[:, j] = beta[:, j] + 2.0
    j = col["both_overflow"]
    beta[0, j] = -2000.0 * y[0, j]
    j = col["proposal_overflow"]
    step[0, j] = 2000.0 / abs(z[0, j])
    y[0, j] = -np.sign(z[0, j])
    j = col["current_overflow"]
    beta[0, j] = -np.sign(z[0, j]) * 1000.0
    step[0, j] = 1000.0 / abs(z[0, j])
    y[0, j] = np.sign(z[0, j])
    j = col["proposal_overflow_s1"]
    step[1, j] = 200.0 / abs(z[1, j])
    y[0, j] = -np.sign(z[1, j])
    if n > 1:
        y[1, j] = np.sign(z[1, j])
    if n > 2:                                        # the last row (row 256 of 257) is observed wherever a near-tie would miss it
        tie_cols = [col[t[0]] for t in BETA_TIES]
        y[n - 1, tie_cols] = np.where(np.isnan(y[n - 1, tie_cols]), 1.0, y[n - 1, tie_cols])
    y = np.asfortranarray(y)

    def solve(j, k, delta):
        step[:, j] = 0.5
        pm[k, j] = 0.0
        ref = beta_exact(beta[:, j], theta, y[:, j], f[:, j], pm[:, j], ps[:, j], step[:, j], z[:, j], u[:, j])
        slope = (LD(ref["proposal"][k]) - LD(beta[k, j])) / (LD(ps[k, j]) ** 2)        # d r / d pm[k]: (pv - cv) / ps^2
        pm[k, j] = float((np.log(LD(u[k, j])) + LD(delta) - ref["r"][k]) / slope)

    for nm, k, delta in BETA_TIES:
        if k == 1:                                   # the tie at step 1 behind a forced step 0: accepted (1e-6), rejected (1e-9)
            solve(col[nm], 0, 1.0 if abs(delta) == 1e-6 else -1.0)
        solve(col[nm], k, delta)
    solve(col["accept_then_decide"], 0, 1.0)
    solve(col["reject_then_decide"], 0, -1.0)
    return dict(names=names, beta=beta, theta=theta, y=y, f=f, pm=pm, ps=ps, step=step, seed=seed, it=it)


def draw_beta_reference(n, z=None):
    """beta_exact for every column of draw_beta_cases(n); z (2 x m): the normals as the device drew them (default: restated)"""
    c = draw_beta_cases(n)
    zr, u = beta_randoms(c["seed"], c["it"], len(c["names"]))
    z = zr if z is None else z
    return [beta_exact(c["beta"][:, j], c["theta"], c["y"][:, j], c["f"][:, j], c["pm"][:, j], c["ps"][:, j], c["step"][:, j],
                       z[:, j], u[:, j]) for j in range(len(c["names"]))]
