"""Long-double references of the two stages the headline iteration spends its time in behind the factorisation, and the
constructed inputs the GPU tests feed them (tests/test_gpu_draw_f_constructed.py, tests/test_gpu_fstar_ranks.py).

  slice_exact        one column of ess(), src/draw-f.cpp:21-60, with a derived bound on the device's rounding
  fstar_rank_exact   draw_fstar through K(theta, theta*) = K(theta, c) V^T at r Chebyshev nodes (r = 0: the full solve)
  item_uniforms / item_normals   the counter-based item RNG restated in NumPy (checked against the oracle's)
  draw_f_cases       the constructed columns of the draw_f test, per order n and scale sigma of L = sigma I

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
