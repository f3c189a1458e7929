"""Per-item GP amplitudes, fixed or sampled in the chain (include/gpirt_hip.h, "per-item GP amplitudes": gpirt_amp_check,
gpirt_sampler_amp_*, gpirt_sampler_draw_amp; csrc/amp.hip, csrc/sampler.hip).

Item j has an amplitude a_j > 0 and the prior f_j ~ N(0, a_j^2 (K + 0.001 I)): the amplitude multiplies the whole prior, jitter
included, so item j's model is a_j times the reference's unit model.  The factor L stays shared by all items; draw_f's prior
draw is a_j L z_j, draw_fstar's mean is unchanged and its standard deviation is a_j s.  a_j -> 0 says item j is a 2PL item, a
large a_j that the data need a nonparametric curve.

Sampled, a_j lives on a fixed logarithmic grid a_k = lo (hi / lo)^(k / (P - 1)) (gpirt_ell_grid's), the chain's state per item
is the index k_j, and the prior is a table of P finite log masses on the grid, i.e. a density with respect to log a; the default
-(ln a_k)^2 / 2 (log-normal, median 1, log-sd 1) is a choice, not a measurement.  The update is the prior-whitened Metropolis
step of Murray & Adams (2010, section 2.2) per item: nu_j = L^-1 f_j / a_j is held fixed, a proposal moves
f_j' = (a_k' / a_k) f_j and the likelihood decides.  All m items are updated in one launch with no host read.

`run` is the one-call way in: gpirt_amd.kernel.run's stage loop with Sampler.draw_amp() after every `every`-th step() and
Sampler.amp_record() per kept draw.  `step_exact` is the NumPy statement of one update of all items (c and f' in fp64 exactly as
the device forms them, everything after them in long double), `conditional_posterior` the exact discrete
p(k_j' | nu_j, theta, mu, y) per item.

Beside it, since library version 135, the centred update on the GP's rank-64 smooth part (Sampler.draw_amp_centred,
csrc/amp_centred.hip): `centred_basis`, `centred_exact_coef` and `centred_exact_update` are its NumPy statement,
`centred_normals` and `centred_uniforms` its draws, and `run(update="both")` runs the two in turn.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import ST_AMP, check
from .ell import ADAPT_EVERY, ADAPT_HIGH, ADAPT_LOW, LD, ll_term, proposal  # noqa: F401  (ll_term: the long-double term)


# ---------------------------------------------------------------------------------------------------- the contract ---
def grid(lo=0.1, hi=10.0, points=129) -> np.ndarray:
    """a_k = lo (hi / lo)^(k / (points - 1)), k = 0 .. points - 1, as the library keeps it (gpirt_ell_grid: long double on the
    host, rounded to fp64, the end points exact).  2 <= points <= 1025 and 0.01 <= lo < hi <= 1000, else GpirtError."""
    P = int(points)
    out = np.empty(max(P, 1))
    check(_lib.load().gpirt_ell_grid(float(lo), float(hi), P, out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def default_log_prior(amp_grid) -> np.ndarray:
    """-(ln a_k)^2 / 2: a log-normal mass with median 1 and log-sd 1 on the grid (long double, rounded to fp64)."""
    l = np.log(np.asarray(amp_grid, dtype=np.float64).astype(LD))
    return (-(l * l) / LD(2)).astype(np.float64)


def nearest_one(amp_grid) -> int:
    """the index of the grid point nearest 1 in log a (the first of a tie): where every item starts when k0 is not given"""
    return int(np.argmin(np.abs(np.log(np.asarray(amp_grid, dtype=np.float64).astype(LD)))))


def check_args(lo, hi, points, log_prior=None, width=4, k0=None, m=0, options=None) -> None:
    """gpirt_amp_check (no device is touched): every refusal of Sampler.amp_enable's arguments as a GpirtError that names its
    reason.  k0: None or m indices; options: a gpirt_options (_lib.Options) or None."""
    lp = None if log_prior is None else np.ascontiguousarray(log_prior, dtype=np.float64)
    if lp is not None and lp.shape != (int(points),):
        raise ValueError(f"amp: log_prior must hold points = {int(points)} values")
    kk = None if k0 is None else np.ascontiguousarray(k0, dtype=np.int32).reshape(-1)
    if kk is not None and kk.shape != (int(m),):
        raise ValueError(f"amp: k0 must hold m = {int(m)} indices")
    check(_lib.load().gpirt_amp_check(float(lo), float(hi), int(points), None if lp is None else lp.ctypes.data_as(C.POINTER(C.c_double)),
                                      int(width), None if kk is None else kk.ctypes.data_as(C.POINTER(C.c_int)), int(m),
                                      None if options is None else C.byref(options)))


def uniforms(seed, t, item) -> tuple:
    """(u0, u1) of item `item` in the t-th draw_amp call on a sampler (t counted from 1): item_uniform(seed, t, GPIRT_ST_AMP,
    item, 0 / 1).  item may be an array (item0 + j): two arrays come back."""
    from .ppc import item_uniform
    it = np.asarray(item, dtype=np.uint64)
    u = item_uniform(seed, int(t), ST_AMP, it[..., None], np.arange(2, dtype=np.uint64))
    if it.ndim == 0:
        return float(u[0]), float(u[1])
    return u[..., 0], u[..., 1]


# ------------------------------------------------------------------------------------------------------- NumPy -------
def _loglik(fcol, mucol, ycol):
    """-sum over observed rows of t(y (f + mu)) in long double (fcol long double)"""
    obs = ~np.isnan(ycol)
    ys = np.where(obs, ycol, 0.0).astype(LD)
    with np.errstate(all="ignore"):
        return -np.where(obs, ll_term(ys * (fcol + mucol.astype(LD))), LD(0)).sum()


def step_exact(f, mu, y, k, widths, seed, t, amp_grid, log_prior, item0=0) -> dict:
    """One update of all items as gpirt_sampler_draw_amp states it.  f, mu, y (n x m; y of +1 / -1 / NaN), k and widths (m), the
    sampler's seed, t the count of draw_amp calls including this one, the tables.  c = grid[k'] / grid[k] and f' = c f are fp64,
    formed as the device forms them; everything after them is long double.
    Returns dict(status (m of "accepted", "rejected", "out_of_range", "failed"), k (the indices afterwards), k_prop, f (fp64: c f
    in the accepted columns, else as given), amplitude (grid[k] afterwards), u0, u1, and per item -- NaN where the update was
    out of range -- c, dll, log_ratio, log_u (long double), nonfinite (rows whose f' is not finite))."""
    g = np.asarray(amp_grid, dtype=np.float64)
    lp = np.asarray(log_prior, dtype=np.float64)
    P = g.shape[0]
    f = np.asarray(f, dtype=np.float64)
    mu = np.asarray(mu, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n, m = f.shape
    k = np.asarray(k, dtype=np.int64).reshape(m)
    widths = np.broadcast_to(np.asarray(widths, dtype=np.int64), (m,))
    u0, u1 = uniforms(seed, t, np.arange(m, dtype=np.uint64) + np.uint64(item0))
    out_f, out_k = f.copy(order="F"), k.copy()
    k_prop = np.empty(m, dtype=np.int64)
    status = []
    nan = LD(np.nan)
    c = np.full(m, np.nan)
    dll, ratio, log_u = np.full(m, nan, dtype=LD), np.full(m, nan, dtype=LD), np.full(m, nan, dtype=LD)
    nonfinite = np.zeros(m, dtype=np.int64)
    for j in range(m):
        kp = int(k[j]) + proposal(u0[j], widths[j])
        k_prop[j] = kp
        if kp < 0 or kp >= P:
            status.append("out_of_range")
            continue
        with np.errstate(all="ignore"):
            c[j] = g[kp] / g[k[j]]                                   # one fp64 division
            fp = c[j] * f[:, j]                                      # one fp64 multiplication per row
            nonfinite[j] = int((~np.isfinite(fp)).sum())
            obs = ~np.isnan(y[:, j])
            ys = np.where(obs, y[:, j], 0.0).astype(LD)
            terms = np.where(obs, ll_term(ys * (f[:, j].astype(LD) + mu[:, j].astype(LD))) - ll_term(ys * (fp.astype(LD) + mu[:, j].astype(LD))), LD(0))
            dll[j] = terms.sum()                                     # cell by cell, a difference of the two terms
        ratio[j] = dll[j] + (LD(lp[kp]) - LD(lp[k[j]]))
        log_u[j] = np.log(LD(u1[j]))
        if nonfinite[j] or not np.isfinite(dll[j]):
            status.append("failed")
        elif log_u[j] < ratio[j]:
            status.append("accepted")
            out_k[j] = kp
            out_f[:, j] = fp
        else:
            status.append("rejected")
    return dict(status=status, k=out_k, k_prop=k_prop, f=out_f, amplitude=g[out_k], u0=u0, u1=u1, c=c, dll=dll, log_ratio=ratio,
                log_u=log_u, nonfinite=nonfinite)


def conditional_posterior(f, k, mu, y, amp_grid, log_prior) -> np.ndarray:
    """p(k' | nu_j, theta, mu, y) per item on the grid (P x m) by direct summation: with nu_j = L^-1 f_j / a_k held fixed the
    curve at k' is (a_k' / a_k) f_j, so the mass is proportional to exp(log_prior[k'] - sum over observed rows of
    t(y ((a_k' / a_k) f + mu))), in long double: the stationary distribution of the update."""
    g = np.asarray(amp_grid, dtype=np.float64).astype(LD)
    f = np.asarray(f, dtype=np.float64)
    mu = np.asarray(mu, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    m = f.shape[1]
    k = np.asarray(k, dtype=np.int64).reshape(m)
    out = np.empty((g.shape[0], m))
    for j in range(m):
        lw = np.array([LD(log_prior[kk]) + _loglik((g[kk] / g[k[j]]) * f[:, j].astype(LD), mu[:, j], y[:, j])
                       for kk in range(g.shape[0])], dtype=LD)
        w = np.exp(lw - lw.max())
        out[:, j] = (w / w.sum()).astype(np.float64)
    return out


# ------------------------------------------------------------------------- the centred update: the NumPy statement ---
# gpirt_sampler_draw_amp_centred (include/gpirt_hip.h, "a centred amplitude update"; csrc/amp_centred.hip).  With Phi = V F
# (V the Lagrange basis at theta on the 64 Chebyshev nodes, Kcc = F F^T) and eps the jitter the model
# f_j ~ N(0, a_j^2 (K + eps I)) is the marginal of xi_j ~ N(0, a_j^2 I_r), e_j ~ N(0, eps I_n), f_j = Phi xi_j + a_j e_j:
# the update draws xi_j | f_j, a_j, proposes k' from the exact discrete conditional of a given xi_j alone, moves f_j with the
# nugget's whitened coordinates held fixed and lets the likelihood decide.
U = 2.0 ** -53
DEAD = 1e-13                      # a column of F whose squared norm (the eigenvalue of Kcc) is at most this is dead
JITTER = 1.0e-3
_AS241 = (
    ((2509.0809287301226727, 33430.575583588128105, 67265.770927008700853, 45921.953931549871457, 13731.693765509461125,
      1971.5909503065514427, 133.14166789178437745, 3.387132872796366608),
     (5226.495278852545925, 28729.085735721942674, 39307.89580009271061, 21213.794301586595867, 5394.1960214247511077,
      687.1870074920579083, 42.313330701600911252, 1.0)),
    ((7.7454501427834140764e-4, 0.0227238449892691845833, 0.24178072517745061177, 1.27045825245236838258,
      3.64784832476320460504, 5.7694972214606914055, 4.6303378461565452959, 1.42343711074968357734),
     (1.05075007164441684324e-9, 5.475938084995344946e-4, 0.0151986665636164571966, 0.14810397642748007459,
      0.68976733498510000455, 1.6763848301838038494, 2.05319162663775882187, 1.0)),
    ((2.01033439929228813265e-7, 2.71155556874348757815e-5, 0.0012426609473880784386, 0.026532189526576123093,
      0.29656057182850489123, 1.7848265399172913358, 5.4637849111641143699, 6.6579046435011037772),
     (2.04426310338993978564e-15, 1.4215117583164458887e-7, 1.8463183175100546818e-5, 7.868691311456132591e-4,
      0.0148753612908506148525, 0.13692988092273580531, 0.59983220655588793769, 1.0)))


def _qnorm(p):
    """Wichura's AS 241 (PPND16) in fp64, R's Horner order (csrc/common.h qnorm_as241)"""
    def horner(r, coef):
        acc = np.full_like(r, coef[0])
        for c in coef[1:]:
            acc = acc * r + c
        return acc
    p = np.asarray(p, dtype=np.float64)
    q = p - 0.5
    out = np.empty_like(p)
    mid = np.abs(q) <= 0.425
    r = 0.180625 - q[mid] * q[mid]
    out[mid] = q[mid] * horner(r, _AS241[0][0]) / horner(r, _AS241[0][1])
    t = ~mid
    r = np.sqrt(-np.log(np.where(q[t] < 0, p[t], 1.0 - p[t])))
    near = r <= 5.0
    val = np.empty_like(r)
    val[near] = horner(r[near] - 1.6, _AS241[1][0]) / horner(r[near] - 1.6, _AS241[1][1])
    val[~near] = horner(r[~near] - 5.0, _AS241[2][0]) / horner(r[~near] - 5.0, _AS241[2][1])
    out[t] = np.where(q[t] < 0, -val, val)
    return out


def centred_uniforms(seed, t, item) -> tuple:
    """(u0, u1) of item `item` in the t-th draw_amp_centred call (t counted from 1): item_uniform(seed, t, GPIRT_ST_AMP_CENTRED,
    item, 64 / 65).  item may be an array (item0 + j): two arrays come back."""
    from .ppc import item_uniform
    it = np.asarray(item, dtype=np.uint64)
    u = item_uniform(seed, int(t), _lib.ST_AMP_CENTRED, it[..., None], np.arange(64, 66, dtype=np.uint64))
    if it.ndim == 0:
        return float(u[0]), float(u[1])
    return u[..., 0], u[..., 1]


def centred_normals(seed, t, item, handle=None) -> np.ndarray:
    """z (64 x len(item)): z[k, j] = qnorm(item_uniform(seed, t, GPIRT_ST_AMP_CENTRED, item[j], k)), the 64 normals of the
    augmentation in the t-th draw_amp_centred call.  The uniforms are integer arithmetic and the same bits everywhere.  AS 241
    takes a logarithm in its tails and the device library's differs from the host's in the last place there, so, as
    gpirt_amd.consistent states the carry's normals, the bits of the statement are the device's: with `handle` (a Handle) they
    come from gpirt_item_normals; without one they are evaluated here, equal in the central branch |u - 0.5| <= 0.425 and within
    4e-15 relative in the tails."""
    from .ppc import item_uniform
    items = np.atleast_1d(np.asarray(item, dtype=np.uint64))
    if handle is not None:
        from .ops import to_host
        if items.size and np.any(np.diff(items.astype(np.int64)) != 1):
            raise ValueError("centred_normals: with a handle the items must be consecutive")
        return np.asfortranarray(to_host(handle.item_normals(int(seed), int(t), _lib.ST_AMP_CENTRED, int(items[0]), int(items.size),
                                                             _lib.AMP_CENTRED_RANK)))
    u = item_uniform(seed, int(t), _lib.ST_AMP_CENTRED, items[None, :], np.arange(_lib.AMP_CENTRED_RANK, dtype=np.uint64)[:, None])
    return np.asfortranarray(_qnorm(u))


_FACTORS = {}


def centred_factor(kernel=None) -> tuple:
    """(F, live, r): F (64 x 64 fp64) with K(c, c) = F F^T at the 64 nodes as the library forms it on the host -- Kcc and a cyclic
    Jacobi eigendecomposition in long double, F = Q sqrt(max(Lambda, 0)) rounded to fp64 --, then the dead columns (squared norm
    <= 1e-13) zeroed; live: 64 booleans; r their count.  Squared-exponential kernels only.  Cached per length scale."""
    from . import fstar_free as FF, kernel as K
    fam, ell = K.spec(kernel)
    if K.family_name(fam) != "se":
        raise ValueError("centred_factor: a Matern kernel has no rank-64 form")
    if ell not in _FACTORS:
        c, _ = FF.nodes()
        d = np.abs(c.astype(LD)[:, None] - c.astype(LD)[None, :]) / LD(ell)
        lam, Q = FF.jacobi_eigh(np.exp(LD(-0.5) * d * d))
        F = (Q * np.sqrt(np.maximum(lam, LD(0)))[None, :]).astype(np.float64)
        live = (F.astype(LD) ** 2).sum(axis=0) > LD(DEAD)
        F[:, ~live] = 0.0
        _FACTORS[ell] = (F, live, int(live.sum()))
    F, live, r = _FACTORS[ell]
    return F.copy(), live.copy(), r


def centred_basis(theta, kernel=None, F=None) -> tuple:
    """(Phi, live, r): Phi = V F (n x 64, long double) with V the fp64 basis at theta (gpirt_amd.fstar_free.basis) and F of
    `centred_factor` (or the 64 x 64 `F` given, e.g. the device's amp_get("centred_F")); Phi Phi^T is K(theta, theta) to 1e-13."""
    from . import fstar_free as FF
    if F is None:
        F, live, r = centred_factor(kernel)
    else:
        F = np.asarray(F, dtype=np.float64)
        live = (F != 0.0).any(axis=0)
        r = int(live.sum())
    return FF.basis(theta).astype(LD) @ F.astype(LD), live, r


def centred_exact_coef(theta, f, a, seed, t, item0=0, kernel=None, F=None, z=None, eps=JITTER) -> dict:
    """Steps 1 to 3's fixed part for all items in long double.  theta (n), f (n x m fp64), a (m amplitudes), the sampler's seed,
    t the count of draw_amp_centred calls including this one.  z: the 64 x m normals (None: centred_normals without a handle).
    A = Phi^T Phi + eps I = R R^T, t_j = R^-1 Phi^T f_j, w_j = t_j + (a_j sqrt(eps)) z_j with the sd and its product in fp64
    as the device forms them, xi_j = R^-T w_j, Q_j = |xi_j|^2 over the live coordinates, g_j = F xi_j, h_j = V g_j.
    Returns dict(V (fp64), F, live, r, A, R, T = V^T f, t, z, w, xi, Q, g, H, cond = cond_2(A)); long double but V, F, z."""
    from . import fstar_free as FF
    f = np.asarray(f, dtype=np.float64)
    n, m = f.shape
    V = FF.basis(theta)
    Phi, live, r = centred_basis(theta, kernel, F)
    if F is None:
        F = centred_factor(kernel)[0]
    F = np.asarray(F, dtype=np.float64)
    if z is None:
        z = centred_normals(seed, t, np.arange(m, dtype=np.uint64) + np.uint64(item0))
    A = Phi.T @ Phi + LD(eps) * np.eye(64, dtype=LD)
    R = _chol_ld(A)
    T = V.astype(LD).T @ f.astype(LD)
    tt = _solve_lower(R, F.astype(LD).T @ T)
    sd = np.asarray(a, dtype=np.float64) * np.sqrt(np.float64(eps))                  # fp64, one product
    noise = (sd[None, :] * np.asarray(z, dtype=np.float64)).astype(LD)               # fp64, one product
    w = tt + noise
    xi = _solve_lower(R, w, transposed=True)
    Q = (xi[live] ** 2).sum(axis=0)
    g = F.astype(LD) @ xi
    H = V.astype(LD) @ g
    return dict(V=V, F=F, live=live, r=r, A=A, R=R, T=T, t=tt, z=z, w=w, xi=xi, Q=Q, g=g, H=H,
                cond=float(np.linalg.cond(A.astype(np.float64))))


def _chol_ld(A):
    """the lower Cholesky factor in long double (NumPy's own is fp64)"""
    n = A.shape[0]
    R = np.zeros_like(A)
    for k in range(n):
        R[k, k] = np.sqrt(A[k, k] - (R[k, :k] ** 2).sum())
        R[k + 1:, k] = (A[k + 1:, k] - R[k + 1:, :k] @ R[k, :k]) / R[k, k]
    return R


def _solve_lower(R, B, transposed=False):
    """R^-1 B (or R^-T B) for lower-triangular R by substitution in long double"""
    X = np.array(B, dtype=LD, copy=True)
    n = R.shape[0]
    if not transposed:
        for k in range(n):
            X[k] = (X[k] - R[k, :k] @ X[:k]) / R[k, k]
    else:
        for k in range(n - 1, -1, -1):
            X[k] = (X[k] - R[k + 1:, k] @ X[k + 1:]) / R[k, k]
    return X


def centred_tables(amp_grid) -> tuple:
    """(ln_a, half_inv_a2): the proposal's two tables as the library forms them at the first call, long double rounded once"""
    g = np.asarray(amp_grid, dtype=np.float64).astype(LD)
    return np.log(g).astype(np.float64), (LD(0.5) / (g * g)).astype(np.float64)


def centred_exact_update(H, Q, f, mu, y, k, seed, t, amp_grid, log_prior, r, item0=0) -> dict:
    """Step 4 (and the draw of step 2) for all items given the device's H (n x m) and Q (m), as gpirt_sampler_draw_amp_centred
    states it.  lq, the draw and dll are long double with a bound on what the device's fp64 may differ by; c = grid[k'] / grid[k]
    and f' = h + c (f - h) are fp64, three roundings, formed as the device forms them: bit for bit.
    Returns dict(status (m of "accepted", "rejected", "same", "failed"), k (afterwards), k_prop (-1 where no draw could be made),
    f (fp64, the accepted columns rewritten), amplitude, u0, u1, c, lq (P x m), e_lq (its bound), draw_decided (m: the cut
    u0 C_last clears C_k' and C_k'-1 by their bounds), dll, e_dll, log_u (long double), decided (m: the draw is decided and
    |log u1 - dll| > e_dll + 2 u |log u1|, or the status does not hang on a margin)).

    THE BOUNDS, u = 2^-53.  lq[k] = (lp - r ln a) - Q h2 is two products, two differences: e_lq = 4 u (|lp| + r |ln a| + Q h2).
    p = exp(lq - max) carries e_lq of both, the difference's rounding and the exponential's two ulp: relative e_p = e_lq[k] +
    e_lq[kmax] + 6 u.  C_k adds at most 5 of a thread's points, 8 scan levels and the base: e_C[k] = sum_{i <= k} p_i e_p_i +
    14 u C_k.  The cut u0 C_last carries e_C[last] u0 + u u0 C_last.  dll is gpirt_sampler_draw_amp's sum: per observed cell
    2 u (|a0| + |a1|) + 5 u (t0 + t1), the additions (n / 256 + 9) u sum |t0 - t1|."""
    g = np.asarray(amp_grid, dtype=np.float64)
    lp = np.asarray(log_prior, dtype=np.float64)
    P = g.shape[0]
    f, mu, y, H = (np.asarray(x, dtype=np.float64) for x in (f, mu, y, H))
    Q = np.asarray(Q, dtype=np.float64)
    n, m = f.shape
    k = np.asarray(k, dtype=np.int64).reshape(m)
    ln_a, h2 = centred_tables(g)
    u0, u1 = centred_uniforms(seed, t, np.arange(m, dtype=np.uint64) + np.uint64(item0))
    out_f, out_k = f.copy(order="F"), k.copy()
    k_prop = np.full(m, -1, dtype=np.int64)
    status = []
    nan = LD(np.nan)
    c = np.full(m, np.nan)
    lq_all, e_lq_all = np.full((P, m), nan, dtype=LD), np.full((P, m), np.nan)
    dll, log_u = np.full(m, nan, dtype=LD), np.full(m, nan, dtype=LD)
    e_dll = np.full(m, np.nan)
    draw_decided, decided = np.zeros(m, dtype=bool), np.zeros(m, dtype=bool)
    for j in range(m):
        if not np.isfinite(Q[j]):
            status.append("failed")
            draw_decided[j] = decided[j] = True
            continue
        lq = (LD(1) * lp - LD(r) * ln_a.astype(LD)) - LD(Q[j]) * h2.astype(LD)
        e_lq = 4 * U * (np.abs(lp) + r * np.abs(ln_a) + Q[j] * h2)
        lq_all[:, j], e_lq_all[:, j] = lq, e_lq
        kmax = int(np.argmax(lq))
        p = np.exp(lq - lq[kmax])
        e_p = (e_lq + e_lq[kmax] + 6 * U).astype(LD)
        Cs = np.cumsum(p)
        e_C = np.cumsum(p * e_p) + 14 * U * Cs
        cut = LD(u0[j]) * Cs[-1]
        e_cut = LD(u0[j]) * e_C[-1] + U * cut
        kp = int(np.argmax(Cs > cut))
        k_prop[j] = kp
        draw_decided[j] = bool(Cs[kp] - cut > e_C[kp] + e_cut) and (kp == 0 or bool(cut - Cs[kp - 1] > e_C[kp - 1] + e_cut))
        if kp == k[j]:
            status.append("same")
            decided[j] = draw_decided[j]
            continue
        with np.errstate(all="ignore"):
            c[j] = g[kp] / g[k[j]]                                   # one fp64 division
            fp = H[:, j] + c[j] * (f[:, j] - H[:, j])                # fp64: a difference, a product, a sum
            bad = int((~np.isfinite(fp)).sum() + (~np.isfinite(H[:, j])).sum())
            obs = ~np.isnan(y[:, j])
            ys = np.where(obs, y[:, j], 0.0).astype(LD)
            a0, a1 = ys * (f[:, j].astype(LD) + mu[:, j].astype(LD)), ys * (fp.astype(LD) + mu[:, j].astype(LD))
            t0, t1 = ll_term(a0), ll_term(a1)
            dll[j] = np.where(obs, t0 - t1, LD(0)).sum()
            cells = np.where(obs, 2 * U * (np.abs(a0) + np.abs(a1)) + 5 * U * (t0 + t1), LD(0)).sum()
            e_dll[j] = float(cells + (n / 256 + 9) * U * np.where(obs, np.abs(t0 - t1), LD(0)).sum())
        log_u[j] = np.log(LD(u1[j]))
        if bad or not np.isfinite(dll[j]):
            status.append("failed")
            decided[j] = draw_decided[j]
            continue
        decided[j] = draw_decided[j] and abs(float(log_u[j] - dll[j])) > e_dll[j] + 2 * U * abs(float(log_u[j]))
        if log_u[j] < dll[j]:
            status.append("accepted")
            out_k[j] = kp
            out_f[:, j] = fp
        else:
            status.append("rejected")
    return dict(status=status, k=out_k, k_prop=k_prop, f=out_f, amplitude=g[out_k], u0=u0, u1=u1, c=c, lq=lq_all, e_lq=e_lq_all,
                draw_decided=draw_decided, dll=dll, e_dll=e_dll, log_u=log_u, decided=decided)


# ------------------------------------------------------------------------------------------------------- summaries ---
def retune(width, accept_rate, points) -> np.ndarray:
    """The burn-in's rule per item: halve the width below an acceptance of 0.2, double it above 0.5, within 1 .. points - 1.
    width and accept_rate: m values each (a NaN rate leaves the width)."""
    w = np.asarray(width, dtype=np.int64).copy()
    r = np.asarray(accept_rate, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        low, high = r < ADAPT_LOW, r > ADAPT_HIGH
    w = np.where(low, np.maximum(1, w // 2), w)
    w = np.where(high, np.minimum(int(points) - 1, 2 * w), w)
    return w.astype(np.int32)


def summarise(draws, hist, amp_grid, probs=(0.025, 0.25, 0.5, 0.75, 0.975)) -> dict:
    """Exact summaries per item from the histogram hist (P x m counts): mean and sd of a_j, quantiles (grid values: the smallest
    a_k whose cumulative count reaches p times the draws), mode, p_below (P x m: p_below[t, j] = the posterior mass at or below
    grid point t).  From the recorded indices `draws` (chains x S x m, or S x m): rhat and ess of log a_j
    (gpirt_amd.chains.diagnostics_from_draws)."""
    from . import chains as CH
    g = np.asarray(amp_grid, dtype=np.float64)
    hist = np.asarray(hist, dtype=np.int64)
    P, m = hist.shape
    total = hist.sum(axis=0)
    w = hist.astype(LD) / total.astype(LD)[None, :]
    mean = (w * g.astype(LD)[:, None]).sum(axis=0)
    var = (w * (g.astype(LD)[:, None] - mean[None, :]) ** 2).sum(axis=0)
    cum = np.cumsum(hist, axis=0)
    qs = {}
    for p in probs:
        need = np.ceil(float(p) * total)
        qs[float(p)] = g[np.array([int(np.searchsorted(cum[:, j], need[j], side="left")) for j in range(m)]).clip(0, P - 1)]
    idx = np.asarray(draws, dtype=np.int64)
    if idx.ndim == 2:
        idx = idx[None]
    with np.errstate(all="ignore"):
        d = CH.diagnostics_from_draws(np.log(g)[idx])
    return dict(hist=hist, mean=mean.astype(np.float64), sd=np.sqrt(var).astype(np.float64), quantiles=qs,
                mode=g[np.argmax(hist, axis=0)], p_below=(cum.astype(LD) / total.astype(LD)[None, :]).astype(np.float64),
                rhat=np.asarray(d["rhat"], dtype=np.float64), ess=np.asarray(d["ess"], dtype=np.float64))


# ------------------------------------------------------------------------------------------------ one call per run ---
def run(y, sample_iterations, burn_iterations, chains=1, seed=1, lo=0.1, hi=10.0, points=129, width=4, every=1, adapt=True,
        kernel=None, fixed=None, top=20, log_prior=None, k0=None, loo=False, preset="fast", store_draws=True, theta_init=None, *,
        handle=None, consistent=False, update="whitened", **sampler_kw) -> dict:
    """gpirt_amd.kernel.run's stage loop with per-item amplitudes: `chains` chains of the stage-driven Sampler under `kernel`, one
    after the other, each with Sampler.draw_amp() after every `every`-th step() and Sampler.amp_record() per kept draw.  y: n x m
    of +1 / -1 / NaN.  Every item starts at index k0 (None: the grid point nearest 1).  adapt=True: during the burn-in, and nowhere
    else, each item's width is retuned every 50 updates towards an acceptance between 0.2 and 0.5 (`retune`).

    fixed: m amplitudes (or one for all) -- the chains run with Sampler.amp_set(fixed) and no update; res["amp"] then holds
    mode="fixed" and the amplitudes alone.

    Returns what kernel.run returns -- theta, beta, f, IRFs, summary, diagnostics, loo, kernel, kstar_rank, chains -- plus amp:
    mode ("sampled"), draws (the recorded indices, chains x S x m; S x m for one chain) and amplitude (grid[draws]); hist
    (P x m, pooled over the chains), mean, sd, quantiles, mode_amplitude, p_below, rhat and ess of log a_j (`summarise`);
    accept_rate and width per chain and item (of the sampling phase), counts per chain (4 x m), grid, log_prior, every;
    smallest and largest: the `top` items with the smallest and with the largest posterior mean amplitude (item, mean, sd).

    consistent=True: every iteration is Sampler.step(consistent=True) -- f is carried to the new theta with the model's nugget,
    whose sd carries a_j (gpirt_amd.consistent); the result's "consistent" names it.

    update: "whitened" (the default: Sampler.draw_amp() alone, the result as it always was), "centred" (Sampler.draw_amp_centred()
    alone) or "both" (draw_amp() then draw_amp_centred() after every `every`-th step).  The centred move reads the prior density
    of f: run it with consistent=True.  res["amp"]["update"] names the mode; with the centred move res["amp"] also carries
    counts_centred per chain (4 x m: updates, accepted, same, failed), accept_rate_centred (of the sampling phase's decided
    updates, per chain and item) and rank.  Width retuning stays the whitened move's alone."""
    from . import chains as CH
    from . import kernel as K
    from . import loo as LO
    from .ops import Handle
    from .sampler import Sampler, _keep, _options
    y = np.asfortranarray(np.asarray(y, dtype=np.float64))
    n, m = y.shape
    S, B, nc, every = int(sample_iterations), int(burn_iterations), int(chains), int(every)
    if update not in ("whitened", "centred", "both"):
        raise ValueError(f"amp.run: update = {update!r}, it is \"whitened\", \"centred\" or \"both\"")
    whiten, centre = update in ("whitened", "both"), update in ("centred", "both")
    if nc < 1 or S < 1 or B < 0 or every < 1:
        raise ValueError("amp.run: chains >= 1, sample_iterations >= 1, burn_iterations >= 0 and every >= 1 are needed")
    sampled = fixed is None
    if sampled:
        g = grid(lo, hi, points)
        kk = None if k0 is None else np.ascontiguousarray(np.broadcast_to(np.asarray(k0, dtype=np.int32), (m,)))
        check_args(lo, hi, points, log_prior, width, kk, m)
    else:
        fixed = np.ascontiguousarray(np.broadcast_to(np.asarray(fixed, dtype=np.float64), (m,)))
    want_loo = None
    if loo is not None and loo is not False:
        want_loo = LO.parse(loo)
        LO.tail_length(nc * S, want_loo["tail"])
    keep = _keep(store_draws)
    inits = CH.default_inits(n, nc, seed) if theta_init is None else np.asarray(theta_init, dtype=np.float64).reshape(nc, -1)
    if inits.shape != (nc, n):
        raise ValueError("theta_init must have one value per respondent (and chain)")
    own = handle is None
    h = Handle() if own else handle
    samplers = []
    try:
        if kernel is not None or own:
            h.set_kernel(kernel)
        used = h.kernel()
        if preset == "fast":
            rank = K.fast_rank(used)
            if K.is_default(used):
                opts = dict(preset="fast")
            else:                                          # the preset's fields (gpirt_fast_options) with the rank the kernel allows
                opts = dict(rng="item", theta_stabilise=True, fstar_fused=True, kstar_rank=rank)
        elif preset is None:
            opts = {}
            rank = int(sampler_kw.get("kstar_rank", 0))
        else:
            raise ValueError(f"unknown preset {preset!r}")
        opts.update(sampler_kw)
        # the refusals that need no device, before anything is created: they name their reason (gpirt_amp_check)
        o = _options(opts.get("rng", "item"), seed, True, True, None, opts.get("item0", 0), opts.get("m_total", 0),
                     opts.get("kernel_fp32", False), 0)
        check_args(0.1, 10.0, 2, None, 1, None, m, options=o)
        th = np.empty((nc, S + 1, n)) if "theta" in keep else None
        be = np.empty((nc, 2, m, S + 1)) if "beta" in keep else None
        ff = np.empty((nc, n, m, S + 1)) if "f" in keep else None
        draws = np.empty((nc, S, m), dtype=np.int32)
        hist = np.zeros((int(points), m), dtype=np.int64)
        rates, widths, counts = [], [], []
        rates_c, counts_c, rank_c = [], [], 0

        def store(c, slot, s):
            if th is not None:
                th[c, slot] = s.get("theta")
            if be is not None:
                be[c, :, :, slot] = s.get("beta")
            if ff is not None:
                ff[c, :, :, slot] = s.get("f")

        irf_one = None
        for c in range(nc):
            s = Sampler(h, y, inits[c], seed=seed if c == 0 else _lib.chain_seed(seed, c), **opts)
            samplers.append(s)
            s.init()
            s.check()
            if sampled:
                s.amp_enable(lo, hi, points, log_prior, width, k0, planned_draws=S)
            else:
                s.amp_set(fixed)
            store(c, 0, s)
            s.summary_enable(_lib.SUM_THETA_BETA | _lib.SUM_DIAG, planned_draws=S)
            if want_loo is not None:
                s.loo_enable(nc * S, want_loo["tail"])
            w = np.full(m, int(width), dtype=np.int32)
            seen = np.zeros((4, m), dtype=np.int64)
            start = np.zeros((4, m), dtype=np.int64)
            start_c = np.zeros((4, m), dtype=np.int64)
            done = 0
            for it in range(S + B):
                s.step(consistent=consistent)
                if sampled and (it + 1) % every == 0:
                    if whiten:
                        s.draw_amp()
                    if centre:
                        s.draw_amp_centred()
                    done += 1
                    if whiten and adapt and it < B and done % ADAPT_EVERY == 0:
                        cn = s.amp_get("counts")
                        with np.errstate(all="ignore"):
                            w = retune(w, (cn[1] - seen[1]) / (cn[0] - seen[0]), points)
                        s.amp_width(w)
                        seen = cn
                if sampled and it == B - 1:
                    start = s.amp_get("counts")
                    if centre and done:
                        start_c = s.amp_get("counts_centred")
                if it >= B:
                    s.accumulate_irf()
                    store(c, it - B + 1, s)
                    if sampled:
                        s.amp_record()
                    s.summary_accumulate()
                    if want_loo is not None:
                        s.loo_accumulate()
            s.check()
            if sampled:
                cn = s.amp_get("counts")
                with np.errstate(all="ignore"):
                    rates.append((cn[1] - start[1]) / (cn[0] - start[0]))
                widths.append(s.amp_get("width"))
                counts.append(cn)
                draws[c] = s.amp_get("draws")
                hist += s.amp_get("hist")
                if centre:
                    cc = s.amp_get("counts_centred") if done else np.zeros((4, m), dtype=np.int64)
                    with np.errstate(all="ignore"):
                        dcd = (cc[0] - cc[2] - cc[3]) - (start_c[0] - start_c[2] - start_c[3])
                        rates_c.append((cc[1] - start_c[1]) / dcd)
                    counts_c.append(cc)
                    rank_c = s.amp_centred()["rank"]
            if nc == 1:
                irf_one = s.finish_irfs(S)
        pooled = CH.combine(h, samplers)
        if sampled:
            amp = summarise(draws, hist, g)
            amp["mode_amplitude"] = amp.pop("mode")
            order = np.argsort(amp["mean"], kind="stable")
            row = lambda j: dict(item=int(j), mean=float(amp["mean"][j]), sd=float(amp["sd"][j]))        # noqa: E731
            tp = max(0, min(int(top), m))
            amp.update(mode="sampled", draws=draws if nc > 1 else draws[0], amplitude=g[draws] if nc > 1 else g[draws[0]],
                       accept_rate=np.array(rates), width=np.array(widths), counts=np.array(counts), grid=g,
                       log_prior=samplers[0].amp_get("log_prior"), every=every, update=update,
                       smallest=[row(j) for j in order[:tp]], largest=[row(j) for j in order[::-1][:tp]])
            if centre:
                amp.update(counts_centred=np.array(counts_c), accept_rate_centred=np.array(rates_c), rank=rank_c)
        else:
            amp = dict(mode="fixed", amplitude=fixed.copy())
        out = dict(consistent=bool(consistent), theta=th, beta=be, f=ff, IRFs=irf_one if nc == 1 else pooled["IRFs"], summary=pooled["summary"],
                   diagnostics=pooled["diagnostics"], kernel=used, kstar_rank=rank, chains=nc, amp=amp,
                   loo=LO.combine(h, samplers, top=want_loo["top"]) if want_loo is not None else None)
        if nc == 1:
            for k_ in ("theta", "beta", "f"):
                if out[k_] is not None:
                    out[k_] = np.asfortranarray(out[k_][0])
        return out
    finally:
        for s in samplers:
            s.close()
        if own:
            h.close()
