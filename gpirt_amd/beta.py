"""The centred update of the mean function's coefficients (library version 136; include/gpirt_hip.h "a centred beta update",
csrc/beta_centred.hip, Sampler.draw_beta_centred).

draw_beta is the reference's random-walk Metropolis step per coefficient of mu_j = beta_0j + beta_1j theta with f_j held fixed.
The likelihood reads only g_j = f_j + mu_j, so that step changes g_j and only tiny steps are accepted.  The centred move changes
beta_j and f_j together with g_j held fixed: the likelihood does not change, there is no accept step, and with X = [1, theta],
S = K(theta, theta) + eps I and f_j = g_j - X beta_j ~ N(0, a_j^2 S) the conditional of beta_j is Gaussian,

    beta_j | g_j, theta, a_j ~ N(Lam_j^-1 b_j, Lam_j^-1),   Lam_j = B / a_j^2 + diag(1 / s0^2),   B = X^T S^-1 X,
    b_j = (W^T f_j + B beta_j) / a_j^2 + m0 / s0^2,   W = S^-1 X,   f_j' = f_j + (mu_j - mu_j').

`centred_normals`, `centred_shared` and `centred_exact_update` are the NumPy statement of one call in long double,
`conditional` the same conditional by the dense formula with the true kernel, and `run` one call per run: the stage loop with
the move after every step, against the chain without it.
"""
from __future__ import annotations

import numpy as np

from . import _lib

LD = np.longdouble
U = 2.0 ** -53
JITTER = 1.0e-3
GRID = -5.0 + 0.01 * np.arange(1001)          # theta* as the library forms it: -5 + i 0.01 in fp64


def centred_normals(seed, t, items, handle=None) -> np.ndarray:
    """z (2 x len(items)): z[k, j] = qnorm(item_uniform(seed, t, GPIRT_ST_BETA_CENTRED, items[j], k)), the two normals of item j in
    the t-th draw_beta_centred call (t counted from 1).  As gpirt_amd.amp.centred_normals: the uniforms are integer arithmetic and
    the same bits everywhere; AS 241 takes a logarithm in its tails, where the device library's differs from the host's in the
    last place, so with `handle` (a Handle) the normals come from gpirt_item_normals and are the device's bits; without one they
    are evaluated here, equal in the central branch |u - 0.5| <= 0.425 and within 4e-15 relative in the tails."""
    from .amp import _qnorm
    from .ppc import item_uniform
    it = np.atleast_1d(np.asarray(items, dtype=np.uint64))
    if handle is not None:
        from .ops import to_host
        if it.size and np.any(np.diff(it.astype(np.int64)) != 1):
            raise ValueError("centred_normals: with a handle the items must be consecutive")
        return np.asfortranarray(to_host(handle.item_normals(int(seed), int(t), _lib.ST_BETA_CENTRED, int(it[0]), int(it.size), 2)))
    u = item_uniform(seed, int(t), _lib.ST_BETA_CENTRED, it[None, :], np.arange(2, dtype=np.uint64)[:, None])
    return np.asfortranarray(_qnorm(u))


def centred_shared(theta, kernel=None, F=None, eps=JITTER) -> dict:
    """The shared part of one call from theta alone, in long double on the rank-64 identity: Phi = V F (V the fp64 basis at theta,
    F of gpirt_amd.amp.centred_factor or the 64 x 64 `F` given, e.g. the device's), A = Phi^T Phi + eps I = R R^T,
    W = (X - Phi A^-1 Phi^T X) / eps = (Phi Phi^T + eps I)^-1 X and B = X^T W.  Returns dict(V (fp64), F (fp64), Phi, R, P = V^T X,
    Gx = F A^-1 Phi^T X, W (n x 2), B (2 x 2, symmetrised), cond = cond_2(A)); long double but V and F."""
    from . import amp as A_, fstar_free as FF
    th = np.asarray(theta, dtype=np.float64)
    V = FF.basis(th)
    Phi, live, r = A_.centred_basis(th, kernel, F)
    if F is None:
        F = A_.centred_factor(kernel)[0]
    F = np.asarray(F, dtype=np.float64)
    X = np.stack([np.ones_like(th), th], axis=1).astype(LD)
    A = Phi.T @ Phi + LD(eps) * np.eye(64, dtype=LD)
    R = A_._chol_ld(A)
    P = V.astype(LD).T @ X
    u = A_._solve_lower(R, F.astype(LD).T @ P)
    xi = A_._solve_lower(R, u, transposed=True)                     # A^-1 Phi^T X
    Gx = F.astype(LD) @ xi
    W = (X - V.astype(LD) @ Gx) / LD(eps)
    B = X.T @ W
    B = (B + B.T) / LD(2)
    return dict(V=V, F=F, Phi=Phi, R=R, P=P, Gx=Gx, W=W, B=B, live=live, rank=r, cond=float(np.linalg.cond(A.astype(np.float64))))


def centred_exact_update(W, B, f, beta, a, prior_means, prior_sds, theta, tstar, z, beta_new=None) -> dict:
    """Steps 2 and 3 of one call for all items given W (n x 2) and B (2 x 2) -- the device's, or centred_shared's -- as
    gpirt_sampler_draw_beta_centred states them.  f (n x m fp64), beta (2 x m), a (m amplitudes, or None: all 1), the prior's
    means and sds (2 x m), theta (n), tstar (the grid; None: GRID), z (2 x m normals).  T, Lam, chol, mean and beta' are long
    double; the rewrite is fp64 formed as the device forms it (mu = beta'_0 + theta beta'_1, f' = f + ((beta_0 + theta beta_1) - mu),
    mu_star = beta'_0 + theta* beta'_1) from beta' rounded to fp64 -- or from `beta_new` (2 x m fp64, e.g. the device's),
    with which f', mu' and mu_star' are the device's bit for bit.
    Returns dict(T (2 x m), Lam (m x 2 x 2), chol (3 x m: c00, c10, c11), mean (2 x m), beta (2 x m, beta'), cov (m x 2 x 2, the
    conditional covariance Lam^-1), f, mu, mu_star (fp64, the updated items rewritten; mu and mu_star of a failed item are
    NaN columns: the statement does not know them), status (m of "updated" / "failed"))."""
    W, f = np.asarray(W, dtype=np.float64), np.asarray(f, dtype=np.float64)
    n, m = f.shape
    B = np.asarray(B, dtype=LD).reshape(2, 2)
    beta = np.asarray(beta, dtype=np.float64).reshape(2, m)
    a = np.ones(m) if a is None else np.broadcast_to(np.asarray(a, dtype=np.float64), (m,))
    pm = np.asarray(prior_means, dtype=np.float64).reshape(2, m)
    ps = np.asarray(prior_sds, dtype=np.float64).reshape(2, m)
    th = np.asarray(theta, dtype=np.float64)
    ts = GRID if tstar is None else np.asarray(tstar, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64).reshape(2, m)
    with np.errstate(all="ignore"):
        T = W.astype(LD).T @ f.astype(LD)
    Lam, cov = np.empty((m, 2, 2), dtype=LD), np.empty((m, 2, 2), dtype=LD)
    chol, mean, new = np.empty((3, m), dtype=LD), np.empty((2, m), dtype=LD), np.empty((2, m), dtype=LD)
    out_f = f.copy(order="F")
    mu, mu_star = np.full((n, m), np.nan, order="F"), np.full((ts.size, m), np.nan, order="F")
    status = []
    for j in range(m):
        with np.errstate(all="ignore"):
            ia = LD(1) / (LD(a[j]) * LD(a[j]))
            p = LD(1) / (ps[:, j].astype(LD) ** 2)
            L = B * ia + np.diag(p)
            b = (T[:, j] + B @ beta[:, j].astype(LD)) * ia + pm[:, j].astype(LD) * p
            c00 = np.sqrt(L[0, 0])
            c10 = L[1, 0] / c00
            piv = L[1, 1] - c10 * c10
            c11 = np.sqrt(piv)
            y0 = b[0] / c00
            y1 = (b[1] - c10 * y0) / c11
            m1 = y1 / c11
            m0 = (y0 - c10 * m1) / c00
            x1 = LD(z[1, j]) / c11
            x0 = (LD(z[0, j]) - c10 * x1) / c00
            Lam[j], chol[:, j], mean[:, j], new[:, j] = L, (c00, c10, c11), (m0, m1), (m0 + x0, m1 + x1)
            cov[j] = np.array([[L[1, 1], -L[0, 1]], [-L[1, 0], L[0, 0]]], dtype=LD) / (L[0, 0] * L[1, 1] - L[0, 1] * L[1, 0])
            ok = bool(np.isfinite(T[:, j]).all() and np.isfinite(L).all() and L[0, 0] > 0 and piv > 0 and np.isfinite(chol[:, j]).all()
                      and np.isfinite(mean[:, j]).all() and np.isfinite(new[:, j]).all())
        status.append("updated" if ok else "failed")
        if not ok:
            continue
        bn = new[:, j].astype(np.float64) if beta_new is None else np.asarray(beta_new, dtype=np.float64).reshape(2, m)[:, j]
        mu[:, j] = bn[0] + th * bn[1]
        out_f[:, j] = f[:, j] + ((beta[0, j] + th * beta[1, j]) - mu[:, j])
        mu_star[:, j] = bn[0] + ts * bn[1]
    return dict(T=T, Lam=Lam, chol=chol, mean=mean, beta=new, cov=cov, f=out_f, mu=mu, mu_star=mu_star, status=status)


def conditional(theta, g, a, prior_means, prior_sds, kernel=None, eps=JITTER) -> tuple:
    """(mean (2 x m), cov (m x 2 x 2)) of beta_j | g_j, theta, a_j by the dense formula in long double with the true kernel:
    S = K(theta, theta) + eps I factored whole, Lam_j = X^T S^-1 X / a_j^2 + diag(1 / s0^2), b_j = X^T S^-1 g_j / a_j^2 + m0 / s0^2.
    For the tests: no rank-64 identity is used.  Squared-exponential kernels only."""
    g = np.asarray(g, dtype=LD)
    n, m = g.shape
    a = np.ones(m) if a is None else np.broadcast_to(np.asarray(a, dtype=np.float64), (m,))
    pm = np.asarray(prior_means, dtype=np.float64).reshape(2, m).astype(LD)
    ps = np.asarray(prior_sds, dtype=np.float64).reshape(2, m).astype(LD)
    B, SX, _ = dense_B(theta, kernel, eps)
    Xg = SX.T @ g                                                      # X^T S^-1 g
    mean, cov = np.empty((2, m), dtype=LD), np.empty((m, 2, 2), dtype=LD)
    for j in range(m):
        ia = LD(1) / (LD(a[j]) * LD(a[j]))
        L = B * ia + np.diag(LD(1) / ps[:, j] ** 2)
        b = Xg[:, j] * ia + pm[:, j] / ps[:, j] ** 2
        cov[j] = np.array([[L[1, 1], -L[0, 1]], [-L[1, 0], L[0, 0]]], dtype=LD) / (L[0, 0] * L[1, 1] - L[0, 1] * L[1, 0])
        mean[:, j] = cov[j] @ b
    return mean, cov


def dense_B(theta, kernel=None, eps=JITTER) -> tuple:
    """(B = X^T S^-1 X (2 x 2), S^-1 X (n x 2), the lower Cholesky factor of S) in long double with the true squared-exponential
    kernel S = exp(-(theta_i - theta_k)^2 / (2 ell^2)) + eps I: the dense statement B of centred_shared is held against."""
    from . import amp as A_, kernel as K
    fam, ell = K.spec(kernel)
    if K.family_name(fam) != "se":
        raise ValueError("dense_B: squared-exponential kernels only")
    th = np.asarray(theta, dtype=np.float64).astype(LD)
    d = (th[:, None] - th[None, :]) / LD(ell)
    S = np.exp(LD(-0.5) * d * d) + LD(eps) * np.eye(th.size, dtype=LD)
    L = A_._chol_ld(S)
    X = np.stack([np.ones_like(th), th], axis=1)
    SX = A_._solve_lower(L, A_._solve_lower(L, X), transposed=True)
    B = X.T @ SX
    return (B + B.T) / LD(2), SX, L


def geyer_ess(x) -> float:
    """ESS of one series by Geyer's initial positive sequence: N / (-1 + 2 sum of the pair sums Gamma_k = rho_2k + rho_2k+1 while
    they stay positive), autocorrelations by direct sums; a constant series has ESS 0."""
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


def summarise(beta_draws) -> dict:
    """rhat (2 x m: split-R-hat, gpirt_amd.chains.diagnostics_from_draws, the code amp.run uses for log a_j), ess (2 x m: Geyer's
    ESS per chain, summed over the chains) and ess_batch (2 x m, that function's batch-means ESS) of the coefficients from their
    draws (chains x S x 2 x m)."""
    from . import chains as CH
    x = np.asarray(beta_draws, dtype=np.float64)
    with np.errstate(all="ignore"):
        d = CH.diagnostics_from_draws(x)
    nc, _, _, m = x.shape
    ess = np.array([[sum(geyer_ess(x[c, :, k, j]) for c in range(nc)) for j in range(m)] for k in range(2)])
    return dict(rhat=np.asarray(d["rhat"], dtype=np.float64), ess=ess, ess_batch=np.asarray(d["ess"], dtype=np.float64))


# ------------------------------------------------------------------------------------------------ one call per run ---
def run(y, sample_iterations, burn_iterations, chains=1, seed=1, consistent=True, update="both", kernel=None, preset="fast",
        store_draws=True, theta_init=None, fixed_amp=None, *, handle=None, **sampler_kw) -> dict:
    """`chains` chains of the stage-driven Sampler, one after the other: step(consistent=consistent) and, for update="both",
    Sampler.draw_beta_centred() after every step.  update="mh" is the chain without the move, draw for draw what a plain loop of
    step(consistent=...) gives.  y: n x m of +1 / -1 / NaN.  fixed_amp: m amplitudes (or one for all) set with Sampler.amp_set
    before the first step.  The move reads the prior density of f: run it with consistent=True.

    Returns dict(theta, beta_draws, f (the stored draws as amp.run's theta, beta and f: chains x ..., the chain axis dropped for
    one chain; None where store_draws leaves them out), IRFs, summary, diagnostics, kernel, kstar_rank, chains, consistent) and
    under "beta" a dict(update, rhat, ess (2 x m each: split-R-hat and Geyer's ESS of the sampling phase's draws of each
    coefficient, `summarise`), ess_batch, calls, updates, failed (per chain), rank, seconds (wall time of the chains' loops))."""
    import time
    from . import chains as CH
    from . import kernel as K
    from .ops import Handle
    from .sampler import Sampler, _keep
    if update not in ("both", "mh"):
        raise ValueError(f"beta.run: update = {update!r}, it is \"both\" or \"mh\"")
    y = np.asfortranarray(np.asarray(y, dtype=np.float64))
    n, m = y.shape
    S, B, nc = int(sample_iterations), int(burn_iterations), int(chains)
    if nc < 1 or S < 1 or B < 0:
        raise ValueError("beta.run: chains >= 1, sample_iterations >= 1 and burn_iterations >= 0 are needed")
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
            opts = dict(preset="fast") if K.is_default(used) else dict(rng="item", theta_stabilise=True, fstar_fused=True, kstar_rank=rank)
        elif preset is None:
            opts = {}
            rank = int(sampler_kw.get("kstar_rank", 0))
        else:
            raise ValueError(f"unknown preset {preset!r}")
        opts.update(sampler_kw)
        th = np.empty((nc, S + 1, n)) if "theta" in keep else None
        be = np.empty((nc, 2, m, S + 1)) if "beta" in keep else None
        ff = np.empty((nc, n, m, S + 1)) if "f" in keep else None
        series = np.empty((nc, S, 2, m))
        stats, seconds = [], 0.0
        irf_one = None
        for c in range(nc):
            s = Sampler(h, y, inits[c], seed=seed if c == 0 else _lib.chain_seed(seed, c), **opts)
            samplers.append(s)
            s.init()
            s.check()
            if fixed_amp is not None:
                s.amp_set(np.ascontiguousarray(np.broadcast_to(np.asarray(fixed_amp, dtype=np.float64), (m,))))
            s.summary_enable(_lib.SUM_THETA_BETA | _lib.SUM_DIAG, planned_draws=S)

            def store(slot):
                if th is not None:
                    th[c, slot] = s.get("theta")
                if be is not None:
                    be[c, :, :, slot] = s.get("beta")
                if ff is not None:
                    ff[c, :, :, slot] = s.get("f")

            store(0)
            t0 = time.perf_counter()
            for it in range(S + B):
                s.step(consistent=consistent)
                if update == "both":
                    s.draw_beta_centred()
                if it >= B:
                    s.accumulate_irf()
                    store(it - B + 1)
                    series[c, it - B] = s.get("beta")
                    s.summary_accumulate()
            s.check()
            seconds += time.perf_counter() - t0
            stats.append(s.beta_centred())
            if nc == 1:
                irf_one = s.finish_irfs(S)
        pooled = CH.combine(h, samplers)
        bd = summarise(series)
        bd.update(update=update, calls=[st["calls"] for st in stats], updates=[st["updates"] for st in stats],
                  failed=[st["failed"] for st in stats], rank=stats[-1]["rank"], seconds=seconds)
        out = dict(consistent=bool(consistent), theta=th, f=ff, IRFs=irf_one if nc == 1 else pooled["IRFs"], summary=pooled["summary"],
                   diagnostics=pooled["diagnostics"], kernel=used, kstar_rank=rank, chains=nc, beta=bd, beta_draws=be)
        if nc == 1:
            for k_ in ("theta", "beta_draws", "f"):
                if out[k_] is not None:
                    out[k_] = np.asfortranarray(out[k_][0])
        return out
    finally:
        for s in samplers:
            s.close()
        if own:
            h.close()
