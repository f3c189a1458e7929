"""The collapsed scale and shift move (library version 137; include/gpirt_hip.h "a collapsed scale and shift move",
csrc/scale.hip, Sampler.draw_scale).

theta_finish draws theta given the curves on the grid and every update of beta is given theta, so theta's scale and location
move only as fast as n respondents and m coefficients random-walk together: each chain sits at its own.  Between
theta_partial and theta_finish the sampler holds logpost (N x n), from which theta is summed out in closed form: respondent i's
log normaliser lz_i is one pass over a column.  The move proposes one joint change of every item's linear mean on the grid --
"scale": b1_j' = b1_j exp(-eps), "shift": b0_j' = b0_j + b1_j delta -- with the GP part hstar = fstar - mu_star held fixed,
and decides it on sum_i (lz'_i - lz_i) plus beta's prior and, for the scale, the Jacobian -m eps.  The theta_finish that follows
redraws every theta under whichever curve stands.

`normals`, `proposal`, `log_normalisers` and `step_exact` are the NumPy statement of one call, `collapsed_density` the target
the accumulated eps (or delta) has for a fixed hstar, and `run` one call per run: beta.run's loop with the move inside every
consistent step, against the chain without it.
"""
from __future__ import annotations

import numpy as np

from . import _lib

LD = np.longdouble
U = 2.0 ** -53
NGRID = _lib.NGRID
GRID = -5.0 + np.arange(NGRID, dtype=np.float64) * 0.01          # x_k as the library forms it: -5.0 + (double)k * 0.01
LN_SQRT_2PI = 0.918938533204672741780329736406
KINDS = _lib.SCALE_KINDS


def _kind(kind) -> int:
    if kind in KINDS:
        return KINDS.index(kind)
    if kind in (0, 1):
        return int(kind)
    raise ValueError(f"scale: kind = {kind!r}, it is \"scale\" or \"shift\"")


def ldn(x, mean, sd):
    """R's dnorm(x, mean, sd, log=TRUE) as the library forms it, in the precision of its arguments: -(ln sqrt(2 pi) + 0.5 z^2 +
    log(sd)), z = |(x - mean) / sd|."""
    z = np.abs((x - mean) / sd)
    half = LD(0.5) if np.result_type(z) == LD else 0.5
    c = LD(LN_SQRT_2PI) if np.result_type(z) == LD else LN_SQRT_2PI
    return -(c + half * z * z + np.log(sd))


def default_lprior() -> np.ndarray:
    """The N(0, 1) row on the grid, the fp64 bits the kernels form (log(1.0) = 0 exactly)."""
    z = np.abs((GRID - 0.0) / 1.0)
    return -(LN_SQRT_2PI + 0.5 * z * z + 0.0)


def normals(seed, t, kind, handle=None) -> tuple:
    """(z, u) of the t-th call of the kind (t counted from 1): z = qnorm(item_uniform(seed, t, GPIRT_ST_SCALE, kind, 0)), u =
    item_uniform(seed, t, GPIRT_ST_SCALE, kind, 1).  The uniforms are integer arithmetic, the same bits everywhere.  AS 241
    takes a logarithm in its tails, where the device's differs from the host's in the last place: with `handle` (a Handle) z is
    gpirt_item_normals' and so the device's bits; without one it is evaluated here, equal in the central branch
    |u - 0.5| <= 0.425 and within 4e-15 relative in the tails."""
    from .amp import _qnorm
    from .ppc import item_uniform
    k = _kind(kind)
    u = item_uniform(seed, int(t), _lib.ST_SCALE, np.uint64(k), np.arange(2, dtype=np.uint64))
    if handle is not None:
        from .ops import to_host
        z = float(np.asarray(to_host(handle.item_normals(int(seed), int(t), _lib.ST_SCALE, k, 1, 1))).ravel()[0])
    else:
        z = float(_qnorm(u[:1])[0])
    return z, float(u[1])


def proposal(beta, kind, width, z, c=None) -> dict:
    """The proposal in fp64 as the device forms it.  beta (2 x m), width, z.  step = width * z; scale: c = exp(-step) -- or the
    `c` given, e.g. the device's record's, whose exp may differ from NumPy's in the last place -- b1' = b1 * c; shift: b0' = b0 +
    b1 * step.  Returns dict(step, c, beta (2 x m, beta'), mu (N x m: b0' + x_k * b1', draw_beta's bits), jacobian (the
    log Jacobian: -m * step for the scale, 0 for the shift))."""
    k = _kind(kind)
    b = np.asarray(beta, dtype=np.float64).reshape(2, -1)
    m = b.shape[1]
    step = float(np.float64(width) * np.float64(z))
    new = b.copy(order="F")
    if k == 0:
        c = float(np.exp(-step)) if c is None else float(c)
        new[1] = b[1] * c
        jac = -(float(m) * step)
    else:
        c = 1.0
        new[0] = b[0] + b[1] * step
        jac = 0.0
    mu = np.asfortranarray(new[0][None, :] + GRID[:, None] * new[1][None, :])
    return dict(step=step, c=c, beta=new, mu=mu, jacobian=jac)


def curve(fstar, mu_star, mu_prop) -> np.ndarray:
    """fstar2 = fstar + (mu2 - mu_star) in fp64: the difference of the two rounded means."""
    return np.asfortranarray(np.asarray(fstar, dtype=np.float64) + (np.asarray(mu_prop, dtype=np.float64) - np.asarray(mu_star, dtype=np.float64)))


def loglik_grid(y, fstar) -> np.ndarray:
    """logpost (N x n) in long double: logpost[k, i] = -sum over i's observed items of log(1 + exp(-y_ij fstar[k, j]))."""
    y = np.asarray(y, dtype=np.float64)
    fs = np.asarray(fstar, dtype=LD)
    out = np.zeros((fs.shape[0], y.shape[0]), dtype=LD)
    for j in range(y.shape[1]):
        for sign in (1.0, -1.0):
            who = y[:, j] == sign
            if who.any():
                a = LD(sign) * fs[:, j]
                out[:, who] -= (np.maximum(-a, 0) + np.log1p(np.exp(-np.abs(a))))[:, None]
    return out


def _lprior_rows(lprior, n):
    lp = default_lprior() if lprior is None else np.asarray(lprior)
    return np.broadcast_to(lp, (n, lp.shape[-1])) if lp.ndim == 1 else lp


def log_normalisers(logpost, lprior=None, order="exact") -> np.ndarray:
    """lz (n): lz_i = M_i + log sum_{k=1}^{N-1} exp(P_i[k] - M_i), P_i[k] = lprior_i[k] + logpost[k, i], M_i = max_{k>=1} P_i[k]:
    the log normaliser of the law theta_finish draws from (index 0 is never drawn).  logpost: N x n.  lprior: None (N(0, 1)), one
    row (N) or one row per respondent (n x N; with a population prior, table[codes]).
    order="device": fp64 in the kernel's layout and order -- P in fp64, thread t's four terms k = 4 t .. 4 t + 3 added ascending
    from 0, the 256 totals by the adjacent-pair tree -- with NumPy's exp and log in place of the device's; order="exact": long
    double, sorted sums."""
    lp = np.asarray(logpost)
    N, n = lp.shape
    pr = _lprior_rows(lprior, n)
    if order == "device":
        P = pr.astype(np.float64).T + lp.astype(np.float64)            # N x n
        with np.errstate(all="ignore"):
            M = np.max(np.where(np.isnan(P[1:]), -np.inf, P[1:]), axis=0)
            e = np.zeros((1024, n))
            e[1:N] = np.exp(P[1:] - M[None, :])
            e = e.reshape(256, 4, n)
            s = ((e[:, 0] + e[:, 1]) + e[:, 2]) + e[:, 3]              # (0 + e0 = e0 exactly)
            while s.shape[0] > 1:
                s = s[0::2] + s[1::2]
            return M + np.log(s[0])
    if order != "exact":
        raise ValueError(f"log_normalisers: order = {order!r}, it is \"device\" or \"exact\"")
    P = pr.astype(LD).T + lp.astype(LD)
    with np.errstate(all="ignore"):
        M = np.max(np.where(np.isnan(P[1:]), -np.inf, P[1:]), axis=0)
        e = np.sort(np.exp(P[1:] - M[None, :]), axis=0)
        return M + np.log(e.sum(axis=0))


def step_exact(logpost, logpost_prop, beta, beta_prop, prior_means, prior_sds, kind, step, u, lprior=None) -> dict:
    """The decision of one call given logpost and the proposal's logpost_prop (N x n each; the device's, or loglik_grid's), in long
    double: lz, lz_prop, dlz (n), D = sum_i dlz_i, Q = the prior's sum over the moved coefficient (the slopes for the scale, the
    intercepts for the shift), J = m * step (scale) or 0, log_r = (D + Q) - J, log_u, and status: "failed" when any of lz, lz',
    beta' or log r is not finite or a column's maximum is not > -1e300, else "accepted" iff log(u) < log r, else "rejected"."""
    k = _kind(kind)
    b = np.asarray(beta, dtype=np.float64).reshape(2, -1)
    bp = np.asarray(beta_prop, dtype=np.float64).reshape(2, -1)
    m = b.shape[1]
    pm = np.asarray(prior_means, dtype=np.float64).reshape(2, m).astype(LD)
    ps = np.asarray(prior_sds, dtype=np.float64).reshape(2, m).astype(LD)
    lz = log_normalisers(logpost, lprior)
    lzp = log_normalisers(logpost_prop, lprior)
    with np.errstate(all="ignore"):
        dlz = lzp - lz
        D = dlz.sum()
        q = 1 if k == 0 else 0                                         # row 1 (slopes) for the scale, row 0 for the shift
        Q = (ldn(bp[q].astype(LD), pm[q], ps[q]) - ldn(b[q].astype(LD), pm[q], ps[q])).sum()
        J = LD(m) * LD(step) if k == 0 else LD(0)
        log_r = (D + Q) - J
        log_u = np.log(LD(u))
    n = lz.size
    pr = _lprior_rows(lprior, n)
    degenerate = False
    with np.errstate(all="ignore"):
        for x in (logpost, logpost_prop):
            P = pr.astype(np.float64).T[1:] + np.asarray(x, dtype=np.float64)[1:]
            degenerate = degenerate or not (np.max(np.where(np.isnan(P), -np.inf, P), axis=0) > -1e300).all()
    failed = bool(degenerate or not np.isfinite(lz.astype(np.float64)).all() or not np.isfinite(lzp.astype(np.float64)).all()
                  or not np.isfinite(bp).all() or not np.isfinite(np.float64(log_r)))
    status = "failed" if failed else ("accepted" if log_u < log_r else "rejected")
    return dict(lz=lz, lz_prop=lzp, dlz=dlz, D=D, Q=Q, J=J, log_r=log_r, log_u=log_u, status=status)


def collapsed_density(x, kind, hstar, beta, y, prior_means, prior_sds, lprior=None) -> float:
    """The unnormalised log density of the ACCUMULATED step x (the sum of the accepted eps, or delta) for a fixed hstar (N x m),
    starting coefficients beta (2 x m) and answers y (n x m), in long double: with beta(x) the coefficients x away from the start
    (b1 exp(-x), or b0 + b1 x),  sum_i lz_i(hstar + mu(beta(x))) + sum_j ldn(the moved coefficient) - m x  (the last term for the
    scale alone).  What a chain of the move's calls on a fixed hstar must sample: the 1-d quadrature of this is the test's
    reference."""
    k = _kind(kind)
    b = np.asarray(beta, dtype=np.float64).reshape(2, -1).astype(LD)
    m = b.shape[1]
    pm = np.asarray(prior_means, dtype=np.float64).reshape(2, m).astype(LD)
    ps = np.asarray(prior_sds, dtype=np.float64).reshape(2, m).astype(LD)
    x = LD(x)
    if k == 0:
        b0, b1 = b[0], b[1] * np.exp(-x)
        prior = ldn(b1, pm[1], ps[1]).sum() - LD(m) * x
    else:
        b0, b1 = b[0] + b[1] * x, b[1]
        prior = ldn(b0, pm[0], ps[0]).sum()
    fs = np.asarray(hstar, dtype=LD) + (b0[None, :] + GRID.astype(LD)[:, None] * b1[None, :])
    return float(log_normalisers(loglik_grid(y, fs), lprior).sum() + prior)


def retune(width, accept_rate) -> float:
    """The burn-in's rule (ell.retune's, on a continuous width): halve the width below an acceptance of 0.2, double it above
    0.5."""
    w = float(width)
    if accept_rate < 0.2:
        return w / 2.0
    if accept_rate > 0.5:
        return w * 2.0
    return w


def _series_diag(x) -> dict:
    """split-R-hat and Geyer's ESS (summed over the chains) of series x (chains x S x ...)."""
    from . import chains as CH
    from .beta import geyer_ess
    x = np.asarray(x, dtype=np.float64)
    nc, S = x.shape[:2]
    flat = x.reshape(nc, S, -1)
    with np.errstate(all="ignore"):
        d = CH.diagnostics_from_draws(flat)
    ess = np.array([sum(geyer_ess(flat[c, :, q]) for c in range(nc)) for q in range(flat.shape[2])])
    return dict(rhat=np.asarray(d["rhat"], dtype=np.float64).reshape(x.shape[2:]), ess=ess.reshape(x.shape[2:]))


# ------------------------------------------------------------------------------------------------ one call per run ---
def run(y, sample_iterations, burn_iterations, chains=1, seed=1, update="both", consistent=True, adapt=True, w_scale=None,
        w_shift=None, kernel=None, preset="fast", theta_init=None, *, handle=None, **sampler_kw) -> dict:
    """`chains` chains of the stage-driven Sampler, one after the other: beta.run's loop -- step(consistent=consistent) and
    Sampler.draw_beta_centred() after every step -- with the kinds `update` names ("both": the scale and then the shift, "scale",
    "shift", or "none") proposed between theta_partial and theta_finish of every step.  update="none" is beta.run(update="both")
    draw for draw.  adapt=True: during the burn-in, and nowhere else, each kind's width is retuned on the host every 50 of its
    updates towards an acceptance between 0.2 and 0.5 (`retune`); the sampling phase runs at fixed widths.  The move is part of
    the consistent step: with consistent=False the stages are called one by one, which measurements need, and the chain is not
    the model's.

    Returns dict(update, consistent, chains, seconds, theta (chains x (S + 1) x n), beta_draws (chains x S x 2 x m), series
    (dict of chains x S arrays: S = mean_j log|b1_j|, mean_theta, sd_theta), diag (dict by series name, and "beta", of dict(rhat,
    ess): split-R-hat and Geyer's ESS summed over the chains), counts (per chain, per kind: calls, accepted, failed, width,
    accept_rate of the sampling phase))."""
    import time
    from . import chains as CH
    from . import kernel as K
    from .ops import Handle
    from .sampler import Sampler
    if update not in ("both", "scale", "shift", "none"):
        raise ValueError(f"scale.run: update = {update!r}, it is \"both\", \"scale\", \"shift\" or \"none\"")
    kinds = {"both": ("scale", "shift"), "scale": ("scale",), "shift": ("shift",), "none": ()}[update]
    y = np.asfortranarray(np.asarray(y, dtype=np.float64))
    n, m = y.shape
    S, B, nc = int(sample_iterations), int(burn_iterations), int(chains)
    if nc < 1 or S < 1 or B < 0:
        raise ValueError("scale.run: chains >= 1, sample_iterations >= 1 and burn_iterations >= 0 are needed")
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
        else:
            raise ValueError(f"unknown preset {preset!r}")
        opts.update(sampler_kw)
        th = np.empty((nc, S + 1, n))
        be = np.empty((nc, S, 2, m))
        counts, seconds = [], 0.0
        for c in range(nc):
            s = Sampler(h, y, inits[c], seed=seed if c == 0 else _lib.chain_seed(seed, c), **opts)
            samplers.append(s)
            s.init()
            s.check()
            if kinds:
                s.scale_enable(w_scale, w_shift)
            th[c, 0] = s.get("theta")
            seen = {kd: (0, 0) for kd in kinds}
            start = {kd: (0, 0) for kd in kinds}
            t0 = time.perf_counter()
            for it in range(S + B):
                if not kinds:
                    s.step(consistent=consistent)
                elif consistent:
                    s.step(consistent=True, scale=kinds)
                else:
                    s.draw_f(); s.draw_fstar(); s.theta_partial()
                    for kd in kinds:
                        s.draw_scale(kd)
                    s.theta_finish(); s.draw_beta(); s.factor()
                s.draw_beta_centred()
                if kinds and adapt and it < B and (it + 1) % 50 == 0:
                    st = s.scale()
                    for kd in kinds:
                        e = st[kd]
                        done = e["calls"] - seen[kd][0]
                        if done > 0:
                            s.scale_width(kd, retune(e["width"], (e["accepted"] - seen[kd][1]) / done))
                        seen[kd] = (e["calls"], e["accepted"])
                if kinds and it == B - 1:
                    st = s.scale()
                    start = {kd: (st[kd]["calls"], st[kd]["accepted"]) for kd in kinds}
                if it >= B:
                    th[c, it - B + 1] = s.get("theta")
                    be[c, it - B] = s.get("beta")
            s.check()
            seconds += time.perf_counter() - t0
            st = s.scale() if kinds else {}
            per = {}
            for kd in kinds:
                e = dict(st[kd])
                done = e["calls"] - start[kd][0]
                e["accept_rate"] = (e["accepted"] - start[kd][1]) / done if done > 0 else float("nan")
                per[kd] = e
            counts.append(per)
        series = dict(S=np.log(np.abs(be[:, :, 1, :])).mean(axis=2), mean_theta=th[:, 1:].mean(axis=2), sd_theta=th[:, 1:].std(axis=2))
        diag = {k_: _series_diag(v) for k_, v in series.items()}
        diag["beta"] = _series_diag(be)
        return dict(update=update, consistent=bool(consistent), chains=nc, seconds=seconds, theta=th, beta_draws=be, series=series,
                    diag=diag, counts=counts)
    finally:
        for s in samplers:
            s.close()
        if own:
            h.close()
