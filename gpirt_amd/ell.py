"""The kernel's length scale as a parameter of the chain (include/gpirt_hip.h, "the kernel's length scale as a parameter of the
chain": gpirt_ell_grid, gpirt_ell_check, gpirt_sampler_ell_*, gpirt_sampler_draw_ell; csrc/ell.hip, csrc/sampler.hip).

One length scale ell, shared by all items, lives on a fixed logarithmic grid ell_k = lo (hi / lo)^(k / (P - 1)); the chain's
state is the index k, so every count, histogram and quantile of ell is exact.  The prior is a table of P finite log masses on
the grid, i.e. a density with respect to log ell; the default -(ln ell_k)^2 / 2 (log-normal, median 1, log-sd 1) is a choice,
not a measurement.  The update is the prior-whitened Metropolis step of Murray & Adams (2010, "Slice sampling covariance
hyperparameters of latent Gaussian models", section 2.2): nu = L(ell)^-1 f is held fixed, not f.

`run` is the one-call way in: gpirt_amd.kernel.run's stage loop with Sampler.draw_ell() after every `every`-th step().
`step_exact` is the NumPy statement of one update (Cholesky in fp64 on gpirt_amd.kernel.kernel_matrix, everything after it in
long double), `conditional_posterior` the exact discrete p(k | nu, theta, mu, y) by direct summation.

Beside it stands the centred update of the same paper (section 2.1; gpirt_sampler_draw_ell_centred, Sampler.draw_ell("centred")):
f is held fixed and the GP prior decides, p(k | f, theta) proportional to prod_j N(f_j; 0, S_k) exp(log_prior[k]).  It has its
own width, call count, uniforms (item index 1 of GPIRT_ST_ELL) and counters.  `step_exact_centred` is its NumPy statement,
`conditional_posterior_centred` its stationary distribution, and run(update="centred" | "both") drives it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import ST_ELL, check

LD = np.longdouble
JITTER = 0.001
ADAPT_EVERY, ADAPT_LOW, ADAPT_HIGH = 50, 0.2, 0.5


# ---------------------------------------------------------------------------------------------------- the contract ---
def grid(lo=0.25, hi=4.0, points=129) -> np.ndarray:
    """ell_k = lo (hi / lo)^(k / (points - 1)), k = 0 .. points - 1, as the library keeps it (gpirt_ell_grid: long double on the
    host, rounded to fp64, the end points exact).  2 <= points <= 1025 and 0.01 <= lo < hi <= 1000, else GpirtError."""
    P = int(points)
    out = np.empty(max(P, 1))
    check(_lib.load().gpirt_ell_grid(float(lo), float(hi), P, out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def default_log_prior(ell_grid) -> np.ndarray:
    """-(ln ell_k)^2 / 2: a log-normal mass with median 1 and log-sd 1 on the grid (long double, rounded to fp64)."""
    l = np.log(np.asarray(ell_grid, dtype=np.float64).astype(LD))
    return (-(l * l) / LD(2)).astype(np.float64)


def check_args(lo, hi, points, log_prior=None, width=4, k0=None, kernel=None, options=None, m=0) -> None:
    """gpirt_ell_check (no device is touched): every refusal of Sampler.ell_enable as a GpirtError that names its reason.
    kernel: a gpirt_amd.kernel argument (the handle's kernel) or None; options: a gpirt_options (_lib.Options) or None."""
    from . import kernel as K
    lp = None if log_prior is None else np.ascontiguousarray(log_prior, dtype=np.float64)
    if lp is not None and lp.shape != (int(points),):
        raise ValueError(f"ell: log_prior must hold points = {int(points)} values")
    check(_lib.load().gpirt_ell_check(float(lo), float(hi), int(points),
                                      None if lp is None else lp.ctypes.data_as(C.POINTER(C.c_double)), int(width),
                                      -1 if k0 is None else int(k0), None if kernel is None else C.byref(K.struct(kernel)),
                                      None if options is None else C.byref(options), int(m)))


def uniforms(seed, t, kind="whitened") -> tuple:
    """(u0, u1) of the t-th draw_ell call of that kind on a sampler (t counted from 1, per kind): item_uniform(seed, t,
    GPIRT_ST_ELL, item, 0 / 1) with item 0 for "whitened" and 1 for "centred"."""
    from .ppc import item_uniform
    u = item_uniform(seed, int(t), ST_ELL, _lib.ELL_KINDS.index(kind), np.arange(2, dtype=np.uint64))
    return float(u[0]), float(u[1])


def proposal(u0, w) -> int:
    """The offset d of the proposed index k' = k + d: j = min(floor(u0 2w), 2w - 1), d = j - w for j < w, else j - w + 1 --
    uniform on -w .. w without 0, symmetric."""
    w = int(w)
    j = min(int(np.floor(float(u0) * (2 * w))), 2 * w - 1)
    return j - w if j < w else j - w + 1


# ------------------------------------------------------------------------------------------------------- NumPy -------
def ll_term(a):
    """t(a) = log(1 + exp(-a)) in long double: max(-a, 0) + log1p(exp(-|a|))"""
    a = np.asarray(a, dtype=LD)
    return np.maximum(-a, LD(0)) + np.log1p(np.exp(-np.abs(a)))


def factor(theta, family, length_scale) -> np.ndarray:
    """chol(K(theta, theta; length_scale) + 0.001 I), lower, in fp64 (numpy.linalg.cholesky), as long double"""
    from . import kernel as K
    th = np.asarray(theta, dtype=np.float64)
    S = K.kernel_matrix(th, th, family, float(length_scale))
    S[np.diag_indices_from(S)] += JITTER
    return np.linalg.cholesky(S).astype(LD)


def solve_lower(L, b) -> np.ndarray:
    """L^-1 b by forward substitution in long double (L lower, n x n; b n x m)"""
    L = np.asarray(L, dtype=LD)
    x = np.array(b, dtype=LD, copy=True)
    for i in range(L.shape[0]):
        if i:
            x[i] -= L[i, :i] @ x[:i]
        x[i] /= L[i, i]
    return x


def _factor_of(cache, theta, family, ell_grid, k):
    if cache is None:
        return factor(theta, family, ell_grid[k])
    if k not in cache:
        cache[k] = factor(theta, family, ell_grid[k])
    return cache[k]


def step_exact(theta, f, mu, y, k, u0, u1, ell_grid, log_prior, width, family="se", cache=None) -> dict:
    """One update as gpirt_sampler_draw_ell states it.  theta (n), f, mu, y (n x m; y of +1 / -1 / NaN), the index k, the two
    uniforms, the tables and the family; cache: a dict that keeps the factors per index between calls with the same theta.
    Returns dict(status ("accepted", "rejected", "out_of_range", "failed"), k (the index afterwards), k_prop, f (fp64: f', rounded,
    when accepted, else f as given), and for an update that got that far nu, f_prop (long double), delta (m), dll, log_ratio,
    log_u)."""
    ell_grid = np.asarray(ell_grid, dtype=np.float64)
    lp = np.asarray(log_prior, dtype=np.float64)
    P = ell_grid.shape[0]
    f = np.asarray(f, dtype=np.float64)
    kp = int(k) + proposal(u0, width)
    out = dict(status="out_of_range", k=int(k), k_prop=kp, f=f)
    if kp < 0 or kp >= P:
        return out
    mu = np.asarray(mu, dtype=np.float64).astype(LD)
    y = np.asarray(y, dtype=np.float64)
    out["status"] = "failed"
    try:
        nu = solve_lower(_factor_of(cache, theta, family, ell_grid, int(k)), f)
        Lp = _factor_of(cache, theta, family, ell_grid, kp)
    except np.linalg.LinAlgError:
        return out
    fp = Lp @ nu
    obs = ~np.isnan(y)
    ys = np.where(obs, y, 0.0).astype(LD)
    with np.errstate(all="ignore"):
        terms = np.where(obs, ll_term(ys * (f.astype(LD) + mu)) - ll_term(ys * (fp + mu)), LD(0))
    delta = terms.sum(axis=0)
    dll = delta.sum()
    log_ratio = dll + (LD(lp[kp]) - LD(lp[int(k)]))
    log_u = np.log(LD(u1))
    out.update(nu=nu, f_prop=fp, delta=delta, dll=dll, log_ratio=log_ratio, log_u=log_u)
    if not (np.isfinite(fp).all() and np.isfinite(dll)):
        return out
    if log_u < log_ratio:
        out.update(status="accepted", k=kp, f=fp.astype(np.float64))
    else:
        out["status"] = "rejected"
    return out


def conditional_posterior(nu, theta, mu, y, ell_grid, log_prior, family="se") -> np.ndarray:
    """p(k | nu, theta, mu, y) on the grid by direct summation: proportional to exp(log_prior[k] - sum over observed cells of
    t(y (L_k nu + mu))), in long double (the stationary distribution of the update with nu held fixed)."""
    ell_grid = np.asarray(ell_grid, dtype=np.float64)
    nu = np.asarray(nu, dtype=LD)
    mu = np.asarray(mu, dtype=np.float64).astype(LD)
    y = np.asarray(y, dtype=np.float64)
    obs = ~np.isnan(y)
    ys = np.where(obs, y, 0.0).astype(LD)
    lw = np.empty(ell_grid.shape[0], dtype=LD)
    for k in range(ell_grid.shape[0]):
        fk = factor(theta, family, ell_grid[k]) @ nu
        lw[k] = LD(log_prior[k]) - np.where(obs, ll_term(ys * (fk + mu)), LD(0)).sum()
    w = np.exp(lw - lw.max())
    return (w / w.sum()).astype(np.float64)


def step_exact_centred(theta, f, k, u0, u1, ell_grid, log_prior, width, family="se", cache=None) -> dict:
    """One update as gpirt_sampler_draw_ell_centred states it: f (n x m) is held fixed and
    log_ratio = sum_j [log N(f_j; 0, S_k') - log N(f_j; 0, S_k)] + log_prior[k'] - log_prior[k]
              = -0.5 sum_j dq_j - m dld + log_prior[k'] - log_prior[k],
    dq_j = sum_i (nu'_ij - nu_ij)(nu'_ij + nu_ij) with nu = L_k^-1 f and nu' = L_k'^-1 f, dld = sum_i (log L'_ii - log L_ii).
    Cholesky in fp64, everything after it in long double; cache as step_exact's.  Returns dict(status ("accepted", "rejected",
    "out_of_range", "failed"), k (the index afterwards), k_prop, and for an update that got that far nu, nu_prop (long double),
    dq (m), dld, log_ratio, log_u)."""
    ell_grid = np.asarray(ell_grid, dtype=np.float64)
    lp = np.asarray(log_prior, dtype=np.float64)
    f = np.asarray(f, dtype=np.float64)
    kp = int(k) + proposal(u0, width)
    out = dict(status="out_of_range", k=int(k), k_prop=kp)
    if kp < 0 or kp >= ell_grid.shape[0]:
        return out
    out["status"] = "failed"
    try:
        L = _factor_of(cache, theta, family, ell_grid, int(k))
        Lp = _factor_of(cache, theta, family, ell_grid, kp)
    except np.linalg.LinAlgError:
        return out
    nu, nup = solve_lower(L, f), solve_lower(Lp, f)
    dq = ((nup - nu) * (nup + nu)).sum(axis=0)
    dld = (np.log(np.diagonal(Lp)) - np.log(np.diagonal(L))).sum()
    log_ratio = LD(-0.5) * dq.sum() - LD(f.shape[1]) * dld + (LD(lp[kp]) - LD(lp[int(k)]))
    log_u = np.log(LD(u1))
    out.update(nu=nu, nu_prop=nup, dq=dq, dld=dld, log_ratio=log_ratio, log_u=log_u)
    if not (np.isfinite(nup).all() and np.isfinite(dq).all() and np.isfinite(dld)):
        return out
    if log_u < log_ratio:
        out.update(status="accepted", k=kp)
    else:
        out["status"] = "rejected"
    return out


def conditional_posterior_centred(f, theta, ell_grid, log_prior, family="se") -> np.ndarray:
    """p(k | f, theta) on the grid by direct summation: proportional to exp(log_prior[k] - 0.5 sum_j |L_k^-1 f_j|^2 -
    m sum_i log (L_k)_ii), in long double (the stationary distribution of the centred update with f held fixed)."""
    ell_grid = np.asarray(ell_grid, dtype=np.float64)
    f = np.asarray(f, dtype=np.float64)
    lw = np.empty(ell_grid.shape[0], dtype=LD)
    for k in range(ell_grid.shape[0]):
        L = factor(theta, family, ell_grid[k])
        nu = solve_lower(L, f)
        lw[k] = LD(log_prior[k]) - (nu * nu).sum() / LD(2) - LD(f.shape[1]) * np.log(np.diagonal(L)).sum()
    w = np.exp(lw - lw.max())
    return (w / w.sum()).astype(np.float64)


# ------------------------------------------------------------------------------------------------------- summaries ---
def retune(width, accept_rate, points) -> int:
    """The burn-in's rule: halve the width below an acceptance of 0.2, double it above 0.5, within 1 .. points - 1."""
    w = int(width)
    if accept_rate < ADAPT_LOW:
        w = max(1, w // 2)
    elif accept_rate > ADAPT_HIGH:
        w = min(int(points) - 1, 2 * w)
    return w


def summarise(index, ell_grid, probs=(0.025, 0.25, 0.5, 0.75, 0.975)) -> dict:
    """Exact summaries of kept indices (chains x S, or S): hist (P counts), mean and sd of ell, quantiles (grid values: the
    smallest ell_k whose cumulative count reaches p times the draws), mode, and rhat / ess of log ell
    (gpirt_amd.chains.diagnostics_from_draws)."""
    from . import chains as CH
    ell_grid = np.asarray(ell_grid, dtype=np.float64)
    idx = np.atleast_2d(np.asarray(index, dtype=np.int64))
    hist = np.bincount(idx.ravel(), minlength=ell_grid.shape[0]).astype(np.int64)
    total = int(hist.sum())
    w = hist.astype(LD) / LD(total)
    mean = float((w * ell_grid.astype(LD)).sum())
    var = float((w * (ell_grid.astype(LD) - LD(mean)) ** 2).sum())
    cum = np.cumsum(hist)
    qs = {float(p): float(ell_grid[int(np.searchsorted(cum, np.ceil(p * total), side="left"))]) for p in probs}
    d = CH.diagnostics_from_draws(np.log(ell_grid)[idx])
    return dict(hist=hist, mean=mean, sd=float(np.sqrt(var)), quantiles=qs, mode=float(ell_grid[int(np.argmax(hist))]),
                rhat=float(d["rhat"]), ess=float(d["ess"]))


# ------------------------------------------------------------------------------------------------ one call per run ---
def run(y, sample_iterations, burn_iterations, chains=1, seed=1, family="se", lo=0.25, hi=4.0, points=129, width=4,
        log_prior=None, every=1, adapt=True, loo=False, preset="fast", store_draws=True, theta_init=None, k0=None, *,
        handle=None, update="whitened", width_centred=None, consistent=False, **sampler_kw) -> dict:
    """gpirt_amd.kernel.run's stage loop with the length scale in the chain: `chains` chains of the stage-driven Sampler, one
    after the other, each with Sampler.draw_ell() after every `every`-th step().  y: n x m of +1 / -1 / NaN.

    The handle's kernel is (family, the grid point nearest 1 in log ell -- or ell_k0 with k0 given); every chain starts there.
    preset="fast": the item RNG, theta_stabilise, fstar_fused and kstar_rank = gpirt_amd.kernel.fast_rank at lo (the rank
    whose certificate holds on the whole grid); preset=None: sampler_kw as given.  adapt=True: during the burn-in, and nowhere
    else, the width is retuned on the host every 50 updates towards an acceptance between 0.2 and 0.5 (`retune`); the sampling
    phase runs a fixed kernel.  Returns what kernel.run returns -- theta, beta, f, IRFs, summary, diagnostics, loo, kernel (the
    handle's), kstar_rank, chains -- plus ell: index and length_scale per kept draw (chains x S; S for one chain), hist, mean, sd,
    exact quantiles, mode, rhat and ess of log ell (`summarise`), accept_rate and width per chain (of the sampling phase),
    counts per chain, grid and log_prior.

    update: which update follows every `every`-th step() -- "whitened" (the default: exactly what this function returned before
    the keyword existed), "centred" (Sampler.draw_ell("centred"), width `width_centred`, None: `width`), or "both": the whitened
    update and then the centred one, in that fixed order.  The burn-in retunes each kind's width from that kind's own
    acceptance.  ell["update"] names the mode; with "centred" or "both", ell's accept_rate, width and counts are dicts with one
    entry per kind that ran ("whitened", "centred"), each what the default mode holds for its one kind.

    consistent=True: every iteration is Sampler.step(consistent=True) -- f is carried to the new theta with the model's nugget
    (gpirt_amd.consistent), the state the centred update's prior density assumes; the result's "consistent" names it."""
    from . import chains as CH
    from . import kernel as K
    from . import loo as LO
    from .ops import Handle
    from .sampler import Sampler, _keep, _options
    y = np.asfortranarray(np.asarray(y, dtype=np.float64))
    n, m = y.shape
    S, B, nc, every = int(sample_iterations), int(burn_iterations), int(chains), int(every)
    if nc < 1 or S < 1 or B < 0 or every < 1:
        raise ValueError("ell.run: chains >= 1, sample_iterations >= 1, burn_iterations >= 0 and every >= 1 are needed")
    kinds = {"whitened": ("whitened",), "centred": ("centred",), "both": _lib.ELL_KINDS}.get(update)
    if kinds is None:
        raise ValueError(f"ell.run: update must be 'whitened', 'centred' or 'both', not {update!r}")
    width0 = {"whitened": int(width), "centred": int(width if width_centred is None else width_centred)}
    g = grid(lo, hi, points)
    if k0 is None:
        k0 = int(np.argmin(np.abs(np.log(g))))
    check_args(lo, hi, points, log_prior, width, k0)
    check_args(lo, hi, points, log_prior, width0["centred"], k0)
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
        h.set_kernel(dict(family=family, length_scale=float(g[k0])))
        used = h.kernel()
        if preset == "fast":
            rank = K.fast_rank(dict(family=family, length_scale=float(g[0])))
            opts = dict(rng="item", theta_stabilise=True, fstar_fused=True, kstar_rank=rank)
        elif preset is None:
            opts = {}
            rank = int(sampler_kw.get("kstar_rank", 0))
        else:
            raise ValueError(f"unknown preset {preset!r}")
        opts.update(sampler_kw)
        # the refusals that need no device, before anything is created: they name their reason (gpirt_ell_check)
        o = _options(opts.get("rng", "item"), seed, True, opts.get("fstar_fused", False), None, opts.get("item0", 0),
                     opts.get("m_total", 0), opts.get("kernel_fp32", False), opts.get("kstar_rank", 0))
        check_args(lo, hi, points, log_prior, width, k0, kernel=used, options=o, m=m)
        th = np.empty((nc, S + 1, n)) if "theta" in keep else None
        be = np.empty((nc, 2, m, S + 1)) if "beta" in keep else None
        ff = np.empty((nc, n, m, S + 1)) if "f" in keep else None
        index = np.empty((nc, S), dtype=np.int64)
        rates, widths, counts = ({kd: [] for kd in kinds} for _ in range(3))

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
            s.ell_enable(lo, hi, points, log_prior, width, k0)
            store(c, 0, s)
            s.summary_enable(_lib.SUM_THETA_BETA | _lib.SUM_DIAG, planned_draws=S)
            if want_loo is not None:
                s.loo_enable(nc * S, want_loo["tail"])
            if "centred" in kinds:
                s.ell_width(width0["centred"], "centred")
            of = lambda e, kd: e if kd == "whitened" else e["centred"]                   # noqa: E731
            w, seen, start = dict(width0), {kd: (0, 0) for kd in kinds}, {kd: (0, 0) for kd in kinds}
            for it in range(S + B):
                s.step(consistent=consistent)
                if (it + 1) % every == 0:
                    for kd in kinds:
                        s.draw_ell(kd)
                        if adapt and it < B:
                            e = of(s.ell(), kd)
                            if e["updates"] - seen[kd][0] >= ADAPT_EVERY:
                                w[kd] = retune(w[kd], (e["accepted"] - seen[kd][1]) / (e["updates"] - seen[kd][0]), points)
                                s.ell_width(w[kd], kd)
                                seen[kd] = (e["updates"], e["accepted"])
                if it == B - 1:
                    for kd in kinds:
                        e = of(s.ell(), kd)
                        start[kd] = (e["updates"], e["accepted"])
                if it >= B:
                    s.accumulate_irf()
                    store(c, it - B + 1, s)
                    index[c, it - B] = s.ell()["index"]
                    s.summary_accumulate()
                    if want_loo is not None:
                        s.loo_accumulate()
            s.check()
            for kd in kinds:
                e = of(s.ell(), kd)
                done = e["updates"] - start[kd][0]
                rates[kd].append((e["accepted"] - start[kd][1]) / done if done else float("nan"))
                widths[kd].append(e["width"])
                counts[kd].append({k: e[k] for k in _lib.ELL_COUNTS})
            if nc == 1:
                irf_one = s.finish_irfs(S)
        pooled = CH.combine(h, samplers)
        ell = summarise(index, g)
        if update == "whitened":
            rates, widths, counts = rates["whitened"], widths["whitened"], counts["whitened"]
        ell.update(update=update, index=index if nc > 1 else index[0], length_scale=g[index] if nc > 1 else g[index[0]], accept_rate=rates,
                   width=widths, counts=counts, grid=g, log_prior=samplers[0].ell_get("log_prior"), every=every)
        out = dict(consistent=bool(consistent), theta=th, beta=be, f=ff, IRFs=irf_one if nc == 1 else pooled["IRFs"], summary=pooled["summary"],
                   diagnostics=pooled["diagnostics"], kernel=used, kstar_rank=rank, chains=nc, ell=ell,
                   loo=LO.combine(h, samplers, top=want_loo["top"]) if want_loo is not None else None)
        if nc == 1:
            for k in ("theta", "beta", "f"):
                if out[k] is not None:
                    out[k] = np.asfortranarray(out[k][0])
        return out
    finally:
        for s in samplers:
            s.close()
        if own:
            h.close()
