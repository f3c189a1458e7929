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
        handle=None, consistent=False, **sampler_kw) -> dict:
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
    whose sd carries a_j (gpirt_amd.consistent); the result's "consistent" names it."""
    from . import chains as CH
    from . import kernel as K
    from . import loo as LO
    from .ops import Handle
    from .sampler import Sampler, _keep, _options
    y = np.asfortranarray(np.asarray(y, dtype=np.float64))
    n, m = y.shape
    S, B, nc, every = int(sample_iterations), int(burn_iterations), int(chains), int(every)
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
            done = 0
            for it in range(S + B):
                s.step(consistent=consistent)
                if sampled and (it + 1) % every == 0:
                    s.draw_amp()
                    done += 1
                    if adapt and it < B and done % ADAPT_EVERY == 0:
                        cn = s.amp_get("counts")
                        with np.errstate(all="ignore"):
                            w = retune(w, (cn[1] - seen[1]) / (cn[0] - seen[0]), points)
                        s.amp_width(w)
                        seen = cn
                if sampled and it == B - 1:
                    start = s.amp_get("counts")
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
                       log_prior=samplers[0].amp_get("log_prior"), every=every,
                       smallest=[row(j) for j in order[:tp]], largest=[row(j) for j in order[::-1][:tp]])
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
