"""The covariance kernel of the GP prior: the squared exponential with a length scale and the Matern 5/2 and 3/2 forms
(include/gpirt_hip.h, "the covariance kernel": gpirt_kernel, gpirt_kernel_check, gpirt_kernel_set; csrc/se_kernel.hip).

K(a, b) = k(|a - b| / length_scale) with k(0) = 1 for every family, S = K(theta, theta) + 0.001 I:
    "se"        k(r) = exp(-r^2 / 2)                            (the reference's kernel at length_scale = 1)
    "matern52"  k(r) = (1 + a + a^2 / 3) exp(-a),  a = sqrt(5) r
    "matern32"  k(r) = (1 + a) exp(-a),            a = sqrt(3) r
0.01 <= length_scale <= 1000 (the lower limit is the spacing of the theta grid).  There is no signal variance: draw_fstar's
standard deviation is the reference's s = 1 - sqrt(q), which is only meaningful for a prior with k(0) = 1.

The kernel belongs to the Handle (Handle(kernel=...), Handle.set_kernel); gpirtMCMC creates its own handle inside the library
and runs the default kernel.  `run` is the one-call way in: the stage loop of gpirt_amd.acf.run under a kernel, with PSIS-LOO
on, and `compare` ranks several kernels by elpd_loo on one handle.  `kernel_matrix` is the NumPy statement and
`rank_certificate` wraps gpirt_kernel_check: whether draw_fstar's rank-r Chebyshev form (kstar_rank) is exact to rounding
under a kernel.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import KERNEL_FAMILIES, KERNEL_MATERN32, KERNEL_MATERN52, KERNEL_SE, check

FAST_RANK = 64                                   # gpirt_fast_options' kstar_rank
_NAMES = {v: k for k, v in KERNEL_FAMILIES.items()}


# ---------------------------------------------------------------------------------------------------- the contract ---
def family_name(code: int) -> str:
    return _NAMES[int(code)]


def spec(kernel) -> tuple:
    """(family code, length_scale) of a kernel argument: None (the default), a family name, dict(family=..., length_scale=...)
    (family a name or a code; length_scale defaults to 1) or a gpirt_kernel.  Unknown names and keys are ValueErrors; the
    range of length_scale is the library's to check."""
    if kernel is None:
        return KERNEL_SE, 1.0
    if isinstance(kernel, _lib.Kernel):
        return int(kernel.family), float(kernel.length_scale)
    if isinstance(kernel, str):
        kernel = dict(family=kernel)
    if not isinstance(kernel, dict):
        raise ValueError(f"kernel: expected None, a family name or dict(family=..., length_scale=...), got {kernel!r}")
    unknown = set(kernel) - {"family", "length_scale"}
    if unknown or "family" not in kernel:
        raise ValueError(f"kernel: a dict gives family and length_scale (unknown keys {sorted(unknown)})")
    fam = kernel["family"]
    if isinstance(fam, str):
        if fam not in KERNEL_FAMILIES:
            raise ValueError(f"kernel: unknown family {fam!r}; known: {sorted(KERNEL_FAMILIES)}")
        fam = KERNEL_FAMILIES[fam]
    elif isinstance(fam, bool) or not isinstance(fam, (int, np.integer)):
        raise ValueError(f"kernel: family = {fam!r}, it must be a name or a code")
    return int(fam), float(kernel.get("length_scale", 1.0))


def struct(kernel) -> _lib.Kernel:
    """A gpirt_kernel from a kernel argument (spec's forms)."""
    fam, ell = spec(kernel)
    k = _lib.Kernel()
    _lib.load().gpirt_kernel_default(C.byref(k))
    k.family, k.length_scale = fam, ell
    return k


def as_dict(kernel) -> dict:
    fam, ell = spec(kernel)
    return dict(family=_NAMES.get(fam, fam), length_scale=ell)


def is_default(kernel) -> bool:
    return spec(kernel) == (KERNEL_SE, 1.0)


# ------------------------------------------------------------------------------------------------------- NumPy -------
def kernel_matrix(x1, x2, family="se", length_scale=1.0) -> np.ndarray:
    """K(x1, x2) (len(x1) x len(x2)) in fp64, operation by operation as the device forms it (csrc/se_kernel.hip): the
    default kernel as exp(-0.5 d d), the others on |d| (1 / length_scale)."""
    fam, ell = spec(dict(family=family, length_scale=length_scale))
    if not (np.isfinite(ell) and _lib.LENGTH_SCALE_MIN <= ell <= _lib.LENGTH_SCALE_MAX):
        raise ValueError(f"kernel: length_scale = {ell!r}, it must be finite and lie in {_lib.LENGTH_SCALE_MIN} .. "
                         f"{_lib.LENGTH_SCALE_MAX}")
    d = np.asarray(x1, dtype=np.float64).reshape(-1, 1) - np.asarray(x2, dtype=np.float64).reshape(1, -1)
    if fam == KERNEL_SE and ell == 1.0:
        return np.exp(-0.5 * d * d)
    inv = 1.0 / ell
    if fam == KERNEL_SE:
        r = d * inv
        return np.exp(-0.5 * r * r)
    r = np.abs(d) * inv
    if fam == KERNEL_MATERN52:
        a = np.sqrt(5.0) * r
        return ((1.0 + a) + (a * a) * (1.0 / 3.0)) * np.exp(-a)
    if fam == KERNEL_MATERN32:
        a = np.sqrt(3.0) * r
        return (1.0 + a) * np.exp(-a)
    raise ValueError(f"kernel: unknown family code {fam}")


# ----------------------------------------------------------------------------------------------- the rank certificate ---
def rank_certificate(family="se", length_scale=1.0, r=FAST_RANK) -> dict:
    """gpirt_kernel_check (no device is touched): may draw_fstar's rank-r form be used under this kernel?
    Returns dict(accepted, certificate, min_rank, message): certificate = max |K(theta, c) V^T - K(theta, theta*)| over theta
    and theta* on the grid, in long double with V as the device holds it; a rank is accepted exactly when its certificate is
    no larger than that of ("se", 1, r = 48).  A refusal names the smallest allowed rank that passes (min_rank, 0: none --
    always for a Matern kernel) in its message.  A bad kernel raises GpirtError, a bad r (not 0 or a multiple of 16 in
    16..128) ValueError."""
    lib = _lib.load()
    if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not (r == 0 or (16 <= r <= 128 and r % 16 == 0)):
        raise ValueError(f"rank_certificate: r = {r!r}, it must be 0 or a multiple of 16 in 16..128")
    k = struct(dict(family=family, length_scale=length_scale))
    check(lib.gpirt_kernel_check(C.byref(k), 0, None, None))          # the kernel itself
    cert, mr = C.c_double(), C.c_int()
    rc = lib.gpirt_kernel_check(C.byref(k), int(r), C.byref(cert), C.byref(mr))
    if rc not in (0, _lib.E_ARG):
        check(rc)
    return dict(accepted=rc == 0, certificate=float(cert.value), min_rank=int(mr.value),
                message="" if rc == 0 else _lib.last_error())


def fast_rank(kernel) -> int:
    """The kstar_rank of the fast preset under a kernel: 64 where its certificate allows it, else the smallest rank that
    passes, else (always for a Matern kernel) 0, the full solve."""
    fam, ell = spec(kernel)
    if fam != KERNEL_SE:
        check(_lib.load().gpirt_kernel_check(C.byref(struct(kernel)), 0, None, None))
        return 0
    c = rank_certificate(fam, ell, FAST_RANK)
    return FAST_RANK if c["accepted"] else c["min_rank"]


# ------------------------------------------------------------------------------------------------ one call per kernel ---
def run(y, sample_iterations, burn_iterations, chains=1, seed=1, kernel=None, loo=True, preset="fast", theta_init=None,
        store_draws=True, *, handle=None, consistent=False, **sampler_kw) -> dict:
    """`chains` chains of the stage-driven Sampler under `kernel`, one after the other -- the stage loop of gpirt_amd.acf.run:
    chain c runs with the seed chain_seed(seed, c) from gpirtMCMC(chains=...)'s default init, with the DIAG summaries and
    (loo=True, or dict(tail=..., top=...)) PSIS-LOO on.  y: n x m of +1 / -1 / NaN.

    kernel: None (with a handle given: the handle's kernel as it is; else the default), a family name, or dict(family=...,
    length_scale=...).  handle: a Handle without live Samplers (its kernel is set); None creates one for the call.
    preset="fast": the item RNG, theta_stabilise, fstar_fused and kstar_rank = fast_rank(kernel); preset=None: sampler_kw as
    given (a kstar_rank the kernel's certificate refuses is the library's GpirtError).
    Returns theta ((S + 1) x n), beta (2 x m x (S + 1)), f (n x m x (S + 1)) as gpirtMCMC stores them (slot 0: the state
    after init; stacked with a leading chain axis for chains > 1; None where store_draws leaves a draw out), IRFs (1001 x m,
    pooled over the chains), summary and diagnostics (gpirt_amd.chains.combine), loo (gpirt_amd.loo's dict, or None),
    kernel (dict(family, length_scale)) and kstar_rank, the rank used.  With kernel=None and the defaults the draws are
    gpirtMCMC(y, S, B, preset="fast", seed=seed)'s.
    consistent=True: every iteration is Sampler.step(consistent=True) -- f is carried to the new theta with the model's nugget
    (gpirt_amd.consistent); the result's "consistent" names it."""
    from . import chains as CH
    from . import loo as LO
    from .ops import Handle
    from .sampler import Sampler, _keep
    y = np.asfortranarray(np.asarray(y, dtype=np.float64))
    n, m = y.shape
    S, B, nc = int(sample_iterations), int(burn_iterations), int(chains)
    if nc < 1 or S < 1 or B < 0:
        raise ValueError("kernel.run: chains >= 1, sample_iterations >= 1 and burn_iterations >= 0 are needed")
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
            rank = fast_rank(used)
            if is_default(used):
                opts = dict(preset="fast")
            else:                                          # the preset's fields (gpirt_fast_options) with the rank the kernel allows
                opts = dict(rng="item", theta_stabilise=True, fstar_fused=True, kstar_rank=rank)
        elif preset is None:
            opts = {}
            rank = int(sampler_kw.get("kstar_rank", 0))
        else:
            raise ValueError(f"unknown preset {preset!r}")
        opts.update(sampler_kw)
        th = np.empty((nc, S + 1, n)) if "theta" in keep else None
        be = np.empty((nc, 2, m, S + 1)) if "beta" in keep else None
        ff = np.empty((nc, n, m, S + 1)) if "f" in keep else None

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
            store(c, 0, s)
            s.summary_enable(_lib.SUM_THETA_BETA | _lib.SUM_DIAG, planned_draws=S)
            if want_loo is not None:
                s.loo_enable(nc * S, want_loo["tail"])
            for it in range(S + B):
                s.step(consistent=consistent)
                if it >= B:
                    s.accumulate_irf()
                    store(c, it - B + 1, s)
                    s.summary_accumulate()
                    if want_loo is not None:
                        s.loo_accumulate()
            s.check()
            if nc == 1:
                irf_one = s.finish_irfs(S)
        pooled = CH.combine(h, samplers)
        out = dict(consistent=bool(consistent), theta=th, beta=be, f=ff, IRFs=irf_one if nc == 1 else pooled["IRFs"], summary=pooled["summary"],
                   diagnostics=pooled["diagnostics"], kernel=used, kstar_rank=rank, chains=nc,
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


def max_rhat(diagnostics) -> float:
    """the largest split-R-hat over theta and beta of a diagnostics dict (NaN where neither has one)"""
    v = [diagnostics["scalars"][b]["max_rhat"] for b in ("theta", "beta")]
    v = [x for x in v if not np.isnan(x)]
    return float(max(v)) if v else float("nan")


def compare(y, kernels, sample_iterations, burn_iterations, chains=4, seed=1, *, loo=True, preset="fast", theta_init=None,
            handle=None, **sampler_kw) -> list:
    """One `run` per entry of `kernels` on ONE handle (the kernel is set, the chains run, their samplers are closed before the
    next kernel is set), every run with the same seed, inits and PSIS-LOO on, no draws stored.  Returns the rows sorted by
    elpd_loo, best first: dict(index (the entry's position in `kernels`), kernel, kstar_rank, elpd_loo, se_elpd_loo, p_loo,
    elpd_diff and se_diff against the best row (gpirt_amd.loo.compare; 0 for the best), k_bad (cells whose Pareto k is above
    the threshold: their elpd is not to be trusted), max_rhat (theta and beta) and n_obs).

    A dict entry may also carry amplitude= (a scalar or m values): that candidate runs under fixed per-item GP amplitudes
    (gpirt_amd.amp.run with fixed=amplitude, Sampler.amp_set) and its row gains `amplitude`."""
    from . import amp as AM
    from . import loo as LO
    from .ops import Handle
    if loo is None or loo is False:
        raise ValueError("kernel.compare ranks by elpd_loo: loo must be on")
    kernels = list(kernels)
    if not kernels:
        raise ValueError("kernel.compare: no kernels")
    amps = [k.get("amplitude") if isinstance(k, dict) else None for k in kernels]
    kernels = [{q: v for q, v in k.items() if q != "amplitude"} if isinstance(k, dict) else k for k in kernels]
    for k in kernels:
        spec(k)

    def one(k, a):
        kw = dict(chains=chains, seed=seed, kernel=as_dict(k), loo=loo, preset=preset, theta_init=theta_init, store_draws=False,
                  handle=h, **sampler_kw)
        if a is None:
            return run(y, sample_iterations, burn_iterations, **kw)
        return AM.run(y, sample_iterations, burn_iterations, fixed=a, **kw)
    own = handle is None
    h = Handle() if own else handle
    before = h.kernel()
    try:
        runs = [one(k, a) for k, a in zip(kernels, amps)]
    finally:
        if own:
            h.close()
        else:
            h.set_kernel(before)
    order = sorted(range(len(runs)), key=lambda i: (-runs[i]["loo"]["elpd_loo"], i))
    best = runs[order[0]]["loo"]
    rows = []
    for i in order:
        r = runs[i]
        d = LO.compare(r["loo"], best)
        rows.append(dict(index=i, kernel=r["kernel"], kstar_rank=r["kstar_rank"], elpd_loo=r["loo"]["elpd_loo"],
                         se_elpd_loo=r["loo"]["se_elpd_loo"], p_loo=r["loo"]["p_loo"], elpd_diff=d["elpd_diff"],
                         se_diff=d["se_diff"], k_bad=r["loo"]["k_bad"] + r["loo"]["k_very_bad"],
                         max_rhat=max_rhat(r["diagnostics"]), n_obs=d["n_obs"]))
        if amps[i] is not None:
            rows[-1]["amplitude"] = r["amp"]["amplitude"]
    return rows
