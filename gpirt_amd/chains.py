"""Several chains of one model and their convergence diagnostics (include/gpirt_hip.h GPIRT_SUM_DIAG, gpirt_chains_combine).

Each chain keeps its posterior summaries in ONE device block (Sampler.summary_state()): Welford moments, the WAIC and
prediction sums, the split-half and batch-means accumulators of GPIRT_SUM_DIAG and the IRF sum.  `combine` pools C such
blocks on the device -- moments by Chan's formula, WAIC by a logaddexp over chains -- and computes split-R-hat (BDA3), a
batch-means ESS and the MCSE of every theta, beta and (with "f") f value.  The ESS is the batch-means one, not the
rank-normalised ESS of Vehtari et al. (2021): rank normalisation needs every draw, and the point here is to keep none.

The reflection theta -> -theta (with the beta slope) leaves the likelihood unchanged under the default symmetric priors, so
two chains can settle in mirror modes.  Negating a chain's accumulated means is the same as negating all of its draws, so
`combine` aligns chain c >= 1 to chain 0 when sum_i thetabar_c,i thetabar_0,i < 0 (align=True), or with forced signs.

`diagnostics_from_draws` computes the same quantities in NumPy from stored draws (two-pass): the tests' reference, and a
tool for users who kept their draws.  `run_distributed` runs one chain per torch.distributed rank and combines on rank 0.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import NGRID, check

_dp = C.POINTER(C.c_double)


def _ptr(a):
    return a.ctypes.data_as(_dp)


def state_header(state) -> dict:
    """The header of a state block (a torch tensor on the device, as Sampler.summary_state() returns)."""
    h = _lib.header_words(state)
    return dict(n=int(h[0]), m=int(h[1]), parts=int(h[2]), planned=int(h[3]), draws=int(h[4]), layout=int(h[5]))


def diag_struct(parts: int, n: int, m: int, chains: int):
    """A gpirt_diag with host arrays for every output the parts allow, and those arrays (kept alive by the caller)."""
    d = _lib.Diag()
    arrays = {}
    shapes = {"theta": (n,), "beta": (2, m), "f": (n, m)}
    for b in _lib.DIAG_BLOCKS:
        if b == "f" and not parts & _lib.SUM_F:
            continue
        for k in ("rhat", "ess", "mcse"):
            a = np.empty(shapes[b], order="F")
            arrays[f"{b}_{k}"] = a
            setattr(d, f"h_{b}_{k}", _ptr(a))
    refl = np.zeros(chains, dtype=np.int32)
    d.reflected = refl.ctypes.data_as(C.POINTER(C.c_int))
    arrays["reflected"] = refl
    return d, arrays


def diag_result(d, arrays) -> dict:
    out = {k: v for k, v in arrays.items() if k != "reflected"}
    out["reflected"] = arrays["reflected"].astype(bool)
    out["scalars"] = {b: {k: float(d.scalars[i][j]) for j, k in enumerate(_lib.DIAG_SCALARS)}
                      for i, b in enumerate(_lib.DIAG_BLOCKS)}
    return out


def combine(handle, states, align=True, signs=None, summaries=None) -> dict:
    """Pool the state blocks `states` (device tensors or Samplers with summaries on, all on handle's device) with
    gpirt_chains_combine.  Returns dict(summary=..., diagnostics=... (states with GPIRT_SUM_DIAG), IRFs=...).
    summaries: the pooled parts to return (default: every part the states carry)."""
    from .sampler import _summary_arrays, _totals
    lib = _lib.load()
    tensors, nc, ptrs = _lib.state_ptrs(states, "summary_state")
    hdr = state_header(tensors[0])
    n, m, parts = hdr["n"], hdr["m"], hdr["parts"]
    want = (parts & _lib.SUM_POOLED) if summaries is None else _lib.summary_parts(summaries) | _lib.SUM_THETA_BETA
    sm = _lib.Summary()
    sm.parts = want
    arrays = _summary_arrays(want, n, m)
    for k, a in arrays.items():
        setattr(sm, "h_" + k, _ptr(a))
    sg = None
    if signs is not None:
        sg = (C.c_int * nc)(*[int(x) for x in signs])
    d, darr = diag_struct(parts, n, m, nc) if parts & _lib.SUM_DIAG else (None, None)
    irf = np.empty((NGRID, m), order="F")
    check(lib.gpirt_chains_combine(handle.ptr, nc, ptrs, sg, int(bool(align)), _ptr(irf), C.byref(sm),
                                   C.byref(d) if d is not None else None))
    out = dict(summary=dict(arrays, **({"totals": _totals(sm.totals)} if want & _lib.SUM_WAIC else {})), IRFs=irf)
    if d is not None:
        out["diagnostics"] = diag_result(d, darr)
    return out


# ---------------------------------------------------------------------------------------------------------- NumPy ---
def _split_rhat(half_means, half_vars, N):
    """half_means / half_vars: (M, ...) over the M = 2C half-chains of N draws."""
    M = half_means.shape[0]
    xbar = half_means.mean(axis=0)
    B = N / (M - 1) * ((half_means - xbar) ** 2).sum(axis=0)
    W = half_vars.mean(axis=0)
    varp = (N - 1) / N * W + B / N
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.sqrt(varp / W)
    r = np.where(W > 0, r, np.where(B > 0, np.inf, np.nan))
    return r


def diagnostics_from_draws(draws, signs=None, reflect=None):
    """Split-R-hat, batch-means ESS and MCSE from stored draws `draws` (C, S, ...) in NumPy, two-pass, with the formulas of
    include/gpirt_hip.h GPIRT_SUM_DIAG; also the pooled mean and variance (ddof 1) over all C S draws.  signs (C values of
    +-1, e.g. from reflection_signs) multiply each chain's draws first; `reflect` (a boolean mask over the value axes)
    limits that to the values a reflection negates (theta, the beta slope row; default: all).
    Returns dict(rhat, ess, mcse, mean, var)."""
    x = np.asarray(draws, dtype=np.float64)
    C_, S = x.shape[0], x.shape[1]
    if signs is not None:
        sg = np.asarray(signs, dtype=np.float64).reshape((C_, 1) + (1,) * (x.ndim - 2))
        if reflect is None:
            x = x * sg
        else:
            x = np.where(np.asarray(reflect)[None, None], x * sg, x)
    rest = x.shape[2:]
    nan = np.full(rest, np.nan)
    N = S // 2
    if S >= 4:
        halves = np.concatenate([x[:, :N], x[:, S - N:]], axis=0)          # (2C, N, ...): order does not matter
        rhat = _split_rhat(halves.mean(axis=1), halves.var(axis=1, ddof=1), N)
    else:
        rhat = nan.copy()
    b = int(np.floor(np.sqrt(S))) if S >= 1 else 1
    while b * b > S:
        b -= 1
    while (b + 1) * (b + 1) <= S:
        b += 1
    a = S // b
    if a >= 2 and S >= 2:
        bm = x[:, :a * b].reshape((C_, a, b) + rest).mean(axis=2)           # (C, a, ...)
        sig = b / (a - 1) * ((bm - bm.mean(axis=1, keepdims=True)) ** 2).sum(axis=1)
        lam = x.var(axis=1, ddof=1)
        ess = C_ * S * lam.mean(axis=0) / sig.mean(axis=0)
        mcse = np.sqrt(sig.mean(axis=0) / (C_ * S))
    else:
        ess, mcse = nan.copy(), nan.copy()
    flat = x.reshape((C_ * S,) + rest)
    return dict(rhat=rhat, ess=ess, mcse=mcse, mean=flat.mean(axis=0),
                var=flat.var(axis=0, ddof=1) if C_ * S >= 2 else nan.copy())


def reflection_signs(theta_means):
    """The alignment rule: chain c >= 1 is reflected when sum_i thetabar_c,i thetabar_0,i < 0.  theta_means (C, n)."""
    t = np.asarray(theta_means, dtype=np.float64)
    return np.array([1] + [(-1 if float(np.dot(t[c], t[0])) < 0 else 1) for c in range(1, t.shape[0])])


def block_scalars(rhat, ess) -> dict:
    r, e = np.ravel(rhat), np.ravel(ess)
    rn, en = np.isnan(r), np.isnan(e)
    return dict(max_rhat=float(r[~rn].max()) if (~rn).any() else float("nan"),
                min_ess=float(e[~en].min()) if (~en).any() else float("nan"),
                n_rhat_high=float((r[~rn] > 1.01).sum()), n_rhat_nan=float(rn.sum()), n_ess_nan=float(en.sum()))


# ---------------------------------------------------------------------------------------------------- one per rank ---
def run_distributed(y, sample_iterations, burn_iterations, theta_init=None, beta_prior_means=None, beta_prior_sds=None,
                    beta_proposal_sds=None, *, dist, handle=None, seed=1, preset=None, summaries=None, align=True,
                    **sampler_kw):
    """One chain per torch.distributed rank (chain index = rank): rank r runs the chain gpirt_mcmc_chains runs as chain r
    (seed gpirt_chain_seed(seed, r), theta_init[r] or the default init of gpirtMCMC(chains=...)), sends its state block to
    rank 0, which combines.  Returns the combined dict on rank 0 (summary, diagnostics, IRFs) and None elsewhere.  y is
    the coded n x m response matrix (+1 / -1 / NaN).  Item sharding and chains are separate features."""
    import torch
    from .ops import Handle
    from .sampler import Sampler
    rank, world = dist.get_rank(), dist.get_world_size()
    y = np.asfortranarray(np.asarray(y, dtype=np.float64))
    n = y.shape[0]
    if theta_init is None:
        th0 = default_inits(n, world, seed)[rank]
    else:
        t = np.asarray(theta_init, dtype=np.float64)
        th0 = t[rank] if t.ndim == 2 else t
    own = handle is None
    h = Handle() if own else handle
    parts = (_lib.summary_parts(summaries) if summaries is not None else 0) | _lib.SUM_THETA_BETA
    S, B = int(sample_iterations), int(burn_iterations)
    s = Sampler(h, y, th0, beta_prior_means, beta_prior_sds, beta_proposal_sds, seed=_lib.chain_seed(seed, rank),
                preset=preset, **sampler_kw)
    s.init()
    s.summary_enable(parts | _lib.SUM_DIAG, planned_draws=S)
    for it in range(S + B):
        s.step()
        if it >= B:
            s.accumulate_irf()
            s.summary_accumulate()
    s.check()
    state = s.summary_state()
    torch.cuda.synchronize()
    out = None
    if rank == 0:
        states = [state] + [torch.empty_like(state) for _ in range(world - 1)]
        for r in range(1, world):
            dist.recv(states[r], src=r)
        out = combine(h, states, align=align)
    else:
        dist.send(state, dst=0)
    dist.barrier()
    s.close()
    if own:
        h.close()
    return out


def default_inits(n: int, chains: int, seed: int) -> np.ndarray:
    """gpirtMCMC(chains=C)'s default theta_init (C, n): chain 0 today's RStream(seed).rnorm(n), chain c
    RStream(chain_seed(seed, c) & 0xFFFFFFFF).rnorm(n)."""
    from .ops import RStream
    return np.stack([RStream(seed if c == 0 else _lib.chain_seed(seed, c) & 0xFFFFFFFF).rnorm(n) for c in range(chains)])
