"""Autocorrelation ESS without stored draws: the lag-window estimate of the effective sample size (Geyer's initial monotone
sequence over split chains), the integrated autocorrelation time tau, the MCSE that follows from it and the autocorrelation
function of theta, beta and three log-likelihood series (include/gpirt_hip.h, "autocorrelation ESS": gpirt_sampler_acf_*,
gpirt_acf_combine; csrc/acf.hip).

Per draw the device keeps the last L + 1 centred values of every tracked series in a ring and adds the lag products s_k += d_t
d_{t-k}, k = 0 .. L, for the draw's split half; nothing grows with the chain.  `struct` / `result` wrap the C struct, `combine`
finishes chains' state blocks, `from_draws` is the NumPy statement of the header over fetched draws -- the raw sums as the
device forms them (integers for theta, sequential fp64 in draw order for the rest), everything after them in long double --
and `run` drives the stage API for C chains in one call.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import (ACF_BETA, ACF_BLOCK_COUNTS, ACF_BLOCK_STATS, ACF_BLOCKS, ACF_DEFAULT_LAG, ACF_FLAGS, ACF_LL, ACF_MAX_LAG,
                   ACF_MAX_TOP, ACF_PARTS, ACF_RAW, ACF_THETA, ACF_VALUES, check)

DEFAULT_TOP = 20
LL_ROWS, LL_COLS = 256, 32                       # a work-group of the log-likelihood pass: rows x columns


# ---------------------------------------------------------------------------------------------------- the contract ---
def parts_mask(parts) -> int:
    """A mask of ACF_THETA | ACF_BETA | ACF_LL from an integer, a name or names of ("theta", "beta", "ll"), or "all"."""
    if isinstance(parts, (int, np.integer)) and not isinstance(parts, bool):
        mask = int(parts)
    elif parts == "all":
        mask = ACF_THETA | ACF_BETA | ACF_LL
    else:
        names = [parts] if isinstance(parts, str) else list(parts)
        unknown = [p for p in names if p not in ACF_PARTS]
        if unknown:
            raise ValueError(f"acf: unknown parts {unknown}; known: {sorted(ACF_PARTS)} or 'all'")
        mask = 0
        for p in names:
            mask |= ACF_PARTS[p]
    if mask <= 0 or mask & ~(ACF_THETA | ACF_BETA | ACF_LL):
        raise ValueError(f"acf: parts = {parts!r}, it must be a non-empty mask of theta | beta | ll")
    return mask


def check_top(top):
    if isinstance(top, bool) or not isinstance(top, (int, np.integer)) or not 1 <= int(top) <= ACF_MAX_TOP:
        raise ValueError(f"acf: top must be an integer in 1 .. {ACF_MAX_TOP} (got {top!r})")
    return int(top)


def lag_window(planned_draws, max_lag=None) -> int:
    """L for a chain of `planned_draws` draws: max_lag, or min(H - 1, 256) with H = planned_draws // 2.  H < 4 and a max_lag
    outside 1 .. min(H - 1, 1024) are ValueErrors that say so (gpirt_acf_check's rule)."""
    if planned_draws is None:
        raise ValueError("acf: the planned number of draws is needed (no planned draws)")
    S = int(planned_draws)
    H = S // 2
    if S < 1 or H < 4:
        raise ValueError(f"acf: {S} planned draws give halves of {max(H, 0)} draws, fewer than 4")
    cap = min(H - 1, ACF_MAX_LAG)
    if max_lag is None:
        return min(H - 1, ACF_DEFAULT_LAG)
    if isinstance(max_lag, bool) or not isinstance(max_lag, (int, np.integer)) or not 1 <= int(max_lag) <= cap:
        raise ValueError(f"acf: max_lag = {max_lag!r}, it must lie in 1 .. min(H - 1, {ACF_MAX_LAG}) = {cap} for halves of "
                         f"H = {H} draws")
    return int(max_lag)


def value_blocks(n: int, m: int, parts: int) -> dict:
    """name -> slice of the P tracked values, in the header's order: theta, beta, item_ll, resp_ll, total_ll (an untracked block
    is an empty slice)."""
    Pi = n if parts & ACF_THETA else 0
    o_item = Pi + (2 * m if parts & ACF_BETA else 0)
    ll = bool(parts & ACF_LL)
    edges = [0, Pi, o_item, o_item + (m if ll else 0), o_item + (m + n if ll else 0), o_item + (m + n + 1 if ll else 0)]
    return {name: slice(edges[k], edges[k + 1]) for k, name in enumerate(ACF_BLOCKS)}


def n_values(n: int, m: int, parts: int) -> int:
    return value_blocks(n, m, parts)["total_ll"].stop


def raw_shape(name: str, P: int, L: int):
    if name in ("s", "head", "tail"):
        return (2, L + 1, P)
    if name == "sum":
        return (2, P)
    if name == "ring":
        return (L + 1, P)
    if name in ("centre", "nonfinite", "last"):
        return (P,)
    raise ValueError(f"acf: unknown array '{name}'")


def decode_raw(name: str, words: np.ndarray, Pi: int) -> np.ndarray:
    """A raw array as the device holds it (8-byte words, int64 view) as numbers: nonfinite stays int64; every other array comes
    back as float64, theta's int64 columns (the first Pi values) converted -- exactly, they are far below 2^53."""
    words = np.ascontiguousarray(words).view(np.int64)
    if name == "nonfinite":
        return words.copy()
    out = words.view(np.float64).copy()
    if name != "centre" and Pi:
        out[..., :Pi] = words[..., :Pi].astype(np.float64)
    return out


# ------------------------------------------------------------------------------------------------------ the device ---
def struct(P: int, L: int, top: int = DEFAULT_TOP):
    """A gpirt_acf asking for every array, and the host arrays behind it (kept alive by the caller)."""
    r = _lib.Acf()
    r.top = check_top(top)
    arrays = {}
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    for k, name in enumerate(ACF_VALUES):
        arrays[name] = np.zeros(P)
        r.value[k] = arrays[name].ctypes.data_as(dp)
    for k, name in enumerate(ACF_FLAGS):
        arrays[name] = np.zeros(P, dtype=np.int64)
        r.flag[k] = arrays[name].ctypes.data_as(ip)
    arrays["acf"] = np.zeros((L + 1, P))
    r.acf = arrays["acf"].ctypes.data_as(dp)
    arrays["worst_block"], arrays["worst_index"] = np.zeros(r.top, dtype=np.int64), np.zeros(r.top, dtype=np.int64)
    arrays["worst_ess"] = np.zeros(r.top)
    r.worst_block, r.worst_index = arrays["worst_block"].ctypes.data_as(ip), arrays["worst_index"].ctypes.data_as(ip)
    r.worst_ess = arrays["worst_ess"].ctypes.data_as(dp)
    return r, arrays


def _pack(n, m, parts, S, H, L, P, chains, values, flags, acf, stats, counts, worst) -> dict:
    blocks = value_blocks(n, m, parts)
    out = dict(values)
    out.update(flags)
    out.update(acf=acf, worst=worst, n=n, m=m, parts=parts, S=S, H=H, L=L, P=P, chains=chains, N=2 * chains * H,
               slices=blocks)
    out["blocks"] = {}
    for b, name in enumerate(ACF_BLOCKS):
        d = {k: float(stats[b][q]) for q, k in enumerate(ACF_BLOCK_STATS)}
        d.update({k: int(counts[b][q]) for q, k in enumerate(ACF_BLOCK_COUNTS)})
        out["blocks"][name] = d
    return out


def result(r, arrays) -> dict:
    """The dict of Sampler.acf(), combine() and run(), from a filled gpirt_acf: ess, tau, mcse, rhat, rho1, mean, sd (float64, P),
    lag_used, truncated, nonfinite, constant (int64, P), acf ((L + 1) x P), blocks (name -> min_ess, max_tau, max_rhat,
    n_truncated, n_nan), worst (block, block_name, index, ess), slices (name -> the block's slice of the P values) and the
    counters."""
    nb, ns, ncnt = len(ACF_BLOCKS), len(ACF_BLOCK_STATS), len(ACF_BLOCK_COUNTS)
    stats = np.array(r.block_stat[:]).reshape(nb, ns)
    counts = np.array(r.block_count[:], dtype=np.int64).reshape(nb, ncnt)
    wb = arrays["worst_block"]
    worst = dict(block=wb, block_name=[ACF_BLOCKS[b] if b >= 0 else None for b in wb], index=arrays["worst_index"],
                 ess=arrays["worst_ess"])
    return _pack(int(r.n), int(r.m), int(r.parts), int(r.S), int(r.H), int(r.L), int(r.P), int(r.chains),
                 {k: arrays[k] for k in ACF_VALUES}, {k: arrays[k] for k in ACF_FLAGS}, arrays["acf"], stats, counts, worst)


def state_header(state) -> dict:
    """The header of an ACF state block (a device tensor of int64)."""
    w = _lib.header_words(state, 16)
    names = ("tag", "version", "n", "m", "parts", "S", "H", "L", "P", "draws")
    return {k: int(w[i]) for i, k in enumerate(names)}


def combine(handle, states, signs=None, top=DEFAULT_TOP) -> dict:
    """gpirt_acf_combine over the state blocks `states` (device tensors, or Samplers with acf_enable() on, all on handle's
    device), each with all of its planned draws in.  signs: None, or one +1 / -1 per chain (-1: the chain enters reflected,
    theta -> -theta with the beta slopes; `1 - 2 * diagnostics["reflected"]` of gpirt_amd.chains.combine)."""
    lib = _lib.load()
    tensors, nc, ptrs = _lib.state_ptrs(states, "acf_state")
    hdr = state_header(tensors[0])
    if hdr["tag"] != _lib.ACF_TAG:
        raise ValueError("acf.combine: state 0 is not an ACF state block")
    r, arrays = struct(hdr["P"], hdr["L"], top)
    sg = None
    if signs is not None:
        if len(signs) != nc:
            raise ValueError(f"acf.combine: {len(signs)} signs for {nc} states")
        sg = (C.c_int * nc)(*[int(x) for x in signs])
    check(lib.gpirt_acf_combine(handle.ptr, nc, ptrs, sg, C.byref(r)))
    return result(r, arrays)


# ------------------------------------------------------------------------------------------------------- NumPy -------
def ll_series(g, y) -> np.ndarray:
    """item_ll (m), resp_ll (n) and total_ll of one draw's g = f + mu (n x m) in fp64, in the device's order of additions
    (include/gpirt_hip.h, LOG-LIKELIHOOD).  exp and log1p are NumPy's: equal to the device's up to their last bits."""
    g, y = np.asarray(g, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, m = y.shape
    with np.errstate(all="ignore"):
        cell = np.where(np.isnan(y), 0.0, -(np.log1p(np.exp(-np.abs(g))) + np.fmax(-(y * g), 0.0)))
    resp = np.zeros(n)
    for q0 in range(0, m, LL_COLS):
        part = np.zeros(n)
        for j in range(q0, min(q0 + LL_COLS, m)):
            part = part + cell[:, j]
        resp = resp + part
    nb = -(-n // LL_ROWS)
    v = np.zeros((nb * LL_ROWS, m))
    v[:n] = cell
    v = v.reshape(nb, LL_ROWS // 64, 64, m)
    w = 32
    while w >= 1:
        v = v[:, :, :w] + v[:, :, w:2 * w]
        w //= 2
    v = v[:, :, 0]
    cp = (v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])
    item = np.zeros(m)
    for b in range(nb):
        item = item + cp[b]
    total = 0.0
    for j in range(m):
        total = total + item[j]
    return np.concatenate([item, resp, [total]])


def _theta_d(x):
    """theta draws as the integers k - 500 and the mask of the values off the grid (which enter as 0)"""
    with np.errstate(all="ignore"):
        k = np.rint((x + 5.0) * 100.0)
        ok = (k >= 0.0) & (k <= 1000.0) & (-5.0 + k * 0.01 == x)
    return np.where(ok, k - 500.0, 0.0).astype(np.int64), ~ok


def raw_from_series(x, Pi: int, planned: int, L: int) -> dict:
    """The raw arrays of one chain from its S x P values x (theta's first Pi columns as drawn): s, sum, head, tail, ring (float64,
    theta's columns exact integers), centre and nonfinite, by the header's rules -- one product and one add per term, in draw
    order."""
    x = np.asarray(x, dtype=np.float64)
    S, P = x.shape
    if S != planned:
        raise ValueError(f"acf: {S} draws for {planned} planned draws")
    H, R = planned // 2, L + 1
    dI, offgrid = _theta_d(x[:, :Pi])
    xd = x[:, Pi:]
    fin = np.isfinite(xd)
    centre = np.concatenate([np.zeros(Pi), np.where(fin[0], xd[0], 0.0)])
    with np.errstate(all="ignore"):
        dD = np.where(fin, xd - centre[Pi:], 0.0)
    out = dict(centre=centre)
    s = [np.zeros((2, R, Pi), dtype=np.int64), np.zeros((2, R, P - Pi))]
    sm = [np.zeros((2, Pi), dtype=np.int64), np.zeros((2, P - Pi))]
    hd = [np.zeros((2, R, Pi), dtype=np.int64), np.zeros((2, R, P - Pi))]
    tl = [np.zeros((2, R, Pi), dtype=np.int64), np.zeros((2, R, P - Pi))]
    ring = [np.zeros((R, Pi), dtype=np.int64), np.zeros((R, P - Pi))]
    bad = np.zeros(P, dtype=np.int64)
    for h, lo in enumerate((0, S - H)):
        rows = slice(lo, lo + H)
        bad[:Pi] += offgrid[rows].sum(axis=0)
        bad[Pi:] += (~fin[rows]).sum(axis=0)
        for sec, dall in enumerate((dI, dD)):
            d = dall[rows]
            for t in range(1, H + 1):
                kmax = min(L, t - 1)
                back = d[t - 1 - kmax:t][::-1]                         # d_t, d_{t-1}, ..., d_{t-kmax}
                s[sec][h, :kmax + 1] += d[t - 1] * back
                sm[sec][h] += d[t - 1]
                if t <= L:
                    hd[sec][h, t] = sm[sec][h]
                ring[sec][(t - 1) % R] = d[t - 1]
            acc = np.zeros_like(sm[sec][h])
            for k in range(1, L + 1):
                acc = acc + d[H - k]
                tl[sec][h, k] = acc
    cat = lambda a: np.concatenate([a[0].astype(np.float64), a[1]], axis=-1)     # noqa: E731
    out.update(s=cat(s), sum=cat(sm), head=cat(hd), tail=cat(tl), ring=cat(ring), nonfinite=bad)
    return out


def reflect_raw(raw: dict, n: int, m: int, parts: int) -> dict:
    """A chain's raw arrays as they enter with sign -1: theta's and the beta slopes' sum, head and tail negated, the slopes'
    centre negated; s, the log-likelihood series and the intercepts untouched."""
    bl = value_blocks(n, m, parts)
    flip = np.zeros(bl["total_ll"].stop, dtype=bool)
    flip[bl["theta"]] = True
    flip[bl["beta"]] = np.arange(bl["beta"].stop - bl["beta"].start) % 2 == 1
    out = dict(raw)
    for k in ("sum", "head", "tail", "centre", "ring"):
        out[k] = np.where(flip, -raw[k], raw[k])
    return out


def finish(raws, signs, n: int, m: int, parts: int, planned: int, L: int, top=DEFAULT_TOP, dtype=np.longdouble) -> dict:
    """The finish of the header from the chains' raw arrays (a list of raw_from_series's or Sampler.acf_get's dicts), in `dtype`.
    Beside result()'s keys the dict carries pairs (the P_j as formed, before the running minimum; NaN from the stopping pair
    on) and margin (per value the smallest distance of a P_j from 0 and from its predecessor's running minimum, over the pairs
    up to the one that stops the sequence): what a comparison of lag_used and truncated has to respect."""
    top = check_top(top)
    nc = len(raws)
    signs = [1] * nc if signs is None else [int(v) for v in signs]
    if len(signs) != nc or any(v not in (1, -1) for v in signs):
        raise ValueError("acf: signs must be one +1 or -1 per chain")
    raws = [reflect_raw(r, n, m, parts) if sg < 0 else r for r, sg in zip(raws, signs)]
    H, R = planned // 2, L + 1
    P = raws[0]["centre"].shape[0]
    ld = lambda a: np.asarray(a, dtype=dtype)                                    # noqa: E731
    sm = np.concatenate([ld(r["sum"]) for r in raws])                            # (2C, P): chain 0 half 1, chain 0 half 2, ...
    s = np.concatenate([ld(r["s"]) for r in raws])                               # (2C, R, P)
    hd = np.concatenate([ld(r["head"]) for r in raws])
    tl = np.concatenate([ld(r["tail"]) for r in raws])
    cen = np.repeat(np.stack([ld(r["centre"]) for r in raws]), 2, axis=0)
    M = 2 * nc
    Hd = dtype(H)
    dbar = sm / Hd
    kk = ld(np.arange(R))[None, :, None]
    with np.errstate(all="ignore"):
        gamma = (s - dbar[:, None] * ((sm[:, None] - tl) + (sm[:, None] - hd)) + (Hd - kk) * dbar[:, None] ** 2) / Hd
        gm = gamma.mean(axis=0)
        W = gm[0] * Hd / (Hd - 1)
        hm = cen + dbar
        mean = hm.mean(axis=0)
        B = ((hm - mean) ** 2).sum(axis=0) / (M - 1)
        varp = W * (Hd - 1) / Hd + B
        constant = ~np.isfinite(W) | ~np.isfinite(varp) | (W == 0) | (varp == 0)
        rho = 1 - (W - gm) / varp
    rho[0] = 1
    npairs = (L + 1) // 2
    pairs = np.full((npairs, P), np.nan, dtype=dtype)
    margin = np.full(P, np.inf, dtype=dtype)
    psum, prev = np.zeros(P, dtype=dtype), np.full(P, np.inf, dtype=dtype)
    open_ = ~constant
    lag_used = np.zeros(P, dtype=np.int64)
    for j in range(npairs):
        pj = rho[2 * j] + rho[2 * j + 1]
        pairs[j] = np.where(open_, pj, np.nan)
        with np.errstate(all="ignore"):
            dist = np.minimum(np.abs(pj), np.abs(pj - prev))
        margin = np.where(open_, np.minimum(margin, dist), margin)
        go = open_ & (pj > 0)
        use = np.minimum(pj, prev)
        psum = np.where(go, psum + use, psum)
        prev = np.where(go, use, prev)
        lag_used = np.where(go, 2 * j + 1, lag_used)
        open_ = go
    N = dtype(M * H)
    tau = np.maximum(-1 + 2 * psum, 1 / np.log10(N))
    with np.errstate(all="ignore"):
        ess = N / tau
        vals = dict(ess=ess, tau=tau, mcse=np.sqrt(varp / ess), rhat=np.sqrt(varp / W), rho1=rho[1])
        sd = np.sqrt(varp)
    nan = np.float64("nan")
    values = {k: np.where(constant, nan, v).astype(np.float64) for k, v in vals.items()}
    values.update(mean=mean.astype(np.float64), sd=sd.astype(np.float64))
    flags = dict(lag_used=np.where(constant, 0, lag_used), truncated=np.where(constant, 0, open_).astype(np.int64),
                 nonfinite=sum(np.asarray(r["nonfinite"], dtype=np.int64) for r in raws), constant=constant.astype(np.int64))
    acf = np.where(constant[None], nan, rho).astype(np.float64)
    blocks = value_blocks(n, m, parts)
    nb = len(ACF_BLOCKS)
    stats, counts = np.full((nb, len(ACF_BLOCK_STATS)), np.nan), np.zeros((nb, len(ACF_BLOCK_COUNTS)), dtype=np.int64)
    for b, name in enumerate(ACF_BLOCKS):
        sl = blocks[name]
        e, t, r = values["ess"][sl], values["tau"][sl], values["rhat"][sl]
        if (~np.isnan(e)).any():
            stats[b, 0] = np.nanmin(e)
        if (~np.isnan(t)).any():
            stats[b, 1] = np.nanmax(t)
        if (~np.isnan(r)).any():
            stats[b, 2] = np.nanmax(r)
        counts[b] = (flags["truncated"][sl].sum(), np.isnan(e).sum())
    e = values["ess"]
    order = [p for p in np.lexsort((np.arange(P), e)) if not np.isnan(e[p])][:top]
    starts = np.array([blocks[name].start for name in ACF_BLOCKS])
    sizes = np.array([blocks[name].stop - blocks[name].start for name in ACF_BLOCKS])
    wb = np.full(top, -1, dtype=np.int64)
    wi = np.full(top, -1, dtype=np.int64)
    we = np.full(top, np.nan)
    for r_, p in enumerate(order):
        b = max(k for k in range(nb) if sizes[k] > 0 and starts[k] <= p)
        wb[r_], wi[r_], we[r_] = b, p - starts[b], e[p]
    worst = dict(block=wb, block_name=[ACF_BLOCKS[b] if b >= 0 else None for b in wb], index=wi, ess=we)
    out = _pack(n, m, parts, planned, H, L, P, nc, values, flags, acf, stats, counts, worst)
    out.update(raw=raws, pairs=pairs, margin=margin, W=W, varp=varp)
    return out


def series_from_draws(theta_draws, beta_draws, g_draws, y, ll=None):
    """One chain's S x P values and (n, m, parts): theta_draws (S x n), beta_draws (S x 2 x m), g_draws (S x n x m, f + mu) -- each
    may be None: its series is not tracked.  ll (S x (m + n + 1)) replaces the log-likelihood series computed from g_draws."""
    cols, parts = [], 0
    y = np.asarray(y, dtype=np.float64)
    n, m = y.shape
    if theta_draws is not None:
        cols.append(np.asarray(theta_draws, dtype=np.float64).reshape(-1, n))
        parts |= ACF_THETA
    if beta_draws is not None:
        b = np.asarray(beta_draws, dtype=np.float64)
        cols.append(b.reshape(b.shape[0], 2, m).transpose(0, 2, 1).reshape(b.shape[0], 2 * m))   # value 2j + r
        parts |= ACF_BETA
    if ll is not None:
        cols.append(np.asarray(ll, dtype=np.float64).reshape(-1, m + n + 1))
        parts |= ACF_LL
    elif g_draws is not None:
        g = np.asarray(g_draws, dtype=np.float64)
        cols.append(np.stack([ll_series(g[t], y) for t in range(g.shape[0])]))
        parts |= ACF_LL
    if not cols:
        raise ValueError("acf: no series (theta_draws, beta_draws and g_draws are all None)")
    return np.concatenate(cols, axis=1), n, m, parts


def from_draws(theta_draws, beta_draws, g_draws, y, planned=None, max_lag=None, signs=None, top=DEFAULT_TOP, ll=None,
               dtype=np.longdouble) -> dict:
    """The NumPy statement of the header from stored draws: theta_draws (C x S x n or S x n), beta_draws (C x S x 2 x m), g_draws
    (C x S x n x m, g = f + mu) and the data y (n x m, +1 / -1 / NaN); a None series is not tracked.  planned: S (default: the
    draws given).  The raw sums are integers for theta and sequential fp64 in draw order for the rest; everything after them is
    in long double.  ll (C x S x (m + n + 1)): the log-likelihood series to use in place of NumPy's own evaluation of g_draws
    (whose exp and log1p differ from the device's in their last bits).  Returns finish()'s dict; raw is the list of the
    chains' raw arrays as they entered (a reflected chain's after the reflection)."""
    y = np.asarray(y, dtype=np.float64)
    chains = None                                   # None: one chain's draws without the leading chain axis
    for a, base in ((theta_draws, 2), (beta_draws, 3), (g_draws, 3), (ll, 2)):
        if a is not None:
            chains = np.asarray(a).shape[0] if np.asarray(a).ndim == base + 1 else None
            break
    pick = lambda a, c: None if a is None else (np.asarray(a)[c] if chains is not None else np.asarray(a))   # noqa: E731
    raws = []
    for c in range(chains or 1):
        x, n, m, parts = series_from_draws(pick(theta_draws, c), pick(beta_draws, c), pick(g_draws, c), y, pick(ll, c))
        S = x.shape[0] if planned is None else int(planned)
        L = lag_window(S, max_lag)
        raws.append(raw_from_series(x, n if parts & ACF_THETA else 0, S, L))
    return finish(raws, signs, n, m, parts, S, L, top=top, dtype=dtype)


# ------------------------------------------------------------------------------------------------ one call for C chains ---
def run(y, sample_iterations, burn_iterations, chains=1, seed=1, *, parts="all", max_lag=None, top=DEFAULT_TOP, align=True,
        theta_init=None, preset="fast", handle=None, consistent=False, **sampler_kw) -> dict:
    """`chains` chains of the stage-driven Sampler, one after the other, each with the autocorrelation block and the DIAG
    summaries on; chain c runs with the seed chain_seed(seed, c) from gpirtMCMC(chains=...)'s default init.  The signs are the
    ones gpirt_amd.chains.combine decides for the same chains (align=False: none).  Returns combine()'s dict with
    "diagnostics" (the batch-means ones of the same chains) and "reflected" beside it.  consistent=True: every iteration is Sampler.step(consistent=True)
    (gpirt_amd.consistent); "consistent" in the result names it."""
    from . import chains as CH
    from .ops import Handle
    from .sampler import Sampler
    y = np.asfortranarray(np.asarray(y, dtype=np.float64))
    S, B, nc = int(sample_iterations), int(burn_iterations), int(chains)
    mask = parts_mask(parts)
    lag_window(S, max_lag)
    inits = CH.default_inits(y.shape[0], nc, seed) if theta_init is None else np.asarray(theta_init, dtype=np.float64).reshape(nc, -1)
    own = handle is None
    h = Handle() if own else handle
    samplers = []
    try:
        for c in range(nc):
            s = Sampler(h, y, inits[c], seed=seed if c == 0 else _lib.chain_seed(seed, c), preset=preset, **sampler_kw)
            samplers.append(s)
            s.init()
            s.summary_enable(_lib.SUM_THETA_BETA | _lib.SUM_DIAG, planned_draws=S)
            s.acf_enable(mask, S, max_lag)
            for it in range(S + B):
                s.step(consistent=consistent)
                if it >= B:
                    s.accumulate_irf()
                    s.summary_accumulate()
                    s.acf_accumulate()
            s.check()
        pooled = CH.combine(h, samplers, align=align)
        refl = pooled["diagnostics"]["reflected"]
        out = combine(h, samplers, signs=[-1 if r else 1 for r in refl], top=top)
        out.update(diagnostics=pooled["diagnostics"], reflected=refl, consistent=bool(consistent))
        return out
    finally:
        for s in samplers:
            s.close()
        if own:
            h.close()
