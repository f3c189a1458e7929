"""Posterior predictive checks of items, respondents and the whole matrix without stored draws (include/gpirt_hip.h,
"posterior predictive checks": gpirt_sampler_ppc_*, gpirt_ppc_combine, gpirt_mcmc_ppc; csrc/ppc.hip).

For every sampling draw the device replicates the response matrix -- yrep_ij = +1 if u_ij < plogis(f_ij + mu_ij), else -1,
u_ij the item-RNG uniform of (seed, iter, ST_PPC, item0 + j, i) -- and compares, per item, per respondent and overall, the
number of yes answers and the deviance of the replicate with those of the data.  `result` / `struct` wrap the C struct,
`combine` pools chains' state blocks, and `from_draws` is the NumPy statement of the header over stored g = f + mu draws,
with its own vectorised Philox4x32-10: every integer output comes as a pair (lo, hi) that brackets what any evaluation
of plogis within 1e-13 may decide.
The pairwise item checks ("pairwise item checks" in the header; csrc/ppc_pairs.hip) are an add-on: `pairs_struct` /
`pairs_result` wrap gpirt_ppc_pairs, `pairs_combine` pools chains' state blocks, `pairs_from_rep` is the NumPy statement of
the header over stored replicates (int64 matmuls, Python-integer cross products) and `pairs_from_draws` builds those
replicates from stored g draws.
ShardedSampler is not covered: the respondents' statistics would need one all-reduce per draw.  The keying of the
uniforms by the global item index keeps that possible.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import PAIRS_COUNTS, PAIRS_FIELDS, PAIRS_SUMS, PPC_FIELDS, ST_PPC, check

_dp = C.POINTER(C.c_double)
INT_FIELDS = ("n_obs", "obs_yes", "yes_ge", "yes_gt", "dev_ge", "nonfinite", "rep_yes_sum", "rep_yes_sumsq", "correct_sum")
U_TOL = 1e-13          # |u - p| at or below: the cell's replicate is undecided
D_TOL = 1e-10          # 0 < |Delta| <= D_TOL sum_flipped |g|: the deviance comparison is undecided

_M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------------ the device ---
def struct(n: int, m: int, fields=PPC_FIELDS):
    """A gpirt_ppc with host arrays for `fields` of the items and the respondents, and those arrays (kept alive by the
    caller) as {"item": {...}, "respondent": {...}}."""
    p = _lib.Ppc()
    arrays = {"item": {}, "respondent": {}}
    for name in fields:
        k = PPC_FIELDS.index(name)
        for unit, size in (("item", m), ("respondent", n)):
            a = np.empty(size)
            arrays[unit][name] = a
            getattr(p, unit)[k] = a.ctypes.data_as(_dp)
    return p, arrays


def derive(d: dict) -> dict:
    """Adds ppp_yes = yes_ge / S, ppp_yes_mid = (yes_ge + yes_gt) / 2S and ppp_dev = dev_ge / S, S = draws - nonfinite
    (NaN where S = 0 or the unit has no observed cell); d: the fields of one kind of unit (or the totals)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        S = np.asarray(d["draws"], dtype=np.float64) - np.asarray(d["nonfinite"], dtype=np.float64)
        S = np.where((S > 0) & (np.asarray(d["n_obs"]) > 0), S, np.nan)
        d["ppp_yes"] = np.asarray(d["yes_ge"]) / S
        d["ppp_yes_mid"] = (np.asarray(d["yes_ge"]) + np.asarray(d["yes_gt"])) / (2.0 * S)
        d["ppp_dev"] = np.asarray(d["dev_ge"]) / S
    return d


def result(p, arrays) -> dict:
    """The "ppc" dict of gpirtMCMC(ppc=True) and combine(): "item" and "respondent" (dicts of arrays, the derived ppp_*
    values included) and "totals" (a dict of floats)."""
    tot = {k: float(p.totals[i]) for i, k in enumerate(PPC_FIELDS)}
    out = {}
    for unit in ("item", "respondent"):
        out[unit] = derive(dict(arrays[unit]))
    out["totals"] = {k: float(v) for k, v in derive(dict(tot)).items()}
    return out


def combine(handle, states) -> dict:
    """gpirt_ppc_combine over the PPC state blocks `states` (device tensors, or Samplers with ppc_enable() on, all on
    handle's device): the integer sums and counts added, the double sums added in chain order.  The theta -> -theta
    reflection changes no PPC output, so there are no signs and no alignment."""
    lib = _lib.load()
    tensors = [s.ppc_state() if hasattr(s, "ppc_state") else s for s in states]
    hdr = state_header(tensors[0])
    p, arrays = struct(hdr["n"], hdr["m"])
    nc = len(tensors)
    ptrs = (C.c_void_p * nc)(*[t.data_ptr() for t in tensors])
    check(lib.gpirt_ppc_combine(handle.ptr, nc, ptrs, C.byref(p)))
    return result(p, arrays)


def state_header(state) -> dict:
    """The 8 int64 header words of a PPC state block (a device tensor): n, m, draws, layout version, item0."""
    w = state[:8].cpu().numpy().view(np.int64)
    return dict(n=int(w[0]), m=int(w[1]), draws=int(w[2]), version=int(w[3]), item0=int(w[4]))


# ------------------------------------------------------------------------------------- pairwise item checks: device ---
DEFAULT_PAIRS_TOP = 20


def check_pairs_top(top) -> int:
    t = int(top)
    if t != top or not 1 <= t <= _lib.PAIRS_MAX_TOP:
        raise ValueError(f"pairs: top must be an integer in 1..{_lib.PAIRS_MAX_TOP}")
    return t


def pairs_struct(m: int, top=DEFAULT_PAIRS_TOP):
    """A gpirt_ppc_pairs with host arrays for every output, and those arrays (kept alive by the caller)."""
    p = _lib.PpcPairs()
    p.top = check_pairs_top(top)
    arr = {}
    for k, name in enumerate(PAIRS_FIELDS):
        arr[name] = np.empty((m, m))
        p.field[k] = arr[name].ctypes.data_as(_dp)
    for name in PAIRS_SUMS:
        arr[name] = np.empty((m, m), dtype=np.uint64)
        setattr(p, name, arr[name].ctypes.data_as(C.POINTER(C.c_uint64)))
    for k, name in enumerate(PAIRS_COUNTS):
        arr[name] = np.empty((m, m), dtype=np.uint32)
        p.count[k] = arr[name].ctypes.data_as(C.POINTER(C.c_uint32))
    arr["extreme_pairs"] = np.empty((p.top, 2), dtype=np.int64)
    p.extreme_pairs = arr["extreme_pairs"].ctypes.data_as(C.POINTER(C.c_int64))
    for name in ("extreme_ppp_or_mid", "extreme_log_or_obs"):
        arr[name] = np.empty(p.top)
        setattr(p, name, arr[name].ctypes.data_as(_dp))
    return p, arr


def pairs_result(p, arr) -> dict:
    """The "pairs" dict of gpirtMCMC(ppc=dict(pairs=True)), Sampler.ppc_pairs() and pairs_combine(): every m x m array of
    the header by name (pair (a, b) at [a, b]), "extreme" (dict: pairs (top x 2), ppp_or_mid, log_or_obs) and the counters."""
    out = {k: v for k, v in arr.items() if not k.startswith("extreme_")}
    out["extreme"] = dict(pairs=arr["extreme_pairs"], ppp_or_mid=arr["extreme_ppp_or_mid"], log_or_obs=arr["extreme_log_or_obs"])
    out.update(n=int(p.n), m=int(p.m), pair_draws=int(p.pair_draws), pair_skipped=int(p.pair_skipped))
    return out


def pairs_combine(handle, states, top=DEFAULT_PAIRS_TOP) -> dict:
    """gpirt_ppc_pairs_combine over the pairwise state blocks `states` (device tensors, or Samplers with ppc_pairs_enable()
    on, all on handle's device): every array and both counters added.  Blocks with another n, m or n_co are refused."""
    lib = _lib.load()
    tensors = [s.ppc_pairs_state() if hasattr(s, "ppc_pairs_state") else s for s in states]
    m = pairs_state_header(tensors[0])["m"]
    p, arr = pairs_struct(m, top)
    nc = len(tensors)
    ptrs = (C.c_void_p * nc)(*[t.data_ptr() for t in tensors])
    check(lib.gpirt_ppc_pairs_combine(handle.ptr, nc, ptrs, C.byref(p)))
    return pairs_result(p, arr)


def pairs_state_header(state) -> dict:
    """The 8 int64 header words of a pairwise state block (a device tensor)."""
    w = state[:8].cpu().numpy().view(np.int64)
    return dict(n=int(w[0]), m=int(w[1]), version=int(w[2]), pair_draws=int(w[3]), pair_skipped=int(w[4]), item0=int(w[5]),
                tag=int(w[7]))


# -------------------------------------------------------------------------------------- pairwise item checks: NumPy ---
def pairs_from_rep(y, rep_draws, top=DEFAULT_PAIRS_TOP, skipped=0) -> dict:
    """The header's pairwise item checks from stored replicates: y (n x m; NaN = missing), rep_draws (S, n, m) with
    rep[s, i, j] != 0 where yrep = +1 (cells where y is missing are masked out here), one entry per COUNTED draw.  Returns
    pairs_result's dict: the counts are int64 matrix products, the odds-ratio decisions Python-integer cross products, every
    finished double one correctly rounded division of exact integers (log_or_obs: that and math.log)."""
    import math
    top = check_pairs_top(top)
    y = np.asarray(y, dtype=np.float64)
    n, m = y.shape
    rep_draws = np.asarray(rep_draws)
    S = rep_draws.shape[0]
    assert rep_draws.shape == (S, n, m)
    O = (~np.isnan(y)).astype(np.int64)
    Y = (y > 0).astype(np.int64)
    n_co, o11, o1 = O.T @ O, Y.T @ Y, Y.T @ O

    def table(x11, x1):
        t10, t01 = x1 - x11, x1.T - x11
        return x11, t10, t01, n_co - x11 - t10 - t01

    o = table(o11, o1)
    live = (n_co > 0) & ~np.eye(m, dtype=bool)
    z = lambda dt: np.zeros((m, m), dtype=dt)            # noqa: E731
    sum_n11, sumsq_n11, sum_n1 = z(np.int64), z(np.int64), z(np.int64)
    cnt = {k: z(np.int64) for k in PAIRS_COUNTS}
    # the cross products as Python integers (object arrays): exact whatever n is
    big = lambda t: (2 * t + 1).astype(object)           # noqa: E731
    obs_main, obs_cross = big(o[0]) * big(o[3]), big(o[1]) * big(o[2])
    for s in range(S):
        rep = (rep_draws[s] != 0).astype(np.int64) * O
        r = table(rep.T @ rep, rep.T @ O)
        sum_n11 += np.where(live, r[0], 0)
        sumsq_n11 += np.where(live, r[0] * r[0], 0)
        sum_n1 += np.where(live, r[0] + r[1], 0)
        cnt["n11_ge"] += live & (r[0] >= o[0]); cnt["n11_gt"] += live & (r[0] > o[0])
        cnt["agree_ge"] += live & (r[0] + r[3] >= o[0] + o[3]); cnt["agree_gt"] += live & (r[0] + r[3] > o[0] + o[3])
        lhs, rhs = big(r[0]) * big(r[3]) * obs_cross, obs_main * big(r[1]) * big(r[2])
        cnt["or_ge"] += live & (lhs >= rhs).astype(bool)
        cnt["or_gt"] += live & (lhs > rhs).astype(bool)
    nan = np.full((m, m), np.nan)

    def ratio(num, den, ok=True):
        """num / den where `live` (and ok): both exact integers below 2^53, so one correctly rounded division each"""
        out = nan.copy()
        if not ok:
            return out
        num = np.broadcast_to(np.asarray(num, dtype=np.int64), (m, m))[live]
        den = np.broadcast_to(np.asarray(den, dtype=np.int64), (m, m))[live]
        assert (np.abs(num) < 2**53).all() and (den > 0).all() and (den < 2**53).all()
        out[live] = num.astype(np.float64) / den.astype(np.float64)
        return out

    Sn = S * n_co
    f = {"n_co": n_co.astype(np.float64)}
    for k, t in zip(("obs_n11", "obs_n10", "obs_n01", "obs_n00"), o):
        f[k] = np.where(live, t, np.nan).astype(np.float64)
    f["rep_n11_mean"] = ratio(sum_n11, S, S >= 1)
    f["rep_n11_var"] = nan.copy()
    if S >= 2:
        for a, b in np.argwhere(live):                   # the numerator may pass 2^53: Python integers, rounded once
            f["rep_n11_var"][a, b] = float(S * int(sumsq_n11[a, b]) - int(sum_n11[a, b]) ** 2) / (float(S) * float(S - 1))
    f["rep_n10_mean"] = ratio(sum_n1 - sum_n11, S, S >= 1)
    f["rep_n01_mean"] = ratio(sum_n1.T - sum_n11, S, S >= 1)
    f["rep_n00_mean"] = ratio(Sn + sum_n11 - sum_n1 - sum_n1.T, S, S >= 1)
    f["agree_obs"] = ratio(o[0] + o[3], n_co)
    f["agree_rep_mean"] = ratio(Sn + 2 * sum_n11 - sum_n1 - sum_n1.T, np.where(live, Sn, 1), S >= 1)
    f["log_or_obs"] = nan.copy()
    for a, b in np.argwhere(live):                       # (math.log: the C library's, as the host code's)
        f["log_or_obs"][a, b] = math.log(float(obs_main[a, b]) / float(obs_cross[a, b]))
    for k in ("n11", "agree", "or"):
        f[f"ppp_{k}"] = ratio(cnt[f"{k}_ge"], S, S >= 1)
        f[f"ppp_{k}_mid"] = ratio(cnt[f"{k}_ge"] + cnt[f"{k}_gt"], 2 * S, S >= 1)
    out = {k: f[k] for k in PAIRS_FIELDS}
    out.update(sum_n11=sum_n11.astype(np.uint64), sumsq_n11=sumsq_n11.astype(np.uint64), sum_n1=sum_n1.astype(np.uint64))
    out.update({k: cnt[k].astype(np.uint32) for k in PAIRS_COUNTS})
    # extreme: the pairs a < b in (a, b) order, stably sorted by decreasing |ppp_or_mid - 0.5|
    ia, ib = np.triu_indices(m, 1)
    mid = f["ppp_or_mid"][ia, ib]
    ok = ~np.isnan(mid)
    ia, ib, mid = ia[ok], ib[ok], mid[ok]
    order = np.argsort(-np.abs(mid - 0.5), kind="stable")[:top]
    ex = dict(pairs=np.full((top, 2), -1, dtype=np.int64), ppp_or_mid=np.full(top, np.nan), log_or_obs=np.full(top, np.nan))
    ex["pairs"][:len(order), 0], ex["pairs"][:len(order), 1] = ia[order], ib[order]
    ex["ppp_or_mid"][:len(order)] = mid[order]
    ex["log_or_obs"][:len(order)] = f["log_or_obs"][ia[order], ib[order]]
    out["extreme"] = ex
    out.update(n=n, m=m, pair_draws=S, pair_skipped=int(skipped))
    return out


def pairs_from_draws(y, g_draws, seed, iters, top=DEFAULT_PAIRS_TOP, item0=0):
    """pairs_from_rep over the replicates of stored draws: g_draws (S, n, m) the draws of g = f + mu, `iters` the
    completed-iteration counters they were accumulated at; rep = [u < plogis(g)] with replicate_uniforms' u.  A draw with a
    non-finite g in an observed cell is skipped whole (pair_skipped).  Returns (result, min |u - p| over the observed cells
    of the counted draws): a cell that close to its uniform may replicate either way under another evaluation of plogis."""
    y = np.asarray(y, dtype=np.float64)
    g_draws = np.asarray(g_draws, dtype=np.float64)
    n, m = y.shape
    obs = ~np.isnan(y)
    reps, skipped, gap = [], 0, np.inf
    for s, it in enumerate(iters):
        g = g_draws[s]
        if not np.isfinite(g[obs]).all():
            skipped += 1
            continue
        p, _ = _plogis(np.where(obs, g, 0.0))
        u = replicate_uniforms(seed, int(it), n, m, item0)
        if obs.any():
            gap = min(gap, float(np.abs(u - p)[obs].min()))
        reps.append(obs & (u < p))
    rep = np.stack(reps) if reps else np.zeros((0, n, m), dtype=bool)
    return pairs_from_rep(y, rep, top, skipped), gap


# ------------------------------------------------------------------------------------------------------- NumPy -------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of 32-bit words held in uint64 (broadcast against each other); returns the four output
    words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in (c0, c1, c2, c3))
    k0 = np.asarray(k0, dtype=np.uint64) & _M32
    k1 = np.asarray(k1, dtype=np.uint64) & _M32
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = m0 * c0
        p1 = m1 * c2
        n0 = (p1 >> s32) ^ c1 ^ k0
        n2 = (p0 >> s32) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & _M32, n2, p0 & _M32
        k0 = (k0 + w0) & _M32
        k1 = (k1 + w1) & _M32
    return c0, c1, c2, c3


def item_uniform(seed, it, stage, item, index):
    """The item-RNG uniform of (seed, iteration, stage, item, index), vectorised: 52 random bits + half an ulp."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    o0, o1, _, _ = philox4x32_10(index, item, stage, it, seed & 0xFFFFFFFF, seed >> 32)
    v = ((o0 >> np.uint64(6)) << np.uint64(26)) | (o1 >> np.uint64(6))
    return (v.astype(np.float64) + 0.5) * 2.220446049250313e-16


def replicate_uniforms(seed, it, n, m, item0=0):
    """u (n x m): u[i, j] = item_uniform(seed, it, ST_PPC, item0 + j, i)."""
    return item_uniform(seed, it, ST_PPC, (np.arange(m, dtype=np.uint64) + np.uint64(item0))[None, :],
                        np.arange(n, dtype=np.uint64)[:, None])


def _plogis(g):
    e = np.exp(-np.abs(g))
    return np.where(g >= 0, 1.0 / (1.0 + e), e / (1.0 + e)), e


def _exact_var(S, s1, s2):
    """(S sum R^2 - (sum R)^2) / (S (S - 1)): the numerator in exact integers, rounded once"""
    out = np.full(len(S), np.nan)
    for k in range(len(S)):
        Sk = int(S[k])
        if Sk >= 2:
            out[k] = float(Sk * int(s2[k]) - int(s1[k]) ** 2) / (float(Sk) * float(Sk - 1))
    return out


def from_draws(y, g_draws, seed, iters, item0=0) -> dict:
    """What the device accumulates, from stored draws: y (n x m; NaN = missing), g_draws (S, n, m) the draws of
    g = f + mu, `iters` the S completed-iteration counters the draws were accumulated at.  Returns "item", "respondent"
    and "totals" (dicts; "totals" holds 1-element arrays) with every field of the header.  Every integer field is a
    pair (lo, hi) of int64 arrays: a cell with |u - p| <= 1e-13 may replicate either way, a deviance comparison with such
    a cell in it, or with 0 < |Delta| <= 1e-10 sum_flipped |g|, may go either way.  The double fields are computed with
    the undecided cells at yrep = (u < p).  "undecided" counts those cells and comparisons, "comparisons" every
    deviance comparison made."""
    y = np.asarray(y, dtype=np.float64)
    g_draws = np.asarray(g_draws, dtype=np.float64)
    n, m = y.shape
    S = g_draws.shape[0]
    iters = [int(x) for x in iters]
    assert g_draws.shape == (S, n, m) and len(iters) == S
    obs = ~np.isnan(y)
    yes = obs & (y > 0)
    ysign = np.where(obs, y, 0.0)
    units = (("item", 0, m), ("respondent", 1, n), ("totals", None, 1))

    def usum(a, axis):
        return a.sum(axis=axis) if axis is not None else np.array([a.sum()])

    acc = {}
    for name, axis, size in units:
        z = lambda: np.zeros(size, dtype=np.int64)      # noqa: E731
        acc[name] = dict(n_obs=usum(obs, axis).astype(np.int64), obs_yes=usum(yes, axis).astype(np.int64), nonfinite=z(),
                         sum_lo=z(), sum_hi=z(), sq_lo=z(), sq_hi=z(), ge_lo=z(), ge_hi=z(), gt_lo=z(), gt_hi=z(),
                         dge_lo=z(), dge_hi=z(), correct=z(), dev_obs=np.zeros(size), dev_rep=np.zeros(size))
    und_cells = und_cmp = n_cmp = 0
    for s in range(S):
        g = g_draws[s]
        with np.errstate(invalid="ignore", over="ignore"):
            bad = obs & ~np.isfinite(g)
            gz = np.where(obs & ~bad, g, 0.0)
            p, e = _plogis(gz)
            u = replicate_uniforms(seed, iters[s], n, m, item0)
            live = obs & ~bad
            rep_yes = live & (u < p)
            und = live & (np.abs(u - p) <= U_TOL)
            l1 = np.log1p(e)
            yr = np.where(rep_yes, 1.0, -1.0)
            d_obs = np.where(live, 2.0 * (l1 + np.maximum(-ysign * gz, 0.0)), 0.0)
            d_rep = np.where(live, 2.0 * (l1 + np.maximum(-yr * gz, 0.0)), 0.0)
            flipped = live & (yr != ysign)
            delta = np.where(flipped, ysign * gz, 0.0)
            absg = np.where(flipped, np.abs(gz), 0.0)
            correct = live & ((gz > 0) == (ysign > 0))
        und_cells += int(und.sum())
        for name, axis, size in units:
            a = acc[name]
            nf = usum(bad, axis) > 0
            on = ~nf & (a["n_obs"] > 0)
            a["nonfinite"] += nf
            nu = usum(und, axis)
            R = usum(rep_yes, axis).astype(np.int64)
            R_lo = R - usum(und & rep_yes, axis)
            R_hi = R + usum(und & ~rep_yes, axis)
            T = a["obs_yes"]
            a["sum_lo"] += np.where(on, R_lo, 0); a["sum_hi"] += np.where(on, R_hi, 0)
            a["sq_lo"] += np.where(on, R_lo * R_lo, 0); a["sq_hi"] += np.where(on, R_hi * R_hi, 0)
            a["ge_lo"] += on & (R_lo >= T); a["ge_hi"] += on & (R_hi >= T)
            a["gt_lo"] += on & (R_lo > T); a["gt_hi"] += on & (R_hi > T)
            D = usum(delta, axis)
            open_ = (nu > 0) | ((D != 0) & (np.abs(D) <= D_TOL * usum(absg, axis)))
            a["dge_lo"] += on & ~open_ & (D >= 0); a["dge_hi"] += on & (open_ | (D >= 0))
            und_cmp += int((on & open_).sum())
            n_cmp += int(on.sum())
            a["correct"] += np.where(on, usum(correct, axis), 0)
            a["dev_obs"] += np.where(on, usum(d_obs, axis), 0.0)
            a["dev_rep"] += np.where(on, usum(d_rep, axis), 0.0)
    out = {}
    for name, axis, size in units:
        a = acc[name]
        Sk = S - a["nonfinite"]
        with np.errstate(invalid="ignore", divide="ignore"):
            den = np.where((a["n_obs"] > 0) & (Sk >= 1), Sk, np.nan).astype(np.float64)
            pair = lambda x: (x.copy(), x.copy())       # noqa: E731
            d = dict(n_obs=pair(a["n_obs"]), obs_yes=pair(a["obs_yes"]), nonfinite=pair(a["nonfinite"]),
                     yes_ge=(a["ge_lo"], a["ge_hi"]), yes_gt=(a["gt_lo"], a["gt_hi"]), dev_ge=(a["dge_lo"], a["dge_hi"]),
                     rep_yes_sum=(a["sum_lo"], a["sum_hi"]), rep_yes_sumsq=(a["sq_lo"], a["sq_hi"]),
                     correct_sum=pair(a["correct"]), draws=np.full(size, float(S)),
                     rep_yes_mean=((a["sum_lo"] + a["sum_hi"]) * 0.5) / den,
                     rep_yes_var=np.where(a["n_obs"] > 0, _exact_var(Sk, a["sum_lo"], a["sq_lo"]), np.nan),
                     dev_obs_mean=a["dev_obs"] / den, dev_rep_mean=a["dev_rep"] / den, correct_mean=a["correct"] / den)
        out[name] = d
    out["undecided"] = dict(cells=und_cells, comparisons=und_cmp)
    out["comparisons"] = n_cmp
    return out
