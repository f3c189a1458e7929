"""Posterior predictive checks of items, respondents and the whole matrix without stored draws (include/gpirt_hip.h,
"posterior predictive checks": gpirt_sampler_ppc_*, gpirt_ppc_combine, gpirt_run.ppc; csrc/ppc.hip).

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
The theta-binned item fit ("theta-binned item fit" in the header; csrc/ppc_bins.hip) is the second add-on: `check_cuts`,
`bin_of_index`, `bins_struct` / `bins_result` wrap gpirt_ppc_bins, `bins_combine` pools chains' state blocks with their
reflection signs, `bins_from_rep` is the NumPy statement of the header over stored theta, g and replicates (integers exact,
E, V and X2 in np.longdouble, the chi-square decisions as (lo, hi) brackets from `bins_bounds`) and `bins_from_draws` builds
the replicates from stored g draws.
The group-wise item fit ("group-wise item fit" in the header; csrc/ppc_dif.hip) is the third add-on and the score-based checks
("score-based PPC" in the header; csrc/ppc_scores.hip) the fourth, the person fit ("person fit in the PPC"; csrc/ppc_person.hip)
the fifth, the residual correlations ("residual correlations in the PPC"; csrc/ppc_resid.hip) the sixth: see their sections at the
end of this module.
ShardedSampler is not covered: the respondents' statistics would need one all-reduce per draw.  The keying of the
uniforms by the global item index keeps that possible.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import (BINS_BIN_FIELDS, BINS_CELL_FIELDS, BINS_ITEM_FIELDS, BINS_RAW, PAIRS_COUNTS, PAIRS_FIELDS, PAIRS_SUMS,
                   PPC_FIELDS, ST_PPC, check)

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
    tensors, nc, ptrs = _lib.state_ptrs(states, "ppc_state")
    hdr = state_header(tensors[0])
    p, arrays = struct(hdr["n"], hdr["m"])
    check(lib.gpirt_ppc_combine(handle.ptr, nc, ptrs, C.byref(p)))
    return result(p, arrays)


def state_header(state) -> dict:
    """The 8 int64 header words of a PPC state block (a device tensor): n, m, draws, layout version, item0."""
    w = _lib.header_words(state)
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
    tensors, nc, ptrs = _lib.state_ptrs(states, "ppc_pairs_state")
    m = pairs_state_header(tensors[0])["m"]
    p, arr = pairs_struct(m, top)
    check(lib.gpirt_ppc_pairs_combine(handle.ptr, nc, ptrs, C.byref(p)))
    return pairs_result(p, arr)


def pairs_state_header(state) -> dict:
    """The 8 int64 header words of a pairwise state block (a device tensor)."""
    w = _lib.header_words(state)
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


# ------------------------------------------------------------------------------------ theta-binned item fit: device ---
DEFAULT_CUTS = (14, 43, 76, 122)          # nine bins of equal N(0, 1) probability, snapped to the grid
DEFAULT_BINS_TOP = 20
_BIN_DTYPES = {"u8": np.uint64, "f8": np.float64, "u4": np.uint32}


def check_cuts(cuts) -> tuple:
    """The cuts as a tuple of ints (hundredths of theta): 1 <= d_1 < ... < d_h <= 499, 1 <= h <= 15.  Takes ints, or theta
    values that round to whole hundredths within 1e-9; anything else is a ValueError."""
    try:
        raw = list(cuts)
    except TypeError:
        raise ValueError("bins: the cuts must be a sequence of integers (hundredths of theta) or theta values") from None
    if not 1 <= len(raw) <= _lib.BINS_MAX_H:
        raise ValueError(f"bins: 1..{_lib.BINS_MAX_H} cuts are taken, {len(raw)} given")
    out = []
    for c in raw:
        if isinstance(c, (bool, np.bool_)):
            raise ValueError("bins: a cut must be a number")
        if isinstance(c, (int, np.integer)):
            d = int(c)
        elif isinstance(c, (float, np.floating)):
            d = round(float(c) * 100.0) if np.isfinite(c) else None
            if d is None or abs(float(c) * 100.0 - d) > 1e-9 * 100.0:
                raise ValueError(f"bins: the cut {c!r} is not a whole hundredth of theta")
        else:
            raise ValueError(f"bins: the cut {c!r} is not a number")
        if not 1 <= d <= 499:
            raise ValueError(f"bins: the cut {c!r} is outside 0.01..4.99 (1..499 hundredths)")
        out.append(d)
    if any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError("bins: the cuts must be strictly increasing")
    return tuple(out)


def check_bins_top(top) -> int:
    t = int(top)
    if t != top or not 1 <= t <= _lib.BINS_MAX_TOP:
        raise ValueError(f"bins: top must be an integer in 1..{_lib.BINS_MAX_TOP}")
    return t


def bin_of_index(k, cuts):
    """The header's rule: the bin of grid index k (0..1000) under the cuts d (ints): a = |k - 500|, l = #{t : a >= d_t},
    bin = h + l if k >= 500 else h - l."""
    k = np.asarray(k, dtype=np.int64)
    d = np.asarray(cuts, dtype=np.int64)
    l = (np.abs(k - 500)[..., None] >= d).sum(axis=-1)
    return np.where(k >= 500, len(d) + l, len(d) - l)


def bin_edges(cuts):
    """(bin_lo, bin_hi) in theta of the B = 2h + 1 bins."""
    d = [c / 100.0 for c in cuts] + [5.0]
    h = len(cuts)
    lo = [-d[h - b] for b in range(h)] + [-d[0]] + [d[l - 1] for l in range(1, h + 1)]
    hi = [-d[h - b - 1] for b in range(h)] + [d[0]] + [d[l] for l in range(1, h + 1)]
    return np.array(lo), np.array(hi)


def _bins_shape(kind, m, B):
    return {"c": (B, m), "i": (m,), "b": (B,)}[kind]


def bins_struct(m: int, cuts=DEFAULT_CUTS, top=DEFAULT_BINS_TOP):
    """A gpirt_ppc_bins with the cuts and host arrays for every output, and those arrays (kept alive by the caller)."""
    cuts = check_cuts(cuts)
    B = 2 * len(cuts) + 1
    p = _lib.PpcBins()
    p.top = check_bins_top(top)
    p.h = len(cuts)
    for q, d in enumerate(cuts):
        p.cuts[q] = d
    arr = {}
    for group, names, shape in (("cell", BINS_CELL_FIELDS, (B, m)), ("item", BINS_ITEM_FIELDS, (m,)), ("bin", BINS_BIN_FIELDS, (B,))):
        for k, name in enumerate(names):
            arr[name] = np.empty(shape)
            getattr(p, group)[k] = arr[name].ctypes.data_as(_dp)
    counts = {"cell_ge": ("cell_count", 0), "cell_gt": ("cell_count", 1), "cell_empty": ("cell_count", 2),
              "chi_ge": ("chi_count", 0), "chi_gt": ("chi_count", 1)}
    for name, dt, kind in BINS_RAW:
        arr[name] = np.empty(_bins_shape(kind, m, B), dtype=_BIN_DTYPES[dt])
        ptr = arr[name].ctypes.data_as(C.POINTER({"u8": C.c_uint64, "f8": C.c_double, "u4": C.c_uint32}[dt]))
        if name in counts:
            getattr(p, counts[name][0])[counts[name][1]] = ptr
        else:
            setattr(p, name, ptr)
    arr["worst_items"] = np.empty(p.top, dtype=np.int64)
    p.worst_items = arr["worst_items"].ctypes.data_as(C.POINTER(C.c_int64))
    for name in ("worst_ppp_chi2_mid", "worst_chi2_obs_mean"):
        arr[name] = np.empty(p.top)
        setattr(p, name, arr[name].ctypes.data_as(_dp))
    return p, arr


def bins_result(p, arr) -> dict:
    """The "bins" dict of gpirtMCMC(ppc=dict(bins=True)), Sampler.ppc_bins() and bins_combine(): every array of the header by
    name (cell (b, j) at [b, j]), "cuts", "worst" (dict: items, ppp_chi2_mid, chi2_obs_mean) and the counters."""
    out = {k: v for k, v in arr.items() if not k.startswith("worst_")}
    out["worst"] = dict(items=arr["worst_items"], ppp_chi2_mid=arr["worst_ppp_chi2_mid"], chi2_obs_mean=arr["worst_chi2_obs_mean"])
    out["cuts"] = np.array([p.cuts[q] for q in range(p.h)], dtype=np.int64)
    out.update(n=int(p.n), m=int(p.m), B=int(p.B), bin_draws=int(p.bin_draws), bin_skipped=int(p.bin_skipped))
    return out


def bins_state_header(state) -> dict:
    """The header of a theta-binned state block (a device tensor): its 8 int64 words and the cuts."""
    w = _lib.header_words(state, 24)
    B = int(w[6])
    return dict(n=int(w[0]), m=int(w[1]), version=int(w[2]), bin_draws=int(w[3]), bin_skipped=int(w[4]), item0=int(w[5]),
                B=B, tag=int(w[7]), cuts=tuple(int(x) for x in w[8:8 + max((B - 1) // 2, 0)]))


def bins_combine(handle, states, signs=None, top=DEFAULT_BINS_TOP) -> dict:
    """gpirt_ppc_bins_combine over the theta-binned state blocks `states` (device tensors, or Samplers with ppc_bins_enable()
    on, all on handle's device): the integers added, the doubles added in chain order; a chain whose sign is -1 enters with
    its bin axis reversed.  Blocks with another n, m, item0 or cuts are refused."""
    lib = _lib.load()
    tensors, nc, ptrs = _lib.state_ptrs(states, "ppc_bins_state")
    hdr = bins_state_header(tensors[0])
    if hdr["tag"] != _lib.BINS_TAG:
        raise ValueError("bins_combine: the first state is not a theta-binned PPC state block")
    p, arr = bins_struct(hdr["m"], hdr["cuts"], top)
    sg = None
    if signs is not None:
        if len(signs) != nc:
            raise ValueError("bins_combine: one sign per state")
        sg = (C.c_int * nc)(*[int(x) for x in signs])
    check(lib.gpirt_ppc_bins_combine(handle.ptr, nc, ptrs, sg, C.byref(p)))
    return bins_result(p, arr)


# ------------------------------------------------------------------------------------- theta-binned item fit: NumPy ---
_EPS = float(np.finfo(np.float64).eps)
# relative gaps between any two fp64 evaluations of the header's arithmetic (exp within 1 ulp, 1 + e and the division
# rounded once each: p and q within 4 eps of the true value, so two evaluations within 8 eps; p q within 2 * 9 + 2 eps)
BINS_P_GAP = 8.0 * _EPS
BINS_PQ_GAP = 20.0 * _EPS


def bins_bounds(N, E, V, Cs=()):
    """Bounds on how far an fp64 evaluation of a bin's E = sum p, V = sum p q (N terms, any fixed order: at most N eps of the
    sum of the positive terms) and of (C - E) / sqrt(V), (C - E)^2 / V for the counts C in Cs may lie from the values
    given: (dE, dV, [dz_C ...], [dterm_C ...]).  Derived from the precision of the format alone; first order terms with 1 %
    on top for the higher ones."""
    N = np.asarray(N, dtype=np.float64)
    E = np.asarray(E, dtype=np.float64)
    V = np.asarray(V, dtype=np.float64)
    dE = (BINS_P_GAP + N * _EPS) * E
    aV = BINS_PQ_GAP + N * _EPS
    dV = aV * V
    dz, dt = [], []
    with np.errstate(invalid="ignore", divide="ignore"):
        for Cc in Cs:
            d = np.abs(np.asarray(Cc, dtype=np.float64) - E)
            dd = dE + _EPS * d
            ok = V > 0
            z = np.where(ok, d / np.sqrt(np.where(ok, V, 1.0)), 0.0)
            term = z * z
            dz.append(np.where(ok, 1.01 * (dd / np.sqrt(np.where(ok, V, 1.0)) + z * (0.5 * aV + 2.0 * _EPS)), 0.0))
            dt.append(np.where(ok, 1.01 * ((2.0 * d * dd + dd * dd) / np.where(ok, V, 1.0) + term * (aV + 4.0 * _EPS)), 0.0))
    return dE, dV, dz, dt


def bins_from_rep(y, theta_draws, g_draws, rep_draws, cuts=DEFAULT_CUTS, top=DEFAULT_BINS_TOP, signs=None) -> dict:
    """The header's theta-binned item fit from stored draws: y (n x m; NaN = missing), theta_draws (S, n), g_draws (S, n, m)
    the draws of g = f + mu, rep_draws (S, n, m) with rep != 0 where yrep = +1 (cells where y is missing are masked out
    here).  signs: None, or one of +1 / -1 per draw (its chain's reflection sign): a draw with -1 enters with its bin axis
    reversed, as gpirt_ppc_bins_combine pools it.  A draw with a theta off the grid or a non-finite g in an observed cell is
    skipped.  Returns bins_result's dict with the integers exact and E, V, z and X2 summed in np.longdouble, and
      chi_ge, chi_gt     (lo, hi) brackets: an (item, draw) whose |X2(R) - X2(T)| is at most the sum of the two bounds of
                         bins_bounds is undecided (an integer tie R_b = T_b in every bin is decided: ge, not gt);
      "undecided", "decisions"   those cases and all (item, counted draw) cases;
      "bounds"           dict of the accumulated bounds of sum_e, sum_z, chi_obs_sum, chi_rep_sum;
      "last"             dict(bin, tN, tT, tR, tE, tV, dE, dV) of the last counted draw (None without one)."""
    cuts = check_cuts(cuts)
    top = check_bins_top(top)
    from .quantiles import grid_index
    y = np.asarray(y, dtype=np.float64)
    n, m = y.shape
    theta_draws = np.asarray(theta_draws, dtype=np.float64)
    g_draws = np.asarray(g_draws, dtype=np.float64)
    rep_draws = np.asarray(rep_draws)
    S = theta_draws.shape[0]
    assert theta_draws.shape == (S, n) and g_draws.shape == (S, n, m) and rep_draws.shape == (S, n, m)
    sg = np.ones(S, dtype=np.int64) if signs is None else np.broadcast_to(np.asarray(signs, dtype=np.int64), (S,))
    assert np.isin(sg, (1, -1)).all()
    h, B = len(cuts), 2 * len(cuts) + 1
    obs = ~np.isnan(y)
    yes = obs & (y > 0)
    ld = np.longdouble
    zi = lambda *sh: np.zeros(sh, dtype=np.int64)        # noqa: E731
    acc = dict(sum_n=zi(B, m), sum_t=zi(B, m), sum_r=zi(B, m), cell_ge=zi(B, m), cell_gt=zi(B, m), cell_empty=zi(B, m),
               occ_sum=zi(B), sum_e=np.zeros((B, m), dtype=ld), sum_z=np.zeros((B, m), dtype=ld),
               chi_obs_sum=np.zeros(m, dtype=ld), chi_rep_sum=np.zeros(m, dtype=ld))
    bnd = dict(sum_e=np.zeros((B, m)), sum_z=np.zeros((B, m)), chi_obs_sum=np.zeros(m), chi_rep_sum=np.zeros(m))
    absz = np.zeros((B, m))
    chi = dict(ge_lo=zi(m), ge_hi=zi(m), gt_lo=zi(m), gt_hi=zi(m))
    draws = skipped = undecided = 0
    last = None
    for s in range(S):
        k = grid_index(theta_draws[s])
        g = g_draws[s]
        if (k < 0).any() or not np.isfinite(g[obs]).all():
            skipped += 1
            continue
        draws += 1
        bins = bin_of_index(k, cuts)
        onehot = (bins[None, :] == np.arange(B)[:, None])            # B x n
        oh = onehot.astype(np.int64)
        rep = obs & (rep_draws[s] != 0)
        Nn, T, R = oh @ obs.astype(np.int64), oh @ yes.astype(np.int64), oh @ rep.astype(np.int64)
        gz = np.where(obs, g, 0.0)
        p, e = _plogis(gz)
        q = np.where(gz >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
        pl, vl = np.where(obs, p, 0.0).astype(ld), np.where(obs, p * q, 0.0).astype(ld)
        E = np.stack([pl[onehot[b]].sum(axis=0) for b in range(B)])
        V = np.stack([vl[onehot[b]].sum(axis=0) for b in range(B)])
        Ed, Vd = E.astype(np.float64), V.astype(np.float64)
        dE, dV, (dzT, _), (dtT, dtR) = bins_bounds(Nn, Ed, Vd, (T, R))
        live = Nn > 0
        pos = live & (V > 0)
        Vs = np.where(pos, V, ld(1))
        z = np.where(pos, (T - E) / np.sqrt(Vs), ld(0))
        tT = np.where(pos, (T - E) ** 2 / Vs, ld(0))
        tR = np.where(pos, (R - E) ** 2 / Vs, ld(0))
        x2T, x2R = tT.sum(axis=0), tR.sum(axis=0)
        bT = np.where(pos, dtT, 0.0).sum(axis=0) + B * _EPS * x2T.astype(np.float64)
        bR = np.where(pos, dtR, 0.0).sum(axis=0) + B * _EPS * x2R.astype(np.float64)
        tie = (np.where(live, R, 0) == np.where(live, T, 0)).all(axis=0)
        gap = (x2R - x2T).astype(np.float64)
        open_ = ~tie & (np.abs(gap) <= bT + bR)
        undecided += int(open_.sum())
        chi["ge_lo"] += tie | (~open_ & (gap >= 0)); chi["ge_hi"] += tie | open_ | (gap >= 0)
        chi["gt_lo"] += ~tie & ~open_ & (gap > 0); chi["gt_hi"] += ~tie & (open_ | (gap > 0))
        flip = (lambda a: a[::-1]) if sg[s] < 0 else (lambda a: a)
        acc["sum_n"] += flip(Nn); acc["sum_t"] += flip(np.where(live, T, 0)); acc["sum_r"] += flip(np.where(live, R, 0))
        acc["cell_ge"] += flip(live & (R >= T)); acc["cell_gt"] += flip(live & (R > T)); acc["cell_empty"] += flip(~live)
        acc["occ_sum"] += flip(oh.sum(axis=1))
        acc["sum_e"] += flip(np.where(live, E, ld(0))); acc["sum_z"] += flip(z)
        acc["chi_obs_sum"] += x2T; acc["chi_rep_sum"] += x2R
        bnd["sum_e"] += flip(np.where(live, dE, 0.0)); bnd["sum_z"] += flip(np.where(pos, dzT, 0.0))
        absz += flip(np.abs(z).astype(np.float64))
        bnd["chi_obs_sum"] += bT; bnd["chi_rep_sum"] += bR
        last = dict(bin=bins.astype(np.uint8), tN=Nn.astype(np.int32), tT=T.astype(np.int32), tR=R.astype(np.int32), tE=Ed, tV=Vd,
                    dE=dE, dV=dV)
    # the accumulation over the draws (and, pooled, over the chains): one rounding per addition
    f64 = {k: acc[k].astype(np.float64) for k in ("sum_e", "sum_z", "chi_obs_sum", "chi_rep_sum")}
    bnd["sum_e"] += (draws + 1) * _EPS * f64["sum_e"]
    bnd["sum_z"] += (draws + 1) * _EPS * absz
    bnd["chi_obs_sum"] += (draws + 1) * _EPS * f64["chi_obs_sum"]
    bnd["chi_rep_sum"] += (draws + 1) * _EPS * f64["chi_rep_sum"]
    out = dict(sum_n=acc["sum_n"].astype(np.uint64), sum_t=acc["sum_t"].astype(np.uint64), sum_r=acc["sum_r"].astype(np.uint64),
               cell_ge=acc["cell_ge"].astype(np.uint32), cell_gt=acc["cell_gt"].astype(np.uint32),
               cell_empty=acc["cell_empty"].astype(np.uint32), occ_sum=acc["occ_sum"].astype(np.uint64), **f64)
    out["chi_ge"] = (chi["ge_lo"], chi["ge_hi"])
    out["chi_gt"] = (chi["gt_lo"], chi["gt_hi"])
    with np.errstate(invalid="ignore", divide="ignore"):
        sN = np.where(acc["sum_n"] > 0, acc["sum_n"], np.nan).astype(np.float64)
        Sc = draws - acc["cell_empty"]
        Sc = np.where(Sc > 0, Sc, np.nan).astype(np.float64)
        Sd = float(draws) if draws > 0 else np.nan
        out["obs_rate"] = acc["sum_t"] / sN
        out["rep_rate"] = acc["sum_r"] / sN
        out["exp_rate"] = f64["sum_e"] / sN
        out["z_mean"] = f64["sum_z"] / Sc
        out["ppp_cell"] = acc["cell_ge"] / Sc
        out["ppp_cell_mid"] = (acc["cell_ge"] + acc["cell_gt"]) / (2.0 * Sc)
        out["n_mean"] = acc["sum_n"] / Sd
        # the finished chi-square fields from the brackets' lower ends (equal to the upper ones unless "undecided" > 0)
        out["ppp_chi2"] = chi["ge_lo"] / Sd
        out["ppp_chi2_mid"] = (chi["ge_lo"] + chi["gt_lo"]) / (2.0 * Sd)
        out["chi2_obs_mean"] = f64["chi_obs_sum"] / Sd
        out["chi2_rep_mean"] = f64["chi_rep_sum"] / Sd
        out["occupancy"] = acc["occ_sum"] / Sd
    out["bin_lo"], out["bin_hi"] = bin_edges(cuts)
    out["cuts"] = np.array(cuts, dtype=np.int64)
    out["worst"] = bins_worst(out["ppp_chi2_mid"], out["chi2_obs_mean"], top)
    out.update(n=n, m=m, B=B, bin_draws=draws, bin_skipped=skipped, undecided=undecided, decisions=draws * m, bounds=bnd, last=last)
    return out


def bins_worst(ppp_chi2_mid, chi2_obs_mean, top=DEFAULT_BINS_TOP) -> dict:
    """The `top` items by increasing ppp_chi2_mid, ties to the lowest j, NaN never listed; padded with -1 / NaN."""
    top = check_bins_top(top)
    mid = np.asarray(ppp_chi2_mid, dtype=np.float64)
    js = np.flatnonzero(~np.isnan(mid))
    order = js[np.argsort(mid[js], kind="stable")][:top]
    w = dict(items=np.full(top, -1, dtype=np.int64), ppp_chi2_mid=np.full(top, np.nan), chi2_obs_mean=np.full(top, np.nan))
    w["items"][:len(order)] = order
    w["ppp_chi2_mid"][:len(order)] = mid[order]
    w["chi2_obs_mean"][:len(order)] = np.asarray(chi2_obs_mean, dtype=np.float64)[order]
    return w


def bins_from_draws(y, theta_draws, g_draws, seed, iters, cuts=DEFAULT_CUTS, top=DEFAULT_BINS_TOP, item0=0, signs=None):
    """bins_from_rep over the replicates of stored draws, built as pairs_from_draws builds them: rep = [u < plogis(g)] with
    replicate_uniforms' u at the completed-iteration counters `iters`.  Returns (result, min |u - p| over the observed cells
    of the draws with finite g): a cell that close to its uniform may replicate either way under another evaluation of
    plogis."""
    y = np.asarray(y, dtype=np.float64)
    g_draws = np.asarray(g_draws, dtype=np.float64)
    n, m = y.shape
    obs = ~np.isnan(y)
    reps, gap = [], np.inf
    for s, it in enumerate(iters):
        g = g_draws[s]
        if not np.isfinite(g[obs]).all():
            reps.append(np.zeros((n, m), dtype=bool))    # (bins_from_rep skips the draw)
            continue
        p, _ = _plogis(np.where(obs, g, 0.0))
        u = replicate_uniforms(seed, int(it), n, m, item0)
        if obs.any():
            gap = min(gap, float(np.abs(u - p)[obs].min()))
        reps.append(obs & (u < p))
    rep = np.stack(reps) if reps else np.zeros((0, n, m), dtype=bool)
    return bins_from_rep(y, theta_draws, g_draws, rep, cuts, top, signs), gap


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


# ------------------------------------------------------------------------------------------ group-wise item fit (DIF) ---
# ("group-wise item fit" in the header; csrc/ppc_dif.hip) the third add-on: `check_groups`, `dif_struct` / `dif_result` wrap
# gpirt_ppc_dif, `dif_combine` pools chains' state blocks with their reflection signs, `dif_tables` / `dif_draw_stats` /
# `dif_from_tables` are the NumPy statement of the header -- integer tables, then fp64 operations in the header's order, so the
# same tables give the same bits --, `dif_from_rep` runs it over stored theta, g and replicates, `dif_from_draws` builds the
# replicates with this module's Philox.
DEFAULT_DIF_TOP = 20
DIF_FIX = 2.0 ** 44


def check_groups(groups, n: int):
    """(codes as int32 (n,), G): -1 = left out, 0 = the reference group, 1 .. G - 1 the focal groups, 2 <= G <= 4, no gap in
    the codes, no empty group; n <= 65534.  Anything else is a ValueError that says which."""
    if n > _lib.DIF_MAX_N:
        raise ValueError(f"dif: n = {n} is beyond {_lib.DIF_MAX_N} respondents")
    g = np.asarray(groups)
    if g.ndim != 1 or g.shape[0] != n:
        raise ValueError(f"dif: groups must hold one code per respondent ({n}), got shape {g.shape}")
    if g.dtype == bool or not (np.issubdtype(g.dtype, np.integer) or (np.issubdtype(g.dtype, np.floating) and np.isfinite(g).all()
                                                                       and (g == np.rint(g)).all())):
        raise ValueError("dif: the group codes must be integers")
    g = g.astype(np.int64)
    if ((g < -1) | (g >= _lib.DIF_MAX_G)).any():
        bad = g[(g < -1) | (g >= _lib.DIF_MAX_G)][0]
        raise ValueError(f"dif: the group code {int(bad)} is outside -1..{_lib.DIF_MAX_G - 1}")
    G = int(g.max()) + 1
    if G < 2:
        raise ValueError("dif: a reference group 0 and at least one focal group 1 are needed")
    for c in range(G):
        if not (g == c).any():
            raise ValueError(f"dif: group {c} has no member (the codes 0..{G - 1} must all be used)")
    return np.ascontiguousarray(g, dtype=np.int32), G


def check_dif_top(top) -> int:
    t = int(top)
    if t != top or not 1 <= t <= _lib.DIF_MAX_TOP:
        raise ValueError(f"dif: top must be an integer in 1..{_lib.DIF_MAX_TOP}")
    return t


def _dif_shape(kind, m, G, B):
    return {"c": (G, B, m), "o": (G, B), "g": (G, m)}[kind]


def dif_struct(m: int, G: int, cuts=DEFAULT_CUTS, top=DEFAULT_DIF_TOP, groups=None):
    """A gpirt_ppc_dif with the cuts (and the group codes, for gpirt_mcmc_run) and host arrays for every output, and those
    arrays (kept alive by the caller)."""
    cuts = check_cuts(cuts)
    B = 2 * len(cuts) + 1
    p = _lib.PpcDif()
    p.top = check_dif_top(top)
    p.G, p.h = int(G), len(cuts)
    for q, d in enumerate(cuts):
        p.cuts[q] = d
    arr = {}
    if groups is not None:
        arr["_groups"] = np.ascontiguousarray(groups, dtype=np.int32)
        p.groups = arr["_groups"].ctypes.data_as(C.POINTER(C.c_int32))
    for grp, names, shape in (("cell", _lib.DIF_CELL_FIELDS, (G, B, m)), ("group", _lib.DIF_GROUP_FIELDS, (G, m)),
                              ("focal", _lib.DIF_FOCAL_FIELDS, (G, m))):
        for k, name in enumerate(names):
            arr[name] = np.empty(shape)
            getattr(p, grp)[k] = arr[name].ctypes.data_as(_dp)
    arr["occupancy"] = np.empty((G, B))
    p.occupancy = arr["occupancy"].ctypes.data_as(_dp)
    for k, (name, dt, kind) in enumerate(_lib.DIF_RAW):
        arr[name] = np.empty(_dif_shape(kind, m, G, B), dtype=_BIN_DTYPES[dt])
        p.raw[k] = arr[name].ctypes.data
    for name in ("flagged_items", "flagged_groups"):
        arr[name] = np.empty(p.top, dtype=np.int64)
        setattr(p, name, arr[name].ctypes.data_as(C.POINTER(C.c_int64)))
    arr["flagged_ppp_mh_mid"] = np.empty(p.top)
    p.flagged_ppp_mh_mid = arr["flagged_ppp_mh_mid"].ctypes.data_as(_dp)
    return p, arr


def dif_result(p, arr) -> dict:
    """The "dif" dict of gpirtMCMC(ppc=dict(dif=...)), Sampler.ppc_dif() and dif_combine(): every array of the header by name
    (cell (g, b, j) at [g, b, j]; the focal arrays indexed by the group code, row 0 NaN), "cuts", "flagged" (dict: items,
    groups, ppp_mh_mid) and the counters."""
    out = {k: v for k, v in arr.items() if not k.startswith("flagged_") and not k.startswith("_")}
    out["flagged"] = dict(items=arr["flagged_items"], groups=arr["flagged_groups"], ppp_mh_mid=arr["flagged_ppp_mh_mid"])
    out["cuts"] = np.array([p.cuts[q] for q in range(p.h)], dtype=np.int64)
    out.update(n=int(p.n), m=int(p.m), B=int(p.B), G=int(p.G), dif_draws=int(p.dif_draws), dif_skipped=int(p.dif_skipped),
               group_size=np.array([p.group_size[g] for g in range(p.G)], dtype=np.int64))
    return out


def dif_state_header(state) -> dict:
    """The header of a group-wise state block (a device tensor): its 8 int64 words, the cuts, G and the groups' sizes."""
    w = _lib.header_words(state, 32)
    B, G = int(w[6]), int(w[24])
    return dict(n=int(w[0]), m=int(w[1]), version=int(w[2]), dif_draws=int(w[3]), dif_skipped=int(w[4]), item0=int(w[5]),
                B=B, tag=int(w[7]), cuts=tuple(int(x) for x in w[8:8 + max((B - 1) // 2, 0)]), G=G,
                group_size=tuple(int(x) for x in w[25:25 + max(min(G, 4), 0)]))


def dif_combine(handle, states, signs=None, top=DEFAULT_DIF_TOP) -> dict:
    """gpirt_ppc_dif_combine over the group-wise state blocks `states` (device tensors, or Samplers with ppc_dif_enable() on,
    all on handle's device): the integers added, the doubles added in chain order; a chain whose sign is -1 enters with the bin
    axis of its tables reversed.  Blocks with another n, m, item0, groups or cuts are refused."""
    lib = _lib.load()
    tensors, nc, ptrs = _lib.state_ptrs(states, "ppc_dif_state")
    hdr = dif_state_header(tensors[0])
    if hdr["tag"] != _lib.DIF_TAG or not 2 <= hdr["G"] <= _lib.DIF_MAX_G:
        raise ValueError("dif_combine: the first state is not a group-wise PPC state block")
    p, arr = dif_struct(hdr["m"], hdr["G"], hdr["cuts"], top)
    sg = None
    if signs is not None:
        if len(signs) != nc:
            raise ValueError("dif_combine: one sign per state")
        sg = (C.c_int * nc)(*[int(x) for x in signs])
    check(lib.gpirt_ppc_dif_combine(handle.ptr, nc, ptrs, sg, C.byref(p)))
    return dif_result(p, arr)


def dif_fix(x):
    """rint(x 2^44) as uint64: a term of E or V in the header's fixed point"""
    return np.rint(np.asarray(x, dtype=np.float64) * DIF_FIX).astype(np.uint64)


def dif_cells(theta, groups, cuts, B):
    """(cell (uint8, n; 255 = left out or off the grid), any theta off the grid) of one draw"""
    from .quantiles import grid_index
    k = grid_index(np.asarray(theta, dtype=np.float64))
    ok = (k >= 0) & (groups >= 0)
    cell = np.where(ok, groups.astype(np.int64) * B + bin_of_index(np.where(k >= 0, k, 500), cuts), 255).astype(np.uint8)
    return cell, bool((k < 0).any())


def dif_tables(y, cell, g, rep, GB):
    """One draw's integer tables (GB x m each): N, T, R (int64) and the fixed-point E, V (uint64), over the observed cells of
    the respondents whose cell is not 255; g must be finite there."""
    y = np.asarray(y, dtype=np.float64)
    m = y.shape[1]
    obs = ~np.isnan(y) & (cell != 255)[:, None]
    gz = np.where(obs, g, 0.0)
    p, e = _plogis(gz)
    q = np.where(gz >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
    ef, vf = np.where(obs, dif_fix(p), 0).astype(np.uint64), np.where(obs, dif_fix(p * q), 0).astype(np.uint64)
    N, T, R = (np.zeros((GB, m), dtype=np.int64) for _ in range(3))
    E, V = (np.zeros((GB, m), dtype=np.uint64) for _ in range(2))
    yes, rp = obs & (y > 0), obs & (np.asarray(rep) != 0)
    for c in np.unique(cell[cell != 255]):
        rows = cell == c
        N[c], T[c], R[c] = obs[rows].sum(axis=0), yes[rows].sum(axis=0), rp[rows].sum(axis=0)
        E[c], V[c] = ef[rows].sum(axis=0, dtype=np.uint64), vf[rows].sum(axis=0, dtype=np.uint64)
    return N, T, R, E, V


def dif_draw_stats(N, T, R, Ef, Vf, G, B) -> dict:
    """The header's statistics of one draw from its tables (G B x m, or G x B x m): fp64 conversions, products, divisions and
    additions in the header's order, the sums in increasing b.  Returns "stats" (8 x G x m: num(T), den(T), num(R), den(R),
    STD(T), STD(R), X2(T), X2(R); NaN as the device leaves it), the bool decisions yes_ge, yes_gt, chi_ge, chi_gt (G x m),
    mh_def, mh_ge, mh_gt, std_def (G x m, row 0 False) and log_obs, log_rep (G x m, 0 where undefined)."""
    m = np.asarray(N).shape[-1]
    N, T, R = (np.asarray(a, dtype=np.int64).reshape(G, B, m) for a in (N, T, R))
    E = np.asarray(Ef, dtype=np.uint64).reshape(G, B, m).astype(np.float64) * (1.0 / DIF_FIX)
    V = np.asarray(Vf, dtype=np.uint64).reshape(G, B, m).astype(np.float64) * (1.0 / DIF_FIX)

    def serial(terms):                                   # (..., B, m) -> (..., m): 0.0 + t_0 + t_1 + ... in increasing b
        s = np.zeros(terms.shape[:-2] + (m,))
        for b in range(B):
            s = s + terms[..., b, :]
        return s

    with np.errstate(invalid="ignore", divide="ignore"):
        pos = (N > 0) & (V > 0.0)
        Vs = np.where(pos, V, 1.0)
        dT, dR = T.astype(np.float64) - E, R.astype(np.float64) - E
        x2T = serial(np.where(pos, dT * dT / Vs, 0.0))
        x2R = serial(np.where(pos, dR * dR / Vs, 0.0))
        Rg, Tg = R.sum(axis=1), T.sum(axis=1)
        tie = (R == T).all(axis=1)
        out = dict(yes_ge=Rg >= Tg, yes_gt=Rg > Tg, chi_ge=tie | (x2R >= x2T), chi_gt=~tie & (x2R > x2T))
        stats = np.full((8, G, m), np.nan)
        stats[6], stats[7] = x2T, x2R
        z = lambda: np.zeros((G, m), dtype=bool)         # noqa: E731
        out.update(mh_def=z(), mh_ge=z(), mh_gt=z(), std_def=z(), log_obs=np.zeros((G, m)), log_rep=np.zeros((G, m)))
        for f in range(1, G):
            common = (N[0] > 0) & (N[f] > 0)
            nb = np.where(common, N[0] + N[f], 1).astype(np.float64)
            n0, nf = np.where(common, N[0], 1).astype(np.float64), np.where(common, N[f], 1).astype(np.float64)
            sums = []
            for Cc in (T, R):
                num = serial(np.where(common, (Cc[0] * (N[f] - Cc[f])).astype(np.float64) / nb, 0.0))
                den = serial(np.where(common, ((N[0] - Cc[0]) * Cc[f]).astype(np.float64) / nb, 0.0))
                sd = serial(np.where(common, nf * (Cc[f].astype(np.float64) / nf - Cc[0].astype(np.float64) / n0), 0.0))
                sums.append((num, den, sd))
            nsum = serial(np.where(common, nf, 0.0))
            (numT, denT, sT), (numR, denR, sR) = sums
            stats[0, f], stats[1, f], stats[2, f], stats[3, f] = numT, denT, numR, denR
            ok = (numT != 0) & (denT != 0) & (numR != 0) & (denR != 0)
            lhs, rhs = numR * denT, numT * denR
            out["mh_def"][f], out["mh_ge"][f], out["mh_gt"][f] = ok, ok & (lhs >= rhs), ok & (lhs > rhs)
            out["log_obs"][f] = np.where(ok, np.log(np.where(ok, numT / np.where(ok, denT, 1.0), 1.0)), 0.0)
            out["log_rep"][f] = np.where(ok, np.log(np.where(ok, numR / np.where(ok, denR, 1.0), 1.0)), 0.0)
            sok = nsum > 0
            out["std_def"][f] = sok
            stats[4, f] = np.where(sok, sT / np.where(sok, nsum, 1.0), np.nan)
            stats[5, f] = np.where(sok, sR / np.where(sok, nsum, 1.0), np.nan)
    out["stats"] = stats
    return out


def dif_flagged(ppp_mh_mid, top=DEFAULT_DIF_TOP) -> dict:
    """The `top` (focal group, item) pairs by decreasing |ppp_mh_mid - 0.5|, ties to the lowest (group, item), NaN never
    listed; padded with -1 / NaN."""
    top = check_dif_top(top)
    mid = np.asarray(ppp_mh_mid, dtype=np.float64)
    G, m = mid.shape
    flat = mid[1:].ravel()
    at = np.flatnonzero(~np.isnan(flat))
    order = at[np.argsort(-np.abs(flat[at] - 0.5), kind="stable")][:top]
    w = dict(items=np.full(top, -1, dtype=np.int64), groups=np.full(top, -1, dtype=np.int64), ppp_mh_mid=np.full(top, np.nan))
    w["items"][:len(order)] = order % m
    w["groups"][:len(order)] = order // m + 1
    w["ppp_mh_mid"][:len(order)] = flat[order]
    return w


def dif_from_tables(draws, G, B, m, top=DEFAULT_DIF_TOP, signs=None, skipped=0, group_size=None) -> dict:
    """The header's accumulators and finished fields from the COUNTED draws' tables: draws = a list of dicts with N, T, R, E, V
    (G B x m; E and V the fixed-point uint64) and occ (G B members per cell).  signs: None, or +1 / -1 per draw: a draw with -1
    enters the (group, bin, item) tables and occ_sum with its bin axis reversed; its counters and per-draw sums stay.  Returns
    dif_result's dict; "log_terms" (G x m) counts the log terms behind mh_log_*_sum, for a bound on them."""
    S = len(draws)
    sg = np.ones(S, dtype=np.int64) if signs is None else np.broadcast_to(np.asarray(signs, dtype=np.int64), (S,))
    zi = lambda *sh: np.zeros(sh, dtype=np.int64)        # noqa: E731
    acc = dict(sum_n=zi(G, B, m), sum_t=zi(G, B, m), sum_r=zi(G, B, m), sum_e=np.zeros((G, B, m)), occ_sum=zi(G, B))
    for k in ("yes_ge", "yes_gt", "chi_ge", "chi_gt", "mh_ge", "mh_gt", "mh_undefined_count", "std_undefined_count"):
        acc[k] = zi(G, m)
    for k in ("chi_obs_sum", "chi_rep_sum", "mh_log_obs_sum", "mh_log_rep_sum", "std_obs_sum", "std_rep_sum"):
        acc[k] = np.zeros((G, m))
    focal = np.arange(G)[:, None] > 0
    last = None
    for s, d in enumerate(draws):
        st = dif_draw_stats(d["N"], d["T"], d["R"], d["E"], d["V"], G, B)
        flip = (lambda a: a[:, ::-1]) if sg[s] < 0 else (lambda a: a)
        r3 = lambda a, dt: np.asarray(a).reshape(G, B, m).astype(dt)      # noqa: E731
        acc["sum_n"] += flip(r3(d["N"], np.int64)); acc["sum_t"] += flip(r3(d["T"], np.int64)); acc["sum_r"] += flip(r3(d["R"], np.int64))
        acc["sum_e"] = acc["sum_e"] + flip(r3(d["E"], np.uint64).astype(np.float64) * (1.0 / DIF_FIX))
        acc["occ_sum"] += flip(np.asarray(d["occ"], dtype=np.int64).reshape(G, B))
        for k in ("yes_ge", "yes_gt", "chi_ge", "chi_gt", "mh_ge", "mh_gt"):
            acc[k] += st[k]
        acc["mh_undefined_count"] += focal & ~st["mh_def"]
        acc["std_undefined_count"] += focal & ~st["std_def"]
        acc["chi_obs_sum"] = acc["chi_obs_sum"] + st["stats"][6]
        acc["chi_rep_sum"] = acc["chi_rep_sum"] + st["stats"][7]
        acc["mh_log_obs_sum"] = acc["mh_log_obs_sum"] + st["log_obs"]
        acc["mh_log_rep_sum"] = acc["mh_log_rep_sum"] + st["log_rep"]
        acc["std_obs_sum"] = acc["std_obs_sum"] + np.where(st["std_def"], st["stats"][4], 0.0)
        acc["std_rep_sum"] = acc["std_rep_sum"] + np.where(st["std_def"], st["stats"][5], 0.0)
        last = dict(tN=r3(d["N"], np.int32), tT=r3(d["T"], np.int32), tR=r3(d["R"], np.int32), tE=r3(d["E"], np.uint64),
                    tV=r3(d["V"], np.uint64), stats=st["stats"], cell=d.get("cell"))
    dts = {name: _BIN_DTYPES[dt] for name, dt, _ in _lib.DIF_RAW}
    out = {k: v.astype(dts[k]) for k, v in acc.items()}
    with np.errstate(invalid="ignore", divide="ignore"):
        sN = np.where(acc["sum_n"] > 0, acc["sum_n"], np.nan).astype(np.float64)
        Sd = float(S) if S > 0 else np.nan
        out["obs_rate"], out["rep_rate"], out["exp_rate"] = acc["sum_t"] / sN, acc["sum_r"] / sN, acc["sum_e"] / sN
        out["occupancy"] = acc["occ_sum"] / Sd
        out["ppp_yes"], out["ppp_yes_mid"] = acc["yes_ge"] / Sd, (acc["yes_ge"] + acc["yes_gt"]) / (2.0 * Sd)
        out["ppp_chi2"], out["ppp_chi2_mid"] = acc["chi_ge"] / Sd, (acc["chi_ge"] + acc["chi_gt"]) / (2.0 * Sd)
        out["chi2_obs_mean"], out["chi2_rep_mean"] = acc["chi_obs_sum"] / Sd, acc["chi_rep_sum"] / Sd
        Sm = S - acc["mh_undefined_count"]
        Sm = np.where(focal & (Sm > 0), Sm, np.nan).astype(np.float64)
        Ss = S - acc["std_undefined_count"]
        Ss = np.where(focal & (Ss > 0), Ss, np.nan).astype(np.float64)
        rows = np.where(focal, 1.0, np.nan)
        out["mh_log_or_obs_mean"], out["mh_log_or_rep_mean"] = acc["mh_log_obs_sum"] / Sm, acc["mh_log_rep_sum"] / Sm
        out["mh_delta_obs_mean"] = -2.35 * out["mh_log_or_obs_mean"]
        out["ppp_mh"], out["ppp_mh_mid"] = acc["mh_ge"] / Sm, (acc["mh_ge"] + acc["mh_gt"]) / (2.0 * Sm)
        out["mh_undefined"], out["std_undefined"] = acc["mh_undefined_count"] * rows, acc["std_undefined_count"] * rows
        out["std_obs_mean"], out["std_rep_mean"] = acc["std_obs_sum"] / Ss, acc["std_rep_sum"] / Ss
    out["flagged"] = dif_flagged(out["ppp_mh_mid"], top)
    out["log_terms"] = np.where(focal, S - acc["mh_undefined_count"], 0)
    out.update(n=None, m=m, B=B, G=G, dif_draws=S, dif_skipped=int(skipped), last=last,
               group_size=None if group_size is None else np.asarray(group_size, dtype=np.int64))
    return out


def dif_from_rep(y, theta_draws, g_draws, rep_draws, groups, cuts=DEFAULT_CUTS, top=DEFAULT_DIF_TOP, signs=None) -> dict:
    """The header's group-wise item fit from stored draws: y (n x m; NaN = missing), theta_draws (S, n), g_draws (S, n, m) the
    draws of g = f + mu, rep_draws (S, n, m) with rep != 0 where yrep = +1, groups (n codes), signs as in dif_from_tables (one
    per draw).  A draw with a theta off the grid, or a non-finite g in an observed cell of a grouped respondent, is skipped.
    Returns dif_from_tables' dict, "cuts" and "n" filled in."""
    cuts = check_cuts(cuts)
    y = np.asarray(y, dtype=np.float64)
    n, m = y.shape
    groups, G = check_groups(groups, n)
    theta_draws = np.asarray(theta_draws, dtype=np.float64)
    g_draws = np.asarray(g_draws, dtype=np.float64)
    S = theta_draws.shape[0]
    assert theta_draws.shape == (S, n) and g_draws.shape == (S, n, m) and np.asarray(rep_draws).shape == (S, n, m)
    sg = np.ones(S, dtype=np.int64) if signs is None else np.broadcast_to(np.asarray(signs, dtype=np.int64), (S,))
    B = 2 * len(cuts) + 1
    obs = ~np.isnan(y) & (groups >= 0)[:, None]
    draws, keep_sg, skipped = [], [], 0
    for s in range(S):
        cell, off = dif_cells(theta_draws[s], groups, cuts, B)
        if off or not np.isfinite(g_draws[s][obs]).all():
            skipped += 1
            continue
        N, T, R, E, V = dif_tables(y, cell, g_draws[s], rep_draws[s], G * B)
        draws.append(dict(N=N, T=T, R=R, E=E, V=V, occ=np.bincount(cell[cell != 255], minlength=G * B), cell=cell))
        keep_sg.append(sg[s])
    out = dif_from_tables(draws, G, B, m, top, keep_sg if draws else None, skipped,
                          [int((groups == c).sum()) for c in range(G)])
    out["n"], out["cuts"] = n, np.array(cuts, dtype=np.int64)
    return out


def dif_from_draws(y, theta_draws, g_draws, seed, iters, groups, cuts=DEFAULT_CUTS, top=DEFAULT_DIF_TOP, item0=0, signs=None):
    """dif_from_rep over the replicates of stored draws, built as bins_from_draws builds them: rep = [u < plogis(g)] with
    replicate_uniforms' u at the completed-iteration counters `iters`.  Returns (result, min |u - p| over the observed cells
    of the draws with finite g): a cell that close to its uniform may replicate either way under another evaluation of
    plogis."""
    y = np.asarray(y, dtype=np.float64)
    g_draws = np.asarray(g_draws, dtype=np.float64)
    n, m = y.shape
    obs = ~np.isnan(y)
    reps, gap = [], np.inf
    for s, it in enumerate(iters):
        with np.errstate(invalid="ignore"):
            gz = np.where(obs & np.isfinite(g_draws[s]), g_draws[s], 0.0)
        p, _ = _plogis(gz)
        u = replicate_uniforms(seed, int(it), n, m, item0)
        fin = obs & np.isfinite(g_draws[s])
        if fin.any():
            gap = min(gap, float(np.abs(u - p)[fin].min()))
        reps.append(obs & (u < p))
    rep = np.stack(reps) if reps else np.zeros((0, n, m), dtype=bool)
    return dif_from_rep(y, theta_draws, g_draws, rep, groups, cuts, top, signs), gap


# ------------------------------------------------------------------------------------------------ score-based checks ---
# ("score-based PPC" in the header; csrc/ppc_scores.hip) the fourth add-on, on the MANIFEST score: `check_score_cuts` /
# `default_score_cuts`, `scores_struct` / `scores_result` wrap gpirt_ppc_scores, `scores_combine` pools chains' state blocks,
# `scores_observed` / `scores_tables` / `scores_draw_stats` / `scores_from_tables` are the NumPy statement of the header --
# integer tables, then fp64 operations in the header's order, so the same tables give the same bits --, `scores_from_rep` runs it
# over stored g and replicates, `scores_from_draws` builds the replicates with this module's Philox.
DEFAULT_SCORES_TOP = 20
DEFAULT_SCORE_GROUPS = 9
SCORES_FIX = 2.0 ** 44
_SC_DTYPES = {"u8": np.uint64, "f8": np.float64, "u4": np.uint32, "i8": np.int64, "i4": np.int32}


def check_scores_top(top) -> int:
    t = int(top)
    if t != top or not 1 <= t <= _lib.SCORES_MAX_TOP:
        raise ValueError(f"scores: top must be an integer in 1..{_lib.SCORES_MAX_TOP}")
    return t


def check_score_cuts(cuts, m: int, n: int = 1) -> tuple:
    """The cuts as a tuple of ints: ascending c_1 < ... < c_{K-1} in 1 .. m - 1, 2 <= K <= 16 groups; 2 <= m <= 4096 items and
    n <= 65534 respondents.  Anything else is a ValueError that says which."""
    if not 2 <= int(m) <= _lib.SCORES_MAX_M:
        raise ValueError(f"scores: m = {m} is outside 2..{_lib.SCORES_MAX_M} items")
    if n > _lib.SCORES_MAX_N:
        raise ValueError(f"scores: n = {n} is beyond {_lib.SCORES_MAX_N} respondents")
    try:
        c = tuple(int(x) for x in cuts)
        whole = all(float(a) == float(b) for a, b in zip(c, cuts))
    except (TypeError, ValueError):
        raise ValueError("scores: the cuts must be a sequence of integers") from None
    if not whole:
        raise ValueError("scores: the cuts must be integers")
    if not 2 <= len(c) + 1 <= _lib.SCORES_MAX_K:
        raise ValueError(f"scores: {len(c)} cuts make {len(c) + 1} score groups, 2..{_lib.SCORES_MAX_K} groups are taken")
    if any(not 1 <= x <= m - 1 for x in c) or any(b <= a for a, b in zip(c, c[1:])):
        raise ValueError(f"scores: the cuts must be increasing integers in 1..{m - 1}, got {c}")
    return c


def default_score_cuts(y, groups: int = DEFAULT_SCORE_GROUPS) -> tuple:
    """Up to `groups` score groups from the quantiles of the data's total scores (raw counts over each respondent's own observed
    items, the respondents without an observed cell left out): the sorted scores at the positions k n_s // groups, k = 1 ..
    groups - 1, those outside 1 .. m - 1 and duplicates dropped.  Fewer than two groups is a ValueError that says so."""
    y = np.asarray(y, dtype=np.float64)
    g = int(groups)
    if g != groups or not 2 <= g <= _lib.SCORES_MAX_K:
        raise ValueError(f"scores: groups must be an integer in 2..{_lib.SCORES_MAX_K}")
    ob = ~np.isnan(y)
    x = np.sort((ob & (y > 0)).sum(axis=1)[ob.any(axis=1)])
    m = y.shape[1]
    c = sorted({int(x[k * len(x) // g]) for k in range(1, g)} & set(range(1, m))) if len(x) else []
    if not c:
        raise ValueError("scores: the data's total scores give fewer than two score groups (no quantile lies in 1 .. m - 1); "
                         "pass cuts")
    return tuple(c)


def _scores_shape(kind, n, m, K):
    return {"h": (m + 1,), "s": (4, m), "v": (2,), "1": (1,), "i": (m,), "c": (K, m), "n": (n,), "x": (2, m)}[kind]


def scores_field(name: str, n: int, m: int, K: int):
    """(shape, dtype) of the array gpirt_sampler_ppc_scores_get copies for `name`: a finished field (SCORES_HIST_FIELDS: m + 1;
    SCORES_VAR_FIELDS: 0-d; SCORES_ITEM_FIELDS: m; SCORES_CELL_FIELDS: K x m), a raw array or constant of SCORES_RAW, group_lo,
    group_hi, cuts, counts, x_obs or an array of SCORES_LAST.  An unknown name is a ValueError that says so."""
    named = {r[0]: r for r in _lib.SCORES_RAW + _lib.SCORES_LAST}
    fixed = {"counts": ((2,), np.int64), "cuts": ((K - 1,), np.int64), "group_lo": ((K,), np.int64), "group_hi": ((K,), np.int64),
             "x_obs": ((n,), np.int32)}
    if name in fixed:
        return fixed[name]
    if name in named:
        _, dt, kind = named[name]
        return _scores_shape(kind, n, m, K), _SC_DTYPES[dt]
    for names, shape in ((_lib.SCORES_HIST_FIELDS, (m + 1,)), (_lib.SCORES_VAR_FIELDS, ()), (_lib.SCORES_ITEM_FIELDS, (m,)),
                         (_lib.SCORES_CELL_FIELDS, (K, m))):
        if name in names:
            return shape, np.float64
    raise ValueError(f"scores: unknown field {name!r}")


def scores_struct(m: int, K: int, top=DEFAULT_SCORES_TOP):
    """A gpirt_ppc_scores with host arrays for every output, and those arrays (kept alive by the caller)."""
    p = _lib.PpcScores()
    p.top = check_scores_top(top)
    arr = {}
    for grp, names, shape in (("hist", _lib.SCORES_HIST_FIELDS, (m + 1,)), ("item", _lib.SCORES_ITEM_FIELDS, (m,)),
                              ("cell", _lib.SCORES_CELL_FIELDS, (K, m))):
        for k, name in enumerate(names):
            arr[name] = np.empty(shape)
            getattr(p, grp)[k] = arr[name].ctypes.data_as(_dp)
    arr["_var"] = np.empty(3)
    p.var = arr["_var"].ctypes.data_as(_dp)
    for k, (name, dt, kind) in enumerate(_lib.SCORES_RAW):
        arr[name] = np.empty(_scores_shape(kind, 0, m, K), dtype=_SC_DTYPES[dt])
        p.raw[k] = arr[name].ctypes.data
    for name in ("group_lo", "group_hi"):
        arr[name] = np.empty(K, dtype=np.int64)
        setattr(p, name, arr[name].ctypes.data_as(C.POINTER(C.c_int64)))
    arr["worst_items"] = np.empty(p.top, dtype=np.int64)
    p.worst_items = arr["worst_items"].ctypes.data_as(C.POINTER(C.c_int64))
    arr["worst_ppp_chi2_mid"] = np.empty(p.top)
    p.worst_ppp_chi2_mid = arr["worst_ppp_chi2_mid"].ctypes.data_as(_dp)
    return p, arr


def scores_result(p, arr) -> dict:
    """The dict of Sampler.ppc_scores() and scores_combine(): every array of the header by name (cell (k, j) at [k, j]), the
    three values of the spread as floats, "cuts", "worst" (dict: items, ppp_chi2_mid) and the counters."""
    out = {k: v for k, v in arr.items() if not k.startswith("worst_") and not k.startswith("_")}
    for k, name in enumerate(_lib.SCORES_VAR_FIELDS):
        out[name] = float(arr["_var"][k])
    out["worst"] = dict(items=arr["worst_items"], ppp_chi2_mid=arr["worst_ppp_chi2_mid"])
    out["cuts"] = np.array([p.cuts[q] for q in range(p.K - 1)], dtype=np.int64)
    out.update(n=int(p.n), m=int(p.m), K=int(p.K), score_draws=int(p.score_draws), score_skipped=int(p.score_skipped),
               n_scored=int(p.n_scored))
    return out


def scores_state_header(state) -> dict:
    """The header of a score-based state block (a device tensor): its 8 int64 words and the cuts."""
    w = _lib.header_words(state, 24)
    K = int(w[4])
    return dict(tag=int(w[0]), version=int(w[1]), n=int(w[2]), m=int(w[3]), K=K, score_draws=int(w[5]), score_skipped=int(w[6]),
                cuts=tuple(int(x) for x in w[8:8 + max(min(K, 16) - 1, 0)]))


def scores_combine(handle, states, top=DEFAULT_SCORES_TOP) -> dict:
    """gpirt_ppc_scores_combine over the score-based state blocks `states` (device tensors, or Samplers with ppc_scores_enable()
    on, all on handle's device): the integers added, the doubles added in chain order; no signs (theta -> -theta leaves f + mu
    as it is).  Blocks with another n, m, K, cuts or response matrix are refused."""
    lib = _lib.load()
    tensors, nc, ptrs = _lib.state_ptrs(states, "ppc_scores_state")
    hdr = scores_state_header(tensors[0])
    if hdr["tag"] != _lib.SCORES_TAG or not 2 <= hdr["K"] <= _lib.SCORES_MAX_K or not 2 <= hdr["m"] <= _lib.SCORES_MAX_M:
        raise ValueError("scores_combine: the first state is not a score-based PPC state block")
    p, arr = scores_struct(hdr["m"], hdr["K"], top)
    check(lib.gpirt_ppc_scores_combine(handle.ptr, nc, ptrs, C.byref(p)))
    return scores_result(p, arr)


def _score_r(N, sums):
    """r = (double)NUM / sqrt((double)VA (double)VC) per item from the integer sums (4 x m: A, B, Cq, D); NaN when VA or VC is 0"""
    N = np.asarray(N, dtype=np.int64)
    A, B, Cq, D = (np.asarray(a, dtype=np.int64) for a in sums)
    NUM, VA, VC = N * D - A * B, N * A - A * A, N * Cq - B * B
    ok = (VA != 0) & (VC != 0)
    den = np.sqrt(np.where(ok, VA, 1).astype(np.float64) * np.where(ok, VC, 1).astype(np.float64))
    return np.where(ok, NUM.astype(np.float64) / den, np.nan)


def _score_group(w, cuts):
    """the group of a rest score: #{k : c_k <= w}"""
    return np.searchsorted(np.asarray(cuts, dtype=np.int64), w, side="right")


def _score_sums(ob, bit, x):
    """(sums (4 x m int64: A, B, Cq, D), the rest scores n x m) of the plane `bit` with the scores x, over the cells ob"""
    W = x.astype(np.int64)[:, None] - bit.astype(np.int64)
    Wo = np.where(ob, W, 0)
    return np.stack([bit.sum(axis=0), Wo.sum(axis=0), (Wo * Wo).sum(axis=0), np.where(bit, Wo, 0).sum(axis=0)]).astype(np.int64), W


def _score_by_group(grp, ob, K, *terms):
    """per term the K x m sums over the cells ob of group k"""
    out = [np.zeros((K, ob.shape[1]), dtype=np.int64) for _ in terms]
    for k in range(K):
        mask = ob & (grp == k)
        for o, t in zip(out, terms):
            o[k] = np.where(mask, t, 0).sum(axis=0)
    return out


def _score_moments(hist):
    """(Vn = n_s S2 - S1^2, n_s) of a histogram of scores, as Python ints"""
    h = [int(v) for v in hist]
    ns, s1, s2 = sum(h), sum(s * v for s, v in enumerate(h)), sum(s * s * v for s, v in enumerate(h))
    return ns * s2 - s1 * s1, ns


def scores_observed(y, cuts) -> dict:
    """The constants of the header from the data: x (int32, n), live (the respondents with an observed cell), hist (m + 1),
    sums (4 x m: A, B, Cq, D), n_item, No, T (K x m), var = (Vn, n_s), r (NaN where undefined), with cuts, K, n, m."""
    y = np.asarray(y, dtype=np.float64)
    n, m = y.shape
    cuts = check_score_cuts(cuts, m, n)
    K = len(cuts) + 1
    ob = ~np.isnan(y)
    Y = ob & (y > 0)
    x, live = Y.sum(axis=1), ob.any(axis=1)
    hist = np.bincount(x[live], minlength=m + 1).astype(np.int64)
    sums, W = _score_sums(ob, Y, x)
    No, T = _score_by_group(_score_group(W, cuts), ob, K, 1, Y)
    n_item = ob.sum(axis=0).astype(np.int64)
    return dict(cuts=cuts, K=K, n=n, m=m, x=x.astype(np.int32), live=live, hist=hist, sums=sums, n_item=n_item, No=No, T=T,
                var=_score_moments(hist), r=_score_r(n_item, sums), W=W)


def scores_observed_from_arrays(cuts, hist_obs, sums_obs, tNo, tT, x_obs=None) -> dict:
    """scores_observed's dict from the constants of a state block (gpirt_sampler_ppc_scores_get): what scores_draw_stats and
    scores_from_tables read of it."""
    tNo, tT = np.asarray(tNo, dtype=np.int64), np.asarray(tT, dtype=np.int64)
    K, m = tNo.shape
    hist = np.asarray(hist_obs, dtype=np.int64)
    sums = np.asarray(sums_obs, dtype=np.int64).reshape(4, m)
    n_item = tNo.sum(axis=0)
    return dict(cuts=tuple(int(c) for c in cuts), K=K, n=None if x_obs is None else len(x_obs), m=m, x=x_obs, hist=hist, sums=sums,
                n_item=n_item, No=tNo, T=tT, var=_score_moments(hist), r=_score_r(n_item, sums))


def scores_tables(y, g, rep, obs) -> dict:
    """One draw's integer tables: xr (int32, n), hist (m + 1), sums (4 x m), Nr, R (K x m) and the fixed-point Eo, Vo, Er, Vr
    (int64, K x m), with "obs" = scores_observed's dict; g must be finite in the observed cells."""
    y = np.asarray(y, dtype=np.float64)
    m, K, cuts = obs["m"], obs["K"], obs["cuts"]
    ob = ~np.isnan(y)
    bit = ob & (np.asarray(rep) != 0)
    xr = bit.sum(axis=1)
    hist = np.bincount(xr[obs["live"]], minlength=m + 1).astype(np.int64)
    sums, Wr = _score_sums(ob, bit, xr)
    gz = np.where(ob, g, 0.0)
    p, e = _plogis(gz)
    q = np.where(gz >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
    ef, vf = np.rint(p * SCORES_FIX).astype(np.int64), np.rint(p * q * SCORES_FIX).astype(np.int64)
    Nr, R, Er, Vr = _score_by_group(_score_group(Wr, cuts), ob, K, 1, bit, ef, vf)
    Eo, Vo = _score_by_group(_score_group(obs["W"], cuts), ob, K, ef, vf)
    return dict(obs=obs, xr=xr.astype(np.int32), hist=hist, sums=sums, Nr=Nr, R=R, Eo=Eo, Vo=Vo, Er=Er, Vr=Vr)


def _score_x2(Cn, E, V):
    """X2 = sum over k ascending with V > 0 of d d / v, d = (double)(C 2^44 - E) 2^-44, v = (double)V 2^-44"""
    K, m = np.asarray(V).shape
    x = np.zeros(m)
    un = 1.0 / SCORES_FIX
    for k in range(K):
        pos = np.asarray(V[k]) > 0
        d = ((np.asarray(Cn[k], dtype=np.int64) << 44) - np.asarray(E[k], dtype=np.int64)).astype(np.float64) * un
        v = np.where(pos, np.asarray(V[k], dtype=np.int64).astype(np.float64) * un, 1.0)
        x = x + np.where(pos, d * d / v, 0.0)
    return x


def scores_draw_stats(tables) -> dict:
    """The header's statistics and decisions of one draw from its tables (scores_tables' dict, or the same arrays read from the
    device): r (m; NaN where VA or VC is 0), chi (2 x m: X2(T), X2(R)), Vn, and the bool decisions hist_ge, hist_gt, cdf_ge,
    cdf_gt (m + 1), var_ge, var_gt, r_def, r_ge, r_gt, chi_ge, chi_gt (m), cell_ge, cell_gt, cell_empty (K x m)."""
    obs = tables["obs"]
    r, r0 = _score_r(obs["n_item"], tables["sums"]), obs["r"]
    with np.errstate(invalid="ignore"):
        r_def = ~np.isnan(r) & ~np.isnan(r0)
        out = dict(r=r, r_def=r_def, r_ge=r_def & (r >= r0), r_gt=r_def & (r > r0))
    No, T = np.asarray(obs["No"], dtype=np.int64), np.asarray(obs["T"], dtype=np.int64)
    Nr, R = np.asarray(tables["Nr"], dtype=np.int64), np.asarray(tables["R"], dtype=np.int64)
    both = (Nr > 0) & (No > 0)
    out.update(cell_ge=both & (R * No >= T * Nr), cell_gt=both & (R * No > T * Nr), cell_empty=~both)
    x2T, x2R = _score_x2(T, tables["Eo"], tables["Vo"]), _score_x2(R, tables["Er"], tables["Vr"])
    out.update(chi=np.stack([x2T, x2R]), chi_ge=x2R >= x2T, chi_gt=x2R > x2T)
    H, Ho = np.asarray(tables["hist"], dtype=np.int64), np.asarray(obs["hist"], dtype=np.int64)
    out.update(hist_ge=H >= Ho, hist_gt=H > Ho, cdf_ge=np.cumsum(H) >= np.cumsum(Ho), cdf_gt=np.cumsum(H) > np.cumsum(Ho))
    Vn, _ = _score_moments(H)
    out.update(Vn=Vn, var_ge=Vn >= obs["var"][0], var_gt=Vn > obs["var"][0])
    return out


def scores_worst(ppp_chi2_mid, top=DEFAULT_SCORES_TOP) -> dict:
    """The `top` items with the smallest ppp_chi2_mid, ties to the lowest j, NaN never listed; padded with -1 / NaN."""
    top = check_scores_top(top)
    mid = np.asarray(ppp_chi2_mid, dtype=np.float64)
    at = np.flatnonzero(~np.isnan(mid))
    order = at[np.argsort(mid[at], kind="stable")][:top]
    w = dict(items=np.full(top, -1, dtype=np.int64), ppp_chi2_mid=np.full(top, np.nan))
    w["items"][:len(order)] = order
    w["ppp_chi2_mid"][:len(order)] = mid[order]
    return w


def scores_from_tables(draws, top=DEFAULT_SCORES_TOP, skipped=0, obs=None) -> dict:
    """The header's accumulators and finished fields from the COUNTED draws' tables (a list of scores_tables' dicts, in draw
    order; obs: the constants, needed only when the list is empty).  Returns scores_result's dict and "last" (the last draw's
    arrays under the getter's names)."""
    S = len(draws)
    obs = draws[0]["obs"] if draws else obs
    m, K = obs["m"], obs["K"]
    kinds = {name: (dt, kind) for name, dt, kind in _lib.SCORES_RAW}
    acc = {name: np.zeros(_scores_shape(kind, 0, m, K), dtype=np.float64 if dt == "f8" else object)
           for name, (dt, kind) in kinds.items() if (name, dt, kind) not in _lib.SCORES_CONST}
    un = 1.0 / SCORES_FIX
    last = None
    for d in draws:
        st = scores_draw_stats(d)
        H = np.array([int(v) for v in d["hist"]], dtype=object)
        acc["hist_sum"] += H; acc["hist_sumsq"] += H * H
        for k in ("hist_ge", "hist_gt", "cdf_ge", "cdf_gt", "r_ge", "r_gt", "cell_ge", "cell_gt", "cell_empty", "chi_ge", "chi_gt"):
            acc[k] += st[k].astype(np.int64)
        acc["var_ge"] += int(st["var_ge"]); acc["var_gt"] += int(st["var_gt"]); acc["var_rep_sum"] += st["Vn"]
        acc["r_undefined_count"] += (~st["r_def"]).astype(np.int64)
        rz = np.where(st["r_def"], st["r"], 0.0)
        acc["r_rep_sum"] = acc["r_rep_sum"] + rz
        acc["r_rep_sumsq"] = acc["r_rep_sumsq"] + rz * rz
        acc["sum_nr"] += np.asarray(d["Nr"], dtype=np.int64); acc["sum_r"] += np.asarray(d["R"], dtype=np.int64)
        acc["sum_eo"] = acc["sum_eo"] + np.asarray(d["Eo"], dtype=np.int64).astype(np.float64) * un
        acc["sum_er"] = acc["sum_er"] + np.asarray(d["Er"], dtype=np.int64).astype(np.float64) * un
        acc["chi_obs_sum"] = acc["chi_obs_sum"] + st["chi"][0]
        acc["chi_rep_sum"] = acc["chi_rep_sum"] + st["chi"][1]
        last = dict(xr=d.get("xr"), hist=np.asarray(d["hist"], dtype=np.int64), sums=np.asarray(d["sums"], dtype=np.int64), r=st["r"],
                    tNr=np.asarray(d["Nr"], dtype=np.uint32), tR=np.asarray(d["R"], dtype=np.uint32),
                    tEo=np.asarray(d["Eo"], dtype=np.int64), tVo=np.asarray(d["Vo"], dtype=np.int64),
                    tEr=np.asarray(d["Er"], dtype=np.int64), tVr=np.asarray(d["Vr"], dtype=np.int64), chi=st["chi"])
    ints = {k: np.array([int(v) for v in np.ravel(a)], dtype=object).reshape(np.shape(a)) for k, a in acc.items() if a.dtype == object}
    out = {k: (ints[k].astype(_SC_DTYPES[kinds[k][0]]) if k in ints else a) for k, a in acc.items()}
    out.update(hist_obs=np.asarray(obs["hist"], dtype=np.int64), sums_obs=np.asarray(obs["sums"], dtype=np.int64),
               var_obs=np.array(obs["var"], dtype=np.int64), r_obs=obs["r"], tNo=np.asarray(obs["No"], dtype=np.uint32),
               tT=np.asarray(obs["T"], dtype=np.uint32))
    nan = float("nan")
    fS = float(S)
    pp = lambda a: np.asarray(a, dtype=np.float64) / fS if S >= 1 else np.full(np.shape(a), nan)         # noqa: E731
    mid = lambda a, b: (a.astype(np.float64) + b.astype(np.float64)) / (2.0 * fS) if S >= 1 else np.full(np.shape(a), nan)   # noqa: E731
    out["score_hist_obs"] = out["hist_obs"].astype(np.float64)
    out["score_hist_rep_mean"] = np.array([float(v) / fS if S >= 1 else nan for v in ints["hist_sum"]])
    out["score_hist_rep_sd"] = np.array([np.sqrt(float(S * q - v * v) / (fS * float(S - 1))) if S >= 2 else nan
                                         for v, q in zip(ints["hist_sum"], ints["hist_sumsq"])])
    out["ppp_hist"], out["ppp_hist_mid"] = pp(out["hist_ge"]), mid(out["hist_ge"], out["hist_gt"])
    out["ppp_cdf"], out["ppp_cdf_mid"] = pp(out["cdf_ge"]), mid(out["cdf_ge"], out["cdf_gt"])
    Vn_obs, ns = obs["var"]
    n2 = float(ns) * float(ns)
    out["score_var_obs"] = float(Vn_obs) / n2 if ns >= 1 else nan
    out["score_var_rep_mean"] = float(int(ints["var_rep_sum"][0])) / (fS * n2) if ns >= 1 and S >= 1 else nan
    out["ppp_var"] = float(int(ints["var_ge"][0])) / fS if ns >= 1 and S >= 1 else nan
    with np.errstate(invalid="ignore", divide="ignore"):
        Sr = S - out["r_undefined_count"].astype(np.int64)
        fr = np.where(Sr >= 1, Sr, 1).astype(np.float64)
        mean = out["r_rep_sum"] / fr
        out["r_rep_mean"] = np.where(Sr >= 1, mean, nan)
        v = (out["r_rep_sumsq"] - out["r_rep_sum"] * mean) / np.where(Sr >= 2, Sr - 1, 1).astype(np.float64)
        out["r_rep_sd"] = np.where(Sr >= 2, np.where(v > 0.0, np.sqrt(np.where(v > 0.0, v, 0.0)), 0.0), nan)
        out["ppp_r"] = np.where(Sr >= 1, out["r_ge"].astype(np.float64) / fr, nan)
        out["ppp_r_mid"] = np.where(Sr >= 1, (out["r_ge"].astype(np.float64) + out["r_gt"].astype(np.float64)) / (2.0 * fr), nan)
        out["r_undefined"] = out["r_undefined_count"].astype(np.float64)
        out["ppp_chi2"], out["ppp_chi2_mid"] = pp(out["chi_ge"]), mid(out["chi_ge"], out["chi_gt"])
        out["chi2_obs_mean"], out["chi2_rep_mean"] = pp(out["chi_obs_sum"]), pp(out["chi_rep_sum"])
        No = out["tNo"].astype(np.float64)
        out["obs_rate"] = np.where(No > 0, out["tT"].astype(np.float64) / np.where(No > 0, No, 1.0), nan)
        sn = out["sum_nr"].astype(np.float64)
        out["rep_rate"] = np.where(sn > 0, out["sum_r"].astype(np.float64) / np.where(sn > 0, sn, 1.0), nan)
        out["exp_rate"] = np.where((No > 0) & (S >= 1), out["sum_eo"] / np.where(No > 0, fS * No, 1.0), nan) if S >= 1 else np.full((K, m), nan)
        Sc = S - out["cell_empty"].astype(np.int64)
        fc = np.where(Sc >= 1, Sc, 1).astype(np.float64)
        out["ppp_cell"] = np.where(Sc >= 1, out["cell_ge"].astype(np.float64) / fc, nan)
        out["ppp_cell_mid"] = np.where(Sc >= 1, (out["cell_ge"].astype(np.float64) + out["cell_gt"].astype(np.float64)) / (2.0 * fc), nan)
    cuts = obs["cuts"]
    out["cuts"] = np.array(cuts, dtype=np.int64)
    out["group_lo"] = np.array((0,) + tuple(cuts), dtype=np.int64)
    out["group_hi"] = np.array(tuple(c - 1 for c in cuts) + (m - 1,), dtype=np.int64)
    out["worst"] = scores_worst(out["ppp_chi2_mid"], top)
    out.update(n=obs["n"], m=m, K=K, score_draws=S, score_skipped=int(skipped), n_scored=int(ns), last=last)
    return out


def scores_from_rep(y, g_draws, rep_draws, cuts=None, top=DEFAULT_SCORES_TOP) -> dict:
    """The header's score-based checks from stored draws: y (n x m; NaN = missing), g_draws (S, n, m) the draws of g = f + mu,
    rep_draws (S, n, m) with rep != 0 where yrep = +1; cuts None: default_score_cuts(y).  A draw with a non-finite g in an
    observed cell is skipped.  Returns scores_from_tables' dict."""
    y = np.asarray(y, dtype=np.float64)
    obs = scores_observed(y, default_score_cuts(y) if cuts is None else cuts)
    g_draws = np.asarray(g_draws, dtype=np.float64)
    S = g_draws.shape[0]
    assert g_draws.shape == (S,) + y.shape and np.asarray(rep_draws).shape == (S,) + y.shape
    ob = ~np.isnan(y)
    draws, skipped = [], 0
    for s in range(S):
        if not np.isfinite(g_draws[s][ob]).all():
            skipped += 1
            continue
        draws.append(scores_tables(y, g_draws[s], rep_draws[s], obs))
    return scores_from_tables(draws, top, skipped, obs)


def scores_from_draws(y, g_draws, seed, iters, cuts=None, top=DEFAULT_SCORES_TOP, item0=0):
    """scores_from_rep over the replicates of stored draws, built as dif_from_draws builds them: rep = [u < plogis(g)] with
    replicate_uniforms' u at the completed-iteration counters `iters`.  Returns (result, min |u - p| over the observed cells
    of the draws with finite g): a cell that close to its uniform may replicate either way under another evaluation of
    plogis."""
    y = np.asarray(y, dtype=np.float64)
    g_draws = np.asarray(g_draws, dtype=np.float64)
    n, m = y.shape
    ob = ~np.isnan(y)
    reps, gap = [], np.inf
    for s, it in enumerate(iters):
        with np.errstate(invalid="ignore"):
            fin = ob & np.isfinite(g_draws[s])
        p, _ = _plogis(np.where(fin, g_draws[s], 0.0))
        u = replicate_uniforms(seed, int(it), n, m, item0)
        if fin.any():
            gap = min(gap, float(np.abs(u - p)[fin].min()))
        reps.append(ob & (u < p))
    rep = np.stack(reps) if reps else np.zeros((0, n, m), dtype=bool)
    return scores_from_rep(y, g_draws, rep, cuts, top), gap


# ------------------------------------------------------------------------------------------------------- person fit ---
# ("person fit in the PPC" in the header; csrc/ppc_person.hip) the fifth add-on, the score-based checks transposed: every
# respondent's Guttman errors, lz and person response function within groups of the items' easiness.  `default_item_order` /
# `default_item_cuts` / `check_person_args`, `person_struct` / `person_result` wrap gpirt_ppc_person, `person_combine` pools chains'
# state blocks, `person_observed` / `person_tables` / `person_draw_stats` / `person_from_tables` are the NumPy statement of the
# header -- integer tables (G by the O(m^2) pair definition) and the lz sums in long double, then fp64 operations in the header's
# order, so the same tables give the same bits --, `person_from_rep` runs it over stored g and replicates, `person_from_draws`
# builds the replicates with this module's Philox.
DEFAULT_PERSON_TOP = 20
DEFAULT_PERSON_GROUPS = 5


def check_person_top(top) -> int:
    t = int(top)
    if t != top or not 1 <= t <= _lib.PERSON_MAX_TOP:
        raise ValueError(f"person: top must be an integer in 1..{_lib.PERSON_MAX_TOP}")
    return t


def default_item_order(y) -> np.ndarray:
    """The items by the data's yes rate T_j / N_j, descending (the easiest first), ties to the lowest j, the items without an
    observed cell last: a permutation of 0 .. m - 1 (int32)."""
    y = np.asarray(y, dtype=np.float64)
    ob = ~np.isnan(y)
    N, T = ob.sum(axis=0), (ob & (y > 0)).sum(axis=0)
    rate = np.where(N > 0, T / np.maximum(N, 1), -np.inf)
    return np.argsort(-rate, kind="stable").astype(np.int32)


def default_item_cuts(m: int, groups: int = DEFAULT_PERSON_GROUPS) -> tuple:
    """`groups` groups of near-equal position counts: the cuts k m // groups, k = 1 .. groups - 1, those outside 1 .. m - 1 and
    duplicates dropped (fewer groups where m < groups)."""
    g = int(groups)
    if g != groups or not 2 <= g <= _lib.PERSON_MAX_K:
        raise ValueError(f"person: groups must be an integer in 2..{_lib.PERSON_MAX_K}")
    return tuple(sorted({(k * int(m)) // g for k in range(1, g)} & set(range(1, int(m)))))


def check_person_args(order, cuts, m: int, n: int = 1):
    """(order as an int32 array, the cuts as a tuple of ints): order a permutation of 0 .. m - 1, the cuts ascending c_1 < ... <
    c_{K-1} in 1 .. m - 1, 2 <= K <= 16 groups; 2 <= m <= 4096 items and n <= 65534 respondents.  Anything else is a ValueError
    that says which."""
    if not 2 <= int(m) <= _lib.PERSON_MAX_M:
        raise ValueError(f"person: m = {m} is outside 2..{_lib.PERSON_MAX_M} items")
    if n > _lib.PERSON_MAX_N:
        raise ValueError(f"person: n = {n} is beyond {_lib.PERSON_MAX_N} respondents")
    try:
        o = np.asarray(order)
        oi = o.astype(np.int64)
        whole_o = o.ndim == 1 and bool(np.all(oi == o))
    except (TypeError, ValueError):
        raise ValueError("person: the order must be a sequence of integers") from None
    if not whole_o or len(oi) != m:
        raise ValueError(f"person: the order must hold {m} integers, a permutation of 0..{m - 1}")
    seen = np.zeros(m, dtype=bool)
    for t, j in enumerate(oi):
        if not 0 <= j < m or seen[j]:
            raise ValueError(f"person: the order is not a permutation of 0..{m - 1} (entry {t} is {int(j)})")
        seen[j] = True
    try:
        c = tuple(int(x) for x in cuts)
        whole = all(float(a) == float(b) for a, b in zip(c, cuts))
    except (TypeError, ValueError):
        raise ValueError("person: the cuts must be a sequence of integers") from None
    if not whole:
        raise ValueError("person: the cuts must be integers")
    if not 2 <= len(c) + 1 <= _lib.PERSON_MAX_K:
        raise ValueError(f"person: {len(c)} cuts make {len(c) + 1} item groups, 2..{_lib.PERSON_MAX_K} groups are taken")
    if any(not 1 <= x <= m - 1 for x in c) or any(b <= a for a, b in zip(c, c[1:])):
        raise ValueError(f"person: the cuts must be increasing integers in 1..{m - 1}, got {c}")
    return oi.astype(np.int32), c


def _person_shape(kind, n, m, K):
    return {"n": (n,), "c": (K, n), "3": (3, n), "2": (2, n)}[kind]


def person_field(name: str, n: int, m: int, K: int):
    """(shape, dtype) of the array gpirt_sampler_ppc_person_get copies for `name`: a finished field (PERSON_RESP_FIELDS: n;
    PERSON_CELL_FIELDS: K x n), a raw array or constant of PERSON_RAW, group_lo, group_hi, group_items, order, cuts, counts or an
    array of PERSON_LAST.  An unknown name is a ValueError that says so."""
    named = {r[0]: r for r in _lib.PERSON_RAW + _lib.PERSON_LAST}
    fixed = {"counts": ((2,), np.int64), "cuts": ((K - 1,), np.int64), "group_lo": ((K,), np.int64), "group_hi": ((K,), np.int64),
             "group_items": ((m,), np.int32), "order": ((m,), np.int32)}
    if name in fixed:
        return fixed[name]
    if name in named:
        _, dt, kind = named[name]
        return _person_shape(kind, n, m, K), _SC_DTYPES[dt]
    for names, shape in ((_lib.PERSON_RESP_FIELDS, (n,)), (_lib.PERSON_CELL_FIELDS, (K, n))):
        if name in names:
            return shape, np.float64
    raise ValueError(f"person: unknown field {name!r}")


def person_struct(n: int, m: int, K: int, top=DEFAULT_PERSON_TOP):
    """A gpirt_ppc_person with host arrays for every output, and those arrays (kept alive by the caller)."""
    p = _lib.PpcPerson()
    p.top = check_person_top(top)
    arr = {}
    for grp, names, shape in (("resp", _lib.PERSON_RESP_FIELDS, (n,)), ("cell", _lib.PERSON_CELL_FIELDS, (K, n))):
        for k, name in enumerate(names):
            arr[name] = np.empty(shape)
            getattr(p, grp)[k] = arr[name].ctypes.data_as(_dp)
    for k, (name, dt, kind) in enumerate(_lib.PERSON_RAW):
        arr[name] = np.empty(_person_shape(kind, n, m, K), dtype=_SC_DTYPES[dt])
        p.raw[k] = arr[name].ctypes.data
    for name in ("group_lo", "group_hi"):
        arr[name] = np.empty(K, dtype=np.int64)
        setattr(p, name, arr[name].ctypes.data_as(C.POINTER(C.c_int64)))
    arr["group_items"] = np.empty(m, dtype=np.int32)
    p.group_items = arr["group_items"].ctypes.data_as(C.POINTER(C.c_int32))
    arr["worst_respondents"] = np.empty(p.top, dtype=np.int64)
    p.worst_respondents = arr["worst_respondents"].ctypes.data_as(C.POINTER(C.c_int64))
    arr["worst_ppp_guttman_mid"] = np.empty(p.top)
    p.worst_ppp_guttman_mid = arr["worst_ppp_guttman_mid"].ctypes.data_as(_dp)
    return p, arr


def person_result(p, arr) -> dict:
    """The dict of Sampler.ppc_person() and person_combine(): every array of the header by name (cell (k, i) at [k, i]), "cuts",
    "worst" (dict: respondents, ppp_guttman_mid) and the counters."""
    out = {k: v for k, v in arr.items() if not k.startswith("worst_")}
    out["worst"] = dict(respondents=arr["worst_respondents"], ppp_guttman_mid=arr["worst_ppp_guttman_mid"])
    out["cuts"] = np.array([p.cuts[q] for q in range(p.K - 1)], dtype=np.int64)
    out.update(n=int(p.n), m=int(p.m), K=int(p.K), person_draws=int(p.person_draws), person_skipped=int(p.person_skipped),
               n_scored=int(p.n_scored))
    return out


def person_state_header(state) -> dict:
    """The header of a person-fit state block (a device tensor): its 8 int64 words and the cuts."""
    w = _lib.header_words(state, 24)
    K = int(w[4])
    return dict(tag=int(w[0]), version=int(w[1]), n=int(w[2]), m=int(w[3]), K=K, person_draws=int(w[5]), person_skipped=int(w[6]),
                cuts=tuple(int(x) for x in w[8:8 + max(min(K, 16) - 1, 0)]))


def person_combine(handle, states, top=DEFAULT_PERSON_TOP) -> dict:
    """gpirt_ppc_person_combine over the person-fit state blocks `states` (device tensors, or Samplers with ppc_person_enable()
    on, all on handle's device): the integers added, the doubles added in chain order; no signs (theta -> -theta leaves f + mu
    as it is).  Blocks with another n, m, K, order, cuts or response matrix are refused."""
    lib = _lib.load()
    tensors, nc, ptrs = _lib.state_ptrs(states, "ppc_person_state")
    hdr = person_state_header(tensors[0])
    if (hdr["tag"] != _lib.PERSON_TAG or not 2 <= hdr["K"] <= _lib.PERSON_MAX_K or not 2 <= hdr["m"] <= _lib.PERSON_MAX_M
            or not 1 <= hdr["n"] <= _lib.PERSON_MAX_N):
        raise ValueError("person_combine: the first state is not a person-fit state block")
    p, arr = person_struct(hdr["n"], hdr["m"], hdr["K"], top)
    check(lib.gpirt_ppc_person_combine(handle.ptr, nc, ptrs, C.byref(p)))
    return person_result(p, arr)


def _person_groups(m, cuts):
    """the group of every position: #{k : c_k <= t}"""
    return np.searchsorted(np.asarray(cuts, dtype=np.int64), np.arange(m), side="right")


def person_guttman(ob, bit) -> np.ndarray:
    """G per respondent by the pair definition: #{positions s < t, both observed : z_s = 0, z_t = 1}; ob and bit are n x m in
    POSITION order.  Every pair is looked at: O(m^2) per respondent."""
    ob = np.asarray(ob, dtype=bool)
    one = ob & (np.asarray(bit) != 0)
    zero = ob & ~one
    G = np.zeros(ob.shape[0], dtype=np.int64)
    for s in range(ob.shape[1] - 1):
        G += (zero[:, s:s + 1] & one[:, s + 1:]).sum(axis=1)
    return G


def _person_cells(grp, K, *terms):
    """per term the K x n sums over the positions of group k (terms n x m in position order, zero off the observed cells)"""
    return [np.stack([t[:, grp == k].sum(axis=1) for k in range(K)]).astype(np.int64) for t in terms]


def person_observed(y, order, cuts) -> dict:
    """The constants of the header from the data: N, x, g, q (int64, n), tN, tT (int64, K x n), live (the respondents with an
    observed cell), with order, cuts, grp (the group of every position), K, n, m."""
    y = np.asarray(y, dtype=np.float64)
    n, m = y.shape
    order, cuts = check_person_args(order, cuts, m, n)
    K = len(cuts) + 1
    yp = y[:, order]
    ob = ~np.isnan(yp)
    Y = ob & (yp > 0)
    grp = _person_groups(m, cuts)
    N, x = ob.sum(axis=1).astype(np.int64), Y.sum(axis=1).astype(np.int64)
    tN, tT = _person_cells(grp, K, ob, Y)
    return dict(order=order, cuts=cuts, grp=grp, K=K, n=n, m=m, N=N, live=N > 0, x=x, g=person_guttman(ob, Y), q=x * (N - x), tN=tN, tT=tT)


def person_observed_from_arrays(order, cuts, x_obs, g_obs, q_obs, tN, tT) -> dict:
    """person_observed's dict from the constants of a state block (gpirt_sampler_ppc_person_get): what person_draw_stats and
    person_from_tables read of it."""
    tN, tT = np.asarray(tN, dtype=np.int64), np.asarray(tT, dtype=np.int64)
    K, n = tN.shape
    order = np.asarray(order, dtype=np.int32)
    N = tN.sum(axis=0)
    return dict(order=order, cuts=tuple(int(c) for c in cuts), grp=_person_groups(len(order), cuts), K=K, n=n, m=len(order), N=N,
                live=N > 0, x=np.asarray(x_obs, dtype=np.int64), g=np.asarray(g_obs, dtype=np.int64), q=np.asarray(q_obs, dtype=np.int64),
                tN=tN, tT=tT)


def person_tables(y, g, rep, obs) -> dict:
    """One draw's tables: xr, gr, qr (int64, n), tR and the fixed-point tE, tV (int64, K x n), lz (3 x n LONG DOUBLE: Wo, Wr, Vl,
    with p and the sums in long double), with "obs" = person_observed's dict; g must be finite in the observed cells."""
    y = np.asarray(y, dtype=np.float64)
    order, K, grp = obs["order"], obs["K"], obs["grp"]
    yp = y[:, order]
    ob = ~np.isnan(yp)
    Y = ob & (yp > 0)
    bit = ob & (np.asarray(rep)[:, order] != 0)
    gz = np.where(ob, np.asarray(g, dtype=np.float64)[:, order], 0.0)
    p, e = _plogis(gz)
    q = np.where(gz >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
    ef = np.where(ob, np.rint(p * SCORES_FIX), 0.0).astype(np.int64)
    vf = np.where(ob, np.rint((p * q) * SCORES_FIX), 0.0).astype(np.int64)
    tR, tE, tV = _person_cells(grp, K, bit, ef, vf)
    xr = bit.sum(axis=1).astype(np.int64)
    ld = np.longdouble
    gl = gz.astype(ld)
    el = np.exp(-np.abs(gl))
    pl = np.where(gl >= 0, 1 / (1 + el), el / (1 + el))
    ql = np.where(gl >= 0, el / (1 + el), 1 / (1 + el))
    zero = ld(0)
    lz = np.stack([np.where(ob, (Y.astype(ld) - pl) * gl, zero).sum(axis=1), np.where(ob, (bit.astype(ld) - pl) * gl, zero).sum(axis=1),
                   np.where(ob, pl * ql * gl * gl, zero).sum(axis=1)])
    return dict(obs=obs, xr=xr, gr=person_guttman(ob, bit), qr=xr * (obs["N"] - xr), tR=tR, tE=tE, tV=tV, lz=lz)


def person_draw_stats(tables) -> dict:
    """The header's statistics and decisions of one draw from its tables (person_tables' dict, or the same arrays read from the
    device; lz is taken as fp64): gn (n: G_rep / Q_rep, 0 where undefined), lz_obs, lz_rep (n; 0 where undefined), chi (2 x n:
    X2(tT), X2(R)) and the bool decisions g_def, g_ge, g_gt, lz_def, chi_ge, chi_gt (n), cell_ge, cell_gt (K x n).  Nothing of a
    respondent without an observed cell is set."""
    obs = tables["obs"]
    live = obs["live"]
    Go, Qo = obs["g"], obs["q"]
    Gr, Qr = np.asarray(tables["gr"], dtype=np.int64), np.asarray(tables["qr"], dtype=np.int64)
    g_def = live & (Qo != 0) & (Qr != 0)
    out = dict(g_def=g_def, g_ge=g_def & (Gr * Qo >= Go * Qr), g_gt=g_def & (Gr * Qo > Go * Qr),
               gn=np.where(g_def, Gr.astype(np.float64) / np.where(g_def, Qr, 1).astype(np.float64), 0.0))
    Wo, Wr, Vl = (np.asarray(a).astype(np.float64) for a in tables["lz"])
    with np.errstate(invalid="ignore", divide="ignore"):
        lz_def = live & np.isfinite(Vl) & (Vl > 0.0) & np.isfinite(Wo) & np.isfinite(Wr)
        sd = np.sqrt(np.where(lz_def, Vl, 1.0))
        out.update(lz_def=lz_def, lz_obs=np.where(lz_def, Wo / sd, 0.0), lz_rep=np.where(lz_def, Wr / sd, 0.0))
    tN, T, R = obs["tN"], obs["tT"], np.asarray(tables["tR"], dtype=np.int64)
    has = tN > 0
    out.update(cell_ge=has & (R >= T), cell_gt=has & (R > T))
    x2T, x2R = _score_x2(T, tables["tE"], tables["tV"]), _score_x2(R, tables["tE"], tables["tV"])
    out.update(chi=np.stack([x2T, x2R]), chi_ge=live & (x2R >= x2T), chi_gt=live & (x2R > x2T))
    return out


def person_worst(ppp_guttman_mid, top=DEFAULT_PERSON_TOP) -> dict:
    """The `top` respondents with the smallest ppp_guttman_mid, ties to the lowest i, NaN never listed; padded with -1 / NaN."""
    top = check_person_top(top)
    mid = np.asarray(ppp_guttman_mid, dtype=np.float64)
    at = np.flatnonzero(~np.isnan(mid))
    order = at[np.argsort(mid[at], kind="stable")][:top]
    w = dict(respondents=np.full(top, -1, dtype=np.int64), ppp_guttman_mid=np.full(top, np.nan))
    w["respondents"][:len(order)] = order
    w["ppp_guttman_mid"][:len(order)] = mid[order]
    return w


def person_from_tables(draws, top=DEFAULT_PERSON_TOP, skipped=0, obs=None) -> dict:
    """The header's accumulators and finished fields from the COUNTED draws' tables (a list of person_tables' dicts, in draw
    order; obs: the constants, needed only when the list is empty).  Returns person_result's dict and "last" (the last draw's
    arrays under the getter's names, lz as fp64)."""
    S = len(draws)
    obs = draws[0]["obs"] if draws else obs
    n, m, K, live = obs["n"], obs["m"], obs["K"], obs["live"]
    kinds = {name: (dt, kind) for name, dt, kind in _lib.PERSON_RAW}
    acc = {name: np.zeros(_person_shape(kind, n, m, K), dtype=np.float64 if dt == "f8" else np.int64)
           for name, (dt, kind) in kinds.items() if (name, dt, kind) not in _lib.PERSON_CONST}
    un = 1.0 / SCORES_FIX
    has = obs["tN"] > 0
    last = None
    for d in draws:
        st = person_draw_stats(d)
        for k in ("g_ge", "g_gt", "cell_ge", "cell_gt", "chi_ge", "chi_gt"):
            acc[k] += st[k].astype(np.int64)
        acc["g_undefined_count"] += (live & ~st["g_def"]).astype(np.int64)
        acc["g_rep_sum"] += np.where(st["g_def"], np.asarray(d["gr"], dtype=np.int64), 0)
        acc["gn_rep_sum"] = acc["gn_rep_sum"] + st["gn"]
        acc["lz_undefined_count"] += (live & ~st["lz_def"]).astype(np.int64)
        acc["lz_obs_sum"] = acc["lz_obs_sum"] + st["lz_obs"]
        acc["lz_rep_sum"] = acc["lz_rep_sum"] + st["lz_rep"]
        acc["lz_rep_sumsq"] = acc["lz_rep_sumsq"] + st["lz_rep"] * st["lz_rep"]
        acc["sum_r"] += np.where(has, np.asarray(d["tR"], dtype=np.int64), 0)
        acc["sum_e"] = acc["sum_e"] + np.where(has, np.asarray(d["tE"], dtype=np.int64).astype(np.float64) * un, 0.0)
        acc["chi_obs_sum"] = acc["chi_obs_sum"] + np.where(live, st["chi"][0], 0.0)
        acc["chi_rep_sum"] = acc["chi_rep_sum"] + np.where(live, st["chi"][1], 0.0)
        last = dict(xr=np.asarray(d["xr"], dtype=np.int64), gr=np.asarray(d["gr"], dtype=np.int64), qr=np.asarray(d["qr"], dtype=np.int64),
                    tR=np.asarray(d["tR"], dtype=np.uint32), tE=np.asarray(d["tE"], dtype=np.int64), tV=np.asarray(d["tV"], dtype=np.int64),
                    lz=np.stack([np.asarray(a).astype(np.float64) for a in d["lz"]]), chi=st["chi"])
    out = {k: (a if a.dtype == np.float64 else a.astype(_SC_DTYPES[kinds[k][0]])) for k, a in acc.items()}
    out.update(x_obs=obs["x"].astype(np.int64), g_obs=obs["g"].astype(np.int64), q_obs=obs["q"].astype(np.int64),
               tN=obs["tN"].astype(np.uint32), tT=obs["tT"].astype(np.uint32))
    nan = float("nan")
    fS = float(S)
    f8 = lambda a: np.asarray(a).astype(np.float64)                                                       # noqa: E731
    with np.errstate(invalid="ignore", divide="ignore"):
        def over(num, cnt, least=1):
            """num / cnt where cnt >= least and the respondent has an observed cell, NaN elsewhere"""
            ok = live & (cnt >= least)
            return np.where(ok, f8(num) / np.where(ok, cnt, 1).astype(np.float64), nan)

        Sg, Sl = S - acc["g_undefined_count"], S - acc["lz_undefined_count"]
        Sall = np.full(n, S, dtype=np.int64)
        Qo = obs["q"]
        out["guttman_obs"] = np.where(live, f8(obs["g"]), nan)
        out["guttman_norm_obs"] = np.where(live & (Qo > 0), f8(obs["g"]) / np.where(Qo > 0, Qo, 1).astype(np.float64), nan)
        out["guttman_rep_mean"], out["guttman_norm_rep_mean"] = over(out["g_rep_sum"], Sg), over(out["gn_rep_sum"], Sg)
        out["ppp_guttman"] = over(out["g_ge"], Sg)
        out["ppp_guttman_mid"] = over(f8(out["g_ge"]) + f8(out["g_gt"]), 2 * Sg, 2)
        out["guttman_undefined"] = np.where(live, f8(out["g_undefined_count"]), nan)
        out["lz_obs_mean"], out["lz_rep_mean"] = over(out["lz_obs_sum"], Sl), over(out["lz_rep_sum"], Sl)
        mean = out["lz_rep_sum"] / np.where(Sl >= 1, Sl, 1).astype(np.float64)
        v = (out["lz_rep_sumsq"] - out["lz_rep_sum"] * mean) / np.where(Sl >= 2, Sl - 1, 1).astype(np.float64)
        out["lz_rep_sd"] = np.where(live & (Sl >= 2), np.where(v > 0.0, np.sqrt(np.where(v > 0.0, v, 0.0)), 0.0), nan)
        out["lz_undefined"] = np.where(live, f8(out["lz_undefined_count"]), nan)
        out["ppp_chi2"] = over(out["chi_ge"], Sall)
        out["ppp_chi2_mid"] = over(f8(out["chi_ge"]) + f8(out["chi_gt"]), 2 * Sall, 2)
        out["chi2_obs_mean"], out["chi2_rep_mean"] = over(out["chi_obs_sum"], Sall), over(out["chi_rep_sum"], Sall)
        tNf = np.where(has, obs["tN"], 1).astype(np.float64)
        out["obs_rate"] = np.where(has, f8(obs["tT"]) / tNf, nan)
        ok = has & (S >= 1)
        out["rep_rate"] = np.where(ok, f8(out["sum_r"]) / (fS * tNf), nan)
        out["exp_rate"] = np.where(ok, out["sum_e"] / (fS * tNf), nan)
        out["ppp_cell"] = np.where(ok, f8(out["cell_ge"]) / (fS if S else 1.0), nan)
        out["ppp_cell_mid"] = np.where(ok, (f8(out["cell_ge"]) + f8(out["cell_gt"])) / (2.0 * fS if S else 1.0), nan)
    cuts = obs["cuts"]
    out["cuts"] = np.array(cuts, dtype=np.int64)
    out["group_lo"] = np.array((0,) + tuple(cuts), dtype=np.int64)
    out["group_hi"] = np.array(tuple(c - 1 for c in cuts) + (m - 1,), dtype=np.int64)
    out["group_items"] = np.asarray(obs["order"], dtype=np.int32)
    out["worst"] = person_worst(out["ppp_guttman_mid"], top)
    out.update(n=n, m=m, K=K, person_draws=S, person_skipped=int(skipped), n_scored=int(live.sum()), last=last)
    return out


def person_from_rep(y, g_draws, rep_draws, order=None, cuts=None, top=DEFAULT_PERSON_TOP) -> dict:
    """The header's person fit from stored draws: y (n x m; NaN = missing), g_draws (S, n, m) the draws of g = f + mu, rep_draws
    (S, n, m) with rep != 0 where yrep = +1; order None: default_item_order(y), cuts None: default_item_cuts(m).  A draw with a
    non-finite g in an observed cell is skipped.  Returns person_from_tables' dict."""
    y = np.asarray(y, dtype=np.float64)
    obs = person_observed(y, default_item_order(y) if order is None else order, default_item_cuts(y.shape[1]) if cuts is None else cuts)
    g_draws = np.asarray(g_draws, dtype=np.float64)
    S = g_draws.shape[0]
    assert g_draws.shape == (S,) + y.shape and np.asarray(rep_draws).shape == (S,) + y.shape
    ob = ~np.isnan(y)
    draws, skipped = [], 0
    for s in range(S):
        if not np.isfinite(g_draws[s][ob]).all():
            skipped += 1
            continue
        draws.append(person_tables(y, g_draws[s], rep_draws[s], obs))
    return person_from_tables(draws, top, skipped, obs)


def person_from_draws(y, g_draws, seed, iters, order=None, cuts=None, top=DEFAULT_PERSON_TOP, item0=0):
    """person_from_rep over the replicates of stored draws, built as scores_from_draws builds them: rep = [u < plogis(g)] with
    replicate_uniforms' u at the completed-iteration counters `iters`.  Returns (result, min |u - p| over the observed cells
    of the draws with finite g): a cell that close to its uniform may replicate either way under another evaluation of
    plogis."""
    y = np.asarray(y, dtype=np.float64)
    g_draws = np.asarray(g_draws, dtype=np.float64)
    n, m = y.shape
    ob = ~np.isnan(y)
    reps, gap = [], np.inf
    for s, it in enumerate(iters):
        with np.errstate(invalid="ignore"):
            fin = ob & np.isfinite(g_draws[s])
        p, _ = _plogis(np.where(fin, g_draws[s], 0.0))
        u = replicate_uniforms(seed, int(it), n, m, item0)
        if fin.any():
            gap = min(gap, float(np.abs(u - p)[fin].min()))
        reps.append(ob & (u < p))
    rep = np.stack(reps) if reps else np.zeros((0, n, m), dtype=bool)
    return person_from_rep(y, g_draws, rep, order, cuts, top), gap


# ---------------------------------------------------------------------------------- residual correlations: device ---
DEFAULT_RESID_TOP = 20
RESID_UNIT = 4194304.0          # 2^22: the terms are integers in units of 2^-22
_RS_DTYPES = {"u8": np.uint64, "f8": np.float64, "u4": np.uint32, "i8": np.int64, "i4": np.int32, "i1": np.int8}


def check_resid_top(top) -> int:
    t = int(top)
    if t != top or not 1 <= t <= _lib.RESID_MAX_TOP:
        raise ValueError(f"resid: top must be an integer in 1..{_lib.RESID_MAX_TOP}")
    return t


def _resid_shape(kind, n, m):
    return {"p": (m, m), "i": (m,), "g": (16,), "c": (n, m), "d": (9, m, n), "s": (8,)}[kind]


def resid_field(name: str, n: int, m: int):
    """(shape, dtype, memory order) of the array gpirt_sampler_ppc_resid_get returns for `name` ("digits" comes as 9 x m x n and is
    transposed by the caller); an unknown name gets the library's refusal through a 1-element buffer."""
    if name in _lib.RESID_PAIR_FIELDS:
        return (m, m), np.float64, "C"
    if name in _lib.RESID_ITEM_FIELDS:
        return (m,), np.float64, "C"
    if name == "scalars":
        return (len(_lib.RESID_SCALARS),), np.float64, "C"
    if name == "counts":
        return (3,), np.int64, "C"
    for nm, dt, kind in _lib.RESID_RAW + _lib.RESID_LAST:
        if nm == name:
            return _resid_shape(kind, n, m), _RS_DTYPES[dt], "F" if kind == "c" else "C"
    return (1,), np.float64, "C"


def resid_struct(m: int, top=DEFAULT_RESID_TOP):
    """A gpirt_ppc_resid with host arrays for every output, and those arrays (kept alive by the caller)."""
    p = _lib.PpcResid()
    p.top = check_resid_top(top)
    arr = {}
    for k, name in enumerate(_lib.RESID_PAIR_FIELDS):
        arr[name] = np.empty((m, m))
        p.pair[k] = arr[name].ctypes.data_as(_dp)
    for k, name in enumerate(_lib.RESID_ITEM_FIELDS):
        arr[name] = np.empty(m)
        p.item[k] = arr[name].ctypes.data_as(_dp)
    for k, (name, dt, kind) in enumerate(_lib.RESID_RAW):
        arr[name] = np.empty(_resid_shape(kind, 0, m), dtype=_RS_DTYPES[dt])
        p.raw[k] = arr[name].ctypes.data
    arr["worst_pairs"] = np.empty((p.top, 2), dtype=np.int64)
    p.worst_pairs = arr["worst_pairs"].ctypes.data_as(C.POINTER(C.c_int64))
    arr["worst_items"] = np.empty(p.top, dtype=np.int64)
    p.worst_items = arr["worst_items"].ctypes.data_as(C.POINTER(C.c_int64))
    for name in ("worst_ppp_rc_mid", "worst_rc_obs_mean", "worst_ppp_ss_mid"):
        arr[name] = np.empty(p.top)
        setattr(p, name, arr[name].ctypes.data_as(_dp))
    return p, arr


def resid_result(p, arr) -> dict:
    """The dict of Sampler.ppc_resid() and resid_combine(): every pair array (m x m, pair (a, b) at [a, b]), item array (m) and
    raw array of the header by name, the scalars as floats, "worst" (dict: pairs (top x 2), ppp_rc_mid, rc_obs_mean), "worst_items"
    (dict: items, ppp_ss_mid) and the counters."""
    out = {k: v for k, v in arr.items() if not k.startswith("worst_")}
    out.update({k: float(p.scalar[i]) for i, k in enumerate(_lib.RESID_SCALARS)})
    out["worst"] = dict(pairs=arr["worst_pairs"], ppp_rc_mid=arr["worst_ppp_rc_mid"], rc_obs_mean=arr["worst_rc_obs_mean"])
    out["worst_items"] = dict(items=arr["worst_items"], ppp_ss_mid=arr["worst_ppp_ss_mid"])
    out.update(n=int(p.n), m=int(p.m), resid_draws=int(p.resid_draws), resid_skipped=int(p.resid_skipped),
               global_undefined=int(p.global_undefined))
    return out


def resid_state_header(state) -> dict:
    """The 8 int64 header words of a residual-correlation state block (a device tensor)."""
    w = _lib.header_words(state)
    return dict(n=int(w[0]), m=int(w[1]), version=int(w[2]), resid_draws=int(w[3]), resid_skipped=int(w[4]), item0=int(w[5]),
                tag=int(w[7]))


def resid_combine(handle, states, top=DEFAULT_RESID_TOP) -> dict:
    """gpirt_ppc_resid_combine over the state blocks `states` (device tensors, or Samplers with ppc_resid_enable() on, all on
    handle's device): the integers added, the double sums added in chain order.  Blocks with another n, m, item0 or n_co are
    refused."""
    lib = _lib.load()
    tensors, nc, ptrs = _lib.state_ptrs(states, "ppc_resid_state")
    m = resid_state_header(tensors[0])["m"]
    p, arr = resid_struct(m if 2 <= m <= _lib.RESID_MAX_M else 2, top)
    check(lib.gpirt_ppc_resid_combine(handle.ptr, nc, ptrs, C.byref(p)))
    return resid_result(p, arr)


# ----------------------------------------------------------------------------------- residual correlations: NumPy ---
def resid_digits(x):
    """x (integers in [-2^22, 2^22]) as three balanced base-256 digits: x = d0 + 256 d1 + 65536 d2, d0 and d1 in [-128, 127],
    |d2| <= 64 -- the int8 planes of the device."""
    x = np.asarray(x, dtype=np.int64)
    d0 = ((x + 128) & 255) - 128
    x1 = (x - d0) >> 8
    d1 = ((x1 + 128) & 255) - 128
    return d0, d1, (x1 - d1) >> 8


def resid_join(d0, d1, d2):
    return np.asarray(d0, dtype=np.int64) + 256 * np.asarray(d1, dtype=np.int64) + 65536 * np.asarray(d2, dtype=np.int64)


def resid_terms(y, g, rep):
    """(dt_obs, dt_rep, wt), int64 n x m in units of 2^-22, from y (NaN = missing), g = f + mu of one draw and the replicate
    (rep != 0 where yrep = +1): d = +q where the answer is +1, -p where it is -1, w = p q, each rounded once by rint; 0 in the
    unobserved cells, whatever g holds there.  p and q by the PPC's arithmetic (g = +-inf gives exactly 0 and 1)."""
    y = np.asarray(y, dtype=np.float64)
    obs = ~np.isnan(y)
    g = np.where(obs, np.asarray(g, dtype=np.float64), 0.0)
    e = np.exp(-np.abs(g))
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)
    p, q = np.where(g >= 0, big, small), np.where(g >= 0, small, big)
    fix = lambda v: np.where(obs, np.rint(v * RESID_UNIT), 0.0).astype(np.int64)            # noqa: E731
    return fix(np.where(y > 0, q, -p)), fix(np.where(np.asarray(rep) != 0, q, -p)), fix(p * q)


def resid_tables(dt_obs, dt_rep, wt, O):
    """The exact tables of one draw: S_obs = dt_obs^T dt_obs, S_rep = dt_rep^T dt_rep (units of 2^-44), V = wt^T O (units of
    2^-22), int64 m x m."""
    a, b, w, O = (np.asarray(x, dtype=np.int64) for x in (dt_obs, dt_rep, wt, O))
    return dict(s_obs=a.T @ a, s_rep=b.T @ b, v=w.T @ O)


def resid_lane_sum(x):
    """The sum over the last axis of non-negative terms in the device's order: lane l of 64 adds the entries l, l + 64, ... in
    ascending order, then the 64 lane sums are added in lane order (np.cumsum adds strictly in order)."""
    x = np.asarray(x, dtype=np.float64)
    pad = (-x.shape[-1]) % 64
    x = np.concatenate([x, np.zeros(x.shape[:-1] + (pad,))], axis=-1).reshape(x.shape[:-1] + (-1, 64))
    return np.cumsum(np.cumsum(x, axis=-2)[..., -1, :], axis=-1)[..., -1]


def resid_draw_stats(tables, n_co) -> dict:
    """One draw's statistics from its integer tables, in the header's arithmetic: r_obs, r_rep (m x m: the correlations, the infit
    on the diagonal, NaN where n_co = 0 or V[a, b] V[b, a] = 0), the integer decisions ge, gt (S_rep >= / > S_obs), live and
    defined (bool m x m), t_obs, t_rep, t_count per item and stats = (Q, M+, M of the data, Q, M+, M of the replicate, the defined
    pairs a < b, 0)."""
    So, Sr, V = (np.asarray(tables[k], dtype=np.int64) for k in ("s_obs", "s_rep", "v"))
    m = So.shape[0]
    eye = np.eye(m, dtype=bool)
    live = np.asarray(n_co) > 0
    defined = live & (V != 0) & (V.T != 0)
    Vd = V.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.where(eye, Vd * RESID_UNIT, np.sqrt(Vd * Vd.T) * RESID_UNIT)
        r_obs = np.where(defined, So.astype(np.float64) / den, np.nan)
        r_rep = np.where(defined, Sr.astype(np.float64) / den, np.nan)
    off = defined & ~eye
    up = off & np.triu(np.ones((m, m), dtype=bool), 1)
    sq = lambda r, mask: np.where(mask, r * r, 0.0)            # noqa: E731
    t_obs, t_rep = resid_lane_sum(sq(r_obs, off)), resid_lane_sum(sq(r_rep, off))
    Q_obs, Q_rep = resid_lane_sum(resid_lane_sum(sq(r_obs, up))), resid_lane_sum(resid_lane_sum(sq(r_rep, up)))
    big = lambda r: float(np.max(r[up])) if up.any() else -np.inf            # noqa: E731
    stats = np.array([Q_obs, big(r_obs), big(np.abs(r_obs)), Q_rep, big(r_rep), big(np.abs(r_rep)), float(up.sum()), 0.0])
    return dict(r_obs=r_obs, r_rep=r_rep, ge=defined & (Sr >= So), gt=defined & (Sr > So), live=live, defined=defined,
                t_obs=t_obs, t_rep=t_rep, t_count=off.sum(axis=1), stats=stats)


def _resid_finish(so, sr, sq, ge, gt, D):
    """obs_mean, rep_mean, rep_sd, ppp, ppp_mid from the sums and counts over D draws, in the host code's arithmetic"""
    so, sr, sq, ge, gt = (np.asarray(x, dtype=np.float64) for x in (so, sr, sq, ge, gt))
    D = np.asarray(D, dtype=np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        dD = np.where(D >= 1, D, 1).astype(np.float64)
        ok = D >= 1
        mean = sr / dD
        var = (sq - sr * mean) / np.where(D >= 2, D - 1, 1).astype(np.float64)
        sd = np.where(var > 0.0, np.sqrt(np.where(var > 0.0, var, 0.0)), 0.0)
        nanif = lambda v, good: np.where(good, v, np.nan)            # noqa: E731
        return (nanif(so / dD, ok), nanif(mean, ok), nanif(sd, D >= 2), nanif(ge / dD, ok), nanif((ge + gt) / (2.0 * dD), ok))


def resid_worst(ppp_rc_mid, rc_obs_mean, top=DEFAULT_RESID_TOP) -> dict:
    """The `top` pairs a < b with the smallest ppp_rc_mid, ties to the lowest (a, b), NaN never listed; padded with -1 / NaN."""
    m = ppp_rc_mid.shape[0]
    ia, ib = np.triu_indices(m, 1)
    mid = ppp_rc_mid[ia, ib]
    ok = ~np.isnan(mid)
    ia, ib, mid = ia[ok], ib[ok], mid[ok]
    order = np.argsort(mid, kind="stable")[:top]
    w = dict(pairs=np.full((top, 2), -1, dtype=np.int64), ppp_rc_mid=np.full(top, np.nan), rc_obs_mean=np.full(top, np.nan))
    w["pairs"][:len(order), 0], w["pairs"][:len(order), 1] = ia[order], ib[order]
    w["ppp_rc_mid"][:len(order)] = mid[order]
    w["rc_obs_mean"][:len(order)] = rc_obs_mean[ia[order], ib[order]]
    return w


def resid_worst_items(ppp_ss_mid, top=DEFAULT_RESID_TOP) -> dict:
    """The `top` items with the smallest ppp_ss_mid, ties to the lowest index, NaN never listed; padded with -1 / NaN."""
    idx = np.flatnonzero(~np.isnan(ppp_ss_mid))
    order = idx[np.argsort(ppp_ss_mid[idx], kind="stable")[:top]]
    w = dict(items=np.full(top, -1, dtype=np.int64), ppp_ss_mid=np.full(top, np.nan))
    w["items"][:len(order)] = order
    w["ppp_ss_mid"][:len(order)] = ppp_ss_mid[order]
    return w


def resid_from_tables(draws, n_co, top=DEFAULT_RESID_TOP, skipped=0, n=0, chains=None) -> dict:
    """resid_result's dict from the integer tables of the COUNTED draws (a list of dicts s_obs, s_rep, v: resid_tables' or the
    device's own) and n_co = O^T O: every accumulator grows draw by draw as the device's does, every finished value by the host
    code's arithmetic.  chains: the number of draws of each pooled chain, in chain order (None: one chain); the chains' sums are
    formed apart and added in chain order, as gpirt_ppc_resid_combine adds them."""
    top = check_resid_top(top)
    n_co = np.asarray(n_co, dtype=np.int64)
    m = n_co.shape[0]
    chains = [len(draws)] if chains is None else list(chains)
    assert sum(chains) == len(draws)
    zf = lambda *s: np.zeros(s)            # noqa: E731
    zi = lambda *s: np.zeros(s, dtype=np.int64)            # noqa: E731
    tot = None
    at = 0
    for count in chains:
        a = dict(undefined_count=zi(m, m), rc_ge=zi(m, m), rc_gt=zi(m, m), rc_obs_sum=zf(m, m), rc_rep_sum=zf(m, m),
                 rc_rep_sumsq=zf(m, m), ss_undefined=zi(m), ss_ge=zi(m), ss_gt=zi(m), ss_obs_sum=zf(m), ss_rep_sum=zf(m),
                 gd=zf(7), gi=zi(7))
        for tables in draws[at:at + count]:
            d = resid_draw_stats(tables, n_co)
            df = d["defined"]
            a["undefined_count"] += d["live"] & ~df
            a["rc_ge"] += d["ge"]
            a["rc_gt"] += d["gt"]
            a["rc_obs_sum"] = np.where(df, a["rc_obs_sum"] + np.where(df, d["r_obs"], 0.0), a["rc_obs_sum"])
            a["rc_rep_sum"] = np.where(df, a["rc_rep_sum"] + np.where(df, d["r_rep"], 0.0), a["rc_rep_sum"])
            a["rc_rep_sumsq"] = np.where(df, a["rc_rep_sumsq"] + np.where(df, d["r_rep"] * d["r_rep"], 0.0), a["rc_rep_sumsq"])
            has = d["t_count"] > 0
            a["ss_undefined"] += ~has
            a["ss_obs_sum"] = np.where(has, a["ss_obs_sum"] + d["t_obs"], a["ss_obs_sum"])
            a["ss_rep_sum"] = np.where(has, a["ss_rep_sum"] + d["t_rep"], a["ss_rep_sum"])
            a["ss_ge"] += has & (d["t_rep"] >= d["t_obs"])
            a["ss_gt"] += has & (d["t_rep"] > d["t_obs"])
            st = d["stats"]
            if st[6] == 0:
                a["gi"][6] += 1
                continue
            a["gd"] += np.array([st[0], st[3], st[3] * st[3], st[1], st[4], st[2], st[5]])
            for k in range(3):
                a["gi"][2 * k] += st[3 + k] >= st[k]
                a["gi"][2 * k + 1] += st[3 + k] > st[k]
        at += count
        tot = a if tot is None else {k: tot[k] + a[k] for k in a}
    S = len(draws)
    eye = np.eye(m, dtype=bool)
    live = n_co > 0
    cell = _resid_finish(tot["rc_obs_sum"], tot["rc_rep_sum"], tot["rc_rep_sumsq"], tot["rc_ge"], tot["rc_gt"], S - tot["undefined_count"])
    pair_ok = live & ~eye
    out = {"n_co": n_co.astype(np.float64)}
    for k, v in zip(("rc_obs_mean", "rc_rep_mean", "rc_rep_sd", "ppp_rc", "ppp_rc_mid"), cell):
        out[k] = np.where(pair_ok, v, np.nan)
    out["undefined"] = np.where(pair_ok, tot["undefined_count"], np.nan).astype(np.float64)
    item_ok = np.diag(live)
    for k, v in zip(("infit_obs_mean", "infit_rep_mean", "infit_rep_sd", "ppp_infit", "ppp_infit_mid"), cell):
        out[k] = np.where(item_ok, np.diag(v), np.nan)
    ss = _resid_finish(tot["ss_obs_sum"], tot["ss_rep_sum"], 0.0 * tot["ss_rep_sum"], tot["ss_ge"], tot["ss_gt"], S - tot["ss_undefined"])
    for k, v in zip(("ss_obs_mean", "ss_rep_mean", None, "ppp_ss", "ppp_ss_mid"), ss):
        if k:
            out[k] = np.where(item_ok, v, np.nan)
    gd, gi = tot["gd"], tot["gi"]
    D = S - int(gi[6])
    fr = _resid_finish(gd[0], gd[1], gd[2], gi[0], gi[1], D)
    mx = _resid_finish(gd[3], gd[4], 0.0, gi[2], gi[3], D)
    am = _resid_finish(gd[5], gd[6], 0.0, gi[4], gi[5], D)
    sc = (fr[0], fr[1], fr[2], fr[3], fr[4], mx[0], mx[1], mx[3], mx[4], am[0], am[1], am[3], am[4])
    out.update({k: float(v) for k, v in zip(_lib.RESID_SCALARS, sc)})
    out["n_co_int"] = n_co.copy()
    for name, dt, _ in _lib.RESID_RAW[1:-1]:
        out[name] = tot[name].astype(_RS_DTYPES[dt])
    glob = np.zeros(16, dtype=np.uint64)
    glob[:7] = gd.view(np.uint64)
    glob[7:14] = gi.astype(np.uint64)
    out["global"] = glob
    out["worst"] = resid_worst(out["ppp_rc_mid"], out["rc_obs_mean"], top)
    out["worst_items"] = resid_worst_items(out["ppp_ss_mid"], top)
    out.update(n=int(n), m=m, resid_draws=S, resid_skipped=int(skipped), global_undefined=int(gi[6]))
    return out


def resid_from_rep(y, g_draws, rep_draws, top=DEFAULT_RESID_TOP) -> dict:
    """The header's residual correlations from stored draws: y (n x m; NaN = missing), g_draws (S, n, m) the draws of g = f +
    mu, rep_draws (S, n, m) with rep != 0 where yrep = +1.  A draw with a NaN g in an observed cell is skipped whole
    (resid_skipped).  Steps: resid_terms, resid_tables (int64 matrix products), resid_draw_stats, resid_from_tables."""
    y = np.asarray(y, dtype=np.float64)
    n, m = y.shape
    obs = ~np.isnan(y)
    O = obs.astype(np.int64)
    draws, skipped = [], 0
    for g, rep in zip(np.asarray(g_draws, dtype=np.float64), np.asarray(rep_draws)):
        if np.isnan(g[obs]).any():
            skipped += 1
            continue
        draws.append(resid_tables(*resid_terms(y, g, rep), O))
    return resid_from_tables(draws, O.T @ O, top, skipped, n)


def resid_from_draws(y, g_draws, seed, iters, top=DEFAULT_RESID_TOP, item0=0):
    """resid_from_rep over the replicates of stored draws: rep = [u < plogis(g)] with replicate_uniforms' u at the
    completed-iteration counters `iters`.  Returns (result, min |u - p| over the observed cells): a cell that close to its uniform
    may replicate either way under another evaluation of plogis."""
    y = np.asarray(y, dtype=np.float64)
    g_draws = np.asarray(g_draws, dtype=np.float64)
    n, m = y.shape
    obs = ~np.isnan(y)
    reps, gap = [], np.inf
    for s, it in enumerate(iters):
        with np.errstate(invalid="ignore"):
            p, _ = _plogis(np.where(obs, g_draws[s], 0.0))
        u = replicate_uniforms(seed, int(it), n, m, item0)
        if obs.any() and not np.isnan(p[obs]).any():
            gap = min(gap, float(np.abs(u - p)[obs].min()))
        reps.append(obs & (u < p))
    rep = np.stack(reps) if reps else np.zeros((0, n, m), dtype=bool)
    return resid_from_rep(y, g_draws, rep, top), gap


def resid_contrasts(result, k=5) -> dict:
    """The PCAR first-contrast view of a residual-correlation result (host only): the k largest eigenvalues and their vectors
    of rc_obs_mean with the diagonal set to 1, by numpy.linalg.eigh.  Items whose row holds a NaN off the diagonal are dropped one
    at a time, the item with the most NaNs first (ties to the highest index), and reported.  Returns dict(values (k,), vectors
    (kept x k), items (the kept items' indices), dropped).  Descriptive only: it has NO p-value -- the posterior predictive tests
    of the same matrix are ppp_frob_mid, ppp_max_mid and ppp_absmax_mid."""
    R = np.array(result["rc_obs_mean"], dtype=np.float64)
    m = R.shape[0]
    np.fill_diagonal(R, 1.0)
    keep = np.arange(m)
    while keep.size:
        bad = np.isnan(R[np.ix_(keep, keep)]).sum(axis=1)
        if not bad.any():
            break
        keep = np.delete(keep, np.flatnonzero(bad == bad.max())[-1])
    dropped = np.setdiff1d(np.arange(m), keep)
    k = int(min(k, keep.size))
    if k < 1:
        return dict(values=np.zeros(0), vectors=np.zeros((0, 0)), items=keep, dropped=dropped)
    w, v = np.linalg.eigh(R[np.ix_(keep, keep)])
    return dict(values=w[::-1][:k].copy(), vectors=v[:, ::-1][:, :k].copy(), items=keep, dropped=dropped)
