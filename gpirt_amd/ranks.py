"""Rank posteriors without stored draws: rank intervals, pivots, pairwise order (include/gpirt_hip.h, "rank posteriors":
gpirt_sampler_rank_*, gpirt_rank_combine, gpirt_run.ranks; csrc/ranks.hip).

Every sampled theta is a grid point -5 + 0.01 k, so a draw's ranks follow from a 1001-bin count and a prefix sum:
less_i = #{k_j < k_i}, eq_i = #{k_j = k_i}, R2_i = 2 less_i + eq_i + 1 (twice the mid-rank).  The device accumulates, per
respondent, sum R2, sum R2^2 and a histogram of R2, per pivot position q the draws in which a respondent covers q
(less_i < q <= less_i + eq_i) and their shares 1 / eq_i, and optionally lt[i, j] = #{draws : k_i < k_j}.  A draw with any
respondent off the grid is skipped whole.  `struct` / `result` wrap the C struct, `combine` pools chains' state blocks
(reflecting a chain exactly where its sign is -1), and `from_draws` is the NumPy statement of the header over stored theta
draws: every integer it returns is what the device must hold bit for bit.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import RANK_MAX_N, RANK_MAX_PIVOTS, RANK_MAX_PIVOTS_CLOSED, check
from .quantiles import grid_index

DEFAULT_PROBS = (0.025, 0.5, 0.975)


# ---------------------------------------------------------------------------------------------------- the contract ---
def bin_scheme(n: int):
    """(B, w, pad) of rank_hist over R2 = 2 .. 2n: w the smallest odd width with ceil((2n - 1) / w) <= 1025,
    B = ceil((2n - 1) / w), plus one if that is even, pad = (B w - (2n - 1)) / 2; bin = (R2 - 2 + pad) // w."""
    span = 2 * int(n) - 1
    w = 1
    while -(-span // w) > 1025:
        w += 2
    B = -(-span // w)
    if B % 2 == 0:
        B += 1
    return B, w, (B * w - span) // 2


def close_pivots(n: int, pivots="median"):
    """The sorted closure under q <-> n + 1 - q of `pivots`: "median", a position, or a sequence of positions and
    "median" ((n + 1) / 2 for odd n, n / 2 and n / 2 + 1 for even n).  Returns (the positions as given, the closed set)."""
    n = int(n)
    if isinstance(pivots, str) or np.isscalar(pivots):
        pivots = (pivots,)
    given = []
    for q in pivots:
        if isinstance(q, str):
            if q != "median":
                raise ValueError(f"unknown pivot {q!r}")
            given += sorted({(n + 1) // 2, n + 1 - (n + 1) // 2})
        else:
            given.append(int(q))
    return given, sorted({q for g in given for q in (g, n + 1 - g)})


# ------------------------------------------------------------------------------------------------------ the device ---
def struct(n: int, pivots="median", probs=DEFAULT_PROBS, pairwise=False, closed=None):
    """A gpirt_ranks asking for every output (lt with pairwise), and the host arrays behind it (kept alive by the
    caller).  The struct's pivots are the ones given: gpirt_mcmc_run reads them; gpirt_rank_combine ignores them.
    closed: the closed set of a state block as it is (up to 32 positions), for gpirt_rank_combine: the arrays are sized
    by it and no positions are given."""
    if closed is not None:
        given, closed = [], [int(q) for q in closed]
        if not 1 <= len(closed) <= RANK_MAX_PIVOTS_CLOSED:
            raise ValueError(f"a closed pivot set has 1..{RANK_MAX_PIVOTS_CLOSED} positions, not {len(closed)}")
    else:
        given, closed = close_pivots(n, pivots)
        if len(given) > RANK_MAX_PIVOTS:
            raise ValueError(f"{len(given)} pivots given, at most {RANK_MAX_PIVOTS} are taken")
    B, _, _ = bin_scheme(n)
    P = len(closed)
    pr = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    arrays = dict(probs=pr, rank_mean=np.empty(n), rank_var=np.empty(n), rank_q=np.empty((pr.size, n)),
                  p_pivot=np.empty((P, n)), pivot_share=np.empty((P, n)), rank2_sum=np.empty(n, dtype=np.uint64),
                  rank2_sumsq=np.empty(n, dtype=np.uint64), rank_hist=np.empty((n, B), dtype=np.uint32),
                  pivot_cover=np.empty((P, n), dtype=np.uint32))
    if pairwise:
        arrays["lt"] = np.empty((n, n), dtype=np.uint32)
    r = _lib.Ranks()
    for k, a in arrays.items():
        setattr(r, k, a.ctypes.data_as(dict(r._fields_)[k]))
    r.nprobs = pr.size
    r.n_pivots = len(given)
    for k, q in enumerate(given):
        r.pivots[k] = q
    r.pairwise = int(bool(pairwise))
    return r, arrays


def result(r, arrays) -> dict:
    """The "ranks" dict of gpirtMCMC(ranks=...), Sampler.ranks() and combine()."""
    S = int(r.draws)
    out = {k: arrays[k] for k in ("probs", "rank_mean", "rank_var", "p_pivot", "pivot_share", "pivot_cover", "rank2_sum",
                                  "rank2_sumsq", "rank_hist")}
    out["rank_quantiles"] = arrays["rank_q"]
    out["rank_bin_width"] = float(r.rank_bin_width)
    out["order"] = np.argsort(arrays["rank_mean"], kind="stable")
    out["pivots"] = np.array([int(r.pivots[k]) for k in range(int(r.n_pivots))], dtype=np.int64)
    out["lt"] = arrays.get("lt")
    with np.errstate(invalid="ignore", divide="ignore"):
        out["p_less"] = arrays["lt"] / np.float64(S) if "lt" in arrays else None
    out["draws"] = S
    out["skipped_draws"] = int(r.skipped)
    return out


def combine(handle, states, signs=None, probs=DEFAULT_PROBS) -> dict:
    """gpirt_rank_combine over the rank state blocks `states` (device tensors, or Samplers with rank_enable() on, all on
    handle's device): the integers added, the shares added in chain order, a chain with sign -1 reflected exactly first
    (signs=None: nothing is reflected).  p_less comes with it when every state holds the pairwise counters."""
    lib = _lib.load()
    tensors, nc, ptrs = _lib.state_ptrs(states, "rank_state")
    hdrs = [state_header(t) for t in tensors]
    r, arrays = struct(hdrs[0]["n"], None, probs, all(h["pairwise"] for h in hdrs), closed=hdrs[0]["pivots"])
    sg = (C.c_int * nc)(*[int(x) for x in signs]) if signs is not None else None
    check(lib.gpirt_rank_combine(handle.ptr, nc, ptrs, sg, C.byref(r)))
    return result(r, arrays)


def state_header(state) -> dict:
    """The header of a rank state block (a device tensor of int64): n, draws (counted), skipped, version, B, w, the closed
    pivots and the pairwise flag."""
    w = _lib.header_words(state, 40)
    return dict(n=int(w[0]), draws=int(w[1]), skipped=int(w[2]), version=int(w[3]), B=int(w[4]), w=int(w[5]),
                pivots=[int(x) for x in w[8:8 + int(w[6])]], pairwise=bool(w[7]))


# ------------------------------------------------------------------------------------------------------- NumPy -------
def _exact_var(S, s1, s2):
    """(S sum R2^2 - (sum R2)^2) / (4 S (S - 1)): the numerator in exact integers, rounded once"""
    if S < 2:
        return np.full(len(s1), np.nan)
    return np.array([float(S * int(b) - int(a) ** 2) / (4.0 * float(S) * float(S - 1)) for a, b in zip(s1, s2)])


def _chain(k, n, closed, B, w, pad, pairwise):
    """One chain's accumulators from its grid indices k (S, n; -1 = off the grid), as Python-int / NumPy-int arrays."""
    P = len(closed)
    acc = dict(S=0, skipped=0, s1=np.zeros(n, dtype=np.uint64), s2=np.zeros(n, dtype=np.uint64),
               hist=np.zeros((n, B), dtype=np.int64), cover=np.zeros((P, n), dtype=np.int64), share=np.zeros((P, n)),
               lt=np.zeros((n, n), dtype=np.uint32) if pairwise else None)
    rows = np.arange(n)
    for kd in k:
        if (kd < 0).any():
            acc["skipped"] += 1
            continue
        acc["S"] += 1
        cnt = np.bincount(kd, minlength=_lib.NGRID)
        less = (np.cumsum(cnt) - cnt)[kd]
        eq = cnt[kd]
        R2 = 2 * less + eq + 1
        acc["s1"] += R2.astype(np.uint64)                # R2 <= 2n <= 2^15 and S < 2^32: both sums stay below 2^64
        acc["s2"] += (R2 * R2).astype(np.uint64)
        acc["hist"][rows, (R2 - 2 + pad) // w] += 1
        for p, q in enumerate(closed):
            on = (less < q) & (q <= less + eq)
            acc["cover"][p] += on
            acc["share"][p] = acc["share"][p] + np.where(on, 1.0 / eq, 0.0)     # draw order; x + 0.0 = x
        if pairwise:
            acc["lt"] += kd[:, None] < kd[None, :]
    return acc


def _reflect(a, n):
    """The header's exact reflection of one chain's accumulators."""
    S, c = a["S"], 2 * n + 2
    s1, s2 = [int(x) for x in a["s1"]], [int(x) for x in a["s2"]]                 # Python integers: exact
    return dict(S=S, skipped=a["skipped"], s1=np.array([S * c - x for x in s1], dtype=np.uint64),
                s2=np.array([S * c * c - 2 * c * x + y for x, y in zip(s1, s2)], dtype=np.uint64), hist=a["hist"][:, ::-1],
                cover=a["cover"][::-1], share=a["share"][::-1], lt=a["lt"].T if a["lt"] is not None else None)


def from_draws(theta_draws, pivots="median", probs=DEFAULT_PROBS, signs=None, pairwise=False) -> dict:
    """What the device accumulates and gpirt_rank_combine reports, from stored draws theta_draws (C, S, n) (or (S, n): one
    chain): each chain accumulated on its own, a chain with signs[c] = -1 reflected by the header's exact rule, the
    integers added and the shares added in chain order.  Returns result()'s keys; the integer arrays are exact."""
    th = np.asarray(theta_draws, dtype=np.float64)
    if th.ndim == 2:
        th = th[None]
    C_, _, n = th.shape
    if n > RANK_MAX_N:
        raise ValueError(f"n = {n} is beyond {RANK_MAX_N} respondents")
    given, closed = close_pivots(n, pivots)
    if len(given) > RANK_MAX_PIVOTS or any(q < 1 or q > n for q in given):
        raise ValueError("at most 16 pivots, each in 1..n")
    B, w, pad = bin_scheme(n)
    sg = [1] * C_ if signs is None else [int(x) for x in signs]
    k = grid_index(th)
    pooled = None
    for c in range(C_):
        a = _chain(k[c], n, closed, B, w, pad, pairwise)
        if sg[c] < 0:
            a = _reflect(a, n)
        if pooled is None:
            pooled = {key: (np.array(v) if isinstance(v, np.ndarray) else v) for key, v in a.items()}
            continue
        pooled["S"] += a["S"]
        pooled["skipped"] += a["skipped"]
        for key in ("s1", "s2", "hist", "cover") + (("lt",) if pairwise else ()):
            pooled[key] = pooled[key] + a[key]
        pooled["share"] = pooled["share"] + a["share"]
    S = pooled["S"]
    pr = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    nan = np.full(n, np.nan)
    s1, s2 = pooled["s1"], pooled["s2"]
    cum = np.cumsum(pooled["hist"], axis=1)
    rq = np.empty((pr.size, n))
    for p, q in enumerate(pr):
        need = max(1, int(math.ceil(q * float(S))))
        b = np.minimum((cum < need).sum(axis=1), B - 1)
        rq[p] = 0.5 * (2 - pad + (b + 1) * w - 1).astype(np.float64) if S >= 1 else nan
    with np.errstate(invalid="ignore", divide="ignore"):
        out = dict(probs=pr, rank_mean=s1.astype(np.float64) / (2.0 * float(S)) if S >= 1 else nan,
                   rank_var=_exact_var(S, s1, s2), rank_quantiles=rq, rank_bin_width=0.5 * w,
                   p_pivot=pooled["share"] / float(S) if S >= 1 else np.full(pooled["share"].shape, np.nan),
                   pivot_share=np.ascontiguousarray(pooled["share"]), pivot_cover=pooled["cover"].astype(np.uint32),
                   rank2_sum=s1, rank2_sumsq=s2, rank_hist=pooled["hist"].astype(np.uint32),
                   pivots=np.array(closed, dtype=np.int64), lt=np.ascontiguousarray(pooled["lt"]) if pairwise else None,
                   draws=S, skipped_draws=pooled["skipped"])
        out["p_less"] = out["lt"] / np.float64(S) if pairwise else None
    out["order"] = np.argsort(out["rank_mean"], kind="stable")
    return out
