"""Posteriors of the sum score S = number of yes answers on a form of items, without stored draws: the score distribution, the
score-to-theta conversion table, the test characteristic curve (TCC), the conditional standard error and the reliability of the
score (include/gpirt_hip.h, "Sum-score posteriors": gpirt_sampler_sumscore_*, gpirt_sumscore_combine, gpirt_run.sumscore;
csrc/sumscore.hip).

Per draw the device runs the Lord-Wingersky recursion over the form's items at every grid point, from the draw's f*:
A[k, s] = P(S = s | theta_k, this draw).  It keeps the JOINT sum_d w_k A_d[k, s] (w the N(0, 1) weights of the grid) and
normalises once at the end -- on purpose not gpirt_amd.score's mean of per-draw posteriors --, so that pooling chains is plain
addition.  `struct` / `result` wrap the C struct, `combine` pools chains' state blocks (a chain with sign -1 enters with its k
axis reversed), `finish` builds the public dict from raw accumulators, and `from_draws` is the NumPy statement of the header
over fetched f*, with the recursion and every sum in long double.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import NGRID, SUMSCORE_MAX_ITEMS, SUMSCORE_RAW, check

DEFAULT_PROBS = (0.025, 0.5, 0.975)
THETA = -5.0 + np.arange(NGRID, dtype=np.float64) * 0.01
_SUMS = ("joint_sum", "pi_sum", "pi_sumsq", "tcc_sum", "tcc_sumsq", "var_sum", "rel")
_COUNTS = ("draws", "skipped", "rel_draws", "rel_skipped")


# ---------------------------------------------------------------------------------------------------- the contract ---
def check_probs(probs):
    p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    if ((p < 0.0) | (p > 1.0) | np.isnan(p)).any():
        raise ValueError("sumscore: probs must lie in [0, 1]")
    return p


def form_mask(items, m: int) -> np.ndarray:
    """The form as m bytes (1: in the form).  items: None (all m); a MASK, which is an array of dtype bool or uint8 and length
    m (non-zero: in the form); or column INDICES, which is any other sequence of integers (0-based, each at most once).  The
    dtype and the length decide which, never the values.  An index outside 0..m-1, a repeated index, an empty form and more
    than 4096 items are refused with a ValueError that says so."""
    m = int(m)
    if items is None:
        mask = np.ones(m, dtype=np.uint8)
    else:
        a = np.asarray(items)
        if a.size == 0:
            raise ValueError("sumscore: the form is empty")
        if a.dtype in (np.bool_, np.uint8) and a.shape == (m,):
            mask = (a != 0).astype(np.uint8)
        else:
            if a.dtype.kind not in "iu" or a.ndim != 1 or a.dtype in (np.bool_, np.uint8):
                raise ValueError("sumscore: items must be None, a bool or uint8 mask of length m, or a list of column indices")
            if a.size and (a.min() < 0 or a.max() >= m):
                bad = int(a[(a < 0) | (a >= m)][0])
                raise ValueError(f"sumscore: item index {bad} is outside 0..{m - 1} (the prepared data's columns, after "
                                 f"unanimous items were dropped)")
            if np.unique(a).size != a.size:
                raise ValueError("sumscore: items names a column index more than once")
            mask = np.zeros(m, dtype=np.uint8)
            mask[a] = 1
    M = int(mask.sum())
    if M < 1:
        raise ValueError("sumscore: the form is empty")
    if M > SUMSCORE_MAX_ITEMS:
        raise ValueError(f"sumscore: the form has M = {M} items, at most {SUMSCORE_MAX_ITEMS} are taken")
    return np.ascontiguousarray(mask)


def parse(sumscore, m: int) -> dict:
    """gpirtMCMC's sumscore= argument (True or a dict(items, probs)) as a checked dict with the form's mask."""
    if sumscore is not True and not isinstance(sumscore, dict):
        raise ValueError("sumscore must be None, False, True or a dict(items=..., probs=...)")
    d = dict(sumscore) if isinstance(sumscore, dict) else {}
    unknown = set(d) - {"items", "probs"}
    if unknown:
        raise ValueError(f"sumscore: unknown keys {sorted(unknown)}")
    return dict(mask=form_mask(d.get("items"), m), probs=check_probs(d.get("probs", DEFAULT_PROBS)))


def grid_weights() -> np.ndarray:
    """w_k: the N(0, 1) density on the grid, normalised -- from the double theta_k = -5 + 0.01 k in long double, the sum in
    ascending k, the quotient rounded once to float64 (what the library stores in the state)."""
    th = THETA.astype(np.longdouble)
    e = np.exp(-(th * th) / np.longdouble(2))
    total = np.longdouble(0)
    for v in e:
        total = total + v
    return (e / total).astype(np.float64)


def _raw_shape(name, m, M):
    return dict(joint_sum=(NGRID, M + 1), pi_sum=(M + 1,), pi_sumsq=(M + 1,), tcc_sum=(NGRID,), tcc_sumsq=(NGRID,), var_sum=(NGRID,),
                rel=(2,), mask=(m,), w=(NGRID,), last=(NGRID, M + 1), last_pi=(M + 1,))[name]


# ------------------------------------------------------------------------------------------------------ the device ---
def struct(m: int, M: int, mask=None):
    """A gpirt_sumscore asking for every raw array, and the host arrays behind it (kept alive by the caller).  mask (m bytes)
    is read by gpirt_mcmc_run; gpirt_sumscore_combine ignores it."""
    r = _lib.Sumscore()
    arrays = {}
    for k, (name, dt) in enumerate(SUMSCORE_RAW):
        arrays[name] = np.zeros(_raw_shape(name, m, M), dtype=np.dtype(dt))
        r.raw[k] = arrays[name].ctypes.data
    if mask is not None:
        arrays["_items"] = np.ascontiguousarray(mask, dtype=np.uint8)
        r.items = arrays["_items"].ctypes.data
    return r, arrays


def result(r, arrays, probs=DEFAULT_PROBS, y=None) -> dict:
    """The "sumscore" dict of gpirtMCMC(sumscore=...), Sampler.sumscore() and combine(), from a filled gpirt_sumscore."""
    raw = {name: arrays[name] for name, _ in SUMSCORE_RAW}
    return finish(raw, probs, int(r.draws), int(r.skipped), int(r.rel_draws), int(r.rel_skipped), y)


def state_header(state) -> dict:
    """The header of a sum-score state block (a device tensor of int64)."""
    w = _lib.header_words(state, 16)
    return dict(tag=int(w[0]), version=int(w[1]), m=int(w[2]), M=int(w[3]), N=int(w[4]), draws=int(w[5]), skipped=int(w[6]),
                rel_draws=int(w[7]), rel_skipped=int(w[8]))


def combine(handle, states, signs=None, probs=DEFAULT_PROBS, y=None) -> dict:
    """gpirt_sumscore_combine over the state blocks `states` (device tensors, or Samplers with sumscore_enable() on, all on
    handle's device): added in chain order, a chain with sign -1 entering with its k axis reversed (signs=None: none is).
    States with another m, another form or other grid weights are refused.  y (the prepared data): also the observed score
    histogram over the respondents who answered every item of the form."""
    lib = _lib.load()
    probs = check_probs(probs)
    tensors, nc, ptrs = _lib.state_ptrs(states, "sumscore_state")
    hdr = state_header(tensors[0])
    if hdr["tag"] != _lib.SUMSCORE_TAG:
        raise ValueError("sumscore.combine: state 0 is not a sum-score state block")
    r, arrays = struct(hdr["m"], hdr["M"])
    sg = (C.c_int * nc)(*[int(x) for x in signs]) if signs is not None else None
    check(lib.gpirt_sumscore_combine(handle.ptr, nc, ptrs, sg, C.byref(r)))
    return result(r, arrays, probs, y)


# ------------------------------------------------------------------------------------------------------- finishing ---
def observed(y, mask):
    """(n_complete, obs_hist): over the respondents who answered every item of the form (y: +1 / -1 / NaN), how many there
    are and how many of them have each score 0 .. M"""
    cols = np.flatnonzero(mask)
    sub = np.asarray(y, dtype=np.float64)[:, cols]
    full = ~np.isnan(sub).any(axis=1)
    scores = (sub[full] == 1.0).sum(axis=1)
    return int(full.sum()), np.bincount(scores, minlength=cols.size + 1).astype(np.int64)


def finish(raw, probs=DEFAULT_PROBS, draws=0, skipped=0, rel_draws=0, rel_skipped=0, y=None) -> dict:
    """The finished outputs from (pooled) raw accumulators; shared by the device path and from_draws."""
    probs = check_probs(probs)
    out = dict(raw)
    mask = np.asarray(raw["mask"])
    items = np.flatnonzero(mask)
    M = items.size
    w = np.asarray(raw["w"], dtype=np.float64)
    joint = np.asarray(raw["joint_sum"], dtype=np.float64)
    D, R = np.float64(draws), np.float64(rel_draws)
    out.update(draws=int(draws), skipped=int(skipped), rel_draws=int(rel_draws), rel_skipped=int(rel_skipped), items=items, M=M,
               probs=probs, theta=THETA.copy(), scores=np.arange(M + 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        out["score_dist"] = raw["pi_sum"] / D
        out["score_dist_sd"] = np.sqrt(np.maximum(raw["pi_sumsq"] - raw["pi_sum"] ** 2 / D, 0.0) / (D - 1.0))
        out["score_cdf"] = np.cumsum(out["score_dist"])
        # the joint, normalised once; a score the pooled chains give no mass at all has no posterior
        tot = joint.sum(axis=0)
        have = (tot > 0.0) & (np.asarray(raw["pi_sum"]) > 0.0)
        post = np.where(have[None, :], joint / np.where(have, tot, 1.0)[None, :], np.nan).T           # (M + 1) x 1001
        out["post"] = post
        eap = post @ THETA
        out["theta_eap"] = eap
        out["theta_sd"] = np.sqrt(np.maximum(post @ (THETA * THETA) - eap * eap, 0.0))
        cum = np.cumsum(np.where(have[:, None], post, 0.0), axis=1)
        tq = np.full((probs.size, M + 1), np.nan)
        for i, q in enumerate(probs):                       # the first grid point whose cumulated mass reaches q
            k = np.minimum((cum < q).sum(axis=1), NGRID - 1)
            tq[i] = np.where(have, THETA[k], np.nan)
        out["theta_quantiles"] = tq
        out["theta_map"] = np.where(have, THETA[np.argmax(np.where(have[:, None], post, 0.0), axis=1)], np.nan)   # lowest k on ties
        out["score_given_theta"] = joint / (D * w)[:, None]
        out["tcc_mean"] = raw["tcc_sum"] / D
        var_t = np.maximum(raw["tcc_sumsq"] - raw["tcc_sum"] ** 2 / D, 0.0) / (D - 1.0)
        out["tcc_sd"] = np.sqrt(var_t)
        out["csem"] = np.sqrt(raw["var_sum"] / D + (var_t if draws > 1 else 0.0))
        out["reliability_mean"] = float(raw["rel"][0] / R)
        out["reliability_sd"] = float(np.sqrt(max(raw["rel"][1] - raw["rel"][0] ** 2 / R, 0.0) / (R - 1.0)))
    if y is not None:
        n_complete, hist = observed(y, mask)
        out.update(n_complete=n_complete, obs_hist=hist, exp_count=n_complete * out["score_dist"])
    return out


# ------------------------------------------------------------------------------------------------------- NumPy -------
def zeros(mask) -> dict:
    """empty accumulators (long double) for the form `mask`"""
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    M, ld = int(mask.sum()), np.longdouble
    return dict(joint_sum=np.zeros((NGRID, M + 1), dtype=ld), pi_sum=np.zeros(M + 1, dtype=ld), pi_sumsq=np.zeros(M + 1, dtype=ld),
                tcc_sum=np.zeros(NGRID, dtype=ld), tcc_sumsq=np.zeros(NGRID, dtype=ld), var_sum=np.zeros(NGRID, dtype=ld),
                rel=np.zeros(2, dtype=ld), mask=mask, w=grid_weights(), last=np.zeros((NGRID, M + 1), dtype=ld),
                last_pi=np.zeros(M + 1, dtype=ld), draws=0, skipped=0, rel_draws=0, rel_skipped=0, rel_terms=[])


def draw_rows(f):
    """A[k, s], T[k], V[k] of one draw's form columns f (rows x M, float64, no NaN) in long double.  Equal rows are worked once."""
    f = np.asarray(f, dtype=np.float64)
    uniq, inv = np.unique(f, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    fl = uniq.astype(np.longdouble)
    one = np.longdouble(1)
    with np.errstate(over="ignore"):
        p = one / (one + np.exp(-fl))                       # each on its own: q is never 1 - p
        q = one / (one + np.exp(fl))
    U, M = fl.shape
    A = np.zeros((U, M + 1), dtype=np.longdouble)
    A[:, 0] = 1
    T = np.zeros(U, dtype=np.longdouble)
    V = np.zeros(U, dtype=np.longdouble)
    with np.errstate(under="ignore"):
        for j in range(M):
            pj, qj = p[:, j:j + 1], q[:, j:j + 1]
            A[:, 1:j + 2] = A[:, 1:j + 2] * qj + A[:, 0:j + 1] * pj
            A[:, 0:1] = A[:, 0:1] * qj
            T += p[:, j]
            V += p[:, j] * q[:, j]
    return A[inv], T[inv], V[inv]


def accumulate(acc, fstar):
    """Add one draw's f* (1001 x m, float64) to the accumulators `acc`: the header's rules, one statement each."""
    fstar = np.asarray(fstar, dtype=np.float64)
    cols = np.flatnonzero(acc["mask"])
    f = fstar[:, cols]
    if np.isnan(f).any():                                   # a NaN in a form column: the draw is skipped whole
        acc["skipped"] += 1
        return
    A, T, V = draw_rows(f)
    w = acc["w"].astype(np.longdouble)
    with np.errstate(under="ignore"):
        wa = w[:, None] * A
        acc["joint_sum"] += wa
        pi = wa.sum(axis=0)
    acc["pi_sum"] += pi
    acc["pi_sumsq"] += pi * pi
    acc["tcc_sum"] += T
    acc["tcc_sumsq"] += T * T
    acc["var_sum"] += V
    acc["last"], acc["last_pi"] = A, pi
    acc["draws"] += 1
    a, b, c = (w * V).sum(), (w * (V + T * T)).sum(), (w * T).sum()
    den = b - c * c
    acc["rel_terms"].append((float(a), float(b), float(c)))
    if den > 0:
        rho = 1 - a / den
        acc["rel"] += np.array([rho, rho * rho])
        acc["rel_draws"] += 1
    else:
        acc["rel_skipped"] += 1


def reflect(acc) -> dict:
    """theta -> -theta on the accumulators: the k axis of everything indexed by k; pi and rel are kept."""
    out = dict(acc)
    for k in ("joint_sum", "tcc_sum", "tcc_sumsq", "var_sum", "last"):
        out[k] = acc[k][::-1].copy()
    return out


def add(a, b) -> dict:
    """a + b (chains pooled in order); mask and w are a's, last and last_pi b's"""
    out = dict(a)
    for k in _SUMS + _COUNTS:
        out[k] = a[k] + b[k]
    out["rel_terms"] = a["rel_terms"] + b["rel_terms"]
    out["last"], out["last_pi"] = b["last"], b["last_pi"]
    return out


def from_draws(fstar_draws, items=None, probs=DEFAULT_PROBS, signs=None, y=None) -> dict:
    """The NumPy statement of the header over fetched f*.  fstar_draws: one chain's f* (S x 1001 x m) or a sequence of chains';
    signs: per chain, -1 reverses that chain's k axis before pooling.  The recursion and every sum run in long double and are
    returned rounded to float64; "rel_terms" lists, per counted draw, the reliability's three sums."""
    chains = [fstar_draws] if isinstance(fstar_draws, np.ndarray) and fstar_draws.ndim == 3 else list(fstar_draws)
    if signs is None:
        signs = [1] * len(chains)
    if len(signs) != len(chains) or any(s not in (1, -1) for s in signs):
        raise ValueError("from_draws: signs must give +1 or -1 per chain")
    pooled = None
    for ch, sg in zip(chains, signs):
        ch = np.asarray(ch, dtype=np.float64)
        if ch.ndim != 3 or ch.shape[1] != NGRID:
            raise ValueError("from_draws: a chain's f* is S x 1001 x m")
        acc = zeros(form_mask(items, ch.shape[2]))
        for f in ch:
            accumulate(acc, f)
        if sg < 0:
            acc = reflect(acc)
        pooled = acc if pooled is None else add(pooled, acc)
    with np.errstate(under="ignore"):
        raw = {name: (np.asarray(pooled[name], dtype=np.float64) if pooled[name].dtype == np.longdouble else pooled[name])
               for name, _ in SUMSCORE_RAW}
    out = finish(raw, probs, pooled["draws"], pooled["skipped"], pooled["rel_draws"], pooled["rel_skipped"], y)
    out["rel_terms"] = np.array(pooled["rel_terms"], dtype=np.float64).reshape(-1, 3)
    return out
