"""Two forms at once, without stored draws: the joint distribution of the sum scores on two disjoint forms X and Y, the
equipercentile equivalents of each form's scores on the other's scale (IRT observed-score equating), the concordance tables, the
correlation of the two scores and the agreement of pass / fail decisions (include/gpirt_hip.h, "Two-form score equating":
gpirt_sampler_equate_*, gpirt_equate_combine, gpirt_run.equate; csrc/equate.hip).

Per draw the device runs the sum-score recursion once per form and contracts the two score tables over the grid in one fp64
matrix-core product: J[s, t] = sum_k (w_k A_X[k, s]) A_Y[k, t].  It keeps the JOINT and normalises once at the end, so pooling
chains is plain addition -- and since theta -> -theta changes none of these quantities, without signs.  `struct` / `result` wrap
the C struct, `combine` pools chains' state blocks, `finish` builds the public dict from raw accumulators, and `from_draws` is the
NumPy statement of the header over fetched f*, with every recursion, sum and quotient in long double.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import sumscore as SS
from ._lib import EQUATE_MAX_CUTS, EQUATE_MAX_ITEMS, EQUATE_RAW, NGRID, check

DEFAULT_PROBS = (0.025, 0.5, 0.975)
_SUMS = ("joint_sum", "pix_sum", "pix_sumsq", "piy_sum", "piy_sumsq", "eyx_sum", "eyx_sumsq", "exy_sum", "exy_sumsq", "corr")
_LAST = ("corr_terms", "last_joint", "last_pix", "last_piy", "last_eyx", "last_exy")
_COUNTS = ("draws", "skipped", "corr_draws", "corr_skipped", "eq_clamped")


# ---------------------------------------------------------------------------------------------------- the contract ---
def check_probs(probs):
    p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    if ((p < 0.0) | (p > 1.0) | np.isnan(p)).any():
        raise ValueError("equate: probs must lie in [0, 1]")
    return p


def form_masks(x, y, m: int):
    """The two forms as m bytes each (1: in the form).  x and y follow gpirt_amd.sumscore.form_mask's rule (a bool or uint8 mask
    of length m, or column indices), except that None is not a form here.  An empty form, a form of more than 2048 items and
    forms that share a column (the first shared column is named) are refused with a ValueError that says so."""
    masks = []
    for name, items in (("x", x), ("y", y)):
        if items is None:
            raise ValueError(f"equate: form {name} is missing (column indices or a boolean mask)")
        try:
            mask = SS.form_mask(items, m)
        except ValueError as e:
            raise ValueError(f"equate: form {name}: {str(e).replace('sumscore: ', '')}") from None
        M = int(mask.sum())
        if M > EQUATE_MAX_ITEMS:
            raise ValueError(f"equate: form {name} has {M} items, at most {EQUATE_MAX_ITEMS} are taken")
        masks.append(mask)
    both = np.flatnonzero(masks[0] & masks[1])
    if both.size:
        raise ValueError(f"equate: the forms overlap (column {int(both[0])} is in both); the two scores factorise given theta "
                         f"only for disjoint forms")
    return masks[0], masks[1]


def check_cuts(cuts, Mx: int, My: int) -> np.ndarray:
    """cuts: up to 8 pairs (cx, cy), 1 <= cx <= M_X and 1 <= cy <= M_Y (a score >= the cut passes), as an int64 C x 2 array"""
    if cuts is None:
        return np.zeros((0, 2), dtype=np.int64)
    a = np.asarray(cuts)
    if a.size == 0:
        return np.zeros((0, 2), dtype=np.int64)
    if a.dtype.kind not in "iu" or a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("equate: cuts must be pairs of integers (cx, cy)")
    if a.shape[0] > EQUATE_MAX_CUTS:
        raise ValueError(f"equate: {a.shape[0]} cuts, at most {EQUATE_MAX_CUTS} are taken")
    if (a[:, 0] < 1).any() or (a[:, 0] > Mx).any() or (a[:, 1] < 1).any() or (a[:, 1] > My).any():
        raise ValueError(f"equate: a cut (cx, cy) needs 1 <= cx <= {Mx} and 1 <= cy <= {My}")
    return np.ascontiguousarray(a, dtype=np.int64)


def parse(equate, m: int) -> dict:
    """gpirtMCMC's equate= argument (a dict(x, y, probs, cuts)) as a checked dict with the two masks."""
    if not isinstance(equate, dict):
        raise ValueError("equate must be None or a dict(x=..., y=..., probs=..., cuts=...)")
    unknown = set(equate) - {"x", "y", "probs", "cuts"}
    if unknown:
        raise ValueError(f"equate: unknown keys {sorted(unknown)}")
    mx, my = form_masks(equate.get("x"), equate.get("y"), m)
    return dict(mask_x=mx, mask_y=my, probs=check_probs(equate.get("probs", DEFAULT_PROBS)),
                cuts=check_cuts(equate.get("cuts"), int(mx.sum()), int(my.sum())))


def _raw_shape(name, m, Mx, My):
    X, Y = (Mx + 1,), (My + 1,)
    return dict(joint_sum=(Mx + 1, My + 1), pix_sum=X, pix_sumsq=X, piy_sum=Y, piy_sumsq=Y, eyx_sum=X, eyx_sumsq=X, exy_sum=Y,
                exy_sumsq=Y, corr=(2,), corr_terms=(5,), mask_x=(m,), mask_y=(m,), w=(NGRID,), last_joint=(Mx + 1, My + 1),
                last_pix=X, last_piy=Y, last_eyx=X, last_exy=Y)[name]


# ------------------------------------------------------------------------------------------------------ the device ---
def struct(m: int, Mx: int, My: int, mask_x=None, mask_y=None):
    """A gpirt_equate asking for every raw array, and the host arrays behind it (kept alive by the caller).  The masks (m bytes
    each) are read by gpirt_mcmc_run; gpirt_equate_combine ignores them."""
    r = _lib.Equate()
    arrays = {}
    for k, (name, dt) in enumerate(EQUATE_RAW):
        arrays[name] = np.zeros(_raw_shape(name, m, Mx, My), dtype=np.dtype(dt))
        r.raw[k] = arrays[name].ctypes.data
    if mask_x is not None:
        arrays["_x"] = np.ascontiguousarray(mask_x, dtype=np.uint8)
        arrays["_y"] = np.ascontiguousarray(mask_y, dtype=np.uint8)
        r.x, r.y = arrays["_x"].ctypes.data, arrays["_y"].ctypes.data
    return r, arrays


def result(r, arrays, probs=DEFAULT_PROBS, cuts=None) -> dict:
    """The "equate" dict of gpirtMCMC(equate=...), Sampler.equate() and combine(), from a filled gpirt_equate."""
    raw = {name: arrays[name] for name, _ in EQUATE_RAW}
    return finish(raw, probs, cuts, int(r.draws), int(r.skipped), int(r.corr_draws), int(r.corr_skipped), int(r.eq_clamped))


def state_header(state) -> dict:
    """The header of an equating state block (a device tensor of int64)."""
    w = _lib.header_words(state, 16)
    return dict(tag=int(w[0]), version=int(w[1]), m=int(w[2]), Mx=int(w[3]), My=int(w[4]), N=int(w[5]), draws=int(w[6]),
                skipped=int(w[7]), corr_draws=int(w[8]), corr_skipped=int(w[9]), eq_clamped=int(w[10]))


def combine(handle, states, probs=DEFAULT_PROBS, cuts=None) -> dict:
    """gpirt_equate_combine over the state blocks `states` (device tensors, or Samplers with equate_enable() on, all on handle's
    device): added in chain order.  There are no signs: a reflected chain enters unchanged.  States with another m, other forms
    or other grid weights are refused."""
    lib = _lib.load()
    probs = check_probs(probs)
    tensors, nc, ptrs = _lib.state_ptrs(states, "equate_state")
    hdr = state_header(tensors[0])
    if hdr["tag"] != _lib.EQUATE_TAG:
        raise ValueError("equate.combine: state 0 is not an equating state block")
    r, arrays = struct(hdr["m"], hdr["Mx"], hdr["My"])
    check(lib.gpirt_equate_combine(handle.ptr, nc, ptrs, C.byref(r)))
    return result(r, arrays, probs, cuts)


# ------------------------------------------------------------------------------------------------------- finishing ---
def _conditional(joint, probs):
    """rows of `joint` normalised once: (cond, mean, quantiles); a row without mass gives NaN"""
    tot = joint.sum(axis=1)
    have = tot > 0.0
    cond = np.where(have[:, None], joint / np.where(have, tot, 1.0)[:, None], np.nan)
    mean = cond @ np.arange(joint.shape[1], dtype=np.float64)
    cum = np.cumsum(np.where(have[:, None], cond, 0.0), axis=1)
    qs = np.full((probs.size, joint.shape[0]), np.nan)
    for i, q in enumerate(probs):                           # the first score whose cumulated mass reaches q
        t = np.minimum((cum < q).sum(axis=1), joint.shape[1] - 1)
        qs[i] = np.where(have, t.astype(np.float64), np.nan)
    return cond, mean, qs


def _mean_sd(s, ss, D):
    with np.errstate(invalid="ignore", divide="ignore"):
        return s / D, np.sqrt(np.maximum(ss - s * s / D, 0.0) / (D - 1.0))


def finish(raw, probs=DEFAULT_PROBS, cuts=None, draws=0, skipped=0, corr_draws=0, corr_skipped=0, eq_clamped=0) -> dict:
    """The finished outputs from (pooled) raw accumulators; shared by the device path and from_draws."""
    probs = check_probs(probs)
    out = dict(raw)
    x_items, y_items = np.flatnonzero(np.asarray(raw["mask_x"])), np.flatnonzero(np.asarray(raw["mask_y"]))
    Mx, My = x_items.size, y_items.size
    cuts = check_cuts(cuts, Mx, My)
    joint = np.asarray(raw["joint_sum"], dtype=np.float64)
    D, R = np.float64(draws), np.float64(corr_draws)
    out.update(draws=int(draws), skipped=int(skipped), corr_draws=int(corr_draws), corr_skipped=int(corr_skipped),
               eq_clamped=int(eq_clamped), x_items=x_items, y_items=y_items, Mx=Mx, My=My, probs=probs, cuts=cuts)
    with np.errstate(invalid="ignore", divide="ignore"):
        out["joint"] = joint / D
        out["x_dist"], out["x_dist_sd"] = _mean_sd(raw["pix_sum"], raw["pix_sumsq"], D)
        out["y_dist"], out["y_dist_sd"] = _mean_sd(raw["piy_sum"], raw["piy_sumsq"], D)
        out["y_of_x_mean"], out["y_of_x_sd"] = _mean_sd(raw["eyx_sum"], raw["eyx_sumsq"], D)
        out["x_of_y_mean"], out["x_of_y_sd"] = _mean_sd(raw["exy_sum"], raw["exy_sumsq"], D)
        # the concordance: the pooled joint, normalised once per row (per column for X given Y)
        out["y_given_x"], out["y_given_x_mean"], out["y_given_x_quantiles"] = _conditional(joint, probs)
        out["x_given_y"], out["x_given_y_mean"], out["x_given_y_quantiles"] = _conditional(np.ascontiguousarray(joint.T), probs)
        cm, cs = _mean_sd(np.float64(raw["corr"][0]), np.float64(raw["corr"][1]), R)
        out["corr_mean"], out["corr_sd"] = float(cm), float(cs)
        # decision consistency at each pair of cuts (a score >= the cut passes): from the pooled joint
        total = joint.sum()
        agree, kappa = np.full(cuts.shape[0], np.nan), np.full(cuts.shape[0], np.nan)
        for c, (cx, cy) in enumerate(cuts):
            pp, ff = joint[cx:, cy:].sum() / total, joint[:cx, :cy].sum() / total
            px, py = joint[cx:, :].sum() / total, joint[:, cy:].sum() / total
            pe = px * py + (1.0 - px) * (1.0 - py)
            agree[c] = pp + ff
            kappa[c] = (agree[c] - pe) / (1.0 - pe)
        out["agreement"], out["kappa"] = agree, kappa
    return out


# ------------------------------------------------------------------------------------------------------- NumPy -------
def zeros(mask_x, mask_y) -> dict:
    """empty accumulators (long double) for the two forms"""
    mask_x, mask_y = np.ascontiguousarray(mask_x, dtype=np.uint8), np.ascontiguousarray(mask_y, dtype=np.uint8)
    Mx, My, ld = int(mask_x.sum()), int(mask_y.sum()), np.longdouble
    acc = {name: np.zeros(_raw_shape(name, mask_x.size, Mx, My), dtype=ld) for name in _SUMS + _LAST}
    acc.update(mask_x=mask_x, mask_y=mask_y, w=SS.grid_weights(), corr_terms_all=[], **{k: 0 for k in _COUNTS})
    return acc


def equivalents(pi_a, pi_b):
    """(e, clamped): the equipercentile equivalents on B's scale of A's scores 0 .. M_A (the header's percentile-rank form),
    in the dtype of the inputs, and how many cells found no t with F_B[t] > P"""
    dt = pi_a.dtype
    half = dt.type(0.5)
    Fa, Fb = np.cumsum(pi_a), np.cumsum(pi_b)                # sequential, ascending score
    P = np.concatenate([[dt.type(0)], Fa[:-1]]) + pi_a * half
    t = np.searchsorted(Fb, P, side="right")                 # the smallest t with F_B[t] > P
    none = t >= pi_b.size
    tc = np.minimum(t, pi_b.size - 1)
    below = np.where(tc > 0, Fb[np.maximum(tc - 1, 0)], dt.type(0))
    with np.errstate(invalid="ignore", divide="ignore"):
        e = (tc.astype(dt) - half) + (P - below) / pi_b[tc]
    e = np.where(none, dt.type(pi_b.size - 1) + half, e)
    return e, int(none.sum())


def accumulate(acc, fstar):
    """Add one draw's f* (1001 x m, float64) to the accumulators `acc`: the header's rules, one statement each."""
    fstar = np.asarray(fstar, dtype=np.float64)
    fx, fy = fstar[:, np.flatnonzero(acc["mask_x"])], fstar[:, np.flatnonzero(acc["mask_y"])]
    if np.isnan(fx).any() or np.isnan(fy).any():            # a NaN in a column of either form: the draw is skipped whole
        acc["skipped"] += 1
        return
    AX, TX, VX = SS.draw_rows(fx)
    AY, TY, VY = SS.draw_rows(fy)
    w = acc["w"].astype(np.longdouble)
    # grid points with equal rows in both forms are contracted once, with their weights added up (all in long double)
    _, first, inv = np.unique(np.concatenate([fx, fy], axis=1), axis=0, return_index=True, return_inverse=True)
    wu = np.zeros(first.size, dtype=np.longdouble)
    np.add.at(wu, np.asarray(inv).reshape(-1), w)
    with np.errstate(under="ignore"):
        J = (wu[:, None] * AX[first]).T @ AY[first]
        pix, piy = (w[:, None] * AX).sum(axis=0), (w[:, None] * AY).sum(axis=0)
    eyx, c1 = equivalents(pix, piy)
    exy, c2 = equivalents(piy, pix)
    acc["joint_sum"] += J
    for k, v in (("pix", pix), ("piy", piy), ("eyx", eyx), ("exy", exy)):
        acc[k + "_sum"] += v
        acc[k + "_sumsq"] += v * v
    acc["eq_clamped"] += c1 + c2
    acc["draws"] += 1
    ax, bx, ay, by, c = (w * TX).sum(), (w * (VX + TX * TX)).sum(), (w * TY).sum(), (w * (VY + TY * TY)).sum(), (w * (TX * TY)).sum()
    terms = np.array([ax, bx, ay, by, c], dtype=np.longdouble)
    acc["corr_terms_all"].append(terms.astype(np.float64))
    vx, vy = bx - ax * ax, by - ay * ay
    if vx > 0 and vy > 0:
        r = (c - ax * ay) / np.sqrt(vx * vy)
        acc["corr"] += np.array([r, r * r])
        acc["corr_draws"] += 1
    else:
        acc["corr_skipped"] += 1
    acc.update(corr_terms=terms, last_joint=J, last_pix=pix, last_piy=piy, last_eyx=eyx, last_exy=exy)


def add(a, b) -> dict:
    """a + b (chains pooled in order); the masks and w are a's, the last_* arrays and corr_terms b's"""
    out = dict(a)
    for k in _SUMS + _COUNTS:
        out[k] = a[k] + b[k]
    out["corr_terms_all"] = a["corr_terms_all"] + b["corr_terms_all"]
    for k in _LAST:
        out[k] = b[k]
    return out


def from_draws(fstar_draws, x, y, probs=DEFAULT_PROBS, cuts=None) -> dict:
    """The NumPy statement of the header over fetched f*.  fstar_draws: one chain's f* (S x 1001 x m) or a sequence of chains'
    (there are no signs: theta -> -theta changes nothing here).  Every recursion, sum and quotient runs in long double and is
    returned rounded to float64; "corr_terms_all" lists, per counted draw, the correlation's five sums."""
    chains = [fstar_draws] if isinstance(fstar_draws, np.ndarray) and fstar_draws.ndim == 3 else list(fstar_draws)
    pooled = None
    for ch in chains:
        ch = np.asarray(ch, dtype=np.float64)
        if ch.ndim != 3 or ch.shape[1] != NGRID:
            raise ValueError("from_draws: a chain's f* is S x 1001 x m")
        acc = zeros(*form_masks(x, y, ch.shape[2]))
        for f in ch:
            accumulate(acc, f)
        pooled = acc if pooled is None else add(pooled, acc)
    with np.errstate(under="ignore"):
        raw = {name: (np.asarray(pooled[name], dtype=np.float64) if pooled[name].dtype == np.longdouble else pooled[name])
               for name, _ in EQUATE_RAW}
    out = finish(raw, probs, cuts, *(pooled[k] for k in _COUNTS))
    out["corr_terms_all"] = np.array(pooled["corr_terms_all"], dtype=np.float64).reshape(-1, 5)
    return out
