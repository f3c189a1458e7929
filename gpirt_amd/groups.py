"""Group posteriors without stored draws: how far apart the groups of respondents lie on theta, how much they overlap, who their
medians are, on which items they take opposite sides and who votes least with their own group (include/gpirt_hip.h, "group
posteriors": gpirt_groups_check, gpirt_sampler_groups_*, gpirt_groups_combine; csrc/groups.hip).

Per counted draw the device forms two sets of tables -- part A from theta alone (a histogram per group on the grid and exact
integer functionals of it), part B from one pass over f + mu (the groups' expected yes counts per item in fixed point, then
every respondent's agreement with their group's side on the contested items) -- and adds them to accumulators in a fixed order.
`latent_tables`, `latent_draw_stats`, `votes_tables`, `votes_draw_stats` and `loyalty_tables` are the NumPy statement of one
draw, `from_tables` of the accumulators, `pool` of gpirt_groups_combine's pooling, `finish` of the outputs; `from_draws` strings
them together over stored draws.  `struct` / `result` wrap the C struct, `combine` pools chains' state blocks and `run` drives
the stage API for C chains in one call.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import (GROUPS_LAST, GROUPS_MAX_G, GROUPS_MAX_M, GROUPS_MAX_N, GROUPS_MAX_TOP, GROUPS_MED_BINS, GROUPS_RAW, GROUPS_TAG,
                   check)

DEFAULT_TOP = 20
NGRID, CENTRE = 1001, 500
FIX = 2.0 ** 44
MEDIAN_PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)
_DT = {"u8": np.uint64, "u4": np.uint32, "f8": np.float64, "i8": np.int64, "i1": np.int8, "u1": np.uint8}
LATENT_RAW = tuple(r[0] for r in GROUPS_RAW[:18])
VOTES_RAW = tuple(r[0] for r in GROUPS_RAW[18:])
COUNTERS = ("latent_draws", "latent_skipped", "votes_draws", "votes_skipped")


# ---------------------------------------------------------------------------------------------------- the contract ---
def check_top(top):
    if isinstance(top, bool) or not isinstance(top, (int, np.integer)) or not 1 <= int(top) <= GROUPS_MAX_TOP:
        raise ValueError(f"groups: top must be an integer in 1 .. {GROUPS_MAX_TOP} (got {top!r})")
    return int(top)


def check_groups(groups, n, m=None):
    """The codes as int32 and G = the largest code + 1, by gpirt_groups_check's rule: one code per respondent, -1 (left out) or
    0 .. G - 1, 2 <= G <= 8, every group with a member, n <= 65534, m <= 4096.  Each refusal is a ValueError that says which."""
    if groups is None:
        raise ValueError("groups: no group codes given")
    a = np.asarray(groups)
    if a.ndim != 1 or a.shape[0] != int(n):
        raise ValueError(f"groups: one code per respondent is needed ({int(n)}), got an array of shape {a.shape}")
    if a.dtype.kind not in "iu" or a.dtype == np.bool_:
        if a.dtype.kind != "f" or not np.all(np.isfinite(a)) or not np.all(a == np.rint(a)):
            raise ValueError("groups: the codes must be integers")
    if int(n) < 1 or int(n) > GROUPS_MAX_N:
        raise ValueError(f"groups: n = {int(n)} respondents, 1 .. {GROUPS_MAX_N} are taken")
    if m is not None and not 1 <= int(m) <= GROUPS_MAX_M:
        raise ValueError(f"groups: m = {int(m)} items, 1 .. {GROUPS_MAX_M} are taken")
    codes = a.astype(np.int64)
    if codes.min() < -1:
        raise ValueError(f"groups: the code {int(codes.min())} is below -1 (-1 = left out)")
    G = int(codes.max()) + 1
    if G < 2 or G > GROUPS_MAX_G:
        raise ValueError(f"groups: {G} groups given, 2 .. {GROUPS_MAX_G} are taken")
    for g in range(G):
        if not np.any(codes == g):
            raise ValueError(f"groups: group {g} has no member")
    return np.ascontiguousarray(codes, dtype=np.int32), G


def pairs(G: int):
    """The pairs (g, h), g < h, in lexicographic order: the pair axis of every per-pair array."""
    return [(g, h) for g in range(G) for h in range(g + 1, G)]


def group_sizes(codes, G: int) -> np.ndarray:
    """n_g for g = 0 .. G - 1 and, at index G, the number of included respondents (int64)."""
    codes = np.asarray(codes)
    return np.array([np.sum(codes == g) for g in range(G)] + [np.sum(codes >= 0)], dtype=np.int64)


def raw_shape(key: str, n: int, m: int, G: int):
    P = G * (G - 1) // 2
    return {"g1k": (G + 1, NGRID), "g1m": (G + 1, GROUPS_MED_BINS), "6p": (6, P), "p": (P,), "g1": (G + 1,), "g": (G,), "n": (n,),
            "m": (m,), "pm": (P, m), "gm": (G, m), "stats": (3 * (G + 1) + 3 * P,), "4": (4,), "9": (GROUPS_MAX_G + 1,)}[key]


def grid_k(theta) -> np.ndarray:
    """theta's grid index k (theta bit for bit -5 + 0.01 k), -1 off the grid: csrc/kernels.h grid_index."""
    t = np.asarray(theta, dtype=np.float64)
    with np.errstate(all="ignore"):
        k = np.rint((t + 5.0) * 100.0)
        ok = (k >= 0.0) & (k <= NGRID - 1.0) & (-5.0 + k * 0.01 == t)
    return np.where(ok, k, -1.0).astype(np.int64)


# ---------------------------------------------------------------------------------------------------- one draw: part A ---
def u2_from_hist(Hg, Hh) -> int:
    """U2 = sum_k H_g[k] (2 less_h[k] + H_h[k]) from two rows of the histogram (what the device forms)."""
    Hg, Hh = np.asarray(Hg, dtype=np.int64), np.asarray(Hh, dtype=np.int64)
    less = np.concatenate([[0], np.cumsum(Hh)[:-1]])
    return int(np.sum(Hg * (2 * less + Hh)))


def latent_tables(theta, codes, G: int):
    """Part A's integer tables of one draw, or None when an included respondent is off the grid (the draw is skipped): hist
    ((G + 1) x 1001 uint32), c1, c2, med2 (G + 1, int64), w, ov (P, int64) and k (n, int64; -1 for a left-out respondent).
    U2 is counted by the O(n^2) pair definition, not from the histogram."""
    codes = np.asarray(codes)
    n = codes.shape[0]
    inc = codes >= 0
    k = np.full(n, -1, dtype=np.int64)
    k[inc] = grid_k(np.asarray(theta, dtype=np.float64)[inc])
    if np.any(k[inc] < 0):
        return None
    rows = [k[codes == g] for g in range(G)] + [k[inc]]
    hist = np.stack([np.bincount(r, minlength=NGRID) for r in rows]).astype(np.uint32)
    c1 = np.array([np.sum(r - CENTRE) for r in rows], dtype=np.int64)
    c2 = np.array([np.sum((r - CENTRE) ** 2) for r in rows], dtype=np.int64)
    med2 = np.zeros(G + 1, dtype=np.int64)
    for g, r in enumerate(rows):
        srt, ng = np.sort(r), r.shape[0]
        med2[g] = srt[(ng + 1) // 2 - 1] + srt[ng // 2]
    w, ov = [], []
    for g, h in pairs(G):
        kg, kh = rows[g], rows[h]
        u2 = 2 * int(np.sum(kg[:, None] > kh[None, :])) + int(np.sum(kg[:, None] == kh[None, :]))
        w.append(u2 - kg.shape[0] * kh.shape[0])
        ov.append(int(np.sum(np.minimum(hist[g].astype(np.int64) * kh.shape[0], hist[h].astype(np.int64) * kg.shape[0]))))
    return dict(hist=hist, c1=c1, c2=c2, med2=med2, w=np.array(w, dtype=np.int64), ov=np.array(ov, dtype=np.int64), k=k)


def latent_draw_stats(tab, codes, G: int) -> dict:
    """Everything part A derives from a draw's integer tables (tab: latent_tables's dict, or the device's own tables with k
    beside them), in the header's fp64 order: mean, var, sd (G + 1), a, overlap, d (P; d NaN where the pooled variance is 0),
    mean_order, med_order (P, the sign of g against h), cover (n, bool), share (n) and latent_stats (the device's vector)."""
    codes = np.asarray(codes)
    n = codes.shape[0]
    ng = group_sizes(codes, G)
    c1, c2 = np.asarray(tab["c1"], dtype=np.int64), np.asarray(tab["c2"], dtype=np.int64)
    med2 = np.asarray(tab["med2"], dtype=np.int64)
    f8 = lambda a: np.asarray(a).astype(np.float64)                              # noqa: E731
    mean = f8(c1) / f8(ng)
    var = f8(ng * c2 - c1 * c1) / f8(ng * ng)
    sd = np.sqrt(var)
    pr = pairs(G)
    gi, hi = np.array([p[0] for p in pr]), np.array([p[1] for p in pr])
    nn = f8(ng[gi] * ng[hi])
    a = f8(tab["w"]) / nn
    overlap = f8(tab["ov"]) / nn
    pooled = (f8(ng[gi]) * var[gi] + f8(ng[hi]) * var[hi]) / (f8(ng[gi]) + f8(ng[hi]))
    with np.errstate(all="ignore"):
        d = np.where(pooled == 0.0, np.nan, (mean[gi] - mean[hi]) / np.sqrt(pooled))
    mean_order = np.sign(c1[gi] * ng[hi] - c1[hi] * ng[gi]).astype(np.int64)
    med_order = np.sign(med2[gi] - med2[hi]).astype(np.int64)
    hist = np.asarray(tab["hist"]).astype(np.int64)
    k = np.asarray(tab["k"], dtype=np.int64)
    cover, share = np.zeros(n, dtype=bool), np.zeros(n)
    for g in range(G):
        idx = np.nonzero(codes == g)[0]
        less_all = np.concatenate([[0], np.cumsum(hist[g])[:-1]])
        less, eq = less_all[k[idx]], hist[g][k[idx]]
        q1, q2 = (ng[g] + 1) // 2, ng[g] // 2 + 1
        c = ((less < q1) & (q1 <= less + eq)).astype(np.int64) + ((less < q2) & (q2 <= less + eq)).astype(np.int64)
        cover[idx] = c > 0
        with np.errstate(all="ignore"):
            share[idx] = np.where(c > 0, f8(c) / f8(2 * eq), 0.0)
    return dict(mean=mean, var=var, sd=sd, a=a, overlap=overlap, d=d, mean_order=mean_order, med_order=med_order, cover=cover,
                share=share, latent_stats=np.concatenate([mean, var, sd, a, overlap, d]))


# ---------------------------------------------------------------------------------------------------- one draw: part B ---
def cell_pq(g):
    """p and q of g = f + mu by the PPC's expression (csrc/ppc.hip, cell_terms): e = exp(-|g|), p = 1 / (1 + e) or e / (1 + e)."""
    g = np.asarray(g, dtype=np.float64)
    with np.errstate(all="ignore"):
        e = np.exp(-np.abs(g))
        big, small = 1.0 / (1.0 + e), e / (1.0 + e)
    return np.where(g >= 0.0, big, small), np.where(g >= 0.0, small, big)


def votes_tables(g, codes, G: int):
    """e (G x m, uint64): per group and item the sum over the members of rint(p 2^44); None when a cell of an included
    respondent is NaN (the draw is skipped).  +-inf is taken: p is 0 or 1."""
    g, codes = np.asarray(g, dtype=np.float64), np.asarray(codes)
    if np.any(np.isnan(g[codes >= 0])):
        return None
    p, _ = cell_pq(np.where((codes >= 0)[:, None], g, 0.0))           # (a left-out row may hold anything)
    t = np.rint(p * FIX).astype(np.uint64)
    return np.stack([t[codes == gr].sum(axis=0, dtype=np.uint64) for gr in range(G)])


def votes_draw_stats(e, sizes) -> dict:
    """Everything one draw's e determines: side (G x m, int8), support, rice (G x m), gap (P x m), split (P x m, bool),
    contested (m, bool), n_split (P) and c_g (G), int64."""
    e = np.asarray(e, dtype=np.uint64)
    G, m = e.shape
    ng = np.asarray(sizes, dtype=np.int64)[:G]
    side = np.sign(2 * e.astype(np.int64) - (ng << 44)[:, None]).astype(np.int8)
    support = e.astype(np.float64) / (ng.astype(np.float64) * FIX)[:, None]
    rice = np.abs(2.0 * support - 1.0)
    pr = pairs(G)
    gap = np.stack([support[g] - support[h] for g, h in pr])
    split = np.stack([side[g].astype(np.int64) * side[h] == -1 for g, h in pr])
    contested = split.any(axis=0)
    c_g = np.array([np.sum(contested & (side[g] != 0)) for g in range(G)], dtype=np.int64)
    return dict(side=side, support=support, rice=rice, gap=gap, split=split, contested=contested,
                n_split=split.sum(axis=1).astype(np.int64), c_g=c_g)


def loyalty_tables(g, y, codes, side, contested) -> dict:
    """Per respondent, over the contested items on which their group takes a side: loy (uint64, the sum of rint(x 2^44), x = p
    for side +1 and q for side -1), obs_with and obs_n (uint32: the observed answers on the group's side, and their number).
    A left-out respondent holds zeros."""
    g, y, codes = np.asarray(g, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(codes)
    side, contested = np.asarray(side).astype(np.int64), np.asarray(contested).astype(bool)
    n = codes.shape[0]
    loy, ow, on = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    for gr in range(side.shape[0]):
        idx = np.nonzero(codes == gr)[0]
        cols = np.nonzero(contested & (side[gr] != 0))[0]
        if idx.size == 0 or cols.size == 0:
            continue
        sub = g[np.ix_(idx, cols)]
        p, q = cell_pq(sub)
        up = side[gr][cols] > 0
        loy[idx] = np.rint(np.where(up[None, :], p, q) * FIX).astype(np.uint64).sum(axis=1, dtype=np.uint64)
        ys = y[np.ix_(idx, cols)]
        seen = ~np.isnan(ys)
        on[idx] = seen.sum(axis=1)
        ow[idx] = (seen & ((ys > 0.0) == up[None, :])).sum(axis=1)
    return dict(loy=loy, obs_with=ow, obs_n=on)


# ---------------------------------------------------------------------------------------------------- the accumulators ---
def empty_raw(n: int, m: int, G: int) -> dict:
    raw = {name: np.zeros(raw_shape(key, n, m, G), dtype=_DT[dt]) for name, dt, key in GROUPS_RAW}
    raw.update({c: 0 for c in COUNTERS})
    return raw


def from_tables(draws, codes, G: int, m: int) -> dict:
    """The accumulators of one chain from its draws' tables, each fp64 cell added to once per counted draw, the value and then
    its square, in draw order.  draws: one dict per draw with "latent" (None: skipped; else latent_tables's and
    latent_draw_stats's keys in one dict) and "votes" (None: skipped; else e, votes_draw_stats's and loyalty_tables's keys)."""
    codes = np.asarray(codes)
    n = codes.shape[0]
    raw = empty_raw(n, m, G)
    inc = np.nonzero(codes >= 0)[0]
    P = G * (G - 1) // 2
    pi = np.arange(P)

    def add(name, v, where=None):
        s, q = raw[name + "_sum"], raw[name + "_sq"]
        if where is None:
            s += v
            q += v * v
        else:
            s[where] = s[where] + v[where]
            q[where] = q[where] + v[where] * v[where]

    for dr in draws:
        la, vo = dr.get("latent"), dr.get("votes")
        if la is None:
            raw["latent_skipped"] += 1
        else:
            raw["latent_draws"] += 1
            H = np.asarray(la["hist"]).astype(np.uint64)
            raw["dens_sum"] += H
            raw["dens_sq"] += H * H
            raw["medhist"][np.arange(G + 1), np.asarray(la["med2"], dtype=np.int64)] += 1
            raw["order"][1 - np.asarray(la["mean_order"]), pi] += 1
            raw["order"][4 - np.asarray(la["med_order"]), pi] += 1
            raw["ov_sum"] += np.asarray(la["ov"]).astype(np.uint64)
            add("mean", la["mean"])
            add("sd", la["sd"])
            add("a", la["a"])
            add("ovl", la["overlap"])
            ok = ~np.isnan(la["d"])
            raw["d_undefined"] += (~ok).astype(np.uint32)
            add("d", np.where(ok, la["d"], 0.0), ok)
            raw["median_cover"] += np.asarray(la["cover"]).astype(np.uint32)
            cv = np.asarray(la["cover"]).astype(bool)
            raw["median_share"][cv] = raw["median_share"][cv] + la["share"][cv]
        if vo is None:
            raw["votes_skipped"] += 1
        else:
            raw["votes_draws"] += 1
            raw["split_count"] += np.asarray(vo["split"]).astype(np.uint32)
            ns = np.asarray(vo["n_split"]).astype(np.uint64)
            raw["nsplit_sum"] += ns
            raw["nsplit_sq"] += ns * ns
            add("support", vo["support"])
            add("rice", vo["rice"])
            add("gap", vo["gap"])
            cg = np.asarray(vo["c_g"], dtype=np.int64)
            raw["loy_undefined"] += (cg == 0).astype(np.uint32)
            raw["obs_with_sum"][inc] += np.asarray(vo["obs_with"]).astype(np.uint64)[inc]
            raw["obs_n_sum"][inc] += np.asarray(vo["obs_n"]).astype(np.uint64)[inc]
            ci = cg[codes[inc]]
            have = np.zeros(n, dtype=bool)
            have[inc] = ci > 0
            loyalty = np.zeros(n)
            with np.errstate(all="ignore"):
                loyalty[inc] = np.where(ci > 0, np.asarray(vo["loy"]).astype(np.float64)[inc] / (ci.astype(np.float64) * FIX), 0.0)
            add("loy", loyalty, have)
    return raw


def reflect_raw(raw: dict) -> dict:
    """A chain's accumulators as they enter with sign -1 (theta -> -theta): dens_sum, dens_sq and medhist reversed along the grid,
    mean_sum, a_sum and d_sum negated, the > and < order counts swapped; everything else is even and kept."""
    out = dict(raw)
    for k in ("dens_sum", "dens_sq", "medhist"):
        out[k] = raw[k][:, ::-1].copy()
    for k in ("mean_sum", "a_sum", "d_sum"):
        out[k] = -raw[k]
    out["order"] = raw["order"][[2, 1, 0, 5, 4, 3]].copy()
    return out


def pool(raws, signs=None) -> dict:
    """gpirt_groups_combine's pooling: integers add, fp64 sums add in chain order, a chain with sign -1 enters reflected."""
    signs = [1] * len(raws) if signs is None else [int(s) for s in signs]
    if len(signs) != len(raws) or any(s not in (1, -1) for s in signs):
        raise ValueError("groups: signs must be one +1 or -1 per chain")
    out = None
    for r, sg in zip(raws, signs):
        r = reflect_raw(r) if sg < 0 else r
        if out is None:
            out = {k: (v.copy() if isinstance(v, np.ndarray) else int(v)) for k, v in r.items()}
        else:
            for k, v in r.items():
                out[k] = out[k] + v
    return out


def _pair_matrix(v, G, anti, diag):
    out = np.full((G, G), diag, dtype=np.float64)
    for p, (g, h) in enumerate(pairs(G)):
        out[g, h] = v[p]
        out[h, g] = -v[p] if anti else v[p]
    return out


def top_lists(raw, codes, G: int, top: int):
    """most_split (per pair the `top` items by split count, ties to the lowest j) and least_loyal (the `top` included
    respondents by mean loyalty, ascending, ties to the lowest i), as gpirt_groups_combine orders them."""
    codes = np.asarray(codes)
    V = raw["votes_draws"]
    m = raw["split_count"].shape[1]
    most = []
    for p in range(len(pairs(G))):
        sc = raw["split_count"][p].astype(np.int64)
        order = np.argsort(-sc, kind="stable")[:top]
        items = np.full(top, -1, dtype=np.int64)
        ps = np.full(top, np.nan)
        items[:order.size] = order
        if V > 0:
            ps[:order.size] = sc[order] / np.float64(V)
        most.append(dict(items=items, p_split=ps))
    den = np.where(codes >= 0, V - raw["loy_undefined"].astype(np.int64)[np.maximum(codes, 0)], 0)
    with np.errstate(all="ignore"):
        loyalty = np.where(den > 0, raw["loy_sum"] / den.astype(np.float64), np.nan)
    cand = np.nonzero(den > 0)[0]
    order = cand[np.argsort(loyalty[cand], kind="stable")][:top]
    resp, lv = np.full(top, -1, dtype=np.int64), np.full(top, np.nan)
    resp[:order.size] = order
    lv[:order.size] = loyalty[order]
    return most, dict(respondents=resp, loyalty=lv), loyalty, den


def finish(raw, codes, G: int, top=DEFAULT_TOP, lists=None) -> dict:
    """The outputs from pooled accumulators (fp64; a ratio without draws is NaN).  Per-group arrays of part A carry G + 1 rows,
    the last one for all included respondents; per-pair matrices are G x G (p_superior[g, h] = P(theta_g > theta_h) with ties
    as a half, d and the order probabilities antisymmetric in the obvious way); gap, gap_sd, p_split, n_split_* and most_split
    are indexed by the pair number of pairs(G).  lists: gpirt_groups_combine's own two lists, taken in place of NumPy's."""
    top = check_top(top)
    codes = np.asarray(codes)
    ng = group_sizes(codes, G)
    L, V = np.float64(raw["latent_draws"]), np.float64(raw["votes_draws"])
    sdv = lambda s, q, cnt: np.sqrt(np.maximum(q / cnt - (s / cnt) ** 2, 0.0))    # noqa: E731
    out = {c: int(raw[c]) for c in COUNTERS}
    out.update(G=G, group_size=ng, pairs=pairs(G), raw=raw)
    with np.errstate(all="ignore"):
        out["mean"] = (raw["mean_sum"] / L) * 0.01
        out["mean_sd"] = sdv(raw["mean_sum"], raw["mean_sq"], L) * 0.01
        out["sd_mean"] = (raw["sd_sum"] / L) * 0.01
        out["sd_sd"] = sdv(raw["sd_sum"], raw["sd_sq"], L) * 0.01
        mq = np.full((len(MEDIAN_PROBS), G + 1), np.nan)
        if raw["latent_draws"] > 0:
            cum = np.cumsum(raw["medhist"].astype(np.int64), axis=1)
            for r, pr in enumerate(MEDIAN_PROBS):
                for g in range(G + 1):
                    mq[r, g] = (int(np.argmax(cum[g] >= pr * L)) - 2 * CENTRE) * 0.005
        out["median_quantiles"] = mq
        cell = (ng.astype(np.float64) * 0.01)[:, None]
        out["density"] = raw["dens_sum"].astype(np.float64) / L / cell
        out["density_sd"] = sdv(raw["dens_sum"].astype(np.float64), raw["dens_sq"].astype(np.float64), L) / cell
        a_mean, a_sd = raw["a_sum"] / L, sdv(raw["a_sum"], raw["a_sq"], L)
        out["p_superior"] = (1.0 + _pair_matrix(a_mean, G, True, 0.0)) / 2.0
        out["p_superior_sd"] = _pair_matrix(a_sd / 2.0, G, False, 0.0)
        out["overlap"] = _pair_matrix(raw["ovl_sum"] / L, G, False, 1.0)
        out["overlap_sd"] = _pair_matrix(sdv(raw["ovl_sum"], raw["ovl_sq"], L), G, False, 0.0)
        od = raw["order"].astype(np.float64)
        for name, r in (("p_mean_gt", 0), ("p_median_gt", 3)):
            mat = np.zeros((G, G))
            for p, (g, h) in enumerate(pairs(G)):
                mat[g, h], mat[h, g] = od[r, p] / L, od[r + 2, p] / L
            out[name] = mat
        dn = L - raw["d_undefined"].astype(np.float64)
        dn = np.where(dn > 0, dn, np.nan)
        out["d_mean"] = _pair_matrix(raw["d_sum"] / dn, G, True, 0.0)
        out["d_sd"] = _pair_matrix(sdv(raw["d_sum"], raw["d_sq"], dn), G, False, 0.0)
        out["d_undefined"] = raw["d_undefined"].astype(np.int64)
        out["p_group_median"] = raw["median_share"] / L
        out["p_median_cover"] = raw["median_cover"].astype(np.float64) / L
        out["support"] = raw["support_sum"] / V
        out["support_sd"] = sdv(raw["support_sum"], raw["support_sq"], V)
        out["rice"] = raw["rice_sum"] / V
        out["rice_sd"] = sdv(raw["rice_sum"], raw["rice_sq"], V)
        out["gap"] = raw["gap_sum"] / V
        out["gap_sd"] = sdv(raw["gap_sum"], raw["gap_sq"], V)
        out["p_split"] = raw["split_count"].astype(np.float64) / V
        out["n_split_mean"] = raw["nsplit_sum"].astype(np.float64) / V
        out["n_split_sd"] = sdv(raw["nsplit_sum"].astype(np.float64), raw["nsplit_sq"].astype(np.float64), V)
        most, least, loyalty, den = top_lists(raw, codes, G, top)
        out["loyalty"] = loyalty
        out["loyalty_sd"] = np.where(den > 0, sdv(raw["loy_sum"], raw["loy_sq"], np.where(den > 0, den, 1).astype(np.float64)), np.nan)
        out["loy_undefined"] = raw["loy_undefined"].astype(np.int64)
        on = raw["obs_n_sum"].astype(np.float64)
        out["obs_loyalty"] = np.where(on > 0, raw["obs_with_sum"].astype(np.float64) / np.where(on > 0, on, 1.0), np.nan)
    out["most_split"], out["least_loyal"] = (most, least) if lists is None else lists
    return out


def draw_tables(theta, g, y, codes, G: int) -> dict:
    """One draw's tables for from_tables: {"latent": ..., "votes": ...}, each None where its part skips the draw."""
    sizes = group_sizes(codes, G)
    la = latent_tables(theta, codes, G)
    if la is not None:
        la.update(latent_draw_stats(la, codes, G))
    vo = None
    e = votes_tables(g, codes, G)
    if e is not None:
        vo = dict(e=e)
        vo.update(votes_draw_stats(e, sizes))
        vo.update(loyalty_tables(g, y, codes, vo["side"], vo["contested"]))
    return dict(latent=la, votes=vo)


def from_draws(theta_draws, g_draws, y, groups, signs=None, top=DEFAULT_TOP) -> dict:
    """The NumPy statement of the header over stored draws: theta_draws (C x S x n, or S x n for one chain), g_draws (C x S x n x
    m, g = f + mu), the data y (n x m, +1 / -1 / NaN), the group codes and one sign per chain (None: all +1).  Returns finish()'s
    dict; its "raw" holds the pooled accumulators and "chain_raw" every chain's own."""
    y = np.asarray(y, dtype=np.float64)
    n, m = y.shape
    codes, G = check_groups(groups, n, m)
    th, gd = np.asarray(theta_draws, dtype=np.float64), np.asarray(g_draws, dtype=np.float64)
    if th.ndim == 2:
        th, gd = th[None], gd[None]
    raws = [from_tables([draw_tables(th[c, t], gd[c, t], y, codes, G) for t in range(th.shape[1])], codes, G, m)
            for c in range(th.shape[0])]
    out = finish(pool(raws, signs), codes, G, top)
    out["chain_raw"] = raws
    return out


# ------------------------------------------------------------------------------------------------------ the device ---
def struct(n: int, m: int, G: int, top: int = DEFAULT_TOP):
    """A gpirt_groups asking for every array, and the host arrays behind it (kept alive by the caller)."""
    r = _lib.Groups()
    r.top = check_top(top)
    P = G * (G - 1) // 2
    arrays = {}
    for k, (name, dt, key) in enumerate(GROUPS_RAW):
        arrays[name] = np.zeros(raw_shape(key, n, m, G), dtype=_DT[dt])
        r.raw[k] = arrays[name].ctypes.data
    arrays["most_split_items"], arrays["most_split_p"] = np.zeros((P, r.top), dtype=np.int64), np.zeros((P, r.top))
    arrays["least_loyal"], arrays["least_loyal_loyalty"] = np.zeros(r.top, dtype=np.int64), np.zeros(r.top)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    r.most_split_items, r.most_split_p = arrays["most_split_items"].ctypes.data_as(ip), arrays["most_split_p"].ctypes.data_as(dp)
    r.least_loyal, r.least_loyal_loyalty = arrays["least_loyal"].ctypes.data_as(ip), arrays["least_loyal_loyalty"].ctypes.data_as(dp)
    return r, arrays


def result(r, arrays, codes) -> dict:
    """The dict of Sampler.groups(), combine() and run() from a filled gpirt_groups: finish() of the pooled accumulators with the
    library's own two lists."""
    raw = {name: arrays[name] for name, _, _ in GROUPS_RAW}
    raw.update({c: int(getattr(r, c)) for c in COUNTERS})
    G, top = int(r.G), int(r.top)
    most = [dict(items=arrays["most_split_items"][p], p_split=arrays["most_split_p"][p]) for p in range(int(r.pairs))]
    least = dict(respondents=arrays["least_loyal"], loyalty=arrays["least_loyal_loyalty"])
    out = finish(raw, codes, G, top, lists=(most, least))
    out.update(n=int(r.n), m=int(r.m), chains=int(r.chains), included=int(r.included))
    return out


def state_header(state) -> dict:
    """The header of a group posterior state block (a device tensor of int64)."""
    w = _lib.header_words(state, 32)
    names = ("tag", "version", "n", "m", "G", "latent_draws", "latent_skipped", "votes_draws", "votes_skipped")
    out = {k: int(w[i]) for i, k in enumerate(names)}
    out["group_size"] = [int(v) for v in w[16:16 + GROUPS_MAX_G + 1]]
    return out


def state_codes(state, n: int) -> np.ndarray:
    """The group codes a state block carries (int8 -> int32)."""
    words = (n + 15) // 16 * 2
    return state[32:32 + words].detach().cpu().numpy().view(np.int8)[:n].astype(np.int32)


def combine(handle, states, signs=None, top=DEFAULT_TOP) -> dict:
    """gpirt_groups_combine over the state blocks `states` (device tensors, or Samplers with groups_enable() on, all on handle's
    device and with the same codes).  signs: None, or one +1 / -1 per chain (-1: the chain enters reflected, theta -> -theta;
    `1 - 2 * diagnostics["reflected"]` of gpirt_amd.chains.combine)."""
    lib = _lib.load()
    tensors, nc, ptrs = _lib.state_ptrs(states, "groups_state")
    hdr = state_header(tensors[0])
    if hdr["tag"] != GROUPS_TAG:
        raise ValueError("groups.combine: state 0 is not a group posterior state block")
    r, arrays = struct(hdr["n"], hdr["m"], hdr["G"], top)
    sg = None
    if signs is not None:
        if len(signs) != nc:
            raise ValueError(f"groups.combine: {len(signs)} signs for {nc} states")
        sg = (C.c_int * nc)(*[int(x) for x in signs])
    check(lib.gpirt_groups_combine(handle.ptr, nc, ptrs, sg, C.byref(r)))
    return result(r, arrays, state_codes(tensors[0], hdr["n"]))


# ------------------------------------------------------------------------------------------------ one call for C chains ---
def run(y, sample_iterations, burn_iterations, groups=None, chains=1, seed=1, *, top=DEFAULT_TOP, align=True, theta_init=None,
        preset="fast", handle=None, consistent=False, **sampler_kw) -> dict:
    """`chains` chains of the stage-driven Sampler, one after the other, each with the group posteriors and the DIAG summaries
    on (gpirt_amd.acf.run's loop); chain c runs with the seed chain_seed(seed, c) from gpirtMCMC(chains=...)'s default init.
    The signs are the ones gpirt_amd.chains.combine decides for the same chains (align=False: none).  Returns combine()'s dict
    with "diagnostics" and "reflected" beside it.  consistent=True: every iteration is Sampler.step(consistent=True)
    (gpirt_amd.consistent); "consistent" in the result names it."""
    from . import chains as CH
    from .ops import Handle
    from .sampler import Sampler
    y = np.asfortranarray(np.asarray(y, dtype=np.float64))
    S, B, nc = int(sample_iterations), int(burn_iterations), int(chains)
    codes, _ = check_groups(groups, y.shape[0], y.shape[1])
    top = check_top(top)
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
            s.groups_enable(codes, top=top)
            for it in range(S + B):
                s.step(consistent=consistent)
                if it >= B:
                    s.accumulate_irf()
                    s.summary_accumulate()
                    s.groups_accumulate()
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


__all__ = ["check_groups", "check_top", "combine", "state_header", "run", "from_draws", "latent_tables", "latent_draw_stats",
           "votes_tables", "votes_draw_stats", "loyalty_tables", "from_tables", "pool", "finish", "pairs", "group_sizes",
           "GROUPS_LAST", "GROUPS_RAW"]
