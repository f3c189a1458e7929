"""PSIS-LOO on the device (csrc/loo.hip) against the NumPy statement of the header (gpirt_amd.loo.from_draws) inside
tests/_loo_bounds.py's bounds: constructed draws through Sampler.set("f") / set("mu") -- key patterns that evict on every draw,
never, tie across the cutoff --, chains pooled on the device (one of them never fills its heap), incomplete cells, the fit at
M = 135, a real chain through the stage API and gpirtMCMC(loo=...), the untouched chain and WAIC's lppd beside it.

Every comparison prints the largest used fraction of its bound ("MEASURED ..."); no figure from a device run is recorded here yet."""
import math
import os

import numpy as np
import pytest

import _loo_bounds as B

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
CODES = dict(yea=[1], nay=[-1], missing=[None])
MU = 0.25
SHAPES = {"37x5": (37, 5), "64x4": (64, 4)}
RUNS = [(1, 3), (1, 26), (1, 40), (1, 400), (3, 50), (4, 20), (8, 10)]          # (chains, draws per chain)


def make_y(n, m, seed, missing):
    rng = np.random.default_rng(seed)
    y = np.where(rng.uniform(size=(n, m)) < 0.6, 1.0, -1.0)
    if missing:
        y[rng.uniform(size=(n, m)) < 0.08] = np.nan
        y[n - 1, m - 1] = 1.0                                         # the odd last cell is observed
    return y


def pattern_keys(n, m, T, seed):
    """T x n x m keys; the cell's pattern is (i + j n) mod 5: ascending in draw order (every draw evicts), descending (nothing
    enters after the fill), constant, two values with ties straddling the cutoff, seeded normal"""
    rng = np.random.default_rng(seed)
    M = max(min(T // 5, math.isqrt(9 * T - 1) + 1), 0)
    s = np.arange(T, dtype=np.float64)
    keys = np.empty((T, n, m))
    for j in range(m):
        for i in range(n):
            c = i + j * n
            base = -3.0 + 0.37 * (c % 11)
            kind = c % 5
            if kind == 0:
                keys[:, i, j] = base + (6.0 / T) * s * (1.0 + 0.01 * (c % 7))
            elif kind == 1:
                keys[:, i, j] = base + 5.0 - (6.0 / T) * s * (1.0 + 0.01 * (c % 7))
            elif kind == 2:
                keys[:, i, j] = base
            elif kind == 3:
                nb = max(M // 2, 1) + (c % 3)                         # the upper value fills part of the tail only
                keys[:, i, j] = np.where((7 * np.arange(T)) % T < nb, base + 1.5, base)
            else:
                keys[:, i, j] = rng.normal(base, 1.5, T)
    return keys


def build_case(shape, C_, S, spoil=False):
    """(name, y, f per chain (C x S x n x m)); g = f + MU.  spoil: one cell sees a NaN f in one draw, another a key of 710"""
    n, m = SHAPES[shape]
    name = f"{shape}-C{C_}-S{S}" + ("-spoiled" if spoil else "")
    y = make_y(n, m, seed=n + S, missing=shape == "37x5")
    keys = pattern_keys(n, m, C_ * S, seed=C_ * 1000 + S)
    g = np.where(np.isnan(y)[None], 0.0, -np.nan_to_num(y)[None] * keys)
    f = g - MU
    cells = []
    if spoil:
        obs = np.argwhere(~np.isnan(y))
        (i0, j0), (i1, j1) = obs[3], obs[len(obs) // 2]
        f[S // 2, i0, j0] = np.nan
        f[S - 1, i1, j1] = -710.0 * y[i1, j1] - MU                    # (exact: f + MU is -+710, a key of 710)
        cells = [(int(i0), int(j0)), (int(i1), int(j1))]
    f = f.reshape(C_, S, n, m)
    B.register(name, y, [f[c] + MU for c in range(C_)])
    return name, y, f, cells


_RUNS = {}


def device_run(handle, shape, C_, S, spoil=False):
    """the case through the device, once: per chain a Sampler fed by set("f") after set("mu"), then loo.combine"""
    key = (shape, C_, S, spoil)
    if key in _RUNS:
        return _RUNS[key]
    from gpirt_amd import Sampler, loo
    name, y, f, cells = build_case(shape, C_, S, spoil)
    n, m = y.shape
    samplers = []
    for c in range(C_):
        s = Sampler(handle, y, np.zeros(n), rng="item", seed=5 + c, theta_stabilise=True)
        s.init()
        s.loo_enable(C_ * S)
        s.set("mu", np.full((n, m), MU))
        for d in range(S):
            s.set("f", f[c, d])
            s.loo_accumulate()
        samplers.append(s)
    single = dict(tail=samplers[0].loo_get("tail"), counts=samplers[0].loo_get("counts")) if C_ == 1 else None
    got = loo.combine(handle, samplers, top=8)
    for s in samplers:
        s.close()
    _RUNS[key] = (name, y, got, single, cells)
    return _RUNS[key]


def same_keys(got, want):
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.nan_to_num(got), np.nan_to_num(want))


# ------------------------------------------------------------------------------------------------ 1. the selection ---
@pytest.mark.parametrize("C_,S", RUNS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_selection_is_exact(handle, shape, C_, S):
    """the kept keys equal NumPy's K largest bit for bit (one chain: loo_get("tail"); several: after combine), the counters
    and p_sum are right and the evicted sums are the long-double sums of the very evicted values within (T + 8) eps"""
    name, y, got, single, _ = device_run(handle, shape, C_, S)
    want, _ = B.reference(name)
    T = C_ * S
    assert got["T"] == T and got["M"] == want["M"] and got["draws"] == T and got["chains"] == C_
    assert same_keys(got["raw"]["tail"], want["raw"]["tail"])
    if single is not None:
        assert same_keys(single["tail"], want["raw"]["tail"])
        assert single["counts"].tolist() == [y.shape[0], y.shape[1], T, want["M"], T, 1]
    obs = ~np.isnan(y)
    assert np.array_equal(got["raw"]["count"], np.where(obs, T, 0)) and not got["raw"]["nonfinite"].any()
    assert np.array_equal(got["raw"]["y"], np.nan_to_num(y).astype(np.int8))
    B.check_sums(name, got["raw"], T)
    assert got["cells_incomplete"] == 0 and got["n_obs"] == int(obs.sum())


def test_spoiled_cells_come_out_incomplete_and_only_they(handle):
    name, y, got, _, cells = device_run(handle, "37x5", 1, 40, spoil=True)
    want, _ = B.reference(name)
    (i0, j0), (i1, j1) = cells
    assert got["cells_incomplete"] == 2 and want["cells_incomplete"] == 2
    bad = np.zeros(y.shape, dtype=bool)
    bad[i0, j0] = bad[i1, j1] = True
    assert np.array_equal(np.isnan(got["pointwise"]["elpd_loo"]), bad | np.isnan(y))
    assert np.array_equal(got["raw"]["nonfinite"], bad.astype(np.int32))
    assert np.array_equal(got["raw"]["count"], np.where(np.isnan(y), 0, 40) - bad)
    assert same_keys(got["raw"]["tail"], want["raw"]["tail"])
    B.check_sums(name, got["raw"], 40)
    B.check_pointwise(name, got)


# ------------------------------------------------------------------------------------------------------ 2. the fit ---
def check_totals(got, y, T):
    """the totals, the sums and the worst cells against the host's own reduction of the device's pointwise arrays"""
    from gpirt_amd import loo
    host = loo.totals(got["pointwise"], y, T, top=len(got["worst"]["index"]))
    e = got["pointwise"]["elpd_loo"]
    N = max(host["n_obs"], 1)
    scale = float(np.nansum(np.abs(e))) if host["n_obs"] else 0.0
    for k in ("n_obs", "k_good", "k_bad", "k_very_bad", "unsmoothed", "cells_incomplete"):
        assert got[k] == host[k], k
    assert got["k_threshold"] == host["k_threshold"]
    for k, s in (("elpd_loo", scale), ("looic", 2 * scale), ("lppd", float(np.nansum(np.abs(got["pointwise"]["lppd"])))),
                 ("p_loo", float(np.nansum(np.abs(got["pointwise"]["p_loo"]))))):
        assert abs(got[k] - host[k]) <= (N + 8) * EPS * s, k
    if host["n_obs"] > 1:                                            # a sum of N squares around a mean within N eps
        assert got["se_elpd_loo"] == pytest.approx(host["se_elpd_loo"], rel=(N + 8) * 4 * EPS, abs=1e-300)
        assert got["se_looic"] == pytest.approx(2 * host["se_elpd_loo"], rel=(N + 8) * 4 * EPS, abs=1e-300)
    fin = ~np.isnan(e)
    col, row = np.where(fin, np.abs(e), 0).sum(axis=0), np.where(fin, np.abs(e), 0).sum(axis=1)
    assert (np.abs(got["item_elpd_loo"] - host["item_elpd_loo"]) <= (y.shape[0] + 8) * EPS * col).all()
    assert (np.abs(got["respondent_elpd_loo"] - host["respondent_elpd_loo"]) <= (y.shape[1] + 8) * EPS * row).all()
    for k in ("index", "row", "col"):
        assert np.array_equal(got["worst"][k], host["worst"][k]), k
    assert np.array_equal(got["worst"]["pareto_k"], host["worst"]["pareto_k"], equal_nan=True)


@pytest.mark.parametrize("C_,S", RUNS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_fit_against_from_draws(handle, shape, C_, S):
    name, y, got, _, _ = device_run(handle, shape, C_, S)
    B.check_pointwise(name, got)
    check_totals(got, y, C_ * S)


def test_fit_at_two_thousand_draws(handle):
    """16 x 3, 2000 seeded normal draws per cell, M = 135: no two cells tie in k, so the worst cells are the reference's"""
    from gpirt_amd import Sampler
    n, m, T = 16, 3, 2000
    rng = np.random.default_rng(2000)
    y = make_y(n, m, seed=9, missing=False)
    f = rng.normal(1.0, 1.2, (T, n, m)) * (1.0 + 0.05 * np.arange(n * m).reshape(m, n).T) - MU
    B.register("16x3-S2000", y, [f + MU], top=8)
    s = Sampler(handle, y, np.zeros(n), rng="item", seed=5, theta_stabilise=True)
    s.init()
    s.loo_enable(T)
    s.set("mu", np.full((n, m), MU))
    for d in range(T):
        s.set("f", f[d])
        s.loo_accumulate()
    got = s.loo(top=8)
    s.close()
    want, _ = B.reference("16x3-S2000")
    assert got["M"] == 135 and want["unsmoothed"] == 0 and got["unsmoothed"] == 0
    assert same_keys(got["raw"]["tail"], want["raw"]["tail"])
    B.check_sums("16x3-S2000", got["raw"], T)
    B.check_pointwise("16x3-S2000", got)
    check_totals(got, y, T)
    assert np.array_equal(got["worst"]["index"], want["worst"]["index"])


# ------------------------------------------------------------------------------------------------ 3. a real chain ---
def senate_slice():
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "senate116_y.npz"))
    y = d["y"].astype(np.float64)
    y[y == 0] = np.nan
    mixed = [j for j in range(y.shape[1]) if (y[:, j] == 1).sum() >= 10 and (y[:, j] == -1).sum() >= 10][:24]
    return np.asfortranarray(y[:100, mixed])


@pytest.fixture(scope="module")
def real_chain(handle):
    """2 chains of 60 draws after 20 of burn-in on a 100 x 24 slice of senate116, preset="fast": gpirtMCMC(loo=...) with the
    summaries and the PPC beside it, the same call without loo, and the stage API over the same chains with g kept per step"""
    from gpirt_amd import Sampler, _lib, gpirtMCMC, loo
    y = senate_slice()
    S, Bn, seed = 60, 20, 17
    inits = np.random.default_rng(4).normal(size=(2, y.shape[0]))
    kw = dict(vote_codes=CODES, theta_init=inits, preset="fast", seed=seed, chains=2, summaries=("waic",), ppc=True)
    res = gpirtMCMC(y, S, Bn, loo=dict(top=8), **kw)
    plain = gpirtMCMC(y, S, Bn, **kw)
    samplers, draws = [], []
    for c in range(2):
        s = Sampler(handle, y, inits[c], preset="fast", seed=_lib.chain_seed(seed, c))
        s.init()
        s.loo_enable(2 * S)
        ch = []
        for it in range(S + Bn):
            s.step()
            if it >= Bn:
                s.loo_accumulate()
                ch.append(s.get("f") + s.get("mu"))
        s.check()
        samplers.append(s)
        draws.append(np.stack(ch))
    blocks = [s.loo_state().cpu().numpy().tobytes() for s in samplers]
    stage = loo.combine(handle, samplers, top=8)
    for s in samplers:
        s.close()
    B.register("senate-100x24", y, draws, top=8)
    return dict(y=y, S=S, Bn=Bn, res=res, plain=plain, stage=stage, blocks=blocks, inits=inits, seed=seed)


def same_tree(a, b, path=()):
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            same_tree(a[k], b[k], path + (k,))
    elif isinstance(a, np.ndarray):
        assert a.tobytes() == b.tobytes(), path
    else:
        assert a == b or (a != a and b != b), path


def test_real_chain_equals_the_stage_api_and_the_statement(real_chain):
    res, stage = real_chain["res"]["loo"], real_chain["stage"]
    same_tree(res, stage)
    assert res["T"] == 120 and res["M"] == 24 and res["chains"] == 2 and res["cells_incomplete"] == 0
    want, _ = B.reference("senate-100x24")
    assert same_keys(res["raw"]["tail"], want["raw"]["tail"])
    B.check_sums("senate-100x24", res["raw"], 120)
    B.check_pointwise("senate-100x24", res)
    check_totals(res, real_chain["y"], 120)


def test_real_chain_is_untouched_by_loo(real_chain):
    res, plain = real_chain["res"], real_chain["plain"]
    assert "loo" in res and "loo" not in plain
    for k in ("theta", "beta", "f", "IRFs"):
        assert np.array_equal(res[k], plain[k], equal_nan=True), k
    same_tree(res["ppc"], plain["ppc"], ("ppc",))
    same_tree(res["summary"], plain["summary"], ("summary",))


def test_two_runs_give_a_byte_identical_state_block(handle, real_chain):
    from gpirt_amd import Sampler, _lib
    y, S, Bn = real_chain["y"], real_chain["S"], real_chain["Bn"]
    s = Sampler(handle, y, real_chain["inits"][1], preset="fast", seed=_lib.chain_seed(real_chain["seed"], 1))
    s.init()
    s.loo_enable(2 * S)
    for it in range(S + Bn):
        s.step()
        if it >= Bn:
            s.loo_accumulate()
    s.check()
    block = s.loo_state().cpu().numpy().tobytes()
    s.close()
    assert block == real_chain["blocks"][1]


def test_reference_rng_with_one_chain_is_untouched(handle):
    from gpirt_amd import gpirtMCMC
    from gpirt_amd.ops import RStream
    y = senate_slice()[:40, :6]
    th0 = np.random.default_rng(8).normal(size=40)
    streams = [RStream(77), RStream(77)]
    out = [gpirtMCMC(y, 6, 2, vote_codes=CODES, theta_init=th0, rng="reference", rstream=streams[k], loo=on)
           for k, on in enumerate((None, True))]
    for k in ("theta", "beta", "f", "IRFs"):
        assert np.array_equal(out[0][k], out[1][k], equal_nan=True), k
    (mt0, i0), (mt1, i1) = streams[0].state(), streams[1].state()
    assert i0 == i1 and np.array_equal(mt0, mt1)
    lo = out[1]["loo"]
    assert lo["T"] == 6 and lo["M"] == 1 and lo["draws"] == 6 and lo["cells_incomplete"] == 0
    assert lo["unsmoothed"] == lo["n_obs"] == int((~np.isnan(y)).sum())             # M = 1 < 5: the raw ratios


# ------------------------------------------------------------------------------------------- 4. beside the WAIC ---
def test_lppd_equals_the_summaries_pooled_lppd(real_chain):
    """log(p_sum / T) against the summaries' log-mean-exp of the same draws: both are a sum of T positive terms under a log, each
    within (T + 8) eps / 2 relative before the log, so the logs differ by at most (T + 8) eps absolutely (and relatively where
    |lppd| > 1)"""
    res = real_chain["res"]
    a, b = res["loo"]["pointwise"]["lppd"], np.asarray(res["summary"]["lppd"])
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    err = np.abs(a[ok] - b[ok]) / np.maximum(1.0, np.abs(b[ok]))
    print(f"MEASURED lppd against the summaries: {err.max() / ((120 + 8) * EPS):.3f} of (T + 8) eps")
    assert (err <= (120 + 8) * EPS).all()


def test_argument_errors(handle):
    from gpirt_amd import Sampler, gpirtMCMC
    y = senate_slice()[:40, :6]
    for bad in (dict(tail=4), dict(tail=1025), dict(top=0), dict(top=65), dict(tails=9), 7):
        with pytest.raises(ValueError):
            gpirtMCMC(y, 30, 1, vote_codes=CODES, preset="fast", loo=bad)
    with pytest.raises(ValueError, match="more than the 6 planned draws"):
        gpirtMCMC(y, 6, 1, vote_codes=CODES, preset="fast", loo=dict(tail=6))
    s = Sampler(handle, y, np.zeros(40), preset="fast", seed=1)
    s.init()
    with pytest.raises(Exception, match="not enabled"):
        s.loo_accumulate()
    with pytest.raises(ValueError, match="GPIRT_LOO_MAX_TAIL"):
        s.loo_enable(200000)
    s.loo_enable(200000, tail=1024)
    assert s.loo_get("counts").tolist() == [40, 6, 200000, 1024, 0, 1] and s.loo_get("keys").shape == (1025, 40, 6)
    s.loo_enable(on=False)
    s.close()
