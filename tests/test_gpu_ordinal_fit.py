"""The ordinal fit block on the device (include/gpirt_hip.h "ordinal model fit", csrc/ordinal_fit.hip) against the NumPy statement
gpirt_amd.ordinal.fit_from_draws under the bounds of tests/_ordinal_fit_bounds.py: the stage API over a few draws, the exported
uniforms, constructed states, the untouched chain and repeatability, the pooling of chains, the refusals and ordinal.run(fit=True).

The shapes are the smallest at which the layout can go wrong: 257 crosses the 256-row block, 33 the 32-item strip, C = 8 is the
category limit, C = 2 the binary anchor; each has about 3 % missing cells, an all-missing column and row and an item with a single
category (tests/_ordinal_fit_bounds.py make_case)."""
import numpy as np
import pytest

import _ordinal_fit_bounds as FB

pytestmark = pytest.mark.gpu
LD = np.longdouble
EPS = FB.EPS
INT_UNIT = ("n_obs", "obs_score", "score_ge", "score_gt", "rep_score_sum", "rep_score_sumsq", "agree_sum", "dev_ge", "nonfinite")
INT_CAT = ("obs_count", "rep_count_sum", "rep_count_sumsq", "count_ge", "count_gt")
UNITS = ("item", "respondent", "totals")


def _sampler(handle, cat, C, seed, K0=None, parts=("waic", "pred", "ppc"), planned=0):
    from gpirt_amd import Sampler
    from gpirt_amd import ordinal as OR
    s = Sampler(handle, OR.dichotomise(cat), FB.theta_start(cat.shape[0], 7), seed=seed, preset="fast")
    s.init()
    s.ordinal_enable(cat, C, K0=OR.init_thresholds(cat, OR.grid(), C) if K0 is None else K0, planned_draws=planned)
    if parts:
        s.ordinal_fit_enable(parts)
    return s


def _run(s, steps, record=False):
    g, B, iters = [], [], []
    for _ in range(steps):
        s.step()
        s.draw_thresholds()
        if record:
            s.ordinal_record()
        if getattr(s, "_ofit", 0):
            s.ordinal_fit_accumulate()
        iters.append(s.iteration)
        g.append(s.get("f") + s.get("mu"))
        B.append(s.ordinal_get("thresholds"))
    s.check()
    return np.stack(g), np.stack(B), iters


def _units(got):
    """item, respondent, totals as dicts of 1-d arrays"""
    tot = {k: np.atleast_1d(np.asarray(got["totals"][k])) for k in got["item"] if k in got["totals"]}
    return dict(item=got["item"], respondent=got["respondent"], totals=tot)


def _ratio(got, want, bound, what):
    """|got - want| <= bound wherever want is finite, the same non-finite values elsewhere; returns the worst |err| / bound"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), want.shape)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), what
    if not fin.any():
        return 0.0
    err = np.abs(got[fin] - want[fin])
    worst = float((err / np.maximum(bound[fin], 1e-300)).max())
    assert (err <= bound[fin]).all(), f"{what}: worst ratio to the bound {worst:.3e}"
    return worst


def _check_ints(got, want, C):
    u = _units(got)
    for unit in UNITS:
        for k in INT_UNIT:
            lo, hi = want[unit][k]
            v = u[unit][k].astype(np.int64)
            assert ((v >= lo) & (v <= hi)).all(), (unit, k, v, lo, hi)
    for k in INT_CAT:
        lo, hi = want["categories"][k]
        v = got["categories"][k].astype(np.int64)
        assert v.shape == lo.shape and ((v >= lo) & (v <= hi)).all(), (k, v, lo, hi)


def _check_derived(got, S):
    """means, variances and p-values are exact functions of the device's own integer sums"""
    from gpirt_amd.ordinal import _exact_var
    u = _units(got)
    for unit in UNITS:
        d = u[unit]
        Sk = S - d["nonfinite"].astype(np.int64)
        with np.errstate(invalid="ignore", divide="ignore"):
            den = np.where((d["n_obs"] > 0) & (Sk >= 1), Sk, np.nan).astype(np.float64)
            f = lambda k: d[k].astype(np.float64)       # noqa: E731
            for k, v in (("ppp_score", f("score_ge") / den), ("ppp_score_mid", (f("score_ge") + f("score_gt")) / (2.0 * den)),
                         ("rep_score_mean", f("rep_score_sum") / den), ("ppp_dev", f("dev_ge") / den),
                         ("agree_mean", f("agree_sum") / den), ("dev_obs_mean", d["dev_obs_sum"] / den),
                         ("dev_rep_mean", d["dev_rep_sum"] / den)):
                assert np.array_equal(np.atleast_1d(d[k]), v, equal_nan=True), (unit, k)
            var = np.where(d["n_obs"] > 0, _exact_var(Sk, d["rep_score_sum"], d["rep_score_sumsq"]), np.nan)
            assert np.array_equal(np.atleast_1d(d["rep_score_var"]), var, equal_nan=True), unit
    it, k = got["item"], got["categories"]
    Sk = S - it["nonfinite"].astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.where((it["n_obs"] > 0) & (Sk >= 1), Sk, np.nan).astype(np.float64)[:, None]
        assert np.array_equal(k["ppp_count"], k["count_ge"].astype(np.float64) / den, equal_nan=True)
        assert np.array_equal(k["ppp_count_mid"], (k["count_ge"].astype(np.float64) + k["count_gt"].astype(np.float64)) / (2.0 * den),
                              equal_nan=True)
        assert np.array_equal(k["rep_count_mean"], k["rep_count_sum"].astype(np.float64) / den, equal_nan=True)


def _check_doubles(got, want, cat, S, tag, h=0.05, dev_rep=True, waic_m2=True):
    n, m = cat.shape
    u = _units(got)
    worst = {}
    for unit, L in (("item", n), ("respondent", m), ("totals", n * m)):
        for k in ("dev_obs_sum", "dev_rep_sum")[:2 if dev_rep else 1]:
            w = np.asarray(want[unit][k], dtype=np.float64)
            worst[f"{unit}_{k}"] = _ratio(u[unit][k], w, FB.dev_rtol(L, S, h) * np.abs(w), f"{unit} {k}")
    w = want["waic"]
    obs = w["observed"]
    M = FB.magnitude(w["ll_absmax"].astype(np.float64), S)
    gw = got["waic"]
    assert (gw["ll_m2"][~obs] == -1.0).all() and (gw["lse"][~obs] == 0.0).all() and np.isnan(gw["lppd"][~obs]).all()
    worst["lse"] = _ratio(gw["lse"][obs], w["lse"][obs].astype(np.float64), FB.lse_atol(M, S, h)[obs], "lse")
    worst["ll_mean"] = _ratio(gw["ll_mean"][obs], w["ll_mean"][obs].astype(np.float64), FB.mean_atol(M, S, h)[obs], "ll_mean")
    if waic_m2:
        worst["ll_m2"] = _ratio(gw["ll_m2"][obs], w["ll_m2"][obs].astype(np.float64), FB.m2_atol(M, S, h)[obs], "ll_m2")
    ps = want["pred_sum"]
    worst["pred_sum"] = _ratio(np.moveaxis(got["pred"]["exceed"], 2, 0) * S, ps, (FB.pred_rtol(S) + 2 * EPS) * np.abs(ps), "pred_sum")
    if S >= 2 and np.isfinite(float(w["totals"]["lppd"])) and waic_m2:
        t, wt = got["totals"], w["totals"]
        lppd, pw = w["lppd"][obs].astype(np.float64), w["p_waic"][obs].astype(np.float64)
        worst["lppd"] = _ratio(t["lppd"], float(wt["lppd"]), FB.total_atol(FB.lse_atol(M, S, h)[obs], lppd), "lppd")
        worst["p_waic"] = _ratio(t["p_waic"], float(wt["p_waic"]), FB.total_atol(FB.m2_atol(M, S, h)[obs] / (S - 1), pw), "p_waic")
        assert t["elpd_waic"] == t["lppd"] - t["p_waic"] and t["waic"] == -2.0 * t["elpd_waic"]
        assert t["n_obs"] == int(obs.sum()) == wt["n_obs"] and t["draws"] == S
        # se = sqrt(N var(elpd_ij)): the cells' elpd within their bounds move the standard deviation by at most the largest of them
        cell = (FB.lse_atol(M, S, h) + FB.m2_atol(M, S, h) / (S - 1))[obs]
        se_tol = float(np.sqrt(obs.sum()) * 2.0 * cell.max() + 1e3 * EPS * float(wt["se_elpd_waic"]))
        worst["se"] = _ratio(t["se_elpd_waic"], float(wt["se_elpd_waic"]), se_tol, "se_elpd_waic")
    for k, v in worst.items():
        print(f"MEASURED {k}_ratio@{tag} {v:.3e} (of the derived bound)")


# ------------------------------------------------------------------------------------------- 1. against the NumPy statement ---
@pytest.mark.parametrize("n,m,C,steps", FB.SHAPES)
def test_stage_api_against_fit_from_draws(handle, n, m, C, steps):
    from gpirt_amd import ordinal as OR
    cat = FB.make_case(n, m, C, 100 + n)["cat"]
    s = _sampler(handle, cat, C, FB.SEED)
    g, B, iters = _run(s, steps)
    got = s.ordinal_fit()
    s.close()
    assert iters == list(range(1, steps + 1))
    want = OR.fit_from_draws(cat, g, B, FB.SEED, iters)
    und = want["undecided"]["cells"] + want["undecided"]["comparisons"]
    print(f"MEASURED undecided@{n}x{m}x{C} cells {want['undecided']['cells']} comparisons {want['undecided']['comparisons']} "
          f"of {want['comparisons']}")
    assert und <= 1e-3 * want["comparisons"]
    _check_ints(got, want, C)
    _check_derived(got, steps)
    _check_doubles(got, want, cat, steps, f"{n}x{m}x{C}", dev_rep=want["undecided"]["cells"] == 0)
    # the units without an observed cell come out as NaN
    assert np.isnan(got["item"]["ppp_score"][m // 3]) and np.isnan(got["respondent"]["ppp_dev"][n // 2])
    assert np.isnan(got["categories"]["ppp_count_mid"][m // 3]).all()
    assert np.isnan(got["item"]["ppp_score"]).sum() == 1 and np.isnan(got["respondent"]["rep_score_mean"]).sum() == 1
    # the predictions: probabilities by difference of the means, p_observed NaN exactly for the missing cells
    p = got["pred"]
    assert np.allclose(p["probs"].sum(axis=2), 1.0, rtol=0, atol=8 * EPS) and (np.diff(p["exceed"], axis=2) <= 0).all()
    assert np.array_equal(np.isnan(p["p_observed"]), cat == 0)


# -------------------------------------------------------------------------------- 2. the uniforms reproduce the replicate ---
def test_uniforms_reproduce_the_replicate(handle):
    n, m, C = 100, 17, 3
    cat = FB.make_case(n, m, C, 200)["cat"].astype(np.int64)
    seed = 2**40 + 3
    s = _sampler(handle, cat.astype(np.int8), C, seed)
    s.step()
    s.draw_thresholds()
    s.ordinal_fit_accumulate()
    it = s.iteration
    e = s.ordinal_fit_get("pred_sum")                                  # one draw: the sums are the e_c themselves
    rep = s.ordinal_fit_get("rep").astype(np.int64)
    score, counts, delta = s.ordinal_fit_get("score"), s.ordinal_fit_get("counts_rep"), s.ordinal_fit_get("delta")
    agree = [s.ordinal_fit_get(f"{u}_agree_sum").astype(np.int64) for u in ("item", "respondent", "total")]
    u = handle.item_uniforms(seed, it, 17, 0, m, n).cpu().numpy()
    s.close()
    obs = cat > 0
    assert np.array_equal(rep, np.where(obs, 1 + (u[None] < e).sum(axis=0), 0))
    assert np.array_equal(score, np.concatenate([rep.sum(axis=0), rep.sum(axis=1), [rep.sum()]]))
    assert np.array_equal(counts, np.stack([(rep == c).sum(axis=0) for c in range(1, C + 1)], axis=1))
    same = obs & (rep == cat)
    assert np.array_equal(agree[0], same.sum(axis=0)) and np.array_equal(agree[1], same.sum(axis=1)) and agree[2][0] == same.sum()
    # Delta is exactly 0 where nothing changed (the unit is counted in dev_ge) and finite everywhere
    changed = obs & (rep != cat)
    assert np.isfinite(delta).all() and (delta[:m][changed.sum(axis=0) == 0] == 0.0).all()
    assert (delta[m:m + n][changed.sum(axis=1) == 0] == 0.0).all()


# ------------------------------------------------------------------------------------------------ 3. constructed states ---
def _constructed(handle, cat, C, K0, f_of_mu, seed=91):
    """one accumulate on a written f (f_of_mu: mu -> f) with the thresholds at K0; returns the device's result, the NumPy
    statement's from the device's own g and thresholds, g, and the raw state block's bytes"""
    from gpirt_amd import ordinal as OR
    s = _sampler(handle, cat, C, seed, K0=np.ascontiguousarray(K0, dtype=np.int32))
    s.set("f", np.asfortranarray(f_of_mu(s.get("mu"))))
    s.ordinal_fit_accumulate()
    g, B, it = s.get("f") + s.get("mu"), s.ordinal_get("thresholds"), s.iteration
    got = s.ordinal_fit()
    got["rep"] = s.ordinal_fit_get("rep")
    got["delta"] = s.ordinal_fit_get("delta")
    raw = s.ordinal_fit_state().cpu().numpy().tobytes()
    s.close()
    want = OR.fit_from_draws(cat, g[None], B[None], seed, [it])
    return got, want, g, raw


def test_constructed_states(handle):
    n, m, C = 100, 17, 3
    cat = FB.make_case(n, m, C, 300)["cat"]
    obs = cat > 0
    K = np.tile(np.array([100, 140]), (m, 1))
    rng = np.random.default_rng(5)
    noise = rng.standard_normal((n, m))
    # g = +-1e3 in the observed cells: the replicate is exactly C or 1, everything finite or not as the NumPy statement has it
    for sign, cat_rep in ((1.0, C), (-1.0, 1)):
        got, want, g, _ = _constructed(handle, cat, C, K, lambda mu: np.where(obs, sign * 1e3 - mu, noise))
        assert (np.abs(g[obs]) > 990).all()
        assert np.array_equal(got["rep"], np.where(obs, cat_rep, 0))
        assert want["undecided"] == dict(cells=0, comparisons=0)
        _check_ints(got, want, C)
        _check_doubles(got, want, cat, 1, f"g={sign * 1e3:+.0f}", waic_m2=False)
        assert np.isfinite(got["delta"]).all()
        assert np.array_equal(got["item"]["agree_sum"], (cat == cat_rep).sum(axis=0))
    # g = NaN in one observed cell: that item, that respondent and the totals count the draw out, nobody else is touched
    i0, j0 = 3, 2
    assert obs[i0, j0]
    base, wbase, _, _ = _constructed(handle, cat, C, K, lambda mu: noise)
    got, want, _, _ = _constructed(handle, cat, C, K, lambda mu: np.where((np.arange(n)[:, None] == i0) & (np.arange(m)[None, :] == j0),
                                                                          np.nan, noise))
    _check_ints(got, want, C)
    assert got["item"]["nonfinite"][j0] == 1 and got["respondent"]["nonfinite"][i0] == 1 and got["totals"]["nonfinite"] == 1
    assert got["item"]["nonfinite"].sum() == 1 and got["respondent"]["nonfinite"].sum() == 1
    for unit, skip in (("item", j0), ("respondent", i0)):
        keep = np.arange(len(got[unit]["n_obs"])) != skip
        for k in INT_UNIT + ("dev_obs_sum", "dev_rep_sum"):
            assert np.array_equal(got[unit][k][keep], base[unit][k][keep]), (unit, k)
        for k in ("rep_score_sum", "score_ge", "agree_sum", "dev_ge"):
            assert got[unit][k][skip] == 0
        assert got[unit]["dev_obs_sum"][skip] == 0.0
    assert (got["categories"]["rep_count_sum"][j0] == 0).all()
    keep = np.arange(m) != j0
    assert np.array_equal(got["categories"]["rep_count_sum"][keep], base["categories"]["rep_count_sum"][keep])
    assert np.isnan(got["waic"]["lse"][i0, j0]) and np.isnan(got["waic"]["ll_mean"][i0, j0]) and np.isnan(got["waic"]["ll_m2"][i0, j0])
    cell = np.zeros((n, m), dtype=bool)
    cell[i0, j0] = True
    assert np.array_equal(got["waic"]["lse"][~cell], base["waic"]["lse"][~cell])
    assert np.isnan(got["pred"]["exceed"][i0, j0]).all() and got["rep"][i0, j0] == 0
    # g = NaN in a missing cell: nothing changes but that cell's prediction
    i1, j1 = np.argwhere(~obs & (np.arange(m)[None, :] != m // 3) & (np.arange(n)[:, None] != n // 2))[0]
    got, _, _, _ = _constructed(handle, cat, C, K, lambda mu: np.where((np.arange(n)[:, None] == i1) & (np.arange(m)[None, :] == j1),
                                                                       np.nan, noise))
    for unit in ("item", "respondent"):
        for k in INT_UNIT + ("dev_obs_sum", "dev_rep_sum"):
            assert np.array_equal(got[unit][k], base[unit][k]), (unit, k)
    assert got["totals"]["nonfinite"] == 0 and got["totals"]["dev_obs_sum"] == base["totals"]["dev_obs_sum"]
    for k in ("lse", "ll_mean", "ll_m2"):
        assert np.array_equal(got["waic"][k], base["waic"][k])
    assert np.array_equal(got["rep"], base["rep"]) and np.array_equal(got["categories"]["rep_count_sum"], base["categories"]["rep_count_sum"])
    cell = np.zeros((n, m), dtype=bool)
    cell[i1, j1] = True
    assert np.isnan(got["pred"]["exceed"][i1, j1]).all() and np.array_equal(got["pred"]["exceed"][~cell], base["pred"]["exceed"][~cell])


def test_constructed_thresholds(handle):
    from gpirt_amd import ordinal as OR
    n, m = 100, 17
    rng = np.random.default_rng(6)
    noise = 1.5 * rng.standard_normal((n, m))
    t = OR.grid()
    # thresholds one grid step apart: the w term is at its largest (log1p(-exp(-0.05)) = -3.02 per interior cell)
    C = 5
    cat = FB.make_case(n, m, C, 301)["cat"]
    K = np.tile(np.array([118, 119, 120, 121]), (m, 1))
    got, want, g, _ = _constructed(handle, cat, C, K, lambda mu: noise)
    assert want["undecided"]["cells"] == 0
    _check_ints(got, want, C)
    _check_doubles(got, want, cat, 1, "one-step", h=float(t[1] - t[0]), waic_m2=False)
    inner = (cat > 1) & (cat < C)
    assert (got["waic"]["lse"][inner] < np.log1p(-np.exp(-0.0501))).all()
    # all thresholds at the grid's two ends
    C = 3
    cat = FB.make_case(n, m, C, 302)["cat"]
    K = np.tile(np.array([0, t.size - 1]), (m, 1))
    got, want, g, _ = _constructed(handle, cat, C, K, lambda mu: noise)
    assert want["undecided"]["cells"] == 0
    _check_ints(got, want, C)
    _check_doubles(got, want, cat, 1, "grid-ends", waic_m2=False)
    # C = 2 at the centre: the binary formula
    from gpirt_amd.ppc import item_uniform
    C = 2
    cat = FB.make_case(n, m, C, 303)["cat"].astype(np.int64)
    seed = 91
    got, want, g, _ = _constructed(handle, cat.astype(np.int8), C, np.full((m, 1), 120), lambda mu: noise, seed=seed)
    _check_ints(got, want, C)
    obs = cat > 0
    y = np.where(cat == 2, 1.0, -1.0)
    u = item_uniform(seed, 0, 17, np.arange(m, dtype=np.uint64)[None, :], np.arange(n, dtype=np.uint64)[:, None])
    e = np.exp(-np.abs(g))
    yes = obs & (u < np.where(g >= 0, 1.0 / (1.0 + e), e / (1.0 + e)))
    flipped = obs & (yes != (cat == 2))
    delta = np.where(flipped, y * g, 0.0)
    for unit, axis in (("item", 0), ("respondent", 1)):
        d = got[unit]
        R = (obs.sum(axis=axis) + yes.sum(axis=axis)).astype(np.uint64)
        T = cat.sum(axis=axis).astype(np.uint64)
        some = obs.sum(axis=axis) > 0
        assert np.array_equal(d["rep_score_sum"], R) and np.array_equal(d["rep_score_sumsq"], R * R) and np.array_equal(d["obs_score"], T)
        assert np.array_equal(d["score_ge"], (some & (R >= T)).astype(np.uint64)) and np.array_equal(d["score_gt"], (some & (R > T)).astype(np.uint64))
        assert np.array_equal(d["agree_sum"], (obs & ~flipped).sum(axis=axis).astype(np.uint64))
        D = delta.sum(axis=axis)
        clear = some & ((D == 0) | (np.abs(D) > 1e-10 * np.abs(delta).sum(axis=axis)))
        assert np.array_equal(d["dev_ge"][clear], (D >= 0)[clear].astype(np.uint64)) and clear.sum() >= some.sum() - 1


# ------------------------------------------------------------------- 4. the chain is untouched and runs repeat ---
def test_chain_untouched_and_runs_repeat(handle):
    n, m, C, steps = 257, 33, 4, 10
    cat = FB.make_case(n, m, C, 400)["cat"]
    outs = []
    for parts in (("waic", "pred", "ppc"), None, ("waic", "pred", "ppc")):
        s = _sampler(handle, cat, C, 4242, parts=parts, planned=steps)
        _run(s, steps, record=True)
        outs.append(dict(theta=s.get("theta").tobytes(), beta=s.get("beta").tobytes(), f=s.get("f").tobytes(),
                         index=s.ordinal_get("index").tobytes(), hist=s.ordinal_get("hist").tobytes(),
                         state=s.ordinal_fit_state().cpu().numpy().tobytes() if parts else None))
        s.close()
    for k in ("theta", "beta", "f", "index", "hist"):
        assert outs[0][k] == outs[1][k] == outs[2][k], k
    assert outs[0]["state"] == outs[2]["state"] and len(outs[0]["state"]) > 8 * n * m * 6


# --------------------------------------------------------------------------------------------------------- 5. pooling ---
def test_pooling_two_chains(handle):
    from gpirt_amd import ordinal as OR
    n, m, C, S = 100, 17, 3, 4
    cat = FB.make_case(n, m, C, 500)["cat"]
    seeds = (11, 12)
    chains, draws, wants = [], [], []
    for sd in seeds:
        s = _sampler(handle, cat, C, sd)
        g, B, iters = _run(s, S)
        chains.append(s)
        draws.append((g, B))
        wants.append(OR.fit_from_draws(cat, g, B, sd, iters))
    own = [c.ordinal_fit() for c in chains]
    pooled = OR.fit_combine(handle, chains, cat)
    # counts: the sum of the chains' own, inside the summed [lo, hi]
    for unit in ("item", "respondent"):
        for k in INT_UNIT:
            if k in ("n_obs", "obs_score"):
                assert np.array_equal(pooled[unit][k], own[0][unit][k])
                continue
            assert np.array_equal(pooled[unit][k], own[0][unit][k] + own[1][unit][k]), (unit, k)
            lo, hi = wants[0][unit][k][0] + wants[1][unit][k][0], wants[0][unit][k][1] + wants[1][unit][k][1]
            v = pooled[unit][k].astype(np.int64)
            assert ((v >= lo) & (v <= hi)).all(), (unit, k)
        for k in ("dev_obs_sum", "dev_rep_sum"):
            assert np.array_equal(pooled[unit][k], own[0][unit][k] + own[1][unit][k])
    for k in INT_CAT[1:]:
        assert np.array_equal(pooled["categories"][k], own[0]["categories"][k] + own[1]["categories"][k])
    assert np.array_equal(pooled["pred"]["exceed"] * (2 * S), own[0]["pred"]["exceed"] * S + own[1]["pred"]["exceed"] * S)
    _check_derived(pooled, 2 * S)
    # WAIC against the NumPy statement over both chains' stored draws
    both = OR.fit_from_draws(cat, np.concatenate([draws[0][0], draws[1][0]]), np.concatenate([draws[0][1], draws[1][1]]), 1,
                             list(range(1, 2 * S + 1)))["waic"]
    obs = both["observed"]
    M = FB.magnitude(both["ll_absmax"].astype(np.float64), 2 * S)
    lse_b, m2_b = FB.lse_atol(M, 2 * S)[obs], FB.pooled_m2_atol(M, S)[obs]
    r1 = _ratio(pooled["waic"]["lse"][obs], both["lse"][obs].astype(np.float64), lse_b, "pooled lse")
    r2 = _ratio(pooled["waic"]["ll_m2"][obs], both["ll_m2"][obs].astype(np.float64), m2_b, "pooled ll_m2")
    t, wt = pooled["totals"], both["totals"]
    r3 = _ratio(t["lppd"], float(wt["lppd"]), FB.total_atol(lse_b, both["lppd"][obs].astype(np.float64)), "pooled lppd")
    r4 = _ratio(t["p_waic"], float(wt["p_waic"]), FB.total_atol(m2_b / (2 * S - 1), both["p_waic"][obs].astype(np.float64)), "pooled p_waic")
    print(f"MEASURED pooled ratios lse {r1:.3e} ll_m2 {r2:.3e} lppd {r3:.3e} p_waic {r4:.3e} (of the derived bounds)")
    assert t["draws"] == 2 * S and t["n_obs"] == int(obs.sum())
    # the pooled block is read by _get and _totals as one chain's is
    st = pooled["state"]
    assert OR.fit_block_header(st)["draws"] == 2 * S
    assert np.array_equal(OR.fit_block_get(handle, st, "item_score_ge"), pooled["item"]["score_ge"])
    assert OR.fit_block_totals(handle, st)["lppd"] == t["lppd"]
    one = chains[0].ordinal_fit_state()
    assert np.array_equal(OR.fit_block_get(handle, one, "lse"), own[0]["waic"]["lse"])
    assert OR.fit_block_totals(handle, one)["elpd_waic"] == own[0]["totals"]["elpd_waic"]
    for c in chains:
        c.close()


# ------------------------------------------------------------------------------------------------------ 6. refusals ---
def test_refusals_name_their_reason(handle):
    from gpirt_amd import Sampler, _lib
    from gpirt_amd import ordinal as OR
    n, m, C = 100, 17, 3
    cat = FB.make_case(n, m, C, 600)["cat"]
    s = Sampler(handle, OR.dichotomise(cat), FB.theta_start(n, 7), seed=3, preset="fast")
    with pytest.raises(_lib.GpirtError, match="needs an initialised sampler"):
        s.ordinal_fit_enable()
    s.init()
    with pytest.raises(_lib.GpirtError, match=r"ordinal responses are not enabled \(gpirt_sampler_ordinal_enable\)"):
        s.ordinal_fit_enable()
    s.ordinal_enable(cat, C)
    with pytest.raises(_lib.GpirtError, match="parts = 8 has bits outside GPIRT_OFIT_WAIC"):
        s.ordinal_fit_enable(8)
    with pytest.raises(_lib.GpirtError, match=r"the ordinal fit block is not enabled \(gpirt_sampler_ordinal_fit_enable\)"):
        s.ordinal_fit_accumulate()
    with pytest.raises(ValueError, match="unknown part"):
        s.ordinal_fit_enable(("waic", "loo"))
    s.ordinal_fit_enable(("waic",))
    s.ordinal_fit_accumulate()
    assert s.ordinal_fit_get("lse").shape == (n, m) and s.ordinal_fit_totals()["draws"] == 1
    with pytest.raises(_lib.GpirtError, match="'pred_sum' belongs to the pred part, which is not enabled"):
        s.ordinal_fit_get("pred_sum")
    with pytest.raises(_lib.GpirtError, match="'item_score_ge' belongs to the ppc part, which is not enabled"):
        s.ordinal_fit_get("item_score_ge")
    with pytest.raises(_lib.GpirtError, match="'rep' belongs to the ppc part, which is not enabled"):
        s.ordinal_fit_get("rep")
    with pytest.raises(_lib.GpirtError, match="unknown ordinal fit array"):
        s.ordinal_fit_get("item_nothing")
    # the binary blocks are still refused while ordinal is on
    with pytest.raises(_lib.GpirtError, match="refused while ordinal responses are on"):
        s.summary_enable(("waic",))
    with pytest.raises(_lib.GpirtError, match="refused while ordinal responses are on"):
        s.ppc_enable()
    # parts = None turns it off; turning ordinal off frees it with the rest
    s.ordinal_fit_enable(None)
    with pytest.raises(_lib.GpirtError, match="the ordinal fit block is not enabled"):
        s.ordinal_fit_accumulate()
    s.ordinal_fit_enable(("pred", "ppc"))
    s.ordinal_enable(None)
    with pytest.raises(_lib.GpirtError, match="the ordinal fit block is not enabled"):
        s.ordinal_fit_totals()
    s.close()


# ---------------------------------------------------------------------------------------------- 7. ordinal.run(fit=) ---
def test_run_with_fit(handle):
    from gpirt_amd import ordinal as OR
    n, m, C = 512, 24, 4
    cat = OR.make_graded(n, m, C, seed=8, na_frac=0.05)["cat"]
    plain = OR.run(cat, 6, 3, C=C, seed=5, handle=handle)
    assert set(plain) == {"theta", "beta", "threshold_draws", "thresholds", "hist", "curves", "counters", "grid", "categories", "chains",
                          "consistent"}
    res = OR.run(cat, 40, 20, C=C, seed=5, handle=handle, fit=True)
    assert set(res) == set(plain) | {"fit"}
    fit = res["fit"]
    assert set(fit) == {"waic", "pred", "item", "respondent", "totals", "categories"}
    assert fit["totals"]["draws"] == 40 and np.isfinite(fit["totals"]["elpd_waic"]) and fit["totals"]["se_elpd_waic"] > 0
    assert fit["totals"]["n_obs"] == int((cat > 0).sum())
    mid = fit["categories"]["ppp_count_mid"]
    assert mid.shape == (m, C) and ((mid >= 0) & (mid <= 1)).all()
    assert fit["pred"]["probs"].shape == (n, m, C) and fit["waic"]["elpd"].shape == (n, m)
    only = OR.run(cat, 4, 2, C=C, seed=5, handle=handle, fit=("waic",))["fit"]
    assert only["pred"] is None and only["item"] is None and np.isfinite(only["totals"]["lppd"])
