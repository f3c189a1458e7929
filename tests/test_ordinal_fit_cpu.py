"""The NumPy statement of the ordinal fit block (gpirt_amd.ordinal.fit_from_draws; csrc/ordinal_fit.hip) without a device and
without a built library: the binary anchor against ppc.from_draws, WAIC against a brute-force long-double evaluation, the
replicate's category frequencies, and no undecided cell or comparison at the GPU test's shapes and seeds."""
import numpy as np
import pytest

import _ordinal_fit_bounds as FB

LD = np.longdouble


def test_two_categories_at_the_centre_are_the_binary_ppc():
    """C = 2, the threshold at 0 and stage = 8 (the binary PPC's): e_1 = plogis(g) and the same uniform, so the replicate is the
    binary one -- score - n_obs is the yes count, and score_ge, score_gt, dev_ge and nonfinite are ppc.from_draws' exactly.
    agree_sum counts the cells with rep == cat; the binary block has no such field (its correct_sum compares the sign of g with y),
    so it is held to a NumPy recomputation from the binary replicate."""
    from gpirt_amd import ordinal as OR
    from gpirt_amd import ppc as P
    n, m, S, seed = 300, 20, 4, 77
    d = OR.make_graded(n, m, 2, seed=3, na_frac=0.05, thresholds=np.full((m, 1), 0.6))
    cat = np.array(d["cat"])
    cat[:, 4] = 0
    cat[9, :] = 0
    y = np.where(cat == 0, np.nan, np.where(cat == 2, 1.0, -1.0))
    assert np.array_equal(OR.dichotomise(cat), y, equal_nan=True)          # (the lower median of every item is category 1)
    rng = np.random.default_rng(1)
    g = d["theta"][None, :, None] * d["slopes"][None, None, :] + 0.4 * rng.standard_normal((S, n, m))
    g[1, 3, 2] = np.nan                                                      # an observed cell
    assert cat[3, 2] > 0
    iters = [3, 4, 7, 9]
    got = OR.fit_from_draws(cat, g, np.zeros((S, m, 1)), seed, iters, item0=5, stage=8)
    want = P.from_draws(y, g, seed, iters, item0=5)
    assert got["undecided"] == dict(cells=0, comparisons=0) and want["undecided"] == dict(cells=0, comparisons=0)
    assert got["comparisons"] == want["comparisons"]
    u = np.stack([P.replicate_uniforms(seed, it, n, m, 5) for it in iters])
    with np.errstate(invalid="ignore"):
        yrep = np.where(u < 1.0 / (1.0 + np.exp(-g)), 1.0, -1.0)
    for unit, axis in (("item", 0), ("respondent", 1), ("totals", None)):
        a, b = got[unit], want[unit]
        for lohi in (0, 1):
            nobs = b["n_obs"][lohi]
            assert np.array_equal(a["n_obs"][lohi], nobs)
            assert np.array_equal(a["obs_score"][lohi] - nobs, b["obs_yes"][lohi])
            live_draws = S - b["nonfinite"][lohi]
            assert np.array_equal(a["nonfinite"][lohi], b["nonfinite"][lohi])
            assert np.array_equal(a["rep_score_sum"][lohi] - live_draws * nobs, b["rep_yes_sum"][lohi])
            for k, kb in (("score_ge", "yes_ge"), ("score_gt", "yes_gt"), ("dev_ge", "dev_ge")):
                assert np.array_equal(a[k][lohi], b[kb][lohi]), (unit, k)
        # agree_sum from the binary replicate, draw by draw, with the unit's non-finite draws left out
        agree = np.zeros_like(a["agree_sum"][0])
        for s in range(S):
            bad = (cat > 0) & ~np.isfinite(g[s])
            same = (cat > 0) & ~bad & (yrep[s] == y)
            if axis is None:
                agree += 0 if bad.any() else int(same.sum())
            else:
                agree += np.where(bad.any(axis=axis), 0, same.sum(axis=axis))
        assert np.array_equal(a["agree_sum"][0], agree) and np.array_equal(a["agree_sum"][1], agree)
    assert want["item"]["nonfinite"][0][2] == 1 and want["respondent"]["nonfinite"][0][3] == 1


def test_waic_against_brute_force_long_double():
    from gpirt_amd import ordinal as OR
    n, m, C, S = 60, 7, 4, 6
    case = FB.make_case(n, m, C, 11)
    g, B = FB.synthetic_draws(case, C, S, 11)
    cat = case["cat"].astype(np.int64)
    out = OR.fit_from_draws(cat, g, B, 5, list(range(1, S + 1)))
    w = out["waic"]
    lppd_tot = p_tot = LD(0)
    elpd = []
    for i in range(n):
        for j in range(m):
            if cat[i, j] == 0:
                continue
            lp = np.array([OR.category_logprobs(np.array([g[s, i, j]]), B[s, j])[cat[i, j] - 1, 0] for s in range(S)], dtype=LD)
            lppd = np.log(np.exp(lp).sum() / LD(S))
            pw = ((lp - lp.mean()) ** 2).sum() / LD(S - 1)
            assert abs(lppd - w["lppd"][i, j]) <= 64 * np.finfo(LD).eps * max(1, abs(lppd))
            assert abs(pw - w["p_waic"][i, j]) <= 64 * np.finfo(LD).eps * max(1, abs(pw))
            lppd_tot += lppd; p_tot += pw
            elpd.append(lppd - pw)
    t = w["totals"]
    elpd = np.array(elpd, dtype=LD)
    assert t["n_obs"] == int((cat > 0).sum()) == elpd.size and t["draws"] == S
    tol = 1e4 * float(np.finfo(LD).eps)
    assert abs(t["lppd"] - lppd_tot) <= tol * abs(lppd_tot) and abs(t["p_waic"] - p_tot) <= tol * abs(p_tot)
    assert abs(t["elpd_waic"] - (lppd_tot - p_tot)) <= tol * abs(lppd_tot) and t["waic"] == -2 * t["elpd_waic"]
    se = np.sqrt(elpd.size * elpd.var(ddof=1))
    assert abs(t["se_elpd_waic"] - se) <= tol * se
    # the category probabilities sum to one: logP is a log-probability, the w term included
    lp_all = OR.category_logprobs(g[0], B[0, 0])
    assert np.allclose(np.exp(lp_all).sum(axis=0).astype(np.float64), 1.0, rtol=0, atol=1e-15)
    # and the float64 streams' logP is the long-double one within a few ulp per term
    e, up, lo = OR._fit_terms(g[0], B[0])
    W = np.zeros((m, C + 1))
    W[:, 2:C] = np.log1p(-np.exp(-(B[0][:, 1:] - B[0][:, :-1])))
    lp64 = OR._fit_logp(np.where(cat > 0, cat, 1), up, lo, W)
    for j in range(m):
        ref = OR.loglik(cat[:, j], g[0][:, j].astype(LD), B[0, j], True, LD)
        sel = cat[:, j] > 0
        assert (np.abs(lp64[sel, j] - ref[sel].astype(np.float64)) <= FB.cell_ulps() * FB.EPS * np.abs(lp64[sel, j])).all()


def test_replicate_frequencies_match_the_category_probabilities():
    """A fixed g and fixed thresholds over many draws: the replicate's category frequencies are e_{c-1} - e_c within 5 standard
    errors of a binomial proportion (a 5.7e-7 event per comparison; 20 comparisons)."""
    from gpirt_amd import ordinal as OR
    n, m, C, S = 2, 2, 5, 4000
    g1 = np.array([[0.3, -1.1], [1.7, 0.2]])
    Bj = np.array([[-1.5, -0.4, 0.5, 1.6], [-2.0, -1.0, 0.0, 2.5]])
    cat = np.ones((n, m), dtype=np.int64)
    out = OR.fit_from_draws(cat, np.broadcast_to(g1, (S, n, m)), np.broadcast_to(Bj, (S, m, C - 1)), 99, list(range(1, S + 1)))
    rep = out["rep"]
    for i in range(n):
        for j in range(m):
            ex = np.concatenate([[1.0], 1.0 / (1.0 + np.exp(-(g1[i, j] - Bj[j]))), [0.0]])
            p = ex[:-1] - ex[1:]
            freq = np.array([(rep[:, i, j] == c).mean() for c in range(1, C + 1)])
            assert (np.abs(freq - p) <= 5.0 * np.sqrt(p * (1 - p) / S)).all(), (i, j, freq, p)
    # rep_count_sum of an item is the number of its cells replicated into each category, over all draws
    assert np.array_equal(out["categories"]["rep_count_sum"][0], np.stack([(rep == c).sum(axis=(0, 1)) for c in range(1, C + 1)], axis=1))
    # and the exceedance sums are S e_c, non-increasing in c
    ex = 1.0 / (1.0 + np.exp(-(g1[0, 0] - Bj[0])))
    assert np.allclose(out["pred_sum"][:, 0, 0], S * ex, rtol=FB.pred_rtol(S), atol=0)
    assert (np.diff(out["pred_sum"], axis=0) <= 0).all()


@pytest.mark.parametrize("n,m,C,steps", FB.SHAPES)
def test_no_undecided_cell_at_the_gpu_shapes(n, m, C, steps):
    """make_graded data, continuous g, thresholds on the 0.05 grid, the GPU test's shapes and seeds: no |u - e_c| within 1e-13 and
    no deviance comparison inside its band (the only zero differences are units whose replicate equals the data in every cell,
    which the Delta-over-changed-cells rule decides exactly)."""
    from gpirt_amd import ordinal as OR
    case = FB.make_case(n, m, C, 100 + n)
    g, B = FB.synthetic_draws(case, C, steps, 100 + n)
    out = OR.fit_from_draws(case["cat"], g, B, FB.SEED, list(range(1, steps + 1)))
    assert out["undecided"] == dict(cells=0, comparisons=0)
    assert out["comparisons"] == steps * ((m - 1) + (n - 1) + 1)             # one item and one respondent have no observed cell
    for unit in ("item", "respondent", "totals"):
        for k in OR.FIT_INT_UNIT:
            lo, hi = out[unit][k]
            assert np.array_equal(lo, hi), (unit, k)
    # the data has what the GPU test needs: an all-missing column and row, an item with a single category
    cat = case["cat"]
    assert (cat[:, m // 3] == 0).all() and (cat[n // 2, :] == 0).all() and set(np.unique(cat[:, m - 1])) <= {0, 1}
    assert 0.01 < (cat == 0).mean() < 0.12
