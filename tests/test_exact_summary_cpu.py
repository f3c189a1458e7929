"""The exact reference (tests/_exact_summary.py) against the NumPy references the GPU tests already use --
chains.diagnostics_from_draws, quantiles.from_draws / from_histograms, test_gpu_summary.ref_summary -- on random and
hand-worked inputs, so that a device test that disagrees with the exact reference points at the kernel."""
import math
from fractions import Fraction

import numpy as np
import pytest

import _exact_summary as X

PROBS = (0.0, 0.025, 0.5, 0.975, 1.0)


def _grid(k):
    return -5.0 + np.asarray(k, dtype=np.float64) * 0.01


def test_moments_exact_against_two_pass():
    rng = np.random.default_rng(11)
    x = rng.normal(size=(40, 5, 3)) * 3.0 + 0.5
    mean, var = X.moments(x)
    np.testing.assert_allclose(mean, x.mean(axis=0), rtol=1e-14)
    np.testing.assert_allclose(var, x.var(axis=0, ddof=1), rtol=1e-13)
    # far from zero the exact values are what a two-pass sum in integers gives: 1e8 + {-1, 0, 1} / 4
    m, v = X.moments(np.array([[1e8 - 0.25], [1e8], [1e8 + 0.25]]))
    assert m[0] == 1e8 and v[0] == 0.0625
    assert np.isnan(X.moments(np.ones((1, 2)))[1]).all()


def test_diag_against_numpy_reference():
    from gpirt_amd.chains import diagnostics_from_draws
    rng = np.random.default_rng(12)
    for C_, S in ((1, 4), (2, 9), (3, 17), (2, 36), (4, 101)):
        x = rng.normal(size=(C_, S, 4)) + np.arange(C_)[:, None, None] * 0.3
        signs = [1] + [(-1) ** c for c in range(1, C_)]
        reflect = np.array([True, False, True, True])
        for sg in (None, signs):
            r, e, mc = X.diag(x, sg, reflect if sg else None)
            d = diagnostics_from_draws(x, sg, reflect if sg else None)
            np.testing.assert_allclose(r, d["rhat"], rtol=1e-12, err_msg=f"rhat C={C_} S={S}")
            np.testing.assert_allclose(e, d["ess"], rtol=1e-11, err_msg=f"ess C={C_} S={S}")
            np.testing.assert_allclose(mc, d["mcse"], rtol=1e-12, err_msg=f"mcse C={C_} S={S}")
            pm, pv = X.pooled_moments(x, sg, reflect if sg else None)
            np.testing.assert_allclose(pm, d["mean"], rtol=1e-13, atol=1e-15)
            np.testing.assert_allclose(pv, d["var"], rtol=1e-13)


def test_diag_hand_worked_two_chains_s9():
    """test_chains_cpu's hand-worked case: R-hat sqrt(10.625 / 1.5), ESS 18 x 4.25 / 14, MCSE sqrt(14 / 18)."""
    x = [[1, 2, 3, 4, 5, 6, 7, 8, 9], [0, 2, 0, 2, 1, 2, 0, 2, 0]]
    r, e, mc = X.diag_value([list(map(float, c)) for c in x])
    assert r == pytest.approx(math.sqrt(10.625 / 1.5), rel=2e-16)
    assert e == float(Fraction(18 * 17, 4 * 14))                # exact: 18 x 4.25 / 14
    assert mc == pytest.approx(math.sqrt(14 / 18), rel=2e-16)


def test_diag_edges():
    from gpirt_amd.chains import diagnostics_from_draws
    rng = np.random.default_rng(3)
    for S in (1, 2, 3):                                           # S < 4: R-hat NaN; S = 1: one batch, no ESS
        x = rng.standard_normal((2, S, 3))
        r, e, mc = X.diag(x)
        d = diagnostics_from_draws(x)
        assert np.isnan(r).all()
        np.testing.assert_allclose(e, d["ess"], rtol=1e-12)
        np.testing.assert_allclose(mc, d["mcse"], rtol=1e-12)
        assert np.isnan(e).all() == (S == 1)
    c = np.zeros((2, 8, 3))
    c[1, :, 0] = 1.0                                              # W = 0, B > 0: +inf
    c[:, 4:, 2] = 2.0                                             # each chain constant within each half, halves apart
    r, e, mc = X.diag(c)
    assert r[0] == math.inf and np.isnan(r[1]) and r[2] == math.inf
    # sigma^2 = 0: every batch mean equal.  Chains that vary: ESS = x / 0 = +inf, MCSE 0; every draw equal: NaN, MCSE 0
    alt = np.tile([0.0, 1.0, 1.0, 0.0], 4)                        # S = 16: b = 4, each batch sums to 2
    r, e, mc = X.diag(np.stack([alt, alt])[:, :, None])
    assert e[0] == math.inf and mc[0] == 0.0
    r, e, mc = X.diag(np.full((2, 16, 1), 3.0))
    assert np.isnan(e[0]) and mc[0] == 0.0 and np.isnan(r[0])
    s = X.block_scalars(np.array([1.0, np.nan, 1.2, np.inf]), np.array([10.0, 3.0, np.nan, 5.0]))
    assert s == dict(max_rhat=np.inf, min_ess=3.0, n_rhat_high=2.0, n_rhat_nan=1.0, n_ess_nan=1.0)
    assert np.isnan(X.block_scalars([np.nan], [np.nan])["max_rhat"])


def test_waic_against_numpy_reference():
    from test_gpu_summary import ref_summary
    rng = np.random.default_rng(13)
    S, n, m = 12, 5, 3
    y = np.where(rng.random((n, m)) < 0.5, 1.0, -1.0)
    y[1, 2] = np.nan
    f = rng.normal(scale=2.0, size=(n, m, S))
    mu = rng.normal(scale=3.0, size=(n, m, S))
    g = np.moveaxis(f + mu, 2, 0)
    ex = X.waic(y, g)
    want, tot = ref_summary(y, np.zeros((S, n)), np.zeros((2, m, S)), f, mu)
    for k in ("p_yes", "lppd", "p_waic"):
        np.testing.assert_allclose(ex[k], want[k], rtol=1e-12, atol=1e-15, err_msg=k)
    for k, v in tot.items():
        assert ex["totals"][k] == pytest.approx(v, rel=1e-12), k
    # the extremes: P(y = 1) and ll at g = +-745 and beyond are exact limits, not overflow
    c = X.waic_cell(1.0, [745.0, 1e4])
    assert float(c["p_yes"]) == 1.0 and -1e-300 < float(c["lppd"]) <= 0.0
    c = X.waic_cell(1.0, [-1e4, -1e4])
    assert float(c["lppd"]) == -1e4 and float(c["p_waic"]) == 0.0


def _theta_draws(rng, C_, S, n):
    k = np.clip(np.rint(rng.normal(500, 40, size=(C_, S, n))), 0, 1000)
    return _grid(k)


def _against_numpy(th, signs=None):
    from gpirt_amd import quantiles as Q
    a = Q.from_draws(th, None, PROBS, signs=signs)
    h = Q.histograms(th)
    b = Q.from_histograms(draws=th.shape[1], probs=PROBS, signs=signs, **h)
    ex = X.theta_quantities(th, PROBS, signs)
    for ref in (a, b):
        np.testing.assert_array_equal(ex["q"], ref["theta"])
        np.testing.assert_array_equal(ex["median"], ref["theta_median"])
        np.testing.assert_array_equal(ex["mode"], ref["theta_mode"])
        np.testing.assert_array_equal(ex["hist"], ref["theta_hist"])
        for k, r in (("bulk", "bulk"), ("tail", "tail"), ("rhat", "max")):
            np.testing.assert_allclose(ex[k], ref["theta_rhat"][r], rtol=1e-12, err_msg=k)
    np.testing.assert_array_equal(ex["off"], h["theta_off_grid"].sum(axis=0))
    return ex


@pytest.mark.parametrize("C_,S", [(1, 9), (2, 10), (3, 11), (2, 3)])
def test_theta_quantities_against_numpy(C_, S):
    rng = np.random.default_rng(100 * C_ + S)
    _against_numpy(_theta_draws(rng, C_, S, 6))


def test_theta_reflection_and_edges_against_numpy():
    rng = np.random.default_rng(9)
    th = _theta_draws(rng, 3, 12, 6)
    th[:, :, 4] = _grid(rng.choice([0, 1000], size=(3, 12)))      # only the two ends
    _against_numpy(th, signs=[1, -1, 1])
    th = _theta_draws(rng, 2, 10, 5)                               # test_quantiles_cpu's constant chains and off grid
    th[:, :, 0] = _grid(321)
    th[0, :, 1] = _grid(400)
    th[1, :, 1] = _grid(410)
    th[1, 3, 2] = 0.123456
    th[0, 7, 3] = np.nan
    ex = _against_numpy(th)
    assert np.isnan(ex["bulk"][0]) and ex["bulk"][1] == math.inf and np.isnan(ex["tail"][1])
    assert np.isnan(ex["q"][:, 2:4]).all() and ex["off"].tolist() == [0, 0, 1, 1, 0]
    assert X.grid_k(-0.0) == 500 and X.grid_k(1e308) == -1 and X.grid_k(np.nextafter(-5.0, 0)) == -1


def test_hand_worked_rank_rhat():
    """test_quantiles_cpu's hand-worked case: the ranks and scores by plain Python (statistics.NormalDist)."""
    import statistics
    ks = [[10, 12, 12, 11, 30, 13, 12, 10, 11], [14, 12, 15, 15, 16, 14, 13, 15, 12]]
    nd = statistics.NormalDist()

    def rhat(vals):
        flat = sorted(v for h in vals for v in h)
        T = len(flat)
        rank = {v: (flat.index(v) + 1 + T - flat[::-1].index(v)) / 2.0 for v in flat}
        z = [[nd.inv_cdf((rank[v] - 0.375) / (T + 0.25)) for v in h] for h in vals]
        N, M = 4, 4
        means = [sum(h) / N for h in z]
        grand = sum(means) / M
        B = N / (M - 1) * sum((x - grand) ** 2 for x in means)
        W = sum(sum((v - mu) ** 2 for v in h) / (N - 1) for h, mu in zip(z, means)) / M
        return math.sqrt(((N - 1) / N * W + B / N) / W)

    halves = [k[:4] for k in ks] + [k[5:] for k in ks]
    ex = X.theta_quantities(_grid(ks)[:, :, None], PROBS)
    assert ex["bulk"][0] == pytest.approx(rhat(halves), rel=1e-13)
    assert ex["tail"][0] == pytest.approx(rhat([[abs(2 * v - 25) for v in h] for h in halves]), rel=1e-13)


def test_band_against_numpy():
    from gpirt_amd import quantiles as Q
    rng = np.random.default_rng(14)
    C_, S, m = 2, 7, 2
    f = rng.normal(scale=2.5, size=(C_, S, 1001, m))
    f[0, 3, 9, 1] = np.nan
    f[1, :, 5, 0] = 0.0
    import mpmath
    with mpmath.workprec(200):
        edges = [X._f(mpmath.log(mpmath.mpf(b) / (256 - b))) for b in range(1, 256)]
    a = Q.from_draws(np.zeros((C_, S, 1)), f, PROBS, signs=[1, -1], edges=np.array(edges))
    ex = X.irf_quantities(f, PROBS, signs=[1, -1])
    np.testing.assert_array_equal(ex["nan"] > 0, np.isnan(a["irf_p_mean"]))
    assert ex["nan"].sum() == 1
    np.testing.assert_allclose(ex["p_mean"], a["irf_p_mean"], rtol=1e-13)
    np.testing.assert_allclose(ex["q"], a["irf_exact"], rtol=1e-15, atol=0)      # the same order statistics (NumPy's
    #                                                                              plogis rounds twice)
    h = Q.histograms(np.zeros((C_, S, 1)), f, edges=np.array(edges))
    for c in range(C_):
        for d in (0, S - 1):
            for k in (0, 5, 9, 1000):
                for j in range(m):
                    x = f[c, d, k, j]
                    b = X.band_bin(x, edges)
                    if b >= 0:
                        assert h["irf_band"][c, b, k, j] >= 1
                        assert b == X.exact_bin(x)                              # no draw here is near an edge
    assert X.exact_bin(0.0) == 128 and X.exact_bin(math.inf) == 255 and X.exact_bin(-math.inf) == 0
    assert X.band_bin(math.nan, edges) == -1 and X.band_bin(-0.0, edges) == 128
