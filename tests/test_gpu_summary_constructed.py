"""The summary, chain and quantile kernels (csrc/summary.hip) fed constructed draws through the stage API -- Sampler.set of
theta, beta, f, mu and f*, then summary_accumulate (and accumulate_irf) -- and held against the exact reference
(tests/_exact_summary.py, checked against the NumPy references in test_exact_summary_cpu.py).  The values are the ones
an MCMC run of a few draws never reaches: moments far from zero, linear predictors up to +-1e4, W = 0 and sigma^2 = 0,
S far from a perfect square, seven chains, the grid's ends, theta off the grid, NaN / +-inf, f* exactly on a band edge,
a reflected chain."""
import math

import numpy as np
import pytest

import _exact_summary as X

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
PROBS = (0.0, 0.025, 0.5, 0.975, 1.0)
NG = 1001


def _sampler(handle, y, parts, S):
    """A small Sampler, init() once, summaries `parts` on with S planned draws."""
    from gpirt_amd import Sampler, _lib
    s = Sampler(handle, y, np.zeros(y.shape[0]), rng="item", seed=5, theta_stabilise=True)
    s.init()
    s.summary_enable(_lib.summary_parts(parts), planned_draws=S)
    return s


def _feed(s, draws, irf=False):
    """Each draw: Sampler.set of every array it names, then accumulate_irf (irf) and summary_accumulate."""
    for vals in draws:
        for k, v in vals.items():
            s.set(k, v)
        if irf:
            s.accumulate_irf()
        s.summary_accumulate()


def _same_nan(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), what
    return ~np.isnan(want) & ~inf


def _rel(got, want, rtol, what, floor=0.0):
    """|got - want| <= rtol |want| + floor wherever want is finite; NaN and +-inf exactly where want has them.
    Returns the largest |got - want| / |want| seen (the measured tolerance)."""
    ok = _same_nan(got, want, what)
    g, w = np.asarray(got, dtype=np.float64)[ok], np.asarray(want, dtype=np.float64)[ok]
    if not ok.any():
        return 0.0
    fl = np.broadcast_to(np.asarray(floor, dtype=np.float64), np.shape(want))[ok]
    err = np.abs(g - w)
    assert (err <= rtol * np.abs(w) + fl).all(), f"{what}: worst {(err / np.maximum(np.abs(w), 1e-300)).max():.3e}"
    return float((err / np.maximum(np.abs(w), 1e-300)).max())


def _report(name, value):
    print(f"MEASURED {name} {value:.3e}")


# --------------------------------------------------------------------------------- (a) moments far from zero -------
@pytest.mark.parametrize("offset,var_rtol", [(1e8, 1e-6), (1e12, 1e-3)])
def test_moments_far_from_zero(handle, offset, var_rtol):
    """theta, beta, f = offset + u, u ~ U[-1, 1], S = 4096, 33 x 3 (an odd cell count): Welford keeps the variance of a
    spread of 1 at 1e8 (a one-pass sum of squares is off by a factor of about 85 there, by 1e10 at 1e12)."""
    n, m, S = 33, 3, 4096
    rng = np.random.default_rng(int(offset) % 997)
    th = offset + rng.uniform(-1, 1, (S, n))
    be = offset + rng.uniform(-1, 1, (S, 2, m))
    ff = offset + rng.uniform(-1, 1, (S, n, m))
    s = _sampler(handle, np.ones((n, m)), ("f",), S)
    _feed(s, [dict(theta=th[d], beta=be[d], f=ff[d]) for d in range(S)])
    sm = s.summary()
    s.close()
    worst_m, worst_v = 0.0, 0.0
    for k, x in (("theta", th), ("beta", be), ("f", ff)):
        mean, var = X.moments(x)
        worst_m = max(worst_m, _rel(sm[k + "_mean"], mean, 1e-14, k + "_mean"))
        worst_v = max(worst_v, _rel(sm[k + "_var"], var, var_rtol, k + "_var"))
    _report(f"moments_mean_rtol@{offset:g}", worst_m)
    _report(f"moments_var_rtol@{offset:g}", worst_v)


def test_pooled_moments_five_chains_far_apart(handle):
    """Five chains whose means differ by 1e8, pooled by Chan's formula in gpirt_chains_combine."""
    from gpirt_amd import chains
    n, m, S, C = 7, 1, 256, 5
    rng = np.random.default_rng(41)
    th = 1e8 * np.arange(1, C + 1)[:, None, None] + rng.uniform(-1, 1, (C, S, n))
    be = 1e8 * np.arange(1, C + 1)[:, None, None, None] + rng.uniform(-1, 1, (C, S, 2, m))
    ff = 1e8 * np.arange(1, C + 1)[:, None, None, None] + rng.uniform(-1, 1, (C, S, n, m))
    ss = []
    for c in range(C):
        s = _sampler(handle, np.ones((n, m)), ("f",), S)
        _feed(s, [dict(theta=th[c, d], beta=be[c, d], f=ff[c, d]) for d in range(S)])
        ss.append(s)
    out = chains.combine(handle, ss, align=False)["summary"]
    for s in ss:
        s.close()
    worst_m, worst_v = 0.0, 0.0
    for k, x in (("theta", th), ("beta", be), ("f", ff)):
        mean, var = X.pooled_moments(x)
        worst_m = max(worst_m, _rel(out[k + "_mean"], mean, 1e-14, "pooled " + k + "_mean"))
        worst_v = max(worst_v, _rel(out[k + "_var"], var, 1e-12, "pooled " + k + "_var"))
    _report("pooled_mean_rtol", worst_m)
    _report("pooled_var_rtol", worst_v)


# ------------------------------------------------------------------------ (b) WAIC and pred at extreme predictors ---
G = (0.0, 1e-8, -1e-8, 20.0, -20.0, 37.0, -37.0, 40.0, -40.0, 709.0, -709.0, 745.0, -745.0, 1e4, -1e4)


def test_waic_and_pred_at_extreme_predictors(handle):
    """g = f + mu around each value of G for y = +1 and -1 (n = 15 x m = 5, 75 cells).  Column 0: g constant
    (p_waic exactly 0); 1: a relative jitter of 1e-3; 2: g and -g mixed; 3: jitter with NaN cells; 4: every y missing."""
    n, m, S = len(G), 5, 200
    rng = np.random.default_rng(7)
    y = np.where((np.arange(n)[:, None] + np.arange(m)[None, :]) % 2 == 0, 1.0, -1.0)
    y[[2, 9, 13], 3] = np.nan
    y[:, 4] = np.nan
    base = np.array(G)[:, None] * np.ones((1, m))
    u = rng.uniform(-1, 1, (S, n, m))
    g = np.broadcast_to(base, (S, n, m)).copy()
    g[:, :, 1] = base[:, 1] * (1 + 1e-3 * u[:, :, 1]) + 1e-3 * u[:, :, 1]
    g[:, :, 2] = np.where(u[:, :, 2] > 0, base[:, 2], -base[:, 2]) + 0.25 * u[:, :, 0]
    g[:, :, 3] = base[:, 3] * (1 + 1e-2 * u[:, :, 3])
    g[:, :, 4] = base[:, 4] + u[:, :, 4]
    mu = np.round(g * 0.5)                                      # f + mu == g is what the kernel sees; the reference
    f = g - mu                                                  # takes fl(f + mu)
    gk = f + mu
    s = _sampler(handle, y, ("waic", "pred", "f"), S)
    _feed(s, [dict(f=f[d], mu=mu[d]) for d in range(S)])
    assert np.array_equal(s.get("mu"), mu[-1]) and np.array_equal(s.get("f"), f[-1])
    sm = s.summary()
    s.close()
    ex = X.waic(y, gk)
    logS = math.log(S)
    # lppd: lse - log S leaves ~ eps (|lppd| + log S) absolutely (g = 40: 2e-15 against a true lppd of -4e-18)
    lp_floor = 8 * EPS * (np.abs(np.nan_to_num(ex["lppd"])) + logS)
    ok = _same_nan(sm["lppd"], ex["lppd"], "lppd")
    err = np.abs(sm["lppd"] - ex["lppd"])[ok]
    assert (err <= lp_floor[ok]).all(), f"lppd: worst {(err / lp_floor[ok]).max():.3f} of the bound"
    _report("lppd_abs_in_units_of_eps(|lppd|+logS)", float((err / (EPS * (np.abs(ex['lppd'][ok]) + logS))).max()))
    # p_yes: a sum of S values in [0, 1], 4 S eps relative, plus the subnormal steps of plogis(-745)
    _report("p_yes_rtol", _rel(sm["p_yes"], ex["p_yes"], 4 * S * EPS, "p_yes", floor=S * 2.0 ** -1074 * 4))
    # p_waic: relative to its size, plus an absolute floor from ll's own rounding (|ll| eps per draw)
    llmax = np.maximum(np.abs(gk).max(axis=0), 1.0)
    pw = np.nan_to_num(ex["p_waic"])
    pw_floor = 8 * EPS * llmax * np.sqrt(pw) + (8 * EPS * llmax) ** 2
    _report("p_waic_rtol", _rel(sm["p_waic"], ex["p_waic"], 1e-9, "p_waic", floor=pw_floor))
    # f moments of the same draws
    fm, fv = X.moments(f)
    _rel(sm["f_mean"], fm, 1e-14, "f_mean", floor=1e-300)
    _rel(sm["f_var"], fv, 1e-12, "f_var", floor=1e-300)
    tot, et = sm["totals"], ex["totals"]
    obs = ~np.isnan(y)
    assert tot["n_obs"] == et["n_obs"] == obs.sum() and tot["draws"] == S
    lp_tot = lp_floor[obs].sum() + 8 * EPS * obs.sum() * np.abs(ex["lppd"][obs]).sum()
    pw_tot = 1e-9 * pw[obs].sum() + pw_floor[obs].sum() + 8 * EPS * obs.sum() * pw[obs].sum()
    assert abs(tot["lppd"] - et["lppd"]) <= lp_tot
    assert abs(tot["p_waic"] - et["p_waic"]) <= pw_tot
    assert abs(tot["elpd_waic"] - et["elpd_waic"]) <= lp_tot + pw_tot
    assert abs(tot["waic"] - et["waic"]) <= 2 * (lp_tot + pw_tot)
    for k in ("se_elpd_waic", "elpd_mean", "elpd_ss"):
        assert tot[k] == pytest.approx(et[k], rel=1e-9), k
    _report("totals_se_rtol", abs(tot["se_elpd_waic"] - et["se_elpd_waic"]) / et["se_elpd_waic"])


# ---------------------------------------------------------------------------------------- (c) DIAG bookkeeping ------
SWEEP = (2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 35, 36, 37, 99, 100, 101, 1023, 1025)


def _sweep_value(d, c, v):
    """draw d (1-based) of chain c, value v: (d + 0.37 c + 0.11 v)^2 mod 97 -- a different sequence per value and chain,
    so a draw in the wrong half or batch moves R-hat, ESS and MCSE"""
    return ((d + 0.37 * c + 0.11 * v) ** 2) % 97.0


def _diag_check(out, th, be, ff, what, rtol=1e-12):
    """the device diagnostics against the exact ones; th (C, S, n), be (C, S, 2, m), ff (C, S, n, m)"""
    dg = out["diagnostics"]
    worst = 0.0
    for b, x in (("theta", th), ("beta", be), ("f", ff)):
        r, e, mc = X.diag(x)
        worst = max(worst, _rel(dg[b + "_rhat"], r, rtol, f"{what} {b}_rhat"))
        worst = max(worst, _rel(dg[b + "_ess"], e, rtol, f"{what} {b}_ess"))
        worst = max(worst, _rel(dg[b + "_mcse"], mc, rtol, f"{what} {b}_mcse", floor=1e-300))
        want = X.block_scalars(r, e)
        got = dg["scalars"][b]
        for k, v in want.items():
            assert (math.isnan(v) and math.isnan(got[k])) or got[k] == pytest.approx(v, rel=rtol), (what, b, k)
    return worst


def test_diag_sweep_of_chain_lengths(handle):
    """S from 2 to 1025 (odd S, S around perfect squares, a b < S), C = 1, 2 and 7 chains, f on, 7 x 1 (an odd cell
    count: the last cell takes the scalar path)."""
    from gpirt_amd import chains
    n, m, C = 7, 1, 7
    ss = [_sampler(handle, np.ones((n, m)), ("f",), SWEEP[0]) for _ in range(C)]
    worst = 0.0
    for S in SWEEP:
        d = np.arange(1, S + 1, dtype=np.float64)[None, :, None]
        cc = np.arange(C, dtype=np.float64)[:, None, None]
        th = _sweep_value(d, cc, np.arange(n)[None, None, :])
        be = _sweep_value(d[..., None], cc[..., None], 10 + np.arange(2 * m).reshape(1, 1, 2, m))
        ff = _sweep_value(d[..., None], cc[..., None], 20 + np.arange(n * m).reshape(1, 1, n, m))
        for c, s in enumerate(ss):
            s.summary_enable(("f", "diag"), planned_draws=S)
            _feed(s, [dict(theta=th[c, k], beta=be[c, k], f=ff[c, k]) for k in range(S)])
        for nc in (1, 2, 7):
            out = chains.combine(handle, ss[:nc], align=False)
            worst = max(worst, _diag_check(out, th[:nc], be[:nc], ff[:nc], f"S={S} C={nc}"))
    for s in ss:
        s.close()
    _report("diag_sweep_rtol", worst)


def test_diag_w_zero_sigma_zero_and_block_scalars(handle):
    """W = 0 with B > 0 (+inf) and B = 0 (NaN), every batch mean equal (ESS +inf or NaN, MCSE 0), in theta, beta and f
    (the odd last cell included), with the per-block scalars over values that hold NaN and +inf."""
    from gpirt_amd import chains
    n, m, S, C = 7, 1, 16, 2
    d = np.arange(1, S + 1, dtype=np.float64)[None, :, None]
    cc = np.arange(C, dtype=np.float64)[:, None, None]
    halves = np.where(d <= S // 2, 1.0, 2.0)                  # constant within each half, the halves apart
    alt = np.tile([0.0, 1.0, 1.0, 0.0], S // 4)[None, :, None]  # b = 4: every batch sums to 2
    th = _sweep_value(d, cc, np.arange(n)[None, None, :])
    th[:, :, 0] = halves[..., 0]
    th[:, :, 1] = 3.0
    th[:, :, 2] = alt[..., 0]
    be = _sweep_value(d[..., None], cc[..., None], 10 + np.arange(2).reshape(1, 1, 2, 1))
    be[:, :, 1, 0] = 5.0 + cc[..., 0]                         # the slope: each chain constant, the chains apart
    ff = _sweep_value(d[..., None], cc[..., None], 20 + np.arange(n).reshape(1, 1, n, 1))
    ff[:, :, 6, 0] = halves[..., 0]                           # the odd last cell: +inf
    ff[:, :, 5, 0] = 4.0                                      # NaN
    ff[:, :, 4, 0] = alt[..., 0] * 3.0                        # ESS +inf
    ss = []
    for c in range(C):
        s = _sampler(handle, np.ones((n, m)), ("f", "diag"), S)
        _feed(s, [dict(theta=th[c, k], beta=be[c, k], f=ff[c, k]) for k in range(S)])
        ss.append(s)
    out = chains.combine(handle, ss, align=False)
    for s in ss:
        s.close()
    _diag_check(out, th, be, ff, "edges")
    dg = out["diagnostics"]
    assert dg["theta_rhat"][0] == math.inf and np.isnan(dg["theta_rhat"][1]) and dg["beta_rhat"][1, 0] == math.inf
    assert dg["f_rhat"][6, 0] == math.inf and np.isnan(dg["f_rhat"][5, 0])
    assert dg["theta_ess"][2] == math.inf and dg["theta_mcse"][2] == 0.0 and dg["f_ess"][4, 0] == math.inf
    assert np.isnan(dg["theta_ess"][1]) and dg["theta_mcse"][1] == 0.0
    sc = dg["scalars"]
    assert sc["theta"]["max_rhat"] == math.inf and sc["theta"]["n_rhat_nan"] == 1 and sc["theta"]["n_ess_nan"] == 1
    assert sc["f"]["max_rhat"] == math.inf and sc["f"]["n_rhat_nan"] == 1


# ---------------------------------------------------------------------------------- (d) theta histograms, quantiles ---
OFF_GRID = ("above", "below", -5.01, 5.01, np.nan, np.inf, -np.inf, 1e308)


def _theta_case(C, S, finite_only):
    """(C, S, n) theta draws as the sampler writes them (-5.0 + k * 0.01), chain 1 the mirror of chain 0 (k -> 1000 - k,
    a few draws moved), and the respondent roles:
    0..15 every grid point between them; 16 one point throughout; 17 each chain constant, the chains apart; 18 only
    k = 0 and k = 1000; 19 a tie for the mode; 20 -0.0 for k = 500; 21.. one draw off the grid each."""
    nc = 16
    def finite(v):
        return isinstance(v, str) or (np.isfinite(v) and abs(v) < 1e300)
    off = [v for v in OFF_GRID if finite(v) or not finite_only]
    n = 21 + len(off)
    k = np.zeros((C, S, n), dtype=np.int64)
    d = np.arange(S)[None, :, None]
    cc = np.arange(C)[:, None, None]
    k[:, :, :nc] = (np.arange(nc)[None, None, :] * ((NG + nc - 1) // nc) + d + cc * 2) % NG      # 16 x 63 >= 1001
    k[:, :, 16] = 500
    k[:, :, 17] = 400 + 10 * cc[:, :, 0]
    k[:, :, 18] = np.where((d[:, :, 0] + cc[:, :, 0]) % 2 == 0, 0, 1000)
    k[:, :, 19] = np.where(d[:, :, 0] % 2 == 0, 300, 700)
    k[:, :, 20] = (500 + (d[:, :, 0] % 3) - 1 + cc[:, :, 0]) % NG
    k[:, :, 21:] = (250 + d * 11 + cc * 5) % NG
    if C > 1:                                                  # chain 1 in the mirror mode
        k[1] = NG - 1 - k[0]
        k[1, ::5, :16] = (k[1, ::5, :16] + 1) % NG
    th = -5.0 + k * 0.01
    th[:, S // 3, 20] = -0.0                                  # -5 + 5 == -0.0 compares equal: k = 500
    for r, v in enumerate(off):
        i, c, dd = 21 + r, r % C, (3 * r + 1) % S
        g = th[c, dd, i]
        th[c, dd, i] = np.nextafter(g, np.inf) if v == "above" else np.nextafter(g, -np.inf) if v == "below" else v
    return th


def _theta_run(handle, th, parts):
    C, S, n = th.shape
    ss = []
    for c in range(C):
        s = _sampler(handle, np.ones((n, 1)), parts, S)
        _feed(s, [dict(theta=th[c, k]) for k in range(S)])
        ss.append(s)
    return ss


@pytest.mark.parametrize("C,S,mode", [(3, 64, "signs"), (3, 63, "signs"), (3, 63, "align"), (1, 9, "signs")])
def test_theta_histograms_and_quantiles(handle, C, S, mode):
    """Every grid point, both ends under reflection, ties, -0.0, theta off the grid (NaN, +-inf and 1e308 only with forced
    signs: the align rule needs finite theta means), even and odd T, probs {0, 0.025, 0.5, 0.975, 1}."""
    from gpirt_amd import quantiles as Q
    th = _theta_case(C, S, finite_only=(mode == "align"))
    signs = [1, -1, 1][:C] if C > 1 else [1]
    ss = _theta_run(handle, th, ("theta_hist", "diag"))
    if C == 3:
        assert np.isin(np.arange(NG), np.rint((th[:, :, :16] + 5.0) * 100)).all()      # every grid point visited
    per_chain_off = [s.summary_get("theta_off_grid") for s in ss]
    q = Q.from_states(handle, ss, PROBS, signs=signs if mode == "signs" else None, align=(mode == "align"))
    for s in ss:
        s.close()
    ex = X.theta_quantities(th, PROBS, signs)
    assert q["reflected"].tolist() == [sg < 0 for sg in signs]
    np.testing.assert_array_equal(q["theta_hist"], ex["hist"])
    np.testing.assert_array_equal(q["theta"], ex["q"])
    np.testing.assert_array_equal(q["theta_median"], ex["median"])
    np.testing.assert_array_equal(q["theta_mode"], ex["mode"])
    worst = 0.0
    for k, r in (("bulk", "bulk"), ("tail", "tail"), ("rhat", "max")):
        worst = max(worst, _rel(q["theta_rhat"][r], ex[k], 1e-12, "rank R-hat " + k))
    _report(f"rank_rhat_rtol C={C} S={S}", worst)
    np.testing.assert_array_equal(np.sum(per_chain_off, axis=0), ex["off"])
    sc = q["scalars"]
    assert sc["theta_off_grid"] == ex["off"].sum() > 0
    assert ex["hist"][500, 20] >= C and np.isfinite(ex["median"][20])
    assert ex["mode"][19] == -5.0 + 300 * 0.01 or C == 1
    r = ex["rhat"]
    rr = r[~np.isnan(r)]
    assert sc["n_rhat_nan"] == np.isnan(r).sum() and sc["n_rhat_high"] == (rr > 1.01).sum()
    assert (np.isnan(sc["max_rhat"]) and not rr.size) or sc["max_rhat"] == pytest.approx(rr.max(), rel=1e-12)
    if S >= 4 and C > 1:
        assert np.isnan(q["theta_rhat"]["bulk"][16]) and q["theta_rhat"]["bulk"][17] == math.inf


def test_theta_count_above_65536(handle):
    """n = 2, C = 4, S = 17000: 68000 pooled draws on one grid point of respondent 0 (theta histogram only)."""
    from gpirt_amd import quantiles as Q
    C, S = 4, 17000
    ss = []
    for c in range(C):
        s = _sampler(handle, np.ones((2, 1)), ("theta_hist",), S)
        s.set("theta", np.array([-5.0 + 250 * 0.01, -5.0 + (100 + c) * 0.01]))
        for _ in range(S):
            s.summary_accumulate()
        ss.append(s)
    q = Q.from_states(handle, ss, PROBS, align=False)
    for s in ss:
        s.close()
    assert q["theta_hist"][250, 0] == C * S and q["theta_hist"][:, 0].sum() == C * S
    assert [q["theta_hist"][100 + c, 1] for c in range(C)] == [S] * C
    np.testing.assert_array_equal(q["theta"][:, 0], -5.0 + 250 * 0.01)
    np.testing.assert_array_equal(q["theta"][:, 1], [-5.0 + k * 0.01 for k in (100, 100, 101, 103, 103)])
    assert q["theta_mode"][0] == -5.0 + 250 * 0.01 and q["theta_mode"][1] == -5.0 + 100 * 0.01
    assert q["theta_median"][1] == -5.0 + 101 * 0.01


# ------------------------------------------------------------------------------------------------ (e) IRF band ------
def _fstar_values(edges):
    e = np.asarray(edges)
    return np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf),
                           [0.0, -0.0, np.inf, -np.inf, 1e308, -1e308]])


def test_irf_band_on_the_edges(handle):
    """f* on each of the 255 exported edges, one ulp either side of each, +-0, +-inf, +-1e308, some NaN, and normal values,
    over C = 2 chains (chain 1 reflected), m = 3."""
    from gpirt_amd import chains
    from gpirt_amd import quantiles as Q
    m, S, C = 3, 12, 2
    edges = Q.band_edges()
    V = _fstar_values(edges)
    rng = np.random.default_rng(17)
    cell = np.arange(NG * m).reshape(NG, m, order="F")
    f = np.empty((C, S, NG, m))
    for c in range(C):
        for d in range(S):
            f[c, d] = V[(cell * 7 + d * 13 + c * 5) % V.size]
    f[:, :, 600:, 2] = rng.normal(scale=3.0, size=(C, S, NG - 600))          # away from the edges
    f[0, 3, 17, 0] = np.nan
    f[1, 5, 1000, 1] = np.nan                                                 # the reflected chain: pooled at k = 0
    f[1, :, 640, 2] = np.nan
    n = 5
    ss = []
    for c in range(C):
        s = _sampler(handle, np.ones((n, m)), ("irf_band",), S)
        _feed(s, [dict(fstar=f[c, d]) for d in range(S)], irf=True)
        ss.append(s)
    # the bins: the exported-edge rule bit for bit, and the exact bin wherever x is more than 4 ulp from an edge
    el = edges.tolist()
    for c, s in enumerate(ss):
        band = s.summary_get("irf_band")                                      # (256, 1001, m)
        want = np.zeros((256, NG, m))
        for d in range(S):
            for (k, j), x in np.ndenumerate(f[c, d]):
                b = X.band_bin(float(x), el)
                if b >= 0:
                    want[b, k, j] += 1
        np.testing.assert_array_equal(band, want)
        np.testing.assert_array_equal(s.summary_get("irf_nan"), np.isnan(f[c]).sum(axis=0))
    ulp = np.array([math.ulp(x) for x in edges])
    for x in np.unique(f[~np.isnan(f)]):
        if np.all(np.abs(x - edges) > 4 * ulp):
            assert X.band_bin(float(x), el) == X.exact_bin(float(x)), x
    irf_sum = [s.get("irf_sum") for s in ss]
    signs = [1, -1]
    q = Q.from_states(handle, ss, PROBS, signs=signs)
    pooled = chains.combine(handle, ss, signs=signs)
    for s in ss:
        s.close()
    ex = X.irf_quantities(f, PROBS, signs)
    T = C * S
    sc = q["scalars"]
    assert sc["irf_nan"] == np.isnan(f).sum() and sc["irf_count_min"] == T and sc["irf_count_max"] == T
    assert q["reflected"].tolist() == [False, True]
    # E[P]: a sum of T values in [0, 1]; NaN where a NaN draw fell (it enters the sum)
    _report("irf_p_mean_rtol", _rel(q["irf_p_mean"], ex["p_mean"], 4 * T * EPS, "irf_p_mean", floor=1e-300))
    assert np.isnan(q["irf_p_mean"][0, 1]) and np.isnan(q["irf_p_mean"][17, 0]) and np.isnan(q["irf_p_mean"][1000 - 640, 2])
    # band quantiles: NaN where a NaN draw fell, else within 1/256 of the exact sample quantile of plogis(f*)
    ok = _same_nan(q["irf"], ex["q"], "irf_q")
    err = np.abs(q["irf"] - ex["q"])[ok]
    assert err.max() <= 1.0 / 256 + 1e-15, err.max()
    _report("irf_q_abs_in_bins", float(err.max() * 256))
    # the pooled IRFs: the reflected chain's IRF sum reversed along the grid
    with np.errstate(over="ignore"):                          # the sums hold +-inf and +-1e308
        want = 1.0 / (1.0 + np.exp(-((0.0 + irf_sum[0] + irf_sum[1][::-1]) * (1.0 / T))))
        unreversed = 1.0 / (1.0 + np.exp(-((irf_sum[0] + irf_sum[1]) * (1.0 / T))))
    _same_nan(pooled["IRFs"], want, "pooled IRFs")
    fin = np.isfinite(want)
    np.testing.assert_allclose(pooled["IRFs"][fin], want[fin], rtol=4 * EPS, atol=0)
    assert not np.allclose(np.nan_to_num(pooled["IRFs"]), np.nan_to_num(unreversed))         # the reversal shows
