"""Quantiles on the device (include/gpirt_hip.h GPIRT_SUM_THETA_HIST, GPIRT_SUM_IRF_BAND, gpirt_summary_quantiles,
gpirt_mcmc_run) against NumPy over the stored draws: exact histograms and theta quantiles, the band interpolation
and its 1/256 bound, E[P], the rank-normalised R-hat; several chains with the reflection; the R-stream chain; the new parts
leaving every existing output alone; a hang-guard rollback; the metric size."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
CODES = dict(yea=[1], nay=[-1], missing=[None])
PROBS = (0.0, 0.025, 0.5, 0.975, 1.0)


@pytest.fixture(scope="module")
def handle():
    from gpirt_amd.ops import Handle
    h = Handle(0)
    yield h
    h.close()


def _data(n, m, seed=11):
    from gpirt_amd.response_matrix import as_response_matrix
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=seed)
    return np.asarray(as_response_matrix(y, CODES), dtype=np.float64), th0


def _run_stage(handle, y, th0, S, seed, parts, fast=False):
    """B = 1, then S draws through the stage API; theta and f* of every draw read back.  Returns (sampler, theta (S, n),
    fstar (S, 1001, m))."""
    from gpirt_amd import Sampler
    s = Sampler(handle, y, th0, preset="fast", seed=seed) if fast else Sampler(handle, y, th0, seed=seed)
    s.init()
    s.step()
    s.check()
    s.summary_enable(parts, planned_draws=S)
    th, fs = [], []
    for _ in range(S):
        s.step()
        s.accumulate_irf()
        s.summary_accumulate()
        s.check()
        th.append(s.get("theta"))
        fs.append(s.get("fstar"))
    return s, np.stack(th), np.stack(fs)


def check_quantiles(got, want, what=""):
    """device (from_states / gpirtMCMC) against quantiles.from_draws"""
    for k in ("theta", "theta_median", "theta_mode", "theta_hist"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=what + k)
    for k in ("bulk", "tail", "max"):
        np.testing.assert_allclose(got["theta_rhat"][k], want["theta_rhat"][k], rtol=1e-10, atol=1e-10, err_msg=what + k)
    if "irf_exact" in want:
        np.testing.assert_allclose(got["irf"], want["irf"], rtol=0, atol=1e-12, err_msg=what + "irf")
        ok = ~np.isnan(want["irf_exact"])
        assert np.abs(got["irf"][ok] - want["irf_exact"][ok]).max() <= 1.0 / 256 + 1e-12
        np.testing.assert_allclose(got["irf_p_mean"], want["irf_p_mean"], rtol=1e-12, err_msg=what + "irf_p_mean")


@pytest.mark.parametrize("n,m", [(256, 32), (1024, 64)])
def test_stage_api_against_numpy(handle, n, m):
    from gpirt_amd import _lib
    from gpirt_amd import quantiles as Q
    y, th0 = _data(n, m, seed=n + m)
    S = 41
    s, th, fs = _run_stage(handle, y, th0, S, 7, ("theta_hist", "irf_band", "diag"))
    assert s._sum_parts & _lib.SUM_DIAG
    want_h = Q.histograms(th[None], fs[None])
    for k in ("theta_hist", "theta_hist_h1", "theta_hist_h2", "theta_off_grid", "irf_nan", "irf_band"):
        np.testing.assert_array_equal(s.summary_get(k), want_h[k][0], err_msg=k)
    assert want_h["theta_off_grid"].sum() == 0 and want_h["irf_nan"].sum() == 0
    np.testing.assert_allclose(s.summary_get("irf_p_mean"), want_h["irf_psum"][0] / S, rtol=1e-12)
    got = Q.from_states(handle, [s], PROBS)
    want = Q.from_draws(th[None], fs[None], PROBS)
    check_quantiles(got, want)
    T = S
    for p, q in enumerate(PROBS):                       # the order statistic itself, C = 1
        np.testing.assert_array_equal(got["theta"][p], np.sort(th, axis=0)[max(math.ceil(q * T), 1) - 1])
    sc = got["scalars"]
    assert sc["draws"] == S and sc["theta_off_grid"] == 0 and sc["irf_nan"] == 0
    assert sc["irf_count_min"] == S and sc["irf_count_max"] == S
    r = want["theta_rhat"]["max"]
    assert sc["n_rhat_nan"] == np.isnan(r).sum() and sc["n_rhat_high"] == (r[~np.isnan(r)] > 1.01).sum()
    np.testing.assert_allclose(sc["max_rhat"], np.nanmax(r), rtol=1e-10)
    # the histogram algebra agrees too
    b = Q.from_histograms(draws=S, probs=PROBS, **{k: v for k, v in want_h.items()})
    np.testing.assert_array_equal(got["theta"], b["theta"])
    s.close()


def test_chains_reflection_and_forced_signs(handle):
    """Three chains on the stage API, the second started in the mirror mode: align reflects it exactly as chains.combine
    does; forced signs too."""
    from gpirt_amd import _lib, chains
    from gpirt_amd import quantiles as Q
    y, th0 = _data(256, 24, seed=3)
    S = 12
    parts = ("theta_hist", "irf_band", "diag")
    runs = [_run_stage(handle, y, t0, S, 11 + c, parts) for c, t0 in enumerate((th0, -th0, th0))]
    ss = [r[0] for r in runs]
    th = np.stack([r[1] for r in runs])
    fs = np.stack([r[2] for r in runs])
    comb = chains.combine(handle, ss)
    got = Q.from_states(handle, ss, PROBS)
    np.testing.assert_array_equal(got["reflected"], comb["diagnostics"]["reflected"])
    signs = np.where(got["reflected"], -1, 1)
    check_quantiles(got, Q.from_draws(th, fs, PROBS, signs=signs), "align ")
    forced = [1, -1, -1]
    rev = PROBS[::-1]                                       # the band is read in one pass, whatever the order of q
    got = Q.from_states(handle, ss, rev, signs=forced)
    assert list(got["reflected"]) == [False, True, True]
    check_quantiles(got, Q.from_draws(th, fs, rev, signs=forced), "forced ")
    assert got["scalars"]["draws"] == 3 * S
    assert got["scalars"]["irf_count_min"] == 3 * S and got["scalars"]["irf_count_max"] == 3 * S
    for s in ss:
        s.close()


def test_new_parts_leave_everything_else_alone(handle):
    from gpirt_amd import _lib, chains
    y, th0 = _data(300, 20, seed=5)
    S = 8
    base = _lib.SUM_WAIC | _lib.SUM_PRED | _lib.SUM_F | _lib.SUM_DIAG
    a, tha, fa = _run_stage(handle, y, th0, S, 3, base)
    b, thb, fb = _run_stage(handle, y, th0, S, 3, base | _lib.SUM_THETA_HIST | _lib.SUM_IRF_BAND)
    np.testing.assert_array_equal(tha, thb)
    np.testing.assert_array_equal(fa, fb)
    sa, sb = a.summary(), b.summary()
    assert sa.keys() == sb.keys()
    for k in sa:
        if k == "totals":
            assert sa[k] == sb[k]
        else:
            np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)
    ca, cb = chains.combine(handle, [a]), chains.combine(handle, [b])
    np.testing.assert_array_equal(ca["IRFs"], cb["IRFs"])
    for k, v in ca["diagnostics"].items():
        if k != "scalars":
            np.testing.assert_array_equal(v, cb["diagnostics"][k], err_msg=k)
    # the state block: the same bytes up to the new arrays, which follow
    sta, stb = a.summary_state().cpu().numpy(), b.summary_state().cpu().numpy()
    hdr = sta[:8].view(np.int64).copy(), stb[:8].view(np.int64).copy()
    assert hdr[1][2] == hdr[0][2] | _lib.SUM_THETA_HIST | _lib.SUM_IRF_BAND and hdr[1][7] == 0
    np.testing.assert_array_equal(sta[8:], stb[8:sta.size])
    a.close()
    b.close()


def _mcmc(y, th0, S, B, **kw):
    from gpirt_amd import gpirtMCMC
    return gpirtMCMC(y, S, B, vote_codes=CODES, theta_init=th0, theta_stabilise=True, **kw)


def test_mcmc_quantiles_item_chains_match_mcmc_chains():
    from gpirt_amd import quantiles as Q
    y, th0 = _data(300, 40)
    inits = np.stack([th0, -th0, np.roll(th0, 7)])
    kw = dict(rng="item", seed=29, chains=3, summaries=("waic", "pred"))
    plain = _mcmc(y, inits, 10, 2, **kw)
    got = _mcmc(y, inits, 10, 2, quantiles=PROBS, **kw)
    for k in ("theta", "beta", "f", "IRFs"):
        np.testing.assert_array_equal(got[k], plain[k], err_msg=k)
    for k, v in plain["summary"].items():
        if k == "totals":
            assert got["summary"][k] == v
        else:
            np.testing.assert_array_equal(got["summary"][k], v, err_msg=k)
    for k, v in plain["diagnostics"].items():
        if k != "scalars":
            np.testing.assert_array_equal(got["diagnostics"][k], v, err_msg=k)
    for b, v in plain["diagnostics"]["scalars"].items():                     # NaN where plain has NaN
        np.testing.assert_array_equal([got["diagnostics"]["scalars"][b][k] for k in v], list(v.values()), err_msg=b)
    qq = got["quantiles"]
    np.testing.assert_array_equal(qq["reflected"], plain["diagnostics"]["reflected"])
    signs = np.where(qq["reflected"], -1, 1)
    want = Q.from_draws(got["theta"][:, 1:], None, PROBS, signs=signs)
    check_quantiles(qq, want)
    assert qq["irf"].shape == (len(PROBS), 1001, 40) and np.isfinite(qq["irf"]).all()
    assert np.all(np.diff(qq["irf"], axis=0) >= 0)
    assert qq["scalars"]["theta_off_grid"] == 0 and qq["scalars"]["irf_nan"] == 0 and qq["scalars"]["draws"] == 30


def test_mcmc_quantiles_rstream_is_mcmc_summary():
    from gpirt_amd import quantiles as Q
    from gpirt_amd.ops import RStream
    y, th0 = _data(100, 40, seed=2)
    rs0, rs1 = RStream(4321), RStream(4321)
    plain = _mcmc(y, th0, 8, 2, rng="reference", rstream=rs0, summaries=("waic", "pred", "f"))
    got = _mcmc(y, th0, 8, 2, rng="reference", rstream=rs1, summaries=("waic", "pred", "f"), quantiles=(0.1, 0.5, 0.9))
    for k in ("theta", "beta", "f", "IRFs"):
        np.testing.assert_array_equal(got[k], plain[k], err_msg=k)
    st0, st1 = rs0.state(), rs1.state()
    assert np.array_equal(np.asarray(st0[0]), np.asarray(st1[0])) and st0[1] == st1[1]
    for k, v in plain["summary"].items():
        if k == "totals":
            assert got["summary"][k] == v
        else:
            np.testing.assert_array_equal(got["summary"][k], v, err_msg=k)
    want = Q.from_draws(got["theta"][None, 1:], None, (0.1, 0.5, 0.9))
    check_quantiles(got["quantiles"], want)


@pytest.mark.parametrize("S,B,nth", [(3, 2, 3)])
def test_quantiles_survive_a_rollback(S, B, nth):
    """The iterations repeated after a hang-guard rollback are counted once: S draws per respondent, the undisturbed run's
    histograms and bands."""
    from gpirt_amd import _lib
    from gpirt_amd.synthetic import make_responses
    lib = _lib.load()
    y, th0 = make_responses(2600, 12, seed=100 + 2600 + 12)
    kw = dict(rng="item", seed=29, quantiles=PROBS, store_draws=False)
    ref = _mcmc(y, th0, S, B, **kw)
    assert lib.gpirt_debug_last_mcmc_fallbacks() == 0
    _lib.check(lib.gpirt_debug_trip_guard(None, nth))
    got = _mcmc(y, th0, S, B, **kw)
    assert lib.gpirt_debug_last_mcmc_fallbacks() == 1
    q0, q1 = ref["quantiles"], got["quantiles"]
    assert (q1["theta_hist"].sum(axis=0) == S).all()
    np.testing.assert_array_equal(q1["theta_hist"], q0["theta_hist"])
    np.testing.assert_array_equal(q1["theta"], q0["theta"])
    # f* after the rollback equals the undisturbed one to rounding (the repeated iterations factor on the fallback panel)
    np.testing.assert_allclose(q1["irf_p_mean"], q0["irf_p_mean"], rtol=1e-10, atol=1e-10)
    # per f* cell: exactly S draws in the band (none lost, none counted twice), as in the undisturbed run
    for q in (q0, q1):
        assert q["scalars"]["irf_nan"] == 0 and q["scalars"]["draws"] == S
        assert q["scalars"]["irf_count_min"] == S and q["scalars"]["irf_count_max"] == S
    np.testing.assert_allclose(q1["irf"], q0["irf"], rtol=0, atol=1e-9)


def test_metric_size_counts(handle):
    """8192 x 1024, the fast preset, 3 draws: every respondent's and every cell's counts sum to the draws, none off the
    grid, no NaN."""
    import torch
    from gpirt_amd import _lib
    from gpirt_amd import quantiles as Q
    from gpirt_amd.synthetic import CONFIGS, make_responses
    n, m = CONFIGS["M"]
    y, th0 = make_responses(n, m, seed=20240)
    S = 3
    s, th, _ = _run_stage(handle, y, th0, S, 5, ("theta_hist", "irf_band", "diag"), fast=True)
    h = s.summary_get("theta_hist")
    assert (h.sum(axis=0) == S).all() and s.summary_get("theta_off_grid").sum() == 0
    np.testing.assert_array_equal(h, Q.histograms(th[None])["theta_hist"][0])
    assert s.summary_get("irf_nan").sum() == 0
    st = s.summary_state()
    nb = 256 * 1001 * m                                  # the band: the block's last array, uint32, bin-major
    words = (nb + 1) // 2
    words += words & 1
    band = st[st.numel() - words:].view(torch.int32)[:nb].view(256, m * 1001)
    tot = band.sum(dim=0, dtype=torch.int64)
    assert bool((tot == S).all()), (int(tot.min()), int(tot.max()))
    got = Q.from_states(handle, [s], (0.975, 0.025))                       # any order of the probabilities
    assert got["scalars"]["theta_off_grid"] == 0 and got["scalars"]["irf_nan"] == 0
    assert got["scalars"]["irf_count_min"] == S and got["scalars"]["irf_count_max"] == S
    assert np.isfinite(got["irf"]).all() and (got["irf"][1] <= got["irf"][0]).all()
    s.close()
