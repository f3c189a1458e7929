"""Posterior predictive checks without a GPU: the NumPy statement of the header (gpirt_amd.ppc.from_draws) -- its Philox
against the oracle's bit for bit, the deterministic replicate, the calibration of the replicate against the
Poisson-binomial variance -- and the C ABI of library version 107 on a machine without a device."""
import ctypes as C

import numpy as np
import pytest

from gpirt_amd import _lib
from gpirt_amd import ppc as P


@pytest.fixture(scope="module")
def lib():
    import os
    from gpirt_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------------ Philox -------
def test_philox_and_uniform_equal_the_oracle_bit_for_bit(oracle):
    """(seed, iter, stage 8, item, index) over a grid with seeds above 2^32 and item / index 0 and 2^32 - 1."""
    assert _lib.ST_PPC == 8
    seeds = (0, 1, 7, 2**32 - 1, 2**32, 2**32 + 5, 0x9E3779B97F4A7C15, 2**64 - 1)
    iters = (0, 1, 2, 1000, 2**31, 2**32 - 1)
    edge = (0, 1, 2, 63, 64, 8191, 2**31, 2**32 - 2, 2**32 - 1)
    item = np.array(edge, dtype=np.uint64)[None, :]
    index = np.array(edge, dtype=np.uint64)[:, None]
    checked = 0
    for seed in seeds:
        for it in iters:
            got = P.item_uniform(seed, it, _lib.ST_PPC, item, index)
            assert got.shape == (len(edge), len(edge))
            for a, i in enumerate(edge):
                for b, j in enumerate(edge):
                    want = oracle.item_uniform(seed, it, 8, j, i)
                    assert got[a, b] == want, (seed, it, j, i, got[a, b], want)
                    checked += 1
    assert checked == len(seeds) * len(iters) * len(edge) ** 2
    # the raw words too
    for ctr, key in (((0, 0, 0, 0), (0, 0)), ((2**32 - 1,) * 4, (2**32 - 1,) * 2), ((1, 2, 8, 3), (0xDEADBEEF, 0x12345678))):
        got = [int(x) for x in P.philox4x32_10(*ctr, *key)]
        assert got == oracle.philox(ctr, key), (ctr, key)
    # the matrix form is the same mapping: u[i, j] = uniform(seed, it, 8, item0 + j, i)
    u = P.replicate_uniforms(2**40 + 3, 5, 4, 3, item0=10)
    for i in range(4):
        for j in range(3):
            assert u[i, j] == oracle.item_uniform(2**40 + 3, 5, 8, 10 + j, i)


# ------------------------------------------------------------------------------------- the deterministic replicate ---
def _y(n, m, rng, nan_frac=0.03):
    y = np.where(rng.random((n, m)) < 0.5, 1.0, -1.0)
    y[rng.random((n, m)) < nan_frac] = np.nan
    return y


def _exact(pair):
    lo, hi = pair
    assert np.array_equal(lo, hi)
    return lo


def test_deterministic_replicate():
    """g = 40 y: p rounds to exactly 1 (u < 1 always) or to 4e-18, below every u (u >= 2^-53): yrep = y in every draw."""
    n, m, S = 23, 7, 5
    rng = np.random.default_rng(3)
    y = _y(n, m, rng)
    y[:, 2] = np.nan                                   # a column and a row without an observed cell
    y[5, :] = np.nan
    g = np.broadcast_to(np.where(np.isnan(y), 1.5, 40.0 * y), (S, n, m))
    out = P.from_draws(y, g, seed=11, iters=range(3, 3 + S))
    assert out["undecided"] == dict(cells=0, comparisons=0)
    obs = ~np.isnan(y)
    for unit, axis in (("item", 0), ("respondent", 1), ("totals", None)):
        d = out[unit]
        n_obs = np.atleast_1d(obs.sum(axis=axis))
        T = np.atleast_1d((y > 0).sum(axis=axis))
        some = n_obs > 0
        assert np.array_equal(_exact(d["n_obs"]), n_obs) and np.array_equal(_exact(d["obs_yes"]), T)
        assert np.array_equal(d["rep_yes_mean"][some], T[some].astype(float))
        assert np.array_equal(d["rep_yes_var"][some], np.zeros(some.sum()))
        assert np.array_equal(_exact(d["yes_ge"])[some], np.full(some.sum(), S))
        assert np.array_equal(_exact(d["yes_gt"])[some], np.zeros(some.sum(), dtype=int))
        assert np.array_equal(_exact(d["dev_ge"])[some], np.full(some.sum(), S))
        assert np.array_equal(d["correct_mean"][some], n_obs[some].astype(float))
        assert np.array_equal(d["dev_obs_mean"][some], d["dev_rep_mean"][some])
        assert np.array_equal(_exact(d["nonfinite"]), np.zeros(len(n_obs), dtype=int))
        # no observed cell: NaN means, counts 0
        for k in ("rep_yes_mean", "rep_yes_var", "dev_obs_mean", "dev_rep_mean", "correct_mean"):
            assert np.isnan(d[k][~some]).all(), (unit, k)
        for k in ("yes_ge", "yes_gt", "dev_ge", "rep_yes_sum", "rep_yes_sumsq", "correct_sum", "n_obs", "obs_yes"):
            assert not _exact(d[k])[~some].any(), (unit, k)
    assert (~(np.atleast_1d(obs.sum(axis=0)) > 0)).sum() == 1 and (~(obs.sum(axis=1) > 0)).sum() == 1


def test_nonfinite_draw_counts_out_its_row_column_and_total():
    n, m, S = 9, 4, 3
    rng = np.random.default_rng(5)
    y = _y(n, m, rng, nan_frac=0.0)
    g = np.array(np.broadcast_to(40.0 * y, (S, n, m)))
    g[1, 2, 3] = np.nan
    g[2, 4, 0] = np.inf
    out = P.from_draws(y, g, seed=1, iters=(1, 2, 3))
    nf_i, nf_r = np.zeros(m, dtype=int), np.zeros(n, dtype=int)
    nf_i[[3, 0]] = 1
    nf_r[[2, 4]] = 1
    assert np.array_equal(_exact(out["item"]["nonfinite"]), nf_i)
    assert np.array_equal(_exact(out["respondent"]["nonfinite"]), nf_r)
    assert _exact(out["totals"]["nonfinite"])[0] == 2
    assert np.array_equal(_exact(out["item"]["yes_ge"]), S - nf_i)
    assert np.array_equal(_exact(out["respondent"]["dev_ge"]), S - nf_r)
    assert _exact(out["totals"]["yes_ge"])[0] == S - 2
    # the means are over the draws that entered: still exactly T and n_obs
    assert np.array_equal(out["item"]["rep_yes_mean"], (y > 0).sum(axis=0).astype(float))
    assert np.array_equal(out["respondent"]["correct_mean"], np.full(n, float(m)))


# -------------------------------------------------------------------------------------------------- calibration ------
@pytest.mark.parametrize("n,m", [(100, 17), (1000, 64)])
def test_calibration_and_no_undecided_on_continuous_draws(n, m):
    """y drawn from the same p as the (constant) draws: per item E[R] = sum_i p_ij and Var[R] = sum_i p (1 - p) (a
    Poisson-binomial count), so the mean of S independent replicates lies within 6 sqrt(sum p (1 - p) / S) of sum p --
    derived, not tuned.  With continuous g no cell is within 1e-13 of its uniform: the restatement alone reports zero
    undecided cells and comparisons at these shapes."""
    S = 64
    rng = np.random.default_rng(n + m)
    g0 = rng.normal(0.0, 1.5, (n, m))
    p = 1.0 / (1.0 + np.exp(-g0))
    y = np.where(rng.random((n, m)) < p, 1.0, -1.0)
    y[rng.random((n, m)) < 0.03] = np.nan
    out = P.from_draws(y, np.broadcast_to(g0, (S, n, m)), seed=2**33 + 9, iters=range(1, S + 1))
    assert out["undecided"] == dict(cells=0, comparisons=0)
    assert out["comparisons"] == S * (n + m + 1)
    obs = ~np.isnan(y)
    for unit, axis in (("item", 0), ("respondent", 1)):
        mean = np.where(obs, p, 0.0).sum(axis=axis)
        sd = np.sqrt(np.where(obs, p * (1 - p), 0.0).sum(axis=axis) / S)
        err = np.abs(out[unit]["rep_yes_mean"] - mean)
        assert (err <= 6.0 * sd).all(), (unit, float((err / sd).max()))
        # ... and the replicate's variance is that of the Poisson-binomial count within 6 of ITS standard errors:
        # Var[s^2] = sigma^4 (2 / (S - 1) + kappa / S) with the excess kurtosis |kappa| <= 1 / sigma^2 of such a count
        v = np.where(obs, p * (1 - p), 0.0).sum(axis=axis)
        se = v * np.sqrt(2.0 / (S - 1) + 1.0 / (v * S))
        assert (np.abs(out[unit]["rep_yes_var"] - v) <= 6.0 * se).all()
    # y itself is one more replicate: the p-values are not piled at 0 or 1
    S_ = float(S)
    mid = (_exact(out["item"]["yes_ge"]) + _exact(out["item"]["yes_gt"])) / (2 * S_)
    assert 0.2 < mid.mean() < 0.8


def test_result_derives_the_p_values():
    p, arrays = P.struct(3, 2)
    for unit in ("item", "respondent"):
        for k, a in arrays[unit].items():
            a[:] = 0.0
        arrays[unit]["n_obs"][:] = 3
        arrays[unit]["draws"][:] = 8
        arrays[unit]["yes_ge"][:] = 6
        arrays[unit]["yes_gt"][:] = 2
        arrays[unit]["dev_ge"][:] = 4
    p.totals[_lib.PPC_FIELDS.index("draws")] = 8.0
    p.totals[_lib.PPC_FIELDS.index("n_obs")] = 6.0
    p.totals[_lib.PPC_FIELDS.index("yes_ge")] = 8.0
    arrays["item"]["nonfinite"][1] = 4
    arrays["respondent"]["n_obs"][0] = 0
    r = P.result(p, arrays)
    assert np.array_equal(r["item"]["ppp_yes"], [0.75, 1.5])
    assert np.array_equal(r["item"]["ppp_yes_mid"], [0.5, 1.0])
    assert np.isnan(r["respondent"]["ppp_yes"][0]) and r["respondent"]["ppp_dev"][1] == 0.5
    assert r["totals"]["ppp_yes"] == 1.0 and r["totals"]["draws"] == 8.0


# --------------------------------------------------------------------------------------------------------- ABI -------
def test_abi_version_symbols_and_struct(lib):
    assert lib.gpirt_version() >= 107
    for name in ("gpirt_sampler_ppc_enable", "gpirt_sampler_ppc_accumulate", "gpirt_sampler_ppc_get", "gpirt_sampler_ppc_totals",
                 "gpirt_sampler_ppc_state", "gpirt_ppc_combine", "gpirt_mcmc_run"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    nf = len(_lib.PPC_FIELDS)
    assert nf == 15 and C.sizeof(_lib.Ppc) == 8 * (3 * nf + 4)
    assert _lib.Ppc.reserved.offset == 8 * 3 * nf


def _mcmc_ppc_args(pp, run=True):
    dp = C.POINTER(C.c_double)
    y = np.ones((4, 2), order="F")
    th = np.zeros(4)
    p = np.zeros((2, 2), order="F")
    irf = np.zeros((1001, 2), order="F")
    o = _lib.fast_options()
    sm = _lib.Summary()
    r = _lib.Run()
    r.ppc = C.pointer(pp)
    keep = (y, th, p, irf, o, sm, r)
    a = lambda x: x.ctypes.data_as(dp)          # noqa: E731
    return keep, (a(y), 4, 2, a(th), 1, 1, 0, a(p), a(p), a(p), C.byref(o), 1, _lib.TICK_FN(0), None, None, None, None,
                  a(irf), C.byref(sm), None, C.byref(r) if run else None)


def test_mcmc_ppc_without_a_gpu_and_argument_errors(lib):
    import torch
    pp = _lib.Ppc()
    pp.reserved[2] = 1
    keep, args = _mcmc_ppc_args(pp)
    assert lib.gpirt_mcmc_run(*args) == _lib.E_ARG           # refused before any device is touched
    assert "bad argument" in _lib.last_error()
    keep, args = _mcmc_ppc_args(_lib.Ppc(), run=False)
    assert lib.gpirt_mcmc_run(*args) == _lib.E_ARG           # run is required
    assert "bad argument" in _lib.last_error()
    assert lib.gpirt_ppc_combine(None, 1, None, C.byref(pp)) == _lib.E_ARG
    if torch.cuda.is_available():
        return
    pp = _lib.Ppc()
    keep, args = _mcmc_ppc_args(pp)
    assert lib.gpirt_mcmc_run(*args) == _lib.E_NODEVICE
    assert "no CPU fallback" in _lib.last_error()
    from gpirt_amd import gpirtMCMC
    with pytest.raises(_lib.GpirtError):
        gpirtMCMC(np.array([[1, 0], [0, 1], [1, 1], [0, 0]]), 1, 0, vote_codes=dict(yea=[1], nay=[0], missing=[None]),
                  preset="fast", ppc=True)


def test_sharded_sampler_refuses_ppc():
    from _oracle_engine import OracleEngine
    from gpirt_amd.distributed import ShardedSampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(40, 6, seed=4)
    ss = ShardedSampler(OracleEngine, y, th0, dist=None)
    with pytest.raises(ValueError, match="posterior predictive"):
        ss.ppc_enable()
