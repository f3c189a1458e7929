"""gpirt_amd.score.from_draws -- the NumPy statement of "scoring new respondents" (include/gpirt_hip.h) -- on inputs whose
answer is known, and the C ABI of library version 109 on a machine without a device."""
import numpy as np

from gpirt_amd import score as SC
from gpirt_amd.synthetic import make_responses

from _score_bounds import EPS, compare, delta_of

N = 1001


def _fstar(S, m, seed=3, C=None):
    """smooth item response functions on the grid plus a little noise per draw: (S, 1001, m) or (C, S, 1001, m)"""
    rng = np.random.default_rng(seed)
    th = SC.grid()
    a, b = rng.uniform(0.3, 2.0, m) * rng.choice([-1.0, 1.0], m), rng.normal(0.0, 1.0, m)
    shape = (S,) if C is None else (C, S)
    return a * th[:, None] + b + 0.1 * rng.standard_normal(shape + (N, m))


def _y_new(n_new, m, seed=11):
    y, _ = make_responses(n_new, m, seed=seed, na_frac=0.05)
    y = np.array(y)
    y[-1, :] = np.nan                                    # one respondent who answered nothing
    return y


def test_zero_fstar_gives_the_prior_and_n_obs_log2():
    y = _y_new(9, 17)
    out = SC.from_draws(y, np.zeros((3, N, 17)))
    prior = np.exp(SC.logprior() - SC.logprior_lse())
    assert np.array_equal(out["draws"], np.full(9, 3)) and not out["nonfinite"].any()
    assert np.array_equal(out["n_obs"], (~np.isnan(y)).sum(axis=1)) and out["n_obs"][-1] == 0
    gap = np.abs(out["grid_post"] - prior[None, :]).max() / prior.max()
    gap_lpd = np.abs(out["lpd"] + out["n_obs"] * np.log(2.0)).max()
    print(f"MEASURED zero f*: grid_post gap {gap:.3e} of the prior's peak, lpd gap {gap_lpd:.3e}; integers bit-equal True")
    assert np.allclose(out["grid_post"], prior[None, :], rtol=4 * N * EPS, atol=0.0)
    assert gap_lpd <= 4 * 17 * EPS * 17 * np.log(2.0)
    assert np.allclose(out["loglik_mean"], out["lpd"], rtol=0, atol=4 * 17 * EPS * 17)
    assert abs(out["lpd"][-1]) <= 2 * N * EPS            # no answers: l = 0 to the rounding of the two logsumexps
    assert np.array_equal(out["theta_map"], np.full(9, SC.grid()[500]))
    assert np.allclose(out["theta_mean"], 0.0, atol=1e-12) and np.array_equal(out["theta_quantiles"][1], out["theta_map"])
    assert abs(out["lpd_total"] - out["lpd"].sum()) <= 1e-12 and out["se_lpd_total"] > 0


def test_mirrored_draws_with_sign_minus_one_give_the_same_scores():
    y, f = _y_new(7, 5), _fstar(4, 5)
    a = SC.from_draws(y, f)
    b = SC.from_draws(y, f[:, ::-1, :], signs=[-1])
    gap = max(float(np.abs(a[k] - b[k]).max()) for k in ("post_sum", "lpd_acc", "ll_sum"))
    print(f"MEASURED mirror: largest gap {gap:.3e}; integers bit-equal {np.array_equal(a['draws'], b['draws'])}")
    # the mirrored chain's weights are the same numbers at 1000 - k (the prior is symmetric bit for bit), summed in the
    # other direction over the grid: equal to the rounding of a 1001-term sum
    assert np.array_equal(a["draws"], b["draws"])
    assert np.allclose(a["post_sum"], b["post_sum"], rtol=4 * N * EPS, atol=1e-300)
    assert np.allclose(a["lpd"], b["lpd"], rtol=4 * N * EPS) and np.allclose(a["theta_mean"], b["theta_mean"], atol=1e-12)


def test_two_chains_pooled_equal_one_pass():
    y, f = _y_new(6, 9), _fstar(6, 9)
    one = SC.from_draws(y, f)
    two = SC.from_draws(y, np.stack([f[:3], f[3:]]))
    assert np.array_equal(one["draws"], two["draws"]) and np.array_equal(one["n_obs"], two["n_obs"])
    worst = 0.0
    for k in ("post_sum", "ll_sum", "lpd_acc", "grid_post", "lpd", "loglik_mean"):
        rel = np.abs(one[k] - two[k]) / np.maximum(np.abs(one[k]), 1e-300)
        worst = max(worst, float(rel.max()))
    print(f"MEASURED pooling: largest relative gap {worst / EPS:.2f} eps; integers bit-equal True")
    assert worst <= 4 * EPS


def test_nan_cell_skips_only_those_who_answered_the_item():
    y, f = _y_new(8, 6), _fstar(3, 6)
    y[0, 2] = np.nan
    y[1, 2] = 1.0
    clean = SC.from_draws(y, f)
    f2 = f.copy()
    f2[1, 400, 2] = np.nan
    out = SC.from_draws(y, f2)
    answered = ~np.isnan(y[:, 2])
    assert answered[1] and not answered[0] and not answered[-1]
    assert np.array_equal(out["nonfinite"], answered.astype(np.int64))
    assert np.array_equal(out["draws"], 3 - answered.astype(np.int64))
    for k in ("post_sum", "lpd_acc", "ll_sum"):          # those who did not answer: the NaN never enters their sums
        assert np.array_equal(out[k][~answered], clean[k][~answered])
    only = SC.from_draws(y, f[[0, 2]])                   # those who did: exactly the other two draws
    for k in ("post_sum", "lpd_acc", "ll_sum"):
        assert np.array_equal(out[k][answered], only[k][answered])
    print("MEASURED NaN cell: gap 0; integers bit-equal True")


def test_chosen_inputs_keep_the_quantile_comparison_meaningful():
    """The GPU test leaves a quantile cell out where the reference's cumulative sum is within the bound of q: on inputs of
    its kind that share stays far below 1 %."""
    y, f = _y_new(65, 33), _fstar(4, 33)
    want = SC.from_draws(y, f, return_products=True)
    share = compare(want, want, delta_of(want["products"][0], 33), "self")
    assert share <= 0.01


def test_refusals():
    import pytest
    with pytest.raises(ValueError, match="unanimous"):
        SC.from_draws(np.ones((2, 4)), np.zeros((1, N, 5)))
    with pytest.raises(ValueError, match=r"\+1, -1 or NaN"):
        SC.check_y_new(np.array([[1.0, 0.0]]))
    with pytest.raises(ValueError, match="outside"):
        SC.check_y_new(np.ones((0, 3)))
    with pytest.raises(ValueError, match="outside"):
        SC.check_y_new(np.ones((16385, 1)))


def test_abi_of_version_109():
    import ctypes as C
    from gpirt_amd import _lib
    lib = _lib.load()
    assert lib.gpirt_version() >= 109
    for name in ("gpirt_sampler_score_enable", "gpirt_sampler_score_accumulate", "gpirt_sampler_score_get",
                 "gpirt_sampler_score_state", "gpirt_score_combine", "gpirt_mcmc_run"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    r, arrays = SC.struct(3, (0.1, 0.9))
    assert r.nprobs == 2 and arrays["grid_post"].shape == (3, N) and arrays["theta_quantiles"].shape == (2, 3)
    assert lib.gpirt_score_combine(None, 1, None, None, C.byref(r)) == _lib.E_ARG
    from gpirt_amd.distributed import ShardedSampler
    assert "score_enable" in vars(ShardedSampler)
