"""gpirt_amd.sumscore on the host: from_draws (the NumPy statement of include/gpirt_hip.h, "Sum-score posteriors") and finish on
hand-built f* with known answers, the tie to the scorer by enumerating answer patterns, the reflection of accumulators and the
version-114 C ABI on a machine without a device."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import _score_bounds as SB
import _sumscore_bounds as B
from gpirt_amd import _lib
from gpirt_amd import score as SC
from gpirt_amd import sumscore as SS

N = 1001
TH = SS.THETA
EPS = B.EPS


def twopl(a, b):
    return (np.asarray(a)[None, :] * (TH[:, None] - np.asarray(b)[None, :]))[None]


def test_flat_items_give_the_binomial_bit_for_bit():
    r = SS.from_draws(np.zeros((2, N, 50)))
    want = np.array([math.comb(50, s) for s in range(51)], dtype=np.float64) * 2.0 ** -50
    assert np.array_equal(r["last"], np.tile(want, (N, 1)))             # every product and sum is exact
    assert np.array_equal(r["tcc_sum"], np.full(N, 50.0)) and np.array_equal(r["var_sum"], np.full(N, 25.0))
    assert r["draws"] == 2 and r["M"] == 50 and r["items"].tolist() == list(range(50))
    assert abs(r["score_dist"] - want).max() <= 1002 * EPS * want.max()
    assert abs(r["reliability_mean"]) < 1e-12                           # flat items: the score says nothing about theta


def test_infinite_columns_put_the_mass_on_one_score():
    for a, M in ((0, 5), (3, 5), (5, 5), (7, 64)):
        f = np.full((1, N, M), -np.inf)
        f[:, :, :a] = np.inf
        r = SS.from_draws(f)
        want = np.zeros(M + 1); want[a] = 1.0
        assert np.array_equal(r["last"], np.tile(want, (N, 1))), (a, M)
        assert np.array_equal(r["tcc_sum"], np.full(N, float(a))) and not r["var_sum"].any()
        assert r["rel_terms"].shape == (1, 3)
        assert np.isnan(r["theta_eap"][[s for s in range(M + 1) if s != a]]).all() and abs(r["theta_eap"][a]) < 1e-12
    f = np.full((1, N, 6), -np.inf)
    f[:, :, :2] = np.inf
    f[:, :, 4] = 0.0                                                    # one more column at 0: two cells of 1/2
    last = SS.from_draws(f)["last"]
    want = np.zeros(7); want[2] = want[3] = 0.5
    assert np.array_equal(last, np.tile(want, (N, 1)))
    big = SS.from_draws(np.where(np.arange(4)[None, None, :] % 2 == 0, 800.0, -800.0) * np.ones((1, N, 4)))
    assert np.isfinite(big["last"]).all() and abs(big["last"][:, 2] - 1.0).max() < 1e-300


def test_enumeration_ties_the_table_to_the_scorer():
    """M = 8, one draw: over the 256 answer patterns scored by gpirt_amd.score.from_draws, the sum of exp(lpd) over the
    patterns with sum s is pi[s] and the sum of exp(lpd) grid_post over them is joint_sum[:, s], within the two modules' bounds."""
    rng = np.random.default_rng(5)
    M = 8
    f = twopl(rng.uniform(0.4, 2.5, M) * rng.choice([-1.0, 1.0], M), rng.normal(size=M)) + 0.3 * rng.normal(size=(1, N, M))
    pats = np.array(list(itertools.product([-1.0, 1.0], repeat=M)))
    sc = SC.from_draws(pats, f, return_products=True)
    ss = SS.from_draws(f)
    delta = SB.delta_of(sc["products"][0], M)
    rho = 2.0 * delta + 2.0 * N * EPS
    e_l = delta + 2.0 * N * EPS * (1.0 + np.abs(sc["lpd"]).max())
    bd = B.bounds(ss)
    sums = (pats == 1.0).sum(axis=1)
    L = np.exp(sc["lpd"])
    share = 0.0
    for s in range(M + 1):
        idx = np.flatnonzero(sums == s)
        pi = L[idx].sum()
        joint = (L[idx, None] * sc["grid_post"][idx]).sum(axis=0)
        # the scorer's prior is exp(logprior - lse) in fp64: within 1001 eps of w, relative
        tol_pi = (e_l + (len(idx) + N + 2) * EPS) * 1.01 * pi + bd["pi_sum"][s]
        tol_j = (e_l + rho + (len(idx) + N + 2) * EPS) * 1.01 * joint + bd["joint_sum"][:, s]
        share = max(share, abs(pi - ss["pi_sum"][s]) / tol_pi, (np.abs(joint - ss["joint_sum"][:, s]) / tol_j).max())
    print(f"MEASURED enumeration identity: share of the bound used {share:.3f}")
    assert share <= 1.0


def test_identities_of_the_statement():
    rng = np.random.default_rng(11)
    M = 40
    a, b = rng.uniform(0.5, 2.0, M), rng.normal(size=M)
    r = SS.from_draws(twopl(a, b))
    A, T, V = r["last"], r["tcc_sum"], r["var_sum"]
    s = np.arange(M + 1, dtype=np.float64)
    rA = B.rel_A(M) + (M + 2) * EPS
    assert np.abs(A.sum(axis=1) - 1.0).max() <= rA
    assert (np.abs(A @ s - T) <= (rA + B.bounds(r)["tcc_sum"] / np.maximum(T, 1e-300)) * (A @ s) + 1e-300).all()
    second = A @ (s * s)                                                # sum s^2 A - T^2 = V cancels: carry absolute errors
    assert (np.abs(second - T * T - V) <= 4 * rA * second + B.bounds(r)["var_sum"]).all()
    p = 1.0 / (1.0 + np.exp(-(a[None, :] * (TH[:, None] - b[None, :]))))
    assert np.abs(T - p.sum(axis=1)).max() <= 2 * M * EPS * M            # the closed-form TCC of a 2PL item set
    assert np.all(np.diff(r["tcc_mean"]) > 0) and np.all(np.diff(r["theta_eap"]) > 0)
    flat = SS.from_draws(np.full((1, N, M), 0.7))
    steep = SS.from_draws(twopl(np.full(M, 25.0), rng.normal(size=M)))
    assert abs(flat["reliability_mean"]) < 1e-12 and r["reliability_mean"] > 0.8 and steep["reliability_mean"] > 0.98
    assert steep["reliability_mean"] > r["reliability_mean"]


def test_nan_inside_the_form_skips_the_draw_and_outside_is_ignored():
    rng = np.random.default_rng(3)
    f = rng.normal(size=(3, N, 6))
    items = [1, 2, 4]
    clean = SS.from_draws(f[[0, 2]], items=items)
    bad = f.copy()
    bad[1, N - 1, 4] = np.nan
    r = SS.from_draws(bad, items=items)
    assert (r["draws"], r["skipped"]) == (2, 1)
    for k in B.SUM_KEYS + ("rel",):
        assert np.array_equal(r[k], clean[k]), k
    out = f.copy()
    out[1, 0, 0] = out[1, 5, 5] = np.nan                                # columns 0 and 5 are outside the form
    r = SS.from_draws(out, items=items)
    full = SS.from_draws(f, items=items)
    assert (r["draws"], r["skipped"]) == (3, 0) and all(np.array_equal(r[k], full[k]) for k in B.SUM_KEYS)
    assert r["items"].tolist() == items and r["mask"].tolist() == [0, 1, 1, 0, 1, 0]
    assert np.array_equal(SS.from_draws(f, items=np.array([False, True, True, False, True, False]))["joint_sum"], full["joint_sum"])


def test_reflection_is_the_grid_reversed():
    rng = np.random.default_rng(8)
    f = twopl(rng.uniform(0.5, 2.0, 7), rng.normal(size=7)) + 0.2 * rng.normal(size=(3, N, 7))
    r = SS.from_draws([f, f[:2]], signs=[1, -1])
    w = SS.from_draws([f, f[:2, ::-1]])
    for k in ("tcc_sum", "tcc_sumsq", "var_sum", "last"):
        assert np.array_equal(r[k], w[k]), k                            # no weight in them: exact
    bd = B.bounds(w)
    # theta_k = -5 + 0.01 k is not the negative of theta_(1000 - k) to the last bit, so neither are the weights: a reflected
    # chain's joint carries w_(1000 - k) where the reversed draws carry w_k
    gw = SS.grid_weights()
    asym = float((np.abs(gw - gw[::-1]) / gw).max())
    assert asym < 64 * EPS
    assert (np.abs(r["joint_sum"] - w["joint_sum"]) <= bd["joint_sum"] + asym * w["joint_sum"]).all()
    for k in ("pi_sum", "pi_sumsq", "rel"):                             # kept as they are: the sum over k ran the other way
        assert (np.abs(r[k] - w[k]) <= bd[k]).all(), k
    with pytest.raises(ValueError, match="signs"):
        SS.from_draws([f], signs=[2])


def test_conversion_table_ties_zero_mass_and_observed_scores():
    w = SS.grid_weights()
    joint = np.zeros((N, 4))
    joint[100, 0] = joint[300, 0] = 0.25                                # a tie: the lowest k; quantiles: the first to reach q
    joint[:, 1] = w
    joint[500, 3] = 1.0
    raw = dict(joint_sum=joint, pi_sum=np.array([0.5, 1.0, 0.0, 1.0]), pi_sumsq=np.zeros(4), tcc_sum=np.zeros(N), tcc_sumsq=np.zeros(N),
               var_sum=np.zeros(N), rel=np.zeros(2), mask=np.array([1, 0, 1, 1], dtype=np.uint8), w=w, last=joint, last_pi=np.zeros(4))
    r = SS.finish(raw, (0.0, 0.5, 0.75, 1.0), draws=1)
    assert r["theta_map"][0] == TH[100] and r["theta_quantiles"][:, 0].tolist() == [TH[0], TH[100], TH[300], TH[300]]
    assert np.isnan(r["theta_map"][2]) and np.isnan(r["theta_eap"][2]) and np.isnan(r["theta_quantiles"][:, 2]).all()
    assert np.isnan(r["post"][2]).all() and r["theta_eap"][3] == TH[500] and r["theta_sd"][3] == 0.0
    assert abs(r["theta_eap"][1]) < 1e-12 and r["theta_quantiles"][1, 1] == TH[500] and r["items"].tolist() == [0, 2, 3]
    assert np.allclose(r["score_given_theta"][:, 1], 1.0) and r["score_cdf"].tolist() == [0.5, 1.5, 1.5, 2.5]
    y = np.array([[1, 1, 1, 1], [1, np.nan, -1, 1], [np.nan, 1, 1, 1], [-1, 1, -1, -1], [1, -1, 1, 1]], dtype=np.float64)
    r = SS.finish(raw, draws=1, y=y)                                    # row 2 misses an item of the form, row 1 only one outside it
    assert r["n_complete"] == 4 and r["obs_hist"].tolist() == [1, 0, 1, 2] and r["exp_count"].tolist() == [2.0, 4.0, 0.0, 4.0]


def test_arguments_are_checked():
    f = np.zeros((1, N, 3))
    for bad, word in (([], "empty"), ([3], "outside"), ([-1], "outside"), (np.zeros(3, dtype=bool), "empty"), ([0.5], "items")):
        with pytest.raises(ValueError, match=word):
            SS.from_draws(f, items=bad)
    with pytest.raises(ValueError, match="at most 4096"):
        SS.form_mask(None, 4097)
    with pytest.raises(ValueError, match="probs"):
        SS.from_draws(f, probs=(1.5,))
    with pytest.raises(ValueError, match="unknown keys"):
        SS.parse(dict(item=[0]), 3)
    with pytest.raises(ValueError, match="sumscore must be"):
        SS.parse(3, 3)
    assert SS.parse(True, 3)["mask"].tolist() == [1, 1, 1] and SS.parse(dict(items=[2, 0]), 3)["mask"].tolist() == [1, 0, 1]
    assert SS.form_mask(None, 4096).sum() == 4096
    # the dtype and the length say whether items is a mask or a list of indices, never the values
    assert SS.form_mask([0, 1], 2).tolist() == [1, 1] and SS.form_mask(np.array([0, 1], dtype=np.uint8), 2).tolist() == [0, 1]
    assert SS.form_mask([1, 0, 2], 3).tolist() == [1, 1, 1] and SS.form_mask(np.array([1, 0, 1], dtype=np.uint8), 3).tolist() == [1, 0, 1]
    assert SS.form_mask(np.array([True, False, True]), 3).tolist() == [1, 0, 1] and SS.form_mask(np.array([0, 2]), 3).tolist() == [1, 0, 1]
    for bad, word in (([0, 0, 1], "more than once"), (np.array([1, 1], dtype=np.int64), "more than once"),
                      (np.array([1, 0], dtype=np.uint8), "items must be"), (np.array([True, False]), "items must be")):
        with pytest.raises(ValueError, match=word):
            SS.form_mask(bad, 3)


def test_c_abi_of_version_114():
    lib = _lib.load()
    assert lib.gpirt_version() >= 114
    p = _lib.Sumscore()
    assert C.sizeof(p) == 8 + 8 * 11 + 8 * 2 + 8 * 4 + 8 * 4 and len(_lib.SUMSCORE_RAW) == 11
    for name in ("gpirt_sampler_sumscore_enable", "gpirt_sampler_sumscore_accumulate", "gpirt_sampler_sumscore_get",
                 "gpirt_sampler_sumscore_state", "gpirt_sumscore_state_bytes", "gpirt_sumscore_grid_weights",
                 "gpirt_sumscore_combine", "gpirt_mcmc_run"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    # argument errors come back before any device is touched
    assert lib.gpirt_sumscore_combine(None, 1, None, None, C.byref(p)) == _lib.E_ARG
    assert lib.gpirt_sampler_sumscore_enable(None, None, 1) == _lib.E_ARG
    assert lib.gpirt_sampler_sumscore_get(None, b"rel", None, 0) == _lib.E_ARG
    nb = C.c_int64()
    assert lib.gpirt_sumscore_state_bytes(1024, 1024, C.byref(nb)) == 0
    m = M = 1024
    pad = lambda nbytes: (nbytes + 15) // 16 * 16                        # noqa: E731  (every array starts on a 16-byte boundary)
    want = 16 * 8 + 2 * pad(8 * 1001 * (M + 1)) + 3 * pad(8 * (M + 1)) + 4 * pad(8 * 1001) + 16 + pad(m)
    assert nb.value == want and 16e6 < nb.value < 17e6
    for m, M in ((0, 0), (8, 9), (8, 0), (5000, 4097)):
        assert lib.gpirt_sumscore_state_bytes(m, M, C.byref(nb)) == _lib.E_ARG
    w = np.empty(N)
    assert lib.gpirt_sumscore_grid_weights(w.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert np.array_equal(w, SS.grid_weights())                        # the state's weights are from_draws' weights bit for bit
