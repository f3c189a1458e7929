"""The group-wise item fit (DIF) of the PPC without a device: the NumPy statement of the header (gpirt_amd.ppc.dif_*) on a
hand-worked example and on constructed edge cases, the argument checks, a planted case and the C ABI of version 115."""
import ctypes as C

import numpy as np
import pytest

from gpirt_amd import _lib
from gpirt_amd import ppc as P

CUT1 = (50,)                                             # B = 3: theta < -0.5, the centre, theta >= 0.5


def _snap(t):
    """onto the theta grid, bit for bit"""
    return -5.0 + np.rint((np.clip(t, -5.0, 5.0) + 5.0) * 100.0) * 0.01


def _hand():
    """8 respondents x 2 items, G = 2, B = 3, g = 0 everywhere (p = 1/2, p q = 1/4: E = N / 2, V = N / 4)"""
    groups = np.array([0, 0, 0, 0, 1, 1, 1, 1])
    theta = np.array([-1.0, -1.0, 0.0, 1.0, -1.0, 0.0, 1.0, 1.0])                # bins 0 0 1 2 | 0 1 2 2
    y = np.array([[1, -1, 1, 1, 1, -1, 1, -1], [1, 1, -1, np.nan, 1, -1, -1, 1]], dtype=float).T
    rep = np.array([[1, 1, 0, 1, 0, 1, 1, 0], [0, 1, 1, 1, 1, 0, 0, 1]]).T
    return y, theta, rep, groups


def test_hand_worked_example():
    y, theta, rep, groups = _hand()
    d = P.dif_from_rep(y, theta[None], np.zeros((1, 8, 2)), rep[None], groups, CUT1)
    last = d["last"]
    assert list(last["cell"]) == [0, 0, 1, 2, 3, 4, 5, 5]
    # tables [group, bin, item]
    assert last["tN"].tolist() == [[[2, 2], [1, 1], [1, 0]], [[1, 1], [1, 1], [2, 2]]]
    assert last["tT"].tolist() == [[[1, 2], [1, 0], [1, 0]], [[1, 1], [0, 0], [1, 1]]]
    assert last["tR"].tolist() == [[[2, 1], [0, 1], [1, 0]], [[0, 1], [1, 0], [1, 1]]]
    assert np.array_equal(last["tE"], last["tN"].astype(np.uint64) * np.uint64(2**43))
    assert np.array_equal(last["tV"], last["tN"].astype(np.uint64) * np.uint64(2**42))
    st = last["stats"]                                   # num(T), den(T), num(R), den(R), STD(T), STD(R), X2(T), X2(R)
    third = 1.0 / 3.0
    # item 0: num(T) = 0 + 1/2 + 1/3, den(T) = 1/3 + 0 + 0; num(R) = 2/3 + 0 + 1/3, den(R) = 0 + 1/2 + 0
    assert st[0, 1, 0] == (0.0 + 0.5) + third and st[1, 1, 0] == third
    assert st[2, 1, 0] == (2.0 / 3.0 + 0.0) + third == 1.0 and st[3, 1, 0] == 0.5
    assert st[0, 1, 0] / st[1, 1, 0] == pytest.approx(2.5) and st[2, 1, 0] / st[3, 1, 0] == 2.0
    assert st[4, 1, 0] == -0.375 and st[5, 1, 0] == -0.25
    assert st[6, :, 0].tolist() == [2.0, 2.0] and st[7, :, 0].tolist() == [4.0, 2.0]
    # item 1: group 0 is absent from bin 2, and both MH products of the data vanish in the two common bins
    assert st[0, 1, 1] == 0.0 and st[1, 1, 1] == 0.0 and st[4, 1, 1] == 0.0 and st[5, 1, 1] == -0.25
    assert np.isnan(st[:6, 0]).all()
    assert d["mh_undefined"][1].tolist() == [0.0, 1.0] and np.isnan(d["mh_undefined"][0]).all()
    assert d["mh_ge"][1].tolist() == [0, 0] and d["mh_gt"][1].tolist() == [0, 0]       # alpha(R) = 2 < alpha(T) = 2.5
    assert d["mh_log_or_obs_mean"][1, 0] == np.log(st[0, 1, 0] / st[1, 1, 0]) and np.isnan(d["mh_log_or_obs_mean"][1, 1])
    assert d["mh_delta_obs_mean"][1, 0] == -2.35 * d["mh_log_or_obs_mean"][1, 0]
    assert d["ppp_mh_mid"][1, 0] == 0.0 and np.isnan(d["ppp_mh"][1, 1]) and np.isnan(d["ppp_mh"][0]).all()
    assert d["std_obs_mean"][1].tolist() == [-0.375, 0.0] and d["std_rep_mean"][1].tolist() == [-0.25, -0.25]
    # the groups' margins: item 0 R = T = 3 and 2; item 1 group 0: T = 2, R = 2; group 1: T = 2, R = 2
    assert d["yes_ge"].tolist() == [[1, 1], [1, 1]] and d["yes_gt"].tolist() == [[0, 0], [0, 0]]
    assert d["chi_ge"][:, 0].tolist() == [1, 1] and d["chi_gt"][:, 0].tolist() == [1, 0]
    assert d["occupancy"].tolist() == [[2.0, 1.0, 1.0], [1.0, 1.0, 2.0]] and list(d["group_size"]) == [4, 4]
    assert d["obs_rate"][0, :, 0].tolist() == [0.5, 1.0, 1.0] and np.isnan(d["obs_rate"][0, 2, 1])
    assert d["exp_rate"][1, 2, 0] == 0.5 and (d["dif_draws"], d["dif_skipped"]) == (1, 0)
    assert list(d["flagged"]["items"][:2]) == [0, -1] and list(d["flagged"]["groups"][:2]) == [1, -1]


def test_fixed_point_rounding_rule():
    p = np.array([0.0, 1.0, 0.5, 2.0**-45, 3 * 2.0**-46, 2.0**-46, 1.0 - 2.0**-53, 0.1])
    want = [0, 2**44, 2**43, 0, 1, 0, 2**44, round(0.1 * 2**44)]     # ties to even: 0.5 -> 0, 0.75 -> 1; 0.25 -> 0
    assert P.dif_fix(p).tolist() == want and P.dif_fix(p).dtype == np.uint64
    # the sums are exact integers: any order of summation gives the same table
    rng = np.random.default_rng(0)
    q = rng.random(65534)
    f = P.dif_fix(q)
    assert f.sum(dtype=np.uint64) == f[::-1].sum(dtype=np.uint64) == np.uint64(sum(int(x) for x in f)) < 2**60


def test_minus_one_rows_one_member_group_and_integer_tie():
    rng = np.random.default_rng(1)
    n, m = 40, 3
    y = np.where(rng.random((n, m)) < 0.5, 1.0, -1.0)
    theta = _snap(rng.normal(size=n))
    g = rng.normal(size=(1, n, m))
    groups = np.where(np.arange(n) < 20, 0, 1)
    groups[5] = 2                                        # a group with one member
    rep = rng.random((1, n, m)) < 0.5
    rep[0, :, 2] = y[:, 2] > 0                           # item 2: R = T in every cell -- the integer tie
    a = P.dif_from_rep(y, theta[None], g, rep, groups, CUT1)
    assert list(a["group_size"]) == [19, 20, 1] and a["sum_n"][2].sum() == m
    assert a["chi_ge"][:, 2].tolist() == [1, 1, 1] and a["chi_gt"][:, 2].tolist() == [0, 0, 0]
    assert a["yes_ge"][:, 2].tolist() == [1, 1, 1] and a["yes_gt"][:, 2].tolist() == [0, 0, 0]
    assert a["mh_ge"][1, 2] == 1 and a["mh_gt"][1, 2] == 0          # alpha(R) = alpha(T)
    # rows coded -1 are ignored entirely: whatever they hold, NaN g included
    groups2 = groups.copy()
    groups2[[7, 30]] = -1
    b = P.dif_from_rep(y, theta[None], g, rep, groups2, CUT1)
    y3, g3, rep3 = y.copy(), g.copy(), rep.copy()
    y3[[7, 30]] *= -1
    g3[0, [7, 30]] = np.nan
    rep3[0, [7, 30]] ^= True
    c = P.dif_from_rep(y3, theta[None], g3, rep3, groups2, CUT1)
    keep = np.ones(n, dtype=bool)
    keep[[7, 30]] = False
    e = P.dif_from_rep(y[keep], theta[None, keep], g[:, keep], rep[:, keep], groups[keep], CUT1)
    for k, _dt, _kind in _lib.DIF_RAW:
        assert np.array_equal(b[k], c[k]) and np.array_equal(b[k], e[k]), k
    assert c["dif_draws"] == 1 and b["last"]["cell"][7] == 255


def test_skipped_draws():
    y, theta, rep, groups = _hand()
    th = np.stack([theta, np.where(np.arange(8) == 2, 0.005, theta), theta, theta])
    g = np.zeros((4, 8, 2))
    g[2, 6, 0] = np.inf                                  # an observed cell of a grouped respondent
    g[3, 3, 1] = np.nan                                  # an unobserved cell: counts
    d = P.dif_from_rep(y, th, g, np.stack([rep] * 4), groups, CUT1)
    one = P.dif_from_rep(y, theta[None], np.zeros((1, 8, 2)), rep[None], groups, CUT1)
    assert (d["dif_draws"], d["dif_skipped"]) == (2, 2)
    assert np.array_equal(d["sum_n"], 2 * one["sum_n"]) and np.array_equal(d["yes_ge"], 2 * one["yes_ge"])


def _random_case(seed, S=6, n=60, m=4, G=3):
    rng = np.random.default_rng(seed)
    y = np.where(rng.random((n, m)) < 0.5, 1.0, -1.0)
    y[rng.random((n, m)) < 0.05] = np.nan
    theta = _snap(rng.normal(size=(S, n)))
    g = rng.normal(size=(S, n, m))
    groups = rng.integers(-1, G, size=n)
    groups[:G] = np.arange(G)
    return y, theta, g, rng.random((S, n, m)) < 0.5, groups


def test_reflection_and_pooling():
    y, theta, g, rep, groups = _random_case(2)
    cuts = (30, 90)
    plain = P.dif_from_rep(y, theta, g, rep, groups, cuts)
    flipped = P.dif_from_rep(y, theta, g, rep, groups, cuts, signs=-1)
    for k in ("sum_n", "sum_t", "sum_r", "sum_e", "occ_sum", "obs_rate"):
        assert np.array_equal(flipped[k], plain[k][:, ::-1], equal_nan=True), k
    assert plain["sum_n"].any() and not np.array_equal(plain["sum_n"], plain["sum_n"][:, ::-1])
    for k, _dt, kind in _lib.DIF_RAW:
        if kind == "g":                                  # every counter and per-draw sum as the chain decided it
            assert np.array_equal(flipped[k], plain[k]), k
    # two states pooled = one state over both draw sets, for the integers
    a = P.dif_from_rep(y, theta[:2], g[:2], rep[:2], groups, cuts)
    b = P.dif_from_rep(y, theta[2:], g[2:], rep[2:], groups, cuts)
    for k, dt, _kind in _lib.DIF_RAW:
        if dt != "f8":
            assert np.array_equal(a[k] + b[k], plain[k]), k
    assert a["dif_draws"] + b["dif_draws"] == plain["dif_draws"] == 6


def test_flagged_order_and_ties():
    nan = np.nan
    mid = np.array([[nan, nan, nan, nan], [0.5, 0.9, 0.1, nan], [0.1, 1.0, 0.5, 0.9]])
    f = P.dif_flagged(mid, top=6)
    # |mid - 0.5|: (2, 1) 0.5 first; then 0.4 four times, in (group, item) order; then 0.0; NaN never
    assert list(zip(f["groups"], f["items"])) == [(2, 1), (1, 1), (1, 2), (2, 0), (2, 3), (1, 0)]
    assert f["ppp_mh_mid"].tolist() == [1.0, 0.9, 0.1, 0.1, 0.9, 0.5]
    g = P.dif_flagged(mid, top=9)
    assert list(g["items"][7:]) == [-1, -1] and np.isnan(g["ppp_mh_mid"][7:]).all() and g["groups"][6] == 2
    with pytest.raises(ValueError):
        P.dif_flagged(mid, top=65)


def test_check_groups_refusals():
    codes, G = P.check_groups([0, 1, -1, 2, 1], 5)
    assert codes.dtype == np.int32 and G == 3 and P.check_groups(np.array([0.0, 1.0]), 2)[1] == 2
    for bad, n, word in (([0, 1, 0], 4, "one code per respondent"), ([0, 1, 4], 3, "outside -1..3"), ([0, -2, 1], 3, "outside"),
                         ([0, 2, 2], 3, "group 1 has no member"), ([1, 1, 2], 3, "group 0 has no member"),
                         ([0, 0, -1], 3, "at least one focal"), ([-1, -1], 2, "at least one focal"), ([0.5, 1, 0], 3, "integers"),
                         ([True, False], 2, "integers"), ([[0, 1]], 2, "one code per respondent")):
        with pytest.raises(ValueError, match=word):
            P.check_groups(bad, n)
    with pytest.raises(ValueError, match="beyond 65534"):
        P.check_groups(np.zeros(65535, dtype=int), 65535)
    with pytest.raises(ValueError):
        P.check_dif_top(0)


def test_planted_dif_is_found_where_the_other_checks_are_blind():
    """n = 600, m = 8; item 3 is one logit easier for the focal half at equal theta, half a logit each way around the curve
    the draws hold -- so its pooled yes count, its theta-binned chi-square and its pair tables replicate."""
    rng = np.random.default_rng(20)
    n, m, S, seed, item = 600, 8, 40, 5, 3
    theta0 = np.clip(np.round(rng.normal(size=n), 2), -4.9, 4.9)
    groups = (np.arange(n) % 2).astype(np.int64)
    b = np.linspace(-0.8, 0.8, m)
    eta = 1.2 * theta0[:, None] + b[None, :]
    true = eta.copy()
    true[:, item] += np.where(groups == 1, 0.5, -0.5)
    y = np.where(rng.random((n, m)) < 1.0 / (1.0 + np.exp(-true)), 1.0, -1.0)
    theta = _snap(theta0[None, :] + 0.01 * rng.integers(-5, 6, size=(S, n)))
    g = 1.2 * theta[:, :, None] + b[None, None, :]
    iters = list(range(1, S + 1))
    d, gap = P.dif_from_draws(y, theta, g, seed, iters, groups)
    assert gap > 0 and d["dif_draws"] == S
    assert (d["flagged"]["items"][0], d["flagged"]["groups"][0]) == (item, 1)
    assert abs(d["ppp_mh_mid"][1, item] - 0.5) >= 0.45 and d["mh_log_or_obs_mean"][1, item] < -0.5      # alpha > 1 favours group 0
    assert d["std_obs_mean"][1, item] > 0.1 and abs(d["std_rep_mean"][1, item]) < 0.05
    # what the other blocks see of item 3: nothing remarkable
    margins = P.from_draws(y, g, seed, iters)["item"]
    ppp_yes = (margins["yes_ge"][0][item] + margins["yes_gt"][0][item]) / (2.0 * S)
    assert 0.05 < ppp_yes < 0.95
    bins, _ = P.bins_from_draws(y, theta, g, seed, iters)
    assert 0.05 < bins["ppp_chi2_mid"][item] < 0.95
    pairs, _ = P.pairs_from_draws(y, g, seed, iters)
    others = [j for j in range(m) if j != item]
    # seven null pairs: |U - 1/2| has mean 1/4 and sd 0.144, their mean sd 0.055 -- 0.4 lies 2.7 sd above
    assert np.abs(pairs["ppp_or_mid"][item, others] - 0.5).mean() < 0.4


def test_c_abi_of_version_115():
    lib = _lib.load()
    assert lib.gpirt_version() >= 115
    p = _lib.PpcDif()
    assert C.sizeof(p) == 4 * 3 + 4 * 16 + 4 + 8 + 8 * (3 + 1 + 6 + 9) + 8 * 19 + 8 * 3 + 8 * 5 + 8 * 4 + 8 * 4
    assert len(_lib.DIF_RAW) == 19 and len(_lib.DIF_FOCAL_FIELDS) == 9
    for name in ("gpirt_sampler_ppc_dif_enable", "gpirt_sampler_ppc_dif_get", "gpirt_sampler_ppc_dif_state",
                 "gpirt_ppc_dif_combine", "gpirt_mcmc_run"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    # argument errors come back before any device is touched
    assert lib.gpirt_ppc_dif_combine(None, 1, None, None, C.byref(p)) == _lib.E_ARG
    assert lib.gpirt_sampler_ppc_dif_enable(None, 2, None, 1, None, 1) == _lib.E_ARG
    assert lib.gpirt_sampler_ppc_dif_get(None, b"counts", None, 0) == _lib.E_ARG
    _, arr = P.dif_struct(5, 3, (14, 43), top=4)
    assert arr["obs_rate"].shape == (3, 5, 5) and arr["mh_ge"].dtype == np.uint32 and arr["flagged_items"].shape == (4,)
