"""The theta-binned item fit of the PPC without a device: the bin rule on every grid index, check_cuts, gpirt_amd.ppc.bins_from_rep
(the NumPy statement of the header, "theta-binned item fit") against a hand-worked example, the reflection, the integer-tie
rule, skipped draws, the ordering of `worst`, and the C ABI of library version 112."""
import ctypes as C
import math

import numpy as np
import pytest

from gpirt_amd import _lib
from gpirt_amd import ppc as P

INT_KEYS = ("sum_n", "sum_t", "sum_r", "cell_ge", "cell_gt", "cell_empty", "occ_sum")
CUT_SETS = {1: (50,), 4: P.DEFAULT_CUTS, 15: tuple(range(10, 460, 30))}


def _grid(k):
    return -5.0 + np.asarray(k, dtype=np.float64) * 0.01


@pytest.mark.parametrize("h", [1, 4, 15])
def test_bin_rule_on_every_grid_index(h):
    cuts = CUT_SETS[h]
    assert len(cuts) == h
    B = 2 * h + 1
    k = np.arange(1001)
    b = P.bin_of_index(k, cuts)
    want = []
    for kk in range(1001):                               # the header, word for word
        a = abs(kk - 500)
        l = sum(1 for d in cuts if a >= d)
        want.append(h + l if kk >= 500 else h - l)
    assert np.array_equal(b, want)
    assert b.min() == 0 and b.max() == B - 1 and (np.diff(b) >= 0).all()
    assert np.array_equal(P.bin_of_index(1000 - k, cuts), B - 1 - b)
    assert (b[np.abs(k - 500) < cuts[0]] == h).all() and b[500 + cuts[0]] == h + 1 and b[500 - cuts[0]] == h - 1
    lo, hi = P.bin_edges(cuts)
    th = _grid(k)
    inside = (th >= lo[b] - 1e-12) & (th <= hi[b] + 1e-12)
    assert inside.all() and np.array_equal(lo, -hi[::-1]) and lo[0] == -5.0 and hi[-1] == 5.0


def test_default_cuts_are_equal_probability_bins():
    # the N(0, 1) quantiles at 5/9 .. 8/9, snapped to hundredths
    from statistics import NormalDist
    assert P.DEFAULT_CUTS == tuple(round(100 * NormalDist().inv_cdf(q / 9)) for q in (5, 6, 7, 8))


def test_check_cuts():
    assert P.check_cuts([14, 43]) == (14, 43)
    assert P.check_cuts(np.array([1, 499])) == (1, 499)
    assert P.check_cuts([0.14, 0.43, 1.22]) == (14, 43, 122)
    assert P.check_cuts([0.14 + 5e-12]) == (14,)
    assert P.check_cuts(range(1, 16)) == tuple(range(1, 16))
    for bad in ([], list(range(1, 17)), [0], [500], [43, 14], [14, 14], [0.145], [float("nan")], ["a"], [True], 7, [0.0], [5.0]):
        with pytest.raises(ValueError):
            P.check_cuts(bad)
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError):
            P.check_bins_top(bad)


def _hand():
    """6 respondents, 2 items, one cut at 0.50 (B = 3): theta = -1, -0.5, 0, 0.49, 0.5, 2 -> bins 0, 0, 1, 1, 2, 2"""
    theta = np.array([[-1.0, -0.5, 0.0, 0.49, 0.5, 2.0]])
    theta = _grid(np.rint((theta + 5.0) * 100.0))
    y = np.array([[1, -1], [-1, np.nan], [1, 1], [1, -1], [-1, 1], [1, np.nan]], dtype=float)
    g = np.array([[[0.0, 1.0], [0.0, 5.0], [math.log(3.0), 0.0], [-math.log(3.0), 0.0], [0.0, 0.0], [0.0, 7.0]]])
    rep = np.array([[[1, 0], [1, 1], [0, 1], [0, 1], [1, 1], [0, 1]]])
    return y, theta, g, rep


def test_bins_from_rep_hand_worked():
    y, theta, g, rep = _hand()
    r = P.bins_from_rep(y, theta, g, rep, cuts=(50,), top=2)
    assert r["B"] == 3 and r["bin_draws"] == 1 and r["bin_skipped"] == 0
    assert np.array_equal(r["last"]["bin"], [0, 0, 1, 1, 2, 2])
    assert np.array_equal(r["occ_sum"], [2, 2, 2])
    assert np.array_equal(r["sum_n"], [[2, 1], [2, 2], [2, 1]])
    assert np.array_equal(r["sum_t"], [[1, 0], [2, 1], [1, 1]])
    assert np.array_equal(r["sum_r"], [[2, 0], [0, 2], [1, 1]])            # (the replicate of a missing cell is masked out)
    assert np.array_equal(r["cell_ge"], [[1, 1], [0, 1], [1, 1]]) and np.array_equal(r["cell_gt"], [[1, 0], [0, 1], [0, 0]])
    assert not r["cell_empty"].any()
    p1 = 1.0 / (1.0 + math.exp(-1.0))
    E = np.array([[1.0, p1], [1.0, 1.0], [1.0, 0.5]])                     # item 0: 0.5 + 0.5, 0.75 + 0.25, 0.5 + 0.5
    V = np.array([[0.5, p1 * (1 - p1)], [0.375, 0.5], [0.5, 0.25]])
    assert np.allclose(r["sum_e"], E, rtol=1e-15) and np.allclose(r["last"]["tV"], V, rtol=1e-15)
    T, R = r["sum_t"].astype(float), r["sum_r"].astype(float)
    assert np.allclose(r["sum_z"], (T - E) / np.sqrt(V), rtol=1e-14, atol=1e-16)
    assert np.allclose(r["chi_obs_sum"], ((T - E) ** 2 / V).sum(axis=0), rtol=1e-14)
    assert np.allclose(r["chi_rep_sum"], ((R - E) ** 2 / V).sum(axis=0), rtol=1e-14)
    # item 0: X2(T) = 0 + 1 / 0.375 + 0, X2(R) = 2 + 1 / 0.375 + 0 -> rep > obs; item 1: T = (0, 1, 1), R = (0, 2, 1)
    for k in ("chi_ge", "chi_gt"):
        assert np.array_equal(r[k][0], r[k][1])
    assert np.array_equal(r["chi_ge"][0], [1, 1]) and np.array_equal(r["chi_gt"][0], [1, 1]) and r["undecided"] == 0
    assert np.array_equal(r["obs_rate"], T / r["sum_n"]) and np.array_equal(r["n_mean"], r["sum_n"].astype(float))
    assert np.array_equal(r["ppp_chi2"], [1.0, 1.0]) and np.array_equal(r["bin_lo"], [-5.0, -0.5, 0.5])
    assert np.array_equal(r["bin_hi"], [-0.5, 0.5, 5.0])


def _mirror(theta):
    """theta -> -theta ON THE GRID: the grid point 1000 - k (-theta itself need not be bit for bit a grid point)"""
    return _grid(1000 - np.rint((theta + 5.0) * 100.0))


def _random(n, m, S, seed, cuts):
    rng = np.random.default_rng(seed)
    y = np.where(rng.random((n, m)) < 0.5, 1.0, -1.0)
    y[rng.random((n, m)) < 0.15] = np.nan
    theta = _grid(np.clip(np.rint(500 + 100 * rng.standard_normal((S, n))), 0, 1000))
    g = 1.5 * rng.standard_normal((S, n, m))
    rep = rng.random((S, n, m)) < 1.0 / (1.0 + np.exp(-g))
    return y, theta, g, rep


@pytest.mark.parametrize("h", [1, 4, 15])
def test_reflection(h):
    cuts = CUT_SETS[h]
    y, theta, g, rep = _random(60, 5, 4, 7 + h, cuts)
    a = P.bins_from_rep(y, theta, g, rep, cuts)
    b = P.bins_from_rep(y, _mirror(theta), g, rep, cuts, signs=-1)
    assert a["bin_draws"] == 4 == b["bin_draws"]
    for k in INT_KEYS:
        assert np.array_equal(a[k], b[k]), k
    for k in ("chi_ge", "chi_gt"):
        assert np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][1], b[k][1])
    for k in ("sum_e", "sum_z", "chi_obs_sum", "chi_rep_sum"):           # (the bins enter X2 in the other order: rounding only)
        assert np.allclose(a[k], b[k], rtol=1e-14, atol=1e-14), k
    # without the sign the bin axis comes out reversed
    c = P.bins_from_rep(y, _mirror(theta), g, rep, cuts)
    assert np.array_equal(c["sum_n"], a["sum_n"][::-1]) and np.array_equal(c["occ_sum"], a["occ_sum"][::-1])
    # mixed signs per draw
    sg = np.array([1, -1, 1, -1])
    d = P.bins_from_rep(y, np.where(sg[:, None] < 0, _mirror(theta), theta), g, rep, cuts, signs=sg)
    for k in INT_KEYS:
        assert np.array_equal(a[k], d[k]), k


def test_integer_tie_counts_in_ge_only():
    cuts = P.DEFAULT_CUTS
    y, theta, g, _ = _random(80, 4, 3, 21, cuts)
    rep = np.broadcast_to(y > 0, (3,) + y.shape)                          # the replicate equals the data: R_b = T_b everywhere
    r = P.bins_from_rep(y, theta, g, rep, cuts)
    assert np.array_equal(r["chi_ge"][0], [3] * 4) and np.array_equal(r["chi_ge"][1], [3] * 4)
    assert not r["chi_gt"][0].any() and not r["chi_gt"][1].any() and r["undecided"] == 0
    assert np.array_equal(r["ppp_chi2"], np.ones(4)) and np.array_equal(r["ppp_chi2_mid"], np.full(4, 0.5))
    live = r["sum_n"] > 0
    assert np.array_equal(r["cell_ge"], 3 - r["cell_empty"]) and not r["cell_gt"].any()
    assert np.array_equal(r["ppp_cell_mid"][live], np.full(live.sum(), 0.5))
    assert np.array_equal(r["sum_t"], r["sum_r"]) and np.array_equal(r["chi_obs_sum"], r["chi_rep_sum"])


def test_skipped_draws_change_only_the_counter():
    cuts = (30, 90)
    y, theta, g, rep = _random(50, 3, 4, 33, cuts)
    y[5, 1] = 1.0
    y[6, 2] = np.nan
    base = P.bins_from_rep(y, theta[[0, 3]], g[[0, 3]], rep[[0, 3]], cuts)
    th, gg = theta.copy(), g.copy()
    th[1, 9] += 1e-4                                                        # off the grid
    gg[2, 5, 1] = np.nan                                                    # a non-finite g in an observed cell
    gg[3, 6, 2] = np.nan                                                    # ... in an UNOBSERVED cell: counts normally
    r = P.bins_from_rep(y, th, gg, rep, cuts)
    assert r["bin_draws"] == 2 and r["bin_skipped"] == 2 and base["bin_skipped"] == 0
    for k in INT_KEYS + ("sum_e", "sum_z", "chi_obs_sum", "chi_rep_sum", "obs_rate", "ppp_chi2"):
        assert np.array_equal(r[k], base[k], equal_nan=True), k
    for bad in (np.nan, np.inf, 5.01):
        th2 = theta.copy()
        th2[0, 0] = bad
        assert P.bins_from_rep(y, th2, g, rep, cuts)["bin_skipped"] == 1
    none = P.bins_from_rep(y, th[[1]], gg[[1]], rep[[1]], cuts)
    assert none["bin_draws"] == 0 and np.isnan(none["ppp_chi2"]).all() and np.isnan(none["obs_rate"]).all()
    assert (none["worst"]["items"] == -1).all() and none["last"] is None


def test_empty_cells_and_v_zero():
    # everyone in the centre bin; item 1 at g = +-800 (V = 0: no z, a zero chi-square term)
    n, cuts = 12, (14, 43)
    y = np.ones((n, 2))
    y[::2] = -1.0
    theta = np.zeros((2, n))
    g = np.zeros((2, n, 2))
    g[:, :, 1] = np.where(y[:, 1] > 0, 800.0, -800.0)
    rep = np.broadcast_to(y > 0, (2, n, 2)).copy()
    rep[:, 0, 0] = True
    r = P.bins_from_rep(y, theta, g, rep, cuts)
    c = len(cuts)
    off = np.arange(5) != c
    assert np.array_equal(r["cell_empty"][off], np.full((4, 2), 2)) and not r["cell_empty"][c].any()
    for k in ("sum_n", "sum_t", "sum_r", "cell_ge", "cell_gt", "sum_e", "sum_z"):
        assert not r[k][off].any(), k
    assert np.isnan(r["obs_rate"][off]).all() and np.isnan(r["z_mean"][off]).all() and np.isnan(r["ppp_cell"][off]).all()
    assert np.array_equal(r["n_mean"][:, 0], [0, 0, n, 0, 0]) and np.array_equal(r["occupancy"], [0, 0, n, 0, 0])
    assert r["sum_e"][c, 1] == n / 2 * 2 and r["sum_z"][c, 1] == 0.0 and r["chi_obs_sum"][1] == 0.0 and r["chi_rep_sum"][1] == 0.0
    assert np.array_equal(r["chi_ge"][0], [2, 2]) and np.array_equal(r["chi_gt"][0], [2, 0])    # item 1: an integer tie


def test_worst_ordering_ties_and_padding():
    mid = np.array([0.5, 0.1, np.nan, 0.1, 0.0, 0.9, 0.5])
    obs = np.arange(7.0)
    w = P.bins_worst(mid, obs, top=10)
    assert list(w["items"]) == [4, 1, 3, 0, 6, 5, -1, -1, -1, -1]
    assert np.array_equal(w["ppp_chi2_mid"][:6], mid[[4, 1, 3, 0, 6, 5]]) and np.isnan(w["ppp_chi2_mid"][6:]).all()
    assert np.array_equal(w["chi2_obs_mean"][:6], obs[[4, 1, 3, 0, 6, 5]]) and np.isnan(w["chi2_obs_mean"][6:]).all()
    assert list(P.bins_worst(mid, obs, top=2)["items"]) == [4, 1]
    y, theta, g, rep = _random(60, 9, 6, 5, P.DEFAULT_CUTS)
    y[:, 8] = np.nan                                                      # never observed: an integer tie in every draw
    r = P.bins_from_rep(y, theta, g, rep, top=64)
    m = r["ppp_chi2_mid"]
    want = sorted(range(9), key=lambda j: (m[j], j))
    assert list(r["worst"]["items"][:9]) == want and (r["worst"]["items"][9:] == -1).all() and m[8] == 0.5


def test_from_draws_matches_from_rep_and_finds_a_planted_misfit():
    """Item 3's data follow a U-shaped curve, g says flat: its binned chi-square is far above every replicate's, while its
    yes count is well replicated."""
    n, m, S, seed = 600, 4, 40, 99
    rng = np.random.default_rng(8)
    k = np.clip(np.rint(500 + 100 * rng.standard_normal(n)), 0, 1000)
    theta = _grid(k)
    slope = np.array([1.0, 1.4, 0.7, 0.0])
    g = theta[:, None] * slope[None, :]
    ptrue = 1.0 / (1.0 + np.exp(-g))
    ptrue[:, 3] = np.where(np.abs(theta) > 0.76, 0.9, 0.22)
    y = np.where(rng.random((n, m)) < ptrue, 1.0, -1.0)
    th, gd = np.broadcast_to(theta, (S, n)), np.broadcast_to(g, (S, n, m))
    r, gap = P.bins_from_draws(y, th, gd, seed, range(1, S + 1), top=2)
    assert gap > 0 and r["bin_draws"] == S and r["undecided"] == 0
    assert r["worst"]["items"][0] == 3 and r["ppp_chi2"][3] == 0.0 and (r["ppp_chi2"][:3] > 0.02).all()
    assert r["obs_rate"][0, 3] > 0.8 and r["obs_rate"][4, 3] < 0.35 and abs(r["exp_rate"][4, 3] - 0.5) < 1e-12
    reps = np.stack([(~np.isnan(y)) & (P.replicate_uniforms(seed, it, n, m) < P._plogis(g)[0]) for it in range(1, S + 1)])
    r2 = P.bins_from_rep(y, th, gd, reps, top=2)
    for key in INT_KEYS:
        assert np.array_equal(r[key], r2[key]), key


def test_c_abi_of_version_112():
    lib = _lib.load()
    assert lib.gpirt_version() >= 112
    p = _lib.PpcBins()
    assert C.sizeof(p) == 8 + 4 * 16 + 8 * (7 + 4 + 3 + 5 + 3 + 2 + 2 + 1 + 3) + 8 * 9
    for name in ("gpirt_sampler_ppc_bins_enable", "gpirt_sampler_ppc_bins_get", "gpirt_sampler_ppc_bins_state",
                 "gpirt_ppc_bins_combine", "gpirt_mcmc_run"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    # argument errors come back before any device is touched
    p.top = 20
    assert lib.gpirt_ppc_bins_combine(None, 1, None, None, C.byref(p)) == _lib.E_ARG
    assert lib.gpirt_sampler_ppc_bins_enable(None, 4, (C.c_int * 4)(*P.DEFAULT_CUTS), 1) == _lib.E_ARG
    assert lib.gpirt_sampler_ppc_bins_get(None, b"obs_rate", None, 0) == _lib.E_ARG
