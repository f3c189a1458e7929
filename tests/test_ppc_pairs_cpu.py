"""The pairwise item checks of the PPC without a device: gpirt_amd.ppc.pairs_from_rep (the NumPy statement of the header,
"pairwise item checks") against a triple loop over (a, b, i), the tables' identities, the odds-ratio decisions against
fractions.Fraction, the deterministic replicate, the ordering of `extreme`, a planted dependence, and the C ABI of library
version 111."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from gpirt_amd import _lib
from gpirt_amd import ppc as P

INT_KEYS = _lib.PAIRS_SUMS + _lib.PAIRS_COUNTS


def _data(n, m, seed, S=5):
    """y with missing cells, one all-missing column (the last) and a pair without a co-observed respondent (0, 1)"""
    rng = np.random.default_rng(seed)
    y = np.where(rng.random((n, m)) < 0.55, 1.0, -1.0)
    y[rng.random((n, m)) < 0.1] = np.nan
    y[:, m - 1] = np.nan
    y[: n // 2, 0] = np.nan
    y[n // 2:, 1] = np.nan
    rep = rng.random((S, n, m)) < 0.5
    return y, rep


def _loops(y, rep):
    """the header, cell by cell: per draw and ordered pair the tables by a loop over the respondents"""
    S, n, m = rep.shape
    obs = ~np.isnan(y)
    z = lambda: [[0] * m for _ in range(m)]              # noqa: E731
    out = {k: z() for k in INT_KEYS + ("n_co", "o11", "o10", "o01", "o00")}
    for a in range(m):
        for b in range(m):
            co = [i for i in range(n) if obs[i, a] and obs[i, b]]
            out["n_co"][a][b] = len(co)
            if a == b or not co:
                continue
            o = [[0, 0], [0, 0]]
            for i in co:
                o[int(y[i, a] > 0)][int(y[i, b] > 0)] += 1
            out["o11"][a][b], out["o10"][a][b], out["o01"][a][b], out["o00"][a][b] = o[1][1], o[1][0], o[0][1], o[0][0]
            for s in range(S):
                r = [[0, 0], [0, 0]]
                for i in co:
                    r[int(rep[s, i, a])][int(rep[s, i, b])] += 1
                out["sum_n11"][a][b] += r[1][1]
                out["sumsq_n11"][a][b] += r[1][1] ** 2
                out["sum_n1"][a][b] += r[1][1] + r[1][0]
                out["n11_ge"][a][b] += r[1][1] >= o[1][1]
                out["n11_gt"][a][b] += r[1][1] > o[1][1]
                out["agree_ge"][a][b] += r[1][1] + r[0][0] >= o[1][1] + o[0][0]
                out["agree_gt"][a][b] += r[1][1] + r[0][0] > o[1][1] + o[0][0]
                orr = Fraction((2 * r[1][1] + 1) * (2 * r[0][0] + 1), (2 * r[1][0] + 1) * (2 * r[0][1] + 1))
                oro = Fraction((2 * o[1][1] + 1) * (2 * o[0][0] + 1), (2 * o[1][0] + 1) * (2 * o[0][1] + 1))
                out["or_ge"][a][b] += orr >= oro
                out["or_gt"][a][b] += orr > oro
    return {k: np.array(v, dtype=np.int64) for k, v in out.items()}


@pytest.mark.parametrize("n,m", [(7, 4), (40, 9)])
def test_pairs_from_rep_against_a_triple_loop(n, m):
    y, rep = _data(n, m, seed=n)
    S = rep.shape[0]
    got = P.pairs_from_rep(y, rep, top=5)
    want = _loops(y, rep)
    assert want["n_co"][0, 1] == 0 and not want["n_co"][:, m - 1].any()
    for k in INT_KEYS:
        assert np.array_equal(got[k].astype(np.int64), want[k]), k
    assert np.array_equal(got["n_co"], want["n_co"].astype(float))
    live = (want["n_co"] > 0) & ~np.eye(m, dtype=bool)
    for k, w in (("obs_n11", "o11"), ("obs_n10", "o10"), ("obs_n01", "o01"), ("obs_n00", "o00")):
        assert np.array_equal(got[k][live], want[w][live].astype(float)), k
    # the tables add up to n_co, and table[a, b] is table[b, a] with n10 <-> n01
    for pre in ("obs", "rep"):
        suf = "" if pre == "obs" else "_mean"
        t = [got[f"{pre}_n{c}{suf}"] for c in ("11", "10", "01", "00")]
        total = t[0] + t[1] + t[2] + t[3]
        assert np.allclose(total[live], want["n_co"][live], rtol=1e-14, atol=0)
        assert np.array_equal(t[0], t[0].T, equal_nan=True) and np.array_equal(t[3], t[3].T, equal_nan=True)
        assert np.array_equal(t[1], t[2].T, equal_nan=True)
    assert np.array_equal(got["obs_n11"][live] + got["obs_n10"][live] + got["obs_n01"][live] + got["obs_n00"][live],
                          want["n_co"][live].astype(float))
    # the finished values are what the header says of the sums
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(got["rep_n11_mean"][live], (want["sum_n11"] / S)[live])
        assert np.array_equal(got["ppp_or"][live], (want["or_ge"] / S)[live])
        assert np.array_equal(got["ppp_or_mid"][live], ((want["or_ge"] + want["or_gt"]) / (2 * S))[live])
        assert np.array_equal(got["ppp_n11_mid"][live], ((want["n11_ge"] + want["n11_gt"]) / (2 * S))[live])
        assert np.array_equal(got["ppp_agree"][live], (want["agree_ge"] / S)[live])
        assert np.array_equal(got["agree_obs"][live], ((want["o11"] + want["o00"]) / want["n_co"])[live])
    a, b = np.argwhere(live)[0]
    var = np.var([int(((rep[s, :, a] & rep[s, :, b])[~np.isnan(y[:, a]) & ~np.isnan(y[:, b])]).sum()) for s in range(S)], ddof=1)
    assert math.isclose(got["rep_n11_var"][a, b], var, rel_tol=1e-12, abs_tol=1e-12)
    lo = math.log((want["o11"][a, b] + 0.5) * (want["o00"][a, b] + 0.5) / ((want["o10"][a, b] + 0.5) * (want["o01"][a, b] + 0.5)))
    assert math.isclose(got["log_or_obs"][a, b], lo, rel_tol=1e-13, abs_tol=1e-13)
    # the diagonal and the pairs without a co-observed respondent: every counter 0, every finished value NaN
    for k in INT_KEYS:
        assert not got[k][~live].any(), k
    for k in _lib.PAIRS_FIELDS[1:]:
        assert np.isnan(got[k][~live]).all() and not np.isnan(got[k][live]).any() , k
    assert got["pair_draws"] == S and got["pair_skipped"] == 0


def test_replicate_equal_to_the_data_ties_every_comparison():
    y, _ = _data(40, 9, seed=3)
    S = 4
    rep = np.broadcast_to(y > 0, (S,) + y.shape)
    got = P.pairs_from_rep(y, rep)
    live = (got["n_co"] > 0) & ~np.eye(9, dtype=bool)
    for k in ("n11", "agree", "or"):
        assert np.array_equal(got[f"{k}_ge"], S * live) and not got[f"{k}_gt"].any(), k
        assert np.array_equal(got[f"ppp_{k}"][live], np.ones(live.sum()))
        assert np.array_equal(got[f"ppp_{k}_mid"][live], np.full(live.sum(), 0.5))
    assert np.array_equal(got["rep_n11_mean"][live], got["obs_n11"][live]) and not got["rep_n11_var"][live].any()
    assert np.array_equal(got["agree_rep_mean"][live], got["agree_obs"][live])


def test_extreme_ordering_ties_and_padding():
    y, rep = _data(40, 6, seed=11, S=4)
    got = P.pairs_from_rep(y, rep, top=64)
    mid = got["ppp_or_mid"]
    cand = [(a, b) for a in range(6) for b in range(a + 1, 6) if not np.isnan(mid[a, b])]
    cand.sort(key=lambda ab: (-abs(mid[ab] - 0.5), ab))
    ex = got["extreme"]
    k = len(cand)
    assert 0 < k < 15 and ex["pairs"].shape == (64, 2)
    assert [tuple(p) for p in ex["pairs"][:k]] == cand
    assert len({abs(mid[ab] - 0.5) for ab in cand}) < k          # ties exist: the lowest (a, b) came first
    assert (ex["pairs"][k:] == -1).all() and np.isnan(ex["ppp_or_mid"][k:]).all() and np.isnan(ex["log_or_obs"][k:]).all()
    assert np.array_equal(ex["ppp_or_mid"][:k], [mid[ab] for ab in cand])
    assert np.array_equal(ex["log_or_obs"][:k], [got["log_or_obs"][ab] for ab in cand])
    short = P.pairs_from_rep(y, rep, top=3)["extreme"]
    assert np.array_equal(short["pairs"], ex["pairs"][:3])
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError):
            P.pairs_from_rep(y, rep, top=bad)


def test_planted_dependence_is_the_most_extreme_pair():
    """n = 400, m = 6, item 5 a copy of item 4, g fixed at the generating 2PL values: the replicates draw items 4 and 5
    independently given theta, the data do not, so the pair's observed odds ratio is far above every replicate's."""
    n, m, S, seed = 400, 6, 200, 12345
    rng = np.random.default_rng(4)
    theta = rng.standard_normal(n)
    slope, icpt = rng.uniform(0.8, 1.6, m), rng.uniform(-0.5, 0.5, m)
    g = theta[:, None] * slope[None, :] + icpt[None, :]
    g[:, 5] = g[:, 4]
    y = np.where(rng.random((n, m)) < 1.0 / (1.0 + np.exp(-g)), 1.0, -1.0)
    y[:, 5] = y[:, 4]
    got, gap = P.pairs_from_draws(y, np.broadcast_to(g, (S, n, m)), seed, range(1, S + 1), top=3)
    assert gap > 0 and got["pair_draws"] == S and got["pair_skipped"] == 0
    assert tuple(got["extreme"]["pairs"][0]) == (4, 5)
    iu = np.triu_indices(m, 1)
    ppp = got["ppp_or"][iu]
    assert ppp.argmin() == list(zip(*iu)).index((4, 5)) and (np.sort(ppp)[1] > ppp.min())
    assert got["ppp_or"][4, 5] == 0.0 and got["extreme"]["ppp_or_mid"][0] == 0.0
    assert got["agree_obs"][4, 5] == 1.0 and got["agree_rep_mean"][4, 5] < 0.9
    # a draw with a non-finite g in an observed cell is skipped whole
    gb = np.broadcast_to(g, (3, n, m)).copy()
    gb[1, 7, 2] = np.nan
    sk, _ = P.pairs_from_draws(y, gb, seed, [1, 2, 3])
    assert sk["pair_draws"] == 2 and sk["pair_skipped"] == 1
    two, _ = P.pairs_from_draws(y, gb[[0, 2]], seed, [1, 3])
    for k in INT_KEYS:
        assert np.array_equal(sk[k], two[k]), k


def test_c_abi_of_version_111():
    lib = _lib.load()
    assert lib.gpirt_version() >= 111
    p = _lib.PpcPairs()
    assert C.sizeof(p) == 8 + 8 * (19 + 3 + 6 + 3) + 8 * 8
    for name in ("gpirt_sampler_ppc_pairs_enable", "gpirt_sampler_ppc_pairs_get", "gpirt_sampler_ppc_pairs_state",
                 "gpirt_ppc_pairs_combine", "gpirt_mcmc_run"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    # argument errors come back before any device is touched
    assert lib.gpirt_ppc_pairs_combine(None, 1, None, C.byref(p)) == _lib.E_ARG
    assert lib.gpirt_sampler_ppc_pairs_enable(None, 1) == _lib.E_ARG
