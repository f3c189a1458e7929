"""gpirt_amd.equate's NumPy statement (from_draws) on its own: against brute-force enumeration of all answer patterns, its ties to
gpirt_amd.sumscore, the properties of the equating function, the clamped edge, the constructed curves that the GPU tests use
against tests/_equate_bounds.py's keep conditions, the argument checks and the C ABI of version 116.  No device is needed."""
import ctypes as C
import itertools

import numpy as np
import pytest

import _equate_bounds as B
import _equate_cases as CASES
from gpirt_amd import _lib
from gpirt_amd import equate as EQ
from gpirt_amd import sumscore as SS

N = 1001
TH = -5.0 + np.arange(N) * 0.01


def twopl(a, b):
    return a[None, :] * (TH[:, None] - b[None, :])


def brute_joint(f, x, y):
    """J[s, t] by enumeration of all 2^(M_X + M_Y) answer patterns, in long double"""
    fl = f.astype(np.longdouble)
    one = np.longdouble(1)
    p, q = one / (one + np.exp(-fl)), one / (one + np.exp(fl))
    w = SS.grid_weights().astype(np.longdouble)
    cols = list(x) + list(y)
    J = np.zeros((len(x) + 1, len(y) + 1), dtype=np.longdouble)
    for pat in itertools.product([0, 1], repeat=len(cols)):
        like = np.ones(N, dtype=np.longdouble)
        for j, yes in zip(cols, pat):
            like = like * (p[:, j] if yes else q[:, j])
        J[sum(pat[:len(x)]), sum(pat[len(x):])] += (w * like).sum()
    return J


@pytest.mark.parametrize("x,y", [([0], [1]), ([3, 0, 5], [1, 2]), ([1, 2, 4, 7, 8, 11], [0, 3, 5, 6, 9, 10])])
def test_joint_against_enumeration_and_the_sum_score_module(x, y):
    rng = np.random.default_rng(len(x))
    f = twopl(rng.uniform(0.4, 2.0, 12) * rng.choice([-1.0, 1.0], 12), rng.normal(size=12)) + 0.3 * rng.normal(size=(N, 12))
    r = EQ.from_draws(f[None], x, y)
    want = brute_joint(f, sorted(x), sorted(y)).astype(np.float64)
    tol = 4096 * 20 * B.EPS
    assert np.allclose(r["last_joint"], want, rtol=tol, atol=0.0) and np.array_equal(r["joint_sum"], r["last_joint"])
    sx, sy, su = (SS.from_draws(f[None], items=it) for it in (x, y, list(x) + list(y)))
    assert np.allclose(r["last_pix"], sx["last_pi"], rtol=tol, atol=0.0) and np.allclose(r["last_piy"], sy["last_pi"], rtol=tol, atol=0.0)
    assert np.allclose(r["last_joint"].sum(axis=1), sx["last_pi"], rtol=tol, atol=0.0)
    assert np.allclose(r["last_joint"].sum(axis=0), sy["last_pi"], rtol=tol, atol=0.0)
    J = r["last_joint"]
    anti = np.array([sum(J[s, u - s] for s in range(J.shape[0]) if 0 <= u - s < J.shape[1]) for u in range(len(x) + len(y) + 1)])
    assert np.allclose(anti, su["last_pi"], rtol=tol, atol=0.0)                 # the two scores add up to the union's score
    assert abs(r["joint"].sum() - 1.0) < 1e-12 and r["draws"] == 1 and r["eq_clamped"] == 0
    # the correlation against the joint's own moments
    s, t = np.arange(len(x) + 1.0), np.arange(len(y) + 1.0)
    ex, ey = J.sum(axis=1) @ s, J.sum(axis=0) @ t
    cov = s @ J @ t - ex * ey
    vx, vy = J.sum(axis=1) @ (s * s) - ex * ex, J.sum(axis=0) @ (t * t) - ey * ey
    assert abs(r["corr_mean"] - cov / np.sqrt(vx * vy)) < 1e-10


def test_the_equating_function():
    rng = np.random.default_rng(2)
    a, b = rng.uniform(0.6, 2.0, 5), rng.normal(size=5)
    f = np.concatenate([twopl(a, b), twopl(a, b)], axis=1)                      # two forms with the same curves
    r = EQ.from_draws(f[None], range(5), range(5, 10))
    assert np.array_equal(r["last_eyx"], np.arange(6.0)) and np.array_equal(r["last_exy"], np.arange(6.0))
    assert np.array_equal(r["last_pix"], r["last_piy"]) and r["y_of_x_sd"].shape == (6,)
    # an easier, longer form Y: more Y points than X points for every X score, increasing in s, inside [-1/2, M_Y + 1/2], and the two
    # functions undo each other up to the discreteness of the scores
    f = np.concatenate([twopl(a, b), twopl(np.tile(a, 2), np.tile(b, 2) - 0.7)], axis=1) + 0.1 * rng.normal(size=(3, N, 15))
    r = EQ.from_draws(f, range(5), range(5, 15), cuts=((3, 7),))
    for d in range(3):
        one = EQ.from_draws(f[d:d + 1], range(5), range(5, 15))
        eyx, exy = one["last_eyx"], one["last_exy"]
        assert (np.diff(eyx) > 0).all() and (np.diff(exy) > 0).all()
        assert eyx.min() >= -0.5 and eyx.max() <= 10.5 and exy.min() >= -0.5 and exy.max() <= 5.5
        assert (eyx > np.arange(6.0) + 1.0).all() and (exy < np.arange(11.0)).all()   # Y is twice as long AND easier
        back = np.interp(eyx, np.arange(11.0), exy)
        assert np.abs(back - np.arange(6.0)).max() < 0.5
    assert np.allclose(r["y_of_x_mean"], r["eyx_sum"] / 3) and (r["y_of_x_sd"] > 0).all() and r["draws"] == 3
    # the concordance, the agreement and kappa from the pooled joint
    J = r["joint_sum"]
    assert np.allclose(r["y_given_x"], J / J.sum(axis=1, keepdims=True)) and np.allclose(r["x_given_y"], (J / J.sum(axis=0)).T)
    assert np.allclose(r["y_given_x"].sum(axis=1), 1.0) and np.allclose(r["y_given_x_mean"], r["y_given_x"] @ np.arange(11.0))
    assert r["y_given_x_quantiles"].shape == (3, 6) and (np.diff(r["y_given_x_quantiles"], axis=0) >= 0).all()
    Jn = J / J.sum()
    agree = Jn[3:, 7:].sum() + Jn[:3, :7].sum()
    px, py = Jn[3:].sum(), Jn[:, 7:].sum()
    pe = px * py + (1 - px) * (1 - py)
    assert np.isclose(r["agreement"][0], agree) and np.isclose(r["kappa"][0], (agree - pe) / (1 - pe)) and 0 < r["kappa"][0] < 1
    assert 0 < r["corr_mean"] < 1 and r["corr_draws"] == 3
    # a row without mass gives NaN
    fin = EQ.finish(dict(r, joint_sum=np.where(np.arange(6)[:, None] == 2, 0.0, J)), draws=3, corr_draws=3)
    assert np.isnan(fin["y_given_x"][2]).all() and np.isnan(fin["y_given_x_mean"][2]) and np.isnan(fin["y_given_x_quantiles"][:, 2]).all()


def test_the_clamped_edge():
    e, n = EQ.equivalents(np.array([0.5, 0.5, 0.0]), np.array([0.5, 0.5]))
    assert n == 1 and np.array_equal(e, [0.0, 1.0, 1.5])                          # P[2] = 1 = F_Y[1]: no t with F_Y[t] > P
    f = np.zeros((1, N, 3))
    f[:, :, 0] = f[:, :, 2] = twopl(np.array([1.3]), np.array([0.2]))[:, 0]
    f[:, :, 1] = -np.inf                                                          # an item nobody answers yes: pi_X[2] = 0
    r = EQ.from_draws(f, [0, 1], [2])
    assert r["last_pix"][2] == 0.0 and r["eq_clamped"] == 1 and np.array_equal(r["last_eyx"], [0.0, 1.0, 1.5])
    assert np.isfinite(r["last_exy"]).all()


def test_nan_in_either_form_skips_the_draw():
    rng = np.random.default_rng(3)
    f = rng.normal(size=(4, N, 6))
    f[1, 7, 0] = f[2, 1000, 4] = f[3, 3, 5] = np.nan                               # in X, in Y, outside both
    r = EQ.from_draws(f, [0, 1], [3, 4])
    assert (r["draws"], r["skipped"]) == (2, 2)
    clean = EQ.from_draws(f[[0, 3]], [0, 1], [3, 4])
    assert np.array_equal(r["joint_sum"], clean["joint_sum"]) and np.array_equal(r["last_eyx"], clean["last_eyx"])


def test_pooling_is_plain_addition():
    rng = np.random.default_rng(8)
    f = rng.normal(size=(5, N, 7))
    whole, parts = EQ.from_draws(f, [0, 2, 4], [1, 5]), EQ.from_draws([f[:3], f[3:]], [0, 2, 4], [1, 5])
    for k in ("joint_sum", "pix_sum", "eyx_sumsq", "corr"):
        assert np.allclose(whole[k], parts[k], rtol=1e-15, atol=0.0), k
    assert np.array_equal(whole["last_joint"], parts["last_joint"]) and parts["draws"] == 5
    rev = EQ.from_draws(f[:, ::-1], [0, 2, 4], [1, 5])                             # theta -> -theta: only the order of the sums
    assert np.allclose(whole["joint_sum"], rev["joint_sum"], rtol=1e-14, atol=0.0) and np.allclose(whole["corr"], rev["corr"], rtol=1e-12)


@pytest.mark.parametrize("Mx,My", CASES.SHAPES)
def test_constructed_curves_meet_the_keep_conditions(Mx, My):
    """the cases of tests/test_gpu_equate.py, from the reference alone: every score in the body of either distribution is
    compared, and at most a quarter of the equating cells are left out"""
    x, y, draws = CASES.small_case(Mx, My)
    singles = [EQ.from_draws(f[None], x, y) for f in draws]
    share = B.keep_conditions(singles, quarter=True, label=f"({Mx}, {My})")
    print(f"MEASURED ({Mx}, {My}): equating cells left out {share:.3f}")
    assert np.abs(np.stack(draws)).max() <= 4.0
    bd = B.bounds(EQ.from_draws(np.stack(draws), x, y), singles)
    assert np.isfinite(bd["corr"]).all()


def test_arguments_are_checked():
    m = 6
    for x, y, word in (([], [1], "empty"), ([0], np.zeros(m, dtype=bool), "empty"), ([0, 1, 2], [4, 2, 1], "column 1 is in both"),
                       ([0], None, "missing"), ([6], [1], "outside"), ([0, 0], [1], "more than once"), ([0.5], [1], "items")):
        with pytest.raises(ValueError, match=word):
            EQ.form_masks(x, y, m)
        with pytest.raises(ValueError, match=word):
            EQ.parse(dict(x=x, y=y), m)
    with pytest.raises(ValueError, match="at most 2048"):
        EQ.form_masks(np.arange(2049), [2049], 2050)
    EQ.form_masks(np.arange(2048), [2048], 2049)
    with pytest.raises(ValueError, match="unknown keys"):
        EQ.parse(dict(x=[0], y=[1], items=[2]), m)
    with pytest.raises(ValueError, match="dict"):
        EQ.parse(True, m)
    with pytest.raises(ValueError, match="probs"):
        EQ.parse(dict(x=[0], y=[1], probs=(1.5,)), m)
    for cuts, word in ((((0, 1),), "1 <= cx"), (((1, 2),), "cy <= 1"), (((3, 1),), "cx <= 2"), (((1, 1),) * 9, "at most 8"),
                       ((1, 1, 1), "pairs"), (((0.5, 1),), "pairs")):
        with pytest.raises(ValueError, match=word):
            EQ.parse(dict(x=[0, 2], y=[1], cuts=cuts), m)
    p = EQ.parse(dict(x=np.array([True, False, True, False, False, False]), y=[1], cuts=((2, 1),)), m)
    assert p["mask_x"].tolist() == [1, 0, 1, 0, 0, 0] and p["mask_y"].tolist() == [0, 1, 0, 0, 0, 0] and p["cuts"].tolist() == [[2, 1]]
    with pytest.raises(ValueError, match="1001"):
        EQ.from_draws(np.zeros((1, 10, 3)), [0], [1])


def test_c_abi_of_version_116():
    lib = _lib.load()
    assert lib.gpirt_version() >= 116
    p = _lib.Equate()
    assert C.sizeof(p) == 8 * 2 + 8 * 19 + 8 * 3 + 8 * 5 + 8 * 4 and len(_lib.EQUATE_RAW) == 19
    for name in ("gpirt_sampler_equate_enable", "gpirt_sampler_equate_accumulate", "gpirt_sampler_equate_get",
                 "gpirt_sampler_equate_state", "gpirt_equate_state_bytes", "gpirt_equate_combine", "gpirt_mcmc_run"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.Run.equate.offset == _lib.Run.dif.offset + 8              # gpirt_run: equate follows dif
    # argument errors come back before any device is touched
    assert lib.gpirt_equate_combine(None, 1, None, C.byref(p)) == _lib.E_ARG
    assert lib.gpirt_sampler_equate_enable(None, None, None, 1) == _lib.E_ARG
    nb = C.c_int64()
    assert lib.gpirt_equate_state_bytes(10, 3, 4, C.byref(nb)) == 0
    words = 16 + sum((b + 15) // 16 * 2 for b in (8 * 20, 8 * 4, 8 * 4, 8 * 5, 8 * 5, 8 * 4, 8 * 4, 8 * 5, 8 * 5, 16, 40, 10, 10, 8 * 1001,
                                                   8 * 20, 8 * 4, 8 * 5, 8 * 4, 8 * 5))
    assert nb.value == 8 * words
    for bad in ((10, 0, 4), (10, 6, 5), (5000, 2049, 1), (5000, 1, 2049)):
        assert lib.gpirt_equate_state_bytes(*bad, C.byref(nb)) == _lib.E_ARG
    assert lib.gpirt_equate_state_bytes(5000, 2048, 2048, C.byref(nb)) == 0
