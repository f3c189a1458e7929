"""gpirt_amd.shape.from_draws, the NumPy statement of the shape posteriors (include/gpirt_hip.h, "IRF shape posteriors"), on
hand-built curves with known answers; the reflection of accumulators; the version-113 C ABI on a machine without a device."""
import ctypes as C

import numpy as np
import pytest

from gpirt_amd import _lib
from gpirt_amd import shape as SH

N = 1001
K = np.arange(N)
TH = -5.0 + K * 0.01
INT_KEYS = ("cls", "peak_hist", "valley_hist", "cross_first_hist", "cross_last_hist", "cross_count", "draws", "nonfinite")


def one(curve_columns, **kw):
    """from_draws of ONE draw whose columns are the given curves"""
    g = np.stack([np.asarray(c, dtype=np.float64) for c in curve_columns], axis=1)[None]
    return SH.from_draws(g, **kw)


def cls_of(r, t, j):
    return int(np.argmax(r["cls"][t, :, j]))


def test_linear_constant_peak_and_w():
    curves = [0.5 * TH, -2.0 * TH, np.full(N, 0.3), 1.0 - (TH - 0.63) ** 2, np.abs(np.abs(TH) - 1.0) - 0.5]
    r = one(curves, window=3.0, tols=(0.0, 0.25, 1.0))
    k_lo, k_hi = 200, 800
    assert (r["k_lo"], r["k_hi"]) == (k_lo, k_hi) and r["draws"].tolist() == [1] * 5 and r["info_draws"] == 1
    # linear up / down: monotone at every tolerance below the rise of 3 / 12 logits, extremes at the window's edges
    assert [cls_of(r, t, 0) for t in range(3)] == [SH.INCREASING] * 3
    assert [cls_of(r, t, 1) for t in range(3)] == [SH.DECREASING] * 3
    assert r["peak_hist"][k_hi, 0] == 1 and r["valley_hist"][k_lo, 0] == 1
    assert r["peak_hist"][k_lo, 1] == 1 and r["valley_hist"][k_hi, 1] == 1
    assert r["crossings"][1, 0] == 1.0 and r["crossings"][1, 1] == 1.0
    assert abs(r["slope_max_mean"][0] - 0.5) < 1e-12 and abs(r["slope_min_mean"][1] + 2.0) < 1e-11
    # constant: flat at every tolerance, all ties -> the lowest k, no crossing, no information
    assert [cls_of(r, t, 2) for t in range(3)] == [SH.FLAT] * 3
    assert r["peak_hist"][k_lo, 2] == 1 and r["valley_hist"][k_lo, 2] == 1 and r["crossings"][0, 2] == 1.0
    assert not r["item_info"][:, 2].any() and r["slope_max_mean"][2] == 0.0
    # one peak at theta = 0.63 (k = 563), rise 13.2 and fall 4.6 logits inside the window: non-monotone at every tolerance
    assert [cls_of(r, t, 3) for t in range(3)] == [SH.NONMONOTONE] * 3
    assert r["peak_hist"][563, 3] == 1 and r["p_peak_interior"][3] == 1.0 and r["p_peak_interior"][0] == 0.0
    assert r["crossings"][2, 3] == 1.0                       # 1 - (theta - 0.63)^2 = 0 at -0.37 and 1.63
    assert r["peak_quantiles"][:, 3].tolist() == [TH[563]] * 3
    assert abs(r["difficulty_quantiles"][1, 3] - (-0.37)) <= 0.01
    # a W: four crossings (counted as >= 3), valleys at +-1 (the lower k wins only on an exact tie)
    assert r["crossings"][3, 4] == 1.0 and cls_of(r, 0, 4) == SH.NONMONOTONE
    assert r["cross_first_hist"][:, 4].sum() == 1 and r["cross_last_hist"][:, 4].sum() == 1
    assert int(np.argmax(r["cross_first_hist"][:, 4])) < 400 and int(np.argmax(r["cross_last_hist"][:, 4])) > 600
    for t in range(3):
        assert np.array_equal(r["cls"][t].sum(axis=0), r["draws"])
        assert np.allclose(r["p_flat"][t] + r["p_increasing"][t] + r["p_decreasing"][t] + r["p_nonmonotone"][t], 1.0)
    assert r["nonmonotone"]["items"].tolist() == [3, 4, 0, 1, 2] and r["nonmonotone"]["p"].tolist() == [1, 1, 0, 0, 0]


def test_fall_equal_to_the_tolerance_is_within_it():
    g = np.where(K < 500, 0.0, 2.0)
    g[500], g[501] = 1.0, 0.75                              # rises to 1, falls by exactly 0.25, rises to 2
    r = one([g, -g], window=1.0, tols=(0.0, 0.25, 0.2499999999999999, 2.0))
    assert [cls_of(r, t, 0) for t in range(4)] == [SH.NONMONOTONE, SH.INCREASING, SH.NONMONOTONE, SH.FLAT]
    assert [cls_of(r, t, 1) for t in range(4)] == [SH.NONMONOTONE, SH.DECREASING, SH.NONMONOTONE, SH.FLAT]


def test_crossings_at_plus_and_minus_zero():
    a = np.full(N, -1.0); a[500] = 0.0                      # sgn: - + - : two crossings, pairs (499, 500) and (500, 501)
    b = np.full(N, -1.0); b[500] = -0.0                     # -0.0 >= 0 holds: the same
    c = np.full(N, 1.0); c[500] = -0.0                      # + + + : none
    d = np.full(N, 1.0); d[700] = -1.0                      # outside the window: none
    r = one([a, b, c, d], window=1.0)
    assert r["cross_count"].T.tolist() == [[0, 0, 1, 0], [0, 0, 1, 0], [1, 0, 0, 0], [1, 0, 0, 0]]
    for j in (0, 1):
        assert r["cross_first_hist"][499, j] == 1 and r["cross_last_hist"][500, j] == 1
    assert not r["cross_first_hist"][:, 2:].any()
    # +0 and -0 tie for the argmax: the lowest k
    e = np.full(N, -1.0); e[510], e[490] = 0.0, -0.0
    assert one([e], window=1.0)["peak_hist"][490, 0] == 1


def test_nonfinite_columns_are_skipped():
    g = np.stack([0.5 * TH, np.cos(TH)], axis=1)[None].repeat(3, axis=0)
    g[1, 0, 1] = np.nan                                     # outside the window: the item is skipped all the same
    g[2, 500, 0] = np.inf
    r = SH.from_draws(g, window=1.0)
    assert r["draws"].tolist() == [2, 2] and r["nonfinite"].tolist() == [1, 1]
    assert (r["info_draws"], r["info_skipped"]) == (1, 2)
    assert np.isfinite(r["info_sum"]).all() and np.isfinite(r["ti_sum"]).all()
    big = one([np.where(K < 500, -800.0, 800.0)], window=5.0)
    assert np.isfinite(big["info_sum"]).all() and big["info_sum"][:499].max() == 0.0


def test_reflection_of_accumulators_is_from_draws_of_the_reversed_curves():
    rng = np.random.default_rng(5)
    S, m = 6, 7
    a, b, c = rng.normal(size=(3, S, 1, m))
    g = a * TH[None, :, None] + b * np.sin(1.3 * TH[None, :, None] + c) + 0.3 * c       # smooth, no exact ties
    tols = (0.0, 0.5)
    acc, rev = SH.zeros(m, 2), SH.zeros(m, 2)
    for s in range(S):
        SH.accumulate(acc, g[s], 250, tols)
        SH.accumulate(rev, g[s, ::-1], 250, tols)
    ref = SH.reflect(acc)
    for k in INT_KEYS + ("slope", "info_sum", "ti_sum", "ti_sumsq"):
        assert np.array_equal(ref[k], rev[k]), k
    assert np.allclose(np.asarray(ref["rel"], dtype=np.float64), np.asarray(rev["rel"], dtype=np.float64), rtol=1e-15)
    assert ref["cls"][:, SH.INCREASING].sum() == acc["cls"][:, SH.DECREASING].sum() > 0
    # pooled through from_draws with signs: the same as adding by hand
    pooled = SH.from_draws([g, g], window=2.5, tols=tols, signs=[1, -1])
    for k in INT_KEYS:
        assert np.array_equal(pooled[k], acc[k] + ref[k]), k
    assert np.array_equal(pooled["peak_hist"], pooled["peak_hist"][::-1])


def test_reliability_of_a_2pl_item_set_against_its_closed_form():
    a = np.array([1.0, 0.5, 2.0, 1.3])
    b = np.array([0.0, 1.0, -1.0, 0.4])
    g = (a[None, :] * (TH[:, None] - b[None, :]))[None]
    r = SH.from_draws(g, window=3.0)
    p = 1.0 / (1.0 + np.exp(-g[0]))
    info = a[None, :] ** 2 * p * (1.0 - p)                  # I = a^2 p q: g' = a exactly up to the grid's rounding
    assert np.allclose(r["item_info"], info, rtol=1e-9, atol=0)
    ti = info.sum(axis=1)
    w = np.exp(-TH * TH / 2.0)
    w /= w.sum()
    assert abs(r["reliability_mean"] - float((w * ti / (ti + 1.0)).sum())) < 1e-12
    assert np.allclose(r["sem"], 1.0 / np.sqrt(ti), rtol=1e-9)
    assert np.isnan(r["reliability_sd"])                    # one draw
    assert r["difficulty_quantiles"][1].tolist() == pytest.approx(b.tolist(), abs=0.0051)


def test_arguments_are_checked():
    g = np.zeros((1, N, 1))
    for bad in (dict(window=0.001), dict(window=5.5), dict(tols=(0, 1, 2, 3, 4)), dict(tols=(-0.1,)), dict(top=0), dict(top=65),
                dict(probs=(1.5,))):
        with pytest.raises(ValueError, match="shape"):
            SH.from_draws(g, **bad)
    with pytest.raises(ValueError, match="unknown keys"):
        SH.parse(dict(windows=3.0))
    assert SH.parse(True)["k_half"] == 300 and SH.check_window(0.01) == 1 and SH.check_window(5.0) == 500


def test_c_abi_of_version_113():
    lib = _lib.load()
    assert lib.gpirt_version() >= 113
    p = _lib.Shape()
    assert C.sizeof(p) == 8 + 8 * 4 + 8 * 13 + 8 * 4 + 8 * 4 and len(_lib.SHAPE_RAW) == 13
    for name in ("gpirt_sampler_shape_enable", "gpirt_sampler_shape_accumulate", "gpirt_sampler_shape_get",
                 "gpirt_sampler_shape_state", "gpirt_shape_state_bytes", "gpirt_shape_combine", "gpirt_mcmc_run"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    # argument errors come back before any device is touched
    assert lib.gpirt_shape_combine(None, 1, None, None, C.byref(p)) == _lib.E_ARG
    assert lib.gpirt_sampler_shape_enable(None, 300, (C.c_double * 1)(0.0), 1, 1) == _lib.E_ARG
    assert lib.gpirt_sampler_shape_get(None, b"cls", None, 0) == _lib.E_ARG
    nb = C.c_int64()
    assert lib.gpirt_shape_state_bytes(1024, C.byref(nb)) == 0
    # four uint32 histograms and info_sum of 1001 x m, the small arrays and the header: about 24 MB at m = 1024
    m = 1024
    want = 16 * 8 + 4 * (16 * m + 4 * 1001 * m + 4 * m + 2 * m) + 8 * (4 * m + 1001 * m) + 2 * 8 * 1002 + 16
    assert nb.value == want and 24e6 < nb.value < 25e6
    assert lib.gpirt_shape_state_bytes(0, C.byref(nb)) == _lib.E_ARG
