"""PSIS-LOO on the host: gpirt_amd.loo.from_draws (the NumPy statement of include/gpirt_hip.h's "PSIS-LOO" section) and compare,
alone -- the tail rule, unsmoothed cells, the generalised Pareto fit on exact Pareto ratios, the bracket of elpd_loo, the model
comparison and the argument errors.  No device is needed."""
import math

import numpy as np
import pytest

from gpirt_amd import loo as LO


def _one_cell(keys, yv=1.0, **kw):
    """a 1 x 1 data set whose only cell sees `keys` (g = -y key)"""
    keys = np.asarray(keys, dtype=np.float64)
    return LO.from_draws(np.array([[yv]]), (-yv * keys)[:, None, None], **kw)


@pytest.mark.parametrize("T,M", [(3, 0), (24, 4), (25, 5), (26, 5), (2000, 135), (8000, 269)])
def test_tail_rule(T, M):
    assert LO.tail_length(T) == M
    if T <= 26:
        out = _one_cell(np.linspace(-1.0, 1.0, T))
        assert out["M"] == M and out["raw"]["tail"].shape[0] == M + 1


def test_constant_cell_is_unsmoothed():
    T = 100
    out = _one_cell(np.full(T, -1.25))
    r = 1.0 + math.exp(-1.25)
    assert out["unsmoothed"] == 1 and out["n_obs"] == 1 and np.isnan(out["pointwise"]["pareto_k"][0, 0])
    assert out["pointwise"]["elpd_loo"][0, 0] == pytest.approx(math.log(T) - math.log(T * r), rel=1e-14)
    assert out["pointwise"]["n_eff"][0, 0] == pytest.approx(T, rel=1e-13)


def test_short_tail_is_unsmoothed():
    rng = np.random.default_rng(3)
    keys = rng.normal(-1.0, 1.0, 24)                                   # M = 4 < 5
    out = _one_cell(keys)
    want = math.log(24) - math.log(float(np.sum(1.0 + np.exp(keys.astype(np.longdouble)))))
    assert out["M"] == 4 and out["unsmoothed"] == 1 and np.isnan(out["pointwise"]["pareto_k"][0, 0])
    assert out["pointwise"]["elpd_loo"][0, 0] == pytest.approx(want, rel=1e-14)


@pytest.mark.parametrize("k,seed", [(0.1, 11), (0.3, 12), (0.7, 13)])
def test_exact_pareto_ratios_recover_k(k, seed):
    """r = u^(-k), u uniform: the ratios' tail is exactly generalised Pareto with shape k.  Keys log(r - 1), T = 2000, 200 cells."""
    T, cells = 2000, 200
    u = np.random.default_rng(seed).uniform(size=(T, cells))
    keys = np.log(np.expm1(-k * np.log(u)))
    out = LO.from_draws(np.ones((cells, 1)), -keys[:, :, None])
    got = out["pointwise"]["pareto_k"]
    assert not np.isnan(got).any()
    print(f"MEASURED mean pareto_k at k = {k}: {got.mean():.4f}")
    assert abs(got.mean() - k) <= 0.08


def test_elpd_bracket_for_a_well_behaved_cell():
    T = 2000
    a = np.random.default_rng(21).normal(2.0, 0.5, T)                  # y g
    out = _one_cell(-a)
    pw = {k: v[0, 0] for k, v in out["pointwise"].items()}
    raw = math.log(T) - math.log(float(np.sum(1.0 + np.exp(-a.astype(np.longdouble)))))
    assert raw - 0.2 <= pw["elpd_loo"] <= pw["lppd"]
    assert pw["p_loo"] > 0 and 0.0 < pw["loo_p_yes"] < 1.0 and pw["n_eff"] <= T
    assert out["k_good"] == 1 and out["k_threshold"] == pytest.approx(min(1 - 1 / math.log10(T), 0.7))


def _two_models():
    rng = np.random.default_rng(5)
    y = np.where(rng.uniform(size=(6, 4)) < 0.5, 1.0, -1.0)
    y[1, 2] = np.nan
    return y, rng.normal(0.5, 1.0, (60, 6, 4)), rng.normal(0.2, 1.0, (60, 6, 4))


def test_compare_with_itself_and_another_model():
    y, ga, gb = _two_models()
    a, b = LO.from_draws(y, ga), LO.from_draws(y, gb)
    same = LO.compare(a, a)
    assert same["elpd_diff"] == 0.0 and same["se_diff"] == 0.0 and same["n_obs"] == 23
    ab = LO.compare(a, b)
    d = (a["pointwise"]["elpd_loo"] - b["pointwise"]["elpd_loo"])[~np.isnan(y)]
    assert ab["elpd_diff"] == pytest.approx(a["elpd_loo"] - b["elpd_loo"], rel=1e-12)
    assert ab["se_diff"] == pytest.approx(math.sqrt(23 * np.var(d, ddof=1)), rel=1e-12)
    assert LO.compare(a["pointwise"]["elpd_loo"], b["pointwise"]["elpd_loo"]) == ab


def test_compare_refuses_differing_masks():
    y, ga, gb = _two_models()
    y2 = y.copy()
    y2[0, 0] = np.nan
    with pytest.raises(ValueError, match="finished cells differ"):
        LO.compare(LO.from_draws(y, ga), LO.from_draws(y2, gb))


def test_totals_follow_from_the_pointwise_arrays():
    y, ga, _ = _two_models()
    ga[7, 2, 1] = np.nan                                              # one incomplete cell
    ga[9, 3, 3] = -710.0 * y[3, 3]                                    # and one whose key exceeds 700
    a = LO.from_draws(y, ga, top=5)
    e = a["pointwise"]["elpd_loo"]
    fin = ~np.isnan(e)
    assert a["cells_incomplete"] == 2 and a["n_obs"] == 21 and not fin[2, 1] and not fin[3, 3]
    assert a["raw"]["nonfinite"][2, 1] == 1 and a["raw"]["count"][3, 3] == 59
    assert a["elpd_loo"] == pytest.approx(e[fin].sum()) and a["looic"] == pytest.approx(-2 * a["elpd_loo"])
    assert a["se_looic"] == pytest.approx(2 * a["se_elpd_loo"])
    assert np.allclose(a["item_elpd_loo"], np.where(fin, e, 0).sum(axis=0))
    assert np.allclose(a["respondent_elpd_loo"], np.where(fin, e, 0).sum(axis=1))
    k = a["pointwise"]["pareto_k"]
    w = a["worst"]
    assert w["index"].shape == (5,) and (np.diff(w["pareto_k"]) <= 0).all()
    assert w["pareto_k"][0] == np.nanmax(k) and k[w["row"][0], w["col"][0]] == w["pareto_k"][0]
    assert a["k_good"] + a["k_bad"] + a["k_very_bad"] + a["unsmoothed"] == a["n_obs"]


def test_float64_statement_is_close_to_the_long_double_one():
    y, ga, _ = _two_models()
    a, b = LO.from_draws(y, ga), LO.from_draws(y, ga, dtype=np.float64)
    for name in ("pareto_k", "elpd_loo", "n_eff", "loo_p_yes"):
        assert np.allclose(a["pointwise"][name], b["pointwise"][name], rtol=1e-9, atol=1e-12, equal_nan=True), name


def test_argument_errors():
    y, ga, _ = _two_models()
    for bad in (4, 1025, 5.0, True):
        with pytest.raises(ValueError, match="tail must be"):
            LO.from_draws(y, ga, tail=bad)
    with pytest.raises(ValueError, match="more than the 60 planned draws"):
        LO.from_draws(y, ga, tail=60)
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError, match="top must be"):
            LO.from_draws(y, ga, top=bad)
    with pytest.raises(ValueError, match="more than GPIRT_LOO_MAX_TAIL"):
        LO.tail_length(200000)
    assert LO.tail_length(200000, tail=1024) == 1024
    with pytest.raises(ValueError, match="unknown keys"):
        LO.parse(dict(tails=7))
    with pytest.raises(ValueError, match="loo must be"):
        LO.parse(7)
    assert LO.parse(True) == dict(tail=None, top=20) and LO.parse(dict(tail=9, top=3)) == dict(tail=9, top=3)
    with pytest.raises(ValueError, match="S x n x m"):
        LO.from_draws(y, ga[:, :5])


def test_c_abi_of_version_117():
    import ctypes as C
    from gpirt_amd import _lib
    lib = _lib.load()
    assert lib.gpirt_version() >= 117
    for T, M in ((3, 0), (24, 4), (25, 5), (26, 5), (2000, 135), (8000, 269)):
        out = C.c_int64()
        assert lib.gpirt_loo_tail_length(T, 0, C.byref(out)) == 0 and out.value == M
    out = C.c_int64()
    assert lib.gpirt_loo_tail_length(200000, 0, C.byref(out)) != 0
    assert b"GPIRT_LOO_MAX_TAIL" in lib.gpirt_last_error()
    assert lib.gpirt_loo_tail_length(100, 4, C.byref(out)) != 0 and lib.gpirt_loo_tail_length(100, 100, C.byref(out)) != 0
    nb = C.c_int64()
    assert lib.gpirt_loo_state_bytes(100, 418, 269, C.byref(nb)) == 0
    assert abs(nb.value - 100 * 418 * (8 * 270 + 33)) < 4096          # (8 K + 32) bytes per cell, a byte of y, the header
