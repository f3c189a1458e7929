"""Ordinal responses on the host (gpirt_amd/ordinal.py, gpirt_ordinal_check, gpirt_ordinal_grid): no GPU.

The NumPy statement of the model, the invariance of the window move from its exact transition matrix, the start values, every
argument refusal with its message, the export list -- and the condition on the inputs of tests/test_gpu_ordinal.py: under the
derived bounds (tests/_ordinal_bounds.py) the constructed slice cases leave no decision of the long-double statement undecided
when nu is a stand-in drawn on the host."""
import numpy as np
import pytest

import _ordinal_bounds as OB

LD = np.longdouble


@pytest.fixture(scope="module")
def OR():
    from gpirt_amd import _lib, build
    import os
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    from gpirt_amd import ordinal
    return ordinal


def test_version_stage_and_exports(OR):
    from gpirt_amd import _lib
    from gpirt_amd.sampler import Sampler
    lib = _lib.load()
    assert lib.gpirt_version() >= 139 and _lib.ST_ORD == 16
    for name in ("gpirt_ordinal_check", "gpirt_ordinal_grid", "gpirt_sampler_ordinal_enable", "gpirt_sampler_draw_thresholds",
                 "gpirt_sampler_ordinal_width", "gpirt_sampler_ordinal_record", "gpirt_sampler_ordinal_accumulate_irf",
                 "gpirt_sampler_ordinal_get", "gpirt_sampler_ordinal_stats"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for name in ("ordinal_enable", "draw_thresholds", "ordinal_width", "ordinal_record", "ordinal_accumulate_irf", "ordinal_get",
                 "ordinal_stats", "ordinal"):
        assert callable(getattr(Sampler, name)), name
    for name in ("dichotomise", "grid", "init_thresholds", "check_args", "run", "summarise", "curves", "loglik", "slice_exact",
                 "theta_logpost_exact", "beta_exact", "threshold_conditional", "thresholds_exact"):
        assert callable(getattr(OR, name)) and name in OR.__all__, name


def test_grid_is_symmetric_with_exact_ends(OR):
    for hi, P in ((6.0, 241), (6.0, 9), (20.0, 1001), (0.7, 21)):
        t = OR.grid(hi, P)
        assert t[0] == -hi and t[-1] == hi and t[(P - 1) // 2] == 0.0
        assert np.array_equal(t, -t[::-1]) and np.all(np.diff(t) > 0)
        want = (np.arange(P, dtype=LD) * 2 - (P - 1)) / LD(P - 1) * LD(hi)
        assert np.array_equal(t, want.astype(np.float64))
    assert np.array_equal(OR.default_log_prior(OR.grid()), -(OR.grid() * OR.grid()) / 18.0)


@pytest.mark.parametrize("C", [2, 3, 5, 8])
def test_category_probabilities_sum_to_one(OR, C):
    rng = np.random.default_rng(C)
    g = np.concatenate([np.linspace(-12.0, 12.0, 97), [-45.0, 45.0, 705.0, -712.0]])
    for _ in range(20):
        b = np.sort(rng.uniform(-4.0, 4.0, C - 1))
        lp = OR.category_logprobs(g, b, LD)
        assert np.all(lp <= 0)
        assert np.abs(np.exp(lp).sum(axis=0) - 1).max() <= 8 * np.finfo(LD).eps
        # the float64 form (as written: it loses e^-a beyond a = 37 and overflows beyond 709, as the reference's term does)
        ok = np.abs(g) < 30
        assert np.abs(np.exp(OR.category_logprobs(g[ok], b, np.float64)).sum(axis=0) - 1).max() <= 16 * 2.0 ** -53 * C


def test_two_categories_at_zero_are_the_binary_ll_bar_bit_for_bit(OR):
    from oracle import np_oracle as NP
    rng = np.random.default_rng(5)
    n = 257
    f, mu = rng.standard_normal(n) * 2, rng.standard_normal(n)
    f[3], f[4], mu[5] = 41.0, -39.5, 0.0
    cat = rng.integers(0, 3, n)
    y = np.where(cat == 0, np.nan, np.where(cat == 2, 1.0, -1.0))
    cell = OR.loglik(cat, f + mu, [0.0])
    ok = cat > 0
    assert np.array_equal(cell[ok], -np.log(1 + np.exp(-(y[ok] * (f + mu)[ok]))))
    assert np.all(cell[~ok] == 0)
    assert float(np.sum(cell[ok])) == NP.ll_bar(f, y, mu)
    # and the long-double form agrees with it to float64's rounding of the as-written term
    # (1 + e^-a rounds by at most 2^-53 absolute, exp and log by an ulp of their results)
    assert np.all(np.abs(OR.loglik(cat, f + mu, [0.0], dtype=LD) - cell) <= 2.0 ** -52 * (1 + np.abs(cell)))


def _toy(OR):
    rng = np.random.default_rng(12)
    cat = np.array([1, 2, 3, 3, 2, 1, 0, 2, 3, 1, 2, 2])
    g = rng.standard_normal(12) * 1.5
    t = OR.grid(6.0, 21)
    return cat, g, t, OR.default_log_prior(t)


@pytest.mark.parametrize("K,c", [([8, 14], 1), ([8, 14], 2), ([9, 11], 1), ([2, 14], 1), ([5, 19], 2), ([0, 20], 1), ([0, 20], 2)],
                         ids=["interior-1", "interior-2", "neighbour-in-window", "left-end", "right-end", "grid-end-1", "grid-end-2"])
def test_window_move_leaves_the_conditional_invariant(OR, K, c):
    """n = 12, C = 3, P = 21, W = 4: the exact transition matrix of one threshold's update, a sum over the W placements of the
    window, has the full conditional on the allowed indices as a left fixed point -- at interior states, with the other
    threshold inside the window, and with the window cut by the grid's ends."""
    cat, g, t, pr = _toy(OR)
    allowed, T, pi = OR.transition_matrix(cat, g, t, pr, K, c, 4)
    left = K[c - 2] if c == 2 else -1
    right = K[c] if c == 1 else 21
    assert np.array_equal(allowed, np.arange(left + 1, right))
    assert np.abs(T.sum(axis=1) - 1).max() < 1e-15
    assert np.abs(pi @ T - pi).max() <= 1e-14
    # detailed balance too: every placement is a Gibbs step on a set that does not depend on the current point
    F = pi[:, None] * T
    assert np.abs(F - F.T).max() <= 1e-14
    # and pi is the model's conditional: loglik with the w term, plus the prior, up to a constant
    full = []
    for q in allowed:
        KK = list(K)
        KK[c - 1] = int(q)
        full.append(OR.loglik(cat, g, t[KK], True, LD).sum() + LD(pr[q]))
    full = np.array(full, dtype=LD)
    want = np.exp(full - full.max())
    assert np.abs(want / want.sum() - pi).max() <= 1e-14


def test_single_candidate_and_non_finite_masses(OR):
    cat, g, t, pr = _toy(OR)
    row = OR.threshold_conditional(cat, g, t, pr, [9, 10], 1, 7, 4)          # candidates 7 .. 9
    assert np.isneginf(row[3]) and np.all(np.isfinite(row[:3]))
    row = OR.threshold_conditional(cat, g, t, pr, [9, 10], 2, 8, 4)          # candidates 10, 11: right of the neighbour at 9
    assert np.isneginf(row[0]) and np.isneginf(row[1]) and np.all(np.isfinite(row[2:]))
    row = OR.threshold_conditional(cat, g, t, pr, [9, 10], 1, 9, 4)          # 9 alone: the neighbour at 10 cuts the window
    assert row[0] == 0 and np.all(np.isneginf(row[1:]))
    gn = g.copy()
    gn[0] = np.nan                                                             # an observed row of category 1
    assert OR.grid_draw(OR.threshold_conditional(cat, gn, t, pr, [8, 14], 1, 6, 4), 0.5)["failed"]
    res = OR.thresholds_exact(cat[:, None], gn[:, None], t, pr, [[8, 14]], 3, 1, 4)
    assert res["failed"] == 1 and res["updates"] == 0 and np.array_equal(res["index"], [[8, 14]])


def test_init_thresholds_and_dichotomise(OR):
    cat, t, _ = OB.make_case(257, 5, 5, 3)
    K = OR.init_thresholds(cat, t, 5)
    assert K.shape == (5, 4) and K.dtype == np.int32
    assert np.all(np.diff(K, axis=1) > 0) and K.min() >= 0 and K.max() <= 240     # item 0 has four empty categories, item 4 one
    tiny = OR.init_thresholds(cat, OR.grid(6.0, 9), 5)
    assert np.all(np.diff(tiny, axis=1) > 0) and tiny.min() >= 0 and tiny.max() <= 8
    full = OR.init_thresholds(np.full((10, 1), 8, dtype=np.int8), OR.grid(6.0, 9), 8)    # 7 thresholds on 9 points, one category
    assert np.all(np.diff(full, axis=1) > 0) and full.min() >= 0 and full.max() <= 8
    y = OR.dichotomise(cat)
    assert np.array_equal(np.isnan(y), cat == 0) and set(np.unique(y[~np.isnan(y)])) <= {-1.0, 1.0}
    j = 2
    srt = np.sort(cat[cat[:, j] > 0, j])
    assert np.array_equal(y[:, j] == 1.0, cat[:, j] > srt[(srt.size - 1) // 2])


def test_check_args_names_every_refusal(OR):
    from gpirt_amd import _lib
    from gpirt_amd._lib import GpirtError
    cat, t, K = OB.make_case(40, 3, 4, 1)
    y = OR.dichotomise(cat)
    OR.check_args(cat, y, 4, 6.0, 241, OR.default_log_prior(t), K, 16, options=_lib.fast_options())

    def refused(match, **kw):
        args = dict(cat=cat, y=y, C=4, hi=6.0, points=241, log_prior=None, K0=K, width=16)
        args.update(kw)
        with pytest.raises(GpirtError, match=match):
            OR.check_args(**args)
    refused("C = 1 categories, it must lie in 2 .. 8", C=1, K0=None)
    refused("C = 9 categories, it must lie in 2 .. 8", C=9, K0=None)
    bad = cat.copy(); bad[3, 1] = 5
    refused(r"cat\[3, 1\] = 5, it must lie in 0 .. C = 4", cat=bad)
    bad = cat.copy(); bad[3, 1] = -1
    refused(r"cat\[3, 1\] = -1, it must lie in 0 .. C = 4", cat=bad)
    yb = y.copy(); yb[np.argmax(cat[:, 2] == 0), 2] = 1.0
    refused("must be NaN exactly where cat is 0", y=yb)
    yb = y.copy(); yb[np.argmax(cat[:, 2] > 0), 2] = np.nan
    refused("must be NaN exactly where cat is 0", y=yb)
    refused("P = 240 grid points, it must be odd", points=240, K0=None)
    refused("P = 7 grid points", points=7, K0=None)
    refused("P = 1003 grid points", points=1003, K0=None)
    for hi in (0.0, -1.0, 20.5, np.inf, np.nan):
        refused(r"hi = .*, it must lie in \(0, 20\]", hi=hi)
    lp = OR.default_log_prior(t); lp[17] = -np.inf
    refused(r"log_prior\[17\] is not finite", log_prior=lp)
    Kb = K.copy(); Kb[1, 2] = Kb[1, 1]
    refused(r"K0\[1, .\] is not strictly increasing at c = 3", K0=Kb)
    Kb = K.copy(); Kb[2, 2] = 241
    refused(r"K0\[2, 3\] = 241 is off the grid", K0=Kb)
    Kb = K.copy(); Kb[0, 0] = -1
    refused(r"K0\[0, 1\] = -1 is off the grid", K0=Kb)
    refused("window width W = 0, it must lie in 1 .. 64", width=0)
    refused("window width W = 65, it must lie in 1 .. 64", width=65)
    o = _lib.default_options()                      # the C default is the R-stream replay
    assert o.rng_kind == _lib.RNG_RSTREAM
    refused("rng = reference .* R's stream has no such draw", options=o)
    o = _lib.fast_options(); o.item0 = 3
    refused("an item shard .* is refused", options=o)
    with pytest.raises(GpirtError, match="n = 16385 respondents is refused"):
        OR.check_args(np.ones((16385, 1), dtype=np.int8), None, 2)


def test_curves_and_summarise(OR):
    rng = np.random.default_rng(2)
    ex = np.sort(rng.random((3, 4, 1001)), axis=1)[:, ::-1] * 7           # 7 draws, decreasing in c
    out = OR.curves(ex, 7)
    assert out["probs"].shape == (3, 5, 1001) and np.abs(out["probs"].sum(axis=1) - 1).max() < 1e-14 and out["probs"].min() >= 0
    assert np.allclose(out["expected"], 1 + out["exceed"].sum(axis=1))
    d = rng.integers(0, 241, (2, 50, 3, 4))
    s = OR.summarise(d, OR.grid())
    assert s["mean"].shape == (3, 4) and s["quantiles"].shape == (5, 3, 4)
    assert np.allclose(s["mean"], OR.grid()[d].reshape(-1, 3, 4).mean(axis=0))


@pytest.mark.parametrize("C,seed", [(3, 31), (5, 32), (8, 33)])
def test_constructed_slice_cases_are_decided_in_long_double(OR, C, seed):
    """The inputs of the GPU slice test with a host stand-in for nu: no decision of the long-double statement lies inside the
    derived band (the cap there is 1 in 100)."""
    from gpirt_amd.ppc import item_uniform
    n = 257
    case = OB.slice_case(n, 3, C, seed)
    rng = np.random.default_rng(seed)
    total = undecided = 0
    for j in range(3):
        nu = rng.standard_normal(n)
        u = np.asarray(item_uniform(9, 1, 4, np.uint64(j), np.arange(200, dtype=np.uint64)))
        b = case["t"][case["K"][j]]
        res = OR.slice_exact(case["cat"][:, j], case["f"][:, j], nu, case["mu"][:, j], b, u)
        for eps, mg in zip(res["eps"], res["margins"]):
            band = OB.slice_bound(case["cat"][:, j], case["f"][:, j], nu, case["mu"][:, j], b, eps, res["ll0"], np.log(u[0]))
            total += 1
            undecided += int(abs(float(mg)) <= band)
        assert res["margins"][-1] > 0
    assert total >= 3 and undecided * 100 <= total
