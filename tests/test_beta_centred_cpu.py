"""The centred beta update without a GPU (include/gpirt_hip.h "a centred beta update"; gpirt_amd.beta): the new C symbols, B of
the rank-64 form against the dense formula with the true kernel, the statement against the dense conditional, g = f + mu held
cell by cell, the non-vacuity conditions of the GPU test's bounds at every constructed shape, and the prior-invariance chain in
NumPy with its wrong variants.  tests/_beta_centred_bounds.py derives every bound."""
import ctypes as C
import os

import numpy as np
import pytest

import _beta_centred_bounds as BB

LD = np.longdouble
U = BB.U


def test_version_stage_and_symbols():
    from gpirt_amd import _lib
    lib = _lib.load()
    assert lib.gpirt_version() >= 136 and _lib.ST_BETA_CENTRED == 14
    for name in ("gpirt_sampler_draw_beta_centred", "gpirt_sampler_beta_centred_get", "gpirt_sampler_beta_centred_stats"):
        assert hasattr(lib, name), name
    assert C.sizeof(_lib.BetaCentred()) == 8 * (4 + 1 + 6)         # gpirt_beta_centred: four counters, one double, six reserved words
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "gpirt_hip.h")).read()
    assert "GPIRT_ST_BETA_CENTRED = 14" in header and "int gpirt_sampler_draw_beta_centred(gpirt_sampler_t s);" in header
    # every existing stage keeps its number
    assert (_lib.ST_AMP, _lib.ST_CARRY, _lib.ST_POP, _lib.ST_AMP_CENTRED, _lib.ST_ELL) == (10, 11, 12, 13, 9)


@pytest.fixture(scope="module")
def shared():
    """centred_shared and the dense triple per n, computed once"""
    from gpirt_amd import beta as Bt
    out = {}
    for n in BB.DENSE_NS:
        theta = BB.CB.case(n, 1)["theta"]
        out[n] = (theta, Bt.centred_shared(theta), Bt.dense_B(theta))
    return out


@pytest.mark.parametrize("n", BB.DENSE_NS)
def test_B_of_the_rank_64_form_against_the_dense_formula(shared, n):
    """thetas with both end points and a repeated value; B = X^T S^-1 X from Phi Phi^T + eps I in long double against the dense
    long-double Cholesky solve with the true squared-exponential kernel, within the exact perturbation bound"""
    theta, sh, dense = shared[n]
    assert theta[0] == -5.0 and theta[-1] == 5.0 and (n < 4 or theta[2] == theta[1])
    tol, nS = BB.dense_tolerance(theta, sh, dense)
    err = np.abs(sh["B"] - dense[0]).astype(np.float64)
    scale = np.sqrt(np.outer(np.diag(dense[0]), np.diag(dense[0])).astype(np.float64))
    print(f"MEASURED n={n}: B = {np.asarray(dense[0], dtype=np.float64).round(4).tolist()}, |dS|_F = {nS:.1e}, largest relative "
          f"difference {float((err / scale).max()):.1e}, used fraction of the bound {float((err / tol).max()):.1e}, cond(A) = {sh['cond']:.1e}")
    assert (err <= tol).all()
    assert (tol <= 1e-7 * scale).all()                              # not vacuous
    # W of the two routes agree as well: the same identity, column by column
    assert float(np.abs(sh["W"] - dense[1]).max()) <= 1e-6 * float(np.abs(dense[1]).max())


@pytest.mark.parametrize("amps", [None, "spread"])
def test_statement_against_the_dense_conditional(amps):
    """65 x 5: centred_exact_update's mean (from f and beta) and covariance (from its factor) against `conditional` from g = f + X
    beta by the dense formula with the true kernel.  The two differ by the rank identity's 1e-13 through cond(S) = 1e5: 1e-7
    relative to the conditional sd is the margin."""
    from gpirt_amd import beta as Bt
    c = BB.state(65, 5, amps)
    sh = Bt.centred_shared(c["theta"])
    z = np.zeros((2, 5))
    up = Bt.centred_exact_update(sh["W"].astype(np.float64), sh["B"], c["f"], c["beta"], c["a"], c["pm"], c["ps"], c["theta"], None, z)
    X = np.stack([np.ones(65), c["theta"]], axis=1)
    g = c["f"].astype(LD) + X.astype(LD) @ c["beta"].astype(LD)
    mean, cov = Bt.conditional(c["theta"], g, c["a"], c["pm"], c["ps"])
    sd = np.sqrt(np.array([np.diag(cov[j]) for j in range(5)], dtype=np.float64)).T
    # W rounded to fp64 above: (n + 2) u sum |W| |f| moves T, the rest is the identity's
    assert (np.abs(up["mean"] - mean).astype(np.float64) <= 1e-7 * sd).all()
    assert (np.abs(up["cov"] - cov).astype(np.float64) <= 1e-7 * np.abs(cov).astype(np.float64).max()).all()
    for j in range(5):                                              # the factor is the covariance's: C C^T = Lam = cov^-1
        c00, c10, c11 = up["chol"][:, j]
        Cm = np.array([[c00, 0], [c10, c11]], dtype=LD)
        assert float(np.abs(Cm @ Cm.T @ up["cov"][j] - np.eye(2)).max()) <= 1e-15
    assert up["status"] == ["updated"] * 5
    # beta' = mean + C^-T z: the unit normals give the columns of C^-T
    up1 = Bt.centred_exact_update(sh["W"].astype(np.float64), sh["B"], c["f"], c["beta"], c["a"], c["pm"], c["ps"], c["theta"], None,
                                  np.stack([np.ones(5), np.zeros(5)]))
    assert (np.abs((up1["beta"] - up1["mean"])[0] - 1 / up["chol"][0]) <= 1e-17).all() and not (up1["beta"] - up1["mean"])[1].any()


_CASES = {}


def _case(n, m, amps):
    """the constructed state, the statement's shared part, W and B in fp64 by the device's formulas and one update from them:
    computed once per shape"""
    from gpirt_amd import beta as Bt
    key = (n, m, amps)
    if key not in _CASES:
        c = BB.state(n, m, amps)
        sh = Bt.centred_shared(c["theta"])
        dev = BB.shared_fp64(c["theta"])
        z = Bt.centred_normals(BB.SEED, 1, np.arange(m))
        up = Bt.centred_exact_update(dev["W"], dev["B"], c["f"], c["beta"], c["a"], c["pm"], c["ps"], c["theta"], None, z)
        dg = np.abs((up["f"].astype(LD) + up["mu"].astype(LD)) - (c["f"].astype(LD) + c["mu"].astype(LD))).astype(np.float64)
        _CASES[key] = (c, sh, dev, z, up, dg)
    return _CASES[key]


SHAPES = [(n, m, amps) for n in BB.NS for m in BB.MS for amps in (None, "spread")]


@pytest.mark.parametrize("n,m,amps", SHAPES)
def test_the_bounds_are_not_vacuous_and_the_likelihood_is_held(n, m, amps):
    """Every constructed shape of the GPU test, with W and B formed in fp64 by the device's formulas: the a-posteriori bound on W
    at most 1e-3 of the column's 2-norm, the bounds on mean and chol given W at most 1e-9 of the conditional sd, the
    likelihood's change within the summed cell bound."""
    c, sh, dev, z, up, dg = _case(n, m, amps)
    e_W = BB.w_bound(sh, dev["W"], c["theta"])
    wn = np.linalg.norm(dev["W"], axis=0)
    err_W = np.linalg.norm((dev["W"] - sh["W"]).astype(np.float64), axis=0)
    e_B = BB.b_bound(dev["W"], c["theta"], e_W)
    err_B = np.abs(dev["B"] - sh["B"]).astype(np.float64)
    ub = BB.update_bounds(up, dev["B"], c["beta"], c["a"], c["pm"], c["ps"], z, BB.t_bound(dev["W"], c["f"]))
    gb = BB.g_cell_bound(c["f"], c["mu"], up["mu"])
    g0, g1 = c["f"].astype(LD) + c["mu"].astype(LD), up["f"].astype(LD) + up["mu"].astype(LD)
    dll = np.abs(BB.loglik(g1, c["y"]) - BB.loglik(g0, c["y"])).astype(np.float64)
    print(f"MEASURED n={n} m={m} amps={amps}: W used {float((err_W / e_W).max()):.1e} of a bound of {float((e_W / wn).max()):.1e} of |W|, "
          f"B used {float((err_B / e_B).max()):.1e}; mean bound / sd {float((ub['mean'] / ub['sd']).max()):.1e}, chol bound / sd "
          f"{float((ub['chol'] / ub['sd'].min(axis=0)[None, :]).max()):.1e}; g' - g used {float((dg / gb).max()):.2f}")
    assert up["status"] == ["updated"] * m
    assert (err_W <= e_W).all() and (err_B <= e_B).all()
    assert (e_W <= 1e-3 * wn).all()
    assert (ub["mean"] <= 1e-9 * ub["sd"]).all() and (ub["chol"] <= 1e-9 * ub["sd"].min(axis=0)[None, :]).all()
    assert (dg <= gb).all()
    obs = ~np.isnan(c["y"])
    assert (dll <= np.where(obs, gb, 0.0).sum(axis=0)).all()


@pytest.mark.parametrize("n,m,amps", SHAPES)
def test_g_is_held_cell_by_cell(n, m, amps):
    """g' - g within 4 u (|f| + |mu| + |mu'|) in every cell, g = f + mu as stored.  The rewrite forms the shift as the difference
    of the two rounded means, so the difference is at most u |mu - mu'| + u |f'|, also where beta0 and theta beta1 cancel
    (n = 257, m = 5 has such cells: with the shift formed as d0 + theta d1 one of them reached 2.99 of the bound)."""
    c, sh, dev, z, up, dg = _case(n, m, amps)
    gb = BB.g_cell_bound(c["f"], c["mu"], up["mu"])
    print(f"MEASURED n={n} m={m} amps={amps}: g' - g used {float((dg / gb).max()):.2f} of 4 u (|f| + |mu| + |mu'|), "
          f"{int((dg > gb).sum())} of {dg.size} cells above it")
    assert (dg <= gb).all()


def test_a_nan_in_f_fails_the_item_and_leaves_its_column():
    from gpirt_amd import beta as Bt
    c = BB.state(65, 5, None)
    f = c["f"].copy(order="F")
    f[7, 2] = np.nan
    dev = BB.shared_fp64(c["theta"])
    up = Bt.centred_exact_update(dev["W"], dev["B"], f, c["beta"], None, c["pm"], c["ps"], c["theta"], None, np.zeros((2, 5)))
    assert up["status"] == ["updated", "updated", "failed", "updated", "updated"]
    assert up["f"][:, 2].tobytes() == f[:, 2].tobytes() and np.isnan(up["mu"][:, 2]).all()


def test_prior_invariance_in_numpy_and_its_wrong_variants():
    """The GPU test's configuration in NumPy: the correct move keeps all 36 |z| within 5; without a_j^2, with f not moved and
    with the f-shift reversed the largest |z| leaves it."""
    worst = {}
    for variant in ("ok", "no_a2", "f_fixed", "reversed"):
        kb, ku = BB.pi_chain_numpy(3, variant)
        assert kb.shape == ku.shape == ((BB.PI_ROUNDS - BB.PI_BURN) // BB.PI_THIN, 2, BB.PI_M)
        z = BB.pi_zscores(kb, ku)
        assert z.shape == (36,)
        worst[variant] = float(np.abs(z).max())
        if variant == "f_fixed":                                    # the beta marginals cannot see it: the correlations do
            assert np.abs(z[:16]).max() <= BB.PI_SDS and np.abs(z[32:]).max() > BB.PI_SDS
    print(f"MEASURED prior invariance in NumPy, largest |z|: {({k: round(v, 2) for k, v in worst.items()})}")
    assert worst["ok"] <= BB.PI_SDS
    assert min(worst["no_a2"], worst["f_fixed"], worst["reversed"]) > BB.PI_SDS


def test_summarise_and_geyer():
    """an AR(1) series with phi = 0.9 has tau = 19: Geyer's ESS of 4000 draws lies near 210; white noise near N"""
    from gpirt_amd import beta as Bt
    rng = np.random.default_rng(5)
    e = rng.standard_normal((2, 4000, 2, 3))
    x = e.copy()
    for t in range(1, 4000):
        x[:, t, 1] = 0.9 * x[:, t - 1, 1] + e[:, t, 1]
    d = Bt.summarise(x)
    assert d["rhat"].shape == d["ess"].shape == (2, 3)
    assert (d["ess"][0] > 6000).all() and (d["ess"][1] > 200).all() and (d["ess"][1] < 900).all() and (d["rhat"] < 1.05).all()
