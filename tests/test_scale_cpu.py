"""The collapsed scale and shift move without a GPU (include/gpirt_hip.h "a collapsed scale and shift move"; gpirt_amd.scale): the
new C symbols and the stage id, the statement against a dense long-double restatement, prior invariance in NumPy with its wrong
variants, the collapsed target against quadrature, and the decision margin of every case the GPU test constructs.
tests/_scale_bounds.py derives every bound."""
import ctypes as C
import os

import numpy as np
import pytest

import _scale_bounds as SB

LD = np.longdouble


def test_version_stage_and_symbols():
    from gpirt_amd import _lib
    lib = _lib.load()
    assert lib.gpirt_version() >= 137 and _lib.ST_SCALE == 15
    for name in ("gpirt_sampler_scale_enable", "gpirt_sampler_draw_scale", "gpirt_sampler_scale_width", "gpirt_sampler_scale_get",
                 "gpirt_sampler_scale_stats", "gpirt_sampler_step_consistent_scale"):
        assert hasattr(lib, name), name
    assert C.sizeof(_lib.Scale()) == 8 * (1 + 6 + 4 + 5)            # gpirt_scale: on, 3 x 2 counters, 2 x 2 doubles, five reserved words
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "gpirt_hip.h")).read()
    assert "GPIRT_ST_SCALE = 15" in header and "int gpirt_sampler_draw_scale(gpirt_sampler_t s, int kind);" in header
    assert "#define GPIRT_SCALE_RECORD 16" in header and len(_lib.SCALE_RECORD) == 16
    # every existing stage keeps its number
    assert (_lib.ST_AMP, _lib.ST_CARRY, _lib.ST_POP, _lib.ST_AMP_CENTRED, _lib.ST_BETA_CENTRED, _lib.ST_ELL) == (10, 11, 12, 13, 14, 9)


def _dense_lz(y, lprior, curve):
    """lz of every respondent, cell by cell in long double with Python loops: nothing shared with gpirt_amd.scale but the inputs"""
    N, m = curve.shape
    res = []
    for i in range(y.shape[0]):
        P = []
        for k in range(1, N):
            ll = LD(0)
            for j in range(m):
                if y[i, j] == y[i, j]:
                    ll -= np.log1p(np.exp(-LD(y[i, j]) * LD(curve[k, j])))
            P.append(LD(lprior[i][k]) + ll)
        M = max(P)
        res.append(M + np.log(sum(np.exp(p - M) for p in P)))
    return np.array(res, dtype=LD)


@pytest.mark.parametrize("kind", ["scale", "shift"])
def test_statement_against_a_dense_restatement(kind):
    """3 respondents x 2 items on a 9-point stretch of the grid: proposal, loglik_grid, log_normalisers (both orders) and
    step_exact against loops in long double over every cell"""
    from gpirt_amd import scale as SC
    rng = np.random.default_rng(4)
    n, m, N = 3, 2, 9
    y = np.array([[1.0, -1.0], [np.nan, 1.0], [-1.0, -1.0]])
    beta = np.array([[0.3, -0.4], [1.1, 0.7]])
    pm, ps = np.array([[0.2, 0.1], [1.0, 0.9]]), np.array([[1.5, 1.2], [0.8, 0.6]])
    z, u = SC.normals(11, 3, kind)
    pr = SC.proposal(beta, kind, 0.4, z)
    step = 0.4 * z
    if kind == "scale":
        want = np.array([beta[0], beta[1] * np.exp(-step)])
        assert pr["jacobian"] == -(2.0 * step)
    else:
        want = np.array([beta[0] + beta[1] * step, beta[1]])
        assert pr["jacobian"] == 0.0
    assert pr["step"] == step and np.array_equal(pr["beta"], want)
    assert pr["mu"].tobytes() == np.asfortranarray(want[0][None, :] + SC.GRID[:, None] * want[1][None, :]).tobytes()
    # a short grid for the loops: the statement's functions take any N
    x = SC.GRID[500:500 + N]
    hstar = 0.3 * rng.standard_normal((N, m))
    f1 = hstar + (beta[0][None, :] + x[:, None] * beta[1][None, :])
    f2 = hstar + (want[0][None, :] + x[:, None] * want[1][None, :])
    lprior = rng.standard_normal((n, N))
    lz, lzp = _dense_lz(y, lprior, f1), _dense_lz(y, lprior, f2)
    lp1, lp2 = SC.loglik_grid(y, f1), SC.loglik_grid(y, f2)
    ex = SC.step_exact(lp1, lp2, beta, want, pm, ps, kind, step, u, lprior=lprior)
    assert float(np.abs(ex["lz"] - lz).max()) <= 1e-17 and float(np.abs(ex["lz_prop"] - lzp).max()) <= 1e-17
    dev = SC.log_normalisers(lp1.astype(np.float64), lprior, order="device")
    assert float(np.abs(dev - lz).max()) <= 40 * SB.U * float(np.abs(lz).max() + 10)
    q = 1 if kind == "scale" else 0
    Q = LD(0)
    for j in range(m):
        for b, sign in ((want[q, j], 1), (beta[q, j], -1)):
            zz = abs((LD(b) - LD(pm[q, j])) / LD(ps[q, j]))
            Q += sign * -(LD(SC.LN_SQRT_2PI) + LD(0.5) * zz * zz + np.log(LD(ps[q, j])))
    log_r = (lzp - lz).sum() + Q - (LD(m) * LD(step) if kind == "scale" else 0)
    assert abs(float(ex["Q"] - Q)) <= 1e-17 and abs(float(ex["log_r"] - log_r)) <= 1e-16
    assert ex["status"] == ("accepted" if np.log(LD(u)) < log_r else "rejected")
    # index 0 is left out: a huge mass there changes nothing
    lp1b = lp1.copy()
    lp1b[0] += 50
    assert np.array_equal(SC.log_normalisers(lp1b, lprior), ex["lz"])
    # a NaN column or a degenerate one is a failed call
    bad = lp2.copy()
    bad[3, 1] = np.nan
    assert SC.step_exact(lp1, bad, beta, want, pm, ps, kind, step, u, lprior=lprior)["status"] == "failed"
    assert SC.step_exact(lp1, np.full_like(lp2, -1e301), beta, want, pm, ps, kind, step, u, lprior=lprior)["status"] == "failed"


def test_normals_are_the_stage_s_own():
    from gpirt_amd import _lib, scale as SC
    from gpirt_amd.ppc import item_uniform
    z0, u0 = SC.normals(9, 1, "scale")
    z1, u1 = SC.normals(9, 1, "shift")
    assert u0 == float(item_uniform(9, 1, _lib.ST_SCALE, np.uint64(0), np.uint64(1))) and u1 == float(item_uniform(9, 1, 15, np.uint64(1), np.uint64(1)))
    assert z0 != z1 and SC.normals(9, 2, "scale")[0] != z0 and SC.normals(9, 1, 0) == (z0, u0)
    with pytest.raises(ValueError, match="scale"):
        SC.normals(9, 1, "tilt")


def test_prior_invariance_in_numpy_and_its_wrong_variants():
    """every answer missing, 64 items, priors off centre (means (0.5, 1.0), sds (0.5, 0.15)), both kinds alternating: 300 replicates
    of 40 calls from fresh prior draws.  The five z-scores of beta's moments lie within 5; without -m eps, and with the shift's
    sign reversed in the state but not in the ratio, they do not."""
    pm, ps = SB.pi_priors()
    got = {}
    for variant in ("right", "no_jacobian", "shift_reversed"):
        finals, rate = SB.pi_chain(variant)
        z = SB.pi_zscores(finals, pm, ps)
        got[variant] = float(np.abs(z).max())
        print(f"MEASURED prior invariance ({variant}): z = {np.round(z, 2).tolist()}, largest |z| / 5 = {got[variant] / SB.PI_SDS:.2f}, accepted {rate:.2f}")
    assert got["right"] <= SB.PI_SDS
    assert got["no_jacobian"] > SB.PI_SDS and got["shift_reversed"] > SB.PI_SDS


@pytest.mark.parametrize("kind", ["scale", "shift"])
def test_the_collapsed_target_against_quadrature(kind):
    """one fixed hstar and y (n = 40, m = 4), 20 000 moves of the kind on the statement: the accumulated step's mean and variance
    against 1-d quadrature of collapsed_density, within 5 MCSE (batch means)"""
    xs, rate = SB.ct_chain(kind)
    mean, var, edge = SB.ct_quadrature(kind)
    se_m, se_v = SB.mcse(xs)
    print(f"MEASURED collapsed target ({kind}): chain mean {xs.mean():.4f} var {xs.var():.4f}, quadrature mean {mean:.4f} var {var:.4f}, "
          f"MCSE {se_m:.4f} {se_v:.4f}, accepted {rate:.2f}, quadrature's edge mass {edge:.1e}")
    assert edge < 1e-8 and 0.1 < rate < 0.9
    assert abs(xs.mean() - mean) <= 5 * se_m and abs(xs.var() - var) <= 5 * se_v
    assert se_m < 0.1 * np.sqrt(var)                                # not vacuous: the chain resolves the target's width


@pytest.mark.parametrize("pop", [False, True])
@pytest.mark.parametrize("m", SB.MS)
@pytest.mark.parametrize("n", SB.NS)
def test_the_decision_margin_of_every_constructed_case(n, m, pop):
    """|log u - log r| >= 100 x the derived bound on the device's log r and log u, for both kinds of every case the GPU test
    constructs, with room for this evaluation's own fp64 logposts (2 m + 2 roundings of sums of order |logpost| per cell)"""
    for kind in ("scale", "shift"):
        c, pr, ex, bd, u = SB.case_on_cpu(n, m, kind, pop)
        margin = abs(float(ex["log_u"] - ex["log_r"]))
        need = SB.MARGIN * (bd["log_r"] + bd["log_u"])
        own = 2.0 * n * (2 * m + 2) * SB.U * float(np.abs(SB.loglik_grid64(c["y"], c["fstar"])[1:]).max())
        print(f"MEASURED n={n} m={m} pop={pop} {kind}: log r {float(ex['log_r']):+.4f}, log u {float(ex['log_u']):+.4f}, margin {margin:.3e}, "
              f"100 x bound {need:.3e}, this evaluation's own error {own:.1e}, {ex['status']}")
        assert ex["status"] in ("accepted", "rejected")
        assert margin >= need + own
        assert need < 1e-6                                          # not vacuous
