"""The consistent step without a GPU (gpirt_amd/consistent.py): carry_exact's contract, and the effect itself on a NumPy
mini-chain built from oracle/np_oracle.py's stage functions -- the prior quadratic form Q = mean_j f_j^T S(theta)^-1 f_j / n,
which a prior-consistent state holds near 1, under the reference's step, under the carry, and under the carry without the nugget.
"""
import numpy as np
import pytest

N, M, ITERS, FROM = 120, 8, 25, 6


def _grid(k):
    return -5.0 + np.asarray(k, dtype=np.float64) * 0.01


def test_library_version_and_stage_id():
    from gpirt_amd import _lib
    lib = _lib.load()
    assert lib.gpirt_version() >= 133 and _lib.ST_CARRY == 11
    assert {"gpirt_sampler_carry_f", "gpirt_sampler_step_consistent", "gpirt_sampler_carry_stats",
            "gpirt_sampler_prior_quad"} <= set(_lib.SIGNATURES)


# ------------------------------------------------------------------------------------------------ 1. carry_exact ---
@pytest.fixture(scope="module")
def state():
    rng = np.random.default_rng(11)
    n, m = 23, 5
    k = rng.integers(0, 1001, n)
    k[:6] = (0, 1000, 417, 417, 417, 3)                 # both grid ends, three respondents on one grid point
    theta = _grid(k)
    theta[7] = np.nan
    theta[8] = 0.123456                                 # off the grid
    theta[9] = 5.01                                     # past its end
    theta[10] = np.nextafter(theta[10], 9.0)            # one ulp beside a grid point
    return dict(n=n, m=m, k=k, theta=theta, off=np.array([7, 8, 9, 10]), fstar=rng.normal(size=(1001, m)),
                mu_star=rng.normal(size=(1001, m)), f=rng.normal(size=(n, m)), z=rng.normal(size=(n, m)))


def test_carry_exact_rows(state):
    from gpirt_amd import consistent as CS
    s = state
    on = np.setdiff1d(np.arange(s["n"]), s["off"])
    for nugget in (False, True):
        out = CS.carry_exact(s["theta"], s["fstar"], s["mu_star"], s["f"], s["z"], nugget=nugget)
        assert out is not s["f"] and out.dtype == np.float64 and out.shape == s["f"].shape
        # off-grid and NaN rows keep their f byte for byte
        assert out[s["off"]].tobytes() == s["f"][s["off"]].tobytes()
        g = s["fstar"][s["k"][on]] - s["mu_star"][s["k"][on]]
        if not nugget:
            assert out[on].tobytes() == g.tobytes()
        else:
            assert out[on].tobytes() == (g + (np.ones(s["m"]) * CS.SQRT_JITTER)[None, :] * s["z"][on]).tobytes()
    # z is not read without the nugget
    assert CS.carry_exact(s["theta"], s["fstar"], s["mu_star"], s["f"], None, nugget=False).tobytes() == \
        CS.carry_exact(s["theta"], s["fstar"], s["mu_star"], s["f"], s["z"], nugget=False).tobytes()
    assert CS.counters_exact(s["theta"], s["fstar"]) == dict(off_grid=4, nonfinite=0)
    bad = s["fstar"].copy()
    bad[417, 2] = np.inf                                # three respondents sit on grid point 417
    assert CS.counters_exact(s["theta"], bad) == dict(off_grid=4, nonfinite=3)


def test_carry_exact_amplitudes_and_duplicates(state):
    from gpirt_amd import consistent as CS
    s = state
    args = (s["theta"], s["fstar"], s["mu_star"], s["f"], s["z"])
    none = CS.carry_exact(*args, amp=None)
    assert CS.carry_exact(*args, amp=np.ones(s["m"])).tobytes() == none.tobytes()
    assert CS.carry_exact(*args, amp=1.0).tobytes() == none.tobytes()
    amp = np.array([0.5, 2.0, 1.0, 3.25, 0.01])
    got = CS.carry_exact(*args, amp=amp)
    smooth = CS.carry_exact(*args, nugget=False)
    on = np.setdiff1d(np.arange(s["n"]), s["off"])
    assert got[on].tobytes() == (smooth[on] + (amp * CS.SQRT_JITTER)[None, :] * s["z"][on]).tobytes()
    assert got[:, 2].tobytes() == none[:, 2].tobytes() and got[on, 0].tobytes() != none[on, 0].tobytes()
    # respondents 2, 3, 4 share grid point 417: the same smooth value, and they differ by their nuggets alone
    assert smooth[2].tobytes() == smooth[3].tobytes() == smooth[4].tobytes()
    for a, b in ((2, 3), (3, 4)):
        assert (none[a] != none[b]).all()
        assert np.array_equal(none[a] - smooth[a], (smooth[a] + CS.SQRT_JITTER * s["z"][a]) - smooth[a])
        assert np.allclose(none[a] - none[b], CS.SQRT_JITTER * (s["z"][a] - s["z"][b]), rtol=0, atol=1e-15)
    assert CS.SQRT_JITTER == float(np.sqrt(np.longdouble(0.001)))      # the correctly rounded square root of the jitter


# ------------------------------------------------------------------------------------- 2. the effect, on the CPU ---
class _Gen:
    """What oracle/np_oracle.py's stage functions ask of a generator, on NumPy's (the draws are not R's: the chain is)."""

    def __init__(self, seed):
        self.g = np.random.default_rng(seed)

    def rnorm(self, mu, sd):
        return mu + sd * self.g.standard_normal()

    def runif(self, a, b):
        return a + (b - a) * self.g.random()


def _responses(seed):
    """synthetic answers with a non-linear part: P(y = +1) = plogis(b0 + b1 theta + a sin(1.7 theta + phase))"""
    g = np.random.default_rng(seed)
    theta = np.clip(np.round(g.normal(size=N), 2), -3, 3)
    b0, b1 = g.normal(0, 0.5, M), g.normal(1.0, 0.5, M)
    eta = b0[None, :] + theta[:, None] * b1[None, :] + g.uniform(0.5, 1.5, M)[None, :] * np.sin(1.7 * theta[:, None] + g.uniform(0, 6.28, M)[None, :])
    return np.where(g.random((N, M)) < 1.0 / (1.0 + np.exp(-eta)), 1.0, -1.0), _grid(np.rint((theta + 5.0) * 100.0))


def _chain(mode, seed=5):
    """The reference's iteration (oracle/np_oracle.py: draw_f, draw_fstar, draw_theta, draw_beta, factor), with the carry
    between draw_theta and draw_beta for mode "carry" / "smooth" (nugget on / off); Q after every iteration."""
    from gpirt_amd import consistent as CS
    from oracle import np_oracle as NP
    y, theta = _responses(seed)
    r = _Gen(seed + 1)
    pm, ps, step = np.zeros((2, M)), np.full((2, M), 3.0), np.full((2, M), 0.1)
    ts = NP.theta_star()
    prior = np.array([NP.dnorm_log(t, 0.0, 1.0) for t in ts])
    L = NP.factor(theta)
    f = L @ r.g.standard_normal((N, M))
    beta = pm + ps * r.g.standard_normal((2, M))
    mu = beta[0][None, :] + theta[:, None] * beta[1][None, :]
    mu_star = beta[0][None, :] + ts[:, None] * beta[1][None, :]
    Q = []
    for _ in range(ITERS):
        f, _ = NP.draw_f(r, f, y, L, mu)
        fstar, _, _ = NP.draw_fstar(r, f, theta, ts, L, mu_star)
        theta = NP.draw_theta(r, ts, y, prior, fstar, stabilise=True)
        if mode != "reference":
            f = CS.carry_exact(theta, fstar, mu_star, f, r.g.standard_normal((N, M)), nugget=(mode == "carry"))
        beta = NP.draw_beta(r, beta, theta, y, f, pm, ps, step)
        mu = beta[0][None, :] + theta[:, None] * beta[1][None, :]
        mu_star = beta[0][None, :] + ts[:, None] * beta[1][None, :]
        L = NP.factor(theta)
        Q.append(float(CS.prior_quad_exact(theta, f, None).mean()))
    return np.array(Q)


def test_prior_quad_exact_on_a_prior_draw():
    from gpirt_amd import consistent as CS
    from oracle import np_oracle as NP
    g = np.random.default_rng(2)
    theta = _grid(g.integers(200, 800, 90))
    L = NP.factor(theta)
    f = L @ g.standard_normal((90, 40))
    q = CS.prior_quad_exact(theta, f, "se")
    # q_j n is chi-square with n degrees of freedom: the mean over 40 items has sd sqrt(2 / (90 * 40)) = 0.024
    assert q.shape == (40,) and abs(q.mean() - 1.0) < 0.1
    assert np.allclose(CS.prior_quad_exact(theta, 2.0 * f, "se", amp=2.0), q, rtol=1e-12, atol=0)
    assert np.allclose(CS.prior_quad_exact(theta, f, dict(family="se", length_scale=1.0), amp=np.full(40, 0.5)), 4.0 * q, rtol=1e-12, atol=0)


def test_effect_of_the_carry_on_the_prior_quadratic_form():
    """The issue's table at 120 x 8 (three seeds there: 0.898 .. 1.086 with the carry, 162 .. 334 under the reference's step,
    0.025 .. 0.031 at 300 x 30 without the nugget): bounds [0.8, 1.25], above 20, below 0.2 over iterations 6 .. 25."""
    q = {mode: _chain(mode)[FROM - 1:] for mode in ("reference", "carry", "smooth")}
    for mode, v in q.items():
        print(f"MEASURED Q over iterations {FROM}..{ITERS}, {mode}: {v.min():.3f} .. {v.max():.3f}")
    assert (q["carry"] >= 0.8).all() and (q["carry"] <= 1.25).all()
    assert (q["reference"] > 20.0).all()
    assert (q["smooth"] < 0.2).all()
