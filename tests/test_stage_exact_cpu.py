"""The long-double references of draw_f and draw_fstar (tests/_stage_exact.py) against the CPU oracle, and the conditions
the constructed GPU cases rest on -- no undecided trial, trials inside and near the screen's band, the interpolation
error per rank -- checked here, without a GPU, so that a device test that disagrees points at the kernel."""
import numpy as np
import pytest

import _stage_exact as X

RANKS = (16, 32, 48, 64, 80, 96, 112, 128)


def test_item_rng_restatement_equals_the_oracle(oracle):
    idx = np.arange(40)[:, None]
    for seed, it, stage in ((7, 1, X.ST_F_ESS), (2 ** 40 + 3, 9, X.ST_F_Z), (0, 0, X.ST_FSTAR)):
        u = X.item_uniforms(seed, it, stage, np.array([0, 5, 1023])[None, :], idx)
        ref = np.array([[oracle.item_uniform(seed, it, stage, item, ix) for item in (0, 5, 1023)] for ix in range(40)])
        assert np.array_equal(u, ref)
    p = np.concatenate([np.random.default_rng(0).random(4000), [1e-300, 1e-20, 1 - 1e-16, 0.5, 0.075, 0.925, 0.0750001]])
    assert np.array_equal(X.qnorm(p), np.array([oracle.qnorm(v) for v in p]))


@pytest.mark.parametrize("n,seed", [(8, 3), (60, 4), (257, 5)])
def test_slice_written_equals_oracle_ess(oracle, n, seed):
    rng = np.random.default_rng(seed)
    theta = rng.normal(size=n)
    L, info = oracle.factor(theta)
    assert info == 0
    for item in range(6):
        f = rng.normal(size=n)
        y = np.where(rng.random(n) < 0.5, 1.0, -1.0)
        y[rng.random(n) < 0.1] = np.nan
        mu = 0.4 - 0.7 * theta
        out, nu, tr = oracle.ess(oracle.ItemStream(seed), f, y, L, mu, it=2, item=item)
        us = X.item_uniforms(seed, 2, X.ST_F_ESS, item, np.arange(256))
        for term in ("written", "exact"):          # (ordinary inputs: the two terms differ by 1e-16 per row and agree in k)
            ref = X.slice_exact(f, y, nu, mu, us, term)
            assert ref["undecided"] == 0
            assert ref["k"] == tr["k"]
            assert np.abs(ref["f_new"].astype(np.float64) - out).max() <= 1e-12
            assert len(ref["margin"]) == ref["k"] + 1 and all(b > 0 for b in ref["bound"])


def test_slice_consumes_nothing_once_the_bracket_has_closed():
    """a state no trial point improves on: the bracket closes onto eps = 0 and the loop must end there by the
    eps_min == eps_max rule with f' = f (cos 0 = 1), having consumed at most ~1100 uniforms (52 halvings per side ...)"""
    n = 5
    f, nu, mu, y = np.full(n, 30.0), np.full(n, -40.0), np.zeros(n), np.ones(n)
    us = np.concatenate([[1.0 - 2.0 ** -53], np.full(3000, 0.5)])     # log u = -1.1e-16: only f itself reaches the level
    ref = X.slice_exact(f, y, nu, mu, us, "exact")
    assert ref["eps"] == 0.0 and np.array_equal(ref["f_new"].astype(np.float64), f)


def test_rank64_reference_equals_oracle_draw_fstar(oracle):
    n, m = 200, 3
    rng = np.random.default_rng(8)
    theta = np.clip(rng.normal(size=n), -4.9, 4.9)
    L, info = oracle.factor(theta)
    assert info == 0
    f, mu_star = rng.normal(size=(n, m)), rng.normal(size=(X.NGRID, m))
    fstar, s, mean = oracle.draw_fstar(oracle.ItemStream(5), f, theta, L, mu_star, it=3)
    z = X.item_normals(5, 3, X.ST_FSTAR, np.arange(m), X.NGRID)
    for r in (64, 0):
        ref = X.fstar_rank_exact(theta, L, f, mu_star, r, z)
        assert np.abs(ref["s"].astype(np.float64) - s).max() <= 1e-9
        assert np.abs((ref["mean"] + mu_star).astype(np.float64) - mean).max() <= 1e-9
        assert np.abs(ref["fstar"].astype(np.float64) - fstar).max() <= 1e-9


def test_interpolation_error_per_rank():
    """What include/gpirt_hip.h and the README state about kstar_rank: r = 16 and r = 32 approximate K*, r >= 48 is exact
    to rounding."""
    err = {r: X.interpolation_error(r) for r in RANKS}
    print("MEASURED interpolation error", {r: "%.2e" % e for r, e in err.items()})
    assert err[16] > 1e-9 and err[32] > 1e-9
    assert 1e-3 < err[16] < 1e-2 and 1e-8 < err[32] < 1e-7
    for r in RANKS[2:]:
        assert err[r] < 1e-13
    for r in RANKS[3:]:
        assert err[r] < 2e-16
    c, V = X.cheb_basis(64)
    assert np.abs(V.sum(axis=1) - 1).max() < 1e-17            # a partition of unity
    assert np.all(np.diff(c) < 0) and abs(c[0]) < 5 and np.allclose(c, -c[::-1], atol=1e-15)


@pytest.mark.parametrize("n", X.ORDERS)
def test_constructed_draw_f_inputs_decide_every_trial(n):
    """The conditions on the inputs of tests/test_gpu_draw_f_constructed.py: under both terms no trial's margin is below the
    derived bound of the device's rounding, and at the orders of the register kernels the screen-band columns hold at
    least 5 trials inside the band and 5 within four bands of the level but outside it."""
    for term in ("exact", "written"):
        band = near = 0
        for sigma in X.SIGMAS:
            names = X.draw_f_cases(n, sigma)[0]
            res, _ = X.draw_f_reference(n, sigma, term)
            for nm, r in zip(names, res):
                assert r["undecided"] == 0, (n, sigma, term, nm, min(r["margin"]))
                if nm.startswith("band"):
                    band += r["n_band"]
                    near += r["n_near"]
        print(f"MEASURED n={n} term={term}: {band} trials inside the screen band, {near} within four bands")
        if 2049 <= n <= 16384:
            assert band >= 5 and near >= 5


@pytest.mark.parametrize("n", X.ORDERS)
def test_constructed_columns_are_what_they_claim(n):
    names, F, Y, MU = X.draw_f_cases(n, 1.0)
    ex, Z = X.draw_f_reference(n, 1.0, "exact")
    wr, _ = X.draw_f_reference(n, 1.0, "written")
    col = {nm: j for j, nm in enumerate(names)}
    a = Y * (F + MU)
    j = col["a_30_45"]
    obs = ~np.isnan(Y[:, j])
    assert (np.abs(a[obs, j]) >= 30).all() and (np.abs(a[obs, j]) <= 45).all() and (a[obs, j] > 37).any() and (a[obs, j] < -37).any()
    assert 0.03 < np.isnan(Y[:, col["ordinary"]]).mean() < 0.09 or n == 100
    for nm, lo, hi in (("mu_300", 298, 302), ("mu_700", 698, 702)):
        v = np.abs(MU[:, col[nm]])
        assert (v >= lo).all() and (v <= hi).all()
        assert not any(wr[col[nm]]["overflow"])                # finite under both forms
    j = col["no_observed_row"]
    for r in (ex[j], wr[j]):
        assert r["k"] == 0 and np.array_equal(r["f_new"], F[:, j].astype(X.LD) * np.cos(X.LD(r["eps"])) +
                                              Z[:, j].astype(X.LD) * np.sin(X.LD(r["eps"])))
    # sigma = 50: trial points move by hundreds and stay finite at |mu| = 300
    names50 = X.draw_f_cases(n, 50.0)[0]
    ex50, _ = X.draw_f_reference(n, 50.0, "exact")
    wr50, _ = X.draw_f_reference(n, 50.0, "written")
    j = names50.index("mu_300_s50")
    assert not any(wr50[j]["overflow"])
    # the current state beyond the overflow: the written level is -inf and the first finite trial is accepted; the exact
    # level is a huge finite number and the slice goes on -- the two references disagree in k
    j = names50.index("current_overflow")
    assert wr50[j]["k"] != ex50[j]["k"]
    assert all(wr50[j]["overflow"][:-1]) and not wr50[j]["overflow"][-1]
    # trial points beyond the overflow: the wide trials of the written form hold an overflowing row (nu = 1e3 z; the
    # bracket has to shrink to |sin eps| < 0.7 / max|z| before none does), each of them is a rejection
    wrk, _ = X.draw_f_reference(n, 1000.0, "written")
    ov = wrk[0]["overflow"]
    assert not ov[-1] and sum(ov) >= 3
