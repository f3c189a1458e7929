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


# ------------------------------------------------------------------ draw_theta and draw_beta on constructed states ----
THETA_CASES = ("one_item_finite", "one_item_fallback", "dense_smooth", "dense_nan_cell", "dense_nan_row", "dense_pm800",
               "dense_overflow_item")


def test_theta_and_beta_randoms_equal_the_oracle(oracle):
    u = X.theta_uniforms(X.THETA_SEED, X.THETA_IT, 140)
    assert np.array_equal(u, [oracle.item_uniform(X.THETA_SEED, X.THETA_IT, X.ST_THETA, i, 0) for i in range(140)])
    z, v = X.beta_randoms(9, X.BETA_IT, 25)
    for j in range(25):
        raw = [oracle.item_uniform(9, X.BETA_IT, X.ST_BETA, j, ix) for ix in range(4)]
        assert np.array_equal(v[:, j], [raw[1], raw[3]])
        assert np.array_equal(z[:, j], [oracle.qnorm(raw[0]), oracle.qnorm(raw[2])])


@pytest.mark.parametrize("name", THETA_CASES)
def test_constructed_draw_theta_cases_decide_every_respondent(oracle, name):
    """The conditions tests/test_gpu_draw_theta_constructed.py rests on: under both products' bounds and with and without
    stabilisation no respondent is undecided; every kind is what draw_theta_cases() says it is; the near-ties lie within
    1e-5 of a step of the CDF (the tight ones at 1e-11, at least four bounds away from it); and the CPU oracle draws the
    reference's rows wherever its own sequential fp64 sums are decided."""
    c = X.draw_theta_cases()[name]
    y, kinds, k0 = c["y"], np.array(c["kinds"]), c["k0"]
    n = y.shape[0]
    for stabilise in (False, True):
        idx = None
        for product in ("fixed", "gemm"):
            r = X.draw_theta_reference(name, stabilise, product)
            assert r["undecided"].sum() == 0, (name, stabilise, product, np.flatnonzero(r["undecided"])[:8])
            assert idx is None or np.array_equal(idx, r["index"])
            idx = r["index"]
            tie = kinds == "tie"
            if tie.any():
                delta = np.array(X.TIE_DELTAS)[k0[tie]]
                assert (r["margin"][tie] <= 1e-5).all()
                assert (np.abs(r["margin"][tie] / np.abs(delta) - 1) < 0.05).all(), r["margin"][tie] / np.abs(delta)
                assert (4 * r["bound"][tie] < np.abs(delta)).all(), (r["bound"][tie].max(), product)
                assert np.array_equal(idx[tie], np.where(delta > 0, X.TIE_ROWS[0], X.TIE_ROWS[1]))
                assert set(np.abs(delta)) == {1e-6, 1e-9, 1e-11} and (delta > 0).any() and (delta < 0).any()
                print(f"MEASURED {name} stabilise={stabilise} {product}: largest bound at a near-tie {r['bound'][tie].max():.2e}")
        fin = np.isfinite(r["bound"])
        print(f"MEASURED {name} stabilise={stabilise}: degenerate {r['degenerate']}, smallest margin {r['margin'].min():.2e}, "
              f"largest bound {r['bound'][fin].max():.2e}")
        if name.startswith("one_item"):
            for kind in ("point", "last_row"):
                assert np.array_equal(idx[kinds == kind], k0[kinds == kind]) and (kinds == kind).any()
            assert (idx[kinds == "last_row"] == X.NGRID - 1).all()
            assert (idx[kinds == "row_0"] == -1).all() and (kinds == "row_0").any()
            assert (idx[kinds == "flat"] > 0).all() and (kinds == "flat").any()
            assert ((idx[kinds == "peaked"] >= 0) == stabilise).all() and (kinds == "peaked").any()
            assert (idx[kinds == "overflow"] == -1).all()
            assert (kinds == "overflow").any() == (name == "one_item_fallback") == X.theta_hands_over(c["fstar"])
            assert kinds[128] == "tie" and kinds[129] == "point"          # the ragged tile's respondents are not idle ones
        else:
            smooth = X.draw_theta_reference("dense_smooth", stabilise, "gemm")["index"]
            sees = ~np.isnan(y[:, X.DENSE_J0]) if name == "dense_nan_cell" else ~np.isnan(y).all(axis=1)
            if name in ("dense_nan_cell", "dense_nan_row"):
                assert (idx[sees] < X.DENSE_K0).all() and sees.any() and (~sees).any()
                assert np.array_equal(idx[~sees], smooth[~sees])            # a missing answer hides the NaN
                assert (smooth[sees] >= X.DENSE_K0).any()                   # ... and for some who see it the draw moves
                if name == "dense_nan_cell":
                    assert (idx[~sees] >= X.DENSE_K0).any()                 # where 0 * NaN = NaN would have moved it
            if name == "dense_overflow_item":
                assert r["degenerate"] == int((y[:, 11] == -1.0).sum()) > 0 and (idx[y[:, 11] == -1.0] == -1).all()
            if name in ("dense_smooth", "dense_pm800"):
                assert r["degenerate"] == 0
            assert 0.04 < np.isnan(y[1:]).mean() < 0.10
        ro = X.draw_theta_reference(name, stabilise, "oracle")
        th, deg = oracle.draw_theta(oracle.ItemStream(X.THETA_SEED), y, c["fstar"], it=X.THETA_IT, stabilise=stabilise)
        rows = np.where(np.isnan(th), -1, np.rint((th + 5.0) / 0.01)).astype(np.int64)
        ok = ~ro["undecided"]
        assert ok.sum() >= n - 2 and np.array_equal(rows[ok], ro["index"][ok]) and deg == ro["degenerate"]


@pytest.mark.parametrize("n", X.BETA_ORDERS)
def test_constructed_draw_beta_cases_decide_every_step(oracle, n):
    """The conditions tests/test_gpu_draw_beta_constructed.py rests on: no decision is undecided; the near-ties lie within 1e-5
    of log u, on the side their name says; both branches of the kept log-likelihood occur, and each overflow branch; and
    the CPU oracle's beta is the reference's."""
    c = X.draw_beta_cases(n)
    ref = X.draw_beta_reference(n)
    col = {nm: j for j, nm in enumerate(c["names"])}
    for nm, r in zip(c["names"], ref):
        assert r["undecided"] == 0, (n, nm, r["margin"], r["bound"])
    for nm, k, delta in X.BETA_TIES:
        r = ref[col[nm]]
        assert r["margin"][k] <= 1e-5 and abs(r["margin"][k] / abs(delta) - 1) < 0.05 and 4 * r["bound"][k] < abs(delta)
        assert r["accept"][k] == (delta > 0)
        if k == 1:
            # behind a forced step 0, whose two sums differ by far more than the tie's margin: a kept sum from the wrong
            # branch moves r by that difference and flips one tie of the pair
            assert r["accept"][0] == (abs(delta) == 1e-6) and r["margin"][0] > 0.9
            j = col[nm]
            th, yy, ff = c["theta"], c["y"][:, j], c["f"][:, j]
            lls = [-np.nansum(np.log1p(np.exp(-yy * (ff + b0 + th * c["beta"][1, j])))) for b0 in (c["beta"][0, j], r["proposal"][0])]
            assert abs(lls[1] - lls[0]) > 1e3 * abs(delta), (nm, lls)
        if n == 257:
            # without row 256 (the one a loop that stops at 256 rows misses) r moves by far more than the tie's margin
            j = col[nm]
            y2 = c["y"][:, j].copy()
            assert not np.isnan(y2[256])
            y2[256] = np.nan
            z, u = X.beta_randoms(c["seed"], c["it"], len(c["names"]))
            r2 = X.beta_exact(c["beta"][:, j], c["theta"], y2, c["f"][:, j], c["pm"][:, j], c["ps"][:, j], c["step"][:, j], z[:, j], u[:, j])
            assert abs(float(r2["r"][k] - r["r"][k])) > 1e3 * abs(delta), (nm, float(r2["r"][k] - r["r"][k]))
    for nm in ("step0_zero", "step1_zero", "both_zero"):
        r = ref[col[nm]]
        assert all(r["accept"][k] and r["r"][k] == 0 for k in range(2) if c["step"][k, col[nm]] == 0.0)
    a, b = ref[col["accept_then_decide"]], ref[col["reject_then_decide"]]
    assert a["accept"][0] and not b["accept"][0] and a["margin"][0] > 0.9 and b["margin"][0] > 0.9
    assert min(a["margin"][1], b["margin"][1]) > 1e-3
    r = ref[col["both_overflow"]]
    assert r["overflow"] == [(True, True), (True, True)] and r["accept"] == [False, False] and np.isnan(r["r"][0])
    r = ref[col["proposal_overflow"]]
    assert r["overflow"][0] == (True, False) and not r["accept"][0] and r["r"][0] == -np.inf
    r = ref[col["current_overflow"]]
    assert r["overflow"][0] == (False, True) and r["accept"][0] and r["r"][0] == np.inf and r["overflow"][1] == (False, False)
    r = ref[col["proposal_overflow_s1"]]
    assert r["overflow"][1] == (True, False) and not r["accept"][1]
    assert not np.isnan(c["y"][:min(n, 2), [j for nm, j in col.items() if nm not in ("no_observed_row", "single_observed_row")]]).any()
    assert np.isnan(c["y"][:, col["no_observed_row"]]).all() and (~np.isnan(c["y"][:, col["single_observed_row"]])).sum() == 1
    worst = max(bd / mg for r in ref for bd, mg in zip(r["bound"], r["margin"]) if np.isfinite(mg))
    print(f"MEASURED n={n}: worst bound / margin {worst:.3f}")
    o = oracle.draw_beta(oracle.ItemStream(c["seed"]), c["beta"], c["theta"], c["y"], c["f"], c["pm"], c["ps"], c["step"], it=c["it"])
    assert np.abs(o - np.stack([r["beta"] for r in ref], axis=1)).max() <= 1e-12
