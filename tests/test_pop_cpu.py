"""The population prior for theta on the host (gpirt_amd/pop.py, csrc/pop.hip's host tables and gpirt_pop_check): no GPU.

Also the condition on the inputs of tests/test_gpu_pop.py: under the reference's own bound every constructed draw_theta case
leaves at most 1 % of its respondents undecided, and no hyper-draw of the update cases is undecided."""
import numpy as np
import pytest

import _pop_exact as PX
import _stage_exact as X

LD = np.longdouble


@pytest.fixture(scope="module")
def PO():
    from gpirt_amd import _lib, build
    import os
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    from gpirt_amd import pop
    return pop


def test_version_and_stage(PO):
    from gpirt_amd import _lib
    assert _lib.load().gpirt_version() >= 134 and _lib.ST_POP == 12
    for name in ("gpirt_pop_check", "gpirt_sampler_pop_set", "gpirt_sampler_pop_enable", "gpirt_sampler_draw_pop",
                 "gpirt_sampler_pop_record", "gpirt_sampler_pop_get", "gpirt_sampler_pop_stats"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)


def test_default_row_is_the_kernels_expression(PO):
    """theta_sample_kernel: ts = -5.0 + k * 0.01; z = fabs((ts - 0.0) / 1.0); -(LN_SQRT_2PI + 0.5 * z * z + log(1.0)), every
    operation rounded on its own (the library is built without contraction)"""
    ts = -5.0 + np.arange(1001, dtype=np.float64) * 0.01
    z = np.abs((ts - 0.0) / 1.0)
    ln = np.float64(0.918938533204672741780329736406)
    want = -((ln + (0.5 * z) * z) + np.log(1.0))
    assert np.array_equal(PO.default_row(), want)
    # the long-double prior of theta_exact is within the three roundings its bound grants
    ref = -(X.LN_SQRT_2PI + LD(0.5) * ts.astype(LD) ** 2)
    assert (np.abs((PO.default_row().astype(LD) - ref).astype(np.float64)) <= 3 * 2.0 ** -53 * np.abs(want) + 1e-300).all()


def test_normal_table_and_grids(PO):
    t = PO.theta_grid()
    tab = PO.normal_table([0.0, 1.25], [1.0, 0.8])
    z = (t - 1.25) / 0.8
    assert np.array_equal(tab[1], -((0.5 * z) * z))
    mu, sd = PO.grids(2.5, 256, 0.25, 4.0, 255)
    assert mu[0] == -2.5 and mu[-1] == 2.5 and np.array_equal(mu, -mu[::-1]) and (np.diff(mu) > 0).all()
    assert sd[0] == 0.25 and sd[-1] == 4.0 and (np.diff(sd) > 0).all()
    k = np.arange(255, dtype=LD)
    want = (LD(0.25) * (LD(4.0) / LD(0.25)) ** (k / 254)).astype(np.float64)
    assert np.abs(sd - want).max() <= 2 * np.spacing(4.0)
    mu3, _ = PO.grids(1.0, 3, 0.5, 1.0, 2)
    assert np.array_equal(mu3, [-1.0, 0.0, 1.0])


def _lse_brute(mu, sd):
    t = (-5.0 + np.arange(1001, dtype=np.float64) * 0.01).astype(LD)
    return np.log(np.exp(-(t - LD(mu)) ** 2 / (2 * LD(sd) * LD(sd))).sum())


def test_lse_table_against_a_brute_force_sum(PO):
    """at the grids' corners, and where mu + 3 sd passes 5 (the truncation matters: lse is then well below log(sd sqrt(2 pi) 100)).
    The tolerance: 1001 long-double terms in (0, 1], each exp within 1 ulp_ld and the sum's 1000 additions one each, so the sum
    is within 2002 2^-64 relative, the log adds 2^-64 |lse| and the rounding to fp64 2^-53 |lse|."""
    mu, sd = PO.grids(5.0, 9, 0.05, 10.0, 7)
    lse = PO.lse_table(mu, sd)
    for a, b in ((0, 0), (0, 6), (8, 0), (8, 6), (4, 3), (7, 2), (7, 3), (6, 4)):
        ref = _lse_brute(mu[a], sd[b])
        tol = 2002 * 2.0 ** -64 + (2.0 ** -64 + 2.0 ** -53) * abs(float(ref))
        assert abs(float(LD(lse[a, b]) - ref)) <= tol, (a, b)
    a, b = 7, 3                                                           # mu = 3.75, sd about 0.7: mu + 3 sd passes 5
    assert mu[a] + 3 * sd[b] > 5.0
    full = np.log(sd[b] * np.sqrt(2 * np.pi) * 100.0)
    assert lse[a, b] < full - 1e-5


def test_step_exact_lp_against_direct_enumeration(PO):
    """lp[a] (flat hyperprior) is sum_i log pi_ab(k_i), pi_ab(k) = exp(-(t_k - mu_a)^2 / (2 sd_b^2)) / sum_k' exp(.), up to
    rounding.  The fp64 row: Q is 8 operations on terms of magnitude at most M = S2 c^2 + 2 |mu S1| c + n mu^2, so
    |dQ| <= 8 u M; Q / den and the subtraction 2 u |Q / den| more; n lse one product of a table entry with its own u |lse| and
    the last subtraction one rounding: in all (8 M / den + 3 |Q| / den + 3 n |lse|) u, taken with a factor 2 for the long-double
    enumeration's own n terms (each 2^-64 relative: far below)."""
    c = PX.update_case(257, 8, 2, 1024)
    mu, sd = PO.grids(2.5, 17, 0.25, 4.0, 9)
    lse = PO.lse_table(mu, sd)
    st = PO.stats_exact(c["theta"], c["codes"], 8)
    t = PO.theta_grid().astype(LD)
    u = 2.0 ** -53
    for g, b in ((1, 0), (3, 4), (7, 8)):
        n, S1, S2 = int(st["n"][g]), int(st["S1"][g]), int(st["S2"][g])
        row = PO.lp_mu_row(n, S1, S2, mu, sd[b], lse[:, b], np.zeros(17))
        k = PO.grid_index(c["theta"][c["codes"] == g])
        den = 2 * sd[b] * sd[b]
        for a in range(17):
            e = -(t - LD(mu[a])) ** 2 / (2 * LD(sd[b]) * LD(sd[b]))
            direct = (e[k] - np.log(np.exp(e).sum())).sum()
            M = S2 * 1e-4 + 2 * abs(mu[a] * S1) * 0.01 + n * mu[a] ** 2
            Q = S2 * 1e-4 - 2 * mu[a] * S1 * 0.01 + n * mu[a] ** 2
            tol = 2 * (8 * M / den + 3 * abs(Q) / den + 3 * n * abs(lse[a, b])) * u
            assert abs(float(LD(row[a]) - direct)) <= tol, (g, a, float(LD(row[a]) - direct), tol)
        rs = PO.lp_sd_row(n, S1, S2, mu[5], sd, lse[5, :], np.zeros(9))
        assert rs[b] == PO.lp_mu_row(n, S1, S2, mu, sd[b], lse[:, b], np.zeros(17))[5]


def test_stats_exact_and_off_grid(PO):
    theta = np.array([-5.0, 0.0, -5.0 + 501 * 0.01, 5.0, 0.123456, np.nan, -5.0 + 250 * 0.01])
    codes = np.array([0, 0, 1, 1, 1, 2, 2])
    st = PO.stats_exact(theta, codes, 3)
    assert st["n"].tolist() == [2, 2, 1] and st["off_grid"].tolist() == [0, 1, 1]
    assert st["S1"].tolist() == [-500, 501, -250] and st["S2"].tolist() == [250000, 1 + 250000, 62500]


def test_conditional_sums_to_one(PO):
    c = PX.frozen_case()
    F = PX.FROZEN
    mu, sd = PO.grids(F["mu_hi"], F["P"], F["sd_lo"], F["sd_hi"], F["P"])
    lse = PO.lse_table(mu, sd)
    st = PO.stats_exact(c["theta"], c["codes"], F["G"])
    for g in (1, 2):
        p = PO.conditional(st["n"][g], st["S1"][g], st["S2"][g], mu, sd, lse)
        assert p.shape == (F["P"], F["P"]) and abs(float(p.sum()) - 1.0) <= 1e-15 and (p >= 0).all()
        assert (p[0, :] == 0).all() and (p[:, 0] == 0).all()              # the rule of the draw: index 0 is never taken
        a, b = np.unravel_index(np.argmax(p), p.shape)
        mem = c["theta"][c["codes"] == g]
        assert abs(mu[a] - mem.mean()) <= 2 * (mu[1] - mu[0]) and abs(np.log(sd[b] / mem.std())) <= 0.3


def test_grid_draw_exact_against_the_loop(PO):
    rng = np.random.default_rng(3)
    for P in (2, 3, 255, 1024):
        lp = -rng.uniform(0, 30, P)
        for u in (0.013, 0.5, 0.97):
            d = PO.grid_draw_exact(lp, u)
            k, margin, bound = PX.hyper_draw(lp, u)
            assert d["index"] == k and k >= 1
            assert abs(d["margin"] - margin) <= 1e-15 and abs(d["bound"] - bound) <= 0.01 * bound
    assert PO.grid_draw_exact(np.array([0.0, -1e4]), 0.5)["index"] == -1 and PX.hyper_draw([0.0, -1e4], 0.5)[0] == -1


def test_summarise_reverses_a_reflected_chain(PO):
    mu, sd = PO.grids(2.0, 5, 0.5, 2.0, 3)
    draws = np.array([[[[-1, -1], [4, 1]], [[-1, -1], [3, 2]]], [[[-1, -1], [0, 1]], [[-1, -1], [1, 2]]]])      # 2 chains x 2 x G=2 x 2
    hm = np.zeros((2, 5, 2), dtype=np.int64)
    hs = np.zeros((2, 3, 2), dtype=np.int64)
    for c in range(2):
        for s in range(2):
            hm[c, draws[c, s, 1, 0], 1] += 1
            hs[c, draws[c, s, 1, 1], 1] += 1
    out = PO.summarise(draws, hm, hs, mu, sd, signs=[1, -1])
    assert np.array_equal(out["draws"][1, :, 1, 0], [4, 3]) and np.array_equal(out["draws"][1, :, 0, 0], [-1, -1])
    assert out["hist_mu"][:, 1].tolist() == [0, 0, 0, 2, 2] and out["hist_sd"][:, 1].tolist() == [0, 2, 2]
    assert out["mu_mean"][1] == 1.5 and np.isnan(out["mu_mean"][0])


def test_check_args_refuses(PO):
    from gpirt_amd import _lib
    from gpirt_amd.sampler import _options
    codes = np.array([0, 1, 2, 1, 0], dtype=np.int32)
    ok = dict(codes=codes, groups=3, sampled=True)
    PO.check_args(**ok)
    PO.check_args(codes, 3, np.zeros((3, 1001)))

    def refused(word, **kw):
        with pytest.raises(_lib.GpirtError, match=word) as e:
            PO.check_args(**dict(ok, **kw))
        assert e.value.code == _lib.E_ARG

    refused("no member", groups=4)
    refused("G = 0", groups=0, codes=None)
    refused("G = 9", groups=9, codes=None)
    refused(r"codes\[1\] = -1", codes=np.array([0, -1, 2, 1, 0]))
    refused(r"codes\[2\] = 3", codes=np.array([0, 1, 3, 1, 0]))
    bad = np.zeros((3, 1001))
    bad[2, 17] = np.inf
    refused(r"log_prior\[2, 17\] is not finite", log_prior=bad, sampled=False)
    bad[2, 17] = np.nan
    refused(r"log_prior\[2, 17\] is not finite", log_prior=bad, sampled=False)
    for pm, ps in ((1, 65), (1025, 65), (121, 1), (121, 1025)):
        refused("each must lie in 2 .. 1024", points_mu=pm, points_sd=ps)
    for hi in (0.0, -1.0, 5.000001, np.nan, np.inf):
        refused(r"mu_hi = .* \(0, 5\]", mu_hi=hi)
    for lo, hi in ((0.049, 5.0), (1.0, 1.0), (2.0, 1.0), (0.2, 10.5), (np.nan, 5.0)):
        refused("sd_lo = .* sd_hi = ", sd_lo=lo, sd_hi=hi)
    h = np.zeros(121)
    h[5] = np.nan
    refused(r"log_hyper_mu\[5\]", log_hyper_mu=h)
    h = np.zeros(65)
    h[64] = -np.inf
    refused(r"log_hyper_sd\[64\]", log_hyper_sd=h)
    refused(r"a0\[1\] = 121", a0=121)
    refused(r"b0\[1\] = -1", b0=-1)
    ref = _options("reference", 1, True, True, None)
    refused("R's stream has no such draw", options=ref)
    PO.check_args(codes, 3, np.zeros((3, 1001)), options=ref)             # fixed: both RNG contracts
    refused("item shard", options=_options("item", 1, True, True, None, 4, 8))
    with pytest.raises(_lib.GpirtError, match="item shard"):
        PO.check_args(codes, 3, np.zeros((3, 1001)), options=_options("item", 1, True, True, None, 4, 8))


def test_uniforms_are_stage_12(PO):
    u0, u1 = PO.uniforms(31, 3, np.arange(4))
    want = X.item_uniforms(31, 3, 12, np.arange(4, dtype=np.uint64)[:, None], np.arange(2, dtype=np.uint64)[None, :])
    assert np.array_equal(u0, want[:, 0]) and np.array_equal(u1, want[:, 1])
    assert PO.uniforms(31, 3, 2) == (u0[2], u1[2])


# ------------------------------------------------------------------------- the conditions on the GPU tests' inputs ---
@pytest.mark.parametrize("shape", PX.THETA_SHAPES)
def test_theta_cases_are_decided(PO, shape):
    n, G = shape
    c = PX.theta_case(n, G)
    assert np.bincount(c["codes"], minlength=G).min() >= 1 and (G == 1 or np.bincount(c["codes"])[G - 1] == 1)
    for product in ("fixed", "gemm"):
        ref = PX.theta_exact_table(c["y"], c["fstar"], c["u"], True, c["codes"], c["table"], product)
        assert ref["undecided"].sum() <= 0.01 * n, (shape, product, int(ref["undecided"].sum()))
        assert np.isfinite(ref["bound"]).all() and (ref["index"] >= 0).all()


def test_theta_exact_table_with_default_rows_is_theta_exact(PO):
    c = PX.theta_case(65, 2)
    tab = np.tile(PO.default_row(), (2, 1))
    a = PX.theta_exact_table(c["y"], c["fstar"], c["u"], True, c["codes"], tab)
    b = X.theta_exact(c["y"], c["fstar"], c["u"], True)
    assert np.array_equal(a["index"], b["index"]) and (a["bound"] <= b["bound"]).all()


@pytest.mark.parametrize("case", PX.UPDATE_CASES)
def test_update_cases_are_decided(PO, case):
    n, G, P_mu, P_sd = case
    c = PX.update_case(*case)
    assert np.bincount(c["codes"], minlength=G).min() >= 1
    mu, sd = PO.grids(PX.MU_HI, P_mu, PX.SD_LO, PX.SD_HI, P_sd)
    lse = PO.lse_table(mu, sd)
    idx = np.stack([c["a0"], c["b0"]], axis=1)
    ref = PO.step_exact(c["theta"], c["codes"], idx, PX.UPDATE_SEED, 1, mu, sd, lse)
    assert ref["status"] == ["anchor"] + ["updated"] * (G - 1)
    assert ref["decided"].all(), (case, ref["margin"], ref["bound"])
    for g in range(1, G):                                                  # the loop of tests/_pop_exact.py agrees
        assert PX.hyper_draw(ref["lp_mu"][g], ref["u0"][g])[0] == ref["index"][g, 0]
        assert PX.hyper_draw(ref["lp_sd"][g], ref["u1"][g])[0] == ref["index"][g, 1]
