"""The covariance kernel on the device (include/gpirt_hip.h "the covariance kernel", csrc/se_kernel.hip, gpirt_amd.kernel):
the squared exponential with a length scale and the Matern 5/2 and 3/2 forms against long double (tests/_kernel_exact.py),
through the operators, the sampler's lower build, the factorisation, draw_fstar in its three forms, whole chains, and the
one-call runs of gpirt_amd.kernel.  Every handle is the test's own: the session's `handle` keeps the default kernel."""
import numpy as np
import pytest

import _kernel_exact as KX
import _stage_exact as X

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
CODES = dict(yea=[1], nay=[-1], missing=[None])
FAST = dict(rng="item", theta_stabilise=True, fstar_fused=True)


@pytest.fixture
def handles():
    """make(kernel) -> a fresh Handle under that kernel; all closed when the test ends"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpirt_amd.ops import Handle
    made = []

    def make(kernel=None):
        made.append(Handle(kernel=kernel))
        return made[-1]

    yield make
    for h in made:
        h.close()


def _grid_theta(n, seed):
    return -5.0 + np.random.default_rng(seed).integers(0, X.NGRID, n) * 0.01


# ------------------------------------------------------------------------------------------------ 1. the operator ---
@pytest.mark.parametrize("shape", [(1, 1), (129, 33), (257, 1001), (258, 37)])
@pytest.mark.parametrize("ell", KX.LENGTH_SCALES)
@pytest.mark.parametrize("family", KX.FAMILIES)
def test_se_kernel_against_long_double(handles, family, ell, shape):
    """Handle.se_kernel under every family and length scale against kernel_ld, with the jitter where n1 = n2.  (1, 1),
    (129, 33) and (257, 1001) have an odd leading dimension: the scalar stores; (258, 37) an even one: the two-row stores,
    three row blocks, a ragged last strip.  The bound is derived in tests/_kernel_exact.py: test_se_kernel's 4e-16 for the
    default kernel, + 4 u / e for the squared exponential at a length scale, 12.1 u and 7.8 u for the Matern forms."""
    from gpirt_amd.ops import to_device, to_host
    n1, n2 = shape
    h = handles(dict(family=family, length_scale=ell))
    assert h.kernel() == dict(family=family, length_scale=ell)
    rng = np.random.default_rng(n1 + n2)
    x1, x2 = rng.standard_normal(n1) * 2, rng.standard_normal(n2) * 2
    K = to_host(h.se_kernel(to_device(x1), to_device(x2), jitter=0.001 if n1 == n2 else 0.0))
    ref = KX.kernel_ld(family, ell, x1, x2)
    if n1 == n2:
        ref[np.diag_indices(n1)] += KX.LD(0.001)
    err = float(np.abs(K.astype(KX.LD) - ref).max())
    tol = KX.k_tolerance(family, ell)
    print(f"MEASURED se_kernel {family} ell={ell} {n1}x{n2}: max |K - long double| {err:.2e} (bound {tol:.2e})")
    assert K.shape == (n1, n2) and err <= tol


# --------------------------------------------------------------------------------------------- 2. the lower builder ---
@pytest.mark.parametrize("family,ell", [("matern52", 0.7), ("se", 2.5)])
def test_lower_builder(handles, family, ell):
    """Sampler.build_cov() at n = 300: three row blocks of 128, so the triangular enumeration of the block pairs runs (six
    pairs, 24 work-groups).  The lower triangle of L holds S = K + 0.001 I to the operator's bound; the strict upper part of
    the diagonal tiles is exactly 0 (as is everything above: nothing else is ever written there)."""
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    n = 300
    y, th0 = make_responses(n, 4, seed=3)
    h = handles(dict(family=family, length_scale=ell))
    s = Sampler(h, y, th0, seed=5, **FAST)
    s.init()
    s.build_cov()
    s.check()
    L, theta = np.array(s.get("L")), np.array(s.get("theta"))
    s.close()
    ref = KX.kernel_ld(family, ell, theta, theta)
    ref[np.diag_indices(n)] += KX.LD(0.001)
    low = np.tril(np.ones((n, n), dtype=bool))
    err = float(np.abs(L.astype(KX.LD) - ref)[low].max())
    tol = KX.k_tolerance(family, ell)
    print(f"MEASURED lower build {family} ell={ell} n={n}: max |S - long double| {err:.2e} (bound {tol:.2e})")
    assert err <= tol
    for b0 in range(0, n, 128):
        tile = L[b0:b0 + 128, b0:b0 + 128]
        assert (tile[np.triu_indices(tile.shape[0], 1)] == 0.0).all()
    assert (L[~low] == 0.0).all()


# -------------------------------------------------------------------------------------------------- 3. the factor ---
def test_factor_under_matern32(handles):
    """Handle.factor under Matern 3/2, length scale 0.5, n = 200: L L^T against the fp64-rounded kernel_ld + jitter within
    1e-11, the project's bound for n <= 1024"""
    from gpirt_amd.ops import to_device, to_host
    n = 200
    theta = _grid_theta(n, 8)
    h = handles(dict(family="matern32", length_scale=0.5))
    L = to_host(h.factor(to_device(theta)))
    S = KX.kernel_ld("matern32", 0.5, theta, theta)
    S[np.diag_indices(n)] += KX.LD(0.001)
    S = S.astype(np.float64)
    err = float(np.abs(L @ L.T - S).max())
    print(f"MEASURED factor matern32 ell=0.5 n={n}: max |L L^T - S| {err:.2e}")
    assert (np.triu(L, 1) == 0.0).all() and err <= 1e-11


# ---------------------------------------------------------------------------------------------- 4. default identity ---
def test_the_default_kernel_set_explicitly_changes_no_bit(handles):
    from gpirt_amd.ops import to_device, to_host
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    never, explicit = handles(), handles(dict(family="se", length_scale=1.0))
    assert never.kernel() == explicit.kernel() == dict(family="se", length_scale=1.0)
    rng = np.random.default_rng(4)
    x1, x2 = rng.standard_normal(258) * 2, rng.standard_normal(37) * 2
    for a, b in ((x1, x2), (x1[:129], x2[:33])):
        Ka, Kb = (to_host(h.se_kernel(to_device(a), to_device(b))) for h in (never, explicit))
        assert np.array_equal(Ka, Kb)
        assert np.abs(Ka - np.exp(-0.5 * (a[:, None] - b[None, :]) ** 2)).max() <= 4e-16
    theta = _grid_theta(200, 9)
    La, Lb = (to_host(h.factor(to_device(theta))) for h in (never, explicit))
    assert np.array_equal(La, Lb)
    n, m = 96, 7
    y, th0 = make_responses(n, m, seed=6)
    outs = []
    for h in (never, explicit):
        s = Sampler(h, y, th0, preset="fast", seed=21)
        s.init()
        for _ in range(5):
            s.step()
        s.check()
        outs.append([np.array(s.get(k)) for k in ("theta", "beta", "f", "fstar")])
        s.close()
    for xa, xb in zip(*outs):
        assert np.isfinite(xa).all() and np.array_equal(xa, xb)


# -------------------------------------------------------------------------------------------------- 5. draw_fstar ---
FSTAR_CASES = {
    "se_0.7_as_written": ("se", 0.7, dict(fstar_fused=False, kstar_rank=0)),
    "se_0.7_fused": ("se", 0.7, dict(fstar_fused=True, kstar_rank=0)),
    "se_0.7_rank_64": ("se", 0.7, dict(fstar_fused=True, kstar_rank=64)),
    "se_2_rank_48": ("se", 2.0, dict(fstar_fused=True, kstar_rank=48)),
    "matern52_1_as_written": ("matern52", 1.0, dict(fstar_fused=False, kstar_rank=0)),
    "matern52_1_fused": ("matern52", 1.0, dict(fstar_fused=True, kstar_rank=0)),
}


@pytest.mark.parametrize("case", list(FSTAR_CASES))
def test_draw_fstar_against_long_double(handles, case):
    """draw_fstar on the sampler's state after init and one draw_f (n = 150, m = 3: theta is the snapped random init of
    tests/test_gpu_fstar_ranks.py), given the device's own L, against fstar_kernel_exact.

    Tolerances, by the rules of tests/test_gpu_fstar_ranks.py::test_constructed_theta (u = 2^-53).  s = 1 - sqrt(q): the
    solve moves q by 4 n u sqrt(cond(S)) q; forming q adds, for the rank form, (n + 2 r) u Lam^2 (Lam = max_j sum_k |V_jk|: the
    quadratic form cancels) and for the full form n u (a sum of n squares, q <= 1); |d sqrt(q)| <= min(sqrt(dq), dq / sqrt(q)),
    and 2 u for the subtraction.  mean and f*: 8 n u cond(S) relative to max(1, max|ref|).  The NaN cells (s < 0) coincide
    wherever |s| is clear of 0."""
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    family, ell, kw = FSTAR_CASES[case]
    n, m, seed = 150, 3, 5
    y, th0 = make_responses(n, m, seed=3)
    h = handles(dict(family=family, length_scale=ell))
    s = Sampler(h, y, th0, rng="item", seed=seed, theta_stabilise=True, **kw)
    s.init()
    s.draw_f()
    st = {k: np.array(s.get(k)) for k in ("theta", "L", "f", "mu_star")}
    it = s.iteration + 1
    s.draw_fstar()
    s.check()
    out = {k: np.array(s.get(k)) for k in ("s", "mean", "fstar")}
    s.close()
    z = np.asarray(h.item_normals(seed, it, X.ST_FSTAR, 0, m, X.NGRID).T.contiguous().cpu().numpy().T)
    r = kw["kstar_rank"]
    ref = KX.fstar_kernel_exact(family, ell, st["theta"], st["L"], st["f"], st["mu_star"], r, z)
    cond = ref["cond"]
    q = np.maximum(ref["q"].astype(np.float64), 0.0)
    if r > 0:
        lam = float(np.abs(X.cheb_basis(r)[1]).sum(axis=1).max())
        dq = 4 * n * U * np.sqrt(cond) * q + (n + 2 * r) * U * lam ** 2
    else:
        dq = 4 * n * U * np.sqrt(cond) * q + n * U
    tol_s = np.minimum(np.sqrt(dq), dq / np.maximum(np.sqrt(q), 1e-300)) + 2 * U
    s_ref = ref["s"].astype(np.float64)
    err_s = np.abs(out["s"].astype(X.LD) - ref["s"]).astype(np.float64)
    print(f"MEASURED {case}: cond(S) {cond:.2e}  min s {s_ref.min():.3e}  max |s - ref| {err_s.max():.2e}  "
          f"max |s - ref| / tol {(err_s / tol_s).max():.3f}")
    assert np.isfinite(out["s"]).all() and np.isfinite(out["mean"]).all()
    assert (err_s <= tol_s).all(), (float(err_s.max()), int(np.argmax(err_s / tol_s)))
    clear = np.abs(s_ref) > 1e-9
    nan_dev, nan_ref = np.isnan(out["fstar"]), np.isnan(ref["fstar"].astype(np.float64))
    assert np.array_equal(nan_dev[clear], nan_ref[clear])
    tol = 8 * n * U * cond
    for k in ("mean", "fstar"):
        rk = ref[k].astype(np.float64)
        ok = ~(np.isnan(rk) | np.isnan(out[k]))
        e = float(np.abs(out[k].astype(X.LD) - ref[k])[ok].max()) / max(1.0, float(np.abs(rk[ok]).max()))
        print(f"MEASURED {case}: |{k} - ref| {e:.2e} (tolerance {tol:.2e})")
        assert e <= tol


# ----------------------------------------------------------------------------------------------------- 6. refusals ---
def test_refusals_on_the_device(handles):
    from gpirt_amd import _lib
    from gpirt_amd.distributed import ShardedSampler
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(64, 5, seed=4)
    h = handles()
    s = Sampler(h, y, th0, seed=1, **FAST)
    with pytest.raises(_lib.GpirtError) as ei:                        # a live sampler keeps the kernel it was created under
        h.set_kernel("matern52")
    assert ei.value.code == _lib.E_ARG and "alive" in str(ei.value)
    assert h.kernel() == dict(family="se", length_scale=1.0)
    s.close()
    h.set_kernel(dict(family="se", length_scale=0.5))
    with pytest.raises(_lib.GpirtError) as ei:                        # the rank's certificate, in the message
        Sampler(h, y, th0, seed=1, kstar_rank=64, **FAST)
    cert = KX.certificate("se", 0.5, 64)
    assert ei.value.code == _lib.E_ARG and f"{cert:.3g}" in str(ei.value) and f"passes is {KX.min_rank('se', 0.5)}" in str(ei.value)
    s = Sampler(h, y, th0, seed=1, kstar_rank=KX.min_rank("se", 0.5), **FAST)      # ... and the rank it names is taken
    s.close()
    h.set_kernel("matern32")                                          # (the refused creations left no sampler behind)
    with pytest.raises(_lib.GpirtError) as ei:
        Sampler(h, y, th0, seed=1, kstar_rank=64, **FAST)
    assert ei.value.code == _lib.E_ARG and "Matern" in str(ei.value)
    with pytest.raises(_lib.GpirtError) as ei:
        Sampler(h, y, th0, seed=1, kernel_fp32=True, **FAST)
    assert ei.value.code == _lib.E_ARG and "kernel_fp32" in str(ei.value) and "default kernel" in str(ei.value)
    with pytest.raises(_lib.GpirtError):
        h.set_kernel(dict(family="se", length_scale=0.001))
    assert h.kernel() == dict(family="matern32", length_scale=1.0)

    def factory(yl, th, pm, ps, st, item0, m_total):
        return Sampler(h, yl, th, pm, ps, st, rng="item", seed=77, item0=item0, m_total=m_total)

    with pytest.raises(ValueError) as ei:
        ShardedSampler(factory, y, th0, dist=None)
    assert "default kernel" in str(ei.value)
    h.set_kernel(None)                                                # (the refused engine was closed)
    ss = ShardedSampler(factory, y, th0, dist=None)
    ss.engine.close()
    s = Sampler(h, y, th0, seed=1, kernel_fp32=True, **FAST)          # under the default kernel: as ever
    s.init()
    s.check()
    s.close()


# ------------------------------------------------------------------------------------------------------- 7. chains ---
def _chain(h, y, th0, iters, **kw):
    from gpirt_amd.sampler import Sampler
    s = Sampler(h, y, th0, **kw)
    s.init()
    for _ in range(iters):
        s.step()
    s.check()
    out = {k: np.array(s.get(k)) for k in ("theta", "beta", "f", "fstar")}
    s.close()
    return out


def test_chain_under_matern52(handles):
    """Matern 5/2, length scale 0.7: n = 120, m = 10, 30 iterations under the item RNG -- finite, theta on the grid, check()
    clean, two runs byte-identical and different from the default kernel's chain"""
    from gpirt_amd.synthetic import make_responses
    n, m, iters = 120, 10, 30
    y, th0 = make_responses(n, m, seed=12)
    kern = dict(family="matern52", length_scale=0.7)
    a = _chain(handles(kern), y, th0, iters, seed=31, **FAST)
    b = _chain(handles(kern), y, th0, iters, seed=31, **FAST)
    d = _chain(handles(), y, th0, iters, seed=31, **FAST)
    for k in a:
        assert np.isfinite(a[k]).all() and np.array_equal(a[k], b[k]), k
    kk = np.rint((a["theta"] + 5.0) * 100.0)
    assert (kk >= 0).all() and (kk <= 1000).all() and np.array_equal(-5.0 + kk * 0.01, a["theta"])
    assert not np.array_equal(a["f"], d["f"]) and not np.array_equal(a["fstar"], d["fstar"])


def test_chain_under_matern52_replays_the_r_stream(handles):
    """n = 64, m = 5, three iterations under rng="reference": two runs byte-identical, R's stream at the same position"""
    from gpirt_amd.ops import RStream
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(64, 5, seed=13)
    kern = dict(family="matern52", length_scale=0.7)
    outs = []
    for _ in range(2):
        rs = RStream(2718)
        out = _chain(handles(kern), y, th0, 3, rng="reference", rstream=rs)
        outs.append((out, rs.state()))
    (a, sa), (b, sb) = outs
    for k in a:
        assert np.isfinite(a[k]).all() and np.array_equal(a[k], b[k]), k
    assert np.array_equal(sa[0], sb[0]) and sa[1] == sb[1]
    fresh = RStream(2718).state()
    assert not (np.array_equal(sa[0], fresh[0]) and sa[1] == fresh[1])


def test_analysis_blocks_run_under_matern52(handles):
    """the blocks read the sampler's arrays and know nothing of the kernel: the PPC and the shape posteriors accumulate and
    return finite output"""
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    n, m, draws = 120, 10, 6
    y, th0 = make_responses(n, m, seed=12)
    s = Sampler(handles(dict(family="matern52", length_scale=0.7)), y, th0, seed=31, **FAST)
    s.init()
    s.ppc_enable()
    s.shape_enable()
    for _ in range(draws):
        s.step()
        s.ppc_accumulate()
        s.shape_accumulate()
    s.check()
    p = s.ppc()
    for unit in ("item", "respondent"):
        assert (p[unit]["draws"] == draws).all() and (p[unit]["nonfinite"] == 0).all()
        assert np.isfinite(p[unit]["rep_yes_mean"]).all() and np.isfinite(p[unit]["dev_rep_mean"]).all()
    assert (s.shape_get("draws") == draws).all() and (s.shape_get("nonfinite") == 0).all()
    assert s.shape_get("counts")[0] == draws
    assert np.isfinite(s.shape_get("info")).all() and np.isfinite(s.shape_get("ti")).all()
    s.close()


# --------------------------------------------------------------------------------------------------- 8. kernel.run ---
def test_run_with_the_default_kernel_is_gpirtmcmc(handle):
    """kernel.run(kernel=None) is the stage loop of the whole call: the draws of gpirtMCMC(preset="fast") bit for bit, the
    IRFs as tests/test_gpu_sampler.py holds them (1e-9)"""
    from gpirt_amd import gpirtMCMC, kernel as K
    from gpirt_amd.synthetic import make_responses
    n, m, S, B = 60, 8, 20, 5
    y, _ = make_responses(n, m, seed=15)
    got = K.run(y, S, B, seed=9)
    ref = gpirtMCMC(y, S, B, vote_codes=CODES, preset="fast", seed=9)
    assert got["kernel"] == dict(family="se", length_scale=1.0) and got["kstar_rank"] == 64 and got["chains"] == 1
    for k in ("theta", "beta", "f"):
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), k
    err = float(np.abs(got["IRFs"] - ref["IRFs"]).max())
    print(f"MEASURED kernel.run against gpirtMCMC: max |IRFs - IRFs| {err:.2e}")
    assert err <= 1e-9
    assert got["loo"]["T"] == S and np.isfinite(got["loo"]["elpd_loo"])
    off = K.run(y, 4, 1, seed=9, loo=False, store_draws=("theta",))
    assert off["loo"] is None and off["f"] is None and off["beta"] is None and off["theta"].shape == (5, n)
    assert np.array_equal(off["theta"][0], ref["theta"][0])


# ----------------------------------------------------------------------------------------------- 9. kernel.compare ---
def test_compare_ranks_the_kernels_by_elpd_loo(handles):
    from gpirt_amd import kernel as K, loo as LO
    from gpirt_amd.synthetic import make_responses
    n, m, S, B, chains = 60, 8, 40, 10, 2
    y, _ = make_responses(n, m, seed=16)
    kernels = ["se", dict(family="matern52", length_scale=1.0), dict(family="se", length_scale=0.5)]
    h = handles("matern32")
    rows = K.compare(y, kernels, S, B, chains=chains, seed=4, handle=h)
    assert h.kernel() == dict(family="matern32", length_scale=1.0)          # the caller's handle gets its kernel back
    assert sorted(r["index"] for r in rows) == [0, 1, 2]
    elpd = [r["elpd_loo"] for r in rows]
    assert elpd == sorted(elpd, reverse=True)
    assert rows[0]["elpd_diff"] == 0.0 and rows[0]["se_diff"] == 0.0 and all(r["elpd_diff"] <= 0.0 for r in rows)
    byhand = [K.run(y, S, B, chains=chains, seed=4, kernel=k, store_draws=False) for k in kernels]
    best = byhand[rows[0]["index"]]
    for r in rows:
        one = byhand[r["index"]]
        d = LO.compare(one["loo"], best["loo"])
        print(f"MEASURED compare {one['kernel']}: rank {one['kstar_rank']}  elpd_loo {one['loo']['elpd_loo']:.3f}  "
              f"elpd_diff {d['elpd_diff']:.3f} +- {d['se_diff']:.3f}  k_bad {r['k_bad']}  max_rhat {r['max_rhat']:.3f}")
        assert r["kernel"] == one["kernel"] == K.as_dict(kernels[r["index"]])
        assert r["kstar_rank"] == one["kstar_rank"]
        assert r["elpd_loo"] == one["loo"]["elpd_loo"] and r["se_elpd_loo"] == one["loo"]["se_elpd_loo"]
        assert r["elpd_diff"] == d["elpd_diff"] and (r["se_diff"] == d["se_diff"]) and r["n_obs"] == d["n_obs"]
        assert r["k_bad"] == one["loo"]["k_bad"] + one["loo"]["k_very_bad"]
        assert r["max_rhat"] == K.max_rhat(one["diagnostics"]) or (np.isnan(r["max_rhat"]) and np.isnan(K.max_rhat(one["diagnostics"])))
        assert one["loo"]["T"] == chains * S and one["loo"]["chains"] == chains
    ranks = {r["index"]: r["kstar_rank"] for r in rows}
    assert ranks == {0: 64, 1: 0, 2: KX.min_rank("se", 0.5)}
