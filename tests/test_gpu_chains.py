"""Several chains on the device (include/gpirt_hip.h gpirt_mcmc_chains, gpirt_chains_combine, GPIRT_SUM_DIAG) against the
single-chain runs and against NumPy over the stored draws: the chains ARE the single-chain runs, the pooled summaries equal
a summary over the concatenated draws, split-R-hat / ESS / MCSE and their per-block scalars, the reflection alignment
(automatic and forced), DIAG leaving every existing summary alone, the argument checks, a hang-guard rollback, one chain
per rank, and a multi-block size with f."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = dict(yea=[1], nay=[-1], missing=[None])
ALL = ("waic", "pred", "f")


def close(got, want, rtol, what, scale=0.0):
    """NaN and +-inf where want has them; elsewhere |got - want| <= rtol max(|want|, scale)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), what
    assert np.isfinite(got[fin]).all(), what
    if fin.any():
        s = np.broadcast_to(np.asarray(scale, dtype=np.float64), want.shape)[fin]
        err = np.abs(got[fin] - want[fin]) / np.maximum(np.maximum(np.abs(want[fin]), s), 1e-300)
        assert err.max() <= rtol, f"{what}: relative error {err.max():.3e}"


def ref_summary(y, theta, beta, f):
    """From S draws: theta (S, n), beta (2, m, S), f (n, m, S) (the summaries of tests/test_gpu_summary.py)."""
    S = theta.shape[0]
    mu = beta[0][None, :, :] + theta.T[:, None, :] * beta[1][None, :, :]
    g = f + mu
    e = np.exp(-np.abs(g))
    p = np.where(g >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    ll = -(np.log1p(e) + np.maximum(-(y[:, :, None] * g), 0.0))
    mx = ll.max(axis=2)
    lppd = mx + np.log(np.exp(ll - mx[:, :, None]).sum(axis=2)) - np.log(S)
    obs = ~np.isnan(y)
    nan = np.full(y.shape, np.nan)
    out = dict(p_yes=p.mean(axis=2), lppd=np.where(obs, lppd, nan), p_waic=np.where(obs, ll.var(axis=2, ddof=1), nan),
               f_mean=f.mean(axis=2), f_var=f.var(axis=2, ddof=1), theta_mean=theta.mean(axis=0),
               theta_var=theta.var(axis=0, ddof=1), beta_mean=beta.mean(axis=2), beta_var=beta.var(axis=2, ddof=1))
    lp, pw = out["lppd"][obs], out["p_waic"][obs]
    el = lp - pw
    tot = dict(lppd=lp.sum(), p_waic=pw.sum(), elpd_waic=el.sum(), waic=-2.0 * el.sum(), n_obs=float(obs.sum()),
               draws=float(S), elpd_mean=el.mean(), elpd_ss=((el - el.mean()) ** 2).sum(),
               se_elpd_waic=np.sqrt(obs.sum() * el.var(ddof=1)))
    return out, tot


def check_pooled(summary, y, th, be, ff, signs):
    """th (C, S, n), be (C, 2, m, S), ff (C, n, m, S): the pooled summary equals one over the concatenated draws, with the
    reflected chains' theta and beta slope negated."""
    sg = np.asarray(signs, dtype=np.float64)
    th = th * sg[:, None, None]
    be = be.copy()
    be[:, 1] *= sg[:, None, None]
    C_, S = th.shape[0], th.shape[1]
    want, tot = ref_summary(y, th.reshape(C_ * S, -1), np.concatenate(list(be), axis=2), np.concatenate(list(ff), axis=2))
    mag = dict(f_mean=np.abs(ff).max(axis=(0, 3)), theta_mean=np.abs(th).max(axis=(0, 1)), beta_mean=np.abs(be).max(axis=(0, 3)))
    for k, v in want.items():
        if k in summary:
            rt = 1e-10 if k in ("p_yes", "lppd", "p_waic", "f_var") else 1e-12
            close(summary[k], v, rt, k, mag.get(k, 1e-6 * max(1.0, np.nanmax(np.abs(v)))))
    if "totals" in summary:
        for k, v in tot.items():
            close(summary["totals"][k], v, 1e-9, "totals." + k)


def check_diag(diag, th, be, ff, signs, fo):
    """th (C, S, n), be (C, 2, m, S), ff (C, n, m, S) against chains.diagnostics_from_draws."""
    from gpirt_amd.chains import block_scalars, diagnostics_from_draws
    sg = np.asarray(signs, dtype=np.float64)
    blocks = dict(theta=diagnostics_from_draws(th, signs=sg),
                  beta=diagnostics_from_draws(np.moveaxis(be, 3, 1), signs=sg, reflect=np.array([[False], [True]])))
    if fo:
        blocks["f"] = diagnostics_from_draws(np.moveaxis(ff, 3, 1))
    for b, d in blocks.items():
        close(diag[f"{b}_rhat"], d["rhat"], 1e-10, b + "_rhat", 1.0)
        close(diag[f"{b}_ess"], d["ess"], 1e-10, b + "_ess", 1e-3)
        close(diag[f"{b}_mcse"], d["mcse"], 1e-10, b + "_mcse", 1e-6)
        want = block_scalars(d["rhat"], d["ess"])
        got = diag["scalars"][b]
        for k in ("n_rhat_high", "n_rhat_nan", "n_ess_nan"):
            assert got[k] == want[k], (b, k, got[k], want[k])
        close(got["max_rhat"], want["max_rhat"], 1e-10, b + ".max_rhat", 1.0)
        close(got["min_ess"], want["min_ess"], 1e-10, b + ".min_ess", 1e-3)
    if not fo:
        assert np.isnan(diag["scalars"]["f"]["max_rhat"]) and "f_rhat" not in diag


def logit(p):
    with np.errstate(divide="ignore"):
        return np.log(p) - np.log1p(-p)


def _data(n, m, seed=11):
    from gpirt_amd.synthetic import make_responses
    from gpirt_amd.response_matrix import as_response_matrix
    y, th0 = make_responses(n, m, seed=seed)
    return np.asarray(as_response_matrix(y, CODES), dtype=np.float64), th0


def test_chains_are_the_single_chain_runs():
    from gpirt_amd import _lib, gpirtMCMC
    y, th0 = _data(300, 40)
    C_, S, B = 3, 4, 2
    inits = np.stack([th0, -th0, np.roll(th0, 7)])
    res = gpirtMCMC(y, S, B, vote_codes=CODES, theta_init=inits, rng="item", seed=29, theta_stabilise=True, chains=C_)
    assert res["theta"].shape == (C_, S + 1, 300) and res["beta"].shape == (C_, 2, 40, S + 1)
    assert res["f"].shape == (C_, 300, 40, S + 1)
    for c in range(C_):
        one = gpirtMCMC(y, S, B, vote_codes=CODES, theta_init=inits[c], rng="item", seed=_lib.chain_seed(29, c),
                        theta_stabilise=True)
        for k in ("theta", "beta", "f"):
            assert np.array_equal(res[k][c], one[k]), (c, k)


def _chains_and_singles(n, m, C_, S, B, inits, align, summaries=ALL, seed=5):
    from gpirt_amd import _lib, gpirtMCMC
    y, _ = _data(n, m)
    res = gpirtMCMC(y, S, B, vote_codes=CODES, theta_init=inits, rng="item", seed=seed, theta_stabilise=True, chains=C_,
                    align=align, summaries=summaries)
    irfs = [gpirtMCMC(y, S, B, vote_codes=CODES, theta_init=inits[c], rng="item", seed=_lib.chain_seed(seed, c),
                      theta_stabilise=True, store_draws=False, summaries=("waic",))["IRFs"] for c in range(C_)]
    return y, res, irfs


@pytest.mark.parametrize("S,align,flip", [(10, True, False), (9, False, False), (8, True, True)])
def test_pooled_summaries_and_diagnostics_match_numpy(S, align, flip):
    """S even and odd, align on and off; flip: chain 1 starts at -theta0, and the automatic flag is the NumPy rule."""
    from gpirt_amd.chains import reflection_signs
    n, m, C_, B = 300, 40, 3, 2
    _, th0 = _data(n, m)
    inits = np.stack([th0, -th0 if flip else np.roll(th0, 3), np.roll(th0, 11)])
    y, res, irfs = _chains_and_singles(n, m, C_, S, B, inits, align)
    th, be, ff = res["theta"][:, 1:], res["beta"][..., 1:], res["f"][..., 1:]
    dg = res["diagnostics"]
    signs = reflection_signs(th.mean(axis=1)) if align else np.ones(C_, dtype=int)
    assert np.array_equal(dg["reflected"], signs < 0)
    if flip:
        print("reflected:", dg["reflected"])
    check_pooled(res["summary"], y, th, be, ff, signs)
    check_diag(dg, th, be, ff, signs, True)
    check_irfs(res["IRFs"], irfs, signs)


def check_irfs(got, irfs, signs):
    """The pooled IRFs against plogis(mean_c logit(IRF_c)), reflected chains reversed along the grid.  IRF_c is
    plogis(irf_sum_c / S) rounded, so logit(IRF_c) recovers the sum only where IRF_c is away from 0 and 1: the cells where
    every chain's IRF lies in [1e-6, 1 - 1e-6] (the IRF sums themselves are checked exactly on the stage API below)."""
    lg = [logit(ir)[::-1] if s < 0 else logit(ir) for ir, s in zip(irfs, signs)]
    ok = np.all([(ir >= 1e-6) & (ir <= 1 - 1e-6) for ir in (x[::-1] if s < 0 else x for x, s in zip(irfs, signs))], axis=0)
    assert ok.mean() > 0.5
    want = 1.0 / (1.0 + np.exp(-sum(lg) / len(lg)))
    assert np.abs(got[ok] - want[ok]).max() <= 1e-9
    assert ((got >= 0) & (got <= 1)).all()


def _stage_chain(handle, y, th0, seed, S, B, parts, keep=True):
    """One chain on the stage API (as run_distributed runs it), its draws and its sampler (summaries on, DIAG planned)."""
    from gpirt_amd import Sampler, _lib
    s = Sampler(handle, y, th0, rng="item", seed=seed, theta_stabilise=True)
    s.init()
    s.summary_enable(_lib.summary_parts(parts) | _lib.SUM_DIAG, planned_draws=S)
    th, be, ff = [], [], []
    for it in range(S + B):
        s.step()
        if it >= B:
            s.accumulate_irf()
            s.summary_accumulate()
            if keep:
                th.append(s.get("theta")); be.append(s.get("beta")); ff.append(s.get("f"))
    s.check()
    return s, (np.stack(th) if keep else None), (np.stack(be, axis=2) if keep else None), (np.stack(ff, axis=2) if keep else None)


def test_forced_signs_reflect_chain_one(handle):
    from gpirt_amd import _lib, chains
    y, th0 = _data(200, 24)
    S, B = 8, 1
    runs = [_stage_chain(handle, y, t, _lib.chain_seed(3, c), S, B, ALL) for c, t in enumerate((th0, np.roll(th0, 5)))]
    samplers = [r[0] for r in runs]
    irf_sum = [s.get("irf_sum") for s in samplers]
    out = chains.combine(handle, samplers, signs=[1, -1])
    th = np.stack([r[1] for r in runs]); be = np.stack([r[2] for r in runs]); ff = np.stack([r[3] for r in runs])
    assert out["diagnostics"]["reflected"].tolist() == [False, True]
    check_pooled(out["summary"], y, th, be, ff, [1, -1])
    check_diag(out["diagnostics"], th, be, ff, [1, -1], True)
    want = (irf_sum[0] + irf_sum[1][::-1]) / (2 * S)
    close(out["IRFs"], 1.0 / (1.0 + np.exp(-want)), 1e-12, "IRFs", 1e-3)
    # align off and no signs: nothing is reflected
    out0 = chains.combine(handle, samplers, align=False)
    assert not out0["diagnostics"]["reflected"].any()
    check_pooled(out0["summary"], y, th, be, ff, [1, 1])
    for s in samplers:
        s.close()


def test_diag_leaves_existing_summaries_unchanged(handle):
    """Every existing summary output and the chain, bit-identical with DIAG on and off; one chain through
    gpirt_mcmc_chains gives gpirt_mcmc_summary's summaries bit for bit."""
    from gpirt_amd import Sampler, _lib, gpirtMCMC
    y, th0 = _data(257, 9)
    S = 5
    out = []
    for planned in (None, S):
        s = Sampler(handle, y, th0, rng="item", seed=41, theta_stabilise=True)
        s.init()
        parts = _lib.summary_parts(ALL) | (_lib.SUM_DIAG if planned else 0)
        s.summary_enable(parts, planned_draws=planned)
        for _ in range(S):
            s.step()
            s.summary_accumulate()
        s.check()
        out.append((s.summary(), {k: s.get(k) for k in ("theta", "beta", "f", "mu")}))
        s.close()
    (a, ca), (b, cb) = out
    for k in ca:
        assert np.array_equal(ca[k], cb[k]), k
    assert a["totals"] == b["totals"]
    for k in a:
        if k != "totals":
            assert np.array_equal(a[k], b[k], equal_nan=True), k
    one = gpirtMCMC(y, S, 1, vote_codes=CODES, theta_init=th0, rng="item", seed=8, summaries=ALL)
    ch = gpirtMCMC(y, S, 1, vote_codes=CODES, theta_init=th0[None], rng="item", seed=8, summaries=ALL, chains=1)
    for k in ("theta", "beta", "f"):
        assert np.array_equal(one[k], ch[k][0]), k
    assert np.array_equal(one["IRFs"], ch["IRFs"])
    assert one["summary"]["totals"] == ch["summary"]["totals"]
    for k, v in one["summary"].items():
        if k != "totals":
            assert np.array_equal(v, ch["summary"][k], equal_nan=True), k


def test_argument_checks(handle):
    import ctypes as C
    from gpirt_amd import Sampler, _lib, chains
    lib = _lib.load()
    y, th0 = _data(90, 6)
    s = Sampler(handle, y, th0, rng="item", seed=2, theta_stabilise=True)
    s.init()
    s.summary_enable(("waic",) , planned_draws=3)          # no DIAG bit: planned is only recorded
    with pytest.raises(_lib.GpirtError):
        s.summary_enable(_lib.SUM_DIAG | _lib.SUM_WAIC, planned_draws=0)
    assert lib.gpirt_sampler_summary_enable(s._s, _lib.SUM_DIAG) == _lib.E_ARG     # only enable_planned takes DIAG
    s.summary_enable(_lib.SUM_DIAG | _lib.SUM_WAIC, planned_draws=3)
    for _ in range(2):
        s.step()
        s.summary_accumulate()
    t = Sampler(handle, y, th0, rng="item", seed=3, theta_stabilise=True)
    t.init()
    t.summary_enable(_lib.SUM_DIAG | _lib.SUM_WAIC, planned_draws=3)
    for _ in range(3):
        t.step()
        t.summary_accumulate()
    with pytest.raises(_lib.GpirtError, match="planned"):                # early read: 2 of 3 draws
        chains.combine(handle, [s, s])
    with pytest.raises(_lib.GpirtError, match="differs"):                # headers differ (draws 2 and 3)
        chains.combine(handle, [t, s])
    s.step()
    s.summary_accumulate()
    with pytest.raises(_lib.GpirtError, match="planned"):                # a fourth draw of three
        s.step()
        s.summary_accumulate()
    out = chains.combine(handle, [s, t])
    assert out["summary"]["totals"]["draws"] == 6
    with pytest.raises(_lib.GpirtError):
        chains.combine(handle, [s, t], signs=[1, 0])
    s.close()
    t.close()
    # gpirt_mcmc_summary still refuses the DIAG bit
    from gpirt_amd import gpirtMCMC
    with pytest.raises(_lib.GpirtError):
        gpirtMCMC(y, 2, 0, vote_codes=CODES, theta_init=th0, rng="item", summaries=_lib.SUM_DIAG | _lib.SUM_WAIC)
    st = C.c_void_p()
    assert lib.gpirt_chains_combine(handle.ptr, 1, C.byref(st), None, 1, None, None, None) == _lib.E_ARG


def test_pooled_results_survive_a_rollback():
    from gpirt_amd import _lib, gpirtMCMC
    lib = _lib.load()
    y, th0 = _data(2600, 12)
    inits = np.stack([th0, np.roll(th0, 1)])
    kw = dict(vote_codes=CODES, theta_init=inits, rng="item", seed=4, theta_stabilise=True, chains=2, summaries=ALL,
              store_draws=False)
    ref = gpirtMCMC(y, 4, 1, **kw)
    assert lib.gpirt_debug_last_mcmc_fallbacks() == 0
    _lib.check(lib.gpirt_debug_trip_guard(None, 9))                    # the 9th factorisation: in chain 1
    got = gpirtMCMC(y, 4, 1, **kw)
    assert lib.gpirt_debug_last_mcmc_fallbacks() == 1
    assert got["summary"]["totals"]["draws"] == 8
    for k, v in ref["summary"].items():
        if k == "totals":
            for t, x in v.items():
                close(got["summary"]["totals"][t], x, 1e-10, t)
        else:
            close(got["summary"][k], v, 1e-10, k, max(1.0, np.nanmax(np.abs(v))))
    for k, v in ref["diagnostics"].items():
        if k.endswith(("rhat", "ess", "mcse")):
            close(got["diagnostics"][k], v, 1e-8, k, max(1.0, np.nanmax(np.abs(v[np.isfinite(v)]))))
    assert np.array_equal(got["diagnostics"]["reflected"], ref["diagnostics"]["reflected"])
    close(got["IRFs"], ref["IRFs"], 1e-10, "IRFs", 1.0)


def _run_rank(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gpirt_amd.chains import run_distributed
    y, th0 = _data(300, 22)
    inits = np.stack([th0, np.roll(th0, 9)])
    out = run_distributed(y, 6, 2, inits, dist=dist, seed=77, summaries=("waic", "pred"), theta_stabilise=True)
    if rank == 0:
        flat = {"s_" + k: v for k, v in out["summary"].items() if k != "totals"}
        flat.update({"t_" + k: v for k, v in out["summary"]["totals"].items()})
        flat.update({"d_" + k: v for k, v in out["diagnostics"].items() if k != "scalars"})
        np.savez(os.path.join(outdir, "chains_dist.npz"), IRFs=out["IRFs"], **flat)
    dist.destroy_process_group()


def test_one_chain_per_rank_matches_gpirt_mcmc_chains(tmp_path):
    import torch.multiprocessing as mp
    from gpirt_amd import gpirtMCMC
    port = 29850 + (os.getpid() % 1000)
    mp.spawn(_run_rank, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    got = np.load(tmp_path / "chains_dist.npz")
    y, th0 = _data(300, 22)
    inits = np.stack([th0, np.roll(th0, 9)])
    ref = gpirtMCMC(y, 6, 2, vote_codes=CODES, theta_init=inits, rng="item", seed=77, theta_stabilise=True, chains=2,
                    summaries=("waic", "pred"), store_draws=False)
    assert np.array_equal(got["IRFs"], ref["IRFs"])
    for k, v in ref["summary"].items():
        if k == "totals":
            for t, x in v.items():
                assert float(got["t_" + t]) == x or (np.isnan(x) and np.isnan(float(got["t_" + t]))), t
        else:
            assert np.array_equal(got["s_" + k], v, equal_nan=True), k
    for k, v in ref["diagnostics"].items():
        if k != "scalars":
            assert np.array_equal(got["d_" + k], v, equal_nan=True), k


def test_multi_block_size_with_f():
    """2048 x 256 with f stored: f's R-hat and ESS where the accumulate and combine kernels run multi-block grids."""
    n, m, C_, S, B = 2048, 256, 2, 8, 1
    _, th0 = _data(n, m)
    inits = np.stack([th0, np.roll(th0, 17)])
    y, res, irfs = _chains_and_singles(n, m, C_, S, B, inits, True)
    th, be, ff = res["theta"][:, 1:], res["beta"][..., 1:], res["f"][..., 1:]
    signs = np.where(res["diagnostics"]["reflected"], -1, 1)
    check_pooled(res["summary"], y, th, be, ff, signs)
    check_diag(res["diagnostics"], th, be, ff, signs, True)
    check_irfs(res["IRFs"], irfs, signs)


def _same(a, b, what):
    """Two results of the same chains: every array bit for bit (NaN where the other has NaN), every scalar equal."""
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _same(a[k], b[k], f"{what}.{k}")
    elif a is None:
        assert b is None, what
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), what


def _mcmc_run_empty(y, inits, S, B, seed, priors, chains):
    """gpirt_mcmc_run through ctypes with an empty gpirt_run, the fast preset and every pooled part: the stored draws chain-major
    in gpirt_mcmc's layout, the IRFs, the pooled arrays by name, the totals and the diagnostics."""
    import ctypes as C
    from gpirt_amd import _lib
    from gpirt_amd import chains as CH
    lib = _lib.load()
    dp = C.POINTER(C.c_double)
    a = lambda x: x.ctypes.data_as(dp)                                           # noqa: E731
    n, m = y.shape
    yf, th0 = np.asfortranarray(y), np.ascontiguousarray(inits)
    pm, ps, st = (np.asfortranarray(p, dtype=np.float64) for p in priors)
    th, be, ff = np.empty((chains, n, S + 1)), np.empty((chains, S + 1, m, 2)), np.empty((chains, S + 1, m, n))
    irf = np.empty((_lib.NGRID, m), order="F")
    o = _lib.fast_options()
    o.seed = seed
    sm = _lib.Summary()
    sm.parts = _lib.summary_parts(ALL) | _lib.SUM_THETA_BETA
    shapes = dict(theta_mean=(n,), theta_var=(n,), beta_mean=(2, m), beta_var=(2, m))
    pooled = {k: np.empty(shapes.get(k, (n, m)), order="F") for k in ("theta_mean", "theta_var", "beta_mean", "beta_var", "p_yes",
                                                                      "lppd", "p_waic", "f_mean", "f_var")}
    for k, v in pooled.items():
        setattr(sm, "h_" + k, a(v))
    d, darr = CH.diag_struct(sm.parts, n, m, chains)
    run = _lib.Run()
    _lib.check(lib.gpirt_mcmc_run(a(yf), n, m, a(th0), chains, S, B, a(pm), a(ps), a(st), C.byref(o), 1, _lib.TICK_FN(0), None,
                                  a(th), a(be), a(ff), a(irf), C.byref(sm), C.byref(d), C.byref(run)))
    return dict(theta=th.transpose(0, 2, 1), beta=be.transpose(0, 3, 2, 1), f=ff.transpose(0, 3, 2, 1), IRFs=irf, pooled=pooled,
                totals=list(sm.totals), diagnostics=CH.diag_result(d, darr))


def test_mcmc_run_is_mcmc_chains_and_the_analyses_leave_the_chains_alone():
    """gpirt_mcmc_run with an empty gpirt_run against gpirt_mcmc_chains -- draws, IRFs, pooled summary and diagnostics bit for
    bit, as two calls with one seed are everywhere in this file --; then with ppc, ranks, shape and loo all set: the same
    draws, IRFs and pooled summary, ranks over chains x S draws, and PSIS-LOO over one chain (chain 0's state alone, no
    merge) and over two (chain 1 merged into it)."""
    from gpirt_amd import _lib, gpirtMCMC
    n, m, C_, S, B = 8, 3, 2, 4, 1
    y = np.array([[1, -1, 1], [-1, 1, 1], [1, 1, -1], [-1, -1, 1], [1, np.nan, -1], [1, 1, 1], [-1, 1, -1], [1, -1, -1]],
                 dtype=np.float64)
    inits = np.round(np.random.default_rng(3).normal(size=(C_, n)), 2)
    priors = (np.zeros((2, m)), np.full((2, m), 3.0), np.full((2, m), 0.1))
    kw = dict(vote_codes=CODES, beta_prior_means=priors[0], beta_prior_sds=priors[1], beta_proposal_sds=priors[2], preset="fast",
              seed=17, summaries=ALL)
    ref = gpirtMCMC(y, S, B, theta_init=inits, chains=C_, **kw)
    empty = _mcmc_run_empty(y, inits, S, B, 17, priors, C_)
    for k in ("theta", "beta", "f", "IRFs", "diagnostics"):
        _same(empty[k], ref[k], "empty run: " + k)
    _same(empty["pooled"], {k: v for k, v in ref["summary"].items() if k != "totals"}, "empty run: summary")
    assert dict(zip(_lib.SUM_TOTALS, empty["totals"])) == ref["summary"]["totals"]
    every = dict(ppc=True, ranks=True, shape=True, loo=True)
    full = gpirtMCMC(y, S, B, theta_init=inits, chains=C_, **every, **kw)
    for k in ("theta", "beta", "f", "IRFs", "summary"):
        _same(full[k], ref[k], k)
    assert full["ranks"]["draws"] == C_ * S and full["ranks"]["skipped_draws"] == 0
    assert full["ppc"]["totals"]["draws"] == C_ * S and (full["shape"]["draws"] == C_ * S).all()
    lo = full["loo"]
    assert (lo["T"], lo["M"], lo["draws"], lo["chains"], lo["cells_incomplete"]) == (C_ * S, 1, C_ * S, C_, 0)
    assert lo["n_obs"] == 23 and (lo["raw"]["count"][~np.isnan(y)] == C_ * S).all()
    one = gpirtMCMC(y, S, B, theta_init=inits[:1], chains=1, **every, **kw)
    for k in ("theta", "beta", "f"):
        _same(one[k][0], ref[k][0], k + " of chain 0")
    lo = one["loo"]
    assert (lo["T"], lo["M"], lo["draws"], lo["chains"], lo["cells_incomplete"]) == (S, 0, S, 1, 0)
    assert lo["n_obs"] == 23 and (lo["raw"]["count"][~np.isnan(y)] == S).all() and one["ranks"]["draws"] == S
