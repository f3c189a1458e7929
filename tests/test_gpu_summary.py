"""Posterior summaries on the device (csrc/summary.hip; include/gpirt_hip.h gpirt_sampler_summary_*, gpirt_mcmc_summary)
against NumPy from the stored draws: p_yes, lppd, p_waic, f / theta / beta moments and the WAIC totals; the chain itself
untouched by them; a hang-guard rollback that counts no iteration twice; the metric size; the edges; held-out votes; two
ranks on one card."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = dict(yea=[1], nay=[-1], missing=[None])
ALL = ("waic", "pred", "f")
CELL = ("p_yes", "lppd", "p_waic", "f_mean", "f_var")
TB = ("theta_mean", "theta_var", "beta_mean", "beta_var")


def ref_summary(y, theta, beta, f, mu=None):
    """From S draws: theta (S, n), beta (2, m, S), f (n, m, S); mu (n, m, S) or rebuilt as [1, theta_s] beta_s."""
    S = theta.shape[0]
    if mu is None:
        mu = beta[0][None, :, :] + theta.T[:, None, :] * beta[1][None, :, :]
    g = f + mu
    e = np.exp(-np.abs(g))
    p = np.where(g >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    a = y[:, :, None] * g
    ll = -(np.log1p(e) + np.maximum(-a, 0.0))
    mx = ll.max(axis=2)
    lppd = mx + np.log(np.exp(ll - mx[:, :, None]).sum(axis=2)) - np.log(S)
    obs = ~np.isnan(y)
    nan = np.full(y.shape, np.nan)
    var = (lambda x, ax: x.var(axis=ax, ddof=1)) if S >= 2 else (lambda x, ax: np.full(x.shape[:ax] + x.shape[ax + 1:], np.nan))
    out = dict(p_yes=p.mean(axis=2), lppd=np.where(obs, lppd, nan), p_waic=np.where(obs, var(ll, 2), nan),
               f_mean=f.mean(axis=2), f_var=var(f, 2), theta_mean=theta.mean(axis=0), theta_var=var(theta, 0),
               beta_mean=beta.mean(axis=2), beta_var=var(beta, 2))
    lp, pw = out["lppd"][obs], out["p_waic"][obs]
    el = lp - pw
    tot = dict(lppd=lp.sum(), p_waic=pw.sum(), elpd_waic=lp.sum() - pw.sum(), waic=-2.0 * (lp.sum() - pw.sum()),
               n_obs=float(obs.sum()), draws=float(S), elpd_mean=el.mean(),
               elpd_ss=((el - el.mean()) ** 2).sum(), se_elpd_waic=np.sqrt(obs.sum() * el.var(ddof=1)))
    return out, tot


def close(got, want, rtol, what="", scale=None):
    """|got - want| <= rtol * max(|want|, scale) wherever want is not NaN (and NaN exactly where want is).  scale: the
    magnitude the value is a sum of -- a mean near zero of draws of size 1 carries their rounding, not its own; default
    1e-6 of the array's largest value."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    if not ok.any():
        return
    if scale is None:
        scale = 1e-6 * max(1.0, np.abs(want[ok]).max())
    scale = np.broadcast_to(np.asarray(scale, dtype=np.float64), want.shape)[ok]
    err = np.abs(got[ok] - want[ok]) / np.maximum(np.maximum(np.abs(want[ok]), scale), np.finfo(np.float64).tiny)
    assert err.max() <= rtol, f"{what}: relative error {err.max():.3e}"


def check_against(summary, y, theta, beta, f, mu=None):
    want, tot = ref_summary(y, theta, beta, f, mu)
    # the means relative to the size of the draws they average (a mean near zero keeps their rounding)
    mags = dict(f_mean=np.abs(f).max(axis=2), theta_mean=np.abs(theta).max(axis=0), beta_mean=np.abs(beta).max(axis=2))
    for k in CELL:
        if k in summary:
            close(summary[k], want[k], 1e-10, k, mags.get(k))
    for k in TB:
        close(summary[k], want[k], 1e-12, k, mags.get(k))
    if "totals" in summary:
        for k, v in tot.items():
            close(summary["totals"][k], v, 1e-9, "totals." + k)


def _mcmc(rng, n, m, S, B, kw, **extra):
    from gpirt_amd import gpirtMCMC
    from gpirt_amd.ops import RStream
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=100 + n + m)
    args = dict(vote_codes=CODES, theta_init=th0, theta_stabilise=True, **kw, **extra)
    if rng == "reference":
        rs = RStream(4321)
        res = gpirtMCMC(y, S, B, rng="reference", rstream=rs, **args)
        return y, res, rs.state()
    return y, gpirtMCMC(y, S, B, rng="item", seed=29, **args), None


CASES = [("item", 40, 6, 3, 2, {}), ("reference", 130, 5, 4, 1, {}), ("item", 257, 3, 5, 1, {}),
         ("reference", 57, 1, 3, 2, {}), ("item", 200, 20, 3, 1, dict(fstar_fused=True, kstar_rank=64))]


@pytest.mark.parametrize("rng,n,m,S,B,kw", CASES)
def test_summaries_match_numpy_from_stored_draws(rng, n, m, S, B, kw):
    """Missing cells (make_responses leaves 5 % NaN), odd n m (the vector tail: 257 x 3, 57 x 1), m = 1, both RNGs, the
    fused rank-64 draw_fstar."""
    y, res, _ = _mcmc(rng, n, m, S, B, kw, summaries=ALL)
    sm = res["summary"]
    assert np.isnan(y).any()
    assert sm["totals"]["draws"] == S
    check_against(sm, y, res["theta"][1:], res["beta"][:, :, 1:], res["f"][:, :, 1:])


@pytest.mark.parametrize("rng", ["item", "reference"])
def test_summaries_leave_the_chain_alone(rng):
    """Draws and IRFs bit-identical to gpirt_mcmc's, R's generator at the same end state; a call that stores no draw at all
    gives the same summaries as one that stores them."""
    n, m, S, B = 96, 7, 3, 2
    _, plain, st0 = _mcmc(rng, n, m, S, B, {})
    _, withs, st1 = _mcmc(rng, n, m, S, B, {}, summaries=ALL)
    for k in ("theta", "beta", "f", "IRFs"):
        assert np.array_equal(plain[k], withs[k]), k
    if rng == "reference":
        assert np.array_equal(np.asarray(st0[0]), np.asarray(st1[0])) and st0[1] == st1[1]
    _, bare, st2 = _mcmc(rng, n, m, S, B, {}, summaries=ALL, store_draws=False)
    assert bare["theta"] is None and bare["beta"] is None and bare["f"] is None
    assert np.array_equal(bare["IRFs"], plain["IRFs"])
    if rng == "reference":
        assert np.array_equal(np.asarray(st0[0]), np.asarray(st2[0])) and st0[1] == st2[1]
    for k, v in withs["summary"].items():
        if k == "totals":
            assert v == bare["summary"]["totals"]
        else:
            assert np.array_equal(v, bare["summary"][k], equal_nan=True), k
    _, only_f, _ = _mcmc(rng, n, m, S, B, {}, store_draws=("f",))
    assert only_f["theta"] is None and np.array_equal(only_f["f"], plain["f"]) and "summary" not in only_f


@pytest.mark.parametrize("S,B,nth", [(3, 2, 3), (2, 3, 5)])
def test_summaries_survive_a_rollback(S, B, nth):
    """Mirror of test_gpu_guard.py::test_gpirt_mcmc_rolls_back_and_continues with summaries on: the iterations repeated after
    the rollback are added once (draws == S, p_waic would show a double count) and every summary is the undisturbed one --
    to 1e-10 of the array's magnitude, as that test holds the draws (the repeated iterations factor on the fallback panel:
    L, and so f, equal to rounding)."""
    from gpirt_amd import _lib
    lib = _lib.load()
    _, ref, _ = _mcmc("item", 2600, 12, S, B, {}, summaries=ALL)
    assert lib.gpirt_debug_last_mcmc_fallbacks() == 0
    _lib.check(lib.gpirt_debug_trip_guard(None, nth))
    _, got, _ = _mcmc("item", 2600, 12, S, B, {}, summaries=ALL)
    assert lib.gpirt_debug_last_mcmc_fallbacks() == 1
    assert got["summary"]["totals"]["draws"] == S
    for k, v in ref["summary"].items():
        if k == "totals":
            for t, x in v.items():
                close(got["summary"]["totals"][t], x, 1e-10, t)
        else:
            close(got["summary"][k], v, 1e-10, k, max(1.0, np.nanmax(np.abs(v))))


def test_metric_size_stage_api(handle):
    """8192 x 1024, the fast preset, B = 1, S = 3 on the stage API; the reference reads f, mu, theta and beta of each draw."""
    from gpirt_amd import Sampler
    from gpirt_amd.synthetic import CONFIGS, make_responses
    n, m = CONFIGS["M"]
    y, th0 = make_responses(n, m, seed=20240)
    s = Sampler(handle, y, th0, preset="fast", seed=5)
    s.init()
    s.step()
    s.check()
    s.summary_enable(("waic", "pred", "f"))
    th, be, ff, mu = [], [], [], []
    for _ in range(3):
        s.step()
        s.summary_accumulate()
        s.check()
        ff.append(s.get("f")); mu.append(s.get("mu")); th.append(s.get("theta")); be.append(s.get("beta"))
    sm = s.summary()
    s.close()
    check_against(sm, y, np.stack(th), np.stack(be, axis=2), np.stack(ff, axis=2), np.stack(mu, axis=2))


def test_edges(handle):
    """S = 1: every variance and p_waic NaN, lppd and p_yes finite; a fully missing column: NaN lppd / p_waic there, not
    counted in n_obs; parts = 0 frees the summaries and leaves the chain as if they had never been on."""
    from gpirt_amd import Sampler, _lib
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(90, 5, seed=13)
    y[:, 2] = np.nan
    s = Sampler(handle, y, th0, rng="item", seed=41, theta_stabilise=True)
    s.init()
    s.summary_enable(("waic", "pred", "f"))
    s.step()
    s.summary_accumulate()
    one = s.summary()
    obs = ~np.isnan(y)
    assert np.isfinite(one["lppd"][obs]).all() and np.isfinite(one["p_yes"]).all() and np.isfinite(one["f_mean"]).all()
    for k in ("p_waic", "f_var", "theta_var", "beta_var"):
        assert np.isnan(one[k]).all(), k
    assert one["totals"]["draws"] == 1 and np.isnan(one["totals"]["p_waic"]) and np.isnan(one["totals"]["se_elpd_waic"])
    assert np.isfinite(one["totals"]["lppd"])
    th, be, ff = [s.get("theta")], [s.get("beta")], [s.get("f")]
    for _ in range(2):
        s.step()
        s.summary_accumulate()
        th.append(s.get("theta")); be.append(s.get("beta")); ff.append(s.get("f"))
    sm = s.summary()
    assert np.isnan(sm["lppd"][:, 2]).all() and np.isnan(sm["p_waic"][:, 2]).all()
    assert np.isfinite(sm["p_yes"][:, 2]).all()
    assert sm["totals"]["n_obs"] == obs.sum() and sm["totals"]["n_obs"] < y.size
    check_against(sm, y, np.stack(th), np.stack(be, axis=2), np.stack(ff, axis=2))
    # parts = 0
    s.summary_enable(0)
    with pytest.raises(_lib.GpirtError):
        s.summary_accumulate()
    s.step()
    t = Sampler(handle, y, th0, rng="item", seed=41, theta_stabilise=True)
    t.init()
    for _ in range(4):
        t.step()
    for k in ("theta", "f", "beta", "mu"):
        assert np.array_equal(s.get(k), t.get(k)), k
    s.close()
    t.close()


def test_held_out_votes_beat_the_item_marginal():
    """10 % of the observed votes masked to NaN: their log score under p_yes beats each item's marginal yes-frequency."""
    from gpirt_amd import gpirtMCMC
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(300, 40, seed=2024)
    rng = np.random.default_rng(7)
    obs = np.argwhere(~np.isnan(y))
    held = obs[rng.choice(len(obs), size=len(obs) // 10, replace=False)]
    train = y.copy()
    train[held[:, 0], held[:, 1]] = np.nan
    res = gpirtMCMC(train, 100, 100, vote_codes=CODES, theta_init=th0, preset="fast", seed=3, summaries=("pred", "waic"),
                    store_draws=False)
    p = res["summary"]["p_yes"]
    truth = y[held[:, 0], held[:, 1]]
    ph = p[held[:, 0], held[:, 1]]
    score = np.mean(np.log(np.where(truth > 0, ph, 1.0 - ph)))
    freq = np.array([np.mean(train[:, j][~np.isnan(train[:, j])] > 0) for j in range(y.shape[1])])
    pb = freq[held[:, 1]]
    base = np.mean(np.log(np.where(truth > 0, pb, 1.0 - pb)))
    print(f"held-out log score: model {score:.4f}, item marginal {base:.4f}")
    assert np.isfinite(score) and score > base
    assert np.isnan(res["summary"]["lppd"][held[:, 0], held[:, 1]]).all()


def _run_sharded(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gpirt_amd.distributed import ShardedSampler
    from gpirt_amd.ops import Handle
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(300, 22, seed=6)
    h = Handle(0)

    def factory(yl, th, pm, ps, st, item0, m_total):
        return Sampler(h, yl, th, pm, ps, st, rng="item", seed=77, item0=item0, m_total=m_total)

    ss = ShardedSampler(factory, y, th0, dist=dist, chol="replicated")
    ss.init()
    ss.step()
    ss.summary_enable(("waic", "pred"))
    for _ in range(3):
        ss.step()
        ss.summary_accumulate()
    ss.engine.check()
    tot = ss.summary_totals()
    p_yes, lppd = ss.summary_gather("p_yes"), ss.summary_gather("lppd")
    if rank == 0:
        np.savez(os.path.join(outdir, "sharded_summary.npz"), p_yes=p_yes, lppd=lppd,
                 **{"t_" + k: v for k, v in tot.items()})
    dist.destroy_process_group()


def test_two_ranks_on_one_card_match_single_process(handle, tmp_path):
    import torch.multiprocessing as mp
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    port = 29650 + (os.getpid() % 1000)
    mp.spawn(_run_sharded, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    got = np.load(tmp_path / "sharded_summary.npz")
    y, th0 = make_responses(300, 22, seed=6)
    s = Sampler(handle, y, th0, rng="item", seed=77)
    s.init()
    s.step()
    s.summary_enable(("waic", "pred"))
    for _ in range(3):
        s.step()
        s.summary_accumulate()
    s.check()
    ref = s.summary()
    s.close()
    for k, v in ref["totals"].items():
        close(got["t_" + k], v, 1e-12, k)
    assert float(got["t_n_obs"]) == ref["totals"]["n_obs"] and float(got["t_draws"]) == 3
    close(got["p_yes"], ref["p_yes"], 1e-10, "p_yes")
    close(got["lppd"], ref["lppd"], 1e-10, "lppd")
