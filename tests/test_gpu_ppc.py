"""Posterior predictive checks on the device (csrc/ppc.hip) against the NumPy statement of the header
(gpirt_amd.ppc.from_draws), the exported uniforms, the untouched chain, the pooling of chains, constructed states,
repeatability and the refusal for item shards."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
INT_FIELDS = ("n_obs", "obs_yes", "yes_ge", "yes_gt", "dev_ge", "nonfinite", "rep_yes_sum", "rep_yes_sumsq", "correct_sum")
CODES = dict(yea=[1], nay=[-1], missing=[None])


def _responses(n, m, seed):
    """about 3 % NaN, plus one column and one row without an observed cell"""
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=seed, na_frac=0.03)
    y = np.array(y, order="F")
    y[:, m // 3] = np.nan
    y[n // 2, :] = np.nan
    return y, th0


def _rel(got, want, rtol, what):
    """|got - want| <= rtol |want| wherever want is finite, NaN exactly where want has it; returns the worst ratio"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    err = np.abs(got[ok] - want[ok])
    worst = float((err / np.maximum(np.abs(want[ok]), 1e-300)).max())
    assert (err <= rtol * np.abs(want[ok])).all(), f"{what}: worst {worst:.3e} > {rtol:.3e}"
    return worst


def _exact_var(S, s1, s2):
    return np.array([float(int(a) * int(c) - int(b) ** 2) / (float(a) * float(a - 1)) if a >= 2 else np.nan
                     for a, b, c in zip(S, s1, s2)])


@pytest.mark.parametrize("n,m,steps", [(100, 17, 5), (257, 33, 5), (1000, 64, 4), (8192, 1024, 3)])
def test_stage_api_against_from_draws(handle, n, m, steps):
    """A few steps with ppc_accumulate after each; g per draw = get("f") + get("mu").  Every integer output lies inside
    from_draws' [lo, hi]; the undecided cells and comparisons are reported and capped (the cap keeps the test from hiding
    a failure behind wide bounds; with continuous g the expected number is 1e-13 x cells: none); the doubles are held to
    tolerances derived from the sum lengths."""
    from gpirt_amd import Sampler
    from gpirt_amd import ppc as P
    y, th0 = _responses(n, m, seed=100 + n)
    seed = 2**35 + 17
    s = Sampler(handle, y, th0, preset="fast", seed=seed)
    s.init()
    s.ppc_enable()
    g, iters = [], []
    for _ in range(steps):
        s.step()
        s.ppc_accumulate()
        iters.append(s.iteration)
        g.append(s.get("f") + s.get("mu"))
    s.check()
    got = s.ppc()
    s.close()
    assert iters == list(range(1, steps + 1))
    want = P.from_draws(y, np.stack(g), seed, iters)
    und = want["undecided"]["cells"] + want["undecided"]["comparisons"]
    print(f"MEASURED undecided@{n}x{m} cells {want['undecided']['cells']} comparisons {want['undecided']['comparisons']} "
          f"of {want['comparisons']}")
    assert und <= 1e-3 * want["comparisons"]
    for unit, L in (("item", n), ("respondent", m), ("totals", n * m)):
        w = want[unit]
        d = {k: np.atleast_1d(v) for k, v in got[unit].items()}
        for k in INT_FIELDS:
            lo, hi = w[k]
            assert ((d[k] >= lo) & (d[k] <= hi)).all(), (unit, k, d[k], lo, hi)
        assert np.array_equal(d["draws"], np.full(len(d["draws"]), float(steps)))
        # the means of the integer sums are exact functions of the device's own sums (S = draws - nonfinite)
        Sk = (steps - d["nonfinite"]).astype(np.int64)
        with np.errstate(invalid="ignore", divide="ignore"):
            den = np.where((d["n_obs"] > 0) & (Sk >= 1), Sk, np.nan).astype(np.float64)
            assert np.array_equal(d["rep_yes_mean"], d["rep_yes_sum"] / den, equal_nan=True)
            assert np.array_equal(d["correct_mean"], d["correct_sum"] / den, equal_nan=True)
            var = np.where(d["n_obs"] > 0, _exact_var(Sk, d["rep_yes_sum"].astype(np.int64),
                                                      d["rep_yes_sumsq"].astype(np.int64)), np.nan)
            assert np.array_equal(d["rep_yes_var"], var, equal_nan=True)
        # D(y), D(yrep): a sum of L positive terms per draw, each term within a few ulp of NumPy's (exp, log1p: 2 ulp each,
        # two roundings more), summed in another order (<= L eps relative), then S draws: 4 L S eps bounds it
        rtol = 4.0 * L * steps * EPS
        # (D(yrep) is compared where the replicate is: with an undecided cell NumPy's yrep may differ from the device's)
        for k in ("dev_obs_mean", "dev_rep_mean")[:2 if want["undecided"]["cells"] == 0 else 1]:
            print(f"MEASURED {unit}_{k}_rtol@{n}x{m} {_rel(d[k], w[k], rtol, unit + ' ' + k):.3e} (bound {rtol:.3e})")
    # the derived p-values
    S = float(steps)
    some = got["item"]["n_obs"] > 0
    assert np.array_equal(got["item"]["ppp_yes"][some], got["item"]["yes_ge"][some] / S)
    assert np.array_equal(got["item"]["ppp_yes_mid"][some], (got["item"]["yes_ge"] + got["item"]["yes_gt"])[some] / (2 * S))
    assert np.isnan(got["item"]["ppp_yes"][~some]).all() and (~some).sum() == 1
    assert np.isnan(got["respondent"]["rep_yes_mean"]).sum() == 1


def test_uniforms_reproduce_the_replicate(handle):
    """100 x 17, one draw: yrep recomputed from Handle.item_uniforms(seed, it, 8, item0, m, n) and the device's own p
    (GPIRT_SUM_PRED of the same draw) gives exactly the counts the device reports (rep_yes_sum is R itself)."""
    from gpirt_amd import Sampler, _lib
    n, m = 100, 17
    y, th0 = _responses(n, m, seed=7)
    seed = 2**40 + 3
    s = Sampler(handle, y, th0, rng="item", seed=seed, theta_stabilise=True)
    s.init()
    s.summary_enable(("pred",))
    s.ppc_enable()
    s.step()
    s.step()
    s.summary_accumulate()
    s.ppc_accumulate()
    it = s.iteration
    p = s.summary_get("p_yes")
    got = s.ppc()
    s.close()
    assert it == 2
    u = handle.item_uniforms(seed, it, _lib.ST_PPC, 0, m, n).cpu().numpy()
    assert u.shape == (n, m)
    rep = ~np.isnan(y) & (u < p)
    assert np.array_equal(got["item"]["rep_yes_sum"], rep.sum(axis=0).astype(float))
    assert np.array_equal(got["respondent"]["rep_yes_sum"], rep.sum(axis=1).astype(float))
    assert got["totals"]["rep_yes_sum"] == float(rep.sum())
    T = (y > 0).sum(axis=0)
    assert np.array_equal(got["item"]["yes_ge"], (rep.sum(axis=0) >= T).astype(float) * (got["item"]["n_obs"] > 0))


@pytest.mark.parametrize("case", ["fast", "reference", "chains3_quantiles"])
def test_chain_untouched(case):
    """gpirtMCMC(..., ppc=True) against the same call without ppc: theta, beta, f and the IRFs bit-identical; under
    rng="reference" R's stream ends at the same position."""
    from gpirt_amd import gpirtMCMC
    from gpirt_amd.ops import RStream
    from gpirt_amd.synthetic import make_responses
    n, m, S, B = 96, 12, 4, 2
    y, th0 = make_responses(n, m, seed=31, snap_theta=False)
    kw = dict(vote_codes=CODES, theta_init=th0)
    rs = [None, None]
    if case == "fast":
        kw.update(preset="fast", seed=9)
    elif case == "reference":
        rs = [RStream(77), RStream(77)]
    else:
        kw.update(preset="fast", seed=9, chains=3, quantiles=(0.025, 0.5, 0.975), theta_init=None)
    res = []
    for k, ppc in enumerate((None, True)):
        extra = dict(rstream=rs[k]) if rs[k] is not None else {}
        res.append(gpirtMCMC(y, S, B, ppc=ppc, **kw, **extra))
    plain, with_ppc = res
    assert "ppc" not in plain and "ppc" in with_ppc
    for k in ("theta", "beta", "f", "IRFs"):
        assert np.array_equal(plain[k], with_ppc[k], equal_nan=True), k
    if case == "reference":
        (mt0, i0), (mt1, i1) = rs[0].state(), rs[1].state()
        assert i0 == i1 and np.array_equal(mt0, mt1)
    if case == "chains3_quantiles":
        for k in ("theta", "irf", "theta_median", "irf_p_mean"):
            assert np.array_equal(plain["quantiles"][k], with_ppc["quantiles"][k], equal_nan=True), k
        assert with_ppc["ppc"]["totals"]["draws"] == 3 * S
    else:
        assert with_ppc["ppc"]["totals"]["draws"] == S
    pp = with_ppc["ppc"]
    assert pp["item"]["yes_ge"].shape == (m,) and pp["respondent"]["yes_ge"].shape == (n,)
    assert (pp["item"]["ppp_yes"] >= 0).all() and (pp["item"]["ppp_yes"] <= 1).all()
    assert pp["totals"]["n_obs"] == float((~np.isnan(y)).sum()) and pp["totals"]["nonfinite"] == 0


@pytest.mark.parametrize("align", [True, False])
def test_pooled_counts_are_the_sum_of_the_chains(align):
    """chains=3 against the three chains run singly with gpirt_chain_seed and the same inits."""
    from gpirt_amd import _lib, gpirtMCMC
    from gpirt_amd.chains import default_inits
    from gpirt_amd.synthetic import make_responses
    n, m, S, B, seed = 80, 10, 5, 2, 13
    y, _ = make_responses(n, m, seed=32, snap_theta=False)
    th0 = default_inits(n, 3, seed)
    pooled = gpirtMCMC(y, S, B, vote_codes=CODES, theta_init=th0, preset="fast", seed=seed, chains=3, align=align, ppc=True)["ppc"]
    singles = [gpirtMCMC(y, S, B, vote_codes=CODES, theta_init=th0[c], preset="fast", seed=_lib.chain_seed(seed, c),
                         ppc=True)["ppc"] for c in range(3)]
    for unit in ("item", "respondent", "totals"):
        for k in ("yes_ge", "yes_gt", "dev_ge", "nonfinite", "draws", "rep_yes_sum", "rep_yes_sumsq", "correct_sum"):
            want = sum(np.asarray(sg[unit][k]) for sg in singles)
            assert np.array_equal(np.asarray(pooled[unit][k]), want), (unit, k)
        for k in ("n_obs", "obs_yes"):
            assert np.array_equal(np.asarray(pooled[unit][k]), np.asarray(singles[0][unit][k])), (unit, k)
        # the means of the integer sums: exact functions of the pooled sums
        some = np.asarray(pooled[unit]["n_obs"]) > 0
        for k, src in (("rep_yes_mean", "rep_yes_sum"), ("correct_mean", "correct_sum")):
            got = np.atleast_1d(pooled[unit][k])
            assert np.array_equal(got[some], (np.atleast_1d(pooled[unit][src]) / (3.0 * S))[some]), (unit, k)
            assert np.isnan(got[~some]).all()
        for k in ("dev_obs_mean", "dev_rep_mean"):
            # pooled = (s0 + s1 + s2) / 3S against (s0 / S + s1 / S + s2 / S) / 3: three divisions, two additions and a
            # division here, two additions and a division there: nine roundings of positive terms, each at most eps / 2
            # relative, 4.5 eps in all; 8 eps bounds it
            want = sum(np.asarray(sg[unit][k]) for sg in singles) / 3.0
            _rel(np.atleast_1d(pooled[unit][k]), np.atleast_1d(want), 8 * EPS, unit + " " + k)
    assert pooled["totals"]["draws"] == 3 * S


def _constructed(handle, y, S=4):
    from gpirt_amd import Sampler
    s = Sampler(handle, y, np.zeros(y.shape[0]), rng="item", seed=5, theta_stabilise=True)
    s.init()
    s.ppc_enable()
    mu = s.get("mu")
    f = np.where(np.isnan(y), 1.5, 40.0 * y) - mu
    return s, f


def test_constructed_state_is_deterministic_and_nonfinite_counts_out(handle):
    """f = 40 y - mu: p rounds to exactly 1 or lies below every u, so yrep = y in every draw: the outcomes of the CPU test,
    on the device.  Then a NaN in one observed f cell: `nonfinite` rises for exactly that row, that column and the total,
    whose other accumulators stay where they were; every other unit takes the draw."""
    n, m, S = 300, 37, 4                       # two row blocks (the second ragged), two strips (the second ragged)
    rng = np.random.default_rng(8)
    y = np.where(rng.random((n, m)) < 0.5, 1.0, -1.0)
    y[rng.random((n, m)) < 0.03] = np.nan
    y[:, 5] = np.nan
    y[17, :] = np.nan
    y[260, 33] = 1.0
    s, f = _constructed(handle, y)
    for d in range(S):
        s.set_iteration(10 + d)
        s.set("f", f)
        s.ppc_accumulate()
    got = s.ppc()
    obs = ~np.isnan(y)
    for unit, axis in (("item", 0), ("respondent", 1), ("totals", None)):
        d = {k: np.atleast_1d(v) for k, v in got[unit].items()}
        n_obs = np.atleast_1d(obs.sum(axis=axis)).astype(float)
        T = np.atleast_1d((y > 0).sum(axis=axis)).astype(float)
        some = n_obs > 0
        assert np.array_equal(d["n_obs"], n_obs) and np.array_equal(d["obs_yes"], T)
        assert np.array_equal(d["rep_yes_mean"][some], T[some]) and not d["rep_yes_var"][some].any()
        assert np.array_equal(d["yes_ge"], S * some) and not d["yes_gt"].any()
        assert np.array_equal(d["dev_ge"], S * some) and not d["nonfinite"].any()
        assert np.array_equal(d["correct_mean"][some], n_obs[some])
        assert np.array_equal(d["dev_obs_mean"][some], d["dev_rep_mean"][some])
        for k in ("rep_yes_mean", "rep_yes_var", "dev_obs_mean", "dev_rep_mean", "correct_mean"):
            assert np.isnan(d[k][~some]).all(), (unit, k)
        # D(y) = 2 n_obs log1p(exp(-g)), g = (40 y - mu) + mu within 1.5 ulp(64) = 2^-46 = 64 eps of +-40 (|mu| < 24), so each
        # term within 64 eps relative (+ 4 for exp and log1p), and a sum of n_obs such terms: (n_obs + 68) eps
        _rel(d["dev_obs_mean"][some], 2.0 * n_obs[some] * np.log1p(np.exp(-40.0)), (n_obs.max() + 68) * EPS, unit + " D(y)")
    # one more draw with a NaN in the observed cell (260, 33)
    before = got
    fbad = f.copy()
    fbad[260, 33] = np.nan
    s.set_iteration(20)
    s.set("f", fbad)
    s.ppc_accumulate()
    after = s.ppc()
    s.close()
    nf_i, nf_r = np.zeros(m), np.zeros(n)
    nf_i[33], nf_r[260] = 1, 1
    assert np.array_equal(after["item"]["nonfinite"], nf_i) and np.array_equal(after["respondent"]["nonfinite"], nf_r)
    assert after["totals"]["nonfinite"] == 1 and after["totals"]["draws"] == S + 1
    for k in ("yes_ge", "dev_ge", "rep_yes_sum", "rep_yes_sumsq", "correct_sum"):
        assert after["totals"][k] == before["totals"][k], k
        took = (before["item"]["n_obs"] > 0) & (nf_i == 0)
        scale = (S + 1) / S                    # every draw of a constructed state adds the same to each sum
        assert np.array_equal(after["item"][k][took], before["item"][k][took] * scale), k
        assert after["item"][k][33] == before["item"][k][33] and after["respondent"][k][260] == before["respondent"][k][260], k
    for k in ("rep_yes_mean", "dev_obs_mean", "dev_rep_mean", "correct_mean"):
        assert after["totals"][k] == before["totals"][k], k
        assert after["item"][k][33] == before["item"][k][33] and after["respondent"][k][260] == before["respondent"][k][260], k


def test_same_run_twice_gives_a_bit_identical_state(handle):
    from gpirt_amd import Sampler
    from gpirt_amd import ppc as P
    n, m = 1000, 64
    y, th0 = _responses(n, m, seed=55)
    blocks = []
    for _ in range(2):
        s = Sampler(handle, y, th0, preset="fast", seed=21)
        s.init()
        s.ppc_enable()
        for _ in range(4):
            s.step()
            s.ppc_accumulate()
        st = s.ppc_state()
        hdr = P.state_header(st)
        assert hdr == dict(n=n, m=m, draws=4, version=1, item0=0)
        blocks.append(st.cpu().numpy().copy())
        s.close()
    assert blocks[0].dtype == np.int64 and blocks[0].size == 8 + 11 * ((n + m + 2) & ~1)
    assert np.array_equal(blocks[0], blocks[1])
    assert blocks[0][8:].any()


def test_combine_pools_sampler_states(handle):
    """ppc.combine over two samplers' states: the counts add; one state alone comes back as Sampler.ppc() gives it."""
    from gpirt_amd import Sampler
    from gpirt_amd import ppc as P
    n, m = 257, 33
    y, th0 = _responses(n, m, seed=56)
    ss = []
    for c in range(2):
        s = Sampler(handle, y, th0, preset="fast", seed=21 + c)
        s.init()
        s.ppc_enable()
        for _ in range(3):
            s.step()
            s.ppc_accumulate()
        ss.append(s)
    own = [s.ppc() for s in ss]
    one = P.combine(handle, ss[:1])
    both = P.combine(handle, ss)
    for s in ss:
        s.close()
    for unit in ("item", "respondent"):
        for k in P.PPC_FIELDS:
            assert np.array_equal(one[unit][k], own[0][unit][k], equal_nan=True), (unit, k)
        for k in ("yes_ge", "yes_gt", "dev_ge", "nonfinite"):
            assert np.array_equal(both[unit][k], own[0][unit][k] + own[1][unit][k]), (unit, k)
    assert both["totals"]["draws"] == 6 and both["totals"]["rep_yes_sum"] == own[0]["totals"]["rep_yes_sum"] + own[1]["totals"]["rep_yes_sum"]


def test_sharded_sampler_refuses_ppc(handle):
    from gpirt_amd import Sampler
    from gpirt_amd.distributed import ShardedSampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(64, 8, seed=4)

    def factory(yl, th, pm, ps, st, item0, m_total):
        return Sampler(handle, yl, th, pm, ps, st, rng="item", seed=77, item0=item0, m_total=m_total)

    ss = ShardedSampler(factory, y, th0, dist=None)
    with pytest.raises(ValueError, match="posterior predictive"):
        ss.ppc_enable()
    ss.engine.close()
