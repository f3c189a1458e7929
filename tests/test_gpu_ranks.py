"""Rank posteriors on the device (csrc/ranks.hip) against the NumPy statement of the header (gpirt_amd.ranks.from_draws):
the stage API at four sizes with the pairwise counters on, constructed states and skipped draws, the untouched chain, the
pooling of reflected chains, senate116, repeatability and the refusals."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
CODES = dict(yea=[1], nay=[-1], missing=[None])
INT_FIELDS = ("rank2_sum", "rank2_sumsq", "rank_hist", "pivot_cover", "lt", "draws", "skipped_draws", "pivots")
HOST_DOUBLES = ("rank_mean", "rank_var", "rank_quantiles", "p_less", "rank_bin_width")


def grid(k):
    return -5.0 + np.asarray(k).astype(np.float64) * 0.01


def constructed_draws(n, seed=0):
    """tests/test_ranks_cpu.py's constructed draws: heavy ties, all equal, two strict orders, an off-grid value, some
    ties, a NaN."""
    rng = np.random.default_rng(seed)
    k = [rng.integers(498, 503, n), np.full(n, 700), rng.permutation(n) + 100, (rng.permutation(n) + 100)[::-1],
         rng.integers(0, 1001, n), rng.integers(400, 400 + max(2, n // 2), n), rng.integers(0, 1001, n)]
    th = grid(np.stack(k))
    th[4, n // 3] = 0.123456
    th[6, 0] = np.nan
    return th


def check_equal(got, want, S, what=""):
    """Every integer field and every double that is a fixed host function of them bit for bit; pivot_share (and p_pivot,
    one more division) within 4 S eps relative: one division and one addition per draw, each at most 2 ulp if the
    device's division is not correctly rounded."""
    for f in INT_FIELDS + HOST_DOUBLES:
        a, b = got[f], want[f]
        if b is None:
            assert a is None, (what, f)
            continue
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), (what, f)
    assert np.array_equal(got["order"], want["order"]), what
    for f, extra in (("pivot_share", 0), ("p_pivot", 1)):
        a, b = got[f], want[f]
        assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), (what, f)
        ok = ~np.isnan(b)
        assert (np.abs(a[ok] - b[ok]) <= (4 * S + extra) * EPS * np.abs(b[ok])).all(), (what, f)
    same = np.array_equal(got["pivot_share"], want["pivot_share"], equal_nan=True)
    print(f"MEASURED {what} pivot_share bit-equal to NumPy: {same}")


@pytest.mark.parametrize("n,m,steps", [(100, 17, 5), (257, 33, 5), (1000, 64, 4), (8192, 1024, 3)])
def test_stage_api_against_from_draws(handle, n, m, steps):
    """A few steps with rank_accumulate after each, the pairwise counters on (268 MB at 8192); get("theta") per draw is
    the NumPy input."""
    from gpirt_amd import Sampler, ranks
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=100 + n, na_frac=0.03)
    pivots = ("median", 1, n // 3)
    s = Sampler(handle, y, th0, preset="fast", seed=2**35 + 17)
    s.init()
    s.rank_enable(pivots=pivots, pairwise=True)
    th = []
    for _ in range(steps):
        s.step()
        s.rank_accumulate()
        th.append(s.get("theta"))
    s.check()
    got = s.ranks()
    raw = {k: s.rank_get(k) for k in ("rank2_sum", "rank2_sumsq", "rank_hist", "pivot_cover", "pivot_share", "pivots",
                                      "rank_mean", "rank_var", "p_pivot", "counts")}
    lt = s.rank_get("lt") if n <= 1000 else None
    hdr = ranks.state_header(s.rank_state())
    s.close()
    want = ranks.from_draws(np.stack(th), pivots, pairwise=True)
    assert want["draws"] == steps and want["skipped_draws"] == 0
    check_equal(got, want, steps, f"stage@{n}x{m}")
    B, w, _ = ranks.bin_scheme(n)
    assert hdr == dict(n=n, draws=steps, skipped=0, version=1, B=B, w=w, pivots=want["pivots"].tolist(), pairwise=True)
    assert raw["counts"].tolist() == [steps, 0, B, w, len(want["pivots"])]
    for k in ("rank2_sum", "rank2_sumsq", "rank_hist", "pivot_cover", "pivot_share", "pivots", "rank_mean", "rank_var", "p_pivot"):
        assert np.array_equal(raw[k], got[k], equal_nan=True), k
    if lt is not None:
        assert np.array_equal(lt, want["lt"])
    assert not np.diag(got["lt"]).any()
    assert (got["lt"].astype(np.int64) + got["lt"].T <= steps).all() if n <= 1000 else True


@pytest.mark.parametrize("n", [12, 33, 300])
def test_constructed_states(handle, n):
    """theta set to the CPU test's constructed draws, rank_accumulate called directly: equal to from_draws; the off-grid
    value and the NaN each skip their draw and leave every accumulator bit-identical to before."""
    from gpirt_amd import Sampler, ranks
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, 6, seed=5)
    th = constructed_draws(n, seed=n)
    pivots = ("median", 1, min(3, n))
    s = Sampler(handle, y, th0, rng="item", seed=5, theta_stabilise=True)
    s.init()
    s.rank_enable(pivots=pivots, pairwise=True)
    blocks = []
    for t in th:
        s.set("theta", t)
        s.rank_accumulate()
        blocks.append(s.rank_state().cpu().numpy().copy())
    got = s.ranks(probs=(0.0, 0.025, 0.5, 0.975, 1.0))
    s.close()
    want = ranks.from_draws(th, pivots, (0.0, 0.025, 0.5, 0.975, 1.0), pairwise=True)
    assert want["draws"] == 5 and want["skipped_draws"] == 2
    check_equal(got, want, 5, f"constructed@{n}")
    for d in (4, 6):                          # the skipped draws: only the header's skipped counter moved
        before, after = blocks[d - 1].copy(), blocks[d].copy()
        assert after[2] == before[2] + 1 and after[1] == before[1]
        after[2] = before[2]
        assert np.array_equal(before, after), d
    assert not np.array_equal(blocks[4], blocks[5])


def test_sixteen_asymmetric_pivots(handle):
    """The most positions a caller may give, none the mirror image of another: the closed set has 32.  rank_enable,
    ranks(), rank_get and combine (two states, one reflected) against from_draws; gpirtMCMC takes them too."""
    from gpirt_amd import Sampler, gpirtMCMC, ranks
    from gpirt_amd.synthetic import make_responses
    n, m, steps = 100, 17, 4
    pivots = list(range(1, 17))
    y, th0 = make_responses(n, m, seed=77, na_frac=0.03)
    ss, th = [], []
    for c in range(2):
        s = Sampler(handle, y, th0, preset="fast", seed=300 + c)
        s.init()
        s.rank_enable(pivots=pivots, pairwise=True)
        t = []
        for _ in range(steps):
            s.step()
            s.rank_accumulate()
            t.append(s.get("theta"))
        s.check()
        ss.append(s)
        th.append(np.stack(t))
    want_closed = sorted(set(pivots) | {n + 1 - q for q in pivots})
    assert len(want_closed) == 32
    own = ss[0].ranks()
    assert own["pivots"].tolist() == want_closed and ss[0].rank_get("pivots").tolist() == want_closed
    assert ss[0].rank_get("p_pivot").shape == (32, n) and ss[0].rank_get("counts").tolist()[4] == 32
    check_equal(own, ranks.from_draws(th[0], pivots, pairwise=True), steps, "16 pivots, one state")
    both = ranks.combine(handle, ss, signs=[1, -1])
    check_equal(both, ranks.from_draws(np.stack(th), pivots, signs=[1, -1], pairwise=True), 2 * steps, "16 pivots, pooled")
    for s in ss:
        s.close()
    res = gpirtMCMC(y, steps, 1, vote_codes=CODES, theta_init=th0, preset="fast", seed=300, ranks=dict(pivots=pivots))
    assert res["ranks"]["pivots"].tolist() == want_closed
    check_equal(res["ranks"], ranks.from_draws(res["theta"][None, 1:], pivots), steps, "16 pivots, gpirtMCMC")


@pytest.mark.parametrize("case", ["fast", "fast_all", "reference"])
def test_chain_untouched(case):
    """gpirtMCMC(..., ranks=dict(pairwise=True)) against the same call without ranks: theta, beta, f, the IRFs (and the
    summaries, quantiles and PPC when asked together) bit-identical; under rng="reference" R's stream ends at the same
    position."""
    from gpirt_amd import gpirtMCMC, ranks
    from gpirt_amd.ops import RStream
    from gpirt_amd.synthetic import make_responses
    n, m, S, B = 96, 12, 4, 2
    y, th0 = make_responses(n, m, seed=31, snap_theta=False)
    kw = dict(vote_codes=CODES, theta_init=th0)
    rs = [None, None]
    if case == "fast":
        kw.update(preset="fast", seed=9)
    elif case == "fast_all":
        kw.update(preset="fast", seed=9, chains=2, theta_init=None, summaries=("waic",), quantiles=(0.025, 0.5, 0.975), ppc=True)
    else:
        rs = [RStream(77), RStream(77)]
    res = []
    for k, rk in enumerate((None, dict(pairwise=True))):
        extra = dict(rstream=rs[k]) if rs[k] is not None else {}
        res.append(gpirtMCMC(y, S, B, ranks=rk, **kw, **extra))
    plain, with_ranks = res
    assert "ranks" not in plain and "ranks" in with_ranks
    for k in ("theta", "beta", "f", "IRFs"):
        assert np.array_equal(plain[k], with_ranks[k], equal_nan=True), k
    if case == "reference":
        (mt0, i0), (mt1, i1) = rs[0].state(), rs[1].state()
        assert i0 == i1 and np.array_equal(mt0, mt1)
    if case == "fast_all":
        for k, v in plain["summary"].items():
            if k != "totals":
                assert np.array_equal(v, with_ranks["summary"][k], equal_nan=True), k
        for k, v in plain["summary"]["totals"].items():
            assert np.array_equal(v, with_ranks["summary"]["totals"][k], equal_nan=True), k
        for k in ("theta", "irf", "theta_median", "irf_p_mean", "theta_hist"):
            assert np.array_equal(plain["quantiles"][k], with_ranks["quantiles"][k], equal_nan=True), k
        for unit in ("item", "respondent"):
            for k, v in plain["ppc"][unit].items():
                assert np.array_equal(v, with_ranks["ppc"][unit][k], equal_nan=True), (unit, k)
        assert plain["ppc"]["totals"]["rep_yes_sum"] == with_ranks["ppc"]["totals"]["rep_yes_sum"]
    rk = with_ranks["ranks"]
    C_ = 2 if case == "fast_all" else 1
    assert rk["draws"] + rk["skipped_draws"] == C_ * S
    th = with_ranks["theta"][:, 1:] if case == "fast_all" else with_ranks["theta"][None, 1:]
    signs = np.where(with_ranks["diagnostics"]["reflected"], -1, 1)
    check_equal(rk, ranks.from_draws(th, signs=signs, pairwise=True), C_ * S, f"gpirtMCMC {case}")


def test_chains_pool_with_reflection(handle):
    """chains=3, align=True, chain 1 started at -theta0 (as tests/test_gpu_chains.py provokes the mirror mode):
    res["ranks"] equals ranks.combine of the three chains' rank_state() blocks with the signs in
    res["diagnostics"]["reflected"], and from_draws on the stacked stored theta draws with those signs.  Copies of one state
    pooled with signs (+1, -1) give the symmetric result: rank_mean = (n + 1) / 2 for every respondent, exactly."""
    from gpirt_amd import Sampler, _lib, gpirtMCMC, ranks
    from gpirt_amd.synthetic import make_responses
    n, m, S, B, seed = 300, 40, 8, 2, 29
    y, th0 = make_responses(n, m, seed=11)
    inits = np.stack([th0, -th0, np.roll(th0, 11)])
    spec = dict(pivots=("median", 100), pairwise=True)
    res = gpirtMCMC(y, S, B, vote_codes=CODES, theta_init=inits, rng="item", seed=seed, theta_stabilise=True, chains=3,
                    align=True, ranks=spec)
    refl = res["diagnostics"]["reflected"]
    print("reflected:", refl)
    assert refl.any() and not refl[0]
    signs = np.where(refl, -1, 1)
    want = ranks.from_draws(res["theta"][:, 1:], spec["pivots"], signs=signs, pairwise=True)
    check_equal(res["ranks"], want, 3 * S, "chains=3")
    assert res["ranks"]["draws"] == 3 * S
    samplers = []
    for c in range(3):
        s = Sampler(handle, y, inits[c], rng="item", seed=_lib.chain_seed(seed, c), theta_stabilise=True)
        s.init()
        s.rank_enable(**spec)
        for it in range(S + B):
            s.step()
            if it >= B:
                s.rank_accumulate()
        s.check()
        samplers.append(s)
    pooled = ranks.combine(handle, samplers, signs=signs)
    for f in INT_FIELDS + HOST_DOUBLES + ("pivot_share", "p_pivot", "order"):
        assert np.array_equal(np.asarray(pooled[f]), np.asarray(res["ranks"][f]), equal_nan=True), f
    unaligned = ranks.combine(handle, samplers)
    assert np.array_equal(unaligned["rank2_sum"], sum(s.rank_get("rank2_sum") for s in samplers))
    st = samplers[0].rank_state()
    sym = ranks.combine(handle, [st, st.clone()], signs=[1, -1])
    assert np.array_equal(sym["rank_mean"], np.full(n, (n + 1) / 2.0))
    assert np.array_equal(sym["lt"], sym["lt"].T) and np.array_equal(sym["rank_hist"], sym["rank_hist"][:, ::-1])
    assert np.array_equal(sym["pivot_cover"], sym["pivot_cover"][::-1])
    for s in samplers:
        s.close()


def test_senate116():
    """n = 100, pivots "median" plus (41, 60), 200 draws: the histogram is exact (w = 1), sum_i p_pivot = 1 per pivot
    within S n eps, the pivot set is {41, 50, 51, 60}, order is a permutation."""
    from gpirt_amd import gpirtMCMC
    path = os.path.join(os.path.dirname(__file__), "golden", "senate116_y.npz")
    y = np.load(path)["y"].astype(np.float64)
    y[y == 0] = np.nan
    n = y.shape[0]
    assert n == 100
    S = 200
    res = gpirtMCMC(y, S, 50, vote_codes=CODES, preset="fast", seed=116, store_draws=False,
                    ranks=dict(pivots=("median", 41, 60)))
    rk = res["ranks"]
    assert rk["draws"] + rk["skipped_draws"] == S and rk["draws"] > 0
    assert rk["rank_bin_width"] == 0.5 and rk["rank_hist"].shape == (n, 2 * n - 1)
    assert (rk["rank_hist"].sum(axis=1) == rk["draws"]).all()
    r2 = np.arange(2, 2 * n + 1, dtype=np.uint64)
    assert np.array_equal(rk["rank_hist"].astype(np.uint64) @ r2, rk["rank2_sum"])
    assert np.array_equal(rk["rank_hist"].astype(np.uint64) @ (r2 * r2), rk["rank2_sumsq"])
    assert rk["pivots"].tolist() == [41, 50, 51, 60]
    assert np.abs(rk["p_pivot"].sum(axis=1) - 1.0).max() <= rk["draws"] * n * EPS
    assert sorted(rk["order"].tolist()) == list(range(n))
    assert rk["p_less"] is None and rk["lt"] is None
    assert (rk["rank_quantiles"][0] <= rk["rank_quantiles"][1]).all() and (rk["rank_quantiles"][1] <= rk["rank_quantiles"][2]).all()
    print("MEASURED senate116 median pivot: respondent", int(rk["p_pivot"][1].argmax()), "p", float(rk["p_pivot"][1].max()))


def test_repeatability_and_refusals(handle):
    """The same run twice gives a bit-identical state block; more than 16 pivots, a pivot outside 1..n and rank_get before
    rank_enable give the library's error code with a message; rank_enable(on=False) frees the block."""
    import torch

    from gpirt_amd import Sampler, _lib
    from gpirt_amd.synthetic import make_responses
    n, m = 1000, 64
    y, th0 = make_responses(n, m, seed=55)
    blocks = []
    for _ in range(2):
        s = Sampler(handle, y, th0, preset="fast", seed=21)
        s.init()
        s.rank_enable(pivots=("median", 7), pairwise=True)
        for _ in range(4):
            s.step()
            s.rank_accumulate()
        blocks.append(s.rank_state().cpu().numpy().copy())
        s.close()
    assert blocks[0].dtype == np.int64 and np.array_equal(blocks[0], blocks[1]) and blocks[0][40:].any()
    s = Sampler(handle, y, th0, preset="fast", seed=21)
    s.init()
    for call in (lambda: s.rank_get("rank_mean"), lambda: s.rank_accumulate(), lambda: s.rank_state(),
                 lambda: s.rank_enable(pivots=list(range(1, 18))), lambda: s.rank_enable(pivots=[0]),
                 lambda: s.rank_enable(pivots=[n + 1])):
        with pytest.raises(_lib.GpirtError) as e:
            call()
        assert e.value.code == _lib.E_ARG and _lib.last_error()
    with pytest.raises(_lib.GpirtError):
        s.rank_get("rank_mean")                # the refused enables left nothing behind
    free0 = torch.cuda.mem_get_info(handle.device)[0]
    s.rank_enable(pairwise=True)
    free1 = torch.cuda.mem_get_info(handle.device)[0]
    assert free0 - free1 >= 4 * n * n
    with pytest.raises(_lib.GpirtError):
        s.rank_get("no_such_field")
    s.rank_enable(on=False)
    free2 = torch.cuda.mem_get_info(handle.device)[0]
    assert free2 - free1 >= 4 * n * n
    with pytest.raises(_lib.GpirtError):
        s.rank_accumulate()
    s.rank_enable()                            # and again: a fresh, zeroed block
    assert s.rank_get("counts").tolist()[:2] == [0, 0] and not s.rank_get("rank2_sum").any()
    s.close()


def test_sharded_sampler_ranks(handle):
    """theta is replicated on every rank, so the shards' engine ranks it as one GPU does."""
    from gpirt_amd import Sampler, ranks
    from gpirt_amd.distributed import ShardedSampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(64, 8, seed=4)

    def factory(yl, th, pm, ps, st, item0, m_total):
        return Sampler(handle, yl, th, pm, ps, st, rng="item", seed=77, item0=item0, m_total=m_total)

    ss = ShardedSampler(factory, y, th0, dist=None)
    ss.init()
    ss.rank_enable(pairwise=True)
    th = []
    for _ in range(3):
        ss.step()
        ss.rank_accumulate()
        th.append(ss.engine.get("theta"))
    got = ss.ranks()
    ss.engine.close()
    check_equal(got, ranks.from_draws(np.stack(th), pairwise=True), 3, "sharded")
