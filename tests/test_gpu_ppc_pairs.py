"""The pairwise item checks of the PPC on the device (csrc/ppc_pairs.hip) against NumPy: the int8 products exactly, the
replicate they are formed from against the PPC's own, every accumulator and finished array against
gpirt_amd.ppc.pairs_from_rep bit for bit, constructed states, the untouched chain and PPC block, pooling, repeatability and the
refusals.  The shapes sit at the kernel's edges: a 32-wide accumulator tile, a 128-wide work-group tile (one, two and three
per side), 256 respondents per replicate work-group and 128 per chunk of the product."""
import numpy as np
import pytest

from gpirt_amd import _lib

pytestmark = pytest.mark.gpu
CODES = dict(yea=[1], nay=[-1], missing=[None])
# ... and past 128 items, where pair_counts_kernel has several work-group tiles per side: a ragged second tile (129), three
# tiles with a ragged last one (260: the tiles below the diagonal of X^T X are computed once and stored twice), two whole (256)
SHAPES = [(33, 2), (65, 31), (100, 17), (257, 33), (1000, 65), (4097, 96), (257, 129), (300, 260), (130, 256)]
INT_KEYS = _lib.PAIRS_SUMS + _lib.PAIRS_COUNTS
_RUNS = {}


def _responses(n, m, seed):
    """about 3 % NaN; with m > 2 one column without an observed cell and a pair without a co-observed respondent"""
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=seed, na_frac=0.03)
    y = np.array(y, order="F")
    if m > 2:
        y[:, m // 3] = np.nan
        y[: n // 2, 0] = np.nan
        y[n // 2:, 1] = np.nan
    y[n // 2, :] = np.nan
    return y, th0


def _same(got, want, what):
    assert set(INT_KEYS + _lib.PAIRS_FIELDS) <= set(got) and set(INT_KEYS + _lib.PAIRS_FIELDS) <= set(want)
    for k in INT_KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)
    for k in _lib.PAIRS_FIELDS:
        assert np.array_equal(got[k].view(np.int64), want[k].view(np.int64)), (what, k)     # bit for bit, NaN included
    for k in ("pairs", "ppp_or_mid", "log_or_obs"):
        assert np.array_equal(got["extreme"][k], want["extreme"][k], equal_nan=True), (what, "extreme", k)
    for k in ("n", "m", "pair_draws", "pair_skipped"):
        assert got[k] == want[k], (what, k)


def _run(handle, n, m, steps=3):
    """a few steps with ppc_accumulate after each, the last draw's rep / r11 / r1 fetched every time (once per shape)"""
    if (n, m) in _RUNS:
        return _RUNS[(n, m)]
    from gpirt_amd import Sampler
    y, th0 = _responses(n, m, seed=300 + n)
    s = Sampler(handle, y, th0, preset="fast", seed=2**33 + 5)
    s.init()
    s.ppc_enable()
    s.ppc_pairs_enable(top=7)
    const = {k: s.ppc_pairs_get(k) for k in ("n_co", "obs_n11", "obs_n10", "obs_n01", "obs_n00")}
    reps, r11, r1 = [], [], []
    for _ in range(steps):
        s.step()
        s.ppc_accumulate()
        reps.append(s.ppc_pairs_get("rep"))
        r11.append(s.ppc_pairs_get("r11"))
        r1.append(s.ppc_pairs_get("r1"))
    s.check()
    out = dict(y=y, reps=reps, r11=r11, r1=r1, const=const, pairs=s.ppc_pairs(), ppc=s.ppc(),
               raw={k: s.ppc_pairs_get(k) for k in INT_KEYS + _lib.PAIRS_FIELDS + ("counts",)})
    s.close()
    _RUNS[(n, m)] = out
    return out


@pytest.mark.parametrize("n,m", SHAPES)
def test_products_are_exact(handle, n, m):
    r = _run(handle, n, m)
    y = r["y"]
    O = (~np.isnan(y)).astype(np.int64)
    Y = (y > 0).astype(np.int64)
    for rep, r11, r1 in zip(r["reps"], r["r11"], r["r1"]):
        assert rep.dtype == np.int8 and set(np.unique(rep)) <= {0, 1} and rep.any()
        assert not rep[np.isnan(y)].any()
        R = rep.astype(np.int64)
        assert np.array_equal(r11, R.T @ R) and np.array_equal(r1, R.T @ O)
    assert not np.array_equal(r["reps"][0], r["reps"][1])
    n_co, o11, o1 = O.T @ O, Y.T @ Y, Y.T @ O
    live = (n_co > 0) & ~np.eye(m, dtype=bool)
    c = r["const"]
    assert np.array_equal(c["n_co"], n_co.astype(float))
    assert np.array_equal(c["obs_n11"][live], o11[live].astype(float))
    assert np.array_equal(c["obs_n10"][live], (o1 - o11)[live].astype(float))
    assert np.array_equal(c["obs_n01"][live], (o1.T - o11)[live].astype(float))
    assert np.array_equal(c["obs_n00"][live], (n_co - o1 - o1.T + o11)[live].astype(float))
    assert np.isnan(c["obs_n11"][~live]).all()
    if m > 2:
        assert n_co[0, 1] == 0 and (~live).sum() > m


@pytest.mark.parametrize("n,m", SHAPES)
def test_replicate_is_the_ppcs(handle, n, m):
    """summed over the draws, rep's column and row sums are the PPC's own rep_yes_sum"""
    r = _run(handle, n, m)
    tot = sum(rep.astype(np.int64) for rep in r["reps"])
    assert not r["ppc"]["item"]["nonfinite"].any()
    assert np.array_equal(r["ppc"]["item"]["rep_yes_sum"], tot.sum(axis=0).astype(float))
    assert np.array_equal(r["ppc"]["respondent"]["rep_yes_sum"], tot.sum(axis=1).astype(float))


def test_replicate_is_u_below_p(handle):
    """100 x 17, one draw: rep = [u < p] with Handle.item_uniforms' u and the device's own p (GPIRT_SUM_PRED of that draw)"""
    from gpirt_amd import Sampler
    n, m = 100, 17
    y, th0 = _responses(n, m, seed=7)
    seed = 2**40 + 3
    s = Sampler(handle, y, th0, rng="item", seed=seed, theta_stabilise=True)
    s.init()
    s.summary_enable(("pred",))
    s.ppc_enable()
    s.ppc_pairs_enable()
    s.step()
    s.step()
    s.summary_accumulate()
    s.ppc_accumulate()
    it = s.iteration
    p = s.summary_get("p_yes")
    rep = s.ppc_pairs_get("rep")
    s.close()
    u = handle.item_uniforms(seed, it, _lib.ST_PPC, 0, m, n).cpu().numpy()
    assert it == 2 and np.array_equal(rep.astype(bool), ~np.isnan(y) & (u < p))


@pytest.mark.parametrize("n,m", SHAPES)
def test_accumulators_against_pairs_from_rep(handle, n, m):
    from gpirt_amd import ppc as P
    r = _run(handle, n, m)
    want = P.pairs_from_rep(r["y"], np.stack(r["reps"]), top=7)
    _same(r["pairs"], want, "ppc_pairs()")
    for k in INT_KEYS + _lib.PAIRS_FIELDS:           # ... and by name
        assert np.array_equal(r["raw"][k], want[k], equal_nan=True), k
    assert list(r["raw"]["counts"]) == [len(r["reps"]), 0]
    assert r["pairs"]["extreme"]["pairs"].shape == (7, 2)
    if m == 2:
        assert (r["pairs"]["extreme"]["pairs"][1:] == -1).all()


def test_constructed_states(handle):
    """g drawn on the CPU: the device equals pairs_from_draws exactly (no cell within 1e-9 of its uniform: with 1e5 cells
    the expected minimum of |u - p| is 1e-5, so this is a condition on the inputs, no tolerance on the device).  Then
    f = 40 y - mu: rep = Y in every draw.  Then a NaN in one observed cell: the draw is skipped whole for the pairs."""
    from gpirt_amd import Sampler
    from gpirt_amd import ppc as P
    n, m, S, seed = 1000, 100, 3, 5
    rng = np.random.default_rng(8)
    y = np.where(rng.random((n, m)) < 0.5, 1.0, -1.0)
    y[rng.random((n, m)) < 0.03] = np.nan
    y[:, 5] = np.nan
    y[17, :] = np.nan
    y[260, 33] = 1.0
    s = Sampler(handle, y, np.zeros(n), rng="item", seed=seed, theta_stabilise=True)
    s.init()
    s.ppc_enable()
    s.ppc_pairs_enable()
    mu = s.get("mu")
    g, iters = [], []
    for d in range(S):
        f = 2.0 * rng.standard_normal((n, m)) - mu
        s.set_iteration(10 + d)
        s.set("f", f)
        s.ppc_accumulate()
        g.append(f + mu)
        iters.append(10 + d)
    got = s.ppc_pairs()
    want, gap = P.pairs_from_draws(y, np.stack(g), seed, iters)
    print(f"MEASURED min|u - p| {gap:.3e} over {S * int((~np.isnan(y)).sum())} cells")
    assert gap > 1e-9
    _same(got, want, "constructed")
    # rep = Y
    s.ppc_enable()                              # frees the pairs too
    with pytest.raises(_lib.GpirtError):
        s.ppc_pairs_get("counts")
    s.ppc_pairs_enable()
    f = np.where(np.isnan(y), 1.5, 40.0 * y) - mu
    for d in range(S):
        s.set_iteration(20 + d)
        s.set("f", f)
        s.ppc_accumulate()
    assert np.array_equal(s.ppc_pairs_get("rep").astype(bool), y > 0)
    before = s.ppc_pairs()
    live = (before["n_co"] > 0) & ~np.eye(m, dtype=bool)
    for k in ("n11", "agree", "or"):
        assert np.array_equal(before[f"{k}_ge"], (S * live).astype(np.uint32)) and not before[f"{k}_gt"].any(), k
    assert np.array_equal(before["rep_n11_mean"][live], before["obs_n11"][live]) and not before["rep_n11_var"][live].any()
    _same(before, P.pairs_from_rep(y, np.broadcast_to(y > 0, (S, n, m))), "rep = Y")
    # one more draw with a NaN in the observed cell (260, 33)
    ppc_before = s.ppc()
    fbad = f.copy()
    fbad[260, 33] = np.nan
    s.set_iteration(30)
    s.set("f", fbad)
    s.ppc_accumulate()
    after, ppc_after = s.ppc_pairs(), s.ppc()
    assert np.array_equal(s.ppc_pairs_get("rep").astype(bool), y > 0)          # still the last COUNTED draw's
    s.close()
    assert (after["pair_draws"], after["pair_skipped"]) == (S, 1) and before["pair_skipped"] == 0
    after["pair_skipped"] = 0
    _same(after, before, "after the skipped draw")
    nf_i = np.zeros(m)
    nf_i[33] = 1
    assert np.array_equal(ppc_after["item"]["nonfinite"], nf_i) and ppc_after["totals"]["draws"] == S + 1
    took = (ppc_before["item"]["n_obs"] > 0) & (nf_i == 0)
    assert np.array_equal(ppc_after["item"]["yes_ge"][took], ppc_before["item"]["yes_ge"][took] + 1)
    assert ppc_after["item"]["yes_ge"][33] == ppc_before["item"]["yes_ge"][33]


@pytest.mark.parametrize("case", ["fast", "reference"])
def test_chain_and_ppc_untouched(case):
    """gpirtMCMC(ppc=dict(pairs=True)) against ppc=True: draws, IRFs, every PPC output and R's stream position identical"""
    from gpirt_amd import gpirtMCMC
    from gpirt_amd.ops import RStream
    from gpirt_amd.synthetic import make_responses
    n, m, S, B = 96, 12, 4, 2
    y, th0 = make_responses(n, m, seed=31, snap_theta=False)
    kw = dict(vote_codes=CODES, theta_init=th0)
    rs = [None, None]
    if case == "fast":
        kw.update(preset="fast", seed=9)
    else:
        rs = [RStream(77), RStream(77)]
    res = []
    for k, ppc in enumerate((True, dict(pairs=True, top=4))):
        extra = dict(rstream=rs[k]) if rs[k] is not None else {}
        res.append(gpirtMCMC(y, S, B, ppc=ppc, **kw, **extra))
    plain, with_pairs = res
    assert "pairs" not in plain["ppc"] and "pairs" in with_pairs["ppc"]
    for k in ("theta", "beta", "f", "IRFs"):
        assert np.array_equal(plain[k], with_pairs[k], equal_nan=True), k
    for unit in ("item", "respondent"):
        for k, v in plain["ppc"][unit].items():
            assert np.array_equal(v, with_pairs["ppc"][unit][k], equal_nan=True), (unit, k)
    assert plain["ppc"]["totals"] == with_pairs["ppc"]["totals"] or all(
        np.array_equal(v, with_pairs["ppc"]["totals"][k], equal_nan=True) for k, v in plain["ppc"]["totals"].items())
    if case == "reference":
        (mt0, i0), (mt1, i1) = rs[0].state(), rs[1].state()
        assert i0 == i1 and np.array_equal(mt0, mt1)
    pq = with_pairs["ppc"]["pairs"]
    assert pq["pair_draws"] == S and pq["pair_skipped"] == 0 and pq["ppp_or"].shape == (m, m)
    assert pq["extreme"]["pairs"].shape == (4, 2) and (pq["extreme"]["pairs"][:, 0] < pq["extreme"]["pairs"][:, 1]).all()
    if case == "fast":                          # composes with the ranks and the scoring: the same pairs
        both = gpirtMCMC(y, S, B, ppc=dict(pairs=True, top=4), ranks=True, score=dict(data=y[:5], predict=True), **kw)
        assert "ranks" in both and "predict" in both["score"]
        _same(both["ppc"]["pairs"], pq, "with ranks and score")
        assert np.array_equal(both["theta"], plain["theta"])
        with pytest.raises(ValueError):
            gpirtMCMC(y, S, B, ppc=dict(top=4), **kw)
        with pytest.raises(ValueError):
            gpirtMCMC(y, S, B, ppc=dict(pairs=True, top=65), **kw)


def test_state_blocks_untouched_and_repeatable(handle):
    """the stage API with pairs on (twice) and off: the chain's state and the whole PPC state block bit-identical, the two
    pairwise state blocks bit-identical, their layout as the header states it"""
    from gpirt_amd import Sampler
    from gpirt_amd import ppc as P
    n, m = 257, 33
    y, th0 = _responses(n, m, seed=55)
    ppc_blocks, pair_blocks, fs = [], [], []
    for pairs in (True, True, False):
        s = Sampler(handle, y, th0, preset="fast", seed=21)
        s.init()
        s.ppc_enable()
        if pairs:
            s.ppc_pairs_enable()
        for _ in range(3):
            s.step()
            s.ppc_accumulate()
        ppc_blocks.append(s.ppc_state().cpu().numpy().copy())
        if pairs:
            st = s.ppc_pairs_state()
            assert P.pairs_state_header(st) == dict(n=n, m=m, version=1, pair_draws=3, pair_skipped=0, item0=0, tag=0x52494150)
            pair_blocks.append(st.cpu().numpy().copy())
        fs.append((s.get("f"), s.get("theta"), s.get("fstar")))
        s.close()
    assert np.array_equal(ppc_blocks[0], ppc_blocks[2]) and np.array_equal(ppc_blocks[0], ppc_blocks[1])
    for a, b in zip(fs[0], fs[2]):
        assert np.array_equal(a, b)
    pp = m * m
    assert pair_blocks[0].size == 8 + 3 * ((pp + 3) // 4 * 2) + 3 * ((pp + 1) // 2 * 2) + 6 * ((pp + 3) // 4 * 2)
    assert np.array_equal(pair_blocks[0], pair_blocks[1]) and pair_blocks[0][8:].any()


def test_pooled_chains_are_the_sum_of_the_chains():
    from gpirt_amd import gpirtMCMC
    from gpirt_amd.chains import default_inits
    from gpirt_amd.synthetic import make_responses
    n, m, S, B, seed = 80, 10, 5, 2, 13
    y, _ = make_responses(n, m, seed=32, snap_theta=False)
    th0 = default_inits(n, 3, seed)
    kw = dict(vote_codes=CODES, preset="fast", ppc=dict(pairs=True))
    pooled = gpirtMCMC(y, S, B, theta_init=th0, seed=seed, chains=3, **kw)["ppc"]["pairs"]
    singles = [gpirtMCMC(y, S, B, theta_init=th0[c], seed=_lib.chain_seed(seed, c), **kw)["ppc"]["pairs"] for c in range(3)]
    for k in INT_KEYS:
        assert np.array_equal(pooled[k], sum(sg[k] for sg in singles)), k
    for k in ("n_co", "obs_n11", "obs_n10", "obs_n01", "obs_n00", "log_or_obs", "agree_obs"):
        assert np.array_equal(pooled[k], singles[0][k], equal_nan=True), k
    assert pooled["pair_draws"] == 3 * S and pooled["pair_skipped"] == 0
    live = ~np.isnan(pooled["ppp_or"])
    assert np.array_equal(pooled["ppp_or"][live], (pooled["or_ge"] / (3.0 * S))[live])
    assert np.array_equal(pooled["rep_n11_mean"][live], (pooled["sum_n11"] / (3.0 * S))[live])


def test_combine_and_refusals(handle):
    from gpirt_amd import Sampler
    from gpirt_amd import ppc as P
    from gpirt_amd.distributed import ShardedSampler
    from gpirt_amd.synthetic import make_responses
    n, m = 65, 31
    y, th0 = _responses(n, m, seed=56)
    y2 = y.copy()
    y2[3, 4] = np.nan if not np.isnan(y2[3, 4]) else 1.0          # another n_co
    ss = []
    for c, yy in enumerate((y, y, y2)):
        s = Sampler(handle, yy, th0, preset="fast", seed=21 + c)
        s.init()
        if c == 0:
            with pytest.raises(_lib.GpirtError):
                s.ppc_pairs_enable()                               # needs ppc_enable
        s.ppc_enable()
        s.ppc_pairs_enable(top=3)
        for _ in range(2):
            s.step()
            s.ppc_accumulate()
        ss.append(s)
    own = [s.ppc_pairs() for s in ss]
    both = P.pairs_combine(handle, ss[:2], top=3)
    for k in INT_KEYS:
        assert np.array_equal(both[k], own[0][k] + own[1][k]), k
    assert both["pair_draws"] == 4
    with pytest.raises(_lib.GpirtError, match="another response matrix"):
        P.pairs_combine(handle, [ss[0], ss[2]])
    with pytest.raises(_lib.GpirtError):
        P.pairs_combine(handle, [ss[0].ppc_state()])               # a PPC block is no pairwise block
    ss[0].ppc_pairs_enable(on=False)
    with pytest.raises(_lib.GpirtError):
        ss[0].ppc_pairs()
    ss[0].ppc_accumulate()                                         # the PPC itself goes on
    for s in ss:
        s.close()

    ys, ths = make_responses(64, 8, seed=4)

    def factory(yl, th, pm, ps, st, item0, m_total):
        return Sampler(handle, yl, th, pm, ps, st, rng="item", seed=77, item0=item0, m_total=m_total)

    sh = ShardedSampler(factory, ys, ths, dist=None)
    with pytest.raises(ValueError, match="pairwise"):
        sh.ppc_pairs_enable()
    sh.engine.close()
