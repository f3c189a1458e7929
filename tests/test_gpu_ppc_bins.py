"""The theta-binned item fit of the PPC on the device (csrc/ppc_bins.hip and the BINS instances of ppc_replicate_kernel) against
NumPy: every respondent's bin and the last draw's tables, every accumulator against gpirt_amd.ppc.bins_from_rep (integers bit
for bit, doubles within the bounds tests/_bins_bounds.py derives), constructed states, the untouched chain / PPC block / pairs
block, repeatability, pooling with reflection and the refusals.  The shapes are the smallest that cross the kernel's edges: a
wave (64 rows), a work-group (256 rows: one, two, 17 row blocks), a strip of 32 items (one, two, three, five strips, ragged
last ones); every one with 3, 9 and 31 bins.  h = 1 and 15 run with the pairs on (ppc_replicate_kernel<true, true>; the
replicate is then read from the pairs), h = 4 without (<false, true>; the replicate from replicate_uniforms)."""
import numpy as np
import pytest

from gpirt_amd import _lib

from _bins_bounds import DOUBLE_KEYS, INT_KEYS, check_accumulators, check_tables, same_result

pytestmark = pytest.mark.gpu
CODES = dict(yea=[1], nay=[-1], missing=[None])
SHAPES = [(33, 2), (65, 31), (100, 17), (257, 33), (1000, 65), (4097, 96), (257, 129)]
CUT_SETS = {1: (50,), 4: (14, 43, 76, 122), 15: tuple(range(10, 460, 30))}
TABLES = ("bin", "tN", "tT", "tR", "tE", "tV")
_RUNS = {}


def _grid(k):
    return -5.0 + np.asarray(k, dtype=np.float64) * 0.01


def _responses(n, m, seed):
    """about 3 % NaN; with m > 2 one column without an observed cell; one respondent who answered nothing"""
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=seed, na_frac=0.03)
    y = np.array(y, order="F")
    if m > 2:
        y[:, m // 3] = np.nan
    y[n // 2, :] = np.nan
    return y, th0


def _run(handle, n, m, h, steps=3):
    """a few steps with ppc_accumulate after each; theta, g, the replicate and the last draw's tables fetched every time"""
    key = (n, m, h)
    if key in _RUNS:
        return _RUNS[key]
    from gpirt_amd import Sampler
    from gpirt_amd import ppc as P
    y, th0 = _responses(n, m, seed=400 + n)
    seed = 2**33 + 7
    s = Sampler(handle, y, th0, preset="fast", seed=seed)
    s.init()
    s.ppc_enable()
    pairs = h != 4
    if pairs:
        s.ppc_pairs_enable()
    s.ppc_bins_enable(CUT_SETS[h], top=5)
    theta, g, reps, tabs = [], [], [], []
    for _ in range(steps):
        s.step()
        s.ppc_accumulate()
        theta.append(s.get("theta"))
        g.append(s.get("f") + s.get("mu"))
        if pairs:
            reps.append(s.ppc_pairs_get("rep"))
        else:
            p, _e = P._plogis(np.where(np.isnan(y), 0.0, g[-1]))
            u = P.replicate_uniforms(seed, s.iteration, n, m)
            assert np.abs(u - p)[~np.isnan(y)].min() > 1e-9      # a condition on the inputs: no cell near its uniform
            reps.append(~np.isnan(y) & (u < p))
        tabs.append({k: s.ppc_bins_get(k) for k in TABLES})
    s.check()
    names = tuple(r[0] for r in _lib.BINS_RAW) + _lib.BINS_CELL_FIELDS + _lib.BINS_ITEM_FIELDS + _lib.BINS_BIN_FIELDS
    out = dict(y=y, theta=np.stack(theta), g=np.stack(g), reps=np.stack(reps), tabs=tabs, bins=s.ppc_bins(),
               raw={k: s.ppc_bins_get(k) for k in names + ("counts", "cuts")})
    s.close()
    _RUNS[key] = out
    return out


@pytest.mark.parametrize("h", [1, 4, 15])
@pytest.mark.parametrize("n,m", SHAPES)
def test_bins_and_tables_against_numpy(handle, n, m, h):
    from gpirt_amd import ppc as P
    from gpirt_amd.quantiles import grid_index
    r = _run(handle, n, m, h)
    cuts = CUT_SETS[h]
    for d, tab in enumerate(r["tabs"]):
        k = grid_index(r["theta"][d])
        assert (k >= 0).all()
        assert np.array_equal(tab["bin"], P.bin_of_index(k, cuts).astype(np.uint8))
        one = P.bins_from_rep(r["y"], r["theta"][d:d + 1], r["g"][d:d + 1], r["reps"][d:d + 1], cuts)
        assert one["bin_draws"] == 1
        check_tables(tab, one["last"], f"{n} x {m}, h = {h}, draw {d}")
    if h > 1:                                        # (the first cut of h = 1 lies at 0.50: a short chain may sit inside it)
        assert len(np.unique(r["tabs"][-1]["bin"])) > 1


@pytest.mark.parametrize("h", [1, 4, 15])
@pytest.mark.parametrize("n,m", SHAPES)
def test_accumulators_against_bins_from_rep(handle, n, m, h):
    from gpirt_amd import ppc as P
    r = _run(handle, n, m, h)
    want = P.bins_from_rep(r["y"], r["theta"], r["g"], r["reps"], CUT_SETS[h], top=5)
    check_accumulators(r["bins"], want, f"{n} x {m}, h = {h}")
    for k in INT_KEYS + DOUBLE_KEYS + ("chi_ge", "chi_gt") + _lib.BINS_CELL_FIELDS + _lib.BINS_ITEM_FIELDS + _lib.BINS_BIN_FIELDS:
        assert np.array_equal(r["raw"][k], r["bins"][k], equal_nan=True), k       # ... and by name
    assert list(r["raw"]["counts"]) == [3, 0] and tuple(r["raw"]["cuts"]) == CUT_SETS[h]
    assert r["bins"]["worst"]["items"].shape == (5,)
    if m > 2:                                        # the item nobody answered: empty everywhere, an integer tie in every draw
        j = m // 3
        assert not r["bins"]["sum_n"][:, j].any() and (r["bins"]["cell_empty"][:, j] == 3).all()
        assert r["bins"]["chi_ge"][j] == 3 and r["bins"]["chi_gt"][j] == 0 and np.isnan(r["bins"]["obs_rate"][:, j]).all()


def _words(s):
    return s.ppc_bins_state().cpu().numpy().copy()


def test_constructed_states(handle):
    from gpirt_amd import Sampler
    from gpirt_amd import ppc as P
    n, m, seed, cuts = 300, 40, 11, (14, 43, 76, 122)
    h, B = 4, 9
    rng = np.random.default_rng(3)
    y = np.where(rng.random((n, m)) < 0.5, 1.0, -1.0)
    y[rng.random((n, m)) < 0.05] = np.nan
    y[260, 33] = 1.0
    y[261, 34] = np.nan
    y[0, 7] = np.nan                                     # item 7 will be unobserved in bin 0
    s = Sampler(handle, y, np.zeros(n), rng="item", seed=seed, theta_stabilise=True)
    s.init()
    s.ppc_enable()
    s.ppc_bins_enable(cuts)
    mu = s.get("mu")
    obs = ~np.isnan(y)

    def draw(it, theta, g):
        s.set_iteration(it)
        s.set("theta", theta)
        s.set("f", g - mu)
        s.ppc_accumulate()
        return np.asarray(s.get("f") + mu)               # g as the device forms it

    def reference(thetas, gs, its):
        want, gap = P.bins_from_draws(y, np.stack(thetas), np.stack(gs), seed, its, cuts)
        assert gap > 1e-9
        return want

    # everyone in the centre bin: the other bins have N = 0 and only cell_empty moves
    g0 = 1.5 * rng.standard_normal((n, m))
    gd = draw(10, np.zeros(n), g0)
    r = s.ppc_bins()
    check_accumulators(r, reference([np.zeros(n)], [gd], [10]), "centre bin")
    off = np.arange(B) != h
    assert (r["cell_empty"][off] == 1).all() and not r["cell_empty"][h, obs.any(axis=0)].any()
    for k in ("sum_n", "sum_t", "sum_r", "sum_e", "sum_z", "cell_ge", "cell_gt"):
        assert not r[k][off].any(), k
    assert np.array_equal(r["occ_sum"], np.where(off, 0, n).astype(np.uint64))
    assert np.array_equal(s.ppc_bins_get("tN")[h], obs.sum(axis=0).astype(np.int32))
    # one respondent per bin, the others in the centre; item 7 unobserved in bin 0
    s.ppc_bins_enable(cuts)
    lo, hi = P.bin_edges(cuts)
    th = np.zeros(n)
    th[:B] = _grid(np.rint((np.where(np.arange(B) == h, 0.0, (lo + hi) / 2) + 5.0) * 100.0))
    gd = draw(11, th, g0)
    r = s.ppc_bins()
    want = reference([th], [gd], [11])
    check_accumulators(r, want, "one respondent per bin")
    assert np.array_equal(s.ppc_bins_get("bin")[:B], np.arange(B).astype(np.uint8))
    assert np.array_equal(r["occ_sum"], np.where(off, 1, n - B + 1).astype(np.uint64))
    assert np.array_equal(r["sum_n"][off], obs[:B][off].astype(np.uint64))
    empty = ~obs[:B][off]
    assert empty[0, 7] and np.array_equal(r["cell_empty"][off], empty.astype(np.uint32))
    # g = +-800 (p = 0 or 1, V = 0: no z, a zero term) and g = +-40 on items 0 and 1, the extremes agreeing with y
    s.ppc_bins_enable(cuts)
    g1 = g0.copy()
    g1[:, 0] = np.where(y[:, 0] > 0, 800.0, -800.0)
    g1[:, 1] = np.where(y[:, 1] > 0, 40.0, -40.0)
    g1[:, 2] = np.where(rng.random(n) < 0.5, 40.0, -40.0)
    th = _grid(np.clip(np.rint(500 + 100 * rng.standard_normal(n)), 0, 1000))
    gd12 = draw(12, th, np.where(obs, g1, 0.0))
    r = s.ppc_bins()
    check_accumulators(r, reference([th], [gd12], [12]), "g = +-800, +-40")
    assert not s.ppc_bins_get("tV")[:, 0].any() and not r["sum_z"][:, 0].any() and r["chi_obs_sum"][0] == 0.0
    assert np.array_equal(r["sum_e"][:, 0], r["sum_t"][:, 0].astype(float)) and r["chi_ge"][0] == 1 and r["chi_gt"][0] == 0
    assert np.array_equal(r["sum_r"][:, 1], r["sum_t"][:, 1]) and (s.ppc_bins_get("tV")[:, 1][r["sum_n"][:, 1] > 0] > 0).all()
    assert np.isfinite(r["sum_z"]).all() and np.isfinite(r["chi_rep_sum"]).all()
    # skipped draws: one theta off the grid, then one NaN g in an observed cell -- only bin_skipped moves
    before, tabs = _words(s), {k: s.ppc_bins_get(k) for k in TABLES}
    for it, (tt, gg) in enumerate(((np.where(np.arange(n) == 5, 0.005, th), g1), (np.where(np.arange(n) == 5, np.nan, th), g1),
                                   (th, np.where((np.arange(n)[:, None] == 260) & (np.arange(m)[None, :] == 33), np.nan, g1)))):
        draw(13 + it, tt, np.where(obs, gg, 0.0))
        after = _words(s)
        assert after[4] == before[4] + 1 and after[3] == before[3] == 1
        changed = np.flatnonzero(after != before)
        assert list(changed) == [4], changed
        before = after
    for k in TABLES:                                     # still the last COUNTED draw's
        assert np.array_equal(s.ppc_bins_get(k), tabs[k]), k
    # a NaN g in an UNOBSERVED cell counts normally
    g2 = np.where(obs, g1, 0.0)
    g2[261, 34] = np.nan
    gd = draw(16, th, g2)
    r2 = s.ppc_bins()
    assert (r2["bin_draws"], r2["bin_skipped"]) == (2, 3)
    gclean = gd.copy()
    gclean[261, 34] = 0.0
    want2 = reference([th, th], [gd12, gclean], [12, 16])
    want2["bin_skipped"] = 3                             # (the reference saw only the two counted draws)
    check_accumulators(r2, want2, "NaN in an unobserved cell")
    s.close()


@pytest.mark.parametrize("case", ["fast", "reference"])
def test_chain_ppc_and_pairs_untouched(case):
    """gpirtMCMC(ppc=dict(pairs=True, bins=True)) against ppc=dict(pairs=True): draws, IRFs, every PPC and pairs output and R's
    stream position identical; ppc=dict(bins=cuts) alone against ppc=True likewise"""
    from gpirt_amd import gpirtMCMC
    from gpirt_amd.ops import RStream
    from gpirt_amd.synthetic import make_responses
    n, m, S, B = 96, 12, 4, 2
    y, th0 = make_responses(n, m, seed=31, snap_theta=False)
    kw = dict(vote_codes=CODES, theta_init=th0)
    specs = (True, dict(bins=(0.25, 1.0), bins_top=3), dict(pairs=True, top=4), dict(pairs=True, top=4, bins=True))
    rs = [None] * len(specs)
    if case == "fast":
        kw.update(preset="fast", seed=9)
    else:
        rs = [RStream(77) for _ in specs]
    res = [gpirtMCMC(y, S, B, ppc=spec, **kw, **(dict(rstream=rs[k]) if rs[k] is not None else {})) for k, spec in enumerate(specs)]
    plain = res[0]
    for other in res[1:]:
        for k in ("theta", "beta", "f", "IRFs"):
            assert np.array_equal(plain[k], other[k], equal_nan=True), k
        for unit in ("item", "respondent"):
            for k, v in plain["ppc"][unit].items():
                assert np.array_equal(v, other["ppc"][unit][k], equal_nan=True), (unit, k)
        assert all(np.array_equal(v, other["ppc"]["totals"][k], equal_nan=True) for k, v in plain["ppc"]["totals"].items())
    for k, v in res[2]["ppc"]["pairs"].items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, res[3]["ppc"]["pairs"][k], equal_nan=True), k
    if case == "reference":
        for r in rs[1:]:
            (mt0, i0), (mt1, i1) = rs[0].state(), r.state()
            assert i0 == i1 and np.array_equal(mt0, mt1)
    assert "bins" not in plain["ppc"] and "bins" not in res[2]["ppc"] and "pairs" not in res[1]["ppc"]
    b1, b3 = res[1]["ppc"]["bins"], res[3]["ppc"]["bins"]
    assert tuple(b1["cuts"]) == (25, 100) and b1["B"] == 5 and b1["worst"]["items"].shape == (3,)
    assert tuple(b3["cuts"]) == (14, 43, 76, 122) and b3["obs_rate"].shape == (9, m) and b3["worst"]["items"].shape == (20,)
    for b in (b1, b3):
        assert b["bin_draws"] == S and b["bin_skipped"] == 0 and b["occ_sum"].sum() == S * n
        assert np.array_equal(b["sum_t"].sum(axis=0), (S * (y > 0).sum(axis=0)).astype(np.uint64))
    if case == "fast":
        with pytest.raises(ValueError):
            gpirtMCMC(y, S, B, ppc=dict(bins_top=4), **kw)
        with pytest.raises(ValueError):
            gpirtMCMC(y, S, B, ppc=dict(bins=(43, 14)), **kw)
        with pytest.raises(ValueError):
            gpirtMCMC(y, S, B, ppc=dict(bins=True, bins_top=65), **kw)


def test_state_blocks_untouched_and_repeatable(handle):
    """the stage API with the bins on (twice) and off, the pairs on throughout: the chain's state, the whole PPC state block and
    the whole pairs state block bit-identical, the two bins state blocks byte-identical, their layout as the header states it"""
    from gpirt_amd import Sampler
    from gpirt_amd import ppc as P
    n, m, cuts = 257, 33, (14, 43, 76, 122)
    y, th0 = _responses(n, m, seed=55)
    ppc_blocks, pair_blocks, bin_blocks, fs = [], [], [], []
    for bins in (True, True, False):
        s = Sampler(handle, y, th0, preset="fast", seed=21)
        s.init()
        s.ppc_enable()
        s.ppc_pairs_enable()
        if bins:
            s.ppc_bins_enable(cuts)
        for _ in range(3):
            s.step()
            s.ppc_accumulate()
        ppc_blocks.append(s.ppc_state().cpu().numpy().copy())
        pair_blocks.append(s.ppc_pairs_state().cpu().numpy().copy())
        if bins:
            st = s.ppc_bins_state()
            assert P.bins_state_header(st) == dict(n=n, m=m, version=1, bin_draws=3, bin_skipped=0, item0=0, B=9, tag=0x534E4942,
                                                   cuts=cuts)
            bin_blocks.append(st.cpu().numpy().copy())
        fs.append((s.get("f"), s.get("theta"), s.get("fstar")))
        s.close()
    assert np.array_equal(ppc_blocks[0], ppc_blocks[2]) and np.array_equal(ppc_blocks[0], ppc_blocks[1])
    assert np.array_equal(pair_blocks[0], pair_blocks[2]) and np.array_equal(pair_blocks[0], pair_blocks[1])
    for a, b in zip(fs[0], fs[2]):
        assert np.array_equal(a, b)
    c = 9 * m
    even = lambda words: (words + 1) // 2 * 2                 # noqa: E731
    assert bin_blocks[0].size == 8 + 16 + 5 * even(c) + 3 * even((c + 1) // 2) + 2 * even((m + 1) // 2) + 2 * even(m) + even(9)
    assert bin_blocks[0].tobytes() == bin_blocks[1].tobytes() and bin_blocks[0][24:].any()
    assert list(bin_blocks[0][8:24]) == list(cuts) + [0] * 12


def test_chains_pool_with_reflection(handle):
    """chains=3, chain 1 started at -theta0: res["ppc"]["bins"] equals bins_combine of the three chains' stage-API state blocks
    with the signs res["diagnostics"]["reflected"] reports; explicit signs (+1, -1) against NumPy"""
    from gpirt_amd import Sampler, gpirtMCMC
    from gpirt_amd import ppc as P
    from gpirt_amd.synthetic import make_responses
    n, m, S, B, seed = 300, 40, 6, 2, 29
    y, th0 = make_responses(n, m, seed=11)
    inits = np.stack([th0, -th0, np.roll(th0, 11)])
    cuts = (30, 90, 150)
    res = gpirtMCMC(y, S, B, vote_codes=CODES, theta_init=inits, rng="item", seed=seed, theta_stabilise=True, chains=3,
                    align=True, ppc=dict(bins=cuts, bins_top=6))
    refl = res["diagnostics"]["reflected"]
    assert refl.any() and not refl[0]
    signs = np.where(refl, -1, 1)
    samplers = []
    for c in range(3):
        s = Sampler(handle, y, inits[c], rng="item", seed=_lib.chain_seed(seed, c), theta_stabilise=True)
        s.init()
        s.ppc_enable()
        s.ppc_bins_enable(cuts, top=6)
        for it in range(S + B):
            s.step()
            if it >= B:
                s.ppc_accumulate()
        s.check()
        samplers.append(s)
    pooled = P.bins_combine(handle, samplers, signs=signs, top=6)
    same_result(pooled, res["ppc"]["bins"], "chains=3")
    assert pooled["bin_draws"] == 3 * S
    own = [s.ppc_bins() for s in samplers]
    flip = lambda a, sg: a[::-1] if sg < 0 else a            # noqa: E731
    for k in INT_KEYS:
        assert np.array_equal(pooled[k], sum(flip(o[k], sg) for o, sg in zip(own, signs))), k
    for k in ("chi_ge", "chi_gt"):
        assert np.array_equal(pooled[k], sum(o[k] for o in own)), k
    for k in ("sum_e", "sum_z"):                             # the doubles in chain order
        assert np.array_equal(pooled[k], (flip(own[0][k], signs[0]) + flip(own[1][k], signs[1])) + flip(own[2][k], signs[2])), k
    assert np.array_equal(pooled["chi_obs_sum"], (own[0]["chi_obs_sum"] + own[1]["chi_obs_sum"]) + own[2]["chi_obs_sum"])
    # explicit signs: a state pooled with its own mirror image is symmetric in the bins
    st = samplers[0].ppc_bins_state()
    sym = P.bins_combine(handle, [st, st.clone()], signs=[1, -1])
    for k in INT_KEYS + ("sum_e", "obs_rate", "n_mean", "occupancy"):
        assert np.array_equal(sym[k], sym[k][::-1], equal_nan=True), k
    assert np.array_equal(sym["sum_n"], own[0]["sum_n"] + own[0]["sum_n"][::-1])
    assert np.array_equal(samplers[0].ppc_bins(sign=-1)["sum_t"], own[0]["sum_t"][::-1])
    unaligned = P.bins_combine(handle, samplers)
    assert np.array_equal(unaligned["sum_n"], sum(o["sum_n"] for o in own))
    # refusals of the combine: other cuts, another n, another m, a block of another kind, a bad sign
    y2, th2 = make_responses(n - 1, m, seed=12)
    y3, th3 = make_responses(n, m - 1, seed=13)
    others = []
    for yy, tt, cc in ((y, th0, (30, 90, 151)), (y, th0, (30, 90)), (y2, th2, cuts), (y3, th3, cuts)):
        o = Sampler(handle, yy, tt, rng="item", seed=3, theta_stabilise=True)
        o.init()
        o.ppc_enable()
        o.ppc_bins_enable(cc)
        others.append(o)
    for o in others:
        with pytest.raises(_lib.GpirtError, match="another n, m, item0 or cuts"):
            P.bins_combine(handle, [samplers[0], o])
    with pytest.raises(_lib.GpirtError):
        P.bins_combine(handle, [samplers[0].ppc_bins_state(), samplers[0].ppc_state()])
    with pytest.raises(_lib.GpirtError):
        P.bins_combine(handle, [samplers[0]], signs=[0])
    for s in samplers + others:
        s.close()


def test_refusals(handle):
    import ctypes as C
    from gpirt_amd import Sampler
    from gpirt_amd.distributed import ShardedSampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(65, 31, seed=56)
    s = Sampler(handle, y, th0, preset="fast", seed=21)
    s.init()
    with pytest.raises(_lib.GpirtError):
        s.ppc_bins_enable()                                  # needs ppc_enable
    s.ppc_enable()

    def raw(cuts):
        return s.lib.gpirt_sampler_ppc_bins_enable(s._s, len(cuts), (C.c_int * max(len(cuts), 1))(*cuts), 1)

    for bad in ((), tuple(range(1, 17)), (0,), (500,), (43, 14), (14, 14), (-3, 5)):
        assert raw(bad) == _lib.E_ARG, bad
        with pytest.raises(ValueError):
            s.ppc_bins_enable(bad)
    assert s.lib.gpirt_sampler_ppc_bins_enable(s._s, 4, None, 1) == _lib.E_ARG
    with pytest.raises(_lib.GpirtError):
        s.ppc_bins_get("counts")                             # nothing was enabled by the refused calls
    s.ppc_bins_enable((1, 499))
    s.step()
    s.ppc_accumulate()
    assert list(s.ppc_bins_get("counts")) == [1, 0] and s.ppc_bins_get("sum_N").shape == (5, 31)
    with pytest.raises(_lib.GpirtError):
        s.ppc_bins_get("no_such_field")
    with pytest.raises(ValueError):
        s.ppc_bins(top=65)
    s.ppc_enable()                                           # frees the bins too
    with pytest.raises(_lib.GpirtError):
        s.ppc_bins_get("counts")
    s.ppc_bins_enable()
    s.ppc_bins_enable(on=False)
    with pytest.raises(_lib.GpirtError):
        s.ppc_bins()
    s.ppc_accumulate()                                       # the PPC itself goes on
    s.close()

    ys, ths = make_responses(64, 8, seed=4)

    def factory(yl, th, pm, ps, st, item0, m_total):
        return Sampler(handle, yl, th, pm, ps, st, rng="item", seed=77, item0=item0, m_total=m_total)

    sh = ShardedSampler(factory, ys, ths, dist=None)
    with pytest.raises(ValueError, match="theta-binned"):
        sh.ppc_bins_enable()
    sh.engine.close()
