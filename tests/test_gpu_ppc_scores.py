"""The score-based checks of the PPC on the device (csrc/ppc_scores.hip) against NumPy: every draw's integer tables against
gpirt_amd.ppc.scores_from_draws, every statistic and accumulator bit for bit from the device's own tables, device against device
(the PPC's yes counts), constructed states, the untouched chain and blocks, repeatability, pooling and the refusals.  The shapes
cross a tail word of the bit plane, a wave (64 rows), pass A's 256-row work-group and 32-item strip, pass B's 1024-row work-group
and 8-item strip and the update kernel's 128-item work-group; 2 to 16 score groups."""
import numpy as np
import pytest

from gpirt_amd import _lib

pytestmark = pytest.mark.gpu
SHAPES = [(33, 2), (65, 31), (257, 33), (1000, 65), (4097, 96)]
LAST = tuple(r[0] for r in _lib.SCORES_LAST)
CONST = tuple(r[0] for r in _lib.SCORES_CONST)
FIELDS = _lib.SCORES_HIST_FIELDS + _lib.SCORES_VAR_FIELDS + _lib.SCORES_ITEM_FIELDS + _lib.SCORES_CELL_FIELDS
_RUNS = {}


def _responses(n, m, seed):
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=seed, na_frac=0.03)
    y = np.array(y, order="F")
    if m > 2:
        y[:, m // 3] = np.nan
    y[n // 2, :] = np.nan
    return y, th0


def _cuts(m, K):
    """K - 1 ascending cuts in 1 .. m - 1, spread over the scores (K is cut down to m where m - 1 cuts do not exist)"""
    K = min(K, m)
    return tuple(sorted({1 + (k * (m - 1)) // K for k in range(K)} - {0}))[:K - 1] if m > 2 else (1,)


def _run(handle, n, m, K, steps=3):
    key = (n, m, K)
    if key in _RUNS:
        return _RUNS[key]
    from gpirt_amd import Sampler
    y, th0 = _responses(n, m, seed=400 + n)
    cuts = _cuts(m, K)
    seed = 2**33 + 7
    s = Sampler(handle, y, th0, preset="fast", seed=seed)
    s.init()
    s.ppc_enable()
    s.ppc_scores_enable(cuts, top=5)
    const = {k: s.ppc_scores_get(k) for k in CONST + ("x_obs", "cuts", "group_lo", "group_hi")}
    g, its, tabs, ppc_first = [], [], [], None
    for d in range(steps):
        s.step()
        s.ppc_accumulate()
        g.append(s.get("f") + s.get("mu"))
        its.append(s.iteration)
        tabs.append({k: s.ppc_scores_get(k) for k in LAST})
        if d == 0:
            ppc_first = {k: s.ppc_get(k) for k in ("respondent_rep_yes_sum", "item_n_obs", "item_obs_yes")}
            ppc_first["total"] = s.ppc_totals()["rep_yes_sum"]
    s.check()
    names = tuple(r[0] for r in _lib.SCORES_RAW) + FIELDS
    out = dict(y=y, cuts=cuts, seed=seed, g=np.stack(g), its=its, tabs=tabs, const=const, ppc_first=ppc_first, res=s.ppc_scores(),
               raw={k: s.ppc_scores_get(k) for k in names + ("counts",)})
    s.close()
    _RUNS[key] = out
    return out


@pytest.mark.parametrize("K", [2, 5, 16])
@pytest.mark.parametrize("n,m", SHAPES)
def test_tables_and_statistics_against_numpy(handle, n, m, K):
    from gpirt_amd import ppc as P
    r = _run(handle, n, m, K)
    cuts, const = r["cuts"], r["const"]
    Kk = len(cuts) + 1
    # the constants, counted on the device at enable, against the data
    want_obs = P.scores_observed(r["y"], cuts)
    assert np.array_equal(const["x_obs"], want_obs["x"]) and np.array_equal(const["hist_obs"], want_obs["hist"])
    assert np.array_equal(const["sums_obs"], want_obs["sums"]) and list(const["var_obs"]) == list(want_obs["var"])
    assert np.array_equal(const["tNo"], want_obs["No"]) and np.array_equal(const["tT"], want_obs["T"])
    assert np.array_equal(const["r_obs"], want_obs["r"], equal_nan=True)
    assert tuple(const["cuts"]) == cuts and const["group_lo"][0] == 0 and const["group_hi"][-1] == m - 1
    obs = P.scores_observed_from_arrays(cuts, const["hist_obs"], const["sums_obs"], const["tNo"], const["tT"], const["x_obs"])
    worst = 0.0
    draws = []
    for d, tab in enumerate(r["tabs"]):
        ref, gap = P.scores_from_draws(r["y"], r["g"][d:d + 1], r["seed"], r["its"][d:d + 1], cuts)
        assert gap > 1e-9                                # a condition on the inputs: no cell near its uniform
        last = ref["last"]
        assert ref["score_draws"] == 1
        for k in ("xr", "hist", "sums", "tNr", "tR"):
            assert np.array_equal(tab[k], last[k]), (k, d)
        # device exp within 1 ulp: a term's rint can differ by one unit of 2^-44, so a cell's sum by at most N units
        for k, N in (("tEo", const["tNo"]), ("tVo", const["tNo"]), ("tEr", tab["tNr"]), ("tVr", tab["tNr"])):
            N = N.astype(np.int64)
            diff = np.abs(tab[k] - last[k])
            worst = max(worst, float((diff / np.maximum(N, 1)).max()))
            assert (diff <= N).all(), (k, d)
        # the device's own tables through the NumPy statement: every double bit for bit
        own = dict(obs=obs, xr=tab["xr"], hist=tab["hist"], sums=tab["sums"], Nr=tab["tNr"], R=tab["tR"], Eo=tab["tEo"],
                   Vo=tab["tVo"], Er=tab["tEr"], Vr=tab["tVr"])
        st = P.scores_draw_stats(own)
        assert np.array_equal(tab["r"], st["r"], equal_nan=True), d
        assert np.array_equal(tab["chi"], st["chi"]), d
        draws.append(own)
    print(f"{n} x {m}, K = {Kk}: largest |tE, tV difference| / N = {worst:.3f} units of 2^-44 (bound 1)")
    want = P.scores_from_tables(draws, top=5)
    got = r["res"]
    for name, _dt, _kind in _lib.SCORES_RAW:
        assert np.array_equal(got[name], want[name], equal_nan=True), name
        assert got[name].dtype == want[name].dtype, name
        assert np.array_equal(r["raw"][name], got[name], equal_nan=True), name            # ... and by name
    for name in FIELDS:
        assert np.array_equal(got[name], want[name], equal_nan=True), name
        assert np.array_equal(r["raw"][name], got[name], equal_nan=True), name
    for k in ("items", "ppp_chi2_mid"):
        assert np.array_equal(got["worst"][k], want["worst"][k], equal_nan=True), k
    for k in ("cuts", "group_lo", "group_hi"):
        assert np.array_equal(got[k], want[k]), k
    assert list(r["raw"]["counts"]) == [3, 0] and (got["score_draws"], got["score_skipped"], got["K"]) == (3, 0, Kk)
    assert got["n_scored"] == want["n_scored"] == int((~np.isnan(r["y"])).any(axis=1).sum()) and (got["n"], got["m"]) == (n, m)
    # device against device, after the first counted draw: the PPC's own counts
    first, pf = r["tabs"][0], r["ppc_first"]
    assert np.array_equal(first["xr"], pf["respondent_rep_yes_sum"].astype(np.int64))
    assert int((np.arange(m + 1) * first["hist"]).sum()) == int(pf["total"])           # sum_s s H[s] is the PPC's total
    assert np.array_equal(const["tNo"].sum(axis=0), pf["item_n_obs"].astype(np.int64))
    assert np.array_equal(const["tT"].sum(axis=0), pf["item_obs_yes"].astype(np.int64))
    assert np.array_equal(first["tNr"].sum(axis=0), pf["item_n_obs"].astype(np.int64))


def _words(s):
    return s.ppc_scores_state().cpu().numpy().copy()


def test_constructed_states(handle):
    from gpirt_amd import Sampler
    from gpirt_amd import ppc as P
    n, m, seed, cuts = 300, 40, 11, (5, 12, 20, 30)
    rng = np.random.default_rng(3)
    y = np.where(rng.random((n, m)) < 0.5, 1.0, -1.0)
    y[rng.random((n, m)) < 0.05] = np.nan
    y[260, 33] = 1.0
    y[261, 34] = np.nan
    y[17] = np.nan
    s = Sampler(handle, y, np.zeros(n), rng="item", seed=seed, theta_stabilise=True)
    s.init()
    s.ppc_enable()
    s.ppc_scores_enable(cuts)
    mu = s.get("mu")
    obs = ~np.isnan(y)

    def draw(it, g):
        s.set_iteration(it)
        s.set("f", g - mu)
        s.ppc_accumulate()
        return np.asarray(s.get("f") + mu)

    # |g| = 40 everywhere: the replicate is deterministic (p is 1 or 4e-18 against a uniform of 53 bits)
    sign = np.where(rng.random((n, m)) < 0.5, 1.0, -1.0)
    gd = draw(12, 40.0 * sign)
    assert (np.abs(gd) > 39.0).all()
    assert np.array_equal(s.ppc_scores_get("xr"), (obs & (sign > 0)).sum(axis=1))
    want, gap = P.scores_from_draws(y, gd[None], seed, [12], cuts)
    assert gap > 1e-9
    r = s.ppc_scores()
    for k in ("hist_sum", "hist_ge", "cdf_gt", "var_ge", "var_rep_sum", "r_ge", "r_undefined_count", "cell_ge", "cell_empty", "sum_nr",
              "sum_r", "chi_ge"):
        assert np.array_equal(r[k], want[k]), k
    assert np.array_equal(s.ppc_scores_get("r"), want["last"]["r"], equal_nan=True)
    # all positive g: Xr = the observed count, every correlation undefined, the last group holds every cell with a rest score
    # of 30 or more and the replicate's yes rate is 1 wherever a cell is
    s.ppc_scores_enable(cuts)
    draw(13, np.full((n, m), 40.0))
    nobs = obs.sum(axis=1)
    assert np.array_equal(s.ppc_scores_get("xr"), nobs) and np.array_equal(s.ppc_get("respondent_n_obs").astype(np.int64), nobs)
    assert (s.ppc_scores_get("r_undefined_count") == 1).all() and np.isnan(s.ppc_scores_get("r")).all()
    tNr, tR = s.ppc_scores_get("tNr"), s.ppc_scores_get("tR")
    assert np.array_equal(tNr, tR) and np.array_equal(tNr.sum(axis=0), obs.sum(axis=0)) and nobs[nobs > 0].min() > 30
    assert not tNr[:-1].any()                            # one group holds everything
    assert list(s.ppc_scores_get("counts")) == [1, 0]
    # skipped: +-inf and NaN g in an observed cell -- only the counter moves
    g0 = np.where(obs, 1.5 * rng.standard_normal((n, m)), 0.0)
    draw(14, g0)
    before, tabs = _words(s), {k: s.ppc_scores_get(k) for k in LAST}
    at = (np.arange(n)[:, None] == 260) & (np.arange(m)[None, :] == 33)
    for q, bad in enumerate((np.inf, -np.inf, np.nan)):
        draw(15 + q, np.where(at, bad, g0))
        after = _words(s)
        assert list(np.flatnonzero(after != before)) == [6] and after[6] == before[6] + 1
        before = after
    for k in LAST:                                       # still the last COUNTED draw's
        assert np.array_equal(s.ppc_scores_get(k), tabs[k], equal_nan=True), k
    # NaN and inf in missing cells (a whole missing row too): the draw counts, and nothing of it differs
    g2 = g0.copy()
    g2[261, 34] = np.nan
    g2[17] = np.inf
    draw(14, g2)
    assert list(s.ppc_scores_get("counts")) == [3, 3]
    for k in LAST:
        assert np.array_equal(s.ppc_scores_get(k), tabs[k], equal_nan=True), k
    s.close()


def test_state_block_repeatable_and_others_untouched(handle):
    from gpirt_amd import Sampler
    from gpirt_amd import ppc as P
    n, m, cuts = 257, 33, (14, 43, 76, 122)
    y, th0 = _responses(n, m, seed=55)
    groups = np.arange(n) % 3
    blocks = {k: [] for k in ("ppc", "pairs", "bins", "dif", "scores", "chain")}
    for scores in (True, True, False):
        s = Sampler(handle, y, th0, preset="fast", seed=21)
        s.init()
        s.ppc_enable()
        s.ppc_pairs_enable()
        s.ppc_bins_enable(cuts)
        s.ppc_dif_enable(groups, cuts)
        if scores:
            s.ppc_scores_enable()                        # the default cuts
        for _ in range(3):
            s.step()
            s.ppc_accumulate()
        blocks["ppc"].append(s.ppc_state().cpu().numpy().copy())
        blocks["pairs"].append(s.ppc_pairs_state().cpu().numpy().copy())
        blocks["bins"].append(s.ppc_bins_state().cpu().numpy().copy())
        blocks["dif"].append(s.ppc_dif_state().cpu().numpy().copy())
        if scores:
            st = s.ppc_scores_state()
            hdr = P.scores_state_header(st)
            want = P.default_score_cuts(y)
            assert hdr == dict(tag=0x31524353, version=1, n=n, m=m, K=len(want) + 1, score_draws=3, score_skipped=0, cuts=want)
            assert len(want) >= 3
            blocks["scores"].append(st.cpu().numpy().copy())
        blocks["chain"].append(np.concatenate([s.get("f").ravel(), s.get("theta"), s.get("beta").ravel(), s.get("fstar").ravel(),
                                               [float(s.iteration)]]))
        s.close()
    for k in ("ppc", "pairs", "bins", "dif", "chain"):
        assert blocks[k][0].tobytes() == blocks[k][2].tobytes() and blocks[k][0].tobytes() == blocks[k][1].tobytes(), k
    assert blocks["scores"][0].tobytes() == blocks["scores"][1].tobytes() and blocks["scores"][0][24:].any()


def test_chains_pool(handle):
    from gpirt_amd import Sampler
    from gpirt_amd import ppc as P
    from gpirt_amd.synthetic import make_responses
    n, m, cuts, seed = 300, 40, (8, 16, 24), 29
    y, th0 = make_responses(n, m, seed=11)
    # two chains from other starting values, and one state that is handed every draw of both, in chain order
    both = Sampler(handle, y, th0, rng="item", seed=seed, theta_stabilise=True)
    both.init()
    both.ppc_enable()
    both.ppc_scores_enable(cuts, top=6)
    samplers = []
    for c, draws in enumerate((3, 2)):
        s = Sampler(handle, y, th0 if c == 0 else -th0, rng="item", seed=seed, theta_stabilise=True)
        s.init()
        s.ppc_enable()
        s.ppc_scores_enable(cuts, top=6)
        for _ in range(draws):
            s.step()
            s.ppc_accumulate()
            both.set_iteration(s.iteration)
            both.set("mu", s.get("mu"))
            both.set("f", s.get("f"))
            both.ppc_accumulate()
        samplers.append(s)
    own = [s.ppc_scores() for s in samplers]
    pooled = P.scores_combine(handle, samplers, top=6)
    single = both.ppc_scores()
    eps = float(np.finfo(np.float64).eps)
    for name, dt, kind in _lib.SCORES_RAW:
        want = own[0][name] if (name, dt, kind) in _lib.SCORES_CONST else own[0][name] + own[1][name]       # the doubles in chain order
        assert np.array_equal(pooled[name], want, equal_nan=True), name
        if dt != "f8":
            assert np.array_equal(pooled[name], single[name]), name
        elif (name, dt, kind) not in _lib.SCORES_CONST:
            # the same five terms, ((a + b) + c) + (d + e) against (((a + b) + c) + d) + e: four roundings each, every partial sum
            # at most sum |term|, which is at most 5 for the correlations and the sum itself for the others (terms >= 0)
            bound = 8.0 * eps * np.maximum(np.abs(pooled[name]), 5.0)
            assert (np.abs(pooled[name] - single[name]) <= bound).all(), name
    assert pooled["score_draws"] == 5 == single["score_draws"] and pooled["worst"]["items"].shape == (6,)
    both.close()
    # refusals of the combine: other cuts, another m, another response matrix, a block of another kind
    y2, th2 = make_responses(n, m - 1, seed=12)
    y3 = y.copy()
    y3[5, 7] = -y3[5, 7]
    others = []
    for yy, tt, cc in ((y, th0, (8, 16, 25)), (y, th0, (8, 16)), (y2, th2, cuts), (y3, th0, cuts)):
        o = Sampler(handle, yy, tt, rng="item", seed=3, theta_stabilise=True)
        o.init()
        o.ppc_enable()
        o.ppc_scores_enable(cc)
        others.append(o)
    for o in others:
        with pytest.raises(_lib.GpirtError, match="another n, m, K, cuts or response matrix"):
            P.scores_combine(handle, [samplers[0], o])
    with pytest.raises(_lib.GpirtError):
        P.scores_combine(handle, [samplers[0].ppc_scores_state(), samplers[0].ppc_state()])
    with pytest.raises(ValueError):
        P.scores_combine(handle, [samplers[0].ppc_state()])
    for s in samplers + others:
        s.close()


def test_refusals(handle):
    import ctypes as C
    from gpirt_amd import Sampler
    from gpirt_amd import ppc as P
    from gpirt_amd.distributed import ShardedSampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(65, 31, seed=56)
    s = Sampler(handle, y, th0, preset="fast", seed=21)
    s.init()
    with pytest.raises(_lib.GpirtError, match="ppc_enable"):
        s.ppc_scores_enable((5, 10))                         # needs ppc_enable
    s.ppc_enable()

    def raw(K, cuts):
        return s.lib.gpirt_sampler_ppc_scores_enable(s._s, K, (C.c_int * len(cuts))(*cuts) if cuts else None, 1)

    for K, cuts, word in ((1, (5,), "1 score groups"), (17, tuple(range(1, 17)), "17 score groups"), (3, (10, 5), "increasing"),
                          (3, (5, 5), "increasing"), (3, (5, 31), "in 1..30"), (3, (0, 5), "in 1..30"), (3, None, "score groups")):
        assert raw(K, cuts) == _lib.E_ARG and word in _lib.last_error(), (K, cuts)
    with pytest.raises(_lib.GpirtError):
        s.ppc_scores_get("counts")                           # nothing was enabled by the refused calls
    # n > 65534 is refused by the argument check, before anything is allocated
    assert s.lib.gpirt_ppc_scores_check(65535, 31, 2, (C.c_int * 1)(5)) == _lib.E_ARG and "beyond 65534" in _lib.last_error()
    with pytest.raises(ValueError, match="beyond 65534"):
        P.check_score_cuts((5,), 31, n=65535)
    for bad, word in (((10, 5), "increasing"), ((), "1 score groups")):
        with pytest.raises(ValueError, match=word):
            s.ppc_scores_enable(bad)
    with pytest.raises(ValueError, match="top must be"):
        s.ppc_scores_enable((5,), top=65)
    s.ppc_scores_enable((1, 30))
    s.step()
    s.ppc_accumulate()
    assert list(s.ppc_scores_get("counts")) == [1, 0] and s.ppc_scores_get("sum_nr").shape == (3, 31)
    with pytest.raises(ValueError, match="unknown field"):
        s.ppc_scores_get("no_such_field")
    assert s.lib.gpirt_sampler_ppc_scores_get(s._s, b"no_such_field", C.c_void_p(y.ctypes.data), 8) == _lib.E_ARG
    assert "unknown score-based PPC field" in _lib.last_error()
    with pytest.raises(ValueError):
        s.ppc_scores(top=65)
    s.ppc_enable()                                           # frees the block too
    with pytest.raises(_lib.GpirtError):
        s.ppc_scores_get("counts")
    s.ppc_scores_enable((5,))
    s.ppc_scores_enable(on=False)
    with pytest.raises(_lib.GpirtError):
        s.ppc_scores()
    s.ppc_accumulate()                                       # the PPC itself goes on
    s.close()

    ys, ths = make_responses(64, 8, seed=4)

    def factory(yl, th, pm, ps, st, item0, m_total):
        return Sampler(handle, yl, th, pm, ps, st, rng="item", seed=77, item0=item0, m_total=m_total)

    sh = ShardedSampler(factory, ys, ths, dist=None)
    with pytest.raises(ValueError, match="score-based"):
        sh.ppc_scores_enable((2, 4))
    # ... and by the library itself on a sampler that holds a shard of the items
    part = Sampler(handle, ys[:, :4], ths, rng="item", seed=77, item0=4, m_total=8)
    part.init()
    part.ppc_enable()
    with pytest.raises(_lib.GpirtError, match="item shards"):
        part.ppc_scores_enable((2,))
    part.close()
    sh.engine.close()
