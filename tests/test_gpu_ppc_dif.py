"""The group-wise item fit (DIF) of the PPC on the device (csrc/ppc_dif.hip) against NumPy: every respondent's cell and the
draw's integer tables against gpirt_amd.ppc.dif_from_draws, every statistic and accumulator bit for bit from the device's own
tables, device against device (the bins' tables, the PPC's yes counts), constructed states, the untouched chain and blocks,
repeatability, pooling with reflection and the refusals.  The shapes cross a wave (64 rows), dif_tables_kernel's 256-row
sub-block and 1024-row work-group, its 8-item strip and dif_update_kernel's 4-item work-group; 6 to 124 cells."""
import numpy as np
import pytest

from gpirt_amd import _lib

pytestmark = pytest.mark.gpu
CODES = dict(yea=[1], nay=[-1], missing=[None])
SHAPES = [(33, 2), (65, 31), (257, 33), (1000, 65), (4097, 96)]
CUT_SETS = {1: (50,), 4: (14, 43, 76, 122), 15: tuple(range(10, 460, 30))}
TABLES = ("cell", "tN", "tT", "tR", "tE", "tV", "stats")
EPS = float(np.finfo(np.float64).eps)
_RUNS = {}


def _responses(n, m, seed):
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=seed, na_frac=0.03)
    y = np.array(y, order="F")
    if m > 2:
        y[:, m // 3] = np.nan
    y[n // 2, :] = np.nan
    return y, th0


def _groups(n, G, th0):
    """about 10 % left out; the last group confined to the upper tail of the starting values; with G = 4 group 2 has one member"""
    rng = np.random.default_rng(n + G)
    g = rng.integers(0, G - 1, size=n)
    g[rng.random(n) < 0.1] = -1
    g[th0 >= np.sort(th0)[-max(n // 8, 2)]] = G - 1
    if G == 4:
        g[g == 2] = 1
        g[1] = 2
    g[0] = 0
    return g


def _run(handle, n, m, G, h, steps=3):
    key = (n, m, G, h)
    if key in _RUNS:
        return _RUNS[key]
    from gpirt_amd import Sampler
    y, th0 = _responses(n, m, seed=400 + n)
    groups = _groups(n, G, th0)
    seed = 2**33 + 7
    s = Sampler(handle, y, th0, preset="fast", seed=seed)
    s.init()
    s.ppc_enable()
    s.ppc_dif_enable(groups, CUT_SETS[h], top=5)
    theta, g, its, tabs = [], [], [], []
    for _ in range(steps):
        s.step()
        s.ppc_accumulate()
        theta.append(s.get("theta"))
        g.append(s.get("f") + s.get("mu"))
        its.append(s.iteration)
        tabs.append({k: s.ppc_dif_get(k) for k in TABLES})
    s.check()
    names = tuple(r[0] for r in _lib.DIF_RAW) + _lib.DIF_CELL_FIELDS + _lib.DIF_GROUP_FIELDS + _lib.DIF_FOCAL_FIELDS + ("occupancy",)
    out = dict(y=y, groups=groups, seed=seed, theta=np.stack(theta), g=np.stack(g), its=its, tabs=tabs, dif=s.ppc_dif(),
               raw={k: s.ppc_dif_get(k) for k in names + ("counts", "cuts", "groups", "group_size")})
    s.close()
    _RUNS[key] = out
    return out


@pytest.mark.parametrize("h", [1, 4, 15])
@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("n,m", SHAPES)
def test_tables_and_statistics_against_numpy(handle, n, m, G, h):
    from gpirt_amd import ppc as P
    r = _run(handle, n, m, G, h)
    cuts, B = CUT_SETS[h], 2 * h + 1
    worst = 0.0
    draws, logabs = [], np.zeros((G, m))
    for d, tab in enumerate(r["tabs"]):
        ref, gap = P.dif_from_draws(r["y"], r["theta"][d:d + 1], r["g"][d:d + 1], r["seed"], r["its"][d:d + 1], r["groups"], cuts)
        assert gap > 1e-9                                # a condition on the inputs: no cell near its uniform
        last = ref["last"]
        assert ref["dif_draws"] == 1
        for k in ("cell", "tN", "tT", "tR"):
            assert np.array_equal(tab[k], last[k]), (k, d)
        # device exp within 1 ulp: a term's rint can differ by one unit of 2^-44, so a cell's sum by at most N units
        N = tab["tN"].astype(np.int64)
        for k in ("tE", "tV"):
            diff = np.abs(tab[k].astype(np.int64) - last[k].astype(np.int64))
            worst = max(worst, float((diff / np.maximum(N, 1)).max()))
            assert (diff <= N).all(), (k, d)
        # the device's own tables through the NumPy statement: every double bit for bit
        st = P.dif_draw_stats(tab["tN"], tab["tT"], tab["tR"], tab["tE"], tab["tV"], G, B)
        assert np.array_equal(tab["stats"], st["stats"], equal_nan=True), d
        logabs += np.abs(st["log_obs"]) + np.abs(st["log_rep"])
        draws.append(dict(N=tab["tN"], T=tab["tT"], R=tab["tR"], E=tab["tE"], V=tab["tV"],
                          occ=np.bincount(tab["cell"][tab["cell"] != 255], minlength=G * B)))
    print(f"{n} x {m}, G = {G}, h = {h}: largest |tE, tV difference| / N = {worst:.3f} units of 2^-44 (bound 1)")
    want = P.dif_from_tables(draws, G, B, m, top=5)
    got = r["dif"]
    for name, dt, _kind in _lib.DIF_RAW:
        if name in ("mh_log_obs_sum", "mh_log_rep_sum"):
            # the library's log within 2 ulp per term; the same terms are then added in the same order
            bound = 2.0 * EPS * logabs + len(draws) * EPS * np.abs(want[name])
            assert (np.abs(got[name] - want[name]) <= bound).all(), name
        else:
            assert np.array_equal(got[name], want[name]), name
        assert np.array_equal(r["raw"][name], got[name]), name            # ... and by name
    for name in _lib.DIF_CELL_FIELDS + _lib.DIF_GROUP_FIELDS + ("occupancy", "std_obs_mean", "std_rep_mean", "ppp_mh", "ppp_mh_mid",
                                                                "mh_undefined", "std_undefined"):
        assert np.array_equal(got[name], want[name], equal_nan=True), name
        assert np.array_equal(r["raw"][name], got[name], equal_nan=True), name
    for k in ("items", "groups", "ppp_mh_mid"):
        assert np.array_equal(got["flagged"][k], want["flagged"][k], equal_nan=True), k
    assert list(r["raw"]["counts"]) == [3, 0] and tuple(r["raw"]["cuts"]) == cuts and got["G"] == G and got["B"] == B
    assert np.array_equal(r["raw"]["groups"], r["groups"].astype(np.int8))
    assert list(got["group_size"]) == [int((r["groups"] == c).sum()) for c in range(G)]
    assert list(r["raw"]["group_size"][:G]) == list(got["group_size"])
    if G == 4:
        assert got["group_size"][2] == 1


def test_against_the_bins_and_the_ppc(handle):
    """everyone grouped, the bins on the same cuts: the groups' tables add up to the bins', and over the bins to the PPC's R"""
    from gpirt_amd import Sampler
    n, m, cuts = 257, 33, CUT_SETS[4]
    y, th0 = _responses(n, m, seed=71)
    s = Sampler(handle, y, th0, preset="fast", seed=5)
    s.init()
    s.ppc_enable()
    s.ppc_bins_enable(cuts)
    s.ppc_dif_enable(np.arange(n) % 3, cuts)
    before = s.ppc_get("item_rep_yes_sum")
    for _ in range(3):
        s.step()
        s.ppc_accumulate()
        for k in ("tN", "tT", "tR"):
            assert np.array_equal(s.ppc_dif_get(k).sum(axis=0), s.ppc_bins_get(k)), k
        now = s.ppc_get("item_rep_yes_sum")
        assert np.array_equal(s.ppc_dif_get("tR").sum(axis=(0, 1)), (now - before).astype(np.int64))
        before = now
    s.close()


def _words(s):
    return s.ppc_dif_state().cpu().numpy().copy()


def test_constructed_states(handle):
    from gpirt_amd import Sampler
    from gpirt_amd import ppc as P
    n, m, seed, cuts = 300, 40, 11, CUT_SETS[4]
    rng = np.random.default_rng(3)
    y = np.where(rng.random((n, m)) < 0.5, 1.0, -1.0)
    y[rng.random((n, m)) < 0.05] = np.nan
    y[260, 33] = y[270, 12] = 1.0
    y[261, 34] = np.nan
    groups = rng.integers(0, 2, size=n)
    groups[270] = -1
    groups[260] = 1
    s = Sampler(handle, y, np.zeros(n), rng="item", seed=seed, theta_stabilise=True)
    s.init()
    s.ppc_enable()
    s.ppc_dif_enable(groups, cuts)
    mu = s.get("mu")
    obs = ~np.isnan(y)

    def draw(it, theta, g):
        s.set_iteration(it)
        s.set("theta", theta)
        s.set("f", g - mu)
        s.ppc_accumulate()
        return np.asarray(s.get("f") + mu)

    th = -5.0 + np.clip(np.rint(500 + 100 * rng.standard_normal(n)), 0, 1000) * 0.01
    g0 = np.where(obs, 1.5 * rng.standard_normal((n, m)), 0.0)
    gd = draw(12, th, g0)
    want, gap = P.dif_from_draws(y, th[None], gd[None], seed, [12], groups, cuts)
    assert gap > 1e-9
    r = s.ppc_dif()
    for k in ("sum_n", "sum_t", "sum_r", "occ_sum", "yes_ge", "yes_gt"):
        assert np.array_equal(r[k], want[k]), k
    assert (r["dif_draws"], r["dif_skipped"]) == (1, 0)
    # skipped: a theta off the grid (a -1 respondent's too), then +-inf and NaN g in an observed cell of a grouped respondent
    before, tabs = _words(s), {k: s.ppc_dif_get(k) for k in TABLES}
    at = (np.arange(n)[:, None] == 260) & (np.arange(m)[None, :] == 33)
    cases = [(np.where(np.arange(n) == 5, 0.005, th), g0), (np.where(np.arange(n) == 270, np.nan, th), g0)]
    cases += [(th, np.where(at, bad, g0)) for bad in (np.inf, -np.inf, np.nan)]
    for it, (tt, gg) in enumerate(cases):
        draw(13 + it, tt, gg)
        after = _words(s)
        assert list(np.flatnonzero(after != before)) == [4] and after[4] == before[4] + 1
        before = after
    for k in TABLES:                                     # still the last COUNTED draw's
        assert np.array_equal(s.ppc_dif_get(k), tabs[k], equal_nan=True), k
    # +-inf and NaN g in a cell of a -1 respondent, and NaN in an unobserved cell: the draw counts
    for q, bad in enumerate((np.inf, -np.inf, np.nan)):
        g2 = g0.copy()
        g2[270, 12] = bad
        g2[261, 34] = np.nan
        draw(20 + q, th, g2)
        assert list(s.ppc_dif_get("counts")) == [2 + q, 5]
    want2, _ = P.dif_from_draws(y, np.stack([th] * 4), np.stack([gd] * 4), seed, [12, 20, 21, 22], groups, cuts)
    r2 = s.ppc_dif()
    for k in ("sum_n", "sum_t", "sum_r", "occ_sum", "yes_ge", "yes_gt"):
        assert np.array_equal(r2[k], want2[k]), k
    s.close()


@pytest.mark.parametrize("case", ["fast", "reference"])
def test_chain_and_other_blocks_untouched(case):
    from gpirt_amd import gpirtMCMC
    from gpirt_amd.ops import RStream
    from gpirt_amd.synthetic import make_responses
    n, m, S, B = 96, 12, 4, 2
    y, th0 = make_responses(n, m, seed=31, snap_theta=False)
    grp = np.arange(n) % 3 - (np.arange(n) % 7 == 0)
    kw = dict(vote_codes=CODES, theta_init=th0)
    base = dict(pairs=True, top=4, bins=(0.25, 1.0), bins_top=3)
    specs = (base, dict(base, dif=grp), True, dict(dif=dict(groups=grp, cuts=(30, 90), top=7)))
    rs = [None] * len(specs)
    if case == "fast":
        kw.update(preset="fast", seed=9)
    else:
        rs = [RStream(77) for _ in specs]
    res = [gpirtMCMC(y, S, B, ppc=spec, **kw, **(dict(rstream=rs[k]) if rs[k] is not None else {})) for k, spec in enumerate(specs)]
    for other in res[1:]:
        for k in ("theta", "beta", "f", "IRFs"):
            assert np.array_equal(res[0][k], other[k], equal_nan=True), k
        for unit in ("item", "respondent"):
            for k, v in res[0]["ppc"][unit].items():
                assert np.array_equal(v, other["ppc"][unit][k], equal_nan=True), (unit, k)
    for blk in ("pairs", "bins"):
        for k, v in res[0]["ppc"][blk].items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v, res[1]["ppc"][blk][k], equal_nan=True), (blk, k)
    if case == "reference":
        for r in rs[1:]:
            (mt0, i0), (mt1, i1) = rs[0].state(), r.state()
            assert i0 == i1 and np.array_equal(mt0, mt1)
    assert "dif" not in res[0]["ppc"] and "dif" not in res[2]["ppc"] and "pairs" not in res[3]["ppc"]
    d1, d3 = res[1]["ppc"]["dif"], res[3]["ppc"]["dif"]
    assert tuple(d1["cuts"]) == (14, 43, 76, 122) and d1["obs_rate"].shape == (3, 9, m) and d1["flagged"]["items"].shape == (20,)
    assert tuple(d3["cuts"]) == (30, 90) and d3["ppp_mh"].shape == (3, m) and d3["flagged"]["items"].shape == (7,)
    for d in (d1, d3):
        assert d["dif_draws"] == S and d["dif_skipped"] == 0 and d["occ_sum"].sum() == S * (grp >= 0).sum()
        assert list(d["group_size"]) == [int((grp == c).sum()) for c in range(3)]
    if case == "fast":
        for bad, word in ((dict(dif=grp[:-1]), "one code per respondent"), (dict(dif=dict(groups=grp, top=65)), "top"),
                          (dict(dif=dict(groups=grp, cuts=(43, 14))), "increasing"), (dict(dif=dict(cuts=(14,))), "groups"),
                          (dict(diff=grp), "dif")):
            with pytest.raises(ValueError, match=word):
                gpirtMCMC(y, S, B, ppc=bad, **kw)


def test_state_block_repeatable_and_others_untouched(handle):
    from gpirt_amd import Sampler
    from gpirt_amd import ppc as P
    n, m, cuts = 257, 33, CUT_SETS[4]
    y, th0 = _responses(n, m, seed=55)
    groups = _groups(n, 4, th0)
    blocks = {k: [] for k in ("ppc", "pairs", "bins", "dif", "f")}
    for dif in (True, True, False):
        s = Sampler(handle, y, th0, preset="fast", seed=21)
        s.init()
        s.ppc_enable()
        s.ppc_pairs_enable()
        s.ppc_bins_enable(cuts)
        if dif:
            s.ppc_dif_enable(groups, cuts)
        for _ in range(3):
            s.step()
            s.ppc_accumulate()
        blocks["ppc"].append(s.ppc_state().cpu().numpy().copy())
        blocks["pairs"].append(s.ppc_pairs_state().cpu().numpy().copy())
        blocks["bins"].append(s.ppc_bins_state().cpu().numpy().copy())
        if dif:
            st = s.ppc_dif_state()
            hdr = P.dif_state_header(st)
            assert hdr == dict(n=n, m=m, version=1, dif_draws=3, dif_skipped=0, item0=0, B=9, tag=0x31464944, cuts=cuts, G=4,
                               group_size=tuple(int((groups == c).sum()) for c in range(4)))
            blocks["dif"].append(st.cpu().numpy().copy())
        blocks["f"].append(np.concatenate([s.get("f").ravel(), s.get("theta"), s.get("fstar").ravel()]))
        s.close()
    for k in ("ppc", "pairs", "bins", "f"):
        assert np.array_equal(blocks[k][0], blocks[k][2]) and np.array_equal(blocks[k][0], blocks[k][1]), k
    assert blocks["dif"][0].tobytes() == blocks["dif"][1].tobytes() and blocks["dif"][0][32:].any()


def test_chains_pool_with_reflection(handle):
    from gpirt_amd import Sampler, gpirtMCMC
    from gpirt_amd import ppc as P
    from gpirt_amd.synthetic import make_responses
    n, m, S, B, seed = 300, 40, 6, 2, 29
    y, th0 = make_responses(n, m, seed=11)
    inits = np.stack([th0, -th0, np.roll(th0, 11)])
    cuts = (30, 90, 150)
    groups = np.arange(n) % 2
    res = gpirtMCMC(y, S, B, vote_codes=CODES, theta_init=inits, rng="item", seed=seed, theta_stabilise=True, chains=3,
                    align=True, ppc=dict(dif=dict(groups=groups, cuts=cuts, top=6)))
    refl = res["diagnostics"]["reflected"]
    assert refl.any() and not refl[0]
    signs = np.where(refl, -1, 1)
    samplers = []
    for c in range(3):
        s = Sampler(handle, y, inits[c], rng="item", seed=_lib.chain_seed(seed, c), theta_stabilise=True)
        s.init()
        s.ppc_enable()
        s.ppc_dif_enable(groups, cuts, top=6)
        for it in range(S + B):
            s.step()
            if it >= B:
                s.ppc_accumulate()
        s.check()
        samplers.append(s)
    pooled = P.dif_combine(handle, samplers, signs=signs, top=6)
    got = res["ppc"]["dif"]
    for k, v in pooled.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, got[k], equal_nan=True), k
    assert pooled["dif_draws"] == 3 * S == got["dif_draws"]
    own = [s.ppc_dif() for s in samplers]
    flip = lambda a, sg: a[:, ::-1] if sg < 0 else a         # noqa: E731
    for name, dt, kind in _lib.DIF_RAW:
        parts = [flip(o[name], sg) if kind in "co" else o[name] for o, sg in zip(own, signs)]
        assert np.array_equal(pooled[name], (parts[0] + parts[1]) + parts[2]), name       # the doubles in chain order
    assert np.array_equal(samplers[0].ppc_dif(sign=-1)["sum_t"], own[0]["sum_t"][:, ::-1])
    # refusals of the combine: other cuts, another group vector, another G, another n, a block of another kind, a bad sign
    y2, th2 = make_responses(n - 1, m, seed=12)
    others = []
    for yy, tt, gg, cc in ((y, th0, groups, (30, 90, 151)), (y, th0, 1 - groups, cuts), (y, th0, np.arange(n) % 3, cuts),
                           (y2, th2, groups[:-1], cuts)):
        o = Sampler(handle, yy, tt, rng="item", seed=3, theta_stabilise=True)
        o.init()
        o.ppc_enable()
        o.ppc_dif_enable(gg, cc)
        others.append(o)
    for o in others:
        with pytest.raises(_lib.GpirtError, match="another n, m, item0, groups or cuts"):
            P.dif_combine(handle, [samplers[0], o])
    with pytest.raises(_lib.GpirtError):
        P.dif_combine(handle, [samplers[0].ppc_dif_state(), samplers[0].ppc_state()])
    with pytest.raises(_lib.GpirtError):
        P.dif_combine(handle, [samplers[0]], signs=[0])
    for s in samplers + others:
        s.close()


def test_refusals(handle):
    import ctypes as C
    from gpirt_amd import Sampler
    from gpirt_amd.distributed import ShardedSampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(65, 31, seed=56)
    grp = np.arange(65) % 2
    s = Sampler(handle, y, th0, preset="fast", seed=21)
    s.init()
    with pytest.raises(_lib.GpirtError, match="ppc_enable"):
        s.ppc_dif_enable(grp)                                # needs ppc_enable
    s.ppc_enable()

    def raw(G, codes, cuts=(50,)):
        a = np.asarray(codes, dtype=np.int32)
        return s.lib.gpirt_sampler_ppc_dif_enable(s._s, G, a.ctypes.data_as(C.POINTER(C.c_int32)), len(cuts), (C.c_int * len(cuts))(*cuts), 1)

    for G, codes in ((1, grp * 0), (5, np.arange(65) % 5), (3, grp), (2, grp - 2), (2, grp + 1)):
        assert raw(G, codes) == _lib.E_ARG, G
    assert raw(2, grp, (43, 14)) == _lib.E_ARG
    assert s.lib.gpirt_sampler_ppc_dif_enable(s._s, 2, None, 1, (C.c_int * 1)(50), 1) == _lib.E_ARG
    assert "no member" in _lib.last_error() or "groups given" in _lib.last_error()
    with pytest.raises(_lib.GpirtError):
        s.ppc_dif_get("counts")                              # nothing was enabled by the refused calls
    # n > 65534 is refused by the argument check, before anything is allocated
    from gpirt_amd import ppc as P
    with pytest.raises(ValueError, match="beyond 65534"):
        P.check_groups(np.zeros(65535, dtype=int), 65535)
    s.ppc_dif_enable(grp, (1, 499))
    s.step()
    s.ppc_accumulate()
    assert list(s.ppc_dif_get("counts")) == [1, 0] and s.ppc_dif_get("sum_N").shape == (2, 5, 31)
    with pytest.raises(_lib.GpirtError):
        s.ppc_dif_get("no_such_field")
    with pytest.raises(ValueError):
        s.ppc_dif(top=65)
    s.ppc_enable()                                           # frees the block too
    with pytest.raises(_lib.GpirtError):
        s.ppc_dif_get("counts")
    s.ppc_dif_enable(grp)
    s.ppc_dif_enable(on=False)
    with pytest.raises(_lib.GpirtError):
        s.ppc_dif()
    s.ppc_accumulate()                                       # the PPC itself goes on
    s.close()

    ys, ths = make_responses(64, 8, seed=4)

    def factory(yl, th, pm, ps, st, item0, m_total):
        return Sampler(handle, yl, th, pm, ps, st, rng="item", seed=77, item0=item0, m_total=m_total)

    sh = ShardedSampler(factory, ys, ths, dist=None)
    with pytest.raises(ValueError, match="group-wise"):
        sh.ppc_dif_enable(np.arange(64) % 2)
    sh.engine.close()
