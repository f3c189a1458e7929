"""The residual correlations of the PPC on the device (csrc/ppc_resid.hip) against NumPy: the terms within one unit of 2^-22 of
gpirt_amd.ppc.resid_terms on the fetched f + mu, the int8 digit-plane products exactly, everything after the integer tables bit
for bit (gpirt_amd.ppc.resid_draw_stats / resid_from_tables fed the device's own tables), constructed states, the untouched chain
and other PPC blocks, pooling, repeatability and the refusals.  The shapes sit at the kernels' edges: a 32-wide accumulator tile,
a 128-wide work-group tile (one, two and three per side), 16 items and 256 respondents per work-group of the terms kernel, 128
respondents per chunk of the product, 64 lanes of the item sums."""
import numpy as np
import pytest

from gpirt_amd import _lib
from test_gpu_ppc_pairs import _responses

pytestmark = pytest.mark.gpu
SHAPES = [(33, 2), (65, 31), (100, 17), (257, 33), (1000, 65), (257, 129), (300, 260), (130, 256)]
RAW = tuple(nm for nm, _, _ in _lib.RESID_RAW)
FIELDS = _lib.RESID_PAIR_FIELDS + _lib.RESID_ITEM_FIELDS
LAST = ("d_obs", "d_rep", "w", "s_obs", "s_rep", "v", "r_obs", "r_rep", "stats")
U = 2 ** 22
_RUNS = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64) if a.dtype == np.float64 else a


def _same(got, want, what):
    for k in RAW:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)
    for k in FIELDS:
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (what, k)                      # bit for bit, NaN included
    for k in _lib.RESID_SCALARS:
        assert np.array_equal(_bits(np.array([got[k]])), _bits(np.array([want[k]]))), (what, k, got[k], want[k])
    for lst in ("worst", "worst_items"):
        for k in got[lst]:
            assert np.array_equal(got[lst][k], want[lst][k], equal_nan=True), (what, lst, k)
    for k in ("n", "m", "resid_draws", "resid_skipped", "global_undefined"):
        assert got[k] == want[k], (what, k)


def _run(handle, n, m, steps=3):
    """three steps with ppc_accumulate after each, the last draw's arrays fetched every time (once per shape); the pairs block is on
    beside, for its replicate"""
    if (n, m) in _RUNS:
        return _RUNS[(n, m)]
    from gpirt_amd import Sampler
    y, th0 = _responses(n, m, seed=300 + n)
    s = Sampler(handle, y, th0, preset="fast", seed=2**33 + 5)
    s.init()
    s.ppc_enable()
    s.ppc_pairs_enable()
    s.ppc_resid_enable(top=7)
    draws = []
    for _ in range(steps):
        s.step()
        s.ppc_accumulate()
        d = {k: s.ppc_resid_get(k) for k in LAST}
        d.update(g=s.get("f") + s.get("mu"), rep=s.ppc_pairs_get("rep"), digits=s.ppc_resid_get("digits"))
        draws.append(d)
    s.check()
    out = dict(y=y, draws=draws, resid=s.ppc_resid(), raw={k: s.ppc_resid_get(k) for k in RAW + FIELDS + ("scalars", "counts")})
    s.close()
    _RUNS[(n, m)] = out
    return out


@pytest.mark.parametrize("n,m", SHAPES)
def test_terms(handle, n, m):
    """0 at unobserved cells; the replicate is the PPC's (the pairs block's bytes); every cell within ONE unit of resid_terms on
    the fetched f + mu: the device's exp is within 1 ulp of NumPy's, p, q and p q follow by a few roundings, and a relative error
    of a few 2^-53 moves rint(x 2^22) by at most one unit, at a tie."""
    from gpirt_amd import ppc as P
    r = _run(handle, n, m)
    y = r["y"]
    obs = ~np.isnan(y)
    differ = cells = 0
    for d in r["draws"]:
        assert d["d_obs"].dtype == np.int32 and d["d_obs"].shape == (n, m)
        for k in ("d_obs", "d_rep", "w"):
            assert not d[k][~obs].any(), k
        rep = d["rep"].astype(bool)
        same = obs & (rep == (y > 0))
        assert np.array_equal(d["d_rep"][same], d["d_obs"][same])
        flip = obs & ~same                                     # +q against -p of the same cell: rint(q U) + rint(p U) = U +- 1
        gap = np.where(rep, 1, -1)[flip] * (d["d_rep"][flip].astype(np.int64) - d["d_obs"][flip])
        assert flip.any() and (np.abs(gap - U) <= 1).all()
        assert (d["d_rep"][obs & rep] >= 0).all() and (d["d_rep"][obs & ~rep] <= 0).all()
        want = P.resid_terms(y, d["g"], rep)
        for k, wk in zip(("d_obs", "d_rep", "w"), want):
            err = np.abs(d[k].astype(np.int64) - wk)
            assert err.max() <= 1, (k, int(err.max()))
            differ += int((err != 0).sum())
            cells += int(obs.sum())
        # the planes are the digits of the terms
        dg = d["digits"]
        assert dg.dtype == np.int8 and dg.shape == (9, n, m)
        for t, k in enumerate(("d_obs", "d_rep", "w")):
            assert np.array_equal(P.resid_join(dg[3 * t], dg[3 * t + 1], dg[3 * t + 2]), d[k]), k
            for u, dig in enumerate(P.resid_digits(d[k])):
                assert np.array_equal(dig, dg[3 * t + u]), (k, u)
    print(f"MEASURED {n} x {m}: {differ} of {cells} terms differ from NumPy's by one unit")
    assert not np.array_equal(r["draws"][0]["d_rep"], r["draws"][1]["d_rep"])


@pytest.mark.parametrize("n,m", SHAPES)
def test_products_are_exact(handle, n, m):
    from gpirt_amd import ppc as P
    r = _run(handle, n, m)
    O = (~np.isnan(r["y"])).astype(np.int64)
    lows = np.concatenate([d["digits"][[0, 1, 3, 4, 6, 7]].ravel() for d in r["draws"]])
    if n * m >= 1000:                                          # the carries were exercised
        assert lows.min() == -128 and lows.max() == 127
        for d in r["draws"]:
            for u in (0, 1, 3, 4):
                assert d["digits"][u].min() == -128 and d["digits"][u].max() == 127, u
    for d in r["draws"]:
        want = P.resid_tables(d["d_obs"], d["d_rep"], d["w"], O)
        for k in ("s_obs", "s_rep", "v"):
            assert d[k].dtype == np.int64 and np.array_equal(d[k], want[k]), k
    n_co = O.T @ O
    assert np.array_equal(r["raw"]["n_co_int"], n_co) and np.array_equal(r["raw"]["n_co"], n_co.astype(float))
    if m > 2:
        assert n_co[0, 1] == 0


@pytest.mark.parametrize("n,m", SHAPES)
def test_everything_after_the_integers_bit_for_bit(handle, n, m):
    from gpirt_amd import ppc as P
    r = _run(handle, n, m)
    n_co = r["raw"]["n_co_int"]
    for d in r["draws"]:
        st = P.resid_draw_stats(d, n_co)
        for k in ("r_obs", "r_rep", "stats"):
            assert np.array_equal(_bits(d[k]), _bits(st[k])), k
        assert np.array_equal(_bits(d["r_obs"]), _bits(d["r_obs"].T.copy()))
    want = P.resid_from_tables(r["draws"], n_co, top=7, n=n)
    _same(r["resid"], want, "ppc_resid()")
    for k in RAW + FIELDS:                                     # ... and by name
        assert np.array_equal(_bits(r["raw"][k]), _bits(want[k])), k
    assert np.array_equal(_bits(r["raw"]["scalars"]), _bits(np.array([want[k] for k in _lib.RESID_SCALARS])))
    assert list(r["raw"]["counts"]) == [len(r["draws"]), 0, want["global_undefined"]]
    assert r["resid"]["worst"]["pairs"].shape == (7, 2) and r["resid"]["worst_items"]["items"].shape == (7,)
    if m == 2:
        assert (r["resid"]["worst"]["pairs"][1:] == -1).all() and (r["resid"]["worst_items"]["items"][2:] == -1).all()
    else:
        live = (n_co > 0) & ~np.eye(m, dtype=bool)
        assert np.isnan(r["resid"]["ppp_rc"][~live]).all() and not np.isnan(r["resid"]["ppp_rc"][live]).any()
        assert np.isnan(r["resid"]["infit_obs_mean"][m // 3]) and np.isnan(r["resid"]["ss_obs_mean"][m // 3])
        assert r["resid"]["global_undefined"] == 0 and np.isfinite(r["resid"]["frob_obs_mean"])


def _constructed(handle, n=300, m=40, seed=5):
    from gpirt_amd import Sampler
    rng = np.random.default_rng(8)
    y = np.where(rng.random((n, m)) < 0.5, 1.0, -1.0)
    y[rng.random((n, m)) < 0.03] = np.nan
    y[:, 7] = np.nan
    y[17, :] = np.nan
    y[260, 33] = 1.0
    y[261, 33] = np.nan
    s = Sampler(handle, y, np.zeros(n), rng="item", seed=seed, theta_stabilise=True)
    s.init()
    s.ppc_enable()
    s.ppc_resid_enable()
    return s, y, rng


def test_constructed_extreme_g(handle):
    """g = +40 y and +inf y (dt = 0, w = 0), -40 y and -inf y (dt_obs = +-2^22, dt_rep = 0, w = 0) in four columns: each of their
    pairs and their infit is undefined in every draw, nothing else is"""
    from gpirt_amd import ppc as P
    s, y, rng = _constructed(handle)
    n, m = y.shape
    S = 3
    mu = s.get("mu")
    ysign = np.where(np.isnan(y), 1.0, y)
    tabs = []
    for d in range(S):
        g = 1.5 * rng.standard_normal((n, m))
        g[:, 0], g[:, 1], g[:, 2], g[:, 3] = 40.0 * ysign[:, 0], np.inf * ysign[:, 1], -40.0 * ysign[:, 2], -np.inf * ysign[:, 3]
        s.set_iteration(10 + d)
        s.set("f", g - mu)
        s.ppc_accumulate()
        got = {k: s.ppc_resid_get(k) for k in LAST}
        obs = ~np.isnan(y)
        assert not got["d_obs"][:, :2].any() and not got["d_rep"][:, :4].any() and not got["w"][:, :4].any()
        for c in (2, 3):                                       # every answer as surprising as can be; the replicate never is
            assert np.array_equal(got["d_obs"][:, c], np.where(obs[:, c], U * ysign[:, c], 0).astype(np.int32))
            assert got["s_obs"][c, c] == int(obs[:, c].sum()) * 2 ** 44 and got["s_rep"][c, c] == 0
        assert got["s_obs"][2, 3] == int((np.where(obs[:, 2], ysign[:, 2], 0) * np.where(obs[:, 3], ysign[:, 3], 0)).sum()) * 2 ** 44
        tabs.append(got)
    r = s.ppc_resid()
    n_co = r["n_co_int"]
    touched = np.zeros((m, m), dtype=bool)
    touched[:4, :] = touched[:, :4] = True
    assert np.array_equal(r["undefined_count"], (S * (touched & (n_co > 0))).astype(np.uint32))
    assert r["undefined_count"][:4, :4].sum() == 16 * S and (r["resid_draws"], r["resid_skipped"], r["global_undefined"]) == (S, 0, 0)
    assert np.isnan(r["infit_obs_mean"][:4]).all() and not np.isnan(np.delete(r["infit_obs_mean"], [0, 1, 2, 3, 7])).any()
    assert np.isnan(r["ppp_rc"][:4]).all() and np.array_equal(r["undefined"][0, 4:7], np.full(3, float(S)))
    _same(r, P.resid_from_tables(tabs, n_co, n=n), "extreme g")
    s.close()


def test_constructed_nan_and_ties(handle):
    """A NaN in an observed cell skips the draw whole and leaves the block as it was but for resid_skipped; a NaN in an unobserved
    cell changes nothing; where every answer equals the replicate's, S_rep = S_obs and rc_ge - rc_gt counts every draw.  (S[a, b]
    holds item b's replicate too, so the tie needs the whole matrix; g is built from the PPC's own uniforms so that u < p exactly
    where y = +1, with |g| <= 30 so that every item's sum of w stays above 0.)"""
    from gpirt_amd import ppc as P
    s, y, rng = _constructed(handle)
    n, m = y.shape
    S, seed = 3, 5
    mu = s.get("mu")
    obs = ~np.isnan(y)
    gs = [1.5 * rng.standard_normal((n, m)) for _ in range(S)]
    hole = gs[1].copy()
    hole[261, 33] = np.nan                                      # unobserved
    blocks = []
    for draws in (gs, [gs[0], hole, gs[2]]):
        s.ppc_enable()                                          # frees the block too
        with pytest.raises(_lib.GpirtError, match="not enabled"):
            s.ppc_resid_get("counts")
        s.ppc_resid_enable()
        for d, g in enumerate(draws):
            s.set_iteration(10 + d)
            s.set("f", g - mu)
            s.ppc_accumulate()
        blocks.append(s.ppc_resid_state().cpu().numpy().copy())
    assert blocks[0].tobytes() == blocks[1].tobytes() and blocks[0][3] == S and blocks[0][4] == 0
    # one more draw with a NaN in the observed cell (260, 33)
    last = {k: s.ppc_resid_get(k) for k in LAST + ("digits",)}
    bad = gs[0].copy()
    bad[260, 33] = np.nan
    s.set_iteration(20)
    s.set("f", bad - mu)
    s.ppc_accumulate()
    after = s.ppc_resid_state().cpu().numpy().copy()
    assert after[4] == 1 and after[3] == S
    after[4] = 0
    assert after.tobytes() == blocks[1].tobytes()
    for k, v in last.items():                                  # still the last COUNTED draw's
        assert np.array_equal(_bits(s.ppc_resid_get(k)), _bits(v)), k
    assert list(s.ppc_resid_get("counts")) == [S, 1, 0]
    # the replicate equal to the data everywhere
    s.ppc_enable()
    s.ppc_resid_enable()
    for d in range(S):
        u = P.replicate_uniforms(seed, 30 + d, n, m)
        far = np.maximum(u, 1.0 - u)
        g = np.where(obs, y, 1.0) * np.maximum(1.0, np.log(far / (1.0 - far)) + 0.5)
        assert np.abs(g).max() <= 30.0
        s.set_iteration(30 + d)
        s.set("f", g - mu)
        s.ppc_accumulate()
        assert np.array_equal(s.ppc_resid_get("d_rep"), s.ppc_resid_get("d_obs"))
        assert np.array_equal(s.ppc_resid_get("s_rep"), s.ppc_resid_get("s_obs"))
    r = s.ppc_resid()
    live = r["n_co_int"] > 0
    assert not r["undefined_count"].any()
    assert np.array_equal(r["rc_ge"], (S * live).astype(np.uint32)) and not r["rc_gt"].any()
    assert np.array_equal(r["ss_ge"], (S * np.diag(live)).astype(np.uint32)) and not r["ss_gt"].any()
    off = live & ~np.eye(m, dtype=bool)
    assert (r["ppp_rc_mid"][off] == 0.5).all() and r["ppp_frob_mid"] == 0.5 and r["ppp_max_mid"] == 0.5 and r["ppp_absmax_mid"] == 0.5
    assert np.array_equal(r["rc_obs_sum"], r["rc_rep_sum"]) and r["frob_obs_mean"] == r["frob_rep_mean"]
    s.close()


@pytest.mark.parametrize("case", ["fast", "reference"])
def test_others_untouched_and_repeatable(handle, case):
    """the stage API with the block on (twice) and off: the chain's state, R's stream position and the state blocks of the PPC,
    pairs, bins, dif, scores and person byte-identical; the two residual state blocks byte-identical, their layout as the header
    states it"""
    from gpirt_amd import Sampler
    from gpirt_amd import ppc as P
    from gpirt_amd.ops import RStream
    n, m, cuts = 257, 33, (14, 43, 76, 122)
    y, th0 = _responses(n, m, seed=55)
    groups = np.arange(n) % 3
    blocks = {k: [] for k in ("ppc", "pairs", "bins", "dif", "scores", "person", "resid", "chain", "rs")}
    for resid in (True, True, False):
        rs = RStream(77) if case == "reference" else None
        kw = dict(preset="fast", seed=21) if case == "fast" else dict(rng="reference", rstream=rs, theta_stabilise=False)
        s = Sampler(handle, y, th0, **kw)
        s.init()
        s.ppc_enable()
        s.ppc_pairs_enable()
        s.ppc_bins_enable(cuts)
        s.ppc_dif_enable(groups, cuts)
        s.ppc_scores_enable()
        s.ppc_person_enable()
        if resid:
            s.ppc_resid_enable()
        for _ in range(3):
            s.step()
            s.ppc_accumulate()
        for k in ("ppc", "pairs", "bins", "dif", "scores", "person"):
            blocks[k].append(getattr(s, "ppc_state" if k == "ppc" else f"ppc_{k}_state")().cpu().numpy().copy())
        if resid:
            st = s.ppc_resid_state()
            assert P.resid_state_header(st) == dict(n=n, m=m, version=1, resid_draws=3, resid_skipped=0, item0=0, tag=0x31445352)
            blocks["resid"].append(st.cpu().numpy().copy())
        blocks["chain"].append(np.concatenate([s.get("f").ravel(), s.get("theta"), s.get("beta").ravel(), s.get("fstar").ravel(),
                                               [float(s.iteration)]]))
        if rs is not None:
            mt, idx = rs.state()
            blocks["rs"].append(np.concatenate([np.asarray(mt, dtype=np.int64).ravel(), [int(idx)]]))
        s.close()
    for k in ("ppc", "pairs", "bins", "dif", "scores", "person", "chain") + (("rs",) if case == "reference" else ()):
        assert blocks[k][0].tobytes() == blocks[k][2].tobytes() and blocks[k][0].tobytes() == blocks[k][1].tobytes(), k
    pp = m * m
    wide, narrow = (pp + 1) // 2 * 2, (pp + 3) // 4 * 2
    assert blocks["resid"][0].size == 8 + 4 * wide + 3 * narrow + 3 * ((m + 3) // 4 * 2) + 2 * ((m + 1) // 2 * 2) + 16
    assert blocks["resid"][0].tobytes() == blocks["resid"][1].tobytes() and blocks["resid"][0][8 + wide:].any()


def test_pooling_and_refusals(handle):
    from gpirt_amd import Sampler
    from gpirt_amd import ppc as P
    from gpirt_amd.distributed import ShardedSampler
    from gpirt_amd.synthetic import make_responses
    n, m = 65, 31
    y, th0 = _responses(n, m, seed=56)
    y2 = y.copy()
    y2[3, 4] = np.nan if not np.isnan(y2[3, 4]) else 1.0          # another n_co
    ss, tabs = [], []
    for c, (yy, steps) in enumerate(((y, 2), (y, 3), (y2, 2))):
        s = Sampler(handle, yy, th0, preset="fast", seed=21 + c)
        s.init()
        if c == 0:
            with pytest.raises(_lib.GpirtError, match="posterior predictive"):
                s.ppc_resid_enable()                               # needs ppc_enable
        s.ppc_enable()
        if c == 0:
            for top in (65, -1, 2.5):
                with pytest.raises(_lib.GpirtError, match="top = .* is outside 1..64"):
                    s.ppc_resid_enable(top=top)
            with pytest.raises(_lib.GpirtError, match="not enabled"):
                s.ppc_resid()
        s.ppc_resid_enable(top=3)
        for _ in range(steps):
            s.step()
            s.ppc_accumulate()
            if c < 2:
                tabs.append({k: s.ppc_resid_get(k) for k in ("s_obs", "s_rep", "v")})
        ss.append(s)
    both = P.resid_combine(handle, ss[:2], top=3)
    want = P.resid_from_tables(tabs, ss[0].ppc_resid_get("n_co_int"), top=3, n=n, chains=[2, 3])
    _same(both, want, "two chains")
    own = [s.ppc_resid() for s in ss[:2]]
    assert both["resid_draws"] == 5 and np.array_equal(both["rc_ge"], own[0]["rc_ge"] + own[1]["rc_ge"])
    assert np.array_equal(both["rc_rep_sum"], own[0]["rc_rep_sum"] + own[1]["rc_rep_sum"])
    with pytest.raises(_lib.GpirtError, match="another response matrix"):
        P.resid_combine(handle, [ss[0], ss[2]])
    with pytest.raises(_lib.GpirtError, match="not a residual PPC state block"):
        P.resid_combine(handle, [ss[0].ppc_state()])               # a PPC block is no residual block
    with pytest.raises(ValueError):
        P.resid_combine(handle, ss[:2], top=0)
    with pytest.raises(_lib.GpirtError, match="unknown residual PPC field"):
        ss[0].ppc_resid_get("no_such_field")
    ss[0].ppc_resid_enable(on=False)
    with pytest.raises(_lib.GpirtError, match="not enabled"):
        ss[0].ppc_resid()
    ss[0].ppc_accumulate()                                         # the PPC itself goes on
    for s in ss:
        s.close()
    # another n or m
    ya, tha = _responses(65, 17, seed=57)
    yb, thb = _responses(33, 17, seed=58)
    pair = []
    for yy, th in ((ya, tha), (yb, thb)):
        s = Sampler(handle, yy, th, preset="fast", seed=3)
        s.init()
        s.ppc_enable()
        s.ppc_resid_enable()
        pair.append(s)
    with pytest.raises(_lib.GpirtError, match="another n, m or item0"):
        P.resid_combine(handle, pair)
    for s in pair:
        s.close()
    # m out of range
    y1, th1 = make_responses(40, 1, seed=4)
    s = Sampler(handle, np.array(y1, order="F"), th1, preset="fast", seed=3)
    s.init()
    s.ppc_enable()
    with pytest.raises(_lib.GpirtError, match="m = 1 is outside 2..4096"):
        s.ppc_resid_enable()
    s.close()

    ys, ths = make_responses(64, 8, seed=4)

    def factory(yl, th, pm, ps, st, item0, m_total):
        return Sampler(handle, yl, th, pm, ps, st, rng="item", seed=77, item0=item0, m_total=m_total)

    sh = ShardedSampler(factory, ys, ths, dist=None)
    with pytest.raises(ValueError, match="residual"):
        sh.ppc_resid_enable()
    sh.engine.close()
