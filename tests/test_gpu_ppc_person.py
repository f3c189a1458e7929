"""The person fit of the PPC on the device (csrc/ppc_person.hip) against NumPy: the constants and every draw's integer tables
against gpirt_amd.ppc.person_from_draws, the three lz sums against long double within a bound derived from the inputs
(tests/_person_bounds.py), every statistic and accumulator bit for bit from the device's own tables, device against device (the
PPC's respondent counts), constructed states, the untouched chain and blocks, repeatability, pooling and the refusals.  The shapes
cross a wave (64 rows), the strip kernel's 256-row work-group, a 32-position strip, a strip cut short by a group boundary and the
finishing kernel's 128-row work-group; 2 to 16 item groups."""
import numpy as np
import pytest

from _person_bounds import lz_bounds
from gpirt_amd import _lib

pytestmark = pytest.mark.gpu
SHAPES = [(33, 2), (65, 31), (257, 33), (1000, 65), (4097, 96)]
LAST = tuple(r[0] for r in _lib.PERSON_LAST)
CONST = tuple(r[0] for r in _lib.PERSON_CONST)
FIELDS = _lib.PERSON_RESP_FIELDS + _lib.PERSON_CELL_FIELDS
_RUNS = {}


def _responses(n, m, seed):
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=seed, na_frac=0.03)
    y = np.array(y, order="F")
    if m > 2:
        y[:, m // 3] = np.nan
    y[n // 2, :] = np.nan
    return y, th0


def _run(handle, n, m, K, perm=False, steps=3):
    key = (n, m, K, perm)
    if key in _RUNS:
        return _RUNS[key]
    from gpirt_amd import Sampler
    from gpirt_amd import ppc as P
    y, th0 = _responses(n, m, seed=400 + n)
    cuts = P.default_item_cuts(m, min(K, m))             # K is cut down to m where m - 1 cuts do not exist
    order = np.random.default_rng(77).permutation(m).astype(np.int32) if perm else None
    seed = 2**33 + 7
    s = Sampler(handle, y, th0, preset="fast", seed=seed)
    s.init()
    s.ppc_enable()
    s.ppc_person_enable(order, cuts, top=5)
    const = {k: s.ppc_person_get(k) for k in CONST + ("order", "cuts", "group_lo", "group_hi", "group_items")}
    g, its, tabs, ppc_first = [], [], [], None
    for d in range(steps):
        s.step()
        s.ppc_accumulate()
        g.append(s.get("f") + s.get("mu"))
        its.append(s.iteration)
        tabs.append({k: s.ppc_person_get(k) for k in LAST})
        if d == 0:
            ppc_first = {k: s.ppc_get(k) for k in ("respondent_rep_yes_sum", "respondent_obs_yes", "respondent_n_obs")}
    s.check()
    names = tuple(r[0] for r in _lib.PERSON_RAW) + FIELDS
    out = dict(y=y, cuts=cuts, order=P.default_item_order(y) if order is None else order, seed=seed, g=np.stack(g), its=its,
               tabs=tabs, const=const, ppc_first=ppc_first, res=s.ppc_person(), raw={k: s.ppc_person_get(k) for k in names + ("counts",)})
    s.close()
    _RUNS[key] = out
    return out


CASES = [(n, m, K, False) for n, m in SHAPES for K in (2, 5, 16)] + [(257, 33, 5, True)]


@pytest.mark.parametrize("n,m,K,perm", CASES)
def test_tables_and_statistics_against_numpy(handle, n, m, K, perm):
    from gpirt_amd import ppc as P
    r = _run(handle, n, m, K, perm)
    cuts, order, const, y = r["cuts"], r["order"], r["const"], r["y"]
    Kk = len(cuts) + 1
    assert Kk == min(K, m)
    # the constants, counted on the device at enable, against the data: bit for bit
    want_obs = P.person_observed(y, order, cuts)
    for k, w in (("x_obs", "x"), ("g_obs", "g"), ("q_obs", "q"), ("tN", "tN"), ("tT", "tT")):
        assert np.array_equal(const[k], want_obs[w]), k
    assert np.array_equal(const["order"], order) and np.array_equal(const["group_items"], order) and tuple(const["cuts"]) == cuts
    assert const["group_lo"][0] == 0 and const["group_hi"][-1] == m - 1 and const["order"].dtype == np.int32
    obs = P.person_observed_from_arrays(const["order"], const["cuts"], const["x_obs"], const["g_obs"], const["q_obs"], const["tN"],
                                        const["tT"])
    N = const["tN"].astype(np.int64)
    worst_fix = worst_lz = 0.0
    draws = []
    for d, tab in enumerate(r["tabs"]):
        ref, gap = P.person_from_draws(y, r["g"][d:d + 1], r["seed"], r["its"][d:d + 1], order, cuts)
        assert gap > 1e-9                                # a condition on the inputs: no cell near its uniform
        last = ref["last"]
        assert ref["person_draws"] == 1
        for k in ("xr", "gr", "qr", "tR"):
            assert np.array_equal(tab[k], last[k]), (k, d)
            assert tab[k].dtype == last[k].dtype, k
        # device exp within 1 ulp: a term's rint can differ by one unit of 2^-44, so a cell's sum by at most tN units
        for k in ("tE", "tV"):
            diff = np.abs(tab[k] - last[k])
            worst_fix = max(worst_fix, float((diff / np.maximum(N, 1)).max()))
            assert (diff <= N).all(), (k, d)
        # the three lz sums against long double, within the bound of the case's own inputs
        rep = _rep_of(y, r["g"][d], r["seed"], r["its"][d])
        one = P.person_tables(y, r["g"][d], rep, want_obs)
        bound = lz_bounds(y, r["g"][d], rep, order)
        err = np.abs(tab["lz"].astype(np.longdouble) - one["lz"])
        assert (err <= bound).all(), (d, float((err - bound).max()))
        if (bound > 0).any():
            worst_lz = max(worst_lz, float((err[bound > 0] / bound[bound > 0]).max()))
        # the device's own tables through the NumPy statement: every double bit for bit
        own = dict(obs=obs, xr=tab["xr"], gr=tab["gr"], qr=tab["qr"], tR=tab["tR"], tE=tab["tE"], tV=tab["tV"], lz=tab["lz"])
        st = P.person_draw_stats(own)
        assert np.array_equal(tab["chi"], st["chi"]), d
        draws.append(own)
    print(f"{n} x {m}, K = {Kk}: largest |tE, tV difference| / tN = {worst_fix:.3f} units of 2^-44 (bound 1); "
          f"largest lz sum error / bound = {worst_lz:.4f}")
    want = P.person_from_tables(draws, top=5)
    got = r["res"]
    for name, _dt, _kind in _lib.PERSON_RAW:
        assert np.array_equal(got[name], want[name], equal_nan=True), name
        assert got[name].dtype == want[name].dtype, name
        assert np.array_equal(r["raw"][name], got[name], equal_nan=True), name            # ... and by name
    for name in FIELDS:
        assert np.array_equal(got[name], want[name], equal_nan=True), name
        assert np.array_equal(r["raw"][name], got[name], equal_nan=True), name
    for k in ("respondents", "ppp_guttman_mid"):
        assert np.array_equal(got["worst"][k], want["worst"][k], equal_nan=True), k
    for k in ("cuts", "group_lo", "group_hi", "group_items"):
        assert np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype, k
    assert list(r["raw"]["counts"]) == [3, 0] and (got["person_draws"], got["person_skipped"], got["K"]) == (3, 0, Kk)
    live = (~np.isnan(y)).any(axis=1)
    assert got["n_scored"] == want["n_scored"] == int(live.sum()) and (got["n"], got["m"]) == (n, m)
    # the respondent without an observed cell: NaN on the way out, nothing moved
    dead = n // 2
    assert not live[dead] and all(np.isnan(got[f][dead]) for f in _lib.PERSON_RESP_FIELDS) and np.isnan(got["obs_rate"][:, dead]).all()
    assert got["g_undefined_count"][dead] == 0 and got["lz_undefined_count"][dead] == 0 and got["chi_ge"][dead] == 0
    # device against device, after the first counted draw: the PPC's own counts
    first, pf = r["tabs"][0], r["ppc_first"]
    assert np.array_equal(first["tR"].sum(axis=0), pf["respondent_rep_yes_sum"].astype(np.int64))
    assert np.array_equal(first["xr"], pf["respondent_rep_yes_sum"].astype(np.int64))
    assert np.array_equal(const["tT"].sum(axis=0), pf["respondent_obs_yes"].astype(np.int64))
    assert np.array_equal(const["tN"].sum(axis=0), pf["respondent_n_obs"].astype(np.int64))


def _rep_of(y, g, seed, it):
    """the replicate of one draw, as person_from_draws forms it"""
    from gpirt_amd import ppc as P
    n, m = y.shape
    ob = ~np.isnan(y)
    p, _ = P._plogis(np.where(ob, g, 0.0))
    return ob & (P.replicate_uniforms(seed, int(it), n, m) < p)


def _words(s):
    return s.ppc_person_state().cpu().numpy().copy()


def test_constructed_states(handle):
    from gpirt_amd import Sampler
    from gpirt_amd import ppc as P
    n, m, seed, cuts = 300, 40, 11, (8, 16, 24, 32)
    rng = np.random.default_rng(3)
    y = np.where(rng.random((n, m)) < 0.5, 1.0, -1.0)
    y[rng.random((n, m)) < 0.05] = np.nan
    y[260, 33] = 1.0
    y[261, 34] = np.nan
    y[17] = np.nan
    order = rng.permutation(m).astype(np.int32)
    pos = np.argsort(order)                              # the position of every item
    s = Sampler(handle, y, np.zeros(n), rng="item", seed=seed, theta_stabilise=True)
    s.init()
    s.ppc_enable()
    s.ppc_person_enable(order, cuts)
    mu = s.get("mu")
    obs = ~np.isnan(y)
    live = obs.any(axis=1)
    N = obs.sum(axis=1)
    c = s.ppc_person_get

    def draw(it, g):
        s.set_iteration(it)
        s.set("f", g - mu)
        s.ppc_accumulate()
        return np.asarray(s.get("f") + mu)

    # |g| = 40: the replicate is deterministic (p is 1 or 4e-18 against a uniform of 53 bits).  Yes on the positions below a
    # threshold of the respondent's own, no from there on: a perfect Guttman pattern under the order, G_rep = 0
    thr = 5 + (np.arange(n) % 30)
    easy = pos[None, :] < thr[:, None]
    gd = draw(12, np.where(easy, 40.0, -40.0))
    assert (np.abs(gd) > 39.0).all()
    X = (obs & easy).sum(axis=1)
    Q = X * (N - X)
    assert np.array_equal(c("xr"), X) and not c("gr").any() and np.array_equal(c("qr"), Q) and (Q[live] > 0).all()
    Go, Qo = c("g_obs"), c("q_obs")
    assert (Qo[live] > 0).all() and (Go[live] > 0).all()                 # random answers: everybody has errors
    assert not c("g_ge").any() and not c("g_gt").any() and not c("g_undefined_count").any() and not c("gn_rep_sum").any()
    want, gap = P.person_from_draws(y, gd[None], seed, [12], order, cuts)
    assert gap > 1e-9
    r = s.ppc_person()
    for k in ("g_ge", "g_gt", "g_undefined_count", "g_rep_sum", "gn_rep_sum", "sum_r", "cell_ge", "cell_gt", "chi_ge", "lz_undefined_count"):
        assert np.array_equal(r[k], want[k]), k
    assert (r["ppp_guttman"][live] == 0.0).all() and np.isnan(r["ppp_guttman"][17])
    # the reversed pattern: no below the threshold, yes from there on: G_rep = Q_rep exactly, the largest the score allows
    s.ppc_person_enable(order, cuts)
    draw(13, np.where(easy, -40.0, 40.0))
    Xr = (obs & ~easy).sum(axis=1)
    Qr = Xr * (N - Xr)
    assert np.array_equal(c("xr"), Xr) and np.array_equal(c("gr"), Qr) and np.array_equal(c("qr"), Qr)
    assert np.array_equal(c("g_ge"), live.astype(np.uint32)) and np.array_equal(c("g_gt"), (live & (Go < Qo)).astype(np.uint32))
    assert np.array_equal(c("gn_rep_sum"), live.astype(np.float64)) and np.array_equal(c("g_rep_sum"), Qr.astype(np.uint64))
    assert np.array_equal(c("guttman_norm_rep_mean")[live], np.ones(int(live.sum()))) and list(c("counts")) == [1, 0]
    # an all-equal p: lz is well defined, and the three sums are within the bound of the inputs
    s.ppc_person_enable(order, cuts)
    gd = draw(14, np.full((n, m), 0.75))
    assert (np.abs(gd - 0.75) < 1e-12).all()
    rep = _rep_of(y, gd, seed, 14)
    err = np.abs(c("lz").astype(np.longdouble) - P.person_tables(y, gd, rep, P.person_observed(y, order, cuts))["lz"])
    assert (err <= lz_bounds(y, gd, rep, order)).all() and (c("lz")[2][live] > 0).all()
    assert not c("lz_undefined_count").any() and np.isfinite(c("lz_obs_sum")).all() and c("lz_rep_sumsq")[live].min() >= 0.0
    # g = 0 everywhere: Vl = 0, so the draw counts in lz_undefined_count and in nothing else of lz
    sums = {k: c(k) for k in ("lz_obs_sum", "lz_rep_sum", "lz_rep_sumsq")}
    gd = draw(15, np.zeros((n, m)))
    assert not gd.any()
    assert np.array_equal(c("lz_undefined_count"), live.astype(np.uint32)) and list(c("counts")) == [2, 0]
    for k, v in sums.items():
        assert np.array_equal(c(k), v), k
    assert np.array_equal(c("lz_undefined")[live], np.ones(int(live.sum()))) and not c("lz")[2].any()
    # skipped: +-inf and NaN g in an observed cell -- only the counter moves
    g0 = np.where(obs, 1.5 * rng.standard_normal((n, m)), 0.0)
    draw(16, g0)
    before, tabs = _words(s), {k: c(k) for k in LAST}
    at = (np.arange(n)[:, None] == 260) & (np.arange(m)[None, :] == 33)
    for q, bad in enumerate((np.inf, -np.inf, np.nan)):
        draw(17 + q, np.where(at, bad, g0))
        after = _words(s)
        assert list(np.flatnonzero(after != before)) == [6] and after[6] == before[6] + 1
        before = after
    for k in LAST:                                       # still the last COUNTED draw's
        assert np.array_equal(c(k), tabs[k], equal_nan=True), k
    # NaN and inf in missing cells (a whole missing row too): the draw counts, and nothing of it differs
    g2 = g0.copy()
    g2[261, 34] = np.nan
    g2[17] = np.inf
    draw(16, g2)
    assert list(c("counts")) == [4, 3]
    for k in LAST:
        assert np.array_equal(c(k), tabs[k], equal_nan=True), k
    s.close()


def test_state_block_repeatable_and_others_untouched(handle):
    from gpirt_amd import Sampler
    from gpirt_amd import ppc as P
    n, m, cuts = 257, 33, (14, 43, 76, 122)
    y, th0 = _responses(n, m, seed=55)
    groups = np.arange(n) % 3
    blocks = {k: [] for k in ("ppc", "pairs", "bins", "dif", "scores", "person", "chain")}
    for person in (True, True, False):
        s = Sampler(handle, y, th0, preset="fast", seed=21)
        s.init()
        s.ppc_enable()
        s.ppc_pairs_enable()
        s.ppc_bins_enable(cuts)
        s.ppc_dif_enable(groups, cuts)
        s.ppc_scores_enable()
        if person:
            s.ppc_person_enable()                        # the default order and cuts
        for _ in range(3):
            s.step()
            s.ppc_accumulate()
        blocks["ppc"].append(s.ppc_state().cpu().numpy().copy())
        blocks["pairs"].append(s.ppc_pairs_state().cpu().numpy().copy())
        blocks["bins"].append(s.ppc_bins_state().cpu().numpy().copy())
        blocks["dif"].append(s.ppc_dif_state().cpu().numpy().copy())
        blocks["scores"].append(s.ppc_scores_state().cpu().numpy().copy())
        if person:
            st = s.ppc_person_state()
            hdr = P.person_state_header(st)
            want = P.default_item_cuts(m)
            assert hdr == dict(tag=0x31535250, version=1, n=n, m=m, K=5, person_draws=3, person_skipped=0, cuts=want)
            assert want == (6, 13, 19, 26)
            assert np.array_equal(s.ppc_person_get("order"), P.default_item_order(y))
            blocks["person"].append(st.cpu().numpy().copy())
        blocks["chain"].append(np.concatenate([s.get("f").ravel(), s.get("theta"), s.get("beta").ravel(), s.get("fstar").ravel(),
                                               [float(s.iteration)]]))
        s.close()
    for k in ("ppc", "pairs", "bins", "dif", "scores", "chain"):
        assert blocks[k][0].tobytes() == blocks[k][2].tobytes() and blocks[k][0].tobytes() == blocks[k][1].tobytes(), k
    assert blocks["person"][0].tobytes() == blocks["person"][1].tobytes() and blocks["person"][0][24:].any()


def test_chains_pool(handle):
    from gpirt_amd import Sampler
    from gpirt_amd import ppc as P
    from gpirt_amd.synthetic import make_responses
    n, m, cuts, seed = 300, 40, (8, 16, 24), 29
    y, th0 = make_responses(n, m, seed=11)
    order = P.default_item_order(y)
    samplers, tables = [], []
    for c, draws in enumerate((3, 2)):
        s = Sampler(handle, y, th0 if c == 0 else -th0, rng="item", seed=seed, theta_stabilise=True)
        s.init()
        s.ppc_enable()
        s.ppc_person_enable(order, cuts, top=6)
        for _ in range(draws):
            s.step()
            s.ppc_accumulate()
            tables.append({k: s.ppc_person_get(k) for k in LAST})
        samplers.append(s)
    own = [s.ppc_person() for s in samplers]
    pooled = P.person_combine(handle, samplers, top=6)
    obs = P.person_observed(y, order, cuts)
    both = P.person_from_tables([dict(obs=obs, xr=t["xr"], gr=t["gr"], qr=t["qr"], tR=t["tR"], tE=t["tE"], tV=t["tV"], lz=t["lz"])
                                 for t in tables], top=6)
    eps = float(np.finfo(np.float64).eps)
    for name, dt, kind in _lib.PERSON_RAW:
        const = (name, dt, kind) in _lib.PERSON_CONST
        want = own[0][name] if const else own[0][name] + own[1][name]                       # the doubles in chain order
        assert np.array_equal(pooled[name], want, equal_nan=True), name
        if dt != "f8" or const:
            assert np.array_equal(pooled[name], both[name]), name
        else:
            # the same five terms, ((a + b) + c) + (d + e) against (((a + b) + c) + d) + e: four roundings each, every partial sum
            # at most sum |term|, which is at most |own 0| + |own 1| + 4 eps of it for terms of one sign and is bounded by
            # sum |lz| <= 5 max |lz| for the two lz sums, whose terms change sign
            size = np.abs(own[0][name]) + np.abs(own[1][name])
            if name in ("lz_obs_sum", "lz_rep_sum"):
                size = 5.0 * np.max([np.abs(P.person_draw_stats(dict(obs=obs, **t))["lz_obs" if name == "lz_obs_sum" else "lz_rep"])
                                     for t in tables], axis=0)
            assert (np.abs(pooled[name] - both[name]) <= 8.0 * eps * size).all(), name
    assert pooled["person_draws"] == 5 == both["person_draws"] and pooled["worst"]["respondents"].shape == (6,)
    for k in ("ppp_guttman", "ppp_guttman_mid", "ppp_chi2", "ppp_cell", "obs_rate", "guttman_obs", "guttman_norm_obs", "guttman_rep_mean"):
        assert np.array_equal(pooled[k], both[k], equal_nan=True), k
    for k in ("respondents", "ppp_guttman_mid"):
        assert np.array_equal(pooled["worst"][k], both["worst"][k], equal_nan=True), k
    # refusals of the combine: another order, other cuts, another m, another response matrix, a block of another kind
    y2, th2 = make_responses(n, m - 1, seed=12)
    y3 = y.copy()
    y3[5, 7] = -y3[5, 7]
    swapped = order.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    others = []
    for yy, tt, oo, cc in ((y, th0, swapped, cuts), (y, th0, order, (8, 16, 25)), (y, th0, order, (8, 16)), (y2, th2, None, cuts),
                           (y3, th0, order, cuts)):
        o = Sampler(handle, yy, tt, rng="item", seed=3, theta_stabilise=True)
        o.init()
        o.ppc_enable()
        o.ppc_person_enable(oo, cc)
        others.append(o)
    for o in others:
        with pytest.raises(_lib.GpirtError, match="another n, m, K, order, cuts or response matrix"):
            P.person_combine(handle, [samplers[0], o])
    with pytest.raises(_lib.GpirtError):
        P.person_combine(handle, [samplers[0].ppc_person_state(), samplers[0].ppc_state()])
    with pytest.raises(ValueError):
        P.person_combine(handle, [samplers[0].ppc_state()])
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
        s.ppc_person_enable(cuts=(5, 10))                    # needs ppc_enable
    s.ppc_enable()
    ident = tuple(range(31))

    def raw(K, order, cuts):
        return s.lib.gpirt_sampler_ppc_person_enable(s._s, K, (C.c_int32 * len(order))(*order) if order else None,
                                                     (C.c_int * len(cuts))(*cuts) if cuts else None, 1)

    rep = ident[:7] + (3,) + ident[8:]
    far = ident[:4] + (31,) + ident[5:]
    for K, order, cuts, word in ((1, ident, (5,), "1 item groups"), (17, ident, tuple(range(1, 17)), "17 item groups"),
                                 (3, ident, (10, 5), "increasing"), (3, ident, (5, 5), "increasing"), (3, ident, (5, 31), "in 1..30"),
                                 (3, ident, (0, 5), "in 1..30"), (3, ident, None, "item groups"), (3, None, (5, 10), "no item order"),
                                 (3, rep, (5, 10), "entry 7 is 3: a repeat"), (3, far, (5, 10), "entry 4 is 31: out of range")):
        assert raw(K, order, cuts) == _lib.E_ARG and word in _lib.last_error(), (K, cuts, _lib.last_error())
    with pytest.raises(_lib.GpirtError):
        s.ppc_person_get("counts")                           # nothing was enabled by the refused calls
    for bad_o, bad_c, word in ((rep, (5,), "entry 7 is 3"), (ident[:30], (5,), "must hold 31 integers"), (ident, (10, 5), "increasing"),
                               (ident, (), "1 item groups")):
        with pytest.raises(ValueError, match=word):
            s.ppc_person_enable(bad_o, bad_c)
    with pytest.raises(ValueError, match="top must be"):
        s.ppc_person_enable(top=65)
    s.ppc_person_enable(cuts=(1, 30))
    s.step()
    s.ppc_accumulate()
    assert list(s.ppc_person_get("counts")) == [1, 0] and s.ppc_person_get("sum_r").shape == (3, 65)
    with pytest.raises(ValueError, match="unknown field"):
        s.ppc_person_get("no_such_field")
    assert s.lib.gpirt_sampler_ppc_person_get(s._s, b"no_such_field", C.c_void_p(y.ctypes.data), 8) == _lib.E_ARG
    assert "unknown person-fit field" in _lib.last_error()
    with pytest.raises(ValueError):
        s.ppc_person(top=65)
    s.ppc_enable()                                           # frees the block too
    with pytest.raises(_lib.GpirtError):
        s.ppc_person_get("counts")
    s.ppc_person_enable()
    s.ppc_person_enable(on=False)
    with pytest.raises(_lib.GpirtError):
        s.ppc_person()
    s.ppc_accumulate()                                       # the PPC itself goes on
    s.close()

    ys, ths = make_responses(64, 8, seed=4)

    def factory(yl, th, pm, ps, st, item0, m_total):
        return Sampler(handle, yl, th, pm, ps, st, rng="item", seed=77, item0=item0, m_total=m_total)

    sh = ShardedSampler(factory, ys, ths, dist=None)
    with pytest.raises(ValueError, match="person fit"):
        sh.ppc_person_enable()
    # ... and by the library itself on a sampler that holds a shard of the items
    part = Sampler(handle, ys[:, :4], ths, rng="item", seed=77, item0=4, m_total=8)
    part.init()
    part.ppc_enable()
    with pytest.raises(_lib.GpirtError, match="item shards"):
        part.ppc_person_enable(cuts=(2,))
    part.close()
    sh.engine.close()
