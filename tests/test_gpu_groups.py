"""The group posteriors on the device (include/gpirt_hip.h "group posteriors", csrc/groups.hip) against gpirt_amd.groups, the NumPy
statement.  Part A of every draw is held bit for bit to latent_tables / latent_draw_stats of the device's own theta; e to
votes_tables within n_g units (DESIGN.md section 22's bound: one unit per term where another exp within 1 ulp moves p 2^44
across a half-integer); everything after e bit for bit to votes_draw_stats of the device's own e; loy to loyalty_tables within
c_g units given the device's own sides, obs_with and obs_n exactly; every accumulator bit for bit to from_tables of the
per-draw tables collected step by step."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(33, 2), (65, 31), (257, 33), (1000, 65), (4097, 96)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def make_codes(n, G, seed):
    rng = np.random.default_rng(seed)
    codes = rng.integers(-1, G, n).astype(np.int32)
    codes[:G] = np.arange(G)
    return codes


def udiff(a, b):
    """|a - b| of two uint64 arrays as int64"""
    return np.abs(a.astype(np.int64) - b.astype(np.int64))


def check_draw(s, y, codes, G, latent=True, votes=True):
    """The last accumulate's tables against the statement evaluated on the device's own state; returns the draw's tables for
    from_tables (a part that was to be skipped: None, nothing of it is read)."""
    from gpirt_amd import groups as GR
    sizes = GR.group_sizes(codes, G)
    out = dict(latent=None, votes=None)
    if latent:
        theta = s.get("theta")
        want = GR.latent_tables(theta, codes, G)
        assert want is not None
        dev = {k: s.groups_get(k) for k in ("hist", "c1", "c2", "med2", "w", "ov")}
        for k, v in dev.items():
            assert same_bits(v, want[k]), k
        dev["k"] = want["k"]
        st = GR.latent_draw_stats(dev, codes, G)
        assert same_bits(s.groups_get("latent_stats"), st["latent_stats"])
        dev.update(st)
        out["latent"] = dev
    if votes:
        g = s.get("f") + s.get("mu")
        e = s.groups_get("e")
        want = GR.votes_tables(g, codes, G)
        assert want is not None
        assert (udiff(e, want) <= sizes[:G, None]).all(), int(udiff(e, want).max())
        st = GR.votes_draw_stats(e, sizes)
        assert same_bits(s.groups_get("side"), st["side"])
        assert same_bits(s.groups_get("split"), st["split"].astype(np.uint8))
        assert same_bits(s.groups_get("contested"), st["contested"].astype(np.uint8))
        assert same_bits(s.groups_get("n_split"), st["n_split"]) and same_bits(s.groups_get("c_g"), st["c_g"])
        lo = GR.loyalty_tables(g, y, codes, st["side"], st["contested"])
        loy = s.groups_get("loy")
        bound = np.where(codes >= 0, st["c_g"][np.maximum(codes, 0)], 0)
        assert (udiff(loy, lo["loy"]) <= bound).all()
        assert same_bits(s.groups_get("obs_with"), lo["obs_with"]) and same_bits(s.groups_get("obs_n"), lo["obs_n"])
        vo = dict(e=e, loy=loy, obs_with=lo["obs_with"], obs_n=lo["obs_n"])
        vo.update(st)
        out["votes"] = vo
    return out


def check_state(s, draws, codes, G, m, top=7):
    """every accumulator bit for bit from_tables of the collected tables; the library's lists against finish's"""
    from gpirt_amd import _lib
    from gpirt_amd import groups as GR
    raw = GR.from_tables(draws, codes, G, m)
    for name, _, _ in _lib.GROUPS_RAW:
        assert same_bits(s.groups_get(name), raw[name]), name
    assert s.groups_get("counts").tolist() == [raw[c] for c in GR.COUNTERS]
    assert s.groups_get("group_size")[:G + 1].tolist() == GR.group_sizes(codes, G).tolist()
    assert same_bits(s.groups_get("groups"), codes.astype(np.int8))
    got, want = s.groups(top=top), GR.finish(raw, codes, G, top)
    for p in range(len(GR.pairs(G))):
        assert same_bits(got["most_split"][p]["items"], want["most_split"][p]["items"]), p
        assert same_bits(got["most_split"][p]["p_split"], want["most_split"][p]["p_split"]), p
    assert same_bits(got["least_loyal"]["respondents"], want["least_loyal"]["respondents"])
    assert same_bits(got["least_loyal"]["loyalty"], want["least_loyal"]["loyalty"])
    for k in ("mean", "p_superior", "overlap", "p_group_median", "support", "gap", "p_split", "loyalty", "obs_loyalty", "median_quantiles"):
        assert same_bits(got[k], want[k]), k
    return raw, got


@pytest.mark.parametrize("G", [2, 3, 8])
@pytest.mark.parametrize("n,m", SHAPES)
def test_real_draws(handle, n, m, G):
    from gpirt_amd import Sampler
    from gpirt_amd import groups as GR
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=300 + n)
    codes = make_codes(n, G, n + G)
    s = Sampler(handle, y, th0, preset="fast", seed=9)
    s.init()
    s.groups_enable(codes, top=7)
    draws = []
    for _ in range(3):
        s.step()
        s.groups_accumulate()
        draws.append(check_draw(s, y, codes, G))
    raw, got = check_state(s, draws, codes, G, m)
    hdr = GR.state_header(s.groups_state())
    assert (hdr["tag"], hdr["version"], hdr["n"], hdr["m"], hdr["G"]) == (0x31505247, 1, n, m, G)
    assert (hdr["latent_draws"], hdr["votes_draws"], hdr["latent_skipped"], hdr["votes_skipped"]) == (3, 3, 0, 0)
    for g in range(G):
        assert abs(got["p_group_median"][codes == g].sum() - 1.0) < 1e-12
    s.close()


# n at 255 / 256 / 257 and at the row tile's edge (1024 rows a work-group), m at the strip widths (8 and 32) and one beyond
@pytest.mark.parametrize("n,m", [(255, 8), (256, 9), (257, 32), (1024, 33), (1025, 7)])
def test_constructed_states(handle, n, m):
    from gpirt_amd import Sampler
    from gpirt_amd import groups as GR
    G = 3
    rng = np.random.default_rng(n + m)
    codes = make_codes(n, G, 5)
    y = np.where(rng.random((n, m)) < 0.2, np.nan, np.where(rng.random((n, m)) < 0.5, 1.0, -1.0))
    inc = np.nonzero(codes >= 0)[0]
    left = codes < 0
    sizes = GR.group_sizes(codes, G)
    s = Sampler(handle, y, np.zeros(n), rng="item", seed=5, theta_stabilise=True)
    s.init()
    s.groups_enable(codes, top=7)
    s.set("mu", np.zeros((n, m)))
    grid = lambda k: -5.0 + np.asarray(k, dtype=np.float64) * 0.01                       # noqa: E731
    draws = []

    def enter(theta, f, **kw):
        theta, f = theta.copy(), f.copy()
        theta[left] = np.nan                          # a left-out respondent holds anything
        f[left] = np.nan
        s.set("theta", theta)
        s.set("f", f)
        s.groups_accumulate()
        draws.append(check_draw(s, y, codes, G, **kw))
        return draws[-1]

    base = rng.normal(0.0, 2.0, (n, m)) + np.where(codes[:, None] == 1, 1.5, -1.5) * np.sign(rng.normal(size=m))
    # all respondents on one grid point
    d = enter(grid(np.full(n, 437)), base)
    assert not d["latent"]["w"].any() and d["latent"]["ov"].tolist() == [sizes[g] * sizes[h] for g, h in GR.pairs(G)]
    assert same_bits(d["latent"]["share"][inc], 1.0 / sizes[codes[inc]].astype(np.float64))
    assert np.isnan(d["latent"]["d"]).all()
    # thetas at k = 0 and k = 1000
    d = enter(grid(np.where(np.arange(n) % 2 == 0, 0, 1000)), base)
    assert d["latent"]["hist"][G, 0] + d["latent"]["hist"][G, 1000] == sizes[G]
    # a spread of thetas; +-inf and the exact tie g = 0
    f = base.copy()
    f[inc[0], 0], f[inc[1], 0], f[inc[2], m - 1] = np.inf, -np.inf, np.inf
    f[:, m // 2] = 0.0
    d = enter(grid(rng.integers(0, 1001, n)), f)
    assert not d["votes"]["side"][:, m // 2].any() and not d["votes"]["rice"][:, m // 2].any()
    assert (d["votes"]["e"][:, m // 2] == sizes[:G].astype(np.uint64) << np.uint64(43)).all()
    # a NaN theta: part A skipped, part B counted; then a NaN g: the reverse; then a theta off the grid
    th_ = grid(rng.integers(300, 700, n))
    th_[inc[-1]] = np.nan
    enter(th_, base, latent=False)
    f = base.copy()
    f[inc[-1], m - 1] = np.nan
    enter(grid(rng.integers(300, 700, n)), f, votes=False)
    th_ = grid(rng.integers(300, 700, n))
    th_[inc[0]] = 0.005
    enter(th_, base, latent=False)
    raw, _ = check_state(s, draws, codes, G, m)
    assert [raw[c] for c in GR.COUNTERS] == [4, 2, 5, 1]
    s.close()


def run_chain(handle, y, th0, codes, on, case, keep=False):
    from gpirt_amd import Sampler
    from gpirt_amd.ops import RStream
    rs = RStream(77) if case == "reference" else None
    kw = dict(preset="fast", seed=21) if case == "fast" else dict(rng="reference", rstream=rs, theta_stabilise=False)
    s = Sampler(handle, y, th0, **kw)
    s.init()
    s.ppc_enable()
    s.rank_enable()
    s.acf_enable("all", 8, 3)
    if on:
        s.groups_enable(codes)
    kept = dict(theta=[], g=[])
    for _ in range(3):
        s.step()
        s.accumulate_irf()
        s.ppc_accumulate()
        s.rank_accumulate()
        s.acf_accumulate()
        if on:
            s.groups_accumulate()
        if keep:
            kept["theta"].append(s.get("theta"))
            kept["g"].append(s.get("f") + s.get("mu"))
    s.check()
    end = dict(chain=np.concatenate([s.get("f").ravel(), s.get("theta"), s.get("beta").ravel(), s.get("fstar").ravel(),
                                     s.get("irf_sum").ravel(), [float(s.iteration)]]).tobytes(),
               ppc=s.ppc_state().cpu().numpy().tobytes(), rank=s.rank_state().cpu().numpy().tobytes(),
               acf=s.acf_state().cpu().numpy().tobytes())
    if rs is not None:
        mt, idx = rs.state()
        end["rs"] = np.concatenate([np.asarray(mt, dtype=np.int64).ravel(), [int(idx)]]).tobytes()
    if on:
        end["groups"] = s.groups_state().cpu().numpy().tobytes()
    return s, end, {k: np.stack(v) for k, v in kept.items() if v}


@pytest.mark.parametrize("case", ["fast", "reference"])
def test_others_untouched_and_repeatable(handle, case):
    """the chain, the IRF sum, R's stream position and the PPC, rank and acf state blocks byte-identical with the block on and
    off; two runs with the block on give a byte-identical group state"""
    from gpirt_amd.synthetic import make_responses
    n, m = 65, 31
    y, th0 = make_responses(n, m, seed=55)
    codes = make_codes(n, 3, 1)
    ends = []
    for on in (True, True, False):
        s, end, _ = run_chain(handle, y, th0, codes, on, case)
        s.close()
        ends.append(end)
    assert ends[0]["groups"] == ends[1]["groups"] and any(ends[0]["groups"][2048:])
    for k in ends[2]:
        assert ends[0][k] == ends[2][k] and ends[1][k] == ends[2][k], k
    assert (case == "reference") == ("rs" in ends[2])


def test_three_chains_pooled_with_a_forced_reflection(handle):
    from gpirt_amd import _lib
    from gpirt_amd import groups as GR
    from gpirt_amd.synthetic import make_responses
    n, m, G = 65, 31, 3
    y, _ = make_responses(n, m, seed=55)
    codes = make_codes(n, G, 2)
    inits = np.random.default_rng(4).normal(size=(3, n))
    samplers, kept = [], []
    for c in range(3):
        from gpirt_amd import Sampler
        s = Sampler(handle, y, inits[c], preset="fast", seed=_lib.chain_seed(17, c))
        s.init()
        s.groups_enable(codes)
        th, gg = [], []
        for _ in range(3):
            s.step()
            s.groups_accumulate()
            th.append(s.get("theta"))
            gg.append(s.get("f") + s.get("mu"))
        samplers.append(s)
        kept.append((np.stack(th), np.stack(gg)))
    signs = (1, -1, 1)
    got = GR.combine(handle, samplers, signs=signs, top=9)
    plain = GR.combine(handle, samplers, top=9)
    want = GR.from_draws(np.stack([k[0] for k in kept]), np.stack([k[1] for k in kept]), y, codes, signs=signs, top=9)
    assert got["chains"] == 3 and got["latent_draws"] == 9 and got["votes_draws"] == 9
    for name, dt, _ in _lib.GROUPS_RAW:
        if name in GR.LATENT_RAW or dt != "f8":
            assert same_bits(got["raw"][name], want["raw"][name]), name                 # part A does not depend on exp
        else:
            # part B's fp64 sums go through e, which NumPy's exp forms within n_g units: support moves by at most 2^-44, rice
            # and gap by 2^-43, their squares (values in [-1, 1]) by 2^-42, loyalty (c_g units over c_g 2^44) by 2^-44; nine
            # draws add nine such terms, and a factor of two covers the roundings of the sums themselves
            assert np.allclose(got["raw"][name], want["raw"][name], rtol=0, atol=9 * 2.0 ** -41), name
    for k in ("mean", "mean_sd", "sd_mean", "median_quantiles", "density", "density_sd", "p_superior", "overlap", "p_mean_gt",
              "p_median_gt", "d_mean", "d_sd", "p_group_median"):
        assert same_bits(got[k], want[k]), k
    assert not np.array_equal(plain["mean"], got["mean"]) and same_bits(plain["raw"]["support_sum"], got["raw"]["support_sum"])
    # one chain alone with sign -1 is the chain reflected
    one = samplers[1].groups(sign=-1)
    assert same_bits(one["raw"]["dens_sum"], samplers[1].groups_get("dens_sum")[:, ::-1])
    assert same_bits(one["raw"]["mean_sum"], -samplers[1].groups_get("mean_sum"))
    for s in samplers:
        s.close()


def test_run_is_the_stage_api_in_one_call(handle):
    from gpirt_amd import Sampler, _lib, chains
    from gpirt_amd import groups as GR
    from gpirt_amd.synthetic import make_responses
    n, m = 96, 6
    y, _ = make_responses(n, m, seed=8)
    codes = make_codes(n, 2, 3)
    S, Bn, seed = 6, 2, 17
    got = GR.run(y, S, Bn, groups=codes, chains=2, seed=seed, top=5, handle=handle)
    inits = chains.default_inits(n, 2, seed)
    samplers = []
    for c in range(2):
        s = Sampler(handle, y, inits[c], preset="fast", seed=_lib.chain_seed(seed, c))
        s.init()
        s.summary_enable(_lib.SUM_THETA_BETA | _lib.SUM_DIAG, planned_draws=S)
        s.groups_enable(codes, top=5)
        for it in range(S + Bn):
            s.step()
            if it >= Bn:
                s.summary_accumulate()
                s.groups_accumulate()
        s.check()
        samplers.append(s)
    refl = chains.combine(handle, samplers)["diagnostics"]["reflected"]
    want = GR.combine(handle, samplers, signs=[-1 if r else 1 for r in refl], top=5)
    for s in samplers:
        s.close()
    assert np.array_equal(got["reflected"], refl) and got["chains"] == 2 and got["latent_draws"] == 2 * S
    for name, _, _ in _lib.GROUPS_RAW:
        assert same_bits(got["raw"][name], want["raw"][name]), name
    assert same_bits(got["least_loyal"]["respondents"], want["least_loyal"]["respondents"])


def test_refusals(handle):
    from gpirt_amd import Sampler, _lib
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(33, 2, seed=1)
    s = Sampler(handle, y, th0, preset="fast", seed=3)
    s.init()
    with pytest.raises(Exception, match=r"the group posteriors are not enabled \(gpirt_sampler_groups_enable\)"):
        s.groups_accumulate()
    with pytest.raises(ValueError, match="group 1 has no member"):
        s.groups_enable(np.where(np.arange(33) % 2 == 0, 0, 2))
    with pytest.raises(ValueError, match="top must be"):
        s.groups_enable(np.arange(33) % 2, top=65)
    codes = (np.arange(33) % 2).astype(np.int32)
    s.groups_enable(codes)
    s.step()
    s.groups_accumulate()
    assert s.groups_get("counts").tolist() == [1, 0, 1, 0]
    buf = np.zeros(1)
    assert s.lib.gpirt_sampler_groups_get(s._s, b"nope", buf.ctypes.data, 8) == _lib.E_ARG
    assert "unknown groups field" in _lib.last_error()
    assert s.lib.gpirt_sampler_groups_get(s._s, b"c1", buf.ctypes.data, 8) == _lib.E_ARG        # a wrong byte count
    # a refused enable keeps the old state; on=False frees it
    with pytest.raises(ValueError):
        s.groups_enable(np.zeros(33, dtype=np.int32))
    assert s.groups_get("counts").tolist() == [1, 0, 1, 0]
    s.groups_enable(on=False)
    with pytest.raises(Exception, match="not enabled"):
        s.groups_get("counts")
    s.close()
