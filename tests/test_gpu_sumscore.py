"""Sum-score posteriors on the device (csrc/sumscore.hip) against the NumPy statement of the header
(gpirt_amd.sumscore.from_draws) inside tests/_sumscore_bounds.py's counted bounds: constructed f* through set("fstar") at the
edges of the row kernel's register classes, the exact cases bit for bit, NaN handling, the tie to the device's scorer by
enumeration, real chains, the untouched chain, the pooling of reflected chains and the refusals.  n = 33 throughout."""
import itertools
import math

import numpy as np
import pytest

import _score_bounds as SB
import _sumscore_bounds as B

pytestmark = pytest.mark.gpu
N_RESP = 33
NG = 1001
TH = -5.0 + np.arange(NG) * 0.01
CODES = dict(yea=[1], nay=[-1], missing=[None])
RAW = ("joint_sum", "pi_sum", "pi_sumsq", "tcc_sum", "tcc_sumsq", "var_sum", "rel", "mask", "w", "last", "last_pi")


def responses(m, seed=7):
    from gpirt_amd.synthetic import make_responses
    return make_responses(N_RESP, m, seed=seed + m, na_frac=0.03)


def new_sampler(handle, m, **kw):
    from gpirt_amd import Sampler
    y, th0 = responses(m)
    s = Sampler(handle, y, th0, **(kw or dict(preset="fast", seed=3)))
    s.init()
    return s


def raw_of(s):
    """the sampler's raw accumulators and counters as B.check reads them (no finishing: the big forms stay quick)"""
    got = {k: s.sumscore_get(k) for k in RAW}
    c = s.sumscore_get("counts")
    got.update(draws=int(c[0]), skipped=int(c[1]), rel_draws=int(c[2]), rel_skipped=int(c[3]), M=int(got["mask"].sum()))
    return got


def curves(m, seed, scale=1.0):
    """a 2PL-like f* (1001 x m) with noise, either sign of slope, and grid row 777 unlike its neighbours"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.3, 2.5, m) * rng.choice([-1.0, 1.0], m)
    f = scale * (a[None, :] * (TH[:, None] - rng.normal(size=m)[None, :]) + 0.3 * rng.normal(size=(NG, m)))
    f[777] = scale * 3.0 * rng.normal(size=m)
    return f


def blocks(m, seed, scale):
    """f* (1001 x m) of three distinct rows only -- k < 400, k >= 400 and k = 777 -- so that the reference works three rows"""
    rng = np.random.default_rng(seed)
    rows = scale * rng.normal(size=(3, m))
    f = np.where((np.arange(NG) < 400)[:, None], rows[0][None, :], rows[1][None, :])
    f[777] = rows[2]
    return f


def row_sums_are_one(last, M):
    assert np.abs(last.sum(axis=1) - 1.0).max() <= B.rel_A(M) + (M + 2) * B.EPS


@pytest.mark.parametrize("M", [1, 2, 63, 64, 127, 128])
def test_small_forms_at_the_lane_edges(handle, M):
    """the whole of a small m: M + 1 in {2, 3, 64, 65, 128, 129}; two draws, the second of larger scale"""
    from gpirt_amd import sumscore
    s = new_sampler(handle, M)
    s.sumscore_enable()
    draws = [curves(M, 100 + M), curves(M, 200 + M, scale=4.0)]
    for f in draws:
        s.set("fstar", f)
        s.sumscore_accumulate()
    got, full = raw_of(s), s.sumscore()
    hdr = sumscore.state_header(s.sumscore_state())
    s.close()
    want = sumscore.from_draws(np.stack(draws))
    B.check(got, want, f"M = {M}")
    row_sums_are_one(got["last"], M)
    assert hdr == dict(tag=0x43534D53, version=1, m=M, M=M, N=NG, draws=2, skipped=0, rel_draws=2, rel_skipped=0)
    for k in RAW:                               # the getters and the combine read the same block
        assert np.array_equal(full[k], got[k]), k
    for k in ("score_dist", "theta_eap", "tcc_mean", "csem"):
        assert np.allclose(full[k], want[k], rtol=1e-9, atol=1e-300, equal_nan=True), k


@pytest.fixture(scope="module")
def big(handle):
    s = new_sampler(handle, 4096)
    yield s
    s.close()


@pytest.mark.parametrize("M", [1087, 1088, 2111, 2112, 2113, 4096])
def test_masked_forms_at_the_class_edges(big, M):
    """items= masks over one sampler with m = 4096: M + 1 = 1088 | 1089 and 2112 | 2113 are the row kernel's class edges
    (17 | 33 | 65 doubles a lane), 4096 is the longest form.  The forms are no prefix: items 0 and m - 1 are outside
    wherever there is room."""
    from gpirt_amd import sumscore
    m = 4096
    rng = np.random.default_rng(M)
    if M == m:
        items = np.arange(m)
    else:
        items = np.sort(rng.choice(np.arange(1, m - 1), size=M, replace=False))
    big.sumscore_enable(items=items)
    f = blocks(m, M, scale=2.0)
    big.set("fstar", f)
    big.sumscore_accumulate()
    got = raw_of(big)
    big.sumscore_enable(on=False)
    want = sumscore.from_draws(f[None], items=items)
    B.check(got, want, f"m = 4096, M = {M}")
    row_sums_are_one(got["last"], M)
    assert got["M"] == M and np.array_equal(np.flatnonzero(got["mask"]), items)


def test_exact_cases_hold_bit_for_bit(handle):
    """f* = 0 over 50 items: the binomial, every product and sum exact; columns of +-inf: the whole mass on one score, and one
    more column at 0 gives two cells of 1/2; |f*| = 800 gives no NaN"""
    from gpirt_amd import sumscore
    s = new_sampler(handle, 50)
    s.sumscore_enable()
    s.set("fstar", np.zeros((NG, 50)))
    s.sumscore_accumulate()
    want = np.array([math.comb(50, k) for k in range(51)], dtype=np.float64) * 2.0 ** -50
    assert np.array_equal(s.sumscore_get("last"), np.tile(want, (NG, 1)))
    assert np.array_equal(s.sumscore_get("tcc"), np.full(NG, 25.0)) and np.array_equal(s.sumscore_get("var"), np.full(NG, 12.5))   # T = 50 / 2, V = 50 / 4
    w = sumscore.grid_weights()
    assert np.array_equal(s.sumscore_get("w"), w) and np.array_equal(s.sumscore_get("joint_sum"), w[:, None] * want[None, :])
    f = np.full((NG, 50), -np.inf)
    f[:, 3:10] = np.inf
    f[:, 20] = 0.0
    f[:, 30] = np.nan                               # outside the form below
    items = [2, 3, 4, 5, 6, 7, 8, 9, 11, 20, 48]    # 7 at +inf, 3 at -inf, one at 0
    s.sumscore_enable(items=items)
    s.set("fstar", f)
    s.sumscore_accumulate()
    want = np.zeros(12); want[7] = want[8] = 0.5
    assert np.array_equal(s.sumscore_get("last"), np.tile(want, (NG, 1))) and s.sumscore_get("counts").tolist()[:2] == [1, 0]
    assert np.array_equal(s.sumscore_get("tcc"), np.full(NG, 7.5)) and np.array_equal(s.sumscore_get("var"), np.full(NG, 0.25))
    s.sumscore_enable()
    f = np.where(np.arange(50)[None, :] % 2 == 0, 800.0, -800.0) * np.where(np.arange(NG)[:, None] < 500, 1.0, -1.0)
    s.set("fstar", f)
    s.sumscore_accumulate()
    got = raw_of(s)
    s.close()
    for k in RAW:
        assert np.isfinite(got[k]).all(), k
    want = np.zeros(51); want[25] = 1.0
    assert np.array_equal(got["last"], np.tile(want, (NG, 1))) and got["draws"] == 1


def test_a_transposed_or_shifted_row_cannot_pass(handle):
    """one grid row unlike the others, a form that is no prefix of the columns (items 0 and m - 1 outside it), and columns
    outside the form that would change every number if they were read"""
    from gpirt_amd import sumscore
    m = 40
    items = [1, 3, 4, 7, 8, 9, 15, 16, 22, 23, 24, 30, 31, 37, 38]
    f = curves(m, 5)
    f[:, [0, 2, 39]] = 50.0
    s = new_sampler(handle, m)
    s.sumscore_enable(items=items)
    s.set("fstar", f)
    s.sumscore_accumulate()
    got = raw_of(s)
    s.close()
    want = sumscore.from_draws(f[None], items=items)
    B.check(got, want, "m = 40, a form of 15")
    shifted = sumscore.from_draws(np.roll(f, 1, axis=0)[None], items=items)
    prefix = sumscore.from_draws(f[None], items=list(range(15)))
    for other in (shifted, prefix):                 # the test can tell them apart
        assert (np.abs(other["last"] - want["last"]) > B.bounds(want)["last"]).any()


def test_nan_in_the_form_skips_the_draw_whole(handle):
    from gpirt_amd import sumscore
    m = 12
    items = [1, 2, 5, 6, 7, 10]
    f = curves(m, 9)
    s = new_sampler(handle, m)
    s.sumscore_enable(items=items)
    s.set("fstar", f)
    s.sumscore_accumulate()
    before = s.sumscore_state().cpu().numpy().copy()
    bad = curves(m, 10)
    bad[NG - 1, 10] = np.nan                        # a form column, the last grid point
    s.set("fstar", bad)
    s.sumscore_accumulate()
    after = s.sumscore_state().cpu().numpy().copy()
    assert after[6] == 1 and before[6] == 0
    after[6] = 0
    assert after.tobytes() == before.tobytes()      # nothing else was touched
    out = curves(m, 11)
    out[0, 0] = out[500, 11] = out[NG - 1, 3] = np.nan       # outside the form: still counted
    s.set("fstar", out)
    s.sumscore_accumulate()
    got = raw_of(s)
    s.close()
    assert (got["draws"], got["skipped"]) == (2, 1)
    B.check(got, sumscore.from_draws(np.stack([f, bad, out]), items=items), "NaN inside and outside the form")


def test_enumeration_identity_device_against_device(handle):
    """score_enable with the 256 answer patterns of an 8-item form and sumscore_enable on the same sampler and the same
    draw: sum of exp(lpd) over the patterns with sum s = pi[s], sum of exp(lpd) grid_post = joint_sum[:, s]"""
    from gpirt_amd import score, sumscore
    M = 8
    pats = np.array(list(itertools.product([-1.0, 1.0], repeat=M)))
    f = curves(M, 21)
    s = new_sampler(handle, M)
    s.score_enable(pats)
    s.sumscore_enable()
    s.set("fstar", f)
    s.score_accumulate()
    s.sumscore_accumulate()
    sc, ss = s.score(), raw_of(s)
    s.close()
    ref = score.from_draws(pats, f[None], return_products=True)
    delta = SB.delta_of(ref["products"][0], M)
    rho = 2.0 * delta + 2.0 * NG * B.EPS
    e_l = delta + 2.0 * NG * B.EPS * (1.0 + np.abs(ref["lpd"]).max())
    bd = B.bounds(sumscore.from_draws(f[None]))
    sums = (pats == 1.0).sum(axis=1)
    L = np.exp(sc["lpd"])
    share = 0.0
    for k in range(M + 1):
        idx = np.flatnonzero(sums == k)
        pi = L[idx].sum()
        joint = (L[idx, None] * sc["grid_post"][idx]).sum(axis=0)
        tol_pi = (e_l + (len(idx) + NG + 2) * B.EPS) * 1.01 * pi + bd["pi_sum"][k]
        tol_j = (e_l + rho + (len(idx) + NG + 2) * B.EPS) * 1.01 * joint + bd["joint_sum"][:, k]
        share = max(share, abs(pi - ss["pi_sum"][k]) / tol_pi, (np.abs(joint - ss["joint_sum"][:, k]) / tol_j).max())
    print(f"MEASURED enumeration identity on the device: share of the bound used {share:.3f}")
    assert share <= 1.0


@pytest.mark.parametrize("m,form", [(31, "fast"), (65, "fast"), (31, "reference")])
def test_real_chains_against_from_draws(handle, m, form):
    """six steps with sumscore_accumulate() after each, f* fetched each time"""
    from gpirt_amd import Sampler, sumscore
    from gpirt_amd.ops import RStream
    y, th0 = responses(m)
    kw = dict(preset="fast", seed=2**33 + 5) if form == "fast" else dict(rng="reference", rstream=RStream(41), theta_stabilise=False)
    s = Sampler(handle, y, th0, **kw)
    s.init()
    items = None if m == 31 else [j for j in range(m) if j % 3 != 0]
    s.sumscore_enable(items=items)
    draws = []
    for _ in range(6):
        s.step()
        s.sumscore_accumulate()
        draws.append(s.get("fstar"))
    s.check()
    got = s.sumscore(y=y)
    s.close()
    want = sumscore.from_draws(np.stack(draws), items=items, y=y)
    B.check(got, want, f"chain {N_RESP}x{m} {form}")
    assert got["draws"] == 6 and got["obs_hist"].tolist() == want["obs_hist"].tolist() and got["n_complete"] == want["n_complete"]
    for k in ("score_dist", "score_cdf", "theta_eap", "theta_sd", "tcc_mean", "csem", "reliability_mean"):
        assert np.allclose(got[k], want[k], rtol=1e-9, atol=1e-300, equal_nan=True), k


@pytest.mark.parametrize("case", ["fast", "fast_all", "reference"])
def test_chain_untouched_and_repeatable(handle, case):
    """gpirtMCMC(..., sumscore=True) against the same call without: theta, beta, f, the IRFs, R's stream position and the
    other blocks' results bit-identical; a second run gives byte-identical sum-score accumulators; and, one chain under the fast
    preset and under R's stream, res["sumscore"] -- accumulated from the checkpoint slot's f*, or right after the step -- is
    bit for bit the stage API's state over the same chain, and within the bounds of from_draws of that chain's fetched f*."""
    from gpirt_amd import Sampler, gpirtMCMC, sumscore
    from gpirt_amd.ops import RStream
    m, S, Bn = 31, 6, 2
    y, th0 = responses(m, seed=31)
    kw = dict(vote_codes=CODES, theta_init=th0)
    seeds = [None, None, None]
    if case == "fast":
        kw.update(preset="fast", seed=9)
    elif case == "fast_all":
        y_new = np.where(np.random.default_rng(3).random((5, y.shape[1])) < 0.5, 1.0, -1.0)
        kw.update(preset="fast", seed=9, chains=2, theta_init=None, summaries=("waic",), quantiles=(0.025, 0.5, 0.975),
                  ppc=True, ranks=True, score=y_new, shape=True)
    else:
        seeds = [RStream(77), RStream(77), RStream(77)]
    res = []
    for k, on in enumerate((None, True, True)):
        extra = dict(rstream=seeds[k]) if seeds[k] is not None else {}
        res.append(gpirtMCMC(y, S, Bn, sumscore=on, **kw, **extra))
    plain, with_ss, again = res
    assert "sumscore" not in plain and "sumscore" in with_ss
    for k in ("theta", "beta", "f", "IRFs"):
        assert np.array_equal(plain[k], with_ss[k], equal_nan=True), k
    if case == "reference":
        (mt0, i0), (mt1, i1) = seeds[0].state(), seeds[1].state()
        assert i0 == i1 and np.array_equal(mt0, mt1)

    def same(a, b, path):
        if isinstance(a, dict):
            assert set(a) == set(b), path
            for k in a:
                same(a[k], b[k], path + (k,))
        elif a is None:
            assert b is None, path
        else:
            assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), path

    if case == "fast_all":
        for block in ("summary", "quantiles", "ppc", "ranks", "score", "shape"):
            same(plain[block], with_ss[block], (block,))
    ss = with_ss["sumscore"]
    C_ = 2 if case == "fast_all" else 1
    assert ss["draws"] + ss["skipped"] == C_ * S and ss["M"] == y.shape[1] and ss["n_complete"] <= N_RESP
    for k in RAW:
        assert ss[k].tobytes() == again["sumscore"][k].tobytes(), k
    if case == "fast_all":
        return                                  # (several chains against the stage API: test_chains_pool_with_reflection)
    skw = dict(preset="fast", seed=9) if case == "fast" else dict(rng="reference", rstream=RStream(77), theta_stabilise=False)
    s = Sampler(handle, y, th0, **skw)
    s.init()
    s.sumscore_enable()
    draws = []
    for it in range(S + Bn):
        s.step()
        if it >= Bn:
            s.sumscore_accumulate()
            draws.append(s.get("fstar"))
    s.check()
    stage = s.sumscore(y=y)
    s.close()
    for k in RAW + ("score_dist", "post", "theta_eap", "tcc_mean", "csem", "obs_hist"):
        assert np.array_equal(np.asarray(ss[k]), np.asarray(stage[k]), equal_nan=True), k
    assert ss["reliability_mean"] == stage["reliability_mean"] and ss["draws"] == S
    B.check(ss, sumscore.from_draws(np.stack(draws), y=y), f"gpirtMCMC {case}")


def test_chains_pool_with_reflection(handle):
    """chains=2, chain 1 started at -theta0: res["sumscore"] equals sumscore.combine of the two chains' state blocks with the
    run's signs bit for bit; forced signs (+1, -1) against from_draws, whose reflected chain has its grid reversed"""
    from gpirt_amd import Sampler, _lib, gpirtMCMC, sumscore
    m, S, Bn, seed = 33, 5, 2, 29
    y, th0 = responses(m, seed=11)
    inits = np.stack([th0, -th0])
    items = list(range(2, 30))
    res = gpirtMCMC(y, S, Bn, vote_codes=CODES, theta_init=inits, rng="item", seed=seed, theta_stabilise=True, chains=2,
                    align=True, sumscore=dict(items=items), store_draws=False)
    signs = np.where(res["diagnostics"]["reflected"], -1, 1)
    samplers, draws = [], []
    for c in range(2):
        s = Sampler(handle, y, inits[c], rng="item", seed=_lib.chain_seed(seed, c), theta_stabilise=True)
        s.init()
        s.sumscore_enable(items=items)
        ch = []
        for it in range(S + Bn):
            s.step()
            if it >= Bn:
                s.sumscore_accumulate()
                ch.append(s.get("fstar"))
        s.check()
        samplers.append(s)
        draws.append(np.stack(ch))
    pooled = sumscore.combine(handle, samplers, signs=signs, y=y)
    for k in RAW + ("score_dist", "post", "theta_eap", "theta_quantiles", "tcc_sd", "csem", "obs_hist"):
        assert np.array_equal(np.asarray(pooled[k]), np.asarray(res["sumscore"][k]), equal_nan=True), k
    assert pooled["reliability_mean"] == res["sumscore"]["reliability_mean"] and pooled["draws"] == 2 * S
    B.check(pooled, sumscore.from_draws(draws, items=items, signs=list(signs)), "chains=2, the run's signs")
    forced = sumscore.combine(handle, samplers, signs=[1, -1])
    B.check(forced, sumscore.from_draws(draws, items=items, signs=[1, -1]), "signs (+1, -1)")
    one = samplers[1].sumscore()
    assert np.array_equal(samplers[1].sumscore(sign=-1)["joint_sum"], one["joint_sum"][::-1])
    assert np.array_equal(samplers[1].sumscore(sign=-1)["pi_sum"], one["pi_sum"])
    other = Sampler(handle, y, th0, preset="fast", seed=1)
    other.init()
    other.sumscore_enable(items=items[1:])
    samplers.append(other)
    with pytest.raises(_lib.GpirtError, match="another form"):
        sumscore.combine(handle, [samplers[0], other])
    for s in samplers:
        s.close()


def test_refusals(handle):
    from gpirt_amd import _lib, gpirtMCMC
    from gpirt_amd.distributed import ShardedSampler
    y, th0 = responses(3)
    s = new_sampler(handle, 3)
    for call in (s.sumscore_accumulate, s.sumscore_state, lambda: s.sumscore_get("rel")):
        with pytest.raises(_lib.GpirtError, match="not enabled"):
            call()
    for items, word in (([], "empty"), (np.zeros(3, dtype=bool), "empty"), ([3], "outside"), ([-1], "outside")):
        with pytest.raises(ValueError, match=word):
            s.sumscore_enable(items=items)
        with pytest.raises(ValueError, match=word):
            gpirtMCMC(y, 2, 1, vote_codes=CODES, preset="fast", sumscore=dict(items=items))
    none = np.zeros(3, dtype=np.uint8)                # (kept alive: the library reads it)
    zero = none.ctypes.data
    assert s.lib.gpirt_sampler_sumscore_enable(s._s, zero, 1) == _lib.E_ARG and "empty" in _lib.last_error()
    s.sumscore_enable()
    with pytest.raises(_lib.GpirtError, match="unknown sumscore field"):
        s.sumscore_get("nope")
    assert s.lib.gpirt_sampler_sumscore_enable(s._s, zero, 1) == _lib.E_ARG          # refused: the old state is kept
    assert s.sumscore_get("counts").tolist() == [0, 0, 0, 0]
    s.sumscore_enable(on=False)
    with pytest.raises(_lib.GpirtError, match="not enabled"):
        s.sumscore_state()
    s.close()
    # M > 4096 needs m > 4096 and is refused before any device work; the longest form itself is taken (above)
    with pytest.raises(ValueError, match="at most 4096"):
        from gpirt_amd import sumscore
        sumscore.form_mask(None, 4097)
    import ctypes as C
    nb = C.c_int64()
    assert _lib.load().gpirt_sumscore_state_bytes(5000, 4097, C.byref(nb)) == _lib.E_ARG
    assert _lib.load().gpirt_sumscore_state_bytes(5000, 4096, C.byref(nb)) == 0
    wide = new_sampler(handle, 4097)                # the library's own refusal of M > 4096: all 4097 items, and a mask of 4097
    ones = np.ones(4097, dtype=np.uint8)
    for mask in (None, ones.ctypes.data):
        assert wide.lib.gpirt_sampler_sumscore_enable(wide._s, mask, 1) == _lib.E_ARG and "at most 4096" in _lib.last_error()
    ones[5] = 0
    assert wide.lib.gpirt_sampler_sumscore_enable(wide._s, ones.ctypes.data, 1) == 0
    assert wide.sumscore_get("counts").tolist() == [0, 0, 0, 0]
    wide._sumscore_M = 4096
    assert int(wide.sumscore_get("mask").sum()) == 4096 and wide.lib.gpirt_sampler_sumscore_enable(wide._s, None, 0) == 0
    wide.close()
    with pytest.raises(ValueError, match="not offered for item shards"):
        ShardedSampler.sumscore_enable(None)
