"""Scoring new respondents on the device (csrc/score.hip) against the NumPy statement of the header
(gpirt_amd.score.from_draws): the stage API at five sizes under both product forms, the chain's own respondents against
gpirt_debug_theta_logpost, constructed f*, the untouched chain, the pooling of reflected chains, repeatability and the
refusals.  The tolerances are derived from each case's own inputs (tests/_score_bounds.py)."""
import ctypes as C

import numpy as np
import pytest

from _score_bounds import EPS, compare, delta_of

pytestmark = pytest.mark.gpu
CODES = dict(yea=[1], nay=[-1], missing=[None])
N = 1001
RAW = ("draws", "nonfinite", "n_obs", "lpd_acc", "ll_sum", "post_sum")


def y_new_for(n_new, m, seed):
    """make_responses with 5 % NaN plus one all-NaN row (the last)"""
    from gpirt_amd.synthetic import make_responses
    y, _ = make_responses(n_new + 1, m, seed=seed, na_frac=0.05)
    y = np.array(y[:n_new])
    y[-1, :] = np.nan
    return y


def run_stage(handle, n, m, n_new, steps, seed=5):
    from gpirt_amd import Sampler, score
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=100 + n, na_frac=0.03)
    y_new = y_new_for(n_new, m, 7 + n_new)
    s = Sampler(handle, y, th0, preset="fast", seed=seed)
    s.init()
    s.score_enable(y_new)
    fs = []
    for _ in range(steps):
        s.step()
        s.score_accumulate()
        fs.append(s.get("fstar"))
    s.check()
    got = s.score()
    raw = {k: s.score_get(k) for k in RAW + ("grid_post", "lpd", "loglik_mean", "theta_mean", "theta_sd", "theta_map")}
    hdr = score.state_header(s.score_state())
    s.close()
    return y_new, np.stack(fs), got, raw, hdr


_reference = {}


def reference(key, y_new, fs):
    """from_draws once per case, shared by the two product forms"""
    from gpirt_amd import score
    if key not in _reference:
        _reference[key] = score.from_draws(y_new, fs, return_products=True)
    return _reference[key]


@pytest.mark.parametrize("fixed", [1, 2])
@pytest.mark.parametrize("n,m,n_new,steps", [(100, 17, 1, 4), (100, 3, 65, 4), (257, 33, 63, 4), (1000, 65, 257, 4),
                                             (8192, 1024, 256, 2)])
def test_stage_api_against_from_draws(handle, n, m, n_new, steps, fixed):
    """A few steps with score_accumulate after each; get("fstar") per draw is the NumPy input.  fixed = 1: the fixed-point
    product; 2: the fp64 GEMM (GPIRT_THETA_FIXED=2).  The chain does not depend on the product's form to the bit, so each
    form is compared with from_draws on ITS OWN f* draws."""
    with handle.config("GPIRT_THETA_FIXED", fixed):
        y_new, fs, got, raw, hdr = run_stage(handle, n, m, n_new, steps)
    assert hdr == dict(n_new=n_new, m=m, version=1, N=N)
    want = reference((n, m, n_new, fixed), y_new, fs)
    delta = delta_of(want["products"][0], m)
    compare(got, want, delta, f"stage n={n} m={m} n_new={n_new} fixed={fixed}")
    assert np.array_equal(got["draws"], np.full(n_new, steps)) and got["n_obs"][-1] == 0
    for k in raw:                                        # score_get and score() read the same block through one finish
        assert np.array_equal(raw[k], got[k], equal_nan=True), k
    # no answers: the posterior is the prior and l = 0
    from gpirt_amd import score
    prior = np.exp(score.logprior() - score.logprior_lse())
    assert np.allclose(got["grid_post"][-1], prior, rtol=4 * N * EPS, atol=0) and abs(got["lpd"][-1]) <= 4 * N * EPS
    lpd = got["lpd"]
    assert abs(got["lpd_total"] - lpd.sum()) <= 4 * n_new * EPS * np.abs(lpd).sum() + 1e-300
    if n_new >= 2:
        assert abs(got["se_lpd_total"] - np.sqrt(n_new * lpd.var(ddof=1))) <= 1e-9 * (1 + got["se_lpd_total"])


@pytest.mark.parametrize("fixed", [1, 2])
def test_own_respondents(handle, fixed):
    """y_new = y[:n_new]: the scorer's product is gpirt_debug_theta_logpost of the same f* (columns :n_new) within delta;
    theta_map of a single draw is the argmax of that log-posterior plus the prior."""
    from gpirt_amd import Sampler, score
    from gpirt_amd.ops import to_device
    from gpirt_amd.synthetic import make_responses
    n, m, n_new = 257, 33, 70
    y, th0 = make_responses(n, m, seed=41, na_frac=0.05)
    with handle.config("GPIRT_THETA_FIXED", fixed):
        s = Sampler(handle, y, th0, preset="fast", seed=8)
        s.init()
        s.score_enable(y[:n_new])
        s.step()
        s.score_accumulate()
        f = s.get("fstar")
        T = s.score_get("product")
        tmap = s.score_get("theta_map")
        s.check()
        s.close()
        lp, fb = handle.theta_logpost(to_device(np.asfortranarray(y)), to_device(f))
    lp = lp.cpu().numpy()[:, :n_new]
    ref = score.product(y[:n_new], f)
    delta = delta_of([ref], m)
    gap_dbg, gap_ref = float(np.abs(T - lp).max()), float(np.abs(T - ref).max())
    print(f"MEASURED own respondents fixed={fixed}: product vs theta_logpost gap {gap_dbg:.3e} (bit-equal "
          f"{np.array_equal(T, lp)}), vs long double {gap_ref:.3e}, delta {delta:.3e}; fell back {fb}")
    assert fb == 0 and gap_dbg <= delta and gap_ref <= delta
    full = score.logprior()[:, None] + lp
    srt = np.sort(full, axis=0)
    clear = srt[-1] - srt[-2] > 2 * delta + 2 * N * EPS
    assert clear.mean() > 0.5
    assert np.array_equal(tmap[clear], score.grid()[np.argmax(full, axis=0)][clear])


def constructed(handle, fstars, y_new, m=6, n=64):
    """score_accumulate called directly on constructed f* (through set("fstar", ...)); returns the sampler's outputs and
    the state block after each draw"""
    from gpirt_amd import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=5)
    s = Sampler(handle, y, th0, preset="fast", seed=3)
    s.init()
    s.score_enable(y_new)
    blocks = []
    for f in fstars:
        s.set("fstar", np.asfortranarray(f))
        s.score_accumulate()
        blocks.append(s.score_state().cpu().numpy().copy())
    got = s.score()
    s.close()
    return got, blocks


def test_constructed_fstar(handle):
    """All zeros; a step at k = 500; |f*| = 800 in one column (the fixed-point form hands over to the fp64 product, which
    holds the overflowed term at -1e300); together against from_draws, and the zero draw against its closed form."""
    from gpirt_amd import score
    m, n_new = 6, 40
    y_new = y_new_for(n_new, m, 19)
    rng = np.random.default_rng(1)
    zero = np.zeros((N, m))
    step = np.where(np.arange(N)[:, None] >= 500, 1.0, -1.0) * rng.uniform(0.5, 3.0, m)
    big = rng.normal(0, 1, (N, m)) * 0.3
    big[:, 2] = np.where(np.arange(N) >= 500, 800.0, -800.0)
    got0, _ = constructed(handle, [zero], y_new)
    prior = np.exp(score.logprior() - score.logprior_lse())
    gap = float(np.abs(got0["grid_post"] / prior[None, :] - 1).max())
    gap_l = float(np.abs(got0["lpd"] + got0["n_obs"] * np.log(2.0)).max())
    print(f"MEASURED zeros: grid_post rel gap to the prior {gap:.3e}, lpd + n_obs log 2 gap {gap_l:.3e}")
    assert gap <= 2 * (2 * m * EPS * m * np.log(2.0)) + 2 * N * EPS and gap_l <= 2 * m * EPS * m * np.log(2.0) + 4 * N * EPS
    for name, fs in (("zeros", [zero]), ("step", [step]), ("handover", [big]), ("all three", [zero, step, big])):
        got, _ = constructed(handle, fs, y_new)
        want = score.from_draws(y_new, np.stack(fs), return_products=True)
        compare(got, want, delta_of(want["products"][0], m), f"constructed {name}")
        assert not got["nonfinite"].any()
    # the hand-over really held a term: those who said -1 to item 2 have no mass at k >= 500
    no = y_new[:, 2] == -1.0
    got, _ = constructed(handle, [big], y_new)
    assert no.any() and (got["grid_post"][no][:, 500:] == 0).all() and (got["lpd"][no] > -1e299).all()


def test_nan_cell_skips_only_those_who_answered(handle):
    """One NaN cell in the second of three draws: only respondents who answered that item gain `nonfinite`, and their other
    accumulators are bit-identical to before; everybody else's draw counts as if nothing had happened."""
    from gpirt_amd import score
    m, n_new = 6, 40
    y_new = y_new_for(n_new, m, 23)
    y_new[0, 4], y_new[1, 4] = np.nan, 1.0               # one who skipped just that item, one who certainly answered it
    rng = np.random.default_rng(2)
    fs = [rng.normal(0, 1, (N, m)) for _ in range(3)]
    bad = [fs[0], fs[1].copy(), fs[2]]
    bad[1][321, 4] = np.nan
    got, blocks = constructed(handle, bad, y_new)
    clean, clean_blocks = constructed(handle, fs, y_new)
    answered = ~np.isnan(y_new[:, 4])
    assert answered.any() and not answered.all()
    assert np.array_equal(got["nonfinite"], answered.astype(np.int64))
    assert np.array_equal(got["draws"], 3 - answered.astype(np.int64))
    # the state blocks word for word: header 8, draws, nonfinite, n_obs, lpd_acc, ll_sum (n_new each), post_sum
    def parts(b):
        o = 8
        d = {}
        for k in ("draws", "nonfinite", "n_obs", "lpd_acc", "ll_sum"):
            d[k] = b[o:o + n_new]
            o += n_new
        d["post_sum"] = b[o:].reshape(n_new, N)
        return d
    before, after, ok_after = parts(blocks[0]), parts(blocks[1]), parts(clean_blocks[1])
    for k in ("draws", "lpd_acc", "ll_sum", "post_sum", "n_obs"):
        assert np.array_equal(after[k][answered], before[k][answered]), k          # skipped: nothing else changed
        assert np.array_equal(after[k][~answered], ok_after[k][~answered]), k      # the others: as without the NaN
    want = score.from_draws(y_new, np.stack(bad), return_products=True)
    compare(got, want, delta_of(want["products"][0], m), "NaN cell")
    print(f"MEASURED NaN cell: {int(answered.sum())} of {n_new} respondents skipped one draw; integers bit-equal True")


@pytest.mark.parametrize("case", ["fast", "reference"])
def test_chain_untouched(case):
    """gpirtMCMC(..., score=y_new) against the same call without it: theta, beta, f and the IRFs bit-identical; under
    rng="reference" R's stream ends at the same position."""
    from gpirt_amd import gpirtMCMC
    from gpirt_amd.ops import RStream
    from gpirt_amd.synthetic import make_responses
    n, m, S, B = 96, 12, 4, 2
    y, th0 = make_responses(n, m, seed=31, snap_theta=False)
    y_new = y_new_for(9, m, 3)
    rs = [None, None]
    if case == "fast":
        kw = dict(vote_codes=CODES, preset="fast", seed=9, chains=2)
    else:
        kw = dict(vote_codes=CODES, theta_init=th0)
        rs = [RStream(77), RStream(77)]
    res = []
    for k, sc in enumerate((None, y_new)):
        extra = dict(rstream=rs[k]) if rs[k] is not None else {}
        res.append(gpirtMCMC(y, S, B, score=sc, **kw, **extra))
    plain, scored = res
    assert "score" not in plain and "score" in scored and "summary" in scored and "diagnostics" in scored
    same = all(np.array_equal(plain[k], scored[k], equal_nan=True) for k in ("theta", "beta", "f", "IRFs"))
    print(f"MEASURED untouched chain {case}: draws and IRFs bit-equal {same}")
    assert same
    if case == "reference":
        (mt0, i0), (mt1, i1) = rs[0].state(), rs[1].state()
        assert i0 == i1 and np.array_equal(mt0, mt1)
    C_ = 2 if case == "fast" else 1
    sc = scored["score"]
    assert np.array_equal(sc["draws"] + sc["nonfinite"], np.full(9, C_ * S)) and sc["grid_post"].shape == (9, N)
    assert np.allclose(sc["grid_post"].sum(axis=1), 1.0, atol=1e-12) and (sc["lpd"][:-1] < 0).all()
    assert abs(sc["lpd"][-1]) <= 4 * N * EPS


def test_chains_pool_with_reflection(handle):
    """Two chains' states through score.combine with signs (+1, -1) against from_draws(signs=...) on the stacked f*
    draws; gpirtMCMC(chains=2, score=...) equals combine of the replayed chains' states with diagnostics["reflected"]."""
    from gpirt_amd import Sampler, _lib, gpirtMCMC, score
    from gpirt_amd.synthetic import make_responses
    n, m, S, B, seed, n_new = 200, 24, 4, 2, 29, 33
    y, th0 = make_responses(n, m, seed=11)
    y_new = y_new_for(n_new, m, 13)
    inits = np.stack([th0, -th0])
    res = gpirtMCMC(y, S, B, vote_codes=CODES, theta_init=inits, rng="item", seed=seed, theta_stabilise=True, chains=2,
                    align=True, score=dict(data=y_new, probs=(0.1, 0.5, 0.9)))
    refl = res["diagnostics"]["reflected"]
    signs = np.where(refl, -1, 1)
    samplers, fs = [], []
    for c in range(2):
        s = Sampler(handle, y, inits[c], rng="item", seed=_lib.chain_seed(seed, c), theta_stabilise=True)
        s.init()
        s.score_enable(y_new)
        fc = []
        for it in range(S + B):
            s.step()
            if it >= B:
                s.score_accumulate()
                fc.append(s.get("fstar"))
        s.check()
        samplers.append(s)
        fs.append(np.stack(fc))
    pooled = score.combine(handle, samplers, signs=signs, probs=(0.1, 0.5, 0.9))
    equal = all(np.array_equal(np.asarray(pooled[k]), np.asarray(res["score"][k]), equal_nan=True) for k in pooled)
    print(f"MEASURED gpirtMCMC(chains=2) against combine of the replayed states: bit-equal {equal}; reflected {refl}")
    assert equal
    forced = score.combine(handle, samplers, signs=[1, -1], probs=(0.1, 0.5, 0.9))
    want = score.from_draws(y_new, np.stack(fs), probs=(0.1, 0.5, 0.9), signs=[1, -1], return_products=True)
    delta = max(delta_of(p, m) for p in want["products"])
    compare(forced, want, delta, "combine signs (+1, -1)")
    st = samplers[0].score_state()
    sym = score.combine(handle, [st, st.clone()], signs=[1, -1])
    assert np.array_equal(sym["post_sum"], sym["post_sum"][:, ::-1]) and np.array_equal(sym["draws"], np.full(n_new, 2 * S))
    for s in samplers:
        s.close()


def test_repeatable(handle):
    """The same run twice gives bit-identical state blocks."""
    blocks = []
    for _ in range(2):
        from gpirt_amd import Sampler
        from gpirt_amd.synthetic import make_responses
        y, th0 = make_responses(257, 33, seed=21)
        s = Sampler(handle, y, th0, preset="fast", seed=21)
        s.init()
        s.score_enable(y_new_for(63, 33, 2))
        for _ in range(3):
            s.step()
            s.score_accumulate()
        s.check()
        blocks.append(s.score_state().cpu().numpy().copy())
        s.close()
    same = np.array_equal(blocks[0], blocks[1])
    print(f"MEASURED repeatability: state blocks bit-equal {same}")
    assert same


def test_refusals(handle):
    from gpirt_amd import Sampler, _lib, gpirtMCMC
    from gpirt_amd.distributed import ShardedSampler
    from gpirt_amd.synthetic import make_responses
    n, m = 64, 6
    y, th0 = make_responses(n, m, seed=5)
    s = Sampler(handle, y, th0, preset="fast", seed=3)
    s.init()
    with pytest.raises(_lib.GpirtError, match="not enabled"):
        s.score_get("draws")
    with pytest.raises(_lib.GpirtError, match="not enabled"):
        s.score_accumulate()
    with pytest.raises(ValueError, match="unanimous"):
        s.score_enable(np.ones((3, m + 1)))
    bad = np.ones((3, m))
    bad[1, 2] = 0.0
    with pytest.raises(ValueError, match=r"\+1, -1 or NaN"):
        s.score_enable(bad)
    with pytest.raises(ValueError, match="outside"):
        s.score_enable(np.ones((0, m)))
    with pytest.raises(ValueError, match="outside"):
        s.score_enable(np.ones((16385, m)))
    # the library itself refuses the same, before anything is touched: an enabled state survives a refused call
    good = np.asfortranarray(np.ones((3, m)))
    s.score_enable(good)
    dp = C.POINTER(C.c_double)
    big = np.asfortranarray(np.ones((16385, m)))
    badf = np.asfortranarray(bad)
    for arr, cnt in ((big, 16385), (badf, 3), (good, -1)):
        assert s.lib.gpirt_sampler_score_enable(s._s, arr.ctypes.data_as(dp), cnt) == _lib.E_ARG
    assert s.score_get("n_obs").tolist() == [m, m, m]
    s.score_enable(None)                                 # n_new = 0 / NULL: off, the state freed
    with pytest.raises(_lib.GpirtError, match="not enabled"):
        s.score_get("draws")
    s.close()
    with pytest.raises(ValueError, match="unanimous"):
        gpirtMCMC(y, 1, 0, vote_codes=CODES, theta_init=th0, preset="fast", score=np.ones((2, m + 2)))
    with pytest.raises(ValueError, match="item shards"):
        ShardedSampler.score_enable(object(), np.ones((1, m)))
