"""Two-form score equating on the device (csrc/equate.hip) against the NumPy statement of the header
(gpirt_amd.equate.from_draws) inside tests/_equate_bounds.py's counted bounds: constructed f* through set("fstar") at the lane
edges of the row kernel and the tile edges of the product, the register-class edge, a joint that is transposed or shifted, the
device against itself, exact inputs, infinities, the skip rule, real chains, the untouched chain, the pooling of chains and the
refusals.  n = 33 throughout."""
import math

import numpy as np
import pytest

import _equate_bounds as B
import _equate_cases as CASES
import _sumscore_bounds as SB

pytestmark = pytest.mark.gpu
N_RESP = 33
NG = 1001
CODES = dict(yea=[1], nay=[-1], missing=[None])
RAW = B.RAW
DERIVED = ("joint", "x_dist", "y_dist", "y_given_x", "x_given_y", "y_given_x_mean", "x_given_y_mean",
           "y_given_x_quantiles", "x_given_y_quantiles")


def check_derived(got, want):
    """the outputs that are ratios of sums of non-negative cells: relative; agreement and kappa (kappa's numerator cancels):
    within tests/_equate_bounds.py's decision_tol, from the reference alone"""
    for k in DERIVED:
        assert np.allclose(got[k], want[k], rtol=1e-9, atol=1e-300, equal_nan=True), k
    tol_a, tol_k = B.decision_tol(want)
    assert np.isfinite(tol_k).all() and len(tol_k) == len(want["cuts"])
    print("MEASURED agreement / kappa: share of the tolerance used",
          (np.abs(got["agreement"] - want["agreement"]) / tol_a).max(initial=0.0), (np.abs(got["kappa"] - want["kappa"]) / tol_k).max(initial=0.0))
    assert (np.abs(got["agreement"] - want["agreement"]) <= tol_a).all(), "agreement"
    assert (np.abs(got["kappa"] - want["kappa"]) <= tol_k).all(), "kappa"


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
    got = {k: s.equate_get(k) for k in RAW}
    c = s.equate_get("counts")
    got.update(draws=int(c[0]), skipped=int(c[1]), corr_draws=int(c[2]), corr_skipped=int(c[3]), eq_clamped=int(c[4]),
               Mx=int(got["mask_x"].sum()), My=int(got["mask_y"].sum()))
    return got


def run_draws(s, x, y, draws):
    s.equate_enable(x, y)
    for f in draws:
        s.set("fstar", f)
        s.equate_accumulate()
    return raw_of(s)


def reference(draws, x, y, **kw):
    from gpirt_amd import equate
    draws = [np.asarray(f) for f in draws]
    singles = [equate.from_draws(f[None], x, y) for f in draws]
    whole = singles[0] if len(draws) == 1 and not kw else equate.from_draws(np.stack(draws), x, y, **kw)
    return whole, [one for one in singles if one["draws"] == 1]


@pytest.mark.parametrize("Mx,My", CASES.SHAPES)
def test_small_forms_against_the_reference(handle, Mx, My):
    """M + 1 in {2, 3, 64, 65, 66, 128, 129} on either side, M_X != M_Y wherever it can be; two draws"""
    from gpirt_amd import equate
    x, y, draws = CASES.small_case(Mx, My)
    m = draws[0].shape[1]
    s = new_sampler(handle, m)
    got = run_draws(s, x, y, draws)
    cuts = (((Mx + 1) // 2, (My + 1) // 2),)              # pass marks in the body of both distributions
    full = s.equate(cuts=cuts)
    hdr = equate.state_header(s.equate_state())
    s.close()
    want, singles = reference(draws, x, y, cuts=cuts)
    B.check(got, want, singles, f"({Mx}, {My})")
    assert hdr == dict(tag=0x45545145, version=1, m=m, Mx=Mx, My=My, N=NG, draws=2, skipped=0, corr_draws=2, corr_skipped=0,
                       eq_clamped=got["eq_clamped"])
    assert np.array_equal(np.flatnonzero(got["mask_x"]), x) and np.array_equal(np.flatnonzero(got["mask_y"]), y)
    for k in RAW:                               # the getters and the combine read the same block
        assert np.array_equal(full[k], got[k]), k
    check_derived(full, want)
    assert abs(full["corr_mean"] - want["corr_mean"]) < 1e-9


def big_curves(m, x, y, seed):
    """the constructed curves of the small cases, constant over blocks of 20 grid points (51 distinct rows: the reference
    works each row once), smooth enough for every score in the body of either distribution to keep its bound"""
    f = CASES.curves(m, x, y, seed)
    centre = np.minimum((np.arange(NG) // 20) * 20 + 10, NG - 1)
    return np.ascontiguousarray(f[centre])


@pytest.fixture(scope="module")
def big(handle):
    """(1087, 1089) on m = 2200: M_X + 1 = 1088 is the last form of the 17-register row kernel, M_Y + 1 = 1090 the second of
    the 33-register one; one draw"""
    x, y, m = CASES.forms(1087, 1089, m=2200)
    f = big_curves(m, x, y, 5)
    s = new_sampler(handle, m)
    got = run_draws(s, x, y, [f])
    s.close()
    want, singles = reference([f], x, y)
    return got, want, singles


def test_the_register_class_edge(big):
    got, want, singles = big
    B.check(got, want, singles, "(1087, 1089) on m = 2200", quarter=False)
    assert np.abs(got["last_joint"].sum() - 1.0) < 1e-9


def test_a_transposed_or_shifted_joint_cannot_pass(handle):
    """forms of one size and clearly different difficulty: the transposed joint and the joint shifted by one score along
    either axis lie outside the bounds, so the comparison can tell them from the right one"""
    x, y, m = CASES.forms(20, 20)
    f = CASES.curves(m, x, y, 77, shift=2.0)
    s = new_sampler(handle, m)
    got = run_draws(s, x, y, [f])
    s.close()
    want, singles = reference([f], x, y)
    B.check(got, want, singles, "(20, 20), Y much easier")
    bd = B.bounds(want, singles)
    J = want["last_joint"]
    for other in (J.T, np.roll(J, 1, axis=0), np.roll(J, 1, axis=1)):
        assert (np.abs(other - J) > bd["last_joint"]).any()
    assert (np.abs(want["last_exy"] - want["last_eyx"]) > bd["last_eyx"]).any()
    assert (np.abs(want["last_piy"] - want["last_pix"]) > bd["last_pix"]).any()


def test_device_against_device(handle):
    """no reference: on one sampler and one draw, the anti-diagonal sums of last_joint are sumscore's last_pi of the union form,
    and the row and column sums are last_pix and last_piy -- within the two modules' bounds"""
    x, y, m = CASES.forms(40, 70)
    f = CASES.curves(m, x, y, 31)
    s = new_sampler(handle, m)
    got = run_draws(s, x, y, [f])
    s.sumscore_enable(items=np.sort(np.concatenate([x, y])))
    s.sumscore_accumulate()
    union = s.sumscore_get("last_pi")
    s.close()
    J = got["last_joint"]
    bJ = B.rel_J(40, 70) * J + B.floor_J(40, 70)
    share = 0.0
    anti = np.array([np.trace(J[:, ::-1], offset=70 - u) for u in range(111)])
    b_anti = np.array([np.trace(bJ[:, ::-1], offset=70 - u) for u in range(111)])
    tol = b_anti + 41 * B.EPS * anti + B.r_pi(110) * union + 111 * SB.FLOOR
    share = max(share, (np.abs(anti - union) / tol).max())
    for axis, key, M, cells in ((1, "last_pix", 40, 71), (0, "last_piy", 70, 41)):
        tol = bJ.sum(axis=axis) + cells * B.EPS * J.sum(axis=axis) + B.r_pi(M) * got[key] + (M + 1) * SB.FLOOR
        share = max(share, (np.abs(J.sum(axis=axis) - got[key]) / tol).max())
    print(f"MEASURED device against device: share of the bound used {share:.3f}")
    assert share <= 1.0


def test_exact_inputs(handle):
    """f* = 0 everywhere, M_X = 20, M_Y = 30: A is the binomial and exact, last_pix follows bit for bit in the order of the pi
    kernel, and last_joint and its row sums to the product's rounding"""
    from gpirt_amd import sumscore
    s = new_sampler(handle, 53)
    x, y = np.arange(1, 21), np.arange(22, 52)
    got = run_draws(s, x, y, [np.zeros((NG, 53))])
    s.close()
    w = sumscore.grid_weights()
    ax = np.array([math.comb(20, k) for k in range(21)], dtype=np.float64) * 2.0 ** -20
    ay = np.array([math.comb(30, k) for k in range(31)], dtype=np.float64) * 2.0 ** -30
    pix, piy = np.zeros(21), np.zeros(31)
    for k in range(NG):                                      # ascending k, each product rounded once
        pix += w[k] * ax
        piy += w[k] * ay
    assert np.array_equal(got["last_pix"], pix) and np.array_equal(got["last_piy"], piy)
    tol = (1 + NG) * 0.5 * B.EPS
    exact = float(np.sum(w.astype(np.longdouble))) * ax[:, None] * ay[None, :]
    assert (np.abs(got["last_joint"] - exact) <= (tol + 2 * B.EPS) * exact).all()
    assert (np.abs(got["last_joint"].sum(axis=1) - pix) <= (2 * tol + 32 * B.EPS) * pix).all()
    assert got["corr_draws"] == 1 and abs(got["corr"][0]) < 1e-9       # flat curves: the scores are independent


def test_infinities_give_a_point_mass(handle):
    x, y, m = np.array([1, 2, 3, 4, 5]), np.array([7, 8, 9, 10]), 12
    f = CASES.curves(m, x, y, 3)
    f[:, [1, 2, 3]] = np.inf
    f[:, [4, 5]] = -np.inf
    s = new_sampler(handle, m)
    got = run_draws(s, x, y, [f])
    s.close()
    assert got["draws"] == 1 and got["skipped"] == 0
    assert (got["last_pix"][[0, 1, 2, 4, 5]] == 0.0).all() and abs(got["last_pix"][3] - 1.0) < 1e-12
    assert (got["last_joint"][[0, 1, 2, 4, 5]] == 0.0).all() and np.allclose(got["last_joint"][3], got["last_piy"], rtol=1e-12)
    for k in ("last_eyx", "last_exy", "eyx_sum", "exy_sumsq", "joint_sum"):
        assert np.isfinite(got[k]).all(), k
    want, _ = reference([f], x, y)
    assert np.allclose(got["last_exy"], want["last_exy"], atol=1e-9) and np.allclose(got["last_eyx"], want["last_eyx"], atol=1e-9)


def test_the_skip_rule(handle):
    x, y, m = np.array([1, 2, 5, 6]), np.array([3, 7, 10]), 12
    good = CASES.curves(m, x, y, 9)
    s = new_sampler(handle, m)
    s.equate_enable(x, y)
    s.set("fstar", good)
    s.equate_accumulate()
    before = s.equate_state().cpu().numpy().copy()
    bads = []
    for skipped, col in ((1, 6), (2, 10)):                   # a column of X, then a column of Y
        bad = CASES.curves(m, x, y, 10 + col)
        bad[NG - 1 if col == 6 else 0, col] = np.nan
        bads.append(bad)
        s.set("fstar", bad)
        s.equate_accumulate()
        after = s.equate_state().cpu().numpy().copy()
        assert after[7] == skipped and before[7] == 0
        after[7] = 0
        assert after.tobytes() == before.tobytes()           # nothing else was touched
    out = CASES.curves(m, x, y, 11)
    out[0, 0] = out[500, 11] = out[NG - 1, 4] = np.nan        # outside both forms: still counted
    s.set("fstar", out)
    s.equate_accumulate()
    got = raw_of(s)
    s.close()
    assert (got["draws"], got["skipped"]) == (2, 2)
    want, singles = reference([good] + bads + [out], x, y)
    assert want["skipped"] == 2 and len(singles) == 2
    B.check(got, want, singles, "NaN inside and outside the forms")


def chain_forms(m):
    return [j for j in range(m) if j % 3 == 0], [j for j in range(m) if j % 3 == 1]


@pytest.mark.parametrize("m,form", [(31, "fast"), (65, "fast"), (31, "reference")])
def test_real_chains_against_from_draws(handle, m, form):
    """six steps with equate_accumulate() after each, f* fetched each time; the derived outputs included"""
    from gpirt_amd import Sampler
    from gpirt_amd.ops import RStream
    y, th0 = responses(m)
    kw = dict(preset="fast", seed=2**33 + 5) if form == "fast" else dict(rng="reference", rstream=RStream(41), theta_stabilise=False)
    s = Sampler(handle, y, th0, **kw)
    s.init()
    fx, fy = chain_forms(m)
    cuts = ((len(fx) // 2, len(fy) // 2), (1, len(fy)))
    s.equate_enable(fx, fy)
    draws = []
    for _ in range(6):
        s.step()
        s.equate_accumulate()
        draws.append(s.get("fstar"))
    s.check()
    got = s.equate(cuts=cuts)
    s.close()
    want, singles = reference(draws, fx, fy, cuts=cuts)
    B.check(got, want, singles, f"chain {N_RESP}x{m} {form}", quarter=False)
    assert got["draws"] == 6
    check_derived(got, want)
    bd = B.bounds(want, singles)
    for k, e in (("y_of_x", "eyx"), ("x_of_y", "exy")):      # the means: the sums' own bounds over the draws, one division more
        keep = bd[f"{e}_keep"]
        gap = np.abs(got[f"{k}_mean"] - want[f"{k}_mean"])[keep]
        assert (gap <= bd[f"{e}_sum"][keep] / 6 + B.EPS * np.abs(want[f"{k}_mean"][keep])).all(), k
    assert abs(got["corr_mean"] - want["corr_mean"]) <= bd["corr"][0] / 6 + B.EPS
    assert np.isfinite(got["y_of_x_sd"]).all() and np.isfinite(got["corr_sd"])


def same(a, b, path):
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            same(a[k], b[k], path + (k,))
    elif a is None:
        assert b is None, path
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), path


@pytest.mark.parametrize("case", ["fast_all", "reference"])
def test_chain_untouched_and_repeatable(handle, case):
    """gpirtMCMC(..., equate=...) against the same call without: theta, beta, f, the IRFs, R's stream position and the results
    of sumscore, shape and ppc bit-identical; a second run gives byte-identical equating accumulators; one chain under R's
    stream is bit for bit the stage API's state over the same chain"""
    from gpirt_amd import Sampler, gpirtMCMC
    from gpirt_amd.ops import RStream
    m, S, Bn = 31, 5, 2
    y, th0 = responses(m, seed=31)
    fx, fy = chain_forms(y.shape[1])
    kw = dict(vote_codes=CODES, theta_init=th0)
    seeds = [None, None, None]
    if case == "fast_all":
        kw.update(preset="fast", seed=9, chains=2, theta_init=None, summaries=("waic",), quantiles=(0.025, 0.5, 0.975),
                  ppc=True, ranks=True, shape=True, sumscore=True)
    else:
        seeds = [RStream(77), RStream(77), RStream(77)]
        kw.update(sumscore=True)
    res = []
    for k, on in enumerate((None, dict(x=fx, y=fy), dict(x=fx, y=fy))):
        extra = dict(rstream=seeds[k]) if seeds[k] is not None else {}
        res.append(gpirtMCMC(y, S, Bn, equate=on, **kw, **extra))
    plain, with_eq, again = res
    assert "equate" not in plain and "equate" in with_eq
    for k in ("theta", "beta", "f", "IRFs"):
        assert np.array_equal(plain[k], with_eq[k], equal_nan=True), k
    for block in ("sumscore",) + (("summary", "quantiles", "ppc", "ranks", "shape") if case == "fast_all" else ()):
        same(plain[block], with_eq[block], (block,))
    eq = with_eq["equate"]
    C_ = 2 if case == "fast_all" else 1
    assert eq["draws"] + eq["skipped"] == C_ * S and eq["Mx"] == len(fx) and eq["My"] == len(fy)
    for k in RAW:
        assert eq[k].tobytes() == again["equate"][k].tobytes(), k
    if case == "fast_all":
        return                                  # (several chains against the stage API: test_chains_pool)
    (mt0, i0), (mt1, i1) = seeds[0].state(), seeds[1].state()
    assert i0 == i1 and np.array_equal(mt0, mt1)
    s = Sampler(handle, y, th0, rng="reference", rstream=RStream(77), theta_stabilise=False)
    s.init()
    s.equate_enable(fx, fy)
    for it in range(S + Bn):
        s.step()
        if it >= Bn:
            s.equate_accumulate()
    s.check()
    stage = s.equate()
    s.close()
    for k in RAW + DERIVED:
        assert np.array_equal(np.asarray(eq[k]), np.asarray(stage[k]), equal_nan=True), k


def test_chains_pool(handle):
    """chains=3, chain 1 started at -theta0: res["equate"] equals equate.combine of the three chains' state blocks bit for bit
    -- there are no signs, a reflected chain enters unchanged --, and lies within the bounds of from_draws over the three chains"""
    from gpirt_amd import Sampler, _lib, equate, gpirtMCMC
    m, S, Bn, seed = 33, 4, 2, 29
    y, th0 = responses(m, seed=11)
    inits = np.stack([th0, -th0, 0.5 * th0])
    fx, fy = list(range(2, 14)), list(range(15, 30))
    cuts = ((6, 8),)
    res = gpirtMCMC(y, S, Bn, vote_codes=CODES, theta_init=inits, rng="item", seed=seed, theta_stabilise=True, chains=3,
                    align=True, equate=dict(x=fx, y=fy, cuts=cuts), store_draws=False)
    samplers, draws = [], []
    for c in range(3):
        s = Sampler(handle, y, inits[c], rng="item", seed=_lib.chain_seed(seed, c), theta_stabilise=True)
        s.init()
        s.equate_enable(fx, fy)
        ch = []
        for it in range(S + Bn):
            s.step()
            if it >= Bn:
                s.equate_accumulate()
                ch.append(s.get("fstar"))
        s.check()
        samplers.append(s)
        draws.append(np.stack(ch))
    pooled = equate.combine(handle, samplers, cuts=cuts)
    for k in RAW + DERIVED + ("y_of_x_mean", "x_of_y_sd"):
        assert np.array_equal(np.asarray(pooled[k]), np.asarray(res["equate"][k]), equal_nan=True), k
    assert pooled["corr_mean"] == res["equate"]["corr_mean"] and pooled["draws"] == 3 * S
    flat = [f for ch in draws for f in ch]
    want = equate.from_draws(draws, fx, fy, cuts=cuts)
    singles = [equate.from_draws(f[None], fx, fy) for f in flat]
    B.check(pooled, want, singles, "chains=3", quarter=False)
    for k in RAW:                                             # the last_* arrays are the last state's
        if k.startswith("last_") or k == "corr_terms":
            assert np.array_equal(pooled[k], samplers[2].equate_get(k)), k
    other = Sampler(handle, y, th0, preset="fast", seed=1)
    other.init()
    other.equate_enable(fx[1:], fy)
    samplers.append(other)
    with pytest.raises(_lib.GpirtError, match="other forms"):
        equate.combine(handle, [samplers[0], other])
    for s in samplers:
        s.close()


def test_refusals(handle):
    from gpirt_amd import _lib, gpirtMCMC
    from gpirt_amd.distributed import ShardedSampler
    y, th0 = responses(6)
    s = new_sampler(handle, 6)
    for call in (s.equate_accumulate, s.equate_state, lambda: s.equate_get("corr")):
        with pytest.raises(_lib.GpirtError, match="not enabled"):
            call()
    for fx, fy, word in (([], [1], "empty"), ([0, 1], [1, 2], "column 1 is in both"), ([6], [1], "outside"), ([0], None, "missing")):
        with pytest.raises(ValueError, match=word):
            s.equate_enable(fx, fy)
        with pytest.raises(ValueError, match=word):
            gpirtMCMC(y, 2, 1, vote_codes=CODES, preset="fast", equate=dict(x=fx, y=fy))
    with pytest.raises(ValueError, match="unknown keys"):
        gpirtMCMC(y, 2, 1, vote_codes=CODES, preset="fast", equate=dict(x=[0], y=[1], items=[2]))
    with pytest.raises(ValueError, match="cy <= 1"):
        gpirtMCMC(y, 2, 1, vote_codes=CODES, preset="fast", equate=dict(x=[0], y=[1], cuts=((1, 2),)))
    a, b, none = np.array([1, 1, 0, 0, 0, 0], dtype=np.uint8), np.array([0, 1, 1, 0, 0, 0], dtype=np.uint8), np.zeros(6, dtype=np.uint8)
    ptr = lambda v: v.ctypes.data                             # noqa: E731
    assert s.lib.gpirt_sampler_equate_enable(s._s, ptr(a), ptr(b), 1) == _lib.E_ARG and "column 1 is in both" in _lib.last_error()
    assert s.lib.gpirt_sampler_equate_enable(s._s, ptr(a), ptr(none), 1) == _lib.E_ARG and "form y is empty" in _lib.last_error()
    assert s.lib.gpirt_sampler_equate_enable(s._s, ptr(a), None, 1) == _lib.E_ARG
    s.equate_enable([0, 1], [2])
    with pytest.raises(_lib.GpirtError, match="unknown equate field"):
        s.equate_get("nope")
    assert s.lib.gpirt_sampler_equate_enable(s._s, ptr(a), ptr(b), 1) == _lib.E_ARG          # refused: the old state is kept
    assert s.equate_get("counts").tolist() == [0, 0, 0, 0, 0] and s.equate_get("mask_y").tolist() == [0, 0, 1, 0, 0, 0]
    s.equate_enable(on=False)
    with pytest.raises(_lib.GpirtError, match="not enabled"):
        s.equate_state()
    s.close()
    with pytest.raises(ValueError, match="not offered for item shards"):
        ShardedSampler.equate_enable(None)
