"""Ordinal responses on the device (include/gpirt_hip.h "ordinal (graded) responses", csrc/ordinal.hip, csrc/sampler.hip) against
gpirt_amd/ordinal.py in long double under the bounds of tests/_ordinal_bounds.py.

The shapes are the smallest at which the layout can go wrong: n = 255, 256, 257 (the 256-thread loop edge), 2049 and 8193 (the
first sizes of the second and third size class), m = 3 and 5, C = 2, 3, 5, 8, about 10 % missing cells, one item with a category
nobody chose, one item whose every answer is the same category, one respondent with no answer (tests/_ordinal_bounds.py
make_case)."""
import numpy as np
import pytest

import _ordinal_bounds as OB

pytestmark = pytest.mark.gpu
LD = np.longdouble


def _sampler(handle, cat, seed, C, K=None, preset="fast", **kw):
    from gpirt_amd import ordinal as OR
    from gpirt_amd.sampler import Sampler
    s = Sampler(handle, OR.dichotomise(cat), OB.theta_start(cat.shape[0], seed), seed=seed, preset=preset)
    s.init()
    if C:
        s.ordinal_enable(cat, C, K0=K, **kw)
    return s


# ------------------------------------------------------------------------------------------------ the binary anchor ---
@pytest.mark.parametrize("screen", [1, 2], ids=["screen", "full"])
@pytest.mark.parametrize("n,m", [(257, 5), (2049, 3), (8193, 3)])
def test_two_categories_at_the_centre_are_the_binary_slice_bit_for_bit(handle, n, m, screen):
    from gpirt_amd.sampler import Sampler
    cat, t, _ = OB.make_case(n, m, 2, 100 + n)
    y = np.asfortranarray(np.where(cat == 0, np.nan, np.where(cat == 2, 1.0, -1.0)))
    th0 = OB.theta_start(n, 100 + n)
    with handle.config("GPIRT_ESS_SCREEN", screen):
        a = Sampler(handle, y, th0, seed=5, preset="fast")
        a.init()
        a.ordinal_enable(cat, 2, K0=np.full((m, 1), 120, dtype=np.int32))
        assert np.all(a.ordinal_get("thresholds") == 0.0) and np.all(a.get("beta")[0] == 0.0)
        b = Sampler(handle, y, th0, seed=5, preset="fast")
        b.init()
        for name in ("beta", "mu", "mu_star"):
            b.set(name, a.get(name))
        assert a.get("f").tobytes() == b.get("f").tobytes()
        a.draw_f()
        b.draw_f()
        a.check(); b.check()
        assert a.get("f").tobytes() == b.get("f").tobytes()
        assert np.array_equal(a.get("ess_k"), b.get("ess_k"))
        a.close(); b.close()


# ------------------------------------------------------------------------------------------- the slice, long double ---
@pytest.mark.parametrize("n,m,C,seed", [(255, 3, 3, 31), (256, 3, 5, 32), (257, 3, 8, 33), (2049, 3, 5, 34), (8193, 3, 3, 35)])
def test_slice_decisions_against_long_double(handle, n, m, C, seed):
    """Every accept / reject decision of draw_f replayed in long double from the same f, nu (read back: nu = L Z is the
    device's), mu, thresholds and uniforms.  A decision is decided when the long-double margin exceeds the derived band; every
    decided one must agree (the item's rejection count up to its first undecided trial), at most 1 in 100 may be undecided, and
    f' is f cos + nu sin to the bit for one (c, s) within an ulp of NumPy's at the accepted angle."""
    from gpirt_amd import ordinal as OR
    from gpirt_amd.ppc import item_uniform
    case = OB.slice_case(n, m, C, seed)
    s = _sampler(handle, case["cat"], seed, C, case["K"])
    s.set("f", case["f"]); s.set("mu", case["mu"])
    s.draw_f()
    s.check()
    f1, nu, k_dev = s.get("f"), s.get("nu"), s.get("ess_k")
    total = undecided = 0
    for j in range(m):
        u = np.asarray(item_uniform(seed, 1, 4, np.uint64(j), np.arange(400, dtype=np.uint64)))
        b = case["t"][case["K"][j]]
        cj, fj, mj = case["cat"][:, j], case["f"][:, j], case["mu"][:, j]
        res = OR.slice_exact(cj, fj, nu[:, j], mj, b, u)
        clean = True
        for eps, mg in zip(res["eps"], res["margins"]):
            band = OB.slice_bound(cj, fj, nu[:, j], mj, b, eps, res["ll0"], np.log(u[0]))
            total += 1
            if abs(float(mg)) <= band:
                undecided += 1
                clean = False
                break
        if not clean:
            continue
        assert k_dev[j] == res["k"], (j, k_dev[j], res["k"])
        eps = res["eps"][-1]
        hit = False
        for c in (np.nextafter(np.cos(eps), -2), np.cos(eps), np.nextafter(np.cos(eps), 2)):
            for sn in (np.nextafter(np.sin(eps), -2), np.sin(eps), np.nextafter(np.sin(eps), 2)):
                hit = hit or np.array_equal(fj * c + nu[:, j] * sn, f1[:, j])
        assert hit, j
    assert total >= m and undecided * 100 <= total, (undecided, total)
    s.close()


# ------------------------------------------------------------------------------------------------ the theta product ---
@pytest.mark.parametrize("n,m,C,seed", [(257, 5, 5, 41), (256, 3, 2, 42), (255, 3, 8, 43), (2049, 3, 3, 44)])
def test_theta_product_against_long_double(handle, n, m, C, seed):
    from gpirt_amd import ordinal as OR
    case = OB.slice_case(n, m, C, seed)
    cat = case["cat"]
    s = _sampler(handle, cat, seed, C, case["K"])
    rng = np.random.default_rng(seed)
    grid = -5.0 + 0.01 * np.arange(1001)
    fstar = np.asfortranarray(np.outer(grid, case["slopes"]) + 0.3 * rng.standard_normal((1001, m)))
    fstar[10, 0], fstar[11, 1] = 800.0, -800.0                    # beyond exp()'s range: the fast term stays finite
    miss = int(np.argmax(cat[:, 2] == 0))                         # a respondent who did not answer item 2 ...
    obs = int(np.argmax(cat[:, 2] > 0))                           # ... and one who did
    fstar[20, 2], fstar[21, 2] = np.nan, np.inf
    s.set("fstar", fstar)
    s.theta_partial()
    lp = s.get("logpost")
    B = case["t"][case["K"]]
    clean = fstar.copy()
    want = OR.theta_logpost_exact(cat, np.where(np.isfinite(clean), clean, 0.0), B)
    bound = OB.theta_bound(cat, np.where(np.isfinite(clean), clean, 0.0), B)
    rows = np.ones(1001, dtype=bool)
    rows[[20, 21]] = False
    assert np.all(np.isfinite(lp[rows]))
    assert np.all(np.abs(lp[rows].astype(LD) - want[rows]) <= bound[rows] + 1e-300)
    # a NaN f* is not seen by a respondent whose answer to that item is missing, and poisons the one who answered; an infinite
    # one likewise, where it shows as the product's stand-in for -inf or costs nothing (the category it agrees with)
    others = [j for j in range(m) if j != 2]
    part = OR.theta_logpost_exact(cat[:, others], fstar[:, others], B[others])
    pb = OB.theta_bound(cat[:, others], fstar[:, others], B[others])
    gone = cat[:, 2] == 0
    for row in (20, 21):
        assert np.all(np.abs(lp[row, gone].astype(LD) - part[row, gone]) <= pb[row, gone] + 1e-300)
    assert np.isfinite(lp[20, miss]) and np.all(np.isnan(lp[20, ~gone])) and np.isnan(lp[20, obs])
    top = cat[:, 2] == C
    assert np.all(lp[21, ~gone & ~top] <= -1e300)
    assert np.all(np.abs(lp[21, top].astype(LD) - part[21, top]) <= pb[21, top] + 1e-300)
    assert cat[1].max() == 0 and np.all(lp[rows][:, 1] == 0.0)    # the respondent with no answer: an exact zero
    # theta_finish on the finite part: the draw is compared wherever u lies farther from a CDF step than the bound
    fstar[20, 2] = fstar[21, 2] = 0.0
    s.set("fstar", fstar)
    s.theta_partial()
    lp = s.get("logpost")
    s.theta_finish()
    theta = s.get("theta")
    from gpirt_amd.ppc import item_uniform
    want = OR.theta_logpost_exact(cat, fstar, B)
    bound = OB.theta_bound(cat, fstar, B)
    ts = grid.astype(LD)
    prior = -(LD(0.918938533204672741780329736406) + LD(0.5) * ts * ts)
    decided = 0
    for i in range(n):
        P = prior + want[:, i]
        e = np.exp(P - P.max())
        cdf = (np.cumsum(e) - e[0]) / (e.sum() - e[0])
        u = float(item_uniform(seed, 1, 6, np.uint64(i), np.uint64(0)))
        # the relative error of every CDF value: the log-posterior's bound (it enters through exp) and 1001 additions
        tol = 2.0 * float(2 * bound[:, i].max() + 1100 * OB.U)
        k = int(np.argmax(cdf > u))
        if np.min(np.abs(cdf - u)) <= tol:
            continue
        decided += 1
        assert theta[i] == -5.0 + 0.01 * k, (i, theta[i], k)
    assert decided >= 0.9 * n
    s.close()


# ---------------------------------------------------------------------------------------------------- the slope -------
@pytest.mark.parametrize("n,m,C,seed", [(257, 5, 5, 51), (256, 3, 3, 52), (2049, 3, 8, 53)])
def test_slope_update_against_long_double(handle, n, m, C, seed):
    from gpirt_amd import ordinal as OR
    from gpirt_amd.ppc import item_uniform
    case = OB.slice_case(n, m, C, seed)
    cat = case["cat"]
    s = _sampler(handle, cat, seed, C, case["K"])
    f = case["f"].copy()
    f[7:9, :] = 0.5                                              # (keep the sums of unit size: the decision then depends on the slope)
    s.set("f", f)
    beta0 = s.get("beta")
    assert np.all(beta0[0] == 0.0)
    theta = s.get("theta")
    s.draw_beta()
    beta1 = s.get("beta")                                         # (get joins a deferred draw_beta)
    assert np.all(beta1[0] == 0.0)
    assert np.array_equal(s.get("mu"), 0.0 + theta[:, None] * beta1[1][None, :])
    assert np.array_equal(s.get("mu_star"), 0.0 + (-5.0 + np.arange(1001) * 0.01)[:, None] * beta1[1][None, :])
    decided = 0
    for j in range(m):
        un, ud = (float(item_uniform(seed, 1, 7, np.uint64(j), np.uint64(k))) for k in (2, 3))
        res = OR.beta_exact(cat[:, j], f[:, j], theta, beta0[1, j], case["t"][case["K"][j]], 0.1, 0.0, 3.0, un, ud)
        band = OB.beta_bound(cat[:, j], f[:, j], theta, 0.0, beta0[1, j], res["proposal"], case["t"][case["K"][j]],
                             (res["ll_prop"], res["ll_cur"], np.log(ud), 20.0))
        if abs(float(res["margin"])) <= band:
            continue
        decided += 1
        assert beta1[1, j] == (res["proposal"] if res["accept"] else beta0[1, j]), j
    assert decided >= m - 1
    s.close()


# -------------------------------------------------------------------------------------------------- the thresholds ----
def _compare_update(s, cat, g, t, pr, K, seed, call, W):
    """One draw_thresholds against thresholds_exact: the lp masses within the derived bound (csrc/ordinal.hip states that they are
    not bit-equal to NumPy's: the device's exp), the windows exactly, the drawn index where decided.  An undecided draw that
    went the other way ends the comparison of THAT item's later thresholds (they see another left neighbour); the other items
    are compared in full.  Returns the statement's result and the counts (draws, undecided draws) for the caller's cap."""
    from gpirt_amd import ordinal as OR
    m, R = K.shape
    want = OR.thresholds_exact(cat, g, t, pr, K, seed, call, W)
    lp, win, idx = s.ordinal_get("lp"), s.ordinal_get("window"), s.ordinal_get("index")
    Kj = K.astype(np.int64).copy()
    draws = undecided = 0
    for j in range(m):
        agree = True
        for c in range(1, R + 1):
            if not agree:
                break
            assert win[j, c - 1] == want["window"][j, c - 1], (j, c)
            row = want["lp"][j, c - 1]
            cand = row > -np.inf
            assert np.array_equal(np.isneginf(lp[j, c - 1]), ~cand), (j, c)
            bound = OB.lp_bound(cat[:, j], g[:, j], t, pr, Kj[j], c, int(win[j, c - 1]), W)
            assert np.all(np.abs(lp[j, c - 1][cand].astype(LD) - row[cand]) <= bound[cand] + 1e-300), (j, c)
            # decided: u1 farther from every step of the CDF than the masses' bound allows the steps to move
            if want["margin"][j, c - 1] > 4.0 * bound.max() + 64 * OB.U:
                assert idx[j, c - 1] == want["index"][j, c - 1], (j, c)
                Kj[j, c - 1] = idx[j, c - 1]
            elif np.isfinite(float(want["margin"][j, c - 1])):
                undecided += 1
                agree = idx[j, c - 1] == want["index"][j, c - 1]
                Kj[j, c - 1] = idx[j, c - 1]
            draws += int(np.isfinite(float(want["margin"][j, c - 1])))
    assert np.all(np.diff(idx, axis=1) > 0) if R > 1 else True
    return want, draws, undecided


@pytest.mark.parametrize("n,m,C,seed,W", [(255, 3, 2, 61, 16), (256, 3, 3, 62, 16), (257, 5, 5, 63, 16), (257, 3, 8, 64, 5),
                                          (2049, 3, 5, 65, 64), (8193, 3, 3, 66, 16)])
def test_threshold_update_against_long_double(handle, n, m, C, seed, W):
    from gpirt_amd import ordinal as OR
    case = OB.slice_case(n, m, C, seed)
    cat, t = case["cat"], case["t"]
    f = case["f"].copy()
    f[5:9, :] = 0.25
    s = _sampler(handle, cat, seed, C, case["K"], width=W)
    s.set("f", f)
    g = f + s.get("mu")
    pr = OR.default_log_prior(t)
    K = case["K"].copy()
    counts = s.ordinal_get("counts")
    assert np.array_equal(counts, np.stack([(cat == c).sum(axis=0) for c in range(1, C + 1)], axis=1))
    draws = undecided = 0
    for call in (1, 2):
        s.draw_thresholds()
        want, d, u = _compare_update(s, cat, g, t, pr, K, seed, call, W)
        draws, undecided = draws + d, undecided + u
        K = s.ordinal_get("index")
        assert np.array_equal(s.ordinal_get("thresholds"), t[K])
        assert want["failed"] == 0 and s.ordinal_get("failed") == 0
    st = s.ordinal_stats()
    assert st["calls"] == 2 and st["updates"] + st["pinned"] == 2 * m * (C - 1) and st["width"] == W == st["lp_width"]
    assert draws == st["updates"] and undecided * 100 <= draws, (undecided, draws)      # the slice test's cap
    # "lp" keeps the layout of the update that wrote it when the width changes, and takes the new one with the next update
    lp = s.ordinal_get("lp")
    s.ordinal_width(3)
    assert s.ordinal_stats()["width"] == 3 and s.ordinal_stats()["lp_width"] == W
    assert np.array_equal(s.ordinal_get("lp"), lp)
    s.draw_thresholds()
    assert s.ordinal_stats()["lp_width"] == 3 and s.ordinal_get("lp").shape == (m, C - 1, 3)
    _compare_update(s, cat, g, t, pr, K, seed, 3, 3)
    s.close()


def test_threshold_update_constructed_states(handle):
    """Neighbours adjacent (pinned, state unchanged), the window cut by the left neighbour, by the right one and by both grid
    ends (P = 9 with W = 64), an empty category, and a NaN in g at an observed row (failed; the item's later thresholds keep
    their bytes)."""
    from gpirt_amd import ordinal as OR
    n, m, C, seed = 257, 5, 4, 71
    cat, _, _ = OB.make_case(n, m, C, seed)
    assert (cat[:, m - 1] == 2).sum() == 0 and (cat[:, 0] < C).sum() == (cat[:, 0] == 0).sum()
    t = OR.grid(6.0, 241)
    K = np.array([[100, 101, 102], [50, 120, 121], [119, 120, 200], [0, 120, 240], [60, 120, 180]], dtype=np.int32)
    s = _sampler(handle, cat, seed, C, K, width=16)
    g = s.get("f") + s.get("mu")
    pr = OR.default_log_prior(t)
    s.draw_thresholds()
    want, draws, undecided = _compare_update(s, cat, g, t, pr, K, seed, 1, 16)
    assert undecided == 0 and draws == want["updates"]
    idx = s.ordinal_get("index")
    assert idx[0, 1] == 101                                      # both neighbours adjacent: one candidate
    assert s.ordinal_get("pinned") == want["pinned"] >= 1
    lp = s.ordinal_get("lp")
    assert lp[0, 1][101 - s.ordinal_get("window")[0, 1]] == 0.0 and np.isneginf(lp[0, 1]).sum() == 15
    s.close()
    # both grid ends inside the window
    t9 = OR.grid(6.0, 9)
    K9 = np.tile(np.array([[2, 4, 6]], dtype=np.int32), (m, 1))
    s = _sampler(handle, cat, seed, C, K9, points=9, width=64)
    s.draw_thresholds()
    assert _compare_update(s, cat, s.get("f") + s.get("mu"), t9, OR.default_log_prior(t9), K9, seed, 1, 64)[2] == 0
    assert s.ordinal_get("index").min() >= 0 and s.ordinal_get("index").max() <= 8
    s.close()
    # a NaN in g at an observed row of category 2 of item 1: threshold 1 (categories 1 | 2) fails, 2 and 3 keep their bytes
    s = _sampler(handle, cat, seed, C, K, width=16)
    f = s.get("f")
    row = int(np.argmax(cat[:, 1] == 2))
    f[row, 1] = np.nan
    s.set("f", f)
    s.draw_thresholds()
    idx = s.ordinal_get("index")
    assert s.ordinal_get("failed") == 1 and np.array_equal(idx[1], K[1])
    assert np.array_equal(s.ordinal_get("thresholds")[1], t[K[1]])
    assert np.all(np.diff(idx, axis=1) > 0)
    s.close()


# ------------------------------------------------------------------------------------------------------ as it was ----
@pytest.mark.parametrize("opts", [dict(preset="fast"), dict(rng="item")], ids=["fast", "default"])
def test_a_sampler_without_ordinal_is_what_it_was_and_ordinal_runs_repeat(handle, opts):
    from gpirt_amd import ordinal as OR
    from gpirt_amd.sampler import Sampler
    n, m, C = 257, 5, 5
    cat, t, K = OB.make_case(n, m, C, 81)
    y, th0 = OR.dichotomise(cat), OB.theta_start(n, 81)
    plain, ordinal = [], []
    for kind in ("plain", "plain", "ordinal", "ordinal"):
        s = Sampler(handle, y, th0, seed=9, **opts)
        s.init()
        if kind == "ordinal":
            s.ordinal_enable(cat, C, K0=K, planned_draws=5)
        for _ in range(5):
            s.step()
            if kind == "ordinal":
                s.draw_thresholds()
                s.ordinal_record()
        s.check()
        state = {k: s.get(k).tobytes() for k in ("theta", "beta", "f", "fstar")}
        if kind == "ordinal":
            state.update({k: s.ordinal_get(k).tobytes() for k in ("index", "thresholds", "lp", "window", "draws", "hist")})
            ordinal.append(state)
        else:
            plain.append(state)
        s.close()
    assert plain[0] == plain[1]
    assert ordinal[0] == ordinal[1]
    assert ordinal[0]["theta"] != plain[0]["theta"]


def test_ordinal_turned_off_again_is_the_binary_chain(handle):
    """Enable, one ordinal step, off again: from there the sampler runs the binary kernels -- five steps give the bytes of a
    plain sampler started from the same state (the intercepts stay at the 0 the enable pinned them to)."""
    from gpirt_amd import ordinal as OR
    from gpirt_amd.sampler import Sampler
    n, m, C = 257, 5, 5
    cat, t, K = OB.make_case(n, m, C, 82)
    y, th0 = OR.dichotomise(cat), OB.theta_start(n, 82)
    a = Sampler(handle, y, th0, seed=9, preset="fast")
    a.init()
    a.ordinal_enable(cat, C, K0=K)
    a.step()
    a.draw_thresholds()
    a.ordinal_enable(None)
    assert not a.ordinal_stats()["on"] and np.all(a.get("beta")[0] == 0.0)
    b = Sampler(handle, y, th0, seed=9, preset="fast")
    b.init()
    b.step()                                                      # (the same iteration count: it keys every uniform)
    for name in ("theta", "beta", "f", "fstar", "mu", "mu_star"):
        b.set(name, a.get(name))
    a.set("theta", a.get("theta"))                                # (both then factor K(theta) anew, as a set theta asks)
    a.factor(); b.factor()
    for _ in range(5):
        a.step(); b.step()
    a.check(); b.check()
    for name in ("theta", "beta", "f", "fstar"):
        assert a.get(name).tobytes() == b.get(name).tobytes(), name
    assert np.any(a.get("beta")[0] != 0.0)                        # the binary draw_beta moves the intercept again
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------ refusals -----
def test_refusals_name_their_reason(handle):
    from gpirt_amd import ordinal as OR
    from gpirt_amd._lib import GpirtError
    from gpirt_amd.sampler import Sampler
    n, m, C = 64, 4, 3
    cat, t, K = OB.make_case(n, m, C, 91)
    y, th0 = OR.dichotomise(cat), OB.theta_start(n, 91)
    s = Sampler(handle, y, th0, seed=3, preset="fast")
    with pytest.raises(GpirtError, match="needs an initialised sampler"):
        s.ordinal_enable(cat, C)
    s.init()
    for name in ("draw_thresholds", "ordinal_record", "ordinal_accumulate_irf"):
        with pytest.raises(GpirtError, match="ordinal responses are not enabled"):
            getattr(s, name)()
    bad = cat.copy(); bad[0, 0] = 4
    with pytest.raises(GpirtError, match=r"cat\[0, 0\] = 4"):
        s.ordinal_enable(bad, C)
    yb = cat.copy(); yb[np.argmax(cat[:, 1] > 0), 1] = 0
    with pytest.raises(GpirtError, match="NaN exactly where cat is 0"):
        s.ordinal_enable(yb, C)
    for kw, msg in ((dict(points=240), "must be odd"), (dict(hi=0.0), r"hi = 0"), (dict(width=65), "W = 65"),
                    (dict(K0=np.tile([[5, 5]], (m, 1))), "not strictly increasing"), (dict(C=9), "C = 9"),
                    (dict(log_prior=np.full(241, np.nan)), "not finite")):
        with pytest.raises(GpirtError, match=msg):
            s.ordinal_enable(cat, **({"C": C} | kw))
    # each analysis block on the binary side refuses ordinal_enable while it is on ...
    blocks = [("the summaries' WAIC", lambda: s.summary_enable(_sum_waic()), lambda: s.summary_enable(0)),
              ("posterior predictive checks", lambda: s.ppc_enable(), lambda: s.ppc_enable(False)),
              ("PSIS-LOO", lambda: s.loo_enable(200), lambda: s.loo_enable(on=False)),
              ("group posteriors", lambda: s.groups_enable(np.arange(n) % 2), lambda: s.groups_enable(on=False)),
              ("score equating", lambda: s.equate_enable(np.arange(m) < 2, np.arange(m) >= 2), lambda: s.equate_enable(on=False)),
              ("ACF's log-likelihood series", lambda: s.acf_enable(_acf_ll(), 10), lambda: s.acf_enable(on=False)),
              ("sum-score", lambda: s.sumscore_enable(), lambda: s.sumscore_enable(on=False)),
              ("scoring", lambda: s.score_enable(y[:2]), lambda: s.score_enable(None))]
    for what, on, off in blocks:
        on()
        with pytest.raises(GpirtError, match="is refused while .*" + what):
            s.ordinal_enable(cat, C)
        off()
    s.ordinal_enable(cat, C, K0=K)
    assert s.ordinal_stats()["on"] and np.all(s.get("beta")[0] == 0.0)
    # ... and is refused once it is on, with everything else that evaluates the binary likelihood or moves the intercept
    why = "is refused while ordinal responses are on"
    for call in (lambda: s.summary_enable(_sum_waic()), s.ppc_enable, lambda: s.loo_enable(200), s.sumscore_enable,
                 lambda: s.score_enable(y[:2]), lambda: s.groups_enable(np.arange(n) % 2), lambda: s.acf_enable(_acf_ll(), 10),
                 lambda: s.equate_enable(np.arange(m) < 2, np.arange(m) >= 2), s.draw_beta_centred, s.draw_amp_centred,
                 lambda: s.draw_scale("scale"), s.draw_ell, s.draw_amp):
        with pytest.raises(GpirtError, match=why):
            call()
    half = np.arange(n) % 2
    for call in (s.ppc_pairs_enable, s.ppc_bins_enable, lambda: s.ppc_dif_enable(half), lambda: s.ppc_scores_enable(groups=2),
                 lambda: s.ppc_person_enable(groups=2), s.ppc_resid_enable, s.score_predict_enable,
                 lambda: s.step(consistent=True, scale="scale"), lambda: s.step(consistent=True, scale=("scale", "shift"))):
        with pytest.raises(GpirtError, match=why + ": it evaluates the binary likelihood of y"):
            call()
    with pytest.raises(GpirtError, match="set_theta_block " + why + ": the respondent-block theta path has no one-hot product"):
        s.set_theta_block(y[:8], 0, m)
    with pytest.raises(GpirtError, match=r'gpirt_sampler_set\("y"\) ' + why):
        s.set("y", y)
    moved = s.get("beta")
    s.set("beta", moved)                                          # the pinned intercepts as they are: allowed
    moved[0, 1] = 0.25
    with pytest.raises(GpirtError, match="non-zero intercept " + why + ": the intercept is pinned at 0"):
        s.set("beta", moved)
    other = Sampler(handle, y, th0, seed=4, preset="fast")
    other.init()
    for dst, src in ((other, s), (s, other)):
        with pytest.raises(GpirtError, match="copy_state is refused while ordinal responses are on"):
            dst.copy_state_from(src)
    # ... ordinal_enable while a theta block is set, and under GPIRT_LL_EXACT=1
    other.set_theta_block(y[:8], 0, m)
    with pytest.raises(GpirtError, match="is refused while gpirt_sampler_set_theta_block is in use"):
        other.ordinal_enable(cat, C)
    other.close()
    with handle.config("GPIRT_LL_EXACT", 1):
        with pytest.raises(GpirtError, match="is refused under GPIRT_LL_EXACT=1: the ordinal kernels have the fast term alone"):
            _enable_fresh(handle, y, th0, cat, C)
    s.step(consistent=True)                                       # the carry does not read y: allowed
    s.draw_thresholds()
    s.check()
    s.ordinal_width(7)
    with pytest.raises(GpirtError, match="W = 0"):
        s.ordinal_width(0)
    with pytest.raises(GpirtError, match="all 0 planned draws are recorded"):
        s.ordinal_record()
    s.close()
    from gpirt_amd.ops import RStream
    rs = RStream(7)
    r = Sampler(handle, y, rs.rnorm(n), rng="reference", rstream=rs, theta_stabilise=False)
    r.init()
    with pytest.raises(GpirtError, match="R's stream has no such draw"):
        r.ordinal_enable(cat, C)
    r.close()
    sh = Sampler(handle, y, th0, seed=3, preset="fast", item0=0, m_total=2 * m)
    sh.init()
    with pytest.raises(GpirtError, match="an item shard"):
        sh.ordinal_enable(cat, C)
    sh.close()


def _enable_fresh(handle, y, th0, cat, C):
    from gpirt_amd.sampler import Sampler
    s = Sampler(handle, y, th0, seed=4, preset="fast")
    try:
        s.init()
        s.ordinal_enable(cat, C)
    finally:
        s.close()


def test_more_than_16384_respondents_are_refused_at_enable(handle):
    from gpirt_amd._lib import GpirtError
    n = 16385
    cat = np.asfortranarray((1 + np.arange(n) % 3).astype(np.int8).reshape(n, 1))
    with pytest.raises(GpirtError, match="n = 16385 respondents is refused, the register-resident slice and threshold kernels"):
        _enable_fresh(handle, _dich(cat), OB.theta_start(n, 1), cat, 3)


def _dich(cat):
    from gpirt_amd import ordinal as OR
    return OR.dichotomise(cat)


def _sum_waic():
    from gpirt_amd import _lib
    return _lib.SUM_THETA_BETA | _lib.SUM_WAIC


def _acf_ll():
    from gpirt_amd import _lib
    return _lib.ACF_LL


# --------------------------------------------------------------------------------------------------------- a chain ----
def test_a_chain_recovers_theta_no_worse_than_the_dichotomised_run(handle):
    """512 x 24, C = 4, graded-response data from known theta, slopes and thresholds; 100 burn-in and 300 kept draws of step()
    then draw_thresholds().  No failed update, the order holds in every recorded draw, the histograms sum to the draw count, the
    curves are decreasing in c -- and the Fisher z of the correlation between theta's posterior mean and the generating theta is
    at least the binary sampler's on the dichotomised data minus 2 / sqrt(n - 3) (the sampling sd of z, doubled because the two
    runs share the data)."""
    from gpirt_amd import ordinal as OR
    from gpirt_amd.sampler import Sampler
    n, m, C, B, S = 512, 24, 4, 100, 300
    d = OR.make_graded(n, m, C, seed=2024)
    cat = d["cat"]
    y = OR.dichotomise(cat)
    th0 = OB.theta_start(n, 5)
    t = OR.grid()
    means = {}
    for kind in ("ordinal", "binary"):
        s = Sampler(handle, y, th0, seed=11, preset="fast")
        s.init()
        if kind == "ordinal":
            s.ordinal_enable(cat, C, K0=OR.init_thresholds(cat, t, C), planned_draws=S)
        acc = np.zeros(n)
        for it in range(B + S):
            s.step()
            if kind == "ordinal":
                s.draw_thresholds()
            if it >= B:
                acc += s.get("theta")
                if kind == "ordinal":
                    s.ordinal_record()
                    s.ordinal_accumulate_irf()
        s.check()
        means[kind] = acc / S
        if kind == "ordinal":
            st = s.ordinal_stats()
            assert st["failed"] == 0 and st["recorded"] == S and st["irf_draws"] == S and st["calls"] == B + S
            draws, hist = s.ordinal_get("draws"), s.ordinal_get("hist")
            assert draws.shape == (S, m, C - 1) and np.all(np.diff(draws, axis=2) > 0) and draws.min() >= 0 and draws.max() <= 240
            assert np.all(hist.sum(axis=2) == S)
            for j in range(m):
                for c in range(C - 1):
                    assert np.array_equal(hist[j, c], np.bincount(draws[:, j, c], minlength=241))
            cv = OR.curves(s.ordinal_get("cum"), S)
            assert np.all(np.diff(cv["exceed"], axis=1) <= 0) and cv["probs"].min() >= 0
            assert np.all(s.get("beta")[0] == 0.0)
            out = s.ordinal()
            assert out["mean"].shape == (m, C - 1) and np.all(np.diff(out["mean"], axis=1) > 0)
        s.close()
    z = {k: float(np.arctanh(abs(np.corrcoef(v, d["theta"])[0, 1]))) for k, v in means.items()}
    print("fisher z: ordinal %.4f binary %.4f margin %.4f" % (z["ordinal"], z["binary"], 2 / np.sqrt(n - 3)))
    assert z["ordinal"] >= z["binary"] - 2 / np.sqrt(n - 3), z


def test_run_is_the_one_call_way_in(handle):
    from gpirt_amd import ordinal as OR
    n, m, C, S, B = 96, 6, 3, 6, 4
    cat = OR.make_graded(n, m, C, seed=7)["cat"]
    res = OR.run(cat, S, B, chains=2, seed=3, handle=handle)
    assert res["theta"].shape == (2, S, n) and res["beta"].shape == (2, S, 2, m) and np.all(res["beta"][:, :, 0] == 0.0)
    d = res["threshold_draws"]
    assert d.shape == (2, S, m, C - 1) and np.all(np.diff(d, axis=3) > 0)
    assert res["thresholds"]["mean"].shape == (m, C - 1) and np.all(np.diff(res["thresholds"]["mean"], axis=1) > 0)
    assert np.all(res["hist"].sum(axis=2) == 2 * S) and all(c["failed"] == 0 for c in res["counters"])
    pr = res["curves"]["probs"]
    assert pr.shape == (m, C, 1001) and np.abs(pr.sum(axis=1) - 1).max() < 1e-12 and pr.min() >= 0
    assert res["categories"] == C and res["chains"] == 2 and np.array_equal(res["grid"], OR.grid())
    one = OR.run(cat, S, B, seed=3, handle=handle, consistent=True)
    assert one["theta"].shape == (S, n) and one["threshold_draws"].shape == (S, m, C - 1) and one["consistent"]
    assert np.array_equal(OR.run(cat, S, B, seed=3, handle=handle, consistent=True)["threshold_draws"], one["threshold_draws"])
