"""Scoring new respondents under ordinal responses on the device (include/gpirt_hip.h "scoring new respondents under ordinal
responses", csrc/ordinal_score.hip) against the NumPy statement gpirt_amd.ordinal.score_from_draws / predict_from_draws under the
bounds of tests/_ordinal_score_bounds.py: the stage API over a few draws, the C = 2 anchor against the binary scorer's statement,
constructed f*, the predictions and the next item, the untouched chain, repeatability, pooling, the refusals and ordinal.run.

The shapes (n, m, C, n_new): (100, 17, 3, 1) one respondent; (100, 3, 2, 65) the binary anchor, a second work-group; (257, 33, 5,
63); (300, 65, 8, 257) -- K = C m = 520 crosses the GEMM's K tiles, n_new = 257 the 4-respondents-per-group and 256 edges."""
import numpy as np
import pytest

import _ordinal_bounds as OB
import _ordinal_score_bounds as SB
from _score_bounds import delta_of as binary_delta_of

pytestmark = pytest.mark.gpu
EPS = SB.EPS
SHAPES = [(100, 17, 3, 1), (100, 3, 2, 65), (257, 33, 5, 63), (300, 65, 8, 257)]
RAW = ("draws", "nonfinite", "n_obs", "lpd_acc", "ll_sum", "post_sum")


def _sampler(handle, cat, C, seed, K0=None, fit=False):
    from gpirt_amd import Sampler
    from gpirt_amd import ordinal as OR
    s = Sampler(handle, OR.dichotomise(cat), OB.theta_start(cat.shape[0], 7), seed=seed, preset="fast")
    s.init()
    s.ordinal_enable(cat, C, K0=OR.init_thresholds(cat, OR.grid(), C) if K0 is None else K0)
    if fit:
        s.ordinal_fit_enable(("waic", "pred", "ppc"))
    return s


def _run(s, steps, thresholds=True, fit=False):
    f, B = [], []
    for _ in range(steps):
        s.step()
        if thresholds:
            s.draw_thresholds()
        if fit:
            s.ordinal_fit_accumulate()
        if getattr(s, "_oscore", (0,))[0]:
            s.ordinal_score_accumulate()
        f.append(s.get("fstar"))
        B.append(s.ordinal_get("thresholds"))
    s.check()
    return np.stack(f), np.stack(B)


_cache = {}


def _stage_case(handle, shape):
    """One run per shape, shared by the score and the predict test: 4 draws with predict on, top = 5"""
    if shape not in _cache:
        from gpirt_amd import ordinal as OR
        n, m, C, n_new = shape
        cat, _, _ = OB.make_case(n, m, C, 300 + m)
        cat_new = SB.make_new(n_new, m, C, 300 + m)
        s = _sampler(handle, cat, C, 41)
        s.ordinal_score_enable(cat_new, predict=True, top=5)
        f, B = _run(s, 4)
        got = s.ordinal_score()
        pred = s.ordinal_score_predict()
        hdr = (OR.score_state_header(s.ordinal_score_state()), OR.score_state_header(s.ordinal_score_predict_state()))
        T_last, wc_last = s.ordinal_score_get("product"), s.ordinal_score_get("wc")
        s.close()
        want = OR.score_from_draws(cat_new, f, B, return_products=True)
        wpred = OR.predict_from_draws(cat_new, f, B, top=5, return_draws=True)
        delta = SB.delta_of(cat_new, f, B, want["products"][0], want["wc"][0])
        _cache[shape] = dict(cat_new=cat_new, f=f, B=B, got=got, pred=pred, hdr=hdr, want=want, wpred=wpred, delta=delta,
                             T_last=T_last, wc_last=wc_last)
    return _cache[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stage_api_against_the_statement(handle, shape):
    n, m, C, n_new = shape
    c = _stage_case(handle, shape)
    got, want = c["got"], c["want"]
    assert c["hdr"][0] == dict(tag=0x5243534F, version=1, n_new=n_new, m=m, categories=C, N=1001)
    assert c["hdr"][1] == dict(tag=0x5250534F, version=1, n_new=n_new, m=m, categories=C, N=1001, pred_draws=4, pred_skipped=0)
    # the last draw's product and w term, entry by entry
    with np.errstate(invalid="ignore", over="ignore"):
        tb = np.asarray(OB.theta_bound(c["cat_new"], c["f"][-1], c["B"][-1]), dtype=np.float64)
    gap = np.abs(c["T_last"] - want["products"][0][-1])
    assert (gap <= tb + 1e-300).all(), f"product: worst ratio {float((gap / (tb + 1e-300)).max()):.3e}"
    wc = want["wc"][0][-1]
    assert (np.abs(c["wc_last"] - wc) <= (4 + m) * SB.U * np.abs(wc)).all()
    SB.compare_score(got, want, c["delta"], f"stage {shape}")
    for k in ("draws", "nonfinite", "n_obs"):
        assert np.array_equal(got[k], want[k])
    # the last respondent has no answers: the prior, lpd 0
    from gpirt_amd import score as SC
    pi = np.exp(SC.logprior()); pi /= pi.sum()
    assert got["n_obs"][-1] == 0 and np.abs(got["grid_post"][-1] - pi).max() <= 2 * 1001 * EPS * pi.max()
    assert abs(got["lpd"][-1]) <= 2 * 1001 * EPS


@pytest.mark.parametrize("shape", SHAPES + [(100, 9, 3, 20)], ids=lambda s: "x".join(map(str, s)))
def test_predict_and_next_items(handle, shape):
    """next_items is compared where the reference's compared ranks are further apart than twice the info bound.  With these seeds
    the NumPy statement alone leaves out no respondent at any shape.  Observed on the chain's own draws, the smallest compared-rank
    gap against the largest info bound: (100, 17, 3, 1) 8.4e-4 / 3.6e-12; (100, 3, 2, 65) 1.4e-3 / 3.1e-12; (257, 33, 5, 63) 4.3e-6 /
    1.2e-10; (300, 65, 8, 257) 4.2e-6 / 9.4e-10; (100, 9, 3, 20) 1.0e-3 / 6.8e-12 -- the nearest case keeps a factor 2000 over
    twice the bound.  Every run prints its own figures."""
    from gpirt_amd import ordinal as OR
    n, m, C, n_new = shape
    if shape in SHAPES:
        c = _stage_case(handle, shape)
        pred, want, delta, cat_new = c["pred"], c["wpred"], c["delta"], c["cat_new"]
    else:                                                  # top = 16 exceeds the unanswered items: the lists are padded with -1
        cat, _, _ = OB.make_case(n, m, C, 77)
        cat_new = SB.make_new(n_new, m, C, 77)
        s = _sampler(handle, cat, C, 43)
        s.ordinal_score_enable(cat_new, predict=True, top=16)
        f, B = _run(s, 4)
        pred = s.ordinal_score_predict()
        s.close()
        ws = OR.score_from_draws(cat_new, f, B, return_products=True)
        want = OR.predict_from_draws(cat_new, f, B, top=16, return_draws=True)
        delta = SB.delta_of(cat_new, f, B, ws["products"][0], ws["wc"][0])
        assert pred["next_items"].shape == (n_new, 16) and (pred["next_items"][:, m:] == -1).all()
        assert ((pred["next_items"] >= 0).sum(axis=1) == (cat_new == 0).sum(axis=1)).all()
    SB.compare_predict(pred, want, delta, cat_new, f"predict {shape}")
    assert (np.abs(pred["probs"].sum(axis=2) - 1.0) <= (C + 2) * 1001 * EPS).all()
    assert np.array_equal(pred["expected"], (pred["probs"] * np.arange(1, C + 1)).sum(axis=2))


def test_two_categories_against_the_binary_statement(handle):
    """C = 2 with K0 at the grid's centre (b = 0 exactly) and no draw_thresholds: the binary scorer's statement on y = 2 cat - 3"""
    from gpirt_amd import ordinal as OR
    from gpirt_amd import score as SC
    n, m, n_new = 100, 7, 33
    cat, _, _ = OB.make_case(n, m, 2, 5)
    cat_new = SB.make_new(n_new, m, 2, 5)
    s = _sampler(handle, cat, 2, 9, K0=np.full((m, 1), 120, dtype=np.int32))
    s.ordinal_score_enable(cat_new)
    f, B = _run(s, 4, thresholds=False)
    got = s.ordinal_score()
    s.close()
    assert (B == 0.0).all()
    y = np.where(cat_new == 0, np.nan, 2.0 * cat_new - 3.0)
    want = SC.from_draws(y, f, return_products=True)
    own = OR.score_from_draws(cat_new, f, B, return_products=True)
    delta = SB.delta_of(cat_new, f, B, own["products"][0], own["wc"][0]) + binary_delta_of(want["products"][0], m)
    SB.compare_score(got, want, delta, "C = 2 against score.from_draws")


def _constructed(handle, fstars, cat_new, K0, predict=True):
    n, m, C = 64, 6, 4
    cat, _, _ = OB.make_case(n, m, C, 3)
    s = _sampler(handle, cat, C, 5, K0=K0)
    s.ordinal_score_enable(cat_new, predict=predict, top=3)
    for f in fstars:
        s.set("fstar", np.asfortranarray(f))
        s.ordinal_score_accumulate()
    out = dict(score=s.ordinal_score(), pred=s.ordinal_score_predict() if predict else None,
               state=s.ordinal_score_state().cpu().numpy().copy(),
               pstate=s.ordinal_score_predict_state().cpu().numpy().copy() if predict else None,
               B=s.ordinal_get("thresholds"))
    s.close()
    return out


def test_constructed_fstar(handle):
    from gpirt_amd import ordinal as OR
    from gpirt_amd import score as SC
    m, C, n_new = 6, 4, 40
    rng = np.random.default_rng(17)
    th = SC.grid()
    cat_new = SB.make_new(n_new, m, C, 17, na=0.4)       # respondent 0: every answer 1; respondent 1: every answer C
    cat_new[2, 2], cat_new[3, 2] = 2, 0                   # item 2: answered by respondent 2, not by respondent 3
    K0 = np.array([[119, 120, 121]] + [[90 + 3 * j, 120, 150 - 2 * j] for j in range(1, m)], dtype=np.int32)   # item 0: one grid step apart

    def base():
        return th[:, None] * rng.uniform(0.7, 1.5, m)[None, :] * np.where(np.arange(m) % 2 == 0, 1.0, -1.0)[None, :]
    f1 = base()
    f2 = base(); f2[10, 1], f2[20, 1], f2[30, 4], f2[40, 4] = 800.0, -800.0, np.inf, -np.inf
    f3 = base(); f3[500, 2] = np.nan
    f4 = base()
    a = _constructed(handle, [f1, f2, f3, f4], cat_new, K0)
    b = _constructed(handle, [f1, f2, f4], cat_new, K0)
    B = np.broadcast_to(a["B"], (4,) + a["B"].shape)
    fs = np.stack([f1, f2, f3, f4])
    want = OR.score_from_draws(cat_new, fs, B, return_products=True)
    wpred = OR.predict_from_draws(cat_new, fs, B, top=3, return_draws=True)
    assert any((np.abs(T[np.isfinite(T)]) >= 1e299).any() for T in want["products"][0]), "an entry is held at -1e300"
    answered = cat_new[:, 2] != 0
    assert np.array_equal(want["nonfinite"], answered.astype(np.int64)) and np.array_equal(want["draws"], 4 - answered)
    assert wpred["pred_skipped"] == 1 and wpred["pred_draws"] == 3
    delta = SB.delta_of(cat_new, fs, B, want["products"][0], want["wc"][0])
    SB.compare_score(a["score"], want, delta, "constructed")
    SB.compare_predict(a["pred"], wpred, delta, cat_new, "constructed predict", cap=False)
    # end categories alone: no w term, so l is the binary-like sum; the interior respondents carry the largest |w| of item 0
    assert (np.array(want["wc"][0])[:, :2] == 0).all() and np.abs(np.array(want["wc"][0])).max() > 2.0
    # the NaN draw against a block that never saw it, word for word
    from gpirt_amd._lib import NGRID
    wa, wb = a["state"], b["state"]
    off = 8
    A = {k: wa[off + i * n_new: off + (i + 1) * n_new] for i, k in enumerate(RAW[:5])}
    Bk = {k: wb[off + i * n_new: off + (i + 1) * n_new] for i, k in enumerate(RAW[:5])}
    pa, pb = (w[off + 5 * n_new:].reshape(n_new, NGRID) for w in (wa, wb))
    assert np.array_equal(wa[:8], wb[:8])
    assert np.array_equal(A["nonfinite"] - Bk["nonfinite"], answered.astype(np.int64))
    for k in ("n_obs", "lpd_acc", "ll_sum"):
        assert np.array_equal(A[k][answered], Bk[k][answered]), k           # skipped: nothing else of theirs is touched
    assert np.array_equal(A["draws"][answered], Bk["draws"][answered]) and np.array_equal(pa[answered], pb[answered])
    assert np.array_equal(A["draws"][~answered], Bk["draws"][~answered] + 1)
    qa, qb = a["pstate"].copy(), b["pstate"].copy()
    assert qa[7] == 1 and qb[7] == 0 and qa[6] == qb[6] == 3
    qa[7] = 0
    assert np.array_equal(qa, qb), "part B skips the NaN draw whole"


@pytest.fixture(scope="module")
def three_runs(handle):
    """6 iterations on 120 x 12, C = 4 with the fit block on: twice with the score block, once without"""
    n, m, C = 120, 12, 4
    cat, _, _ = OB.make_case(n, m, C, 21)
    cat_new = SB.make_new(30, m, C, 21)
    out = []
    for on in (True, True, False):
        s = _sampler(handle, cat, C, 77, fit=True)
        if on:
            s.ordinal_score_enable(cat_new, predict=True, top=4)
        _run(s, 6, fit=True)
        d = {k: s.get(k).copy() for k in ("theta", "beta", "f", "fstar")}
        d["index"] = s.ordinal_get("index").copy()
        d["fit"] = s.ordinal_fit_state().cpu().numpy().copy()
        if on:
            d["state"] = s.ordinal_score_state().cpu().numpy().copy()
            d["pstate"] = s.ordinal_score_predict_state().cpu().numpy().copy()
        s.close()
        out.append(d)
    return out


def test_chain_untouched(three_runs):
    with_block, _, without = three_runs
    for k in ("theta", "beta", "f", "fstar", "index", "fit"):
        assert with_block[k].tobytes() == without[k].tobytes(), k


def test_repeatable(three_runs):
    a, b, _ = three_runs
    assert a["state"].tobytes() == b["state"].tobytes() and a["pstate"].tobytes() == b["pstate"].tobytes()
    assert a["pstate"][6] == 6 and a["pstate"][7] == 0


def test_pooling(handle):
    from gpirt_amd import ordinal as OR
    n, m, C, n_new = 100, 9, 3, 20
    cat, _, _ = OB.make_case(n, m, C, 61)
    cat_new = SB.make_new(n_new, m, C, 61)
    ss = []
    for seed in (3, 4):
        s = _sampler(handle, cat, C, seed)
        s.ordinal_score_enable(cat_new, predict=True, top=5)
        _run(s, 3)
        ss.append(s)
    one = [OR.score_block_arrays(s.ordinal_score_state().cpu().numpy()) for s in ss]
    pone = [OR.predict_block_arrays(s.ordinal_score_predict_state().cpu().numpy()) for s in ss]
    pooled = OR.score_combine(handle, ss, signs=[1, -1], top=5)
    mirror = OR.score_combine(handle, [ss[0], ss[0]], signs=[1, -1])
    plain = OR.score_combine(handle, ss)
    for s in ss:
        s.close()
    assert np.array_equal(pooled["post_sum"], one[0]["post_sum"] + one[1]["post_sum"][:, ::-1])
    assert np.array_equal(plain["post_sum"], one[0]["post_sum"] + one[1]["post_sum"])
    assert np.array_equal(pooled["draws"], one[0]["draws"] + one[1]["draws"]) and (pooled["draws"] == 6).all()
    assert np.array_equal(pooled["ll_sum"], one[0]["ll_sum"] + one[1]["ll_sum"])
    lae = np.logaddexp(one[0]["lpd_acc"], one[1]["lpd_acc"])
    assert (np.abs(pooled["lpd_acc"] - lae) <= 4 * EPS * (1 + np.abs(lae))).all()
    assert np.array_equal(pooled["lpd_acc"], plain["lpd_acc"])                     # lpd takes no sign
    assert np.array_equal(mirror["grid_post"], mirror["grid_post"][:, ::-1])
    pp = pooled["predict"]
    assert np.array_equal(pp["prob_sum"], pone[0]["prob_sum"] + pone[1]["prob_sum"])
    assert np.array_equal(pp["info_sum"], pone[0]["info_sum"] + pone[1]["info_sum"])
    assert pp["pred_draws"] == 6 and pp["pred_skipped"] == 0 and pp["probs"].shape == (n_new, m, C)
    assert np.array_equal(pone[0]["answered"], cat_new != 0)


def test_refusals(handle):
    from gpirt_amd import Sampler
    from gpirt_amd import ordinal as OR
    from gpirt_amd._lib import GpirtError
    n, m, C = 64, 6, 3
    cat, _, _ = OB.make_case(n, m, C, 1)
    cat_new = SB.make_new(5, m, C, 1)
    s = Sampler(handle, OR.dichotomise(cat), OB.theta_start(n, 7), seed=1, preset="fast")
    with pytest.raises(GpirtError, match="needs an initialised sampler"):
        s.ordinal_score_enable(cat_new)
    s.init()
    with pytest.raises(GpirtError, match="ordinal responses are not enabled"):
        s.ordinal_score_enable(cat_new)
    s.ordinal_enable(cat, C)
    with pytest.raises(GpirtError, match="ordinal scoring is not enabled"):
        s.ordinal_score_accumulate()
    with pytest.raises(GpirtError, match="ordinal scoring is not enabled"):
        s.ordinal_score_get("draws")
    with pytest.raises(ValueError, match="item columns"):
        s.ordinal_score_enable(cat_new[:, :m - 1])
    bad = cat_new.copy(); bad[0, 0] = C + 1
    with pytest.raises(GpirtError, match=r"it must lie in 0 \.\. C = 3"):
        s.ordinal_score_enable(bad)
    with pytest.raises(ValueError, match="outside 1..16384"):
        s.ordinal_score_enable(np.zeros((16385, m), dtype=np.int8))
    import ctypes as ct
    big = np.zeros((16385, m), dtype=np.int8, order="F")
    assert s.lib.gpirt_sampler_ordinal_score_enable(s._s, big.ctypes.data_as(ct.POINTER(ct.c_int8)), 16385, 0, 5) < 0
    assert "n_new = 16385 is outside 1..16384" in s.lib.gpirt_last_error().decode()
    for top in (0, 17):
        with pytest.raises(GpirtError, match=f"top = {top} is outside 1..16"):
            s.ordinal_score_enable(cat_new, predict=True, top=top)
    s.ordinal_score_enable(cat_new)
    with pytest.raises(GpirtError, match="needs the prediction part"):
        s.ordinal_score_get("prob_sum")
    with pytest.raises(GpirtError, match="ordinal prediction is not enabled"):
        s.ordinal_score_predict_state()
    with pytest.raises(GpirtError, match="unknown ordinal score field"):
        s.ordinal_score_get("nothing")
    with pytest.raises(GpirtError, match="refused while ordinal responses are on"):
        s.score_enable(np.where(cat_new == 0, np.nan, 1.0))
    s.ordinal_enable(None)                                 # frees the block with the rest
    with pytest.raises(GpirtError, match="not enabled"):
        s.ordinal_score_accumulate()
    s.close()


def test_run(handle):
    from gpirt_amd import ordinal as OR
    n, m, C = 120, 12, 4
    d = OR.make_graded(n, m, C, seed=5)
    cat_new = SB.make_new(10, m, C, 5)
    base = OR.run(d["cat"], 6, 2, C=C, chains=2, handle=handle)
    res = OR.run(d["cat"], 6, 2, C=C, chains=2, handle=handle, score=dict(data=cat_new, predict=True, top=3))
    assert set(res) == set(base) | {"score"}
    assert set(base) == {"theta", "beta", "threshold_draws", "thresholds", "hist", "curves", "counters", "grid", "categories", "chains",
                         "consistent"}
    sc = res["score"]
    for k in ("grid_post", "theta_mean", "theta_sd", "theta_quantiles", "theta_map", "lpd", "loglik_mean", "lpd_total",
              "se_lpd_total", "post_sum", "lpd_acc", "ll_sum", "draws", "nonfinite", "n_obs", "signs", "predict"):
        assert k in sc, k
    assert set(sc["predict"]) == {"probs", "expected", "info", "next_items", "next_info", "prob_sum", "info_sum", "pred_draws",
                                  "pred_skipped"}
    assert len(sc["signs"]) == 2 and sc["signs"][0] == 1 and sc["signs"][1] in (1, -1)
    assert (sc["draws"] == 12).all() and sc["predict"]["pred_draws"] == 12
    assert (np.abs(sc["grid_post"].sum(axis=1) - 1.0) <= 1e-12).all()
    assert (np.abs(sc["predict"]["probs"].sum(axis=2) - 1.0) <= (C + 2) * 1001 * EPS).all()
    assert sc["predict"]["next_items"].shape == (10, 3)
    assert np.array_equal(res["theta"], base["theta"])     # the chain is the one it was
