"""Predicting new respondents' unseen answers on the device (csrc/predict.hip, the WEIGHTS form of csrc/score.hip) against
the NumPy statement of the header (gpirt_amd.score.predict_from_draws): the stage API at five sizes under both product
forms, the weights, the untouched score state and chain, constructed f*, a NaN cell, pooling, repeatability and the
refusals.  The tolerances are derived from each case's own inputs (tests/_predict_bounds.py)."""
import ctypes as C

import numpy as np
import pytest

from _predict_bounds import compare, delta_from
from _score_bounds import EPS, delta_of

pytestmark = pytest.mark.gpu
CODES = dict(yea=[1], nay=[-1], missing=[None])
N = 1001


def y_new_for(n_new, m, seed):
    """about 30 % NaN; from three respondents on, the last answered nothing and the one before everything"""
    from gpirt_amd.synthetic import make_responses
    y, _ = make_responses(n_new + 2, m, seed=seed, na_frac=0.3)
    full = np.array(y[n_new])
    full[np.isnan(full)] = 1.0
    y = np.array(y[:n_new])
    if n_new >= 3:
        y[-1, :] = np.nan
        y[-2, :] = full
    return y


def run_stage(handle, n, m, n_new, steps, seed=5, predict=True, keep_states=False):
    """steps sampling iterations with score_accumulate after each; returns y_new, the f* draws, the prediction (or None),
    the weights after the first draw and, with keep_states, (score block, theta, f*) after every draw"""
    from gpirt_amd import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=100 + n, na_frac=0.03)
    y_new = y_new_for(n_new, m, 7 + n_new)
    s = Sampler(handle, y, th0, preset="fast", seed=seed)
    s.init()
    s.score_enable(y_new)
    if predict:
        s.score_predict_enable(top=5)
    fs, states, w0 = [], [], None
    for it in range(steps):
        s.step()
        s.score_accumulate()
        fs.append(s.get("fstar"))
        if predict and it == 0:
            w0 = s.score_predict_get("weights")
        if keep_states:
            states.append((s.score_state().cpu().numpy().copy(), s.get("theta"), fs[-1]))
    s.check()
    got = s.score_predict() if predict else None
    if predict:
        raw = {k: s.score_predict_get(k) for k in ("pred_sum", "info_sum", "p_yes", "info", "counts")}
        block = s.score_predict_state().cpu().numpy().copy()
        got = dict(got, raw=raw, block=block)
    s.close()
    return y_new, np.stack(fs), got, w0, states


def check_block(block, y_new, got):
    """the state block word for word: header, packed answered-mask, pred_sum, info_sum"""
    n_new, m = y_new.shape
    assert block[:8].tolist() == [n_new, m, 1, N, got["pred_draws"], got["pred_skipped"], 0, 0x44455250]
    words = (n_new * m + 63) // 64
    bits = np.unpackbits(block[8:8 + words].view(np.uint8), bitorder="little")[:n_new * m]
    assert np.array_equal(bits.reshape(m, n_new).T.astype(bool), ~np.isnan(y_new))
    sums = block[8 + words:].view(np.float64)
    assert sums.size == 2 * n_new * m
    assert np.array_equal(sums[:n_new * m].reshape(m, n_new).T, got["pred_sum"])
    assert np.array_equal(sums[n_new * m:].reshape(m, n_new).T, got["info_sum"])


SHAPES = [(100, 17, 1, 4), (100, 3, 65, 4), (257, 33, 63, 4), (1000, 65, 257, 4)]


@pytest.mark.parametrize("n,m,n_new,steps,fixed", [sh + (fx,) for fx in (1, 2) for sh in SHAPES] + [(8192, 1024, 256, 2, 1)])
def test_stage_api_against_predict_from_draws(handle, n, m, n_new, steps, fixed):
    """n_new = 1, 63 / 65 and 257 are the wave, work-group and tile edges; m is odd and below one tile; the grid's 1001
    points are never a tile multiple.  fixed = 1: the fixed-point product; 2: the fp64 GEMM -- each compared on its OWN f*
    draws (the large case under the fixed-point product only).  Also: the weights of the first draw, and every name of
    score_predict_get against score_predict()."""
    from gpirt_amd import score
    with handle.config("GPIRT_THETA_FIXED", fixed):
        y_new, fs, got, w0, _ = run_stage(handle, n, m, n_new, steps)
    want = score.predict_from_draws(y_new, fs, return_draws=True)
    delta = delta_from(want, m)
    label = f"stage n={n} m={m} n_new={n_new} fixed={fixed}"
    compare(got, want, delta, y_new, label)
    assert got["pred_draws"] == steps and got["pred_skipped"] == 0
    for k in ("pred_sum", "info_sum", "p_yes", "info"):
        assert np.array_equal(got["raw"][k], got[k]), k
    assert got["raw"]["counts"].tolist() == [steps, 0]
    check_block(got["block"], y_new, got)
    if n_new >= 3:
        assert (got["next_items"][-2] == -1).all() and np.isnan(got["next_info"][-2]).all()
    # the weights: the reference's within rho w, every column sums to 1 within 1001 eps
    rho = 2.0 * delta_of([want["products"][0][0]], m) + 2.0 * N * EPS
    wr = want["weights"][0][0]
    gap_w = float((np.abs(w0 - wr) / (wr + 1e-300)).max())
    gap_1 = float(np.abs(w0.sum(axis=0) - 1.0).max())
    print(f"MEASURED {label}: weights rel gap {gap_w:.3e} (rho {rho:.3e}), column sums off 1 by {gap_1:.3e}")
    assert w0.shape == (N, n_new) and (np.abs(w0 - wr) <= rho * wr + 1e-300).all() and gap_1 <= N * EPS


def test_score_state_and_chain_untouched(handle):
    """The same seed with prediction on and off: the score state block, theta and f* bit-equal after every draw."""
    a = run_stage(handle, 257, 33, 63, 3, predict=True, keep_states=True)[4]
    b = run_stage(handle, 257, 33, 63, 3, predict=False, keep_states=True)[4]
    same = [all(np.array_equal(x, y) for x, y in zip(sa, sb)) for sa, sb in zip(a, b)]
    print(f"MEASURED score state / theta / f* with prediction on against off, per draw bit-equal: {same}")
    assert len(same) == 3 and all(same)


def constructed(handle, fstars, y_new, m=6, n=64, top=5):
    """score_accumulate called directly on constructed f* (through set("fstar", ...))"""
    from gpirt_amd import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=5)
    s = Sampler(handle, y, th0, preset="fast", seed=3)
    s.init()
    s.score_enable(y_new)
    s.score_predict_enable(top=top)
    for f in fstars:
        s.set("fstar", np.asfortranarray(f))
        s.score_accumulate()
    got, sc = s.score_predict(), s.score()
    w = s.score_predict_get("weights")
    s.close()
    return got, sc, w


def test_constructed_fstar(handle):
    """All zeros; a step at k = 500; |f*| = 800 in one column: each against its closed form and against
    predict_from_draws."""
    from gpirt_amd import score
    m, n_new = 6, 40
    y_new = y_new_for(n_new, m, 19)
    rng = np.random.default_rng(1)
    zero = np.zeros((N, m))
    step = np.where(np.arange(N)[:, None] >= 500, 1.0, -1.0) * rng.uniform(0.5, 3.0, m)
    big = rng.normal(0, 1, (N, m)) * 0.3
    big[:, 2] = np.where(np.arange(N) >= 500, 800.0, -800.0)
    cases = (("zeros", [zero]), ("step", [step]), ("saturated", [big]), ("all three", [zero, step, big]))
    for name, fs in cases:
        got, _, w = constructed(handle, fs, y_new)
        want = score.predict_from_draws(y_new, np.stack(fs), return_draws=True)
        c = 2.0 * delta_from(want, m) + 5.0 * N * EPS
        compare(got, want, delta_from(want, m), y_new, f"constructed {name}", cap=False)     # (zeros: every rank is tied)
        if name == "zeros":
            gap_p, gap_i = float(np.abs(got["p_yes"] - 0.5).max()), float(np.abs(got["info"]).max())
            print(f"MEASURED zeros: p_yes gap to 1/2 {gap_p:.3e}, info gap to 0 {gap_i:.3e}")
            assert gap_p <= c * 0.5 and gap_i <= 2 * c * np.log(2.0) + 8 * EPS
        if name == "step":            # P takes two values per column: q = p_lo + (p_hi - p_lo) * (the mass at k >= 500)
            mass = w[500:].sum(axis=0)
            P, H = score.plogis_entropy(step)
            q = P[0][None, :] + (P[-1] - P[0])[None, :] * mass[:, None]
            gap = float(np.abs(got["p_yes"] - q).max())
            info = score.binary_entropy(q) - H[0][None, :]             # H is symmetric: the same on both sides of the step
            gap_i = float(np.abs(got["info"] - info).max())
            print(f"MEASURED step: p_yes gap to the closed form {gap:.3e}, info gap {gap_i:.3e}")
            assert gap <= 2 * N * EPS and gap_i <= 16 * N * EPS
        if name == "saturated":       # H = 0 in the column: p_yes is the mass above, info the prediction's whole entropy
            mass = w[500:].sum(axis=0)
            gap = float(np.abs(got["p_yes"][:, 2] - mass).max())
            gap_i = float(np.abs(got["info"][:, 2] - score.binary_entropy(got["p_yes"][:, 2])).max())
            print(f"MEASURED saturated: p_yes gap to the mass above {gap:.3e}, info gap to h(p_yes) {gap_i:.3e}")
            assert gap <= 2 * N * EPS and gap_i <= 8 * EPS


def test_nan_cell_skips_the_draw_for_prediction_only(handle):
    """One draw of three has a NaN cell: pred_skipped = 1, pred_draws = 2, the sums are those of the two clean draws (bit
    for bit), and the scorer's own nonfinite counts only those who answered the item."""
    m, n_new = 6, 40
    y_new = y_new_for(n_new, m, 23)
    y_new[0, 4], y_new[1, 4] = np.nan, 1.0
    rng = np.random.default_rng(2)
    fs = [rng.normal(0, 1, (N, m)) for _ in range(3)]
    bad = [fs[0], fs[1].copy(), fs[2]]
    bad[1][321, 4] = np.nan
    got, sc, _ = constructed(handle, bad, y_new)
    clean, _, _ = constructed(handle, [fs[0], fs[2]], y_new)
    assert got["pred_skipped"] == 1 and got["pred_draws"] == 2 and clean["pred_skipped"] == 0
    same = all(np.array_equal(got[k], clean[k], equal_nan=True) for k in ("pred_sum", "info_sum", "p_yes", "info", "next_items"))
    answered = ~np.isnan(y_new[:, 4])
    print(f"MEASURED NaN cell: sums bit-equal to the two clean draws' {same}; scorer nonfinite {int(sc['nonfinite'].sum())} "
          f"of {int(answered.sum())} who answered the item")
    assert same
    assert np.array_equal(sc["nonfinite"], answered.astype(np.int64)) and np.array_equal(sc["draws"], 3 - answered)
    from gpirt_amd import score
    want = score.predict_from_draws(y_new, np.stack(bad), return_draws=True)
    compare(got, want, delta_from(want, m), y_new, "NaN cell")


def test_chain_untouched_through_gpirtmcmc():
    """gpirtMCMC(score=dict(..., predict=True)) against the same call without predict: draws, IRFs and every score output
    identical; R's stream ends at the same position."""
    from gpirt_amd import gpirtMCMC
    from gpirt_amd.ops import RStream
    from gpirt_amd.synthetic import make_responses
    n, m, S, B = 96, 12, 4, 2
    y, th0 = make_responses(n, m, seed=31, snap_theta=False)
    y_new = y_new_for(9, m, 3)
    for case in ("fast", "reference"):
        kw = dict(vote_codes=CODES, preset="fast", seed=9) if case == "fast" else dict(vote_codes=CODES, theta_init=th0)
        rs = [RStream(77), RStream(77)]
        res = []
        for k, extra in enumerate((dict(), dict(predict=True, top=3))):
            more = dict(rstream=rs[k]) if case == "reference" else {}
            res.append(gpirtMCMC(y, S, B, score=dict(data=y_new, **extra), **kw, **more))
        plain, pred = res
        assert "predict" not in plain["score"] and "predict" in pred["score"]
        same = all(np.array_equal(plain[k], pred[k], equal_nan=True) for k in ("theta", "beta", "f", "IRFs"))
        same_sc = all(np.array_equal(np.asarray(plain["score"][k]), np.asarray(pred["score"][k]), equal_nan=True)
                      for k in plain["score"])
        print(f"MEASURED untouched chain {case}: draws and IRFs bit-equal {same}, score outputs bit-equal {same_sc}")
        assert same and same_sc
        if case == "reference":
            (mt0, i0), (mt1, i1) = rs[0].state(), rs[1].state()
            assert i0 == i1 and np.array_equal(mt0, mt1)
        p = pred["score"]["predict"]
        assert p["pred_draws"] == S and p["pred_skipped"] == 0 and p["next_items"].shape == (9, 3)
        assert p["p_yes"].shape == (9, m) and (p["p_yes"] > 0).all() and (p["p_yes"] < 1).all()
        assert (p["info"] > -1e-12).all() and (p["next_items"][-2] == -1).all()


def test_pooling(handle):
    """Two chains' states through predict_combine against predict_from_draws over both; gpirtMCMC(chains=2) with a
    reflected chain gives the same predict as with align=False."""
    from gpirt_amd import Sampler, _lib, gpirtMCMC, score
    from gpirt_amd.synthetic import make_responses
    n, m, S, B, seed, n_new = 200, 24, 4, 2, 29, 33
    y, _, truth = make_responses(n, m, seed=11, return_truth=True)
    th0 = -5.0 + np.clip(np.rint((truth + 5.0) / 0.01), 0, 1000) * 0.01      # the generating theta on the grid; chain 1
    y_new = y_new_for(n_new, m, 13)                                            # starts at its mirror image
    inits = np.stack([th0, -th0])
    samplers, fs = [], []
    for c in range(2):
        s = Sampler(handle, y, inits[c], rng="item", seed=_lib.chain_seed(seed, c), theta_stabilise=True)
        s.init()
        s.score_enable(y_new)
        s.score_predict_enable(top=7)
        fc = []
        for it in range(S + B):
            s.step()
            if it >= B:
                s.score_accumulate()
                fc.append(s.get("fstar"))
        s.check()
        samplers.append(s)
        fs.append(np.stack(fc))
    pooled = score.predict_combine(handle, samplers, top=7)
    want = score.predict_from_draws(y_new, np.stack(fs), top=7, return_draws=True)
    compare(pooled, want, delta_from(want, m), y_new, "combine of two chains")
    assert pooled["pred_draws"] == 2 * S
    one = [s.score_predict() for s in samplers]
    assert np.array_equal(pooled["pred_sum"], one[0]["pred_sum"] + one[1]["pred_sum"])
    assert np.array_equal(pooled["info_sum"], one[0]["info_sum"] + one[1]["info_sum"])

    def run(sd, al):
        return gpirtMCMC(y, S, B, vote_codes=CODES, theta_init=inits, rng="item", seed=sd, theta_stabilise=True, chains=2,
                         align=al, score=dict(data=y_new, predict=True, top=7))
    first = run(seed, True)
    replay = all(np.array_equal(np.asarray(pooled[k]), np.asarray(first["score"]["predict"][k]), equal_nan=True) for k in pooled)
    # which mode a short chain settles in depends on its seed: take the first seed whose alignment reflects a chain
    found = None
    for sd in range(seed, seed + 16):
        res = first if sd == seed else run(sd, True)
        if res["diagnostics"]["reflected"].any():
            found = sd
            break
    assert found is not None, "no seed in 16 gave a reflected chain"
    plain = run(found, False)
    refl = res["diagnostics"]["reflected"]
    equal = all(np.array_equal(np.asarray(res["score"]["predict"][k]), np.asarray(plain["score"]["predict"][k]),
                               equal_nan=True) for k in res["score"]["predict"])
    moved = not np.array_equal(res["score"]["grid_post"], plain["score"]["grid_post"])      # the SCORE does see the reflection
    print(f"MEASURED gpirtMCMC(chains=2, seed={found}): predict with align bit-equal to without {equal} (reflected {refl}, "
          f"grid_post differs {moved}); seed {seed} bit-equal to combine of the replayed states {replay}")
    assert equal and replay and moved and not plain["diagnostics"]["reflected"].any()
    for s in samplers:
        s.close()


def test_repeatable(handle):
    """The same run twice gives bit-identical predict state blocks."""
    blocks = [run_stage(handle, 257, 33, 63, 3)[2]["block"] for _ in range(2)]
    same = np.array_equal(blocks[0], blocks[1])
    print(f"MEASURED repeatability: predict state blocks bit-equal {same}")
    assert same


def test_refusals(handle):
    from gpirt_amd import Sampler, _lib, gpirtMCMC, score
    from gpirt_amd.distributed import ShardedSampler
    from gpirt_amd.synthetic import make_responses
    n, m = 64, 6
    y, th0 = make_responses(n, m, seed=5)
    s = Sampler(handle, y, th0, preset="fast", seed=3)
    s.init()
    with pytest.raises(_lib.GpirtError, match="scoring is not enabled"):
        s.score_predict_enable()
    s.score_enable(np.ones((3, m)))
    with pytest.raises(_lib.GpirtError, match="prediction is not enabled"):
        s.score_predict_get("counts")
    for top in (0, 17):
        with pytest.raises(ValueError, match="outside 1..16"):
            s.score_predict_enable(top=top)
    s.score_predict_enable(top=2)
    out = np.empty(3 * m)
    assert s.lib.gpirt_sampler_score_predict_get(s._s, b"p_yes", C.c_void_p(out.ctypes.data), out.nbytes - 8) == _lib.E_ARG
    assert s.lib.gpirt_sampler_score_predict_get(s._s, b"counts", C.c_void_p(out.ctypes.data), 8) == _lib.E_ARG
    assert s.lib.gpirt_sampler_score_predict_get(s._s, b"weights", C.c_void_p(out.ctypes.data), 8 * N) == _lib.E_ARG
    assert s.lib.gpirt_sampler_score_predict_get(s._s, b"nothing", C.c_void_p(out.ctypes.data), out.nbytes) == _lib.E_ARG
    assert s.score_predict_get("counts").tolist() == [0, 0]
    assert np.isnan(s.score_predict()["p_yes"]).all()                      # no draw yet: NaN everywhere, nothing listed
    # the struct's own checks
    r, _ = score.predict_struct(3, m, 2)
    ptr = (C.c_void_p * 1)(s.score_predict_state().data_ptr())
    for field, val in (("top", 0), ("top", 17), ("reserved0", 1)):
        r2, _keep = score.predict_struct(3, m, 2)
        setattr(r2, field, val)
        assert s.lib.gpirt_score_predict_combine(handle.ptr, 1, ptr, C.byref(r2)) == _lib.E_ARG
    # mismatched blocks: another y_new of the same size, another size, and a score block in a predict block's place
    others = []
    for y2 in (np.where(np.eye(3, m) > 0, np.nan, 1.0), np.ones((4, m))):
        t = Sampler(handle, y, th0, preset="fast", seed=3)
        t.init()
        t.score_enable(y2)
        t.score_predict_enable()
        others.append(t)
    with pytest.raises(_lib.GpirtError, match="another y_new"):
        score.predict_combine(handle, [s, others[0]])
    with pytest.raises(_lib.GpirtError, match="another n_new or m"):
        score.predict_combine(handle, [s, others[1]])
    with pytest.raises(_lib.GpirtError, match="not a predict state block"):
        score.predict_combine(handle, [s.score_state()])
    s.score_enable(np.ones((2, m)))                      # scoring set up again: the prediction goes with the old state
    with pytest.raises(_lib.GpirtError, match="prediction is not enabled"):
        s.score_predict_get("counts")
    for t in others + [s]:
        t.close()
    with pytest.raises(ValueError, match="unknown keys"):
        gpirtMCMC(y, 1, 0, vote_codes=CODES, theta_init=th0, preset="fast", score=dict(data=np.ones((2, m)), predicts=True))
    with pytest.raises(ValueError, match="outside 1..16"):
        gpirtMCMC(y, 1, 0, vote_codes=CODES, theta_init=th0, preset="fast", score=dict(data=np.ones((2, m)), predict=True, top=0))
    with pytest.raises(ValueError, match="item shards"):
        ShardedSampler.score_predict_enable(object())
