"""Per-item GP amplitudes on the device (include/gpirt_hip.h "per-item GP amplitudes", csrc/amp.hip, csrc/sampler.hip,
gpirt_amd.amp): one update of every item against the NumPy statement gpirt_amd.amp.step_exact within the bounds
tests/_amp_bounds.py derives, a trajectory decision for decision, the chain against the exact conditional posterior, amplitude 1
as the sampler it was, fixed amplitudes in draw_f and draw_fstar, the failure edges, the interplay with the length-scale
updates, the recorder and the one-call run.  Every handle is the test's own."""
import numpy as np
import pytest

import _amp_bounds as AB
import _ell_bounds as EB

pytestmark = pytest.mark.gpu

FAST = dict(rng="item", theta_stabilise=True, fstar_fused=True)
FORMS = {"written": dict(fstar_fused=False), "fused": dict(fstar_fused=True), "rank": dict(fstar_fused=True, kstar_rank=64)}


@pytest.fixture
def handles():
    """make() -> a fresh Handle under the default kernel; all closed when the test ends"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpirt_amd.ops import Handle
    made = []

    def make(kernel=None):
        made.append(Handle(kernel=kernel))
        return made[-1]

    yield make
    for h in made:
        h.close()


def _sampler(handles, c, seed, widths, planned=0, f=None, y=None, **kw):
    """a sampler in the constructed state of case c (theta, f, beta, mu as given), the amplitudes on the grid at c's indices"""
    from gpirt_amd.sampler import Sampler
    s = Sampler(handles(), c["y"] if y is None else y, c["theta"], seed=seed, **dict(FAST, **kw))
    s.init()
    s.set("f", c["f"] if f is None else f)
    s.set("beta", c["beta"])
    s.set("mu", c["mu"])
    s.amp_enable(c["lo"], c["hi"], c["points"], c["log_prior"], int(np.min(widths)), c["k"], planned_draws=planned)
    s.amp_width(widths)
    s.check()
    return s


def _follow(s, c, seed, widths, updates, f, y=None, t0=0):
    """`updates` draw_amp calls, each against step_exact from the state before it: the status, the index, the record within the
    derived bounds, f byte for byte, the amplitude and the counters.  Returns the statuses seen and the proposals made."""
    from gpirt_amd import _lib, amp as A
    y = c["y"] if y is None else y
    k = c["k"].copy()
    g, m = c["grid"], c["m"]
    counts = np.zeros((4, m), dtype=np.int64)
    seen, props, worst = [], [], 0.0
    for t in range(t0 + 1, t0 + updates + 1):
        ref = A.step_exact(f, c["mu"], y, k, widths, seed, t, g, c["log_prior"])
        s.draw_amp()
        rec, idx, f_dev = s.amp_get("record"), s.amp_get("index"), s.get("f")
        status = [_lib.AMP_STATUS[int(x)] for x in rec[3]]
        assert status == ref["status"], (t, status, ref["status"])
        assert np.array_equal(idx, ref["k"]) and np.array_equal(s.amp_get("amplitude"), g[ref["k"]])
        with np.errstate(all="ignore"):
            fp = (g[np.clip(ref["k_prop"], 0, len(g) - 1)] / g[k])[None, :] * f
        for j, st in enumerate(status):
            counts[0, j] += 1
            counts[1, j] += st == "accepted"
            counts[2, j] += st == "out_of_range"
            counts[3, j] += st == "failed"
            if st == "out_of_range":
                assert np.isnan(rec[:3, j]).all() and rec[4, j] == 0
                continue
            assert rec[4, j] == ref["nonfinite"][j]
            assert abs(rec[2, j] - float(ref["log_u"][j])) <= 2 * AB.U * abs(float(ref["log_u"][j]))
            if st == "failed":
                continue
            e_dll, e_ratio = AB.dll_bounds(f[:, j:j + 1], fp[:, j:j + 1], c["mu"][:, j:j + 1], y[:, j:j + 1], [ref["dll"][j]],
                                           [c["log_prior"][ref["k_prop"][j]] - c["log_prior"][k[j]]])
            err_d, err_r = abs(float(AB.LD(rec[0, j]) - ref["dll"][j])), abs(float(AB.LD(rec[1, j]) - ref["log_ratio"][j]))
            if e_dll[0] > 0:                                          # (an item with no observed cell: both are exactly 0)
                worst = max(worst, err_d / e_dll[0], err_r / e_ratio[0])
            assert err_d <= e_dll[0] and err_r <= e_ratio[0], (t, j, err_d, e_dll[0], err_r, e_ratio[0])
            assert e_ratio[0] < 1e-9                                  # the bound is not vacuous: a log ratio is of order 1
        # accepted columns are c f bit for bit, every other column is byte-identical: both are the statement's f
        assert f_dev.tobytes() == np.asfortranarray(ref["f"]).tobytes(), t
        for j, st in enumerate(status):
            want = fp[:, j] if st == "accepted" else f[:, j]
            assert f_dev[:, j].tobytes() == want.tobytes()
        assert np.array_equal(s.amp_get("counts"), counts)
        f, k = f_dev, ref["k"]
        seen += status
        props += list(ref["k_prop"])
    return dict(seen=seen, props=np.array(props), worst=worst, f=f, k=k, counts=counts)


# ---------------------------------------------------------------------------------------- 1. one update, constructed ---
@pytest.mark.parametrize("m", [1, 3, 17])
@pytest.mark.parametrize("n", [40, 255, 257, 1023, 1025, 1300])
def test_updates_from_a_constructed_state_against_step_exact(handles, n, m):
    """n at the edges of the 256-thread loop and its four-fold unroll, m of one, three and seventeen work-groups, 5 % NaN in y.
    P = 9; the items start at index 0, 8 and 4 in turn with widths 3, 2 and 1, so that proposals leave the grid at both ends.
    Four updates, each checked against step_exact from the state before it (seed 1: the statement meets accepted, rejected and
    out-of-range updates, at both ends for m >= 3)."""
    seed = 1
    k0 = np.array([(0, 8, 4)[j % 3] for j in range(m)])
    widths = np.array([(3, 2, 1)[j % 3] for j in range(m)], dtype=np.int32)
    c = AB.case(n, m, 9, 500 + n + m, lo=0.25, hi=4.0, k=k0)
    s = _sampler(handles, c, seed, widths)
    assert np.array_equal(s.amp_get("width"), widths) and np.array_equal(s.amp_get("index"), k0)
    assert np.array_equal(s.amp_get("grid"), c["grid"]) and np.array_equal(s.amp_get("log_prior"), c["log_prior"])
    got = _follow(s, c, seed, widths, 4, c["f"])
    print(f"MEASURED n={n} m={m}: worst error / bound {got['worst']:.3e}; statuses "
          f"{ {st: got['seen'].count(st) for st in set(got['seen'])} }")
    assert (got["props"] < 0).any() and "accepted" in got["seen"]
    if m >= 3:
        assert (got["props"] > 8).any() and "rejected" in got["seen"]
    a = s.amp()
    assert a["mode"] == "sampled" and a["calls"] == 4 and a["updates"] == 4 * m == got["counts"][0].sum()
    assert a["accepted"] == got["counts"][1].sum() and a["out_of_range"] == got["counts"][2].sum() and a["failed"] == 0
    assert a["accept_rate"] == a["accepted"] / a["updates"]
    s.check()
    s.close()


# ------------------------------------------------------------------------------------------------- 2. trajectory ---
def test_trajectory_equals_the_numpy_chain(handles):
    """The CPU test's case (n = 40, m = 3, P = 17, w = 2), 200 draw_amp calls with no step() in between: the index series of
    every item equals the statement's decision for decision, the counters too, and the final f bit for bit."""
    c = AB.case(AB.N, AB.M, AB.P, AB.SEED)
    ch = AB.chain(c, AB.W, AB.UPDATES)
    s = _sampler(handles, c, AB.SEED, np.full(AB.M, AB.W, dtype=np.int32))
    ks = np.empty((AB.UPDATES, AB.M), dtype=np.int64)
    for t in range(AB.UPDATES):
        s.draw_amp()
        ks[t] = s.amp_get("index")
    s.check()
    for j in range(AB.M):
        diff = np.flatnonzero(ks[:, j] != ch["ks"][:, j])
        assert diff.size == 0, f"item {j}: the chains part at update {diff[0] + 1}"
    assert np.array_equal(s.amp_get("counts"), ch["counts"])
    assert s.get("f").tobytes() == np.asfortranarray(ch["f"]).tobytes()
    assert np.array_equal(s.amp_get("amplitude"), c["grid"][ch["k"]])
    print(f"MEASURED trajectory: counts {ch['counts'].tolist()}")
    s.close()


# ----------------------------------------------------------------------------- 3. the chain against its stationary mass ---
def test_chain_against_the_conditional_posterior(handles):
    """4000 updates at n = 40, m = 3, P = 9 with no step(): per item, the total variation between the visit frequencies and
    conditional_posterior lies under tv_bound with the series' own ESS (tests/_ell_bounds.py)."""
    from gpirt_amd import amp as A
    updates = 4000
    c = AB.case(40, 3, 9, 12, lo=0.25, hi=4.0)
    p = A.conditional_posterior(c["f"], c["k"], c["mu"], c["y"], c["grid"], c["log_prior"])
    s = _sampler(handles, c, 8, np.full(3, 2, dtype=np.int32), planned=updates)
    for _ in range(updates):
        s.draw_amp()
        s.amp_record()
    s.check()
    draws, hist = s.amp_get("draws"), s.amp_get("hist")
    assert draws.shape == (updates, 3) and hist.sum(axis=0).tolist() == [updates] * 3
    for j in range(3):
        freq = np.bincount(draws[:, j], minlength=9) / updates
        assert np.array_equal(hist[:, j], np.bincount(draws[:, j], minlength=9))
        ess = EB.index_ess(draws[:, j])
        tv, bound = 0.5 * np.abs(freq - p[:, j]).sum(), EB.tv_bound(p[:, j], ess)
        print(f"MEASURED item {j}: TV {tv:.4f}, bound {bound:.4f}, ESS {ess:.0f}, accept "
              f"{s.amp_get('counts')[1, j] / updates:.3f}")
        assert tv <= bound
        assert bound < 0.5 * np.abs(np.roll(p[:, j], 2) - p[:, j]).sum()      # not vacuous: the mass shifted by two points fails
    s.close()


# ----------------------------------------------------------------------------------------- 4. amplitude 1 is off ---
@pytest.mark.parametrize("form", list(FORMS))
def test_amplitude_one_is_the_sampler_as_it_was(handles, form):
    """three step()s at n = 96, m = 12 under each draw_fstar form: a sampler that never heard of amplitudes, one with
    amp_set(ones), one with amp_enable on a grid whose lo is 1.0, k0 = 0 and no update called -- byte-identical theta, beta, f
    and f*"""
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(96, 12, seed=3)
    out = []
    for mode in ("never", "set", "enable"):
        s = Sampler(handles(), y, th0, seed=5, **dict(rng="item", theta_stabilise=True, **FORMS[form]))
        s.init()
        if mode == "set":
            s.amp_set(np.ones(12))
            assert s.amp()["mode"] == "fixed" and np.array_equal(s.amp_get("amplitude"), np.ones(12))
        elif mode == "enable":
            s.amp_enable(1.0, 4.0, 5, None, 2, 0)
            assert s.amp()["mode"] == "sampled" and np.array_equal(s.amp_get("amplitude"), np.ones(12))
        else:
            assert s.amp()["mode"] is None
        for _ in range(3):
            s.step()
        s.check()
        out.append({k: s.get(k).tobytes() for k in ("theta", "beta", "f", "fstar")})
        s.close()
    assert out[0] == out[1] == out[2]


# --------------------------------------------------------------------------------- 5. fixed amplitudes act where they should ---
@pytest.mark.parametrize("form", list(FORMS))
def test_fixed_amplitudes_in_draw_f_and_draw_fstar(handles, form):
    """From one state and iteration counter, amplitudes 1, 2 and 3 on different items (n = 128, m = 6) beside a unit twin:
    draw_fstar's mean is byte-identical and f* - mean is a_j times the unit run's within tests/_amp_bounds.py's bound;
    draw_f's prior draw is a_j (L z_j) bit for bit, and its f follows the long-double slice of tests/_stage_exact.py fed that
    draw: the rejection counts exactly, f within that file's bound."""
    import _stage_exact as X
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    n, m, seed = 128, 6, 7
    y, th0 = make_responses(n, m, seed=4)
    a = np.array([1.0, 2.0, 3.0, 3.0, 1.0, 2.0])
    pair = []
    for amp in (None, a):
        s = Sampler(handles(), y, th0, seed=seed, **dict(rng="item", theta_stabilise=True, **FORMS[form]))
        s.init()
        if amp is not None:
            s.amp_set(amp)
        s.check()
        pair.append(s)
    unit, scaled = pair
    f0, mu = unit.get("f"), unit.get("mu")
    assert scaled.get("f").tobytes() == f0.tobytes() and unit.iteration == scaled.iteration
    # draw_fstar
    res = []
    for s in pair:
        s.draw_fstar()
        res.append(dict(mean=s.get("mean"), mu_star=s.get("mu_star"), sd=s.get("s"), fstar=s.get("fstar")))
    u, w = res
    assert u["mean"].tobytes() == w["mean"].tobytes() and u["sd"].tobytes() == w["sd"].tobytes()
    mean = u["mean"] + u["mu_star"]
    d_unit, d = (u["fstar"].astype(AB.LD) - mean).astype(np.float64), (w["fstar"].astype(AB.LD) - mean).astype(np.float64)
    err, tol = np.abs(d - a[None, :] * d_unit), AB.fstar_bound(a, mean, u["fstar"], w["fstar"])
    print(f"MEASURED {form}: max |(f* - mean) - a (f*_1 - mean)| / bound {np.max(err / tol):.3e}; max |f*_1 - mean| {np.abs(d_unit).max():.3f}")
    assert (err <= tol).all() and np.abs(d_unit).max() > 1e-3
    ones = a == 1.0
    assert u["fstar"][:, ones].tobytes() == w["fstar"][:, ones].tobytes()
    assert np.abs(d - d_unit)[:, ~ones].max() > 1e3 * tol.max()                       # a scaling that was left out shows
    # draw_f
    for s in pair:
        s.draw_f()
    nu_unit, nu = unit.get("nu"), scaled.get("nu")
    assert nu.tobytes() == np.asfortranarray(a[None, :] * nu_unit).tobytes()
    it = unit.iteration + 1
    us = X.item_uniforms(seed, it, 4, np.arange(m)[None, :], np.arange(4096)[:, None])         # GPIRT_ST_F_ESS
    for s, amp in ((unit, np.ones(m)), (scaled, a)):
        f1, k1 = s.get("f"), s.get("ess_k")
        for j in range(m):
            r = X.slice_exact(f0[:, j], y[:, j], amp[j] * nu_unit[:, j], mu[:, j], us[:, j], "exact")
            assert r["undecided"] == 0 and k1[j] == r["k"], (j, k1[j], r["k"])
            err = np.abs(f1[:, j].astype(X.LD) - r["f_new"]).astype(np.float64)
            assert (err <= r["f_err"]).all(), (j, err.max(), r["f_err"].max())
    assert np.abs(scaled.get("f") - unit.get("f"))[:, ~ones].max() > 1e-3
    for s in pair:
        s.check()
        s.close()


# ------------------------------------------------------------------------------------------ 6. failure and edges ---
@pytest.mark.parametrize("which", ["mixed", "one_inf", "one_overflow", "one_all_nan", "one_ordinary"])
def test_failed_items_and_prior_only_items(handles, which):
    """An item whose f holds an inf and an item whose c f overflows (it sits at index 0 with width 1: every proposal inside the
    grid scales it up) are counted failed with their columns byte-identical while the other items proceed; an item with every
    cell NaN is decided by the prior alone (dll = 0 exactly).  The same on m = 1."""
    n, P = 300, 5
    m = 4 if which == "mixed" else 1
    k0 = np.array([2, 0, 2, 2][:m]) if which != "one_overflow" else np.array([0])
    c = AB.case(n, m, P, 31, lo=0.25, hi=4.0, k=k0)
    f, y = c["f"].copy(order="F"), c["y"].copy(order="F")
    col = dict(mixed=dict(inf=0, over=1, nan=2), one_inf=dict(inf=0), one_overflow=dict(over=0), one_all_nan=dict(nan=0),
               one_ordinary={})[which]
    if "inf" in col:
        f[int(np.flatnonzero(np.isnan(y[:, col["inf"]]))[0]), col["inf"]] = np.inf          # an unobserved row counts too
    if "over" in col:
        f[7, col["over"]] = 1.7e308
    if "nan" in col:
        y[:, col["nan"]] = np.nan
    widths = np.ones(m, dtype=np.int32)
    s = _sampler(handles, c, 3, widths, f=f, y=y)
    got = _follow(s, c, 3, widths, 8, f, y=y)
    cn = got["counts"]
    if "inf" in col:
        assert cn[3, col["inf"]] == 8 and cn[1, col["inf"]] == 0
        assert s.get("f")[:, col["inf"]].tobytes() == f[:, col["inf"]].tobytes()
    if "over" in col:
        j = col["over"]
        assert cn[3, j] + cn[2, j] == 8 and cn[3, j] > 0 and cn[2, j] > 0 and s.amp_get("index")[j] == 0
        assert s.get("f")[:, j].tobytes() == f[:, j].tobytes()
    if "nan" in col:
        assert cn[1, col["nan"]] > 0 and cn[3, col["nan"]] == 0
    if which in ("mixed", "one_ordinary"):
        assert cn[3, m - 1] == 0 and cn[0, m - 1] - cn[2, m - 1] > 0                # the ordinary item is decided on its merits
    if which == "mixed":
        assert cn[1, 3] > 0                                                         # ... and moves beside the failed ones
    s.check()                                                                       # a failed update is not an error
    s.close()


def test_prior_only_item_record(handles):
    """every cell NaN: dll is exactly 0 and log_ratio exactly the prior's difference"""
    from gpirt_amd import amp as A
    c = AB.case(70, 2, 5, 33, lo=0.25, hi=4.0)
    y = c["y"].copy(order="F")
    y[:, 1] = np.nan
    s = _sampler(handles, c, 6, np.ones(2, dtype=np.int32), y=y)
    k = c["k"].copy()
    for t in range(1, 7):
        ref = A.step_exact(s.get("f"), c["mu"], y, k, 1, 6, t, c["grid"], c["log_prior"])
        s.draw_amp()
        rec = s.amp_get("record")
        if ref["status"][1] != "out_of_range":
            assert rec[0, 1] == 0.0 and rec[1, 1] == c["log_prior"][ref["k_prop"][1]] - c["log_prior"][k[1]]
        k = ref["k"]
        assert np.array_equal(s.amp_get("index"), k)
    s.close()


# ------------------------------------------------------------------------------------------------- 7. interplay ---
def test_whitened_draw_ell_does_not_see_the_amplitudes_and_centred_is_refused(handles):
    from gpirt_amd import _lib
    from gpirt_amd.sampler import Sampler
    c = EB.case(70, 3, 5, 3)
    out = []
    for amp in (None, np.array([0.5, 2.0, 3.0])):
        s = Sampler(handles(dict(family="se", length_scale=float(c["grid"][c["k"]]))), c["y"], c["theta"], seed=9, **FAST)
        s.init()
        s.set("f", c["f"]); s.set("beta", c["beta"]); s.set("mu", c["mu"])
        s.ell_enable(c["lo"], c["hi"], c["points"], c["log_prior"], 1)
        if amp is not None:
            s.amp_set(amp)
        for _ in range(3):
            s.draw_ell()
        out.append(dict(record=s.ell_get("record").tobytes(), f=s.get("f").tobytes(), e=s.ell()))
        if amp is not None:
            with pytest.raises(_lib.GpirtError, match=r"1 / a_j\^2"):
                s.draw_ell("centred")
            s.amp_set(None)
        s.draw_ell("centred")                                           # amplitudes off: it runs
        s.check()
        s.close()
    assert out[0]["record"] == out[1]["record"] and out[0]["f"] == out[1]["f"]
    assert out[0]["e"]["index"] == out[1]["e"]["index"] and out[0]["e"]["accepted"] == out[1]["e"]["accepted"]


def test_refusals(handles):
    from gpirt_amd import _lib
    from gpirt_amd.distributed import ShardedSampler
    from gpirt_amd.ops import RStream
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(64, 4, seed=2)
    ones = np.ones(4)

    def both(s, word):
        with pytest.raises(_lib.GpirtError, match=word) as e:
            s.amp_set(ones)
        assert e.value.code == _lib.E_ARG
        with pytest.raises(_lib.GpirtError, match=word):
            s.amp_enable()

    s = Sampler(handles(), y, th0, rng="reference", rstream=RStream(3))
    s.init()
    both(s, "R's stream has no such draw")
    s.close()
    s = Sampler(handles(), y, th0, seed=2, kernel_fp32=True)
    s.init()
    both(s, "kernel_fp32")
    s.close()
    s = Sampler(handles(), y, th0, seed=2, item0=4, m_total=8, **FAST)
    s.init()
    both(s, "item shard")
    s.close()
    for name in ("amp_set", "amp_enable", "draw_amp"):
        with pytest.raises(ValueError, match="not offered for item shards"):
            getattr(ShardedSampler, name)(object(), *((ones,) if name == "amp_set" else ()))
    s = Sampler(handles(), y, th0, seed=2, **FAST)
    with pytest.raises(_lib.GpirtError, match="initialised"):
        s.amp_set(ones)
    s.init()
    with pytest.raises(_lib.GpirtError, match="not enabled"):
        s.draw_amp()
    with pytest.raises(_lib.GpirtError, match="not enabled"):
        s.amp_get("amplitude")
    for bad in (0.009, 1001.0, np.nan, np.inf):
        with pytest.raises(_lib.GpirtError, match=r"a\[2\]"):
            s.amp_set([1.0, 1.0, bad, 1.0])
    s.amp_set(ones * 2)
    with pytest.raises(_lib.GpirtError, match="after gpirt_sampler_amp_set"):
        s.amp_enable()
    with pytest.raises(_lib.GpirtError, match="not enabled"):
        s.draw_amp()
    with pytest.raises(_lib.GpirtError, match="not enabled"):
        s.amp_get("index")
    assert np.array_equal(s.amp_get("amplitude"), ones * 2)
    s.amp_set(None)
    s.amp_enable(0.5, 2.0, 5, planned_draws=1)
    with pytest.raises(_lib.GpirtError, match="after gpirt_sampler_amp_enable"):
        s.amp_set(ones)
    with pytest.raises(_lib.GpirtError, match=r"width\[1\] = 5"):
        s.amp_width([1, 5, 1, 1])
    s.amp_record()
    with pytest.raises(_lib.GpirtError, match="planned draws are recorded"):
        s.amp_record()
    other = Sampler(s.handle, y, th0, seed=2, **FAST)
    other.init()
    for dst, src in ((other, s), (s, other)):
        with pytest.raises(_lib.GpirtError, match="amplitudes are on"):
            dst.copy_state_from(src)
    s.amp_enable(on=False)
    assert s.amp()["mode"] is None
    other.copy_state_from(s)
    other.close()
    s.close()


def test_record_follows_the_index_series(handles):
    """amp_record after every update: draws holds the index series row for row and hist its counts, a rejected update's
    repeated index included; enabling again zeroes the counters and the buffers but not the call count"""
    from gpirt_amd import amp as A
    c = AB.case(40, 3, 9, 14, lo=0.25, hi=4.0)
    T = 25
    s = _sampler(handles, c, 4, np.full(3, 2, dtype=np.int32), planned=T)
    ks = np.empty((T, 3), dtype=np.int32)
    for t in range(T):
        s.draw_amp()
        s.amp_record()
        ks[t] = s.amp_get("index")
        assert s.amp_get("draws").shape == (t + 1, 3)
    assert np.array_equal(s.amp_get("draws"), ks)
    assert (np.diff(ks, axis=0) == 0).any() and (np.diff(ks, axis=0) != 0).any()        # repeats after a reject, moves after an accept
    hist = s.amp_get("hist")
    assert hist.dtype == np.uint32 and np.array_equal(hist, np.stack([np.bincount(ks[:, j], minlength=9) for j in range(3)], axis=1))
    a = s.amp()
    assert a["recorded"] == T == a["planned_draws"] and a["calls"] == T
    s.amp_enable(c["lo"], c["hi"], c["points"], c["log_prior"], 2, ks[-1], planned_draws=2)
    a = s.amp()
    assert a["updates"] == 0 and a["recorded"] == 0 and a["calls"] == T and not s.amp_get("hist").any()
    ref = A.step_exact(s.get("f"), c["mu"], c["y"], ks[-1], 2, 4, T + 1, c["grid"], c["log_prior"])       # t goes on: T + 1
    s.draw_amp()
    assert np.array_equal(s.amp_get("index"), ref["k"])
    s.close()


# -------------------------------------------------------------------------------------------------- 8. the run ---
def test_run_is_deterministic_and_its_summaries_are_summarise(handles):
    """amp.run at 96 x 12, two chains, 30 + 30 iterations, twice: a byte-identical res["amp"], whose summaries are `summarise` of
    the returned draws; fixed=... runs amp_set and no update; kernel.compare takes amplitude= in a candidate"""
    from gpirt_amd import amp as A, kernel as K
    from gpirt_amd.synthetic import make_responses
    y, _ = make_responses(96, 12, seed=2)
    kw = dict(chains=2, seed=3, points=33, width=3, top=4)
    a = A.run(y, 30, 30, **kw)
    b = A.run(y, 30, 30, **kw)

    def same(x, z):
        if isinstance(x, dict):
            return x.keys() == z.keys() and all(same(x[k], z[k]) for k in x)
        if isinstance(x, (list, tuple)):
            return len(x) == len(z) and all(same(p, q) for p, q in zip(x, z))
        if isinstance(x, np.ndarray):
            return x.dtype == z.dtype and x.tobytes() == z.tobytes()
        return x == z or (x != x and z != z)

    assert same(a["amp"], b["amp"])
    for k in ("theta", "beta", "f", "IRFs"):
        assert a[k].tobytes() == b[k].tobytes(), k
    e = a["amp"]
    g = A.grid(0.1, 10.0, 33)
    assert e["mode"] == "sampled" and e["draws"].shape == (2, 30, 12) and ((e["draws"] >= 0) & (e["draws"] < 33)).all()
    assert np.array_equal(e["grid"], g) and np.array_equal(e["amplitude"], g[e["draws"]])
    hist = np.stack([np.bincount(e["draws"][:, :, j].ravel(), minlength=33) for j in range(12)], axis=1)
    assert np.array_equal(e["hist"], hist)
    want = A.summarise(e["draws"], hist, g)
    want["mode_amplitude"] = want.pop("mode")
    for k, v in want.items():
        assert same(e[k], v), k
    assert e["counts"].shape == (2, 4, 12) and (e["counts"][:, 0] == 60).all() and (e["counts"][:, 3] == 0).all()
    assert e["accept_rate"].shape == e["width"].shape == (2, 12)
    assert [r["item"] for r in e["smallest"]] == list(np.argsort(e["mean"], kind="stable")[:4]) and len(e["largest"]) == 4
    assert np.isfinite(a["IRFs"]).all() and a["theta"].shape == (2, 31, 96)
    print(f"MEASURED amp.run: mean amplitude {e['mean'].round(2).tolist()}, accept {e['accept_rate'].mean():.3f}, widths "
          f"{e['width'][0].tolist()}")
    fx = A.run(y, 4, 2, seed=3, fixed=2.0)
    assert fx["amp"]["mode"] == "fixed" and np.array_equal(fx["amp"]["amplitude"], np.full(12, 2.0))
    one = A.run(y, 4, 2, seed=3, fixed=1.0)
    plain = K.run(y, 4, 2, seed=3, loo=False)
    assert one["f"].tobytes() == plain["f"].tobytes() and fx["f"].tobytes() != plain["f"].tobytes()
    rows = K.compare(y, [dict(family="se", amplitude=0.5), "se"], 40, 10, chains=1, seed=3)
    assert {r["index"] for r in rows} == {0, 1} and all(np.isfinite(r["elpd_loo"]) for r in rows)
    assert [("amplitude" in r) for r in sorted(rows, key=lambda r: r["index"])] == [True, False]
