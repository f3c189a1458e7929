"""Item-pair order posteriors on the device (csrc/order.hip) against the NumPy statement of the header
(gpirt_amd.shape.order_from_draws): real chains at the edges in m (the tile width, 64, and 32 should it ever change) and in the
window, constructed curves through set("gbar"), skipped draws, pooling, determinism, the untouched chain, gpirtMCMC end to end
and the refusals.  n = 33 throughout: the grid is fixed at 1001 points, so the edges are in m and in k.

above, cross, depth_sum, set_counts, draws and the last u are compared with ==; e within tests/_order_bounds.py's bound; easier
bit for bit with the device's own e, and with the long-double statement for every pair further apart than twice the bound."""
import ctypes as C

import numpy as np
import pytest

import _order_bounds as OB

pytestmark = pytest.mark.gpu
N_RESP = 33
NG = 1001
K = np.arange(NG)
TH = -5.0 + K * 0.01
BASE = (K - 500) / 64.0                     # exact in fp64, and so is BASE + c for the small dyadic c used below
CODES = dict(yea=[1], nay=[-1], missing=[None])
TOLS = (0.0, 0.25, 1.0)
RAW = ("above", "cross", "easier", "depth_sum", "easiness", "set_counts")
KC = 32                                     # the pair kernel's k-chunk


def sampler_kw(form):
    from gpirt_amd.ops import RStream
    if form == "fast":                      # item RNG, fused, rank-64 K*
        return dict(preset="fast", seed=2**33 + 5)
    if form == "as_written":                # item RNG, draw_fstar as the reference writes it
        return dict(rng="item", seed=77, theta_stabilise=True, fstar_fused=False, kstar_rank=0)
    return dict(rng="reference", rstream=RStream(41), theta_stabilise=False)


def responses(m, seed=7):
    from gpirt_amd.synthetic import make_responses
    return make_responses(N_RESP, m, seed=seed + m, na_frac=0.03)


def accumulate(s, draws):
    """set each curve draw and accumulate; the device's e after each counted draw"""
    es = []
    for g in draws:
        s.set("gbar", g)
        s.shape_accumulate()
        if np.isfinite(g).all():
            es.append(s.shape_order_get("e"))
    return np.array(es).reshape(len(es), s.m)


def check_all(s, got, want, dev_e, label, need_all=True):
    """got = s.shape_order(); the exact arrays, the getters, u, ncross, e and easier"""
    OB.check_exact(got, want, label)
    for k in RAW:
        raw = s.shape_order_get(k)
        assert raw.dtype == got[k].dtype and raw.tobytes() == got[k].tobytes(), (label, k)
    assert s.shape_order_get("counts").tolist() == [want["draws"], want["skipped"]]
    assert (s.shape_order_get("u") == want["u"]).all(), label
    assert s.shape_order_get("ncross").tolist() == want["ncross"].tolist(), label
    easier_dev = OB.check_easiness(dev_e, want, label, need_all)
    from gpirt_amd import shape
    assert np.array_equal(got["easier"], easier_dev) and np.array_equal(easier_dev, shape.order_ranks_from_easiness(dev_e)), label
    if need_all:
        assert np.array_equal(got["easier"], want["easier"]), label
    # easiness: the sums of the device's e and e^2 in draw order
    acc = np.zeros((2, dev_e.shape[1]))
    for e in dev_e:
        acc += np.stack([e, e * e])
    assert np.array_equal(got["easiness"], acc), label
    for k in ("p_above", "p_cross", "p_tied", "depth_mean", "cross_items_mean", "p_iio", "cross_pairs_mean", "cross_pairs_sd"):
        assert np.array_equal(got[k], want[k], equal_nan=True), (label, k)         # host functions of the exact arrays
    assert np.array_equal(got["worst"]["pairs"], want["worst"]["pairs"]), label     # the library's list against NumPy's


@pytest.mark.parametrize("m,window,form", [(2, 0.01, "fast"), (3, 3.0, "reference"), (31, 5.0, "as_written"), (32, 3.0, "fast"),
                                           (33, 0.01, "as_written"), (63, 3.0, "reference"), (64, 5.0, "fast"),
                                           (65, 3.0, "as_written"), (65, 0.01, "reference"), (129, 3.0, "fast"),
                                           (129, 5.0, "reference")])
def test_real_chains_against_order_from_draws(handle, m, window, form):
    from gpirt_amd import Sampler, shape
    y, th0 = responses(m)
    steps = 3
    s = Sampler(handle, y, th0, **sampler_kw(form))
    s.init()
    s.shape_enable(window=window, tols=TOLS)
    s.shape_order_enable()
    curves, es = [], []
    for _ in range(steps):
        s.step()
        s.shape_accumulate()
        curves.append(s.get("gbar"))
        es.append(s.shape_order_get("e"))
        one = shape.order_from_draws(curves[-1][None], window, TOLS)
        assert (s.shape_order_get("u") == one["u"]).all()                # the last u after every step
    s.check()
    curves = np.stack(curves)
    assert np.isfinite(curves).all()
    want = shape.order_from_draws(curves, window, TOLS, top=7)
    got = s.shape_order(top=7)
    label = f"chain {N_RESP}x{m} window {window} {form}"
    check_all(s, got, want, np.array(es), label)
    assert shape.order_state_header(s.shape_order_state()) == dict(tag=0x5244524F, version=1, n=N_RESP, m=m,
                                                                   k_half=int(round(100 * window)), tols=list(TOLS),
                                                                   draws=steps, skipped=0)
    assert s.shape_order_state().numel() * 8 == shape.order_state_bytes(m, len(TOLS))
    s.close()


def constructed_columns(window):
    """Crossings only at k_lo, only at k_hi, only outside W, at the k-chunk boundaries +- 1; gaps exactly equal to each
    tolerance; identical columns; columns that differ only by -0.0; |g| = 800; a large smooth curve; and 60 lines through the
    origin so that the pairs span more than one tile.  Column 0 is BASE."""
    k_half = int(round(100 * window))
    klo, khi = 500 - k_half, 500 + k_half
    zig = np.where(K % 2 == 0, 0.25, -0.25)

    def spike(*ks):
        c = BASE - 1.0
        for k in ks:
            if 0 <= k <= 1000:
                c[k] = BASE[k] + 1.0
        return c

    cols = [BASE, spike(klo), spike(khi), spike(klo - 1, khi + 1)]
    cols += [spike(min(klo + KC + d, khi)) for d in (-1, 0, 1)] + [spike(min(klo + 9 * KC + d, khi)) for d in (-1, 0, 1)]
    cols += [BASE + 0.25, BASE + 1.0, BASE + zig, BASE + 4.0 * zig, BASE.copy()]
    cols += [np.zeros(NG), np.where(K % 2 == 0, -0.0, 0.0), np.where(K < 500, -800.0, 800.0), np.full(NG, 800.0),
             np.full(NG, -800.0), 1e3 * np.sin(2.0 * TH)]
    cols += [BASE * (1.0 + j / 8.0) for j in range(1, 61)]
    return np.stack(cols, axis=1), klo, khi


@pytest.mark.parametrize("window", [0.01, 3.0, 5.0])
def test_constructed_curves_and_skipped_draws(handle, window):
    """The constructed curves, twice (the second time with the columns reversed); then a draw with a NaN at k = 0 in one column
    and one with +-inf inside W: after each the state is byte-identical except that `skipped` is one higher, and u, e and ncross
    still hold the last counted draw; then the first draw again."""
    from gpirt_amd import Sampler, shape
    G, klo, khi = constructed_columns(window)
    m = G.shape[1]
    assert m > 64
    y, th0 = responses(m)
    s = Sampler(handle, y, th0, preset="fast", seed=3)
    s.init()
    s.shape_enable(window=window, tols=TOLS)
    s.shape_order_enable()
    first = [G, G[:, ::-1].copy()]
    es = [accumulate(s, first[:1])]
    dev_easier = s.shape_order_get("easier")
    assert dev_easier[14, 0] == dev_easier[0, 14] == 0 and dev_easier[15, 16] == dev_easier[16, 15] == 0    # neither is easier
    es = [np.concatenate([es[0], accumulate(s, first[1:])])]
    want = shape.order_from_draws(np.stack(first), window, TOLS)
    check_all(s, s.shape_order(), want, es[0], f"constructed window {window}", need_all=False)
    one = shape.order_from_draws(G[None], window, TOLS)
    a, c, u = one["above"], one["cross"], one["u"]
    assert c[:, 1, 0].tolist() == [1, 1, 0] and c[:, 2, 0].tolist() == [1, 1, 0]           # at k_lo only, at k_hi only
    if window < 5.0:
        assert not c[:, 3, 0].any() and a[:, 0, 3].tolist() == [1, 1, 0]                   # outside W: not counted
    assert u[10, 0] == 0.25 and a[:, 10, 0].tolist() == [1, 0, 0] and u[11, 0] == 1.0 and a[:, 11, 0].tolist() == [1, 1, 0]
    assert c[:, 12, 0].tolist() == [1, 0, 0] and c[:, 13, 0].tolist() == [1, 1, 0]
    assert not a[:, 14, 0].any() and not a[:, 0, 14].any() and not c[:, 14, 0].any()       # identical: tied
    assert not a[:, 15, 16].any() and not a[:, 16, 15].any() and not c[:, 15, 16].any()    # -0.0 against 0.0: tied
    assert np.isfinite(es[0]).all() and abs(es[0][0, 18] - 1.0) < 1e-12 and es[0][0, 19] == 0.0    # |g| = 800

    def snapshot():
        return (s.shape_order_state().cpu().numpy().copy(), s.shape_order_get("u"), s.shape_order_get("e"), s.shape_order_get("ncross"))

    nan0 = G.copy(); nan0[0, 5] = np.nan
    infs = G.copy(); infs[500, 2] = np.inf; infs[501, 70] = -np.inf
    for k, bad in enumerate((nan0, infs)):
        before = snapshot()
        accumulate(s, [bad])
        after = snapshot()
        assert after[0][11] == before[0][11] + 1 == k + 1
        after[0][11] = before[0][11]
        for x, z in zip(before, after):
            assert x.tobytes() == z.tobytes()
    es.append(accumulate(s, [G]))
    draws = first + [nan0, infs, G]
    want = shape.order_from_draws(np.stack(draws), window, TOLS)
    got = s.shape_order()
    assert (got["draws"], got["skipped"]) == (3, 2)
    check_all(s, got, want, np.concatenate(es), f"constructed window {window} with skipped draws", need_all=False)
    s.close()


def run_chain(handle, y, th0, kw, steps, burn=0, window=3.0):
    from gpirt_amd import Sampler
    s = Sampler(handle, y, th0, **kw)
    s.init()
    s.shape_enable(window=window, tols=TOLS)
    s.shape_order_enable()
    curves = []
    for it in range(steps + burn):
        s.step()
        if it >= burn:
            s.shape_accumulate()
            curves.append(s.get("gbar"))
    s.check()
    return s, np.stack(curves)


def test_pooling_and_determinism(handle):
    """order_combine over three states equals order_from_draws of the chains' curves (U's arrays with ==; depth_sum added in
    chain order on both sides); two identical runs give byte-identical states; mismatching windows are refused."""
    from gpirt_amd import _lib, shape
    m = 65
    y, th0 = responses(m)
    runs = [run_chain(handle, y, th0, dict(preset="fast", seed=sd), 3) for sd in (5, 6, 5)]
    assert runs[0][0].shape_order_state().cpu().numpy().tobytes() == runs[2][0].shape_order_state().cpu().numpy().tobytes()
    assert runs[0][0].shape_order_state().cpu().numpy().tobytes() != runs[1][0].shape_order_state().cpu().numpy().tobytes()
    pooled = shape.order_combine(handle, [r[0] for r in runs], top=64)
    want = shape.order_from_draws([r[1] for r in runs], 3.0, TOLS, top=64)
    OB.check_exact(pooled, want, "three states pooled")
    assert np.array_equal(pooled["easier"], want["easier"])
    assert np.array_equal(pooled["worst"]["pairs"], want["worst"]["pairs"]) and len(pooled["worst"]["pairs"]) == 64
    # 1530 EPS of e (tests/_order_bounds.py), twice that for e^2, the additions the same on both sides
    assert (np.abs(pooled["easiness"] - want["easiness"]) <= 2 * 1530 * OB.EPS * want["easiness"]).all()
    two = shape.order_combine(handle, [runs[0][0].shape_order_state(), runs[1][0].shape_order_state().clone()])
    OB.check_exact(two, shape.order_from_draws([runs[0][1], runs[1][1]], 3.0, TOLS), "two states pooled")
    other, _ = run_chain(handle, y, th0, dict(preset="fast", seed=5), 1, window=2.0)
    with pytest.raises(_lib.GpirtError, match="window"):
        shape.order_combine(handle, [runs[0][0], other])
    for s in [r[0] for r in runs] + [other]:
        s.close()


@pytest.mark.parametrize("case", ["item_chains", "reference"])
def test_gpirtmcmc_equals_the_stage_loop(handle, case):
    """gpirtMCMC(..., shape=dict(order=True)) -- under the item RNG from the verified checkpoint's gbar, two chains pooled --
    equals the stage-API loop with the same seeds bit for bit."""
    from gpirt_amd import _lib, gpirtMCMC, shape
    from gpirt_amd.ops import RStream
    m, S, Bn, seed = 33, 4, 2, 29
    y, th0 = responses(m, seed=11)
    spec = dict(window=3.0, tols=TOLS, order=True, order_top=6)
    if case == "item_chains":
        inits = np.stack([th0, 0.5 * th0])
        res = gpirtMCMC(y, S, Bn, vote_codes=CODES, theta_init=inits, rng="item", seed=seed, theta_stabilise=True, chains=2,
                        shape=spec, store_draws=False)
        runs = [run_chain(handle, y, inits[c], dict(rng="item", seed=_lib.chain_seed(seed, c), theta_stabilise=True), S, Bn)
                for c in range(2)]
    else:
        res = gpirtMCMC(y, S, Bn, vote_codes=CODES, theta_init=th0, rng="reference", rstream=RStream(77), shape=spec)
        runs = [run_chain(handle, y, th0, dict(rng="reference", rstream=RStream(77), theta_stabilise=False), S, Bn)]
    od = res["shape"]["order"]
    pooled = shape.order_combine(handle, [r[0] for r in runs], top=6)
    for k in RAW:
        assert od[k].tobytes() == pooled[k].tobytes(), k
    assert (od["draws"], od["skipped"]) == (len(runs) * S, 0)
    assert np.array_equal(od["worst"]["pairs"], pooled["worst"]["pairs"]) and len(od["worst"]["pairs"]) == 6
    OB.check_exact(od, shape.order_from_draws([r[1] for r in runs], 3.0, TOLS), case)
    for k in ("p_above", "p_cross", "p_tied", "p_easier", "depth_mean", "easiness_mean", "easiness_sd", "rank_mean", "order",
              "cross_items_mean", "p_iio", "cross_pairs_mean", "cross_pairs_sd"):
        assert k in od, k
    assert np.isnan(np.diagonal(od["p_easier"])).all() and np.array_equal(od["rank_mean"], 1.0 + od["easier"].sum(axis=0) / od["draws"])
    for r in runs:
        r[0].close()


@pytest.mark.parametrize("case", ["fast", "reference"])
def test_chain_untouched(case):
    """With and without order: theta, beta, f, f*, the IRFs, the shape block and R's stream position are bitwise equal."""
    from gpirt_amd import gpirtMCMC
    from gpirt_amd.ops import RStream
    m, S, Bn = 31, 4, 2
    y, th0 = responses(m, seed=31)
    kw = dict(vote_codes=CODES, theta_init=th0)
    seeds = [None, None]
    if case == "fast":
        kw.update(preset="fast", seed=9, chains=2, theta_init=None)
    else:
        seeds = [RStream(77), RStream(77)]
    res = []
    for k, sh in enumerate((True, dict(order=True))):
        extra = dict(rstream=seeds[k]) if seeds[k] is not None else {}
        res.append(gpirtMCMC(y, S, Bn, shape=sh, **kw, **extra))
    plain, with_order = res
    assert "order" not in plain["shape"] and "order" in with_order["shape"]
    for k in ("theta", "beta", "f", "fstar", "IRFs"):
        if k in plain:
            assert np.array_equal(plain[k], with_order[k], equal_nan=True), k
    if case == "reference":
        (mt0, i0), (mt1, i1) = seeds[0].state(), seeds[1].state()
        assert i0 == i1 and np.array_equal(mt0, mt1)
    for k, v in plain["shape"].items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == with_order["shape"][k].tobytes(), k
    assert plain["shape"]["info_draws"] == with_order["shape"]["info_draws"] == with_order["shape"]["order"]["draws"]


def test_refusals(handle):
    from gpirt_amd import Sampler, _lib, gpirtMCMC, shape
    from gpirt_amd.distributed import ShardedSampler
    y, th0 = responses(3)
    s = Sampler(handle, y, th0, preset="fast", seed=1)
    s.init()
    with pytest.raises(_lib.GpirtError, match="need the shape posteriors"):
        s.shape_order_enable()
    s.shape_enable()
    with pytest.raises(_lib.GpirtError, match="not enabled"):
        s.shape_order_get("u")
    s.shape_order_enable()
    with pytest.raises(_lib.GpirtError, match="unknown order field"):
        s.shape_order_get("nope")
    for top in (0, 65):
        with pytest.raises(ValueError, match="order_top"):
            s.shape_order(top=top)
        with pytest.raises(ValueError, match="order_top"):
            gpirtMCMC(y, 2, 1, vote_codes=CODES, preset="fast", shape=dict(order=True, order_top=top))
        r, keep = shape.order_struct(3, 3)                  # (keep: the host arrays behind r)
        r.top = top
        ptrs = (C.c_void_p * 1)(s.shape_order_state().data_ptr())
        assert s.lib.gpirt_shape_order_combine(handle.ptr, 1, ptrs, C.byref(r)) == _lib.E_ARG and "top" in _lib.last_error()
    with pytest.raises(ValueError, match="unknown keys"):
        gpirtMCMC(y, 2, 1, vote_codes=CODES, preset="fast", shape=dict(order=True, ordr=1))
    s.shape_enable()                                        # again: the order block goes with the old shape state
    with pytest.raises(_lib.GpirtError, match="not enabled"):
        s.shape_order_state()
    s.shape_order_enable()
    s.shape_order_enable(on=False)
    with pytest.raises(_lib.GpirtError, match="not enabled"):
        s.shape_order_state()
    s.step(); s.shape_accumulate(); s.check()               # the shape block alone still runs
    s.close()
    y1, th1 = responses(1)
    s = Sampler(handle, y1, th1, preset="fast", seed=1)
    s.init()
    s.shape_enable()
    with pytest.raises(_lib.GpirtError, match="2..4096"):
        s.shape_order_enable()
    s.close()
    with pytest.raises(_lib.GpirtError, match="2..4096"):
        gpirtMCMC(y1, 2, 1, vote_codes=CODES, preset="fast", shape=dict(order=True))
    with pytest.raises(ValueError, match="not offered for item shards"):
        ShardedSampler.shape_order_enable(None)
