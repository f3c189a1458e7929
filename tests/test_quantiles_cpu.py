"""Quantiles (include/gpirt_hip.h GPIRT_SUM_THETA_HIST, GPIRT_SUM_IRF_BAND, gpirt_summary_quantiles, gpirt_mcmc_run)
on a machine without a GPU: the entry points are exported and bound, the state block grows by exactly the new arrays, the
band edges, the argument checks, and the two NumPy routes -- over stored draws (scipy's ranks) and over the histograms
alone -- agree, with ties, odd S, 1..4 chains, reflection, constant chains and draws off the grid, and on a hand-worked
R-hat."""
import ctypes as C
import math
import os
import re
import statistics

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gpirt_irf_band_edges", "gpirt_summary_quantiles", "gpirt_mcmc_run")


@pytest.fixture(scope="module")
def lib():
    from gpirt_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def test_symbols_and_constants(lib):
    from gpirt_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpirt_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.gpirt_version() >= 106
    assert re.search(r"#define GPIRT_SUM_THETA_HIST\s+%d\b" % _lib.SUM_THETA_HIST, hdr)
    assert re.search(r"#define GPIRT_SUM_IRF_BAND\s+%d\b" % _lib.SUM_IRF_BAND, hdr)
    assert re.search(r"#define GPIRT_IRF_BINS\s+%d\b" % _lib.IRF_BINS, hdr)
    for i, k in enumerate(_lib.QNT_SCALARS):
        assert re.search(r"#define GPIRT_QNT_%s\s+%d\b" % (k.upper(), i), hdr), k
    assert re.search(r"#define GPIRT_QNT_NSCALARS\s+%d\b" % len(_lib.QNT_SCALARS), hdr)
    assert 64 not in _lib.SUM_PARTS.values()
    # the struct as the header lays it out: 2 ints, 10 pointers, the flags, the scalars, 4 reserved words
    assert C.sizeof(_lib.Quantiles) == 8 + 8 * 10 + 8 + 8 * len(_lib.QNT_SCALARS) + 32


def _bytes(lib, n, m, parts):
    b = C.c_int64()
    rc = lib.gpirt_summary_state_bytes(n, m, parts, C.byref(b))
    return rc, b.value


def _even(w):
    return w + (w & 1)


def test_state_block_grows_by_the_new_arrays(lib):
    from gpirt_amd import _lib
    n, m, G = 10, 3, 1001
    cells, tb = n * m, n + 2 * m
    # the existing parts' block, as the layout of DESIGN.md section 12 has it (header, moments, WAIC + y, f, IRF sum, DIAG)
    old = 8 + 2 * _even(tb) + 4 * _even(cells) + 2 * _even(cells) + _even(G * m) + 7 * _even(tb) + 7 * _even(cells)
    base = _lib.SUM_WAIC | _lib.SUM_F | _lib.SUM_DIAG
    assert _bytes(lib, n, m, base) == (0, 8 * old)
    hist = _even((n * G + 1) // 2)
    off = _even((n + 1) // 2)
    assert _bytes(lib, n, m, base | _lib.SUM_THETA_HIST) == (0, 8 * (old + 3 * hist + off))
    assert _bytes(lib, n, m, _lib.SUM_WAIC | _lib.SUM_THETA_HIST)[1] - _bytes(lib, n, m, _lib.SUM_WAIC)[1] == 8 * (hist + off)
    band = _even(G * m) + _even((G * m + 1) // 2) + _even((256 * G * m + 1) // 2)
    assert _bytes(lib, n, m, base | _lib.SUM_IRF_BAND) == (0, 8 * (old + band))
    assert _bytes(lib, n, m, base | _lib.SUM_IRF_BAND | _lib.SUM_THETA_HIST) == (0, 8 * (old + 3 * hist + off + band))
    assert _bytes(lib, n, m, 64)[0] == _lib.E_ARG                   # still unassigned
    assert _bytes(lib, 7, 5, _lib.SUM_THETA_HIST | _lib.SUM_IRF_BAND)[1] % 16 == 0


def test_band_edges(lib):
    from gpirt_amd.quantiles import band_edges, plogis
    e = band_edges()
    assert e.shape == (255,) and np.all(np.diff(e) > 0)
    assert np.abs(plogis(e) - np.arange(1, 256) / 256.0).max() <= 1e-15
    assert e[127] == 0.0
    assert lib.gpirt_irf_band_edges(None) != 0
    # within 4 ulp of the correctly rounded logit(b / 256) (log(b) - log(256 - b) was up to 109 ulp off near b = 128)
    import math
    import mpmath
    with mpmath.workprec(200):
        exact = [float(mpmath.log(mpmath.mpf(b) / (256 - b))) for b in range(1, 256)]
    for b, (got, want) in enumerate(zip(e, exact), 1):
        assert abs(got - want) <= 4 * math.ulp(want), (b, got, want)


def _mcmc_q(lib, chains=2, rng_item=True, rs=None, q=None, pooled_parts=None, probs=(0.1, 0.9), no_run=False):
    from gpirt_amd import _lib
    dp = C.POINTER(C.c_double)
    n, m = 4, 2
    y = np.ones((n, m), order="F")
    y[0, 0] = -1.0
    th = np.zeros((chains, n))
    p = np.full((2, m), 0.1, order="F")
    irf = np.zeros((1001, m), order="F")
    sm = _lib.Summary()
    sm.parts = _lib.SUM_WAIC if pooled_parts is None else pooled_parts
    o = _lib.default_options()
    if rng_item:
        o.rng_kind = _lib.RNG_ITEM
    pr = np.asarray(probs, dtype=np.float64)
    if q is None:
        q = _lib.Quantiles()
        q.nprobs = pr.size
        q.probs = pr.ctypes.data_as(dp)
    run = _lib.Run()
    run.rs = rs
    run.quantiles = C.pointer(q)
    return lib.gpirt_mcmc_run(y.ctypes.data_as(dp), n, m, th.ctypes.data_as(dp), chains, 4, 1, p.ctypes.data_as(dp),
                              p.ctypes.data_as(dp), p.ctypes.data_as(dp), C.byref(o), 1, _lib.TICK_FN(0), None, None,
                              None, None, irf.ctypes.data_as(dp), C.byref(sm), None, None if no_run else C.byref(run))


def test_argument_errors_and_no_device(lib):
    import torch
    from gpirt_amd import _lib
    dp = C.POINTER(C.c_double)
    assert lib.gpirt_summary_quantiles(None, 1, None, None, 1, None) == _lib.E_ARG
    q = _lib.Quantiles()
    assert lib.gpirt_summary_quantiles(None, 1, None, None, 1, C.byref(q)) == _lib.E_ARG
    assert _mcmc_q(lib, no_run=True) == _lib.E_ARG                              # run is required
    assert "bad argument" in _lib.last_error()
    assert _mcmc_q(lib, probs=(0.5, 1.5)) == _lib.E_ARG                         # a probability outside [0, 1]
    assert _mcmc_q(lib, probs=(float("nan"),)) == _lib.E_ARG
    assert _mcmc_q(lib, pooled_parts=_lib.SUM_WAIC | _lib.SUM_THETA_HIST) == _lib.E_ARG     # not a pooled part
    assert _mcmc_q(lib, pooled_parts=_lib.SUM_DIAG) == _lib.E_ARG
    assert _mcmc_q(lib, rng_item=False) == _lib.E_ARG                          # the R stream needs rs ...
    rs = C.c_void_p()
    assert lib.gpirt_rstream_create(C.byref(rs), 7) == 0
    try:
        assert _mcmc_q(lib, rng_item=False, rs=rs, chains=2) == _lib.E_ARG     # ... and one chain
        assert _mcmc_q(lib, rng_item=True, rs=rs, chains=1) == _lib.E_ARG      # the item RNG takes no rs
        if not torch.cuda.is_available():
            assert _mcmc_q(lib, rng_item=False, rs=rs, chains=1) == _lib.E_NODEVICE
    finally:
        lib.gpirt_rstream_destroy(rs)
    bad = _lib.Quantiles()
    pr = np.array([0.5])
    bad.nprobs, bad.probs = 1, pr.ctypes.data_as(dp)
    bad.reserved[2] = 1
    assert _mcmc_q(lib, q=bad) == _lib.E_ARG
    bad.reserved[2] = 0
    bad.reserved0 = 1
    assert _mcmc_q(lib, q=bad) == _lib.E_ARG
    bad.reserved0 = 0
    bad.nprobs, bad.probs = 2, None                                              # probabilities without their array
    assert _mcmc_q(lib, q=bad) == _lib.E_ARG
    # gpirt_summary has no place for the new parts' outputs: gpirt_mcmc_summary and gpirt_mcmc_chains still refuse them
    y, th, p1, irf = np.ones((4, 2), order="F"), np.zeros((2, 4)), np.full((2, 2), 0.1, order="F"), np.zeros((1001, 2), order="F")
    o = _lib.default_options()
    o.rng_kind = _lib.RNG_ITEM
    for bit in (_lib.SUM_THETA_HIST, _lib.SUM_IRF_BAND):
        sm = _lib.Summary()
        sm.parts = _lib.SUM_WAIC | bit
        assert lib.gpirt_mcmc_summary(y.ctypes.data_as(dp), 4, 2, th.ctypes.data_as(dp), 1, 0, p1.ctypes.data_as(dp),
                                      p1.ctypes.data_as(dp), p1.ctypes.data_as(dp), C.byref(o), None, _lib.TICK_FN(0), None,
                                      None, None, None, irf.ctypes.data_as(dp), C.byref(sm)) == _lib.E_ARG
        assert lib.gpirt_mcmc_chains(y.ctypes.data_as(dp), 4, 2, th.ctypes.data_as(dp), 2, 4, 1, p1.ctypes.data_as(dp),
                                     p1.ctypes.data_as(dp), p1.ctypes.data_as(dp), C.byref(o), 1, _lib.TICK_FN(0), None, None,
                                     None, None, irf.ctypes.data_as(dp), C.byref(sm), None) == _lib.E_ARG
        assert "bad argument" in _lib.last_error()
    # item shards do not offer the quantile parts (each rank's band would hold its own items only)
    from types import SimpleNamespace
    from gpirt_amd.distributed import ShardedSampler
    for parts in (("theta_hist",), ("waic", "irf_band")):
        with pytest.raises(ValueError):
            ShardedSampler.summary_enable(SimpleNamespace(engine=None), parts)
    if not torch.cuda.is_available():
        assert _mcmc_q(lib) == _lib.E_NODEVICE
        from gpirt_amd import gpirtMCMC
        with pytest.raises(_lib.GpirtError):
            gpirtMCMC(np.array([[1, 0], [0, 1], [1, 1], [0, 0]]), 4, 0, vote_codes=dict(yea=[1], nay=[0], missing=[None]),
                      rng="item", quantiles=(0.5,), store_draws=False)


# ------------------------------------------------------------------------------------------------- NumPy routes -------
def _grid_draws(rng, C_, S, n, spread=30, centre=500, step=1):
    """grid-valued theta draws (C, S, n) with many ties: k in a narrow band"""
    k = centre + step * rng.integers(-spread, spread + 1, size=(C_, S, n))
    return -5.0 + k.astype(np.float64) * 0.01


def _check_routes(th, f, probs, signs=None):
    from gpirt_amd import quantiles as Q
    e = Q.band_edges()
    S = th.shape[1]
    a = Q.from_draws(th, f, probs, signs=signs, edges=e)
    h = Q.histograms(th, f, edges=e)
    b = Q.from_histograms(draws=S, probs=probs, signs=signs, **h)
    for k in ("theta", "theta_median", "theta_mode", "theta_hist"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for k in ("bulk", "tail", "max"):
        np.testing.assert_allclose(a["theta_rhat"][k], b["theta_rhat"][k], rtol=1e-12, atol=1e-12, err_msg=k)
    if f is not None:
        np.testing.assert_allclose(a["irf"], b["irf"], rtol=0, atol=1e-14)
        np.testing.assert_allclose(a["irf_p_mean"], b["irf_p_mean"], rtol=1e-13)
        ok = ~np.isnan(a["irf_exact"])
        assert np.array_equal(ok, ~np.isnan(a["irf"]))
        assert np.abs(a["irf"][ok] - a["irf_exact"][ok]).max() <= 1.0 / 256 + 1e-12
    return a


@pytest.mark.parametrize("C_,S", [(1, 9), (2, 10), (3, 11), (4, 8), (2, 3)])
def test_histograms_equal_draws(C_, S):
    rng = np.random.default_rng(100 * C_ + S)
    n, m = 7, 3
    th = _grid_draws(rng, C_, S, n)
    f = rng.normal(scale=2.5, size=(C_, S, 1001, m))
    f[:, :, 5, 1] = 0.0                                                         # exactly on the middle edge
    a = _check_routes(th, f, (0.0, 0.025, 0.5, 0.975, 1.0))
    # the order statistics themselves
    T = C_ * S
    flat = np.sort(th.reshape(T, n), axis=0)
    for p, q in enumerate((0.0, 0.025, 0.5, 0.975, 1.0)):
        np.testing.assert_array_equal(a["theta"][p], flat[max(math.ceil(q * T), 1) - 1])
    if S < 4:
        assert np.isnan(a["theta_rhat"]["max"]).all()
    else:
        assert np.isfinite(a["theta_rhat"]["max"]).all()


def test_reflection_is_the_grid_reversed():
    from gpirt_amd import quantiles as Q
    rng = np.random.default_rng(5)
    th = _grid_draws(rng, 3, 12, 6, centre=650)
    th[1] = -th[1]                                                               # chain 1 in the mirror mode
    th[1] = -5.0 + Q.grid_index(th[1]) * 0.01                                    # back on the grid bit for bit
    f = rng.normal(size=(3, 12, 1001, 2))
    signs = [1, -1, 1]
    a = _check_routes(th, f, (0.1, 0.5, 0.9), signs=signs)
    # the same as the chain stored unreflected
    th2 = th.copy()
    th2[1] = -5.0 + (1000 - Q.grid_index(th[1])) * 0.01
    f2 = f.copy()
    f2[1] = f[1][:, ::-1]
    b = Q.from_draws(th2, f2, (0.1, 0.5, 0.9))
    for k in ("theta", "theta_median", "theta_hist"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_allclose(a["theta_rhat"]["max"], b["theta_rhat"]["max"], rtol=1e-13)
    np.testing.assert_array_equal(a["irf"], b["irf"])


def test_constant_chains_and_off_grid():
    from gpirt_amd import quantiles as Q
    rng = np.random.default_rng(9)
    th = _grid_draws(rng, 2, 10, 5)
    th[:, :, 0] = -5.0 + 0.01 * 321                                              # one value everywhere: W = 0 and B = 0 -> NaN
    th[0, :, 1] = -5.0 + 0.01 * 400                                              # each chain constant, the chains apart:
    th[1, :, 1] = -5.0 + 0.01 * 410                                              # W = 0, B > 0 -> +inf (bulk; the
    #                                                                              fold maps both to one distance: NaN)
    th[1, 3, 2] = 0.123456                                                       # off the grid
    th[0, 7, 3] = np.nan
    f = rng.normal(size=(2, 10, 1001, 2))
    f[1, 4, 17, 0] = np.nan
    a = _check_routes(th, f, (0.05, 0.5, 0.95))
    assert np.isnan(a["theta_rhat"]["bulk"][0]) and np.isnan(a["theta_rhat"]["max"][0])
    assert a["theta_rhat"]["bulk"][1] == np.inf and np.isnan(a["theta_rhat"]["tail"][1])
    assert np.isnan(a["theta_rhat"]["max"][1])
    for i in (2, 3):
        assert np.isnan(a["theta"][:, i]).all() and np.isnan(a["theta_median"][i]) and np.isnan(a["theta_rhat"]["max"][i])
    assert np.isfinite(a["theta"][:, 4]).all()
    assert np.isnan(a["irf"][:, 17, 0]).all() and np.isnan(a["irf_p_mean"][17, 0])
    assert np.isfinite(a["irf"][:, 16, 0]).all()
    h = Q.histograms(th, f)
    assert h["theta_off_grid"].sum() == 2 and h["irf_nan"].sum() == 1
    assert (h["theta_hist"].sum(axis=1) + h["theta_off_grid"] == 10).all()
    assert (h["irf_band"].sum(axis=1) + h["irf_nan"] == 10).all()


def test_hand_worked_rhat():
    """Two chains, S = 9 (the middle draw of each is in neither half), R-hat worked out with plain Python."""
    from gpirt_amd import quantiles as Q
    ks = [[10, 12, 12, 11, 30, 13, 12, 10, 11], [14, 12, 15, 15, 16, 14, 13, 15, 12]]
    th = (-5.0 + np.array(ks, dtype=np.float64) * 0.01)[:, :, None]
    nd = statistics.NormalDist()

    def rhat(vals):                                  # vals: the 2C = 4 halves of 4 draws each
        flat = sorted(v for h in vals for v in h)
        T = len(flat)
        rank = {v: (flat.index(v) + 1 + T - flat[::-1].index(v)) / 2.0 for v in flat}     # ties averaged
        z = [[nd.inv_cdf((rank[v] - 0.375) / (T + 0.25)) for v in h] for h in vals]
        N, M = 4, 4
        means = [sum(h) / N for h in z]
        grand = sum(means) / M
        B = N / (M - 1) * sum((x - grand) ** 2 for x in means)
        W = sum(sum((v - mu) ** 2 for v in h) / (N - 1) for h, mu in zip(z, means)) / M
        return math.sqrt(((N - 1) / N * W + B / N) / W)

    halves = [k[:4] for k in ks] + [k[5:] for k in ks]
    bulk = rhat(halves)
    allk = sorted(ks[0] + ks[1])                     # R's median of the 18 draws: (9th + 10th) / 2 = (12 + 13) / 2
    s2 = allk[8] + allk[9]
    assert s2 == 25
    tail = rhat([[abs(2 * v - s2) for v in h] for h in halves])
    a = Q.from_draws(th, None, (0.5,))
    b = Q.from_histograms(draws=9, probs=(0.5,), **Q.histograms(th))
    for r in (a, b):
        assert abs(r["theta_rhat"]["bulk"][0] - bulk) <= 1e-12
        assert abs(r["theta_rhat"]["tail"][0] - tail) <= 1e-12
        assert abs(r["theta_rhat"]["max"][0] - max(bulk, tail)) <= 1e-12
        assert r["theta"][0, 0] == -5.0 + 0.01 * 12 and r["theta_mode"][0] == -5.0 + 0.01 * 12
