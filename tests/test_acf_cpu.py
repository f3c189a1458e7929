"""The autocorrelation ESS on the host: gpirt_amd.acf.from_draws (the NumPy statement of include/gpirt_hip.h's "autocorrelation
ESS" section) against a brute-force restatement -- raw sums by plain loops, gamma by direct centring in long double --, the
reflection identities, AR(1) recovery, the C struct against the header, the exports and every refusal of gpirt_acf_check.  No
device is needed."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import _acf_bounds as B
from gpirt_amd import _lib
from gpirt_amd import acf as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ld = np.longdouble


def brute(x, Pi, S, L, signs=None, flip=None):
    """x: C x S x P values (theta's first Pi columns as drawn).  Returns (raw per chain, finished dict) by plain loops: d by the
    header's rules, s / sum / head / tail term by term, gamma_k as the directly centred (1 / H) sum (d_t - dbar)(d_{t-k} - dbar)"""
    C_, _, P = x.shape
    H = S // 2
    raws, halves = [], []
    for c in range(C_):
        raw = dict(s=np.zeros((2, L + 1, P)), sum=np.zeros((2, P)), head=np.zeros((2, L + 1, P)), tail=np.zeros((2, L + 1, P)),
                   centre=np.zeros(P), nonfinite=np.zeros(P, dtype=np.int64))
        for p in range(P):
            col = x[c, :, p]
            if p < Pi:
                cen = 0.0
                d = []
                for v in col:
                    k = np.rint((v + 5.0) * 100.0)
                    ok = 0 <= k <= 1000 and -5.0 + k * 0.01 == v
                    d.append(int(k) - 500 if ok else None)
            else:
                cen = col[0] if np.isfinite(col[0]) else 0.0
                d = [(v - cen) if np.isfinite(v) else None for v in col]
            raw["centre"][p] = cen
            for h, lo in enumerate((0, S - H)):
                dh = d[lo:lo + H]
                raw["nonfinite"][p] += sum(v is None for v in dh)
                dh = [0 if v is None else v for v in dh]
                for k in range(L + 1):
                    acc = 0 if p < Pi else 0.0
                    for t in range(k, H):
                        acc = acc + dh[t] * dh[t - k]
                    raw["s"][h, k, p] = acc
                    head = 0 if p < Pi else 0.0
                    for t in range(k):
                        head = head + dh[t]
                    raw["head"][h, k, p] = head
                    tail = 0 if p < Pi else 0.0
                    for t in range(H - 1, H - 1 - k, -1):
                        tail = tail + dh[t]
                    raw["tail"][h, k, p] = tail
                tot = 0 if p < Pi else 0.0
                for v in dh:
                    tot = tot + v
                raw["sum"][h, p] = tot
                sg = -1 if (signs is not None and signs[c] < 0 and flip[p]) else 1
                halves.append((p, sg * np.asarray(dh, dtype=ld), sg * ld(cen)))
        raws.append(raw)
    M = 2 * C_
    gam = np.zeros((M, L + 1, P), dtype=ld)
    hm = np.zeros((M, P), dtype=ld)
    at = {p: 0 for p in range(P)}
    # halves were appended per chain, per value, per half: regroup as (half-chain, value)
    per = {}
    for p, dh, cen in halves:
        per.setdefault(p, []).append((dh, cen))
    for p in range(P):
        for c, (dh, cen) in enumerate(per[p]):
            dbar = dh.sum() / H
            hm[c, p] = cen + dbar
            e = dh - dbar
            for k in range(L + 1):
                gam[c, k, p] = (e[k:] * e[:H - k]).sum() / H
    del at
    gm = gam.mean(axis=0)
    W = gm[0] * H / ld(H - 1)
    varp = W * (H - 1) / ld(H) + hm.var(axis=0, ddof=1)
    with np.errstate(all="ignore"):
        rho = 1 - (W - gm) / varp
    rho[0] = 1
    N = M * H
    out = dict(tau=np.full(P, np.nan), ess=np.full(P, np.nan), lag_used=np.zeros(P, dtype=np.int64),
               truncated=np.zeros(P, dtype=np.int64), rho=rho, W=W, varp=varp, mean=hm.mean(axis=0), raw=raws)
    for p in range(P):
        if W[p] == 0 or varp[p] == 0 or not np.isfinite(W[p]) or not np.isfinite(varp[p]):
            continue
        tot, prev, j, trunc = ld(0), None, 0, 1
        while 2 * j + 1 <= L:
            pj = rho[2 * j, p] + rho[2 * j + 1, p]
            if pj <= 0:
                trunc = 0
                break
            if prev is not None:
                pj = min(pj, prev)
            tot, prev = tot + pj, pj
            out["lag_used"][p] = 2 * j + 1
            j += 1
        tau = max(-1 + 2 * tot, 1 / np.log10(ld(N)))
        out["tau"][p], out["ess"][p], out["truncated"][p] = tau, N / tau, trunc
    return out


def small_case(S, L, seed=3, chains=2):
    n, m = 5, 3
    xs = [B.constructed(n, m, S, seed + 10 * c) for c in range(chains)]
    y = xs[0]["y"]
    th = np.stack([x["theta"] for x in xs])
    be = np.stack([x["beta"] for x in xs])
    g = np.stack([x["f"] + x["mu"] for x in xs])
    g[0, 2, 1, 1] = np.nan                                            # a NaN log-likelihood: item 1, respondent 1 and the total
    return n, m, y, th, be, g


@pytest.mark.parametrize("S,L", [(40, 7), (41, 7), (40, 19), (12, 1)])
def test_from_draws_against_brute_force(S, L):
    n, m, y, th, be, g = small_case(S, L)
    out = AC.from_draws(th, be, g, y, planned=S, max_lag=L)
    P = out["P"]
    assert P == 2 * n + 3 * m + 1 and out["H"] == S // 2 and out["N"] == 4 * (S // 2)
    x = np.stack([AC.series_from_draws(th[c], be[c], g[c], y)[0] for c in range(2)])
    ref = brute(x, n, S, L)
    for c in range(2):
        for k in ("s", "sum", "head", "tail", "centre", "nonfinite"):
            assert np.array_equal(out["raw"][c][k], ref["raw"][c][k]), (c, k)
        assert (out["raw"][c]["s"][..., :n] == np.rint(out["raw"][c]["s"][..., :n])).all()
    # the special values: a constant theta and beta, the off-grid theta, the NaN beta, the NaN log-likelihoods
    sl = out["slices"]
    assert out["constant"][0] == 1 and out["constant"][sl["beta"].start] == 1 and np.isnan(out["ess"][0])
    assert out["nonfinite"][1] == 2 and out["nonfinite"][sl["beta"].start + 3] == 2
    for p in (sl["item_ll"].start + 1, sl["resp_ll"].start + 1, sl["total_ll"].start):
        assert out["nonfinite"][p] == 1 and out["constant"][p] == 0
    live = out["constant"] == 0
    assert live.sum() == P - 2
    # the identity between the raw-sum form of gamma and the directly centred one, in long double
    rho = np.asarray(out["acf"], dtype=np.float64)
    scale = 1 + np.abs(np.asarray(ref["rho"], dtype=np.float64))
    assert (np.abs(rho - np.asarray(ref["rho"], dtype=np.float64))[:, live] <= 1e-13 * scale[:, live]).all()
    assert np.allclose(out["tau"][live], ref["tau"][live], rtol=1e-12, atol=0)
    assert np.allclose(out["ess"][live], ref["ess"][live], rtol=1e-12, atol=0)
    assert np.array_equal(out["lag_used"][live], ref["lag_used"][live])
    assert np.array_equal(out["truncated"][live], ref["truncated"][live])
    assert np.allclose(out["mean"], np.asarray(ref["mean"], dtype=np.float64), rtol=1e-14, atol=1e-15)
    assert np.allclose(out["rhat"][live], np.sqrt(np.asarray(ref["varp"][live] / ref["W"][live], dtype=np.float64)), rtol=1e-13)
    assert np.allclose(out["mcse"][live], np.sqrt(np.asarray(ref["varp"], dtype=np.float64)[live] / ref["ess"][live]), rtol=1e-12)
    # the block folds and the worst values follow from the per-value arrays
    for name, s_ in sl.items():
        e = out["ess"][s_]
        b = out["blocks"][name]
        assert b["n_nan"] == int(np.isnan(e).sum()) and b["n_truncated"] == int(out["truncated"][s_].sum())
        assert b["min_ess"] == np.nanmin(e) and b["max_tau"] == np.nanmax(out["tau"][s_])
    w = out["worst"]
    held = ~np.isnan(w["ess"])
    assert held.sum() == min(20, live.sum()) and (w["block"][~held] == -1).all() and (w["index"][~held] == -1).all()
    assert (np.diff(w["ess"][held]) >= 0).all() and w["ess"][0] == np.nanmin(out["ess"])
    p0 = sl[w["block_name"][0]].start + w["index"][0]
    assert out["ess"][p0] == w["ess"][0]


def test_reflection_identities():
    S, L = 40, 7
    n, m, y, th, be, g = small_case(S, L)
    signs = [1, -1]
    got = AC.from_draws(th, be, g, y, planned=S, max_lag=L, signs=signs)
    th2, be2 = th.copy(), be.copy()
    th2[1] = -5.0 + (1000.0 - np.rint((th[1] + 5.0) * 100.0)) * 0.01  # the mirrored grid point, as the grid spells it
    th2[1, 3, 1] = 0.123456                                           # the off-grid value enters as 0 either way
    be2[1, :, 1] = -be2[1, :, 1]
    want = AC.from_draws(th2, be2, g, y, planned=S, max_lag=L)
    for k in ("s", "sum", "head", "tail", "centre"):
        assert np.array_equal(got["raw"][1][k], want["raw"][1][k], equal_nan=True), k
    for k in ("ess", "tau", "mcse", "rhat", "rho1", "mean", "sd", "acf"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    # and the signs matter: without them the reflected chain's theta means disagree
    plain = AC.from_draws(th2, be2, g, y, planned=S, max_lag=L, signs=[1, 1])
    flipped = AC.from_draws(th2, be2, g, y, planned=S, max_lag=L, signs=[1, -1])
    assert not np.array_equal(plain["rhat"][:n], flipped["rhat"][:n], equal_nan=True)
    assert np.array_equal(plain["ess"][got["slices"]["item_ll"]], flipped["ess"][got["slices"]["item_ll"]])


@pytest.mark.parametrize("phi", [0.0, 0.5, 0.9])
def test_ar1_tau_is_recovered(phi):
    rng = np.random.default_rng(17)
    C_, S, m = 4, 4000, 8
    x = np.zeros((C_, S, 2, m))
    e = rng.normal(size=(C_, S, 2, m))
    for t in range(1, S):
        x[:, t] = phi * x[:, t - 1] + e[:, t]
    out = AC.from_draws(None, x, None, np.ones((3, m)))
    want = (1 + phi) / (1 - phi)
    print(f"MEASURED tau at phi = {phi}: mean {out['tau'].mean():.3f} (exact {want:.3f}), L = {out['L']}")
    assert out["L"] == 256 and abs(out["tau"].mean() / want - 1) < 0.1 and out["truncated"].sum() == 0
    assert np.allclose(out["ess"], out["N"] / out["tau"]) and (out["rhat"] < 1.02).all()
    assert np.allclose(out["rho1"], phi, atol=0.06)


@pytest.mark.parametrize("n,m", B.SHAPES)
@pytest.mark.parametrize("S,L", B.RUNS)
def test_constructed_inputs_decide_lag_used(n, m, S, L):
    """what the GPU test relies on: the bounds of the constructed cases are finite and small, and at most 2 % of a case's values
    are too close to a tie for lag_used / truncated to be compared"""
    c = B.constructed(n, m, S, seed=n + S + L)
    out = AC.from_draws(c["theta"], c["beta"], c["f"] + c["mu"], c["y"], planned=S, max_lag=L)
    bd = B.finish_bounds(out)
    live = out["constant"] == 0
    empty = int(np.isnan(c["y"]).all(axis=1).sum())                   # a respondent without an answer: resp_ll is constant 0
    assert live.sum() == out["P"] - 2 - empty
    for k in ("ess", "tau", "mcse", "rhat", "sd", "mean", "rho1"):
        rel = bd[k][live] / np.maximum(np.abs(out[k][live]), 1e-300) if k != "mean" else bd[k][live]
        assert np.isfinite(bd[k][live]).all() and rel.max() < 1e-9, (k, rel.max())
    assert bd["acf"][:, live].max() < 1e-10
    left_out = (~bd["decided"][live]).mean()
    print(f"MEASURED undecided fraction {left_out:.4f}")
    assert left_out <= 0.02


def test_ll_series_matches_long_double():
    n, m = 300, 37
    c = B.constructed(n, m, 2, seed=5)
    g = c["f"][1] + c["mu"][1]
    got = AC.ll_series(g, c["y"])
    bound, want = B.ll_bounds(g, c["y"])
    assert (np.abs(got - np.asarray(want, dtype=np.float64)) <= bound).all()
    sat = B.constructed(n, m, 2, seed=5, saturated=True)
    gs = sat["f"][1]
    cell = np.where(np.isnan(sat["y"]) | (sat["y"] * gs > 0), 0.0, -np.abs(gs))
    assert AC.ll_series(gs, sat["y"])[-1] == pytest.approx(cell.sum(), rel=1e-13)


def _header_struct(name):
    """the (type, field, array length or None) triples of a struct of the header, in order"""
    src = open(os.path.join(ROOT, "include", "gpirt_hip.h")).read()
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(GPIRT_\w+)\s+(\d+)", src)}
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, rest = re.match(r"((?:const\s+)?\w+\s*\**)\s*(.*)", decl).groups()
        for item in rest.split(","):
            nm, dim = re.match(r"\s*(\w+)\s*(?:\[(.*?)\])?", item).groups()
            if dim is not None:
                dim = math.prod(int(defs.get(f.strip(), f.strip())) for f in dim.split("*"))
            out.append((typ.replace(" ", ""), nm, dim))
    return out, defs


def test_c_abi_of_version_122():
    lib = _lib.load()
    assert lib.gpirt_version() >= 122
    names = ("gpirt_acf_check", "gpirt_sampler_acf_enable", "gpirt_sampler_acf_accumulate", "gpirt_sampler_acf_get",
             "gpirt_sampler_acf_state", "gpirt_acf_combine")
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    ctype = {"double*": C.POINTER(C.c_double), "int64_t*": C.POINTER(C.c_int64), "int64_t": C.c_int64, "double": C.c_double}
    fields, defs = _header_struct("gpirt_acf")
    assert [f[1] for f in fields] == [f[0] for f in _lib.Acf._fields_]
    for (typ, nm, dim), (pn, pt) in zip(fields, _lib.Acf._fields_):
        assert pt is (ctype[typ] if dim is None else ctype[typ] * dim), nm
    assert C.sizeof(_lib.Acf) == 8 * (1 + 7 + 4 + 1 + 3 + 15 + 10 + 8 + 4)
    assert _lib.Acf.value.offset == 8 and _lib.Acf.acf.offset == 96 and _lib.Acf.block_stat.offset == 128
    assert _lib.Acf.n.offset == 328 and _lib.Acf.reserved.offset == 392
    assert (defs["GPIRT_ACF_THETA"], defs["GPIRT_ACF_BETA"], defs["GPIRT_ACF_LL"]) == (_lib.ACF_THETA, _lib.ACF_BETA, _lib.ACF_LL)
    assert (defs["GPIRT_ACF_MAX_LAG"], defs["GPIRT_ACF_DEFAULT_LAG"], defs["GPIRT_ACF_MAX_TOP"]) == (1024, 256, 64)
    assert defs["GPIRT_ACF_NARRAYS"] == len(_lib.ACF_RAW) and defs["GPIRT_ACF_NVALUE"] == len(_lib.ACF_VALUES)
    assert defs["GPIRT_ACF_NFLAG"] == len(_lib.ACF_FLAGS) and defs["GPIRT_ACF_NBLOCK"] == len(_lib.ACF_BLOCKS)
    # gpirt_run is still what tests/test_run_cpu.py fixes: 17 fields, 8 reserved slots -- the block is stage API only
    run, _ = _header_struct("gpirt_run")
    assert len(run) == 17 == len(_lib.Run._fields_) and run[-1][1:] == ("reserved", 8)


def test_every_refusal_of_the_check_comes_before_a_device():
    lib = _lib.load()
    L, P = C.c_int64(), C.c_int64()
    assert lib.gpirt_acf_check(8192, 1024, 7, 4000, 0, C.byref(L), C.byref(P)) == 0 and (L.value, P.value) == (256, 19457)
    assert lib.gpirt_acf_check(10, 3, 1, 9, 0, C.byref(L), C.byref(P)) == 0 and (L.value, P.value) == (3, 10)
    assert lib.gpirt_acf_check(10, 3, 6, 40, 19, C.byref(L), C.byref(P)) == 0 and (L.value, P.value) == (19, 6 + 3 + 10 + 1)
    assert lib.gpirt_acf_check(10, 3, 7, 5000, 1024, C.byref(L), None) == 0 and L.value == 1024
    for n, m, parts, S, lag, word in ((0, 3, 7, 40, 0, "must be at least 1"), (10, 0, 7, 40, 0, "must be at least 1"),
                                      (10, 3, 0, 40, 0, "non-empty mask"), (10, 3, 8, 40, 0, "non-empty mask"),
                                      (10, 3, 7, 0, 0, "no planned draws"), (10, 3, 7, 7, 0, "fewer than 4"),
                                      (10, 3, 7, 40, 20, "min(H - 1, 1024) = 19"), (10, 3, 7, 40, -1, "must lie in"),
                                      (10, 3, 7, 5000, 1025, "min(H - 1, 1024) = 1024")):
        assert lib.gpirt_acf_check(n, m, parts, S, lag, None, None) == _lib.E_ARG and word in _lib.last_error(), word
    r, _ = AC.struct(4, 2, top=3)
    assert lib.gpirt_acf_combine(None, 1, None, None, C.byref(r)) == _lib.E_ARG
    assert lib.gpirt_sampler_acf_enable(None, 7, 40, 0, 1) == _lib.E_ARG
    assert lib.gpirt_sampler_acf_accumulate(None) == _lib.E_ARG
    assert lib.gpirt_sampler_acf_get(None, b"counts", None, 0) == _lib.E_ARG
    assert lib.gpirt_sampler_acf_state(None, None, None) == _lib.E_ARG
    # the Python mirror refuses the same way
    for S, lag, word in ((None, None, "no planned draws"), (7, None, "fewer than 4"), (40, 20, "= 19"), (40, 0, "must lie in"),
                         (40, True, "must lie in")):
        with pytest.raises(ValueError, match=re.escape(word)):
            AC.lag_window(S, lag)
    assert AC.lag_window(40) == 19 and AC.lag_window(4000) == 256 and AC.lag_window(41, 7) == 7
    with pytest.raises(ValueError, match="unknown parts"):
        AC.parts_mask(["thetas"])
    with pytest.raises(ValueError, match="top must be"):
        AC.check_top(65)
    assert AC.parts_mask("all") == 7 and AC.parts_mask(("theta", "ll")) == 5 and AC.parts_mask(2) == 2


def test_sharded_sampler_refuses():
    from gpirt_amd.distributed import ShardedSampler
    with pytest.raises(ValueError, match="not offered for item shards"):
        ShardedSampler.acf_enable(None, "all", 40)
