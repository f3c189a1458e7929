"""The autocorrelation ESS on the device (csrc/acf.hip) against the NumPy statement of the header (gpirt_amd.acf.from_draws):
constructed draws through Sampler.set("theta" | "beta" | "f" | "mu") and acf_accumulate() with no stepping -- the raw arrays bit
for bit, the log-likelihood pass and the finish inside tests/_acf_bounds.py's bounds --, a real chain through the stage API with
the chain untouched, chains pooled with reflection signs, and the refusals.

The shapes put P across a wave, a 256-thread work-group and the boundary between theta's integer section and the doubles; S = 40
wraps the ring of L + 1 slots many times, L = 19 = H - 1 fills every lag, S = 41 has a middle draw.  Every comparison prints the
largest used fraction of its bound ("MEASURED ...")."""
import numpy as np
import pytest

import _acf_bounds as B

pytestmark = pytest.mark.gpu
RAW = ("s", "sum", "head", "tail", "centre", "nonfinite", "ring")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def feed(handle, c, S, L, parts="all"):
    """the constructed draws of c through a sampler: (sampler, the S x P values the device read)"""
    from gpirt_amd import Sampler
    n, m = c["y"].shape
    s = Sampler(handle, c["y"], np.zeros(n), rng="item", seed=5, theta_stabilise=True)
    s.init()
    s.acf_enable(parts, S, L)
    last = []
    for t in range(S):
        s.set("theta", c["theta"][t])
        s.set("beta", c["beta"][t])
        s.set("f", c["f"][t])
        s.set("mu", c["mu"][t])
        s.acf_accumulate()
        last.append(s.acf_get("last"))
    return s, np.stack(last)


def check_ll_pass(c, last, name):
    """item_ll, resp_ll and total_ll as the device formed them, against long double inside ll_bounds"""
    n, m = c["y"].shape
    used = 0.0
    for t in range(last.shape[0]):
        bound, want = B.ll_bounds(c["f"][t] + c["mu"][t], c["y"])
        err = np.abs(last[t, -(m + n + 1):] - np.asarray(want, dtype=np.float64))
        used = max(used, float((err / np.maximum(bound, 1e-300)).max()))
    print(f"MEASURED {name}: the log-likelihood pass uses {used:.3f} of its bound")
    assert used <= 1.0


def check_finish(got, want, name):
    bd = B.finish_bounds(want)
    live = want["constant"] == 0
    assert np.array_equal(got["constant"], want["constant"]) and np.array_equal(got["nonfinite"], want["nonfinite"])
    for k in ("ess", "tau", "mcse", "rhat", "rho1", "mean", "sd"):
        sel = live if k != "mean" else np.ones_like(live)            # (sd of a constant value: sqrt(var+) exactly, below)
        err = np.abs(got[k][sel] - want[k][sel])
        assert np.isfinite(bd[k][sel]).all(), k
        used = float((err / np.maximum(bd[k][sel], 1e-300)).max()) if sel.any() else 0.0
        print(f"MEASURED {name}: {k} uses {used:.3f} of its bound")
        assert used <= 1.0, k
        assert same_bits(got[k][~sel], want[k][~sel])
    err = np.abs(got["acf"][:, live] - want["acf"][:, live])
    assert (err <= bd["acf"][:, live]).all() and np.isnan(got["acf"][:, ~live]).all()
    ok = bd["decided"] & live
    left_out = 1.0 - ok[live].mean()
    print(f"MEASURED {name}: lag_used / truncated left out for {left_out:.4f} of the values")
    assert left_out <= 0.02
    assert np.array_equal(got["lag_used"][ok], want["lag_used"][ok]) and np.array_equal(got["truncated"][ok], want["truncated"][ok])
    assert (got["lag_used"][~live] == 0).all() and (got["truncated"][~live] == 0).all()
    # the block folds and the worst values follow exactly from the device's own per-value arrays
    for bname, sl in want["slices"].items():
        e, b = got["ess"][sl], got["blocks"][bname]
        assert b["n_nan"] == int(np.isnan(e).sum()) and b["n_truncated"] == int(got["truncated"][sl].sum()), bname
        if (~np.isnan(e)).any():
            assert b["min_ess"] == np.nanmin(e) and b["max_tau"] == np.nanmax(got["tau"][sl]), bname
            assert b["max_rhat"] == np.nanmax(got["rhat"][sl]), bname
        else:
            assert np.isnan(b["min_ess"]) and np.isnan(b["max_tau"]) and np.isnan(b["max_rhat"]), bname
    e = got["ess"]
    order = [p for p in np.lexsort((np.arange(e.size), e)) if not np.isnan(e[p])][:len(got["worst"]["ess"])]
    starts = {k: v.start for k, v in want["slices"].items()}
    for r, p in enumerate(order):
        w = got["worst"]
        assert w["ess"][r] == e[p] and starts[w["block_name"][r]] + w["index"][r] == p, r


@pytest.mark.parametrize("S,L", B.RUNS)
@pytest.mark.parametrize("n,m", B.SHAPES)
def test_constructed_draws(handle, n, m, S, L):
    from gpirt_amd import acf as AC
    name = f"{n}x{m}-S{S}-L{L}"
    c = B.constructed(n, m, S, seed=n + S + L)
    s, last = feed(handle, c, S, L)
    try:
        assert same_bits(last[:, :n], c["theta"]) and same_bits(last[:, n:n + 2 * m], c["beta"].transpose(0, 2, 1).reshape(S, 2 * m))
        check_ll_pass(c, last, name)
        want = AC.from_draws(c["theta"], c["beta"], None, c["y"], planned=S, max_lag=L, ll=last[:, -(m + n + 1):], top=9)
        counts = s.acf_get("counts")
        assert list(counts) == [n, m, 7, S, S // 2, L, 2 * n + 3 * m + 1, S]
        for k in RAW:
            assert same_bits(s.acf_get(k), want["raw"][0][k]), k
        check_finish(s.acf(top=9), want, name)
    finally:
        s.close()


def test_saturated_log_likelihood_is_bit_for_bit_from_g_alone(handle):
    """|g| >= 800: exp(-|g|) is exactly 0, a cell's ll exactly 0 or -|g|, so NumPy's own evaluation has the device's bits and the
    whole state follows from the draws alone -- the order of the row sums, the tree and the folds included (n = 300 rows: two
    work-groups along i, the second with empty lanes; m = 37: two along j)"""
    from gpirt_amd import acf as AC
    n, m, S, L = 300, 37, 12, 5
    c = B.constructed(n, m, S, seed=8, saturated=True)
    s, last = feed(handle, c, S, L, parts="ll")
    try:
        want = AC.from_draws(None, None, c["f"] + c["mu"], c["y"], planned=S, max_lag=L)
        assert same_bits(last, np.stack([AC.ll_series(c["f"][t] + c["mu"][t], c["y"]) for t in range(S)]))
        for k in RAW:
            assert same_bits(s.acf_get(k), want["raw"][0][k]), k
        check_finish(s.acf(), want, "saturated")
    finally:
        s.close()


@pytest.mark.parametrize("parts", ["theta", "beta", ("theta", "ll")])
def test_parts_alone(handle, parts):
    from gpirt_amd import acf as AC
    n, m, S, L = 65, 31, 12, 4
    c = B.constructed(n, m, S, seed=21)
    s, last = feed(handle, c, S, L, parts=parts)
    try:
        names = (parts,) if isinstance(parts, str) else parts
        want = AC.from_draws(c["theta"] if "theta" in names else None, c["beta"] if "beta" in names else None, None, c["y"],
                             planned=S, max_lag=L, ll=last[:, -(m + n + 1):] if "ll" in names else None)
        for k in RAW:
            assert same_bits(s.acf_get(k), want["raw"][0][k]), k
        check_finish(s.acf(), want, "+".join(names))
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------- a real chain ---
N_, M_, S_, L_ = 65, 31, 12, 5


def run_chain(handle, y, init, seed, acf_on, keep=False):
    from gpirt_amd import Sampler
    s = Sampler(handle, y, init, preset="fast", seed=seed)
    s.init()
    s.ppc_enable()
    if acf_on:
        s.acf_enable("all", S_, L_)
    draws = dict(theta=[], beta=[], g=[], last=[])
    for _ in range(S_):
        s.step()
        s.accumulate_irf()
        s.ppc_accumulate()
        if acf_on:
            s.acf_accumulate()
            if keep:
                draws["last"].append(s.acf_get("last"))
        if keep:
            draws["theta"].append(s.get("theta"))
            draws["beta"].append(s.get("beta"))
            draws["g"].append(s.get("f") + s.get("mu"))
    s.check()
    end = dict(theta=s.get("theta"), beta=s.get("beta"), f=s.get("f"), irf_sum=s.get("irf_sum"),
               ppc=s.ppc_state().cpu().numpy().tobytes())
    return s, {k: np.stack(v) for k, v in draws.items() if v}, end


@pytest.fixture(scope="module")
def real(handle):
    from gpirt_amd import _lib
    y = B.make_y(N_, M_, 77)
    inits = np.random.default_rng(4).normal(size=(3, N_))
    samplers, draws, ends = [], [], []
    for c in range(3):
        s, d, e = run_chain(handle, y, inits[c], _lib.chain_seed(17, c), True, keep=True)
        samplers.append(s)
        draws.append(d)
        ends.append(e)
    yield dict(y=y, inits=inits, samplers=samplers, draws=draws, ends=ends)
    for s in samplers:
        s.close()


def test_real_chain_raw_arrays_match_the_statement(real):
    from gpirt_amd import acf as AC
    n, m = N_, M_
    for c in range(3):
        d = real["draws"][c]
        assert same_bits(d["last"][:, :n], d["theta"]) and same_bits(d["last"][:, n:n + 2 * m], d["beta"].transpose(0, 2, 1).reshape(S_, 2 * m))
        check_ll_pass(dict(y=real["y"], f=d["g"], mu=np.zeros_like(d["g"])), d["last"], f"chain {c}")
        want = AC.from_draws(d["theta"], d["beta"], None, real["y"], planned=S_, max_lag=L_, ll=d["last"][:, -(m + n + 1):])
        for k in RAW:
            assert same_bits(real["samplers"][c].acf_get(k), want["raw"][0][k]), (c, k)
        assert (want["nonfinite"] == 0).all()


def test_the_chain_is_untouched_and_the_state_repeats(handle, real):
    from gpirt_amd import _lib
    s, _, end = run_chain(handle, real["y"], real["inits"][1], _lib.chain_seed(17, 1), False)
    s.close()
    for k, v in end.items():
        w = real["ends"][1][k]
        assert (v == w) if isinstance(v, bytes) else same_bits(v, w), k
    s, _, end = run_chain(handle, real["y"], real["inits"][1], _lib.chain_seed(17, 1), True)
    block = s.acf_state().cpu().numpy().tobytes()
    s.close()
    assert block == real["samplers"][1].acf_state().cpu().numpy().tobytes()
    for k, v in end.items():
        w = real["ends"][1][k]
        assert (v == w) if isinstance(v, bytes) else same_bits(v, w), k


@pytest.mark.parametrize("signs", [(1, -1), (1, -1, 1)])
def test_chains_pooled_with_signs(handle, real, signs):
    from gpirt_amd import acf as AC
    C_ = len(signs)
    n, m = N_, M_
    d = real["draws"][:C_]
    want = AC.from_draws(np.stack([x["theta"] for x in d]), np.stack([x["beta"] for x in d]), None, real["y"], planned=S_,
                         max_lag=L_, signs=signs, ll=np.stack([x["last"][:, -(m + n + 1):] for x in d]), top=12)
    got = AC.combine(handle, real["samplers"][:C_], signs=signs, top=12)
    assert got["chains"] == C_ and got["N"] == 2 * C_ * (S_ // 2) and got["L"] == L_
    check_finish(got, want, f"C = {C_} pooled")
    # a sign changes what it should: theta's means flip, the log-likelihood series do not notice
    plain = AC.combine(handle, real["samplers"][:C_], top=12)
    sl = got["slices"]
    assert not np.array_equal(plain["mean"][sl["theta"]], got["mean"][sl["theta"]])
    for k in ("ess", "tau", "mean", "rhat"):
        assert same_bits(plain[k][sl["item_ll"].start:], got[k][sl["item_ll"].start:]), k


def test_run_is_the_stage_api_in_one_call(handle):
    """acf.run: chain c from default_inits with chain_seed(seed, c), DIAG beside the block, the signs from chains.combine"""
    from gpirt_amd import Sampler, _lib, chains
    from gpirt_amd import acf as AC
    y = B.make_y(N_, M_, 77)
    S, Bn, seed, L = 8, 2, 17, 3
    got = AC.run(y, S, Bn, chains=2, seed=seed, max_lag=L, top=5, handle=handle)
    inits = chains.default_inits(N_, 2, seed)
    samplers = []
    for c in range(2):
        s = Sampler(handle, y, inits[c], preset="fast", seed=_lib.chain_seed(seed, c))
        s.init()
        s.summary_enable(_lib.SUM_THETA_BETA | _lib.SUM_DIAG, planned_draws=S)
        s.acf_enable("all", S, L)
        for it in range(S + Bn):
            s.step()
            if it >= Bn:
                s.summary_accumulate()
                s.acf_accumulate()
        s.check()
        samplers.append(s)
    refl = chains.combine(handle, samplers)["diagnostics"]["reflected"]
    want = AC.combine(handle, samplers, signs=[-1 if r else 1 for r in refl], top=5)
    for s in samplers:
        s.close()
    assert np.array_equal(got["reflected"], refl) and got["chains"] == 2 and got["S"] == S and got["L"] == L
    for k in ("ess", "tau", "mcse", "rhat", "rho1", "mean", "sd", "lag_used", "truncated", "nonfinite", "constant", "acf"):
        assert same_bits(got[k], want[k]), k
    assert got["blocks"] == want["blocks"] or all(
        same_bits(np.array(list(got["blocks"][b].values())), np.array(list(want["blocks"][b].values()))) for b in want["blocks"])
    assert same_bits(got["worst"]["ess"], want["worst"]["ess"]) and got["worst"]["block_name"] == want["worst"]["block_name"]


def test_refusals(handle, real):
    from gpirt_amd import Sampler, _lib
    from gpirt_amd import acf as AC
    from gpirt_amd.distributed import ShardedSampler
    s = Sampler(handle, real["y"], np.zeros(N_), rng="item", seed=5, theta_stabilise=True)
    s.init()
    try:
        with pytest.raises(ValueError, match="no planned draws"):
            s.acf_enable("all")
        with pytest.raises(ValueError, match="fewer than 4"):
            s.acf_enable("all", 7)
        with pytest.raises(ValueError, match=r"min\(H - 1, 1024\) = 5"):
            s.acf_enable("all", 12, 6)
        with pytest.raises(Exception, match="not enabled"):
            s.acf_accumulate()
        s.acf_enable("theta", 8, 3)
        for _ in range(8):
            s.acf_accumulate()
        with pytest.raises(Exception, match="all 8 planned draws are in"):
            s.acf_accumulate()
        buf = np.zeros(1)
        assert s.lib.gpirt_sampler_acf_get(s._s, b"nope", buf.ctypes.data, 8) == _lib.E_ARG
        assert "unknown acf field" in _lib.last_error()
        s.acf_enable("theta", 10, 3)
        s.acf_accumulate()
        with pytest.raises(Exception, match="holds 1 of its 10 planned draws"):
            s.acf()
        with pytest.raises(Exception, match="another n, m, parts, S or L"):
            for _ in range(9):
                s.acf_accumulate()
            AC.combine(handle, [s, real["samplers"][0]])
        with pytest.raises(Exception, match="not \\+1 or -1"):
            AC.combine(handle, [s], signs=[0])
        s.acf_enable(on=False)
        with pytest.raises(Exception, match="not enabled"):
            s.acf_state()
    finally:
        s.close()
    with pytest.raises(ValueError, match="not offered for item shards"):
        ShardedSampler.acf_enable(None, "all", 40)
