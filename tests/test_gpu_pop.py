"""The population prior for theta on the device (include/gpirt_hip.h "a population prior for theta", csrc/pop.hip,
csrc/stages.hip theta_sample_kernel<true>, csrc/sampler.hip) against tests/_pop_exact.py and gpirt_amd/pop.py.

tests/test_pop_cpu.py shows without a GPU that the constructed draw_theta cases leave at most 1 % of their respondents, and the
update cases no hyper-draw, undecided under the derived bound of the device's rounding."""
import numpy as np
import pytest

import _pop_exact as PX
import _stage_exact as X

pytestmark = pytest.mark.gpu


def _rows(theta):
    return np.where(np.isnan(theta), -1, np.rint((theta + 5.0) / 0.01)).astype(np.int64)


def _data(n, m, seed):
    from gpirt_amd.synthetic import make_responses
    return make_responses(n, m, seed=seed)


# ------------------------------------------------------------------------------------------------------ as it was ---
@pytest.mark.parametrize("opts", [dict(preset="fast"), dict(rng="item")], ids=["fast", "default"])
def test_default_rows_change_no_bit_item_rng(handle, opts):
    from gpirt_amd import pop as PO
    from gpirt_amd.sampler import Sampler
    n, m = 257, 5
    y, th0 = _data(n, m, 41)
    out = []
    for G in (0, 1, 3):
        s = Sampler(handle, y, th0, seed=9, **opts)
        s.init()
        if G:
            s.pop_set(np.arange(n) % G, np.tile(PO.default_row(), (G, 1)))
            assert s.pop_stats()["mode"] == "fixed" and np.array_equal(s.pop_get("codes"), np.arange(n) % G)
        for _ in range(5):
            s.step()
        s.check()
        out.append({k: s.get(k).tobytes() for k in ("theta", "beta", "f", "fstar")})
        s.close()
    for k in ("theta", "beta", "f", "fstar"):
        assert out[0][k] == out[1][k] == out[2][k], k


def test_default_rows_change_no_bit_reference_rng(handle):
    from gpirt_amd import pop as PO
    from gpirt_amd.ops import RStream
    from gpirt_amd.sampler import Sampler
    n, m = 65, 4
    y, _ = _data(n, m, 42)
    out = []
    for G in (0, 1, 3):
        rs = RStream(77)
        th0 = rs.rnorm(n)
        s = Sampler(handle, y, th0, rng="reference", rstream=rs, theta_stabilise=False)
        s.init()
        if G:
            s.pop_set(np.arange(n) % G, np.tile(PO.default_row(), (G, 1)))
        for _ in range(5):
            s.step()
        s.check()
        mt, mti = rs.state()
        out.append(dict({k: s.get(k).tobytes() for k in ("theta", "beta", "f", "fstar")}, mt=mt.tobytes(), mti=mti))
        s.close()
    for k in ("theta", "beta", "f", "fstar", "mt", "mti"):
        assert out[0][k] == out[1][k] == out[2][k], k


# ------------------------------------------------------------------------------------------ draw_theta under a table ---
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("shape", PX.THETA_SHAPES)
def test_draw_theta_under_a_table(handle, shape, mode):
    from gpirt_amd.sampler import Sampler
    n, G = shape
    c = PX.theta_case(n, G)
    ref = PX.theta_exact_table(c["y"], c["fstar"], c["u"], True, c["codes"], c["table"], "fixed" if mode == 1 else "gemm")
    with handle.config("GPIRT_THETA_FIXED", mode):
        s = Sampler(handle, c["y"], np.zeros(n), rng="item", seed=PX.THETA_SEED, theta_stabilise=True)
        s.init()
        s.pop_set(c["codes"], c["table"])
        assert np.array_equal(s.pop_get("log_prior"), c["table"])
        s.set_iteration(PX.THETA_IT - 1)
        s.set("fstar", c["fstar"])
        s.theta_partial(); s.theta_finish()
        rows = _rows(s.get("theta"))
        s.check()                                                          # (a degenerate draw would be its named error)
        s.close()
    ok = ~ref["undecided"]
    bad = np.flatnonzero((rows != ref["index"]) & ok)
    print(f"MEASURED n={n} G={G} GPIRT_THETA_FIXED={mode}: undecided {int(ref['undecided'].sum())}, rows off {bad.size}, "
          f"degenerate {int((rows < 0).sum())} (reference {ref['degenerate']})")
    assert bad.size == 0, [(int(i), c["kinds"][c["codes"][i]], int(rows[i]), int(ref["index"][i])) for i in bad[:8]]
    assert ref["undecided"].sum() <= 0.01 * n
    assert int((rows < 0).sum()) == ref["degenerate"] == 0


# ------------------------------------------------------------------------------- the update from a constructed theta ---
def _update_sampler(handle, c, planned=0, seed=PX.UPDATE_SEED, **grid):
    from gpirt_amd.sampler import Sampler
    n = c["theta"].shape[0]
    y, _ = _data(max(n, 8), 3, 50 + n)
    s = Sampler(handle, y[:n], np.zeros(n), seed=seed, preset="fast")
    s.init()
    s.set("theta", c["theta"])
    s.pop_enable(c["codes"], c["G"], None, a0=c.get("a0"), b0=c.get("b0"), planned_draws=planned, **grid)
    return s


@pytest.mark.parametrize("case", PX.UPDATE_CASES)
def test_update_from_a_constructed_theta(handle, case):
    """One draw_pop against gpirt_amd.pop.step_exact: the statistics as integers, lp_mu, lp_sd and the rebuilt rows bit for
    bit, both indices (every draw of these inputs is decided, tests/test_pop_cpu.py).  n = 1 with G >= 2 cannot be -- every
    group has a member -- so the smallest case is n = 2, group 1 of one member."""
    from gpirt_amd import pop as PO
    n, G, P_mu, P_sd = case
    c = PX.update_case(*case)
    s = _update_sampler(handle, c, mu_hi=PX.MU_HI, points_mu=P_mu, sd_lo=PX.SD_LO, sd_hi=PX.SD_HI, points_sd=P_sd)
    mu, sd = PO.grids(PX.MU_HI, P_mu, PX.SD_LO, PX.SD_HI, P_sd)
    lse = s.pop_get("lse")
    assert np.array_equal(s.pop_get("mu_grid"), mu) and np.array_equal(s.pop_get("sd_grid"), sd)
    assert np.array_equal(lse, PO.lse_table(mu, sd))
    idx0, table0 = s.pop_get("index"), s.pop_get("log_prior")
    assert np.array_equal(idx0[1:], np.stack([c["a0"], c["b0"]], axis=1)[1:]) and (idx0[0] == -1).all()
    assert np.array_equal(table0[0], PO.default_row())
    assert np.array_equal(table0[1:], PO.normal_table(mu[c["a0"][1:]], sd[c["b0"][1:]]))
    ref = PO.step_exact(c["theta"], c["codes"], idx0, PX.UPDATE_SEED, 1, mu, sd, lse, log_prior=table0)
    s.draw_pop()
    st = s.pop_get("stats")
    assert np.array_equal(st, np.stack([ref["stats"][k] for k in ("n", "S1", "S2")])) and (s.pop_get("off_grid") == 0).all()
    lpm, lps, idx, table = s.pop_get("lp_mu"), s.pop_get("lp_sd"), s.pop_get("index"), s.pop_get("log_prior")
    assert ref["decided"].all() and ref["status"][1:] == ["updated"] * (G - 1)
    assert lpm[1:].tobytes() == ref["lp_mu"][1:].tobytes(), "lp_mu is not step_exact's bit for bit"
    assert np.array_equal(idx[:, 0], ref["index"][:, 0])
    assert lps[1:].tobytes() == ref["lp_sd"][1:].tobytes(), "lp_sd is not step_exact's bit for bit"
    assert np.array_equal(idx, ref["index"])
    assert table.tobytes() == ref["log_prior"].tobytes(), "the rebuilt rows are not the NumPy statement's bit for bit"
    cn = s.pop_get("counts")
    assert cn[0, 1:].tolist() == [1] * (G - 1) and cn[1, 1:].tolist() == [1] * (G - 1) and (cn[2:] == 0).all() and (cn[:, 0] == 0).all()
    p = s.pop_stats()
    assert p["mode"] == "sampled" and p["calls"] == 1 and p["updated"] == G - 1 and p["off_grid"] == 0
    s.check()
    s.close()


def test_off_grid_and_nan_members_leave_their_group_untouched(handle):
    from gpirt_amd import pop as PO
    c = PX.update_case(65, 4, 33, 17)
    theta = c["theta"].copy()
    i1, i2 = np.flatnonzero(c["codes"] == 1)[3], np.flatnonzero(c["codes"] == 2)[5]
    theta[i1], theta[i2] = 0.123456, np.nan
    c = dict(c, theta=theta)
    s = _update_sampler(handle, c, mu_hi=2.0, points_mu=33, sd_lo=0.3, sd_hi=3.0, points_sd=17)
    mu, sd = PO.grids(2.0, 33, 0.3, 3.0, 17)
    before = {k: s.pop_get(k) for k in ("index", "log_prior", "lp_mu", "lp_sd")}
    ref = PO.step_exact(theta, c["codes"], before["index"], PX.UPDATE_SEED, 1, mu, sd, s.pop_get("lse"), log_prior=before["log_prior"])
    assert ref["status"] == ["anchor", "skipped", "skipped", "updated"] and ref["decided"].all()
    s.draw_pop()
    after = {k: s.pop_get(k) for k in before}
    assert s.pop_get("off_grid").tolist() == [0, 1, 1, 0] and s.pop_stats()["off_grid"] == 2
    assert np.array_equal(s.pop_get("stats"), np.stack([ref["stats"][k] for k in ("n", "S1", "S2")]))
    for k in before:
        for g in (0, 1, 2):
            assert before[k][g].tobytes() == after[k][g].tobytes(), (k, g)
    assert np.array_equal(after["index"], ref["index"]) and after["log_prior"].tobytes() == ref["log_prior"].tobytes()
    assert after["lp_mu"][3].tobytes() == ref["lp_mu"][3].tobytes() and after["lp_sd"][3].tobytes() == ref["lp_sd"][3].tobytes()
    cn = s.pop_get("counts")
    assert cn[:, 1].tolist() == [1, 0, 1, 0] and cn[:, 2].tolist() == [1, 0, 1, 0] and cn[:, 3].tolist() == [1, 1, 0, 0]
    s.close()


# ------------------------------------------------------------------------------------------ frozen theta, many calls ---
def test_frozen_theta_many_calls(handle):
    """No step(): theta stays, so the (a, b) of a group are a Gibbs chain on `conditional`'s joint masses.  Per cell the count
    over N calls is within 5 binomial standard deviations sqrt(N p (1 - p)) of N p, p the cell's mass."""
    from gpirt_amd import pop as PO
    F = PX.FROZEN
    c = dict(PX.frozen_case(), G=F["G"])
    N, P, G = F["calls"], F["P"], F["G"]
    runs = []
    for _ in range(2):
        s = _update_sampler(handle, c, planned=N, seed=F["seed"], mu_hi=F["mu_hi"], points_mu=P, sd_lo=F["sd_lo"], sd_hi=F["sd_hi"],
                            points_sd=P)
        series = np.empty((N, G, 2), dtype=np.int32)
        for t in range(N):
            s.draw_pop()
            s.pop_record()
            if t % 500 == 0 or t == N - 1:
                series[t] = s.pop_get("index")
        runs.append({k: s.pop_get(k) for k in ("draws", "hist_mu", "hist_sd", "index", "log_prior", "lp_mu", "lp_sd", "counts")})
        lse, st = s.pop_get("lse"), s.pop_get("stats")
        assert s.pop_stats()["recorded"] == N and s.pop_stats()["calls"] == N
        with pytest.raises(Exception, match="planned draws are recorded"):
            s.pop_record()
        s.check()
        s.close()
    for k in runs[0]:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k
    d = runs[0]["draws"]
    for t in list(range(0, N, 500)) + [N - 1]:                              # the record buffer is the index series
        assert np.array_equal(d[t], series[t])
    assert (d[:, 0] == -1).all() and (runs[0]["counts"][1, 1:] == N).all()
    mu, sd = PO.grids(F["mu_hi"], P, F["sd_lo"], F["sd_hi"], P)
    for g in range(1, G):
        assert np.array_equal(runs[0]["hist_mu"][:, g], np.bincount(d[:, g, 0], minlength=P))
        assert np.array_equal(runs[0]["hist_sd"][:, g], np.bincount(d[:, g, 1], minlength=P))
        p = PO.conditional(st[0, g], st[1, g], st[2, g], mu, sd, lse).astype(np.float64)
        cnt = np.zeros((P, P))
        np.add.at(cnt, (d[:, g, 0], d[:, g, 1]), 1)
        dev = np.abs(cnt - N * p)
        lim = 5.0 * np.sqrt(N * p * (1.0 - p))
        worst = float((dev / np.maximum(lim, 1e-300)).max())
        print(f"MEASURED group {g}: worst |count - N p| / (5 binomial sd) {worst:.3f}; cells hit {int((cnt > 0).sum())}")
        assert (dev <= lim).all(), (g, np.argwhere(dev > lim)[:5].tolist())
    assert (runs[0]["hist_mu"][:, 0] == 0).all() and (runs[0]["hist_sd"][:, 0] == 0).all()


# ------------------------------------------------------------------------------------------------------------ a chain ---
def test_a_chain_follows_its_groups_theta(handle):
    """pop.run, n = 512 in two groups of 256, m = 32, group 1 generated about 1.5 with sd 0.5, 300 draws after 100 of burn-in,
    consistent=True.  Given theta_t, mu_1's draw has mean near group 1's mean theta_t and sd at most sd_hi / sqrt(n_g) (flat
    hyperprior, the Gibbs innovations independent given each theta), so over S draws
    |mean(mu_1) - mean_t(mean of group 1's theta_t)| <= 6 sd_hi / sqrt(n_g S) + one mu grid step.  Nothing about 1.5 is asserted."""
    from gpirt_amd import pop as PO
    n, m, S, B = 512, 32, 300, 100
    codes = (np.arange(n) >= 256).astype(np.int32)
    y, th0, _ = PO.make_grouped(n, m, codes, [0.0, 1.5], [1.0, 0.5], seed=8)
    res = PO.run(y, S, B, groups=codes, chains=1, seed=3, theta_init=th0, handle=handle, consistent=True)
    pop = res["pop"]
    assert res["consistent"] and pop["mode"] == "sampled" and pop["draws"].shape == (S, 2, 2) and pop["hist_mu"][:, 1].sum() == S
    assert (pop["counts"][0][1, 1] == S + B) and (pop["off_grid"] == 0).all()
    step = pop["mu_grid"][1] - pop["mu_grid"][0]
    sd_hi = pop["sd_grid"][-1]
    gap = abs(float(pop["mu"][:, 1].mean()) - float(res["group_theta_mean"][:, 1].mean()))
    bound = 6.0 * sd_hi / np.sqrt(256 * S) + step
    print(f"MEASURED mu_1 mean {pop['mu_mean'][1]:.4f} sd {pop['mu_sd'][1]:.4f}; sd_1 mean {pop['sd_mean'][1]:.4f} sd {pop['sd_sd'][1]:.4f}; "
          f"group 1 theta mean {float(res['group_theta_mean'][:, 1].mean()):.4f}; gap {gap:.4f} (bound {bound:.4f})")
    assert abs(pop["mu_mean"][1] - float(pop["mu"][:, 1].mean())) <= 1e-12
    assert gap <= bound


# ---------------------------------------------------------------------------------------------------------- refusals ---
def test_refusals(handle):
    from gpirt_amd import _lib, pop as PO
    from gpirt_amd.ops import RStream
    from gpirt_amd.sampler import Sampler
    n, m = 64, 4
    y, th0 = _data(n, m, 2)
    codes = np.arange(n) % 3
    tab = np.tile(PO.default_row(), (3, 1))

    def refused(fn, word):
        with pytest.raises(_lib.GpirtError, match=word) as e:
            fn()
        assert e.value.code == _lib.E_ARG

    s = Sampler(handle, y, th0, rng="reference", rstream=RStream(3))
    s.init()
    refused(lambda: s.pop_enable(codes), "R's stream has no such draw")
    s.pop_set(codes, tab)                                                  # fixed: both RNG contracts
    s.step(); s.check()
    s.close()
    s = Sampler(handle, y, th0, seed=2, item0=4, m_total=8, preset="fast")
    s.init()
    refused(lambda: s.pop_set(codes, tab), "item shard")
    refused(lambda: s.pop_enable(codes), "item shard")
    s.close()
    from gpirt_amd.distributed import ShardedSampler
    for name in ("pop_set", "pop_enable", "draw_pop"):
        with pytest.raises(ValueError, match="not offered for item shards"):
            getattr(ShardedSampler, name)(object(), *((codes,) if name != "draw_pop" else ()))
    s = Sampler(handle, y, th0, seed=2, preset="fast")
    s.init()
    s.set_theta_block(y[:8], 0, m)
    refused(lambda: s.pop_set(codes, tab), "gpirt_sampler_set_theta_block is in use")
    refused(lambda: s.pop_enable(codes), "gpirt_sampler_set_theta_block is in use")
    s.close()
    s = Sampler(handle, y, th0, seed=2, preset="fast")
    refused(lambda: s.pop_set(codes, tab), "initialised")
    refused(lambda: s.pop_enable(codes), "initialised")
    s.init()
    refused(s.draw_pop, "not enabled")
    refused(lambda: s.pop_get("codes"), "not enabled")
    bad = tab.copy()
    bad[1, 500] = np.nan
    refused(lambda: s.pop_set(codes, bad), r"log_prior\[1, 500\] is not finite")
    refused(lambda: s.pop_enable(codes, anchor_row=bad[1]), r"log_prior\[0, 500\] is not finite")
    refused(lambda: s.pop_set(codes, np.tile(tab[0], (4, 1))), "group 3 has no member")
    refused(lambda: s.pop_enable(codes, groups=4), "group 3 has no member")
    refused(lambda: s.pop_set(np.where(codes == 2, -1, codes), tab), "-1 is not allowed")
    refused(lambda: s.pop_set(np.arange(n) % 9, np.tile(tab[0], (9, 1))), "G = 9")
    refused(lambda: s.pop_enable(codes, points_mu=1), "each must lie in 2 .. 1024")
    refused(lambda: s.pop_enable(codes, points_sd=1025), "each must lie in 2 .. 1024")
    refused(lambda: s.pop_enable(codes, mu_hi=5.5), r"\(0, 5\]")
    refused(lambda: s.pop_enable(codes, mu_hi=0.0), r"\(0, 5\]")
    refused(lambda: s.pop_enable(codes, sd_lo=0.04), "sd_lo")
    refused(lambda: s.pop_enable(codes, sd_lo=2.0, sd_hi=2.0), "sd_lo")
    refused(lambda: s.pop_enable(codes, sd_hi=10.5), "sd_hi")
    assert s.pop_stats()["mode"] is None
    s.pop_set(codes, tab)
    refused(lambda: s.pop_enable(codes), "after gpirt_sampler_pop_set")
    refused(s.draw_pop, "not enabled")
    refused(lambda: s.pop_get("index"), "not enabled")
    refused(lambda: s.set_theta_block(y[:8], 0, m), "population prior is on")
    s.pop_set(None)
    s.pop_enable(codes, planned_draws=1)
    refused(lambda: s.pop_set(codes, tab), "after gpirt_sampler_pop_enable")
    refused(lambda: s.pop_set(None), "pop_enable\\(on = 0\\)")
    refused(lambda: s.pop_get("nothing"), "unknown population-prior array")
    s.step(); s.draw_pop(); s.pop_record()
    refused(s.pop_record, "planned draws are recorded")
    s.pop_enable(on=False)
    assert s.pop_stats()["mode"] is None and s.pop_stats()["calls"] == 1
    s.step()                                                               # the sampler is usable, the built-in prior again
    s.check()
    s.close()
