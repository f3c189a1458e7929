"""The centred amplitude update on the device (include/gpirt_hip.h "a centred amplitude update", csrc/amp_centred.hip,
csrc/sampler.hip, gpirt_amd.amp.centred_*): one update from constructed states against the long-double statement within the
bounds tests/_amp_centred_bounds.py derives, prior invariance with every answer missing, the byte-identical cases, determinism,
every refusal with its message, the one-call run, and mixing against the whitened update alone.  Every handle is the test's own."""
import numpy as np
import pytest

import _amp_centred_bounds as CB

pytestmark = pytest.mark.gpu

FAST = dict(rng="item", theta_stabilise=True, fstar_fused=True)
U = CB.U


@pytest.fixture
def handles():
    """make() -> a fresh Handle; all closed when the test ends"""
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


def _sampler(handles, c, seed, f=None, y=None, **kw):
    """a sampler in the constructed state of case c, the amplitudes on the grid at c's indices"""
    from gpirt_amd.sampler import Sampler
    s = Sampler(handles(), c["y"] if y is None else y, c["theta"], seed=seed, **dict(FAST, **kw))
    s.init()
    s.set("f", c["f"] if f is None else f)
    s.set("beta", c["beta"])
    s.set("mu", c["mu"])
    s.amp_enable(c["lo"], c["hi"], c["points"], c["log_prior"], 1, c["k"])
    s.check()
    return s


def _check_update(s, c, seed, t, f, y, k, counts):
    """one draw_amp_centred call (the t-th) from (f, k) against centred_exact_update fed the device's H and Q: k' where the draw
    is decided, c and f' and the committed column bit for bit, dll within its bound, the decision where decided, the counters.
    Returns (undecided items, the largest used fraction of dll's bound, the statuses, f and k afterwards, the call's H)."""
    from gpirt_amd import _lib, amp as A
    g, m = c["grid"], c["m"]
    s.draw_amp_centred()
    H, Q = s.amp_get("centred_H"), s.amp_get("centred_Q")
    rec, idx, f_dev = s.amp_get("record_centred"), s.amp_get("index"), s.get("f")
    r = s.amp_get("rank")
    up = A.centred_exact_update(H, Q, f, c["mu"], y, k, seed, t, g, c["log_prior"], r)
    undecided, worst, seen = 0, 0.0, []
    k_new = k.copy()
    for j in range(m):
        st = _lib.AMP_CENTRED_STATUS[int(rec[4, j])]
        seen.append(st)
        counts[0, j] += 1
        if st != "rejected":
            counts[_lib.AMP_CENTRED_STATUS.index(st), j] += 1      # rows: updates, accepted, same, failed
        assert rec[0, j] == Q[j] or (np.isnan(rec[0, j]) and np.isnan(Q[j]))
        if not up["draw_decided"][j]:
            undecided += 1
            k_new[j] = idx[j]
            continue
        if up["status"][j] == "failed" and up["k_prop"][j] < 0:
            assert st == "failed" and rec[1, j] == -1 and f_dev[:, j].tobytes() == f[:, j].tobytes()
            continue
        assert rec[1, j] == up["k_prop"][j], (t, j, rec[1, j], up["k_prop"][j])
        if up["status"][j] == "same":
            assert st == "same" and np.isnan(rec[2, j]) and np.isnan(rec[3, j]) and idx[j] == k[j]
            assert f_dev[:, j].tobytes() == f[:, j].tobytes()
            continue
        kp = int(up["k_prop"][j])
        with np.errstate(all="ignore"):
            fp = H[:, j] + (g[kp] / g[k[j]]) * (f[:, j] - H[:, j])                     # c and f': the statement's own bits
        assert fp.tobytes() == up["f"][:, j].tobytes() or up["status"][j] != "accepted"
        assert abs(rec[3, j] - float(up["log_u"][j])) <= 2 * U * abs(float(up["log_u"][j]))
        if up["status"][j] == "failed":
            assert st == "failed" and f_dev[:, j].tobytes() == f[:, j].tobytes() and idx[j] == k[j]
            continue
        err = abs(float(CB.LD(rec[2, j]) - up["dll"][j]))
        if up["e_dll"][j] > 0:
            worst = max(worst, err / up["e_dll"][j])
        assert err <= up["e_dll"][j], (t, j, err, up["e_dll"][j])
        assert up["e_dll"][j] < 1e-9                                                  # not vacuous: dll is of order one
        if not up["decided"][j]:
            undecided += 1
            k_new[j] = idx[j]
            continue
        assert st == up["status"][j], (t, j, st, up["status"][j])
        if st == "accepted":
            assert idx[j] == kp and f_dev[:, j].tobytes() == fp.tobytes()
            k_new[j] = kp
        else:
            assert idx[j] == k[j] and f_dev[:, j].tobytes() == f[:, j].tobytes()
    assert np.array_equal(s.amp_get("counts_centred"), counts)
    assert np.array_equal(s.amp_get("amplitude"), g[idx])
    return undecided, worst, seen, f_dev, k_new, H


# ---------------------------------------------------------------------------------------- 1. one update, constructed ---
@pytest.mark.parametrize("m", CB.MS)
@pytest.mark.parametrize("n", CB.NS)
def test_update_from_a_constructed_state_against_the_statement(handles, n, m):
    """n at the edges of the 64-row basis tile, the 256-thread row loop and its four-fold unroll, m of one and five items (one
    and two coefficient work-groups); theta on the grid with a repeated value and both end points, amplitudes spread over a
    33-point grid.  Two updates, each checked from the state before it."""
    from gpirt_amd import amp as A
    from gpirt_amd.ops import to_host
    seed = CB.SEED
    c = CB.case(n, m)
    s = _sampler(handles, c, seed)
    f, k = c["f"], c["k"].copy()
    a = c["grid"][k]
    counts = np.zeros((4, m), dtype=np.int64)
    undecided, worst, seen, f1, k1, H1 = _check_update(s, c, seed, 1, f, c["y"], k, counts)
    # the augmentation of that first call: normals and uniforms bit for bit, the coefficients within the derived bounds
    items = np.arange(m)
    z = s.amp_get("centred_z")
    assert z.tobytes() == A.centred_normals(seed, 1, items, handle=s.handle).tobytes()
    z_np = A.centred_normals(seed, 1, items)
    uu = to_host(s.handle.item_uniforms(seed, 1, 13, 0, m, 66))
    central = np.abs(uu[:64] - 0.5) <= 0.425
    assert np.array_equal(z[central], z_np[central]) and (np.abs(z - z_np) <= 4e-15 * np.maximum(1.0, np.abs(z))).all()
    u0, u1 = A.centred_uniforms(seed, 1, items)
    assert np.array_equal(uu[64], u0) and np.array_equal(uu[65], u1)
    F, live, r = s.amp_get("centred_F"), s.amp_get("live").astype(bool), s.amp_get("rank")
    F_np, live_np, r_np = A.centred_factor()
    assert r == r_np == 32 and np.array_equal(live, live_np) and not F[:, ~live].any()
    ref = A.centred_exact_coef(c["theta"], f, a, seed, 1, F=F, z=z)
    b = CB.coef_bounds(ref, f, a)
    nrm = lambda x: np.linalg.norm(np.asarray(x, dtype=np.float64), axis=0)            # noqa: E731
    used = {}
    used["T"] = float((np.abs(s.amp_get("centred_T") - ref["T"]).astype(np.float64) / b["T"]).max())
    used["w"] = float((nrm(s.amp_get("centred_w") - ref["w"]) / b["w"]).max())
    used["xi"] = float((nrm((s.amp_get("centred_xi") - ref["xi"])[live]) / b["xi"]).max())
    used["Q"] = float((np.abs(s.amp_get("centred_Q") - ref["Q"]).astype(np.float64) / b["Q"]).max())
    used["g"] = float((nrm(s.amp_get("centred_g") - ref["g"]) / b["g"]).max())
    used["H"] = float((np.abs(H1 - ref["H"]).astype(np.float64) / b["H"]).max())
    print(f"MEASURED n={n} m={m}: used fraction of the bounds {({q: f'{v:.1e}' for q, v in used.items()})}, dll {worst:.1e}; "
          f"statuses {seen}; rho {b['rho']:.1e}")
    assert max(used.values()) <= 1.0
    und2 = _check_update(s, c, seed, 2, f1, c["y"], k1, counts)[0]
    assert undecided <= 0.02 * m and und2 <= 0.02 * m
    st = s.amp_centred()
    assert st["calls"] == 2 and st["rank"] == 32 and st["updates"] == 2 * m == counts[0].sum()
    assert st["accepted"] == counts[1].sum() and st["same"] == counts[2].sum() and st["failed"] == counts[3].sum() == 0
    s.check()
    s.close()


# ------------------------------------------------------------------------------------------- 2. prior invariance ---
def test_prior_invariance_with_every_answer_missing(handles):
    """64 x 64, every y NaN, a 65-point grid on 0.25 .. 4 with log_prior = -(ln a)^2 / 0.5: 2000 rounds of {draw_f;
    draw_amp_centred}, every 5th index after round 200 kept; the counts of the 8 cells lie within 5 binomial sds of the prior's
    mass (tests/_amp_centred_bounds.py; its NumPy chain shows z up to 3.3, a wrong exponent 42, a missing noise term 1105)."""
    from gpirt_amd.sampler import Sampler
    theta, g, lp, edges, mass = CB.pi_setup()
    y = np.full((CB.PI_N, CB.PI_M), np.nan, order="F")
    kept_n = (CB.PI_ROUNDS - CB.PI_BURN) // CB.PI_THIN
    s = Sampler(handles(), y, theta, seed=21, **FAST)
    s.init()
    s.amp_enable(CB.PI_LO, CB.PI_HI, CB.PI_P, lp, 1, None, planned_draws=kept_n)
    it0 = s.iteration
    for rnd in range(CB.PI_ROUNDS):
        s.draw_f()
        s.draw_amp_centred()
        s.set_iteration(it0 + rnd + 1)                              # the next draw_f's normals and angles are fresh ones
        if rnd >= CB.PI_BURN and (rnd - CB.PI_BURN) % CB.PI_THIN == 0:
            s.amp_record()
    s.check()
    draws = s.amp_get("draws")
    assert draws.shape == (kept_n, CB.PI_M)
    z = CB.pi_zscores(draws, edges, mass)
    cn = s.amp_get("counts_centred")
    print(f"MEASURED prior invariance: z = {np.round(z, 2).tolist()}, largest |z| / 5 = {np.abs(z).max() / CB.PI_SDS:.2f}; accepted "
          f"{cn[1].sum()}, same {cn[2].sum()}, failed {cn[3].sum()} of {cn[0].sum()}")
    assert cn[3].sum() == 0 and cn[1].sum() + cn[2].sum() == cn[0].sum() == CB.PI_ROUNDS * CB.PI_M     # a prior-only item always accepts
    assert np.abs(z).max() <= CB.PI_SDS
    s.close()


# ------------------------------------------------------------------------------------ 3. the byte-identical cases ---
def test_rejected_same_and_failed_columns_are_byte_identical(handles):
    """300 x 4: item 0 with an inf in an unobserved row of f, item 1 with an inf in an observed row, item 2 with every answer
    missing (a prior-only item: never rejected), item 3 ordinary.  Eight updates: the two planted columns fail every time and
    stay byte-identical, every rejected or `same` column is byte-identical, item 2 is accepted or same, and the counters add up."""
    from gpirt_amd import _lib
    c = CB.case(300, 4)
    f, y = c["f"].copy(order="F"), c["y"].copy(order="F")
    f[int(np.flatnonzero(np.isnan(y[:, 0]))[0]), 0] = np.inf
    f[int(np.flatnonzero(~np.isnan(y[:, 1]))[0]), 1] = np.inf
    y[:, 2] = np.nan
    s = _sampler(handles, c, 9, f=f, y=y)
    prev = s.get("f")
    seen = {st: 0 for st in _lib.AMP_CENTRED_STATUS}
    for t in range(8):
        s.draw_amp_centred()
        rec, now = s.amp_get("record_centred"), s.get("f")
        for j in range(4):
            st = _lib.AMP_CENTRED_STATUS[int(rec[4, j])]
            seen[st] += 1
            if j < 2:
                assert st == "failed", (t, j, st)
            if j == 2:
                assert st in ("accepted", "same"), (t, st)
            if st != "accepted":
                assert now[:, j].tobytes() == prev[:, j].tobytes(), (t, j, st)
            else:
                assert now[:, j].tobytes() != prev[:, j].tobytes()
        prev = now
    cn = s.amp_get("counts_centred")
    assert cn[0].tolist() == [8] * 4 and cn[3].tolist()[:2] == [8, 8] and cn[3, 2] == cn[3, 3] == 0
    assert cn[1, 2] + cn[2, 2] == 8 and (cn[1] + cn[2] + cn[3] <= cn[0]).all()
    assert s.get("f")[:, 0].tobytes() == f[:, 0].tobytes() and s.get("f")[:, 1].tobytes() == f[:, 1].tobytes()
    print(f"MEASURED byte-identical cases: {seen}")
    s.check()                                                       # a failed update is not an error
    s.close()


# -------------------------------------------------------------------------------------------------- 4. determinism ---
def _state(s):
    return {k: s.get(k).tobytes() for k in ("theta", "beta", "f", "fstar")}


def test_two_runs_are_byte_identical(handles):
    """30 x {step(consistent=True); draw_amp(); draw_amp_centred()} at 256 x 8, twice: theta, beta, f, f*, the indices, both
    updates' counters and records byte for byte"""
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(256, 8, seed=6)
    out = []
    for _ in range(2):
        s = Sampler(handles(), y, th0, seed=12, **FAST)
        s.init()
        s.amp_enable(0.1, 10.0, 129, None, 4, None)
        for _ in range(30):
            s.step(consistent=True)
            s.draw_amp()
            s.draw_amp_centred()
        s.check()
        st = _state(s)
        for name in ("index", "amplitude", "counts", "record", "counts_centred", "record_centred", "centred_Q"):
            st[name] = s.amp_get(name).tobytes()
        out.append(st)
        cn = s.amp_get("counts_centred")
        s.close()
    assert out[0] == out[1]
    assert cn[0].tolist() == [30] * 8 and cn[1].sum() > 0
    print(f"MEASURED determinism: centred counts {cn.sum(axis=1).tolist()} (updates, accepted, same, failed)")


def test_a_sampler_that_never_calls_it_is_unchanged(handles):
    """257 x 5, five steps with draw_amp() after each: a twin that also ran one draw_amp_centred() on a DIFFERENT sampler of the
    same handle before, and a twin with nothing of the kind, are byte-identical in every stage's output -- the entry leaves no
    trace in a sampler that does not call it, and the whitened update's uniforms keep their numbers"""
    from gpirt_amd import amp as A
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(257, 5, seed=8)
    out = []
    for other in (False, True):
        h = handles()
        if other:
            o = Sampler(h, y, th0, seed=99, **FAST)
            o.init()
            o.amp_enable()
            o.draw_amp_centred()
            o.close()
        s = Sampler(h, y, th0, seed=13, **FAST)
        s.init()
        s.amp_enable(0.1, 10.0, 129, None, 4, None)
        ks = []
        for t in range(1, 6):
            s.step()
            f_before, k_before = s.get("f"), s.amp_get("index").astype(np.int64)
            s.draw_amp()
            ref = A.step_exact(f_before, s.get("mu"), y, k_before, 4, 13, t, s.amp_get("grid"), s.amp_get("log_prior"))
            assert np.array_equal(s.amp_get("index"), ref["k"])          # the whitened update is its statement's, as before
            ks.append(s.amp_get("index").tobytes())
        st = _state(s)
        st["ks"] = b"".join(ks)
        out.append(st)
        s.close()
    assert out[0] == out[1]


# ----------------------------------------------------------------------------------------------------- 5. refusals ---
def test_every_refusal_names_its_reason(handles):
    from gpirt_amd import _lib
    from gpirt_amd.distributed import ShardedSampler
    from gpirt_amd.ops import RStream
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(64, 4, seed=2)

    def refused(s, word):
        with pytest.raises(_lib.GpirtError, match=word) as e:
            s.draw_amp_centred()
        assert e.value.code == _lib.E_ARG

    s = Sampler(handles(), y, th0, seed=2, **FAST)
    refused(s, "needs an initialised sampler")
    s.init()
    refused(s, "not in the sampled mode.*they are off")
    s.amp_set(np.ones(4))
    refused(s, "not in the sampled mode.*they are fixed")
    s.amp_set(None)
    s.amp_enable(0.5, 2.0, 9)
    with pytest.raises(_lib.GpirtError, match="not enabled"):
        s.amp_get("counts_centred")                                  # its arrays exist from its first call on
    s.draw_amp_centred()
    assert s.amp_get("counts_centred")[0].tolist() == [1] * 4 and s.amp_centred()["calls"] == 1
    bad = th0.copy()
    bad[3] = 5.5
    s.set("theta", bad)
    refused(s, r"outside \[-5, 5\]")
    s.close()
    s = Sampler(handles(), y, th0, rng="reference", rstream=RStream(3))
    s.init()
    refused(s, "R's stream has no such draw")
    s.close()
    s = Sampler(handles(), y, th0, seed=2, kernel_fp32=True)
    s.init()
    refused(s, "kernel_fp32")
    s.close()
    s = Sampler(handles(), y, th0, seed=2, item0=4, m_total=8, **FAST)
    s.init()
    refused(s, "item shard")
    s.close()
    with pytest.raises(ValueError, match="not offered for item shards"):
        ShardedSampler.draw_amp_centred(object())
    for kern, word in ((dict(family="matern32", length_scale=1.0), "not a squared exponential"),
                       (dict(family="se", length_scale=0.1), "length_scale")):
        s = Sampler(handles(kern), y, th0, seed=2, rng="item", theta_stabilise=True)
        s.init()
        s.amp_enable(0.5, 2.0, 9)
        refused(s, word)
        s.draw_amp()                                                 # the whitened update runs under any kernel
        s.close()


# ------------------------------------------------------------------------------------------------------ 6. the run ---
def test_run_update_whitened_is_run_as_it_was_and_both_names_its_counters(handles):
    from gpirt_amd import amp as A
    from gpirt_amd.synthetic import make_responses
    y, _ = make_responses(96, 6, seed=2)
    kw = dict(chains=1, seed=3, points=33, width=3, top=2)
    a, b = A.run(y, 20, 20, **kw), A.run(y, 20, 20, update="whitened", **kw)
    assert a["amp"]["draws"].tobytes() == b["amp"]["draws"].tobytes() and a["f"].tobytes() == b["f"].tobytes()
    assert a["amp"]["update"] == "whitened" and "counts_centred" not in a["amp"]
    both = A.run(y, 20, 20, update="both", consistent=True, **kw)
    e = both["amp"]
    assert e["update"] == "both" and e["rank"] == 32 and e["counts_centred"].shape == (1, 4, 6)
    assert (e["counts_centred"][0, 0] == 40).all() and (e["counts"][0, 0] == 40).all() and e["accept_rate_centred"].shape == (1, 6)
    only = A.run(y, 10, 10, update="centred", consistent=True, **kw)
    assert (only["amp"]["counts"][0, 0] == 0).all() and (only["amp"]["counts_centred"][0, 0] == 20).all()
    with pytest.raises(ValueError, match="whitened"):
        A.run(y, 2, 2, update="neither")


# ------------------------------------------------------------------------------------------------------- 7. mixing ---
def test_both_updates_mix_no_worse_than_the_whitened_one():
    """384 x 6 synthetic, odd items with a 1.5-logit bump, consistent=True, one chain, 300 + 1200: the median over the items of
    Geyer's ESS of log a_j under "both" is at least that under "whitened".  The NumPy prototype at fixed theta showed a factor 3
    to 6; the factor 1 is the margin, because theta moves here.  Measured on one MI355X: median 17.2 against 8.0."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpirt_amd import amp as A
    y, th0 = CB.bumped_responses(384, 6)
    ess = {}
    for mode in ("whitened", "both"):
        res = A.run(y, 1200, 300, chains=1, seed=4, update=mode, consistent=True, store_draws=False, theta_init=th0[None, :])
        la = np.log(res["amp"]["amplitude"])
        ess[mode] = np.array([CB.geyer_ess(la[:, j]) for j in range(6)])
        extra = ""
        if mode == "both":
            cc = res["amp"]["counts_centred"][0]
            extra = f"; centred accepted {cc[1].sum()}, same {cc[2].sum()}, failed {cc[3].sum()} of {cc[0].sum()}"
        print(f"MEASURED mixing {mode}: ESS of log a_j {np.round(ess[mode], 1).tolist()}, median {np.median(ess[mode]):.1f}, mean "
              f"amplitude {res['amp']['mean'].round(2).tolist()}{extra}")
    assert np.median(ess["both"]) >= np.median(ess["whitened"])
