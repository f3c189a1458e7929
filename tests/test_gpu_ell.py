"""The length scale as a parameter of the chain on the device (include/gpirt_hip.h "the kernel's length scale as a parameter of
the chain", csrc/ell.hip, csrc/sampler.hip, gpirt_amd.ell): one update against the NumPy statement gpirt_amd.ell.step_exact
within the bounds tests/_ell_bounds.py derives, the sampler's state after accepted, rejected, out-of-range and failed updates,
a 2000-update trajectory decision for decision, and the one-call run.  Every handle is the test's own."""
import numpy as np
import pytest

import _ell_bounds as EB

pytestmark = pytest.mark.gpu

FAST = dict(rng="item", theta_stabilise=True, fstar_fused=True)


@pytest.fixture
def handles():
    """make(kernel) -> a fresh Handle under that kernel; all closed when the test ends"""
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


def _sampler(handles, c, seed, width, k=None, **kw):
    """a sampler in the constructed state of case c (theta, f, beta, mu as given; L the factor under ell_k), the update on"""
    from gpirt_amd.sampler import Sampler
    k = c["k"] if k is None else k
    h = handles(dict(family=c["family"], length_scale=float(c["grid"][k])))
    s = Sampler(h, c["y"], c["theta"], seed=seed, **dict(FAST, **kw))
    s.init()
    s.set("f", c["f"])
    s.set("beta", c["beta"])
    s.set("mu", c["mu"])
    s.ell_enable(c["lo"], c["hi"], c["points"], c["log_prior"], width)
    s.check()
    return h, s


def _buffer(s):
    """the whole factor buffer, the rows below L included ((n + ext) x n, column-major)"""
    s.get("theta")                                                   # (joins the sampler's own stream, drains the main one)
    return s.device_tensor("L").cpu().numpy().copy()


def _state(s):
    return {k: s.get(k).tobytes() for k in ("f", "L", "theta", "beta", "mu")} | {"buffer": _buffer(s).tobytes()}


def _one_update(handles, n, m, family, seed):
    c = EB.case(n, m, EB.P, 100 + n, family)
    h, s = _sampler(handles, c, seed, EB.W)
    L = s.get("L")                                                   # the device's factor under ell_k, before the update
    s.draw_ell()
    e = s.ell()
    out = dict(c=c, e=e, L=L, nu=s.ell_get("nu"), f_prop=s.ell_get("f_prop"), delta=s.ell_get("delta"), record=s.ell_get("record"),
               f=s.get("f"), uniforms=np.asarray(h.item_uniforms(seed, 1, 9, 0, 1, 2).cpu().numpy()).ravel())
    s.check()
    s.close()
    return out


# ------------------------------------------------------------------------------------- 1. one update, determinism ---
@pytest.mark.parametrize("family", ["se", "matern52"])
@pytest.mark.parametrize("n,m", [(200, 5), (65, 1)])
def test_one_update_against_step_exact(handles, n, m, family):
    """n = 200: an odd order, more than one 128 block, a ragged 64 tile; n = 65, m = 1: the 256-thread loop with fewer rows than
    threads.  nu, f', delta, dll and log_ratio within the bounds of tests/_ell_bounds.py; a reference one grid index off violates
    every one of them; a second run leaves byte-identical delta and record."""
    from gpirt_amd import ell as E
    seed = 21
    got = _one_update(handles, n, m, family, seed)
    c, e = got["c"], got["e"]
    u0, u1 = E.uniforms(seed, 1)
    assert np.array_equal(got["uniforms"], [u0, u1]) and (e["last_u0"], e["last_u1"]) == (u0, u1)
    ref = E.step_exact(c["theta"], c["f"], c["mu"], c["y"], c["k"], u0, u1, c["grid"], c["log_prior"], EB.W, family)
    ref["f_in"] = c["f"]
    assert ref["status"] in ("accepted", "rejected") and e["last_proposed"] == ref["k_prop"] and e["factorisations"] == 1
    b = EB.update_bounds(c, c["k"], ref["k_prop"], ref)
    off = E.step_exact(c["theta"], c["f"], c["mu"], c["y"], c["k"] + 1, u0, u1, c["grid"], c["log_prior"], EB.W, family)
    rec = got["record"]
    figures = [("nu", got["nu"], ref["nu"], off["nu"], b["nu"][None, :]), ("f_prop", got["f_prop"], ref["f_prop"], off["f_prop"], b["f_prop"][None, :]),
               ("delta", got["delta"], ref["delta"], off["delta"], b["delta"]), ("dll", rec[0], ref["dll"], off["dll"], b["dll"]),
               ("log_ratio", rec[1], ref["log_ratio"], off["log_ratio"], b["log_ratio"])]
    for name, dev, r, o, tol in figures:
        err = np.abs(np.asarray(dev).astype(EB.LD) - r).astype(np.float64)
        err_off = np.abs(np.asarray(dev).astype(EB.LD) - o).astype(np.float64)
        print(f"MEASURED {family} n={n} m={m} {name}: max err {np.max(err):.3e}, bound {np.max(tol):.3e}, "
              f"max err / bound {np.max(err / tol):.3e}; one index off: {np.max(err_off):.3e}")
        assert (err <= tol).all(), name
        assert np.max(err_off) > np.max(tol), name                      # the bound is not vacuous
    # stage by stage, given the device's own factors: each stage within its own rounding
    from gpirt_amd.sampler import Sampler
    fresh = Sampler(handles(dict(family=family, length_scale=float(c["grid"][ref["k_prop"]]))), c["y"], c["theta"], seed=seed, **FAST)
    fresh.init()
    fresh.check()
    stages = EB.stage_bounds(c, got["L"], fresh.get("L"), got, c["k"], ref["k_prop"])
    fresh.close()
    for name, (err, tol) in stages.items():
        print(f"MEASURED {family} n={n} m={m} {name} given the device's factors: max err {np.max(err):.3e}, bound {np.max(tol):.3e}, "
              f"max err / bound {np.max(err / np.maximum(tol, 1e-300)):.3e}")
        assert (np.asarray(err) <= np.asarray(tol)).all(), name
    assert rec[2] == float(np.log(u1)) and rec[4] == 0.0
    margin = abs(float(ref["log_ratio"] - ref["log_u"]))
    assert margin > 10 * b["log_ratio"]
    assert (rec[3] == 1.0) == (ref["status"] == "accepted") and e["last"] == ref["status"]
    want_f = got["f_prop"] if ref["status"] == "accepted" else c["f"]
    assert got["f"].tobytes() == np.asfortranarray(want_f).tobytes()
    again = _one_update(handles, n, m, family, seed)
    assert again["delta"].tobytes() == got["delta"].tobytes() and again["record"].tobytes() == got["record"].tobytes()


# ------------------------------------------------------------------------------------------ 2. state after an update ---
@pytest.mark.parametrize("n,m,family,lo,hi,rank,seed", [(128, 3, "se", 0.7, 2.8, 64, 4), (70, 2, "matern52", 0.25, 4.0, 0, 229)])
def test_state_after_accept_reject_and_out_of_range(handles, n, m, family, lo, hi, rank, seed):
    """P = 5, w = 4 and seeds for which (on the reference) the first update accepts, the second rejects and the third is out of
    range.  kstar_rank = 64 at n = 128: the bordered layout, the rows below L travel with it; kstar_rank = 0: L alone."""
    from gpirt_amd import ell as E
    from gpirt_amd.sampler import Sampler
    c = EB.case(n, m, 5, 7, family, lo, hi)
    h, s = _sampler(handles, c, seed, 4, kstar_rank=rank)
    assert s.ell()["length_scale"] == c["grid"][2] and s.ell()["last"] is None
    # accepted
    ref = E.step_exact(c["theta"], c["f"], c["mu"], c["y"], 2, *E.uniforms(seed, 1), c["grid"], c["log_prior"], 4, family)
    assert ref["status"] == "accepted"
    s.draw_ell()
    e = s.ell()
    kp = ref["k"]
    assert (e["last"], e["index"], e["updates"], e["accepted"]) == ("accepted", kp, 1, 1)
    assert e["length_scale"] == c["grid"][kp] and h.kernel() == dict(family=family, length_scale=float(c["grid"][2]))
    assert s.get("f").tobytes() == s.ell_get("f_prop").tobytes()
    fresh = Sampler(handles(dict(family=family, length_scale=float(c["grid"][kp]))), c["y"], c["theta"], seed=seed,
                    **dict(FAST, kstar_rank=rank))
    fresh.init()
    fresh.factor()
    fresh.check()
    got, want = _buffer(s), _buffer(fresh)
    assert got.shape == want.shape == ((n + rank) * n,)
    assert got.tobytes() == want.tobytes() and s.get("L").tobytes() == fresh.get("L").tobytes()
    s.draw_fstar()                                                  # the cached products are the new factor's: f* of the two agree
    fresh.set("f", s.get("f")); fresh.set("beta", c["beta"]); fresh.set("mu", c["mu"])
    fresh.set("mu_star", s.get("mu_star"))
    fresh.set_iteration(s.iteration)                              # (factor() closed an iteration: the same normals for both)
    fresh.draw_fstar()
    assert s.get("fstar").tobytes() == fresh.get("fstar").tobytes()
    fresh.close()
    # rejected, then out of range: nothing but the counters moves
    for t, status in ((2, "rejected"), (3, "out_of_range")):
        before, counts = _state(s), s.ell_get("counts")
        s.draw_ell()
        e = s.ell()
        assert e["last"] == status and e["index"] == kp and e["length_scale"] == c["grid"][kp]
        assert _state(s) == before
        moved = s.ell_get("counts") - counts
        assert list(moved) == [1, 0, int(status == "out_of_range"), 0]
    assert s.ell()["factorisations"] == 2                           # one per update that reached the device
    s.check()
    s.close()


# ------------------------------------------------------------------------------------------------- 3. trajectory ---
def test_trajectory_equals_the_numpy_chain(handles):
    """The CPU test's case (n = 40, m = 3, P = 17, w = 2), 2000 draw_ell calls with no step() in between: the index after every
    update and the four counters equal the NumPy chain's exactly (tests/test_ell_cpu.py shows that none of its decisions is a
    near-tie); the final f lies within the derived drift bound."""
    updates = 2000
    c = EB.case(EB.N, EB.M, EB.P, EB.SEED)
    ch = EB.chain(c, EB.W, updates)
    h, s = _sampler(handles, c, EB.SEED, EB.W)
    ks = np.empty(updates, dtype=np.int64)
    for t in range(updates):
        s.draw_ell()
        ks[t] = s.ell_get("index")[0]
    s.check()
    want = np.array([r["k"] for r in ch["records"]])
    first = int(np.argmax(ks != want)) if (ks != want).any() else -1
    assert first == -1, f"the chains part at update {first + 1}"
    e = s.ell()
    count = lambda st: sum(r["status"] == st for r in ch["records"])                    # noqa: E731
    assert [e[k] for k in ("updates", "accepted", "out_of_range", "failed")] == [updates, count("accepted"), count("out_of_range"), count("failed")]
    _, e_f = EB.trajectory_ratio_bound(c, ch["nu0"], updates)
    err = np.abs(s.get("f") - ch["f"]).max(axis=0)
    print(f"MEASURED trajectory: {e['accepted']} accepted of {updates}; final max |f - reference| {err.max():.3e} (bound {e_f.max():.3e})")
    assert (err <= e_f).all()
    s.close()


# ---------------------------------------------------------------------------------------------- 4. failed proposal ---
def test_a_non_finite_proposal_is_rejected_and_counted(handles):
    """one NaN in an observed cell of f: nu, f' and dll are not finite, the update is counted in `failed`, nothing else moves and
    check() is clean"""
    c = EB.case(70, 2, 5, 3)
    i = int(np.argwhere(~np.isnan(c["y"][:, 1]))[0][0])
    c["f"][i, 1] = np.nan
    h, s = _sampler(handles, c, 9, 1)
    before = _state(s)
    s.draw_ell()
    e = s.ell()
    assert (e["last"], e["failed"], e["accepted"], e["updates"], e["index"]) == ("failed", 1, 0, 1, 2)
    assert s.ell_get("record")[3] == 0.0 and s.ell_get("record")[4] >= 1.0
    assert _state(s) == before
    s.check()
    s.close()


def test_a_staged_guard_expiry_in_the_proposals_factor_is_repaired(handles):
    """gpirt_debug_trip_guard stages a hang-guard expiry (guard word raised, columns of NaN: no kernel spins) in the factorisation
    of the first update's proposal: nothing is committed, the factor is repeated on the launch-per-step panel and the decision
    taken again -- the index, the counters and (to the fallback panel's 1e-10) f and L of an undisturbed twin."""
    c = EB.case(128, 3, 5, 7, "se", 0.7, 2.8)
    outs = []
    for trip in (False, True):
        h, s = _sampler(handles, c, 4, 4, kstar_rank=64)
        before = h.guard_fallbacks
        if trip:
            h.debug_trip_guard(1)
        s.draw_ell()
        s.check()
        e = s.ell()
        assert h.guard_fallbacks == before + int(trip) and e["factorisations"] == 1 + int(trip)
        s.draw_ell()                                                # (and the next update finds a sampler in order)
        s.check()
        outs.append(dict(e=e, e2=s.ell(), f=s.get("f"), L=s.get("L"), record=s.ell_get("record")))
        s.close()
    a, b = outs
    for k in ("last", "index", "accepted", "failed", "length_scale"):
        assert a["e"][k] == b["e"][k] and a["e2"][k] == b["e2"][k], k
    assert a["e"]["last"] == "accepted"
    assert np.isfinite(b["f"]).all() and np.abs(a["f"] - b["f"]).max() <= 1e-10 * max(1.0, np.abs(a["f"]).max())
    assert np.abs(np.tril(a["L"]) - np.tril(b["L"])).max() <= 1e-12


def test_a_staged_guard_expiry_in_the_steps_factor_is_repaired_by_draw_ell(handles):
    """step() directly followed by draw_ell(), no check() between, as ell.run drives them: an expiry staged in the step's own
    factorisation is found by the update before it factors, repaired in place (one fallback) and is no error; the decision, the
    index and theta are the undisturbed twin's, f and the record within the fallback panel's 1e-10."""
    c = EB.case(128, 3, 5, 7, "se", 0.7, 2.8)
    outs = []
    for trip in (False, True):
        h, s = _sampler(handles, c, 4, 4, kstar_rank=64)
        before = h.guard_fallbacks
        if trip:
            h.debug_trip_guard(1)                                   # the factorisation that closes the step
        s.step()
        s.draw_ell()
        assert h.guard_fallbacks == before + int(trip)
        s.check()
        e = s.ell()
        assert e["updates"] == 1 == e["accepted"] + e["out_of_range"] + e["failed"] + int(e["last"] == "rejected")
        outs.append(dict(e=e, theta=s.get("theta"), f=s.get("f"), record=s.ell_get("record")))
        s.close()
    a, b = outs
    assert a["e"]["last"] in ("accepted", "rejected")               # (the update reached the device)
    for k in ("last", "index", "last_proposed", "length_scale", "factorisations"):
        assert a["e"][k] == b["e"][k], k
    assert np.array_equal(a["theta"], b["theta"])
    assert np.isfinite(b["f"]).all() and np.abs(a["f"] - b["f"]).max() <= 1e-10 * max(1.0, np.abs(a["f"]).max())
    assert np.abs(a["record"][:2] - b["record"][:2]).max() <= 1e-10 * max(1.0, np.abs(a["record"][:2]).max())


def test_counters_enabling_again_and_copy_state(handles):
    """enabling again zeroes the counters but not the call count t (no pair of uniforms is replayed); copy_state is refused while
    the update is on for either sampler"""
    from gpirt_amd import _lib, ell as E
    c = EB.case(70, 2, 5, 3)
    h, s = _sampler(handles, c, 9, 1)
    for _ in range(3):
        s.draw_ell()
    e = s.ell()
    assert e["updates"] == 3 and (e["last_u0"], e["last_u1"]) == E.uniforms(9, 3)
    s.ell_enable(c["lo"], c["hi"], c["points"], c["log_prior"], 1, k0=e["index"])
    assert s.ell()["updates"] == 0 and s.ell()["last"] is None
    s.draw_ell()
    e = s.ell()
    assert e["updates"] == 1 and (e["last_u0"], e["last_u1"]) == E.uniforms(9, 4)
    from gpirt_amd.sampler import Sampler
    other = Sampler(h, c["y"], c["theta"], seed=9, **FAST)
    other.init()
    for dst, src in ((other, s), (s, other)):
        with pytest.raises(_lib.GpirtError, match="length-scale update is on"):
            dst.copy_state_from(src)
    s.check()
    other.close()
    s.close()


# ------------------------------------------------------------------------------------------------ 5. off means off ---
def test_off_means_off(handles):
    """five step()s of a sampler that never heard of the update, of one with ell_enable(on=False) and of one on which it is on
    but never drawn: byte-identical theta, beta, f and f*"""
    from gpirt_amd import ell as E
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(128, 4, seed=3)
    lo, hi, points = 0.7, 2.8, 5                                     # (the fast preset's rank 64 passes its certificate at 0.7)
    ell1 = float(E.grid(lo, hi, points)[2])
    out = []
    for mode in ("never", "off", "on"):
        s = Sampler(handles(dict(family="se", length_scale=ell1)), y, th0, seed=5, preset="fast")
        s.init()
        if mode == "off":
            s.ell_enable(lo, hi, points, on=False)
        elif mode == "on":
            s.ell_enable(lo, hi, points, width=2)
        for _ in range(5):
            s.step()
        s.check()
        out.append({k: s.get(k).tobytes() for k in ("theta", "beta", "f", "fstar")})
        if mode != "on":
            from gpirt_amd import _lib
            with pytest.raises(_lib.GpirtError, match="not enabled"):
                s.draw_ell()
        s.close()
    assert out[0] == out[1] == out[2]


# -------------------------------------------------------------------------------------------------- 6. composition ---
def test_run(handles):
    """ell.run at n = 96, m = 6, two chains, S = 60, B = 40 with PSIS-LOO: indices on the grid, exact summaries, finite IRFs, a
    second run byte-identical; the refusals with their messages"""
    from gpirt_amd import _lib, ell as E
    from gpirt_amd.distributed import ShardedSampler
    from gpirt_amd.synthetic import make_responses
    y, _ = make_responses(96, 6, seed=2)
    S, B = 60, 40
    kw = dict(chains=2, seed=3, points=33, width=3, loo=True)
    a = E.run(y, S, B, **kw)
    e = a["ell"]
    g = E.grid(0.25, 4.0, 33)
    assert e["index"].shape == (2, S) and ((e["index"] >= 0) & (e["index"] < 33)).all()
    assert np.array_equal(e["length_scale"], g[e["index"]]) and np.array_equal(e["grid"], g)
    assert e["hist"].sum() == 2 * S and all(q in g for q in e["quantiles"].values()) and e["mode"] in g
    assert g[0] <= e["mean"] <= g[-1] and e["sd"] >= 0 and len(e["accept_rate"]) == len(e["width"]) == 2
    assert all(c["updates"] == S + B and c["failed"] == 0 for c in e["counts"])
    assert np.isfinite(a["IRFs"]).all() and a["IRFs"].shape == (1001, 6) and np.isfinite(a["loo"]["elpd_loo"])
    assert a["theta"].shape == (2, S + 1, 96) and a["kernel"] == dict(family="se", length_scale=1.0)
    print(f"MEASURED ell.run: mean {e['mean']:.3f} sd {e['sd']:.3f} mode {e['mode']:.3f} accept {e['accept_rate']} width {e['width']} "
          f"rhat {e['rhat']:.3f} ess {e['ess']:.1f}")
    b = E.run(y, S, B, **kw)
    for k in ("theta", "beta", "f", "IRFs"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["ell"]["index"].tobytes() == b["ell"]["index"].tobytes() and a["loo"]["elpd_loo"] == b["loo"]["elpd_loo"]
    with pytest.raises(_lib.GpirtError, match="R's stream has no such draw"):
        E.run(y, 4, 2, preset=None, rng="reference")
    with pytest.raises(_lib.GpirtError, match="kernel_fp32"):
        E.run(y, 4, 2, kernel_fp32=True)
    with pytest.raises(ValueError, match="not offered for item shards"):
        ShardedSampler.ell_enable(object())
    with pytest.raises(ValueError, match="not offered for item shards"):
        ShardedSampler.draw_ell(object())
