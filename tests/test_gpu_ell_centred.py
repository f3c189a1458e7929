"""The centred length-scale update on the device (include/gpirt_hip.h "Library version 126", csrc/ell.hip, csrc/sampler.hip,
gpirt_amd.ell): one update against the NumPy statement gpirt_amd.ell.step_exact_centred within the bounds
tests/_ell_centred_bounds.py derives, the sampler's state after each outcome, a 2000-update centred and a 500 + 500 mixed
trajectory decision for decision, the whitened update untouched beside it, a failed proposal, a staged guard expiry, and the
one-call run's modes.  Every handle is the test's own."""
import numpy as np
import pytest

import _ell_bounds as EB
import _ell_centred_bounds as CB

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


def _sampler(handles, c, seed, width, k=None, log_prior=None, **kw):
    """a sampler in the constructed state of case c (theta, f, beta, mu as given; L the factor under ell_k), the update on"""
    from gpirt_amd.sampler import Sampler
    k = c["k"] if k is None else k
    h = handles(dict(family=c["family"], length_scale=float(c["grid"][k])))
    s = Sampler(h, c["y"], c["theta"], seed=seed, **dict(FAST, **kw))
    s.init()
    s.set("f", c["f"])
    s.set("beta", c["beta"])
    s.set("mu", c["mu"])
    s.ell_enable(c["lo"], c["hi"], c["points"], c["log_prior"] if log_prior is None else log_prior, width)
    s.check()
    return h, s


def _buffer(s):
    """the whole factor buffer, the rows below L included ((n + ext) x n, column-major)"""
    s.get("theta")                                                   # (joins the sampler's own stream, drains the main one)
    return s.device_tensor("L").cpu().numpy().copy()


def _state(s):
    return {k: s.get(k).tobytes() for k in ("f", "L", "theta", "beta", "mu")} | {"buffer": _buffer(s).tobytes()}


def _rejected(tally, e):
    """updates = accepted + rejected + out_of_range + failed, `rejected` being the tally of the updates whose `last` said so"""
    return e["updates"] == e["accepted"] + tally + e["out_of_range"] + e["failed"]


def _towards(d, points):
    """a prior table under which a move by offset d is accepted and one against it rejected, whatever the data say"""
    return (1e6 if d > 0 else -1e6) * np.arange(points)


# ------------------------------------------------------------------------------------------ 1. one update, both layers ---
@pytest.mark.parametrize("n,m,family", [(200, 5, "se"), (65, 1, "matern52"), (1100, 2, "se"), (65, 1030, "se")])
def test_one_update_against_step_exact_centred(handles, n, m, family):
    """n = 200: an odd order, a ragged 64 tile; n = 65, m = 1: fewer rows than threads; n = 1100: the four-way unrolled row loop and
    its tail in ell_quad_kernel and ell_logdet_kernel; m = 1030: the second 1024-item chunk of the decision's sum.  nu, nu', dq_j,
    dq, dld and log_ratio within the end-to-end bounds; a reference one grid index off misses them by more than 100x; then stage
    by stage from the device's own factors; the uniforms are item index 1's; a second run is byte-identical."""
    from gpirt_amd import ell as E
    from gpirt_amd.sampler import Sampler
    seed = 21
    c = CB.case(n, m, EB.P, 100 + n, family)
    k = c["k"]

    def run():
        h, s = _sampler(handles, c, seed, EB.W)
        before = _state(s)
        L = s.get("L")
        s.draw_ell("centred")
        out = dict(e=s.ell(), L=L, before=before, after=_state(s), **{q: s.ell_get(q) for q in ("nu", "nu_prop", "dq", "record_centred")},
                   uniforms=np.asarray(h.item_uniforms(seed, 1, 9, 1, 1, 2).cpu().numpy()).ravel())
        s.check()
        s.close()
        return out

    got = run()
    e, ec, rec = got["e"], got["e"]["centred"], got["record_centred"]
    u0, u1 = E.uniforms(seed, 1, "centred")
    assert np.array_equal(got["uniforms"], [u0, u1]) and (ec["last_u0"], ec["last_u1"]) == (u0, u1)
    assert e["updates"] == 0 and e["last"] is None and ec["updates"] == 1 and ec["factorisations"] == 1   # the whitened counters are its alone
    cache = {}
    ref = E.step_exact_centred(c["theta"], c["f"], k, u0, u1, c["grid"], c["log_prior"], EB.W, family, cache)
    off = E.step_exact_centred(c["theta"], c["f"], k + 1, u0, u1, c["grid"], c["log_prior"], EB.W, family, cache)
    kp = ref["k_prop"]
    assert ref["status"] in ("accepted", "rejected") and ec["last_proposed"] == kp
    r = CB._record(ref, k, "centred")
    b = CB.update_bounds(c, k, kp, r["nn"], r["nnp"], r["abs_cells"], ref["dq"], ref["dld"],
                         diag=(np.diagonal(cache[k]), np.diagonal(cache[kp])))
    col = lambda x, y_: np.sqrt(((np.asarray(x).astype(EB.LD) - y_).astype(np.float64) ** 2).sum(axis=0))      # noqa: E731
    ab = lambda x, y_: np.abs(np.asarray(x).astype(EB.LD) - y_).astype(np.float64)                             # noqa: E731
    figures = [("nu", col(got["nu"], ref["nu"]), col(got["nu"], off["nu"]), b["nu"]),
               ("nu_prop", col(got["nu_prop"], ref["nu_prop"]), col(got["nu_prop"], off["nu_prop"]), b["nu_prop"]),
               ("dq_j", ab(got["dq"], ref["dq"]), ab(got["dq"], off["dq"]), b["dq"]),
               ("dq", ab(rec[0], ref["dq"].sum()), ab(rec[0], off["dq"].sum()), b["dq_sum"]),
               ("dld", ab(rec[1], ref["dld"]), ab(rec[1], off["dld"]), b["dld"]),
               ("log_ratio", ab(rec[2], ref["log_ratio"]), ab(rec[2], off["log_ratio"]), b["log_ratio"])]
    for name, err, err_off, tol in figures:
        print(f"MEASURED {family} n={n} m={m} {name}: max err {np.max(err):.3e}, bound {np.max(tol):.3e}, max err / bound "
              f"{np.max(err / tol):.3e}; one index off: {np.max(err_off):.3e}")
        assert (err <= tol).all(), name
        assert np.max(err_off) > 100 * np.max(tol), name                 # one grid index off misses by orders of magnitude
    fresh = Sampler(handles(dict(family=family, length_scale=float(c["grid"][kp]))), c["y"], c["theta"], seed=seed, **FAST)
    fresh.init()
    fresh.check()
    stages = CB.stage_bounds(c, got["L"], fresh.get("L"), got, k, kp)
    fresh.close()
    for name, (err, tol) in stages.items():
        print(f"MEASURED {family} n={n} m={m} {name} given the device's factors: max err {np.max(err):.3e}, bound {np.max(tol):.3e}, "
              f"max err / bound {np.max(err / np.maximum(tol, 1e-300)):.3e}")
        assert (np.asarray(err) <= np.asarray(tol)).all(), name
    assert rec[3] == float(np.log(u1)) and rec[5] == 0.0
    margin = abs(float(ref["log_ratio"] - ref["log_u"]))
    assert margin > 10 * b["log_ratio"]
    assert (rec[4] == 1.0) == (ref["status"] == "accepted") and ec["last"] == ref["status"]
    assert e["index"] == ref["k"] and e["length_scale"] == c["grid"][ref["k"]]
    assert got["after"]["f"] == got["before"]["f"]                       # f does not move, whatever the outcome
    if ref["status"] == "rejected":
        assert got["after"] == got["before"]
    again = run()
    for q in ("nu", "nu_prop", "dq", "record_centred"):
        assert again[q].tobytes() == got[q].tobytes(), q


# ------------------------------------------------------------------------------------------ 2. state after an update ---
@pytest.mark.parametrize("n,m,family,lo,hi,rank,seed", [(128, 3, "se", 0.7, 2.8, 64, 4), (70, 2, "matern52", 0.25, 4.0, 0, 229)])
def test_state_after_accept_reject_and_out_of_range(handles, n, m, family, lo, hi, rank, seed):
    """P = 5, w = 1.  Each outcome is driven by a prior table that rises by 1e6 per index towards (accept) or against (reject) the
    offset the call's own uniform proposes, or by starting at the grid's end that offset leaves (out of range).  kstar_rank = 64
    at n = 128: the bordered layout, the rows below L travel with it; kstar_rank = 0: L alone."""
    from gpirt_amd import ell as E
    from gpirt_amd.sampler import Sampler
    c = CB.case(n, m, 5, 7, family, lo, hi)
    d = [E.proposal(E.uniforms(seed, t, "centred")[0], 1) for t in (1, 2, 3)]
    h, s = _sampler(handles, c, seed, 1, log_prior=_towards(d[0], 5), kstar_rank=rank)
    f0 = s.get("f").tobytes()
    # accepted
    s.draw_ell("centred")
    e, kp = s.ell(), 2 + d[0]
    assert (e["centred"]["last"], e["index"], e["centred"]["updates"], e["centred"]["accepted"], e["updates"]) == ("accepted", kp, 1, 1, 0)
    assert e["length_scale"] == c["grid"][kp] and h.kernel() == dict(family=family, length_scale=float(c["grid"][2]))
    assert s.get("f").tobytes() == f0 == np.asfortranarray(c["f"]).tobytes()
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
    fresh.set_iteration(s.iteration)
    fresh.draw_fstar()
    assert s.get("fstar").tobytes() == fresh.get("fstar").tobytes()
    fresh.close()
    # rejected: the table turned against the next offset; t_c runs on through ell_enable
    s.ell_enable(lo, hi, 5, _towards(-d[1], 5), 1, k0=kp)
    s.check()
    before = _state(s)
    s.draw_ell("centred")
    e = s.ell()
    assert (e["centred"]["last_u0"], e["centred"]["last_u1"]) == E.uniforms(seed, 2, "centred")
    assert e["centred"]["last"] == "rejected" and e["centred"]["last_proposed"] == kp + d[1] and e["index"] == kp
    assert list(s.ell_get("counts_centred")) == [1, 0, 0, 0] and _state(s) == before
    # out of range: from the end of the grid the third offset leaves
    end = 0 if d[2] < 0 else 4
    s.ell_enable(lo, hi, 5, None, 1, k0=end)
    s.check()
    before = _state(s)
    s.draw_ell("centred")
    e = s.ell()
    assert e["centred"]["last"] == "out_of_range" and e["centred"]["last_proposed"] == end + d[2] and e["index"] == end
    assert list(s.ell_get("counts_centred")) == [1, 0, 1, 0] and e["centred"]["factorisations"] == 0 and _state(s) == before
    assert list(s.ell_get("counts")) == [0, 0, 0, 0]
    s.check()
    s.close()


# ------------------------------------------------------------------------------------------------- 3. trajectories ---
def test_centred_trajectory_equals_the_numpy_chain(handles):
    """The CPU test's case (n = 40, m = 3, 65 points, w = 4), 2000 centred updates with no step() in between: the index after every
    update and the counters equal the NumPy chain's exactly (tests/test_ell_centred_cpu.py shows that none of its decisions is a
    near-tie); f is byte-identical throughout; the counters' identity holds after every update."""
    updates = CB.GPU_UPDATES
    c = CB.chain_case()
    ch = CB.chain(c, CB.W, updates)
    h, s = _sampler(handles, c, CB.SEED, CB.W)
    ks = np.empty(updates, dtype=np.int64)
    rejected = 0
    for t in range(updates):
        s.draw_ell("centred")
        e = s.ell()
        ks[t] = e["index"]
        rejected += e["centred"]["last"] == "rejected"
        assert _rejected(rejected, e["centred"]), t
    s.check()
    want = np.array([r["k"] for r in ch["records"]])
    first = int(np.argmax(ks != want)) if (ks != want).any() else -1
    assert first == -1, f"the chains part at update {first + 1}"
    e = s.ell()
    count = lambda st: sum(r["status"] == st for r in ch["records"])                    # noqa: E731
    assert list(s.ell_get("counts_centred")) == [updates, count("accepted"), count("out_of_range"), count("failed")]
    assert rejected == count("rejected") and e["centred"]["factorisations"] == updates - count("out_of_range")
    assert e["updates"] == 0 and s.get("f").tobytes() == np.asfortranarray(c["f"]).tobytes()
    print(f"MEASURED centred trajectory: {e['centred']['accepted']} accepted of {updates}")
    s.close()


def test_mixed_trajectory_equals_the_numpy_chain(handles):
    """Whitened and centred alternating, 500 of each, no step() in between: every decision, both counter sets and the final index
    equal NumPy's; the final f within the trajectory bound of tests/_ell_bounds.py; the counters' identity holds for both kinds
    after every update."""
    pairs = CB.MIXED
    c = CB.chain_case()
    mx = CB.mixed_chain(c, CB.W, pairs)
    h, s = _sampler(handles, c, CB.SEED, CB.W)
    got, rejected = [], {"whitened": 0, "centred": 0}
    for t in range(pairs):
        for kind in ("whitened", "centred"):
            s.draw_ell(kind)
            e = s.ell()
            ek = e if kind == "whitened" else e["centred"]
            got.append((ek["last"], e["index"]))
            rejected[kind] += ek["last"] == "rejected"
            assert _rejected(rejected["whitened"], e) and _rejected(rejected["centred"], e["centred"]), (t, kind)
    s.check()
    want = [(r["status"], r["k"]) for r in mx["records"]]
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), -1)
    assert first == -1, f"the chains part at update {first + 1} ({got[first]} against {want[first]})"
    e = s.ell()
    for kind, name in (("whitened", "counts"), ("centred", "counts_centred")):
        count = lambda st: sum(r["status"] == st and r["kind"] == kind for r in mx["records"])     # noqa: E731
        assert list(s.ell_get(name)) == [pairs, count("accepted"), count("out_of_range"), count("failed")], kind
    assert e["index"] == mx["k"]
    _, e_f, _ = CB.mixed_bounds(c, mx["records"])
    err = np.abs(s.get("f") - mx["f"]).max(axis=0)
    print(f"MEASURED mixed trajectory: {e['accepted']} whitened and {e['centred']['accepted']} centred accepted of {pairs} each; final "
          f"max |f - reference| {err.max():.3e} (bound {e_f.max():.3e})")
    assert (err <= e_f).all()
    s.close()


# ------------------------------------------------------------------------------------- 5. the whitened update untouched ---
def test_the_whitened_update_is_untouched_by_centred_calls(handles):
    """Centred calls in between do not shift the whitened stream: its uniforms are those of t = the count of whitened calls alone,
    and one whitened update from the state the centred calls left (f as it was, the index wherever they took it) holds the
    existing comparison against step_exact within tests/_ell_bounds.py's bounds."""
    from gpirt_amd import ell as E
    n, m, seed = 200, 5, 21
    c = EB.case(n, m, EB.P, 100 + n, "se")
    h, s = _sampler(handles, c, seed, EB.W)
    for _ in range(3):
        s.draw_ell("centred")
    k = s.ell()["index"]
    assert s.get("f").tobytes() == np.asfortranarray(c["f"]).tobytes() and s.ell()["updates"] == 0
    s.draw_ell()
    e = s.ell()
    u0, u1 = E.uniforms(seed, 1)
    assert (e["last_u0"], e["last_u1"]) == (u0, u1) and e["updates"] == 1 and e["centred"]["updates"] == 3
    assert (e["centred"]["last_u0"], e["centred"]["last_u1"]) == E.uniforms(seed, 3, "centred")
    ref = E.step_exact(c["theta"], c["f"], c["mu"], c["y"], k, u0, u1, c["grid"], c["log_prior"], EB.W, "se")
    ref["f_in"] = c["f"]
    assert ref["status"] in ("accepted", "rejected") and e["last_proposed"] == ref["k_prop"]
    b = EB.update_bounds(c, k, ref["k_prop"], ref)
    rec = s.ell_get("record")
    for name, dev, r, tol in (("nu", s.ell_get("nu"), ref["nu"], b["nu"][None, :]), ("f_prop", s.ell_get("f_prop"), ref["f_prop"], b["f_prop"][None, :]),
                              ("delta", s.ell_get("delta"), ref["delta"], b["delta"]), ("dll", rec[0], ref["dll"], b["dll"]),
                              ("log_ratio", rec[1], ref["log_ratio"], b["log_ratio"])):
        err = np.abs(np.asarray(dev).astype(EB.LD) - r).astype(np.float64)
        print(f"MEASURED whitened after centred {name}: max err {np.max(err):.3e}, bound {np.max(tol):.3e}")
        assert (err <= tol).all(), name
    if abs(float(ref["log_ratio"] - ref["log_u"])) > 10 * b["log_ratio"]:
        assert e["last"] == ref["status"]
    s.draw_ell("centred")
    s.draw_ell()
    e = s.ell()
    assert (e["last_u0"], e["last_u1"]) == E.uniforms(seed, 2) and (e["centred"]["last_u0"], e["centred"]["last_u1"]) == E.uniforms(seed, 4, "centred")
    s.check()
    s.close()


def test_widths_are_per_kind(handles):
    from gpirt_amd import _lib
    c = CB.case(70, 2, 5, 3)
    h, s = _sampler(handles, c, 9, 2)
    assert s.ell()["width"] == 2 == s.ell()["centred"]["width"]
    s.ell_width(3, "centred")
    assert (s.ell()["width"], s.ell()["centred"]["width"]) == (2, 3)
    s.ell_width(1)
    assert (s.ell()["width"], s.ell()["centred"]["width"]) == (1, 3)
    with pytest.raises(_lib.GpirtError, match="width"):
        s.ell_width(5, "centred")
    with pytest.raises(ValueError):
        s.draw_ell("other")
    s.ell_enable(on=False)
    with pytest.raises(_lib.GpirtError, match="not enabled"):
        s.draw_ell("centred")
    s.close()


# ---------------------------------------------------------------------------------------------- 6. failed proposal ---
def test_a_nan_in_f_is_counted_as_failed(handles):
    """one NaN in f: nu, nu' and dq are not finite, the update is counted in the centred `failed`, nothing else moves and check()
    is clean"""
    c = CB.case(70, 2, 5, 3)
    c["f"][11, 1] = np.nan
    h, s = _sampler(handles, c, 9, 1)
    before = _state(s)
    s.draw_ell("centred")
    e = s.ell()
    ec = e["centred"]
    assert (ec["last"], ec["failed"], ec["accepted"], ec["updates"], e["index"], e["updates"]) == ("failed", 1, 0, 1, 2, 0)
    rec = s.ell_get("record_centred")
    assert rec[4] == 0.0 and rec[5] >= 1.0
    assert _state(s) == before
    s.check()
    s.close()


# --------------------------------------------------------------------------------------------------- 7. the guard ---
def test_a_staged_guard_expiry_in_the_proposals_factor_is_repaired(handles):
    """gpirt_debug_trip_guard stages a hang-guard expiry (guard word raised, columns of NaN: no kernel spins) in the factorisation
    of the first centred update's proposal: one fallback, two factorisations counted, the undisturbed twin's decision, f untouched
    and L within the fallback panel's rounding of the twin's."""
    from gpirt_amd import ell as E
    c = CB.case(128, 3, 5, 7, "se", 0.7, 2.8)
    d = E.proposal(E.uniforms(4, 1, "centred")[0], 1)
    outs = []
    for trip in (False, True):
        h, s = _sampler(handles, c, 4, 1, log_prior=_towards(d, 5), kstar_rank=64)
        before = h.guard_fallbacks
        if trip:
            h.debug_trip_guard(1)
        s.draw_ell("centred")
        s.check()
        e = s.ell()
        assert h.guard_fallbacks == before + int(trip) and e["centred"]["factorisations"] == 1 + int(trip)
        s.draw_ell("centred")                                       # (and the next update finds a sampler in order)
        s.check()
        outs.append(dict(e=e, e2=s.ell(), f=s.get("f"), L=s.get("L"), record=s.ell_get("record_centred")))
        s.close()
    a, b = outs
    for k in ("last", "accepted", "failed", "last_proposed"):
        assert a["e"]["centred"][k] == b["e"]["centred"][k] and a["e2"]["centred"][k] == b["e2"]["centred"][k], k
    assert a["e"]["index"] == b["e"]["index"] == 2 + d and a["e2"]["index"] == b["e2"]["index"]
    assert a["e"]["centred"]["last"] == "accepted"
    assert a["f"].tobytes() == b["f"].tobytes() == np.asfortranarray(c["f"]).tobytes()
    assert np.abs(np.tril(a["L"]) - np.tril(b["L"])).max() <= 1e-12


# ------------------------------------------------------------------------------------------------ 9. composition ---
def test_run_centred_and_both(handles):
    """ell.run at n = 96, m = 6, two chains with update="centred" and "both": counts consistent, no update failed"""
    from gpirt_amd import ell as E
    from gpirt_amd.synthetic import make_responses
    y, _ = make_responses(96, 6, seed=2)
    S, B = 30, 60
    for update, kinds in (("centred", ("centred",)), ("both", ("whitened", "centred"))):
        a = E.run(y, S, B, chains=2, seed=3, points=33, width=3, update=update, width_centred=2)
        e = a["ell"]
        assert e["update"] == update and set(e["counts"]) == set(e["accept_rate"]) == set(e["width"]) == set(kinds)
        assert e["index"].shape == (2, S) and ((e["index"] >= 0) & (e["index"] < 33)).all() and e["hist"].sum() == 2 * S
        for kind in kinds:
            assert len(e["counts"][kind]) == len(e["accept_rate"][kind]) == len(e["width"][kind]) == 2
            for cnt, rate in zip(e["counts"][kind], e["accept_rate"][kind]):
                assert cnt["updates"] == S + B and cnt["failed"] == 0
                assert 0 <= cnt["accepted"] <= cnt["updates"] - cnt["out_of_range"] and 0.0 <= rate <= 1.0
            assert all(1 <= w <= 32 for w in e["width"][kind])
        assert np.isfinite(a["IRFs"]).all() and np.isfinite(a["theta"]).all()
        print(f"MEASURED ell.run update={update}: mean {e['mean']:.3f} sd {e['sd']:.3f} accept {e['accept_rate']} width {e['width']} "
              f"rhat {e['rhat']:.3f} ess {e['ess']:.1f}")


def test_run_whitened_is_the_call_without_the_keyword(handles):
    from gpirt_amd import ell as E
    from gpirt_amd.synthetic import make_responses
    y, _ = make_responses(96, 6, seed=2)
    kw = dict(chains=2, seed=3, points=33, width=3)
    a, b = E.run(y, 30, 60, **kw), E.run(y, 30, 60, update="whitened", **kw)
    for k in ("theta", "beta", "f", "IRFs"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["ell"]["index"].tobytes() == b["ell"]["index"].tobytes() and a["ell"]["update"] == b["ell"]["update"] == "whitened"
    assert a["ell"]["accept_rate"] == b["ell"]["accept_rate"] and a["ell"]["width"] == b["ell"]["width"] and a["ell"]["counts"] == b["ell"]["counts"]
    assert isinstance(a["ell"]["accept_rate"], list) and len(a["ell"]["counts"]) == 2
