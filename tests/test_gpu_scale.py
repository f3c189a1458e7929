"""The collapsed scale and shift move on the device (include/gpirt_hip.h "a collapsed scale and shift move", csrc/scale.hip,
csrc/sampler.hip, gpirt_amd.scale): one call from constructed states against the long-double statement within the bounds
tests/_scale_bounds.py derives, the width 0, forced accepts and rejects, a failed call, prior invariance with every answer
missing, determinism, a sampler that never enables it against the parent's hashes, every refusal with its message, the one-call
run and mixing against the chain without the move.  Every handle is the test's own."""
import hashlib
import json
import os

import numpy as np
import pytest

import _scale_bounds as SB

pytestmark = pytest.mark.gpu

FAST = dict(rng="item", theta_stabilise=True, fstar_fused=True)
LD = np.longdouble
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "beta_centred_parent_257x5.json")
CHAIN = ("theta", "beta", "f", "fstar", "mu", "mu_star", "logpost")


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


def _sampler(handles, c, seed, pop=False, pm=None, ps=None, widths=None, fstar=None, **kw):
    """a sampler in the constructed state c, the move enabled, theta_partial done: the next call is draw_scale"""
    from gpirt_amd.sampler import Sampler
    s = Sampler(handles(), c["y"], c["theta"], c["pm"] if pm is None else pm, c["ps"] if ps is None else ps, seed=seed, **dict(FAST, **kw))
    s.init()
    s.set("fstar", c["fstar"] if fstar is None else fstar)
    s.set("beta", c["beta"])
    s.set("mu", c["mu"])
    s.set("mu_star", c["mu_star"])
    if pop:
        s.pop_set(c["codes"], SB.pop_table())
    w = SB.WIDTH if widths is None else widths
    s.scale_enable(w["scale"], w["shift"])
    s.theta_partial()
    return s


def _chain_state(s):
    return {k: s.get(k).tobytes() for k in CHAIN}


# ---------------------------------------------------------------------------------------- 1. one call, constructed ---
@pytest.mark.parametrize("pop", [False, True])
@pytest.mark.parametrize("m", SB.MS)
@pytest.mark.parametrize("n", SB.NS)
def test_a_call_from_a_constructed_state_against_the_statement(handles, n, m, pop):
    """n at the edges of the decide kernel's 256-row stride and the product's tiles, m of 1, 5 and 33, without and with a
    two-group population prior, both kinds from the same state (a rejected first call leaves it byte for byte; after an accepted
    one the second is checked from the committed state).  z bit for bit; c within 3 u of exp(-eps); given c: beta', mu2 and fstar2
    bit for bit; given the device's logpost and logpost_prop: lz, lz', dlz, D, Q and log r within their bounds; the decision the
    statement's, outside 100 x the bound.  Measured on one MI355X: at most 0.38 of a bound used (lz at 1025 x 33), 0.06 of log r's."""
    from gpirt_amd import scale as SC
    seed = SB.SEED
    c = SB.state(n, m, seed)
    s = _sampler(handles, c, seed, pop=pop)
    rows = SB.lprior_rows(c, pop)
    beta, fstar, mu_star = c["beta"], c["fstar"], c["mu_star"]
    assert s.get("mu_star").tobytes() == mu_star.tobytes()
    used = {}
    for kind in ("scale", "shift"):
        before = _chain_state(s)
        lp = s.scale_get("logpost")
        s.draw_scale(kind)
        rec = s.scale_get("record")
        z, u = SC.normals(seed, 1, kind, handle=s.handle)
        z_np, _ = SC.normals(seed, 1, kind)
        assert rec["kind"] == kind and rec["t"] == 1.0 and rec["width"] == SB.WIDTH[kind]
        assert np.float64(rec["z"]).tobytes() == np.float64(z).tobytes() and abs(z - z_np) <= 4e-15 * max(1.0, abs(z_np)) and rec["u"] == u
        step = SB.WIDTH[kind] * z
        assert rec["step"] == step
        if kind == "scale":
            assert abs(rec["c"] - float(np.exp(-LD(step)))) <= 3 * SB.U * rec["c"]
        else:
            assert rec["c"] == 1.0
        pr = SC.proposal(beta, kind, SB.WIDTH[kind], z, c=rec["c"])
        assert s.scale_get("beta_prop").tobytes() == pr["beta"].tobytes()
        assert s.scale_get("mu_prop").tobytes() == pr["mu"].tobytes()
        assert s.scale_get("fstar_prop").tobytes() == SC.curve(fstar, mu_star, pr["mu"]).tobytes()
        lp2 = s.scale_get("logpost_prop")
        assert lp.tobytes() == before["logpost"]
        ex = SC.step_exact(lp, lp2, beta, pr["beta"], c["pm"], c["ps"], kind, step, u, lprior=rows)
        bd = SB.decision_bounds(ex, lp, lp2, rows, beta, pr["beta"], c["pm"], c["ps"], kind)
        errs = dict(lz=(np.abs(s.scale_get("lz") - ex["lz"]).astype(np.float64), bd["lz"]),
                    lz_prop=(np.abs(s.scale_get("lz_prop") - ex["lz_prop"]).astype(np.float64), bd["lz_prop"]),
                    dlz=(np.abs(s.scale_get("dlz") - ex["dlz"]).astype(np.float64), bd["dlz"]),
                    D=(abs(float(rec["D"] - ex["D"])), bd["D"]), Q=(abs(float(rec["Q"] - ex["Q"])), bd["Q"]),
                    log_r=(abs(float(rec["log_r"] - ex["log_r"])), bd["log_r"]), log_u=(abs(float(rec["log_u"] - ex["log_u"])), bd["log_u"]))
        for k, (e, b) in errs.items():
            used[f"{kind}.{k}"] = float(np.max(e / b))
        print(f"MEASURED n={n} m={m} pop={pop} {kind}: share of each bound used {({q: f'{v:.2f}' for q, v in used.items() if q.startswith(kind)})}; "
              f"log r {rec['log_r']:+.4f}, log u {rec['log_u']:+.4f}, {rec['status']}")
        for k, (e, b) in errs.items():
            assert np.all(e <= b), (kind, k, e, b)
        assert rec["J"] == (float(m) * step if kind == "scale" else 0.0) and rec["bad"] == 0.0
        assert abs(float(ex["log_u"] - ex["log_r"])) >= SB.MARGIN * (bd["log_r"] + bd["log_u"])     # (the case, not the device: see test_scale_cpu)
        assert rec["status"] == ex["status"]
        after = _chain_state(s)
        if rec["status"] == "rejected":
            assert after == before
        else:
            th = c["theta"]
            assert after["beta"] == pr["beta"].tobytes() and after["mu_star"] == pr["mu"].tobytes() and after["logpost"] == lp2.tobytes()
            assert after["fstar"] == s.scale_get("fstar_prop").tobytes()
            assert after["mu"] == np.asfortranarray(pr["beta"][0][None, :] + th[:, None] * pr["beta"][1][None, :]).tobytes()
            assert after["theta"] == before["theta"] and after["f"] == before["f"]
            beta, fstar, mu_star = pr["beta"], s.get("fstar"), pr["mu"]
    st = s.scale()
    assert st["scale"]["calls"] == st["shift"]["calls"] == 1 and st["scale"]["failed"] == st["shift"]["failed"] == 0
    s.check()
    s.close()


# ------------------------------------------------------------------------------------------------ 2. the width 0 ---
@pytest.mark.parametrize("kind", ["scale", "shift"])
def test_width_zero_proposes_the_state_itself(handles, kind):
    """257 x 5, width 0: logpost_prop is byte-equal to logpost, dlz is exactly 0, the move is accepted, and every array of the
    chain is byte-identical"""
    c = SB.state(257, 5)
    s = _sampler(handles, c, 3, widths=dict(scale=0.0, shift=0.0))
    before = _chain_state(s)
    s.draw_scale(kind)
    rec = s.scale_get("record")
    assert s.scale_get("logpost_prop").tobytes() == before["logpost"]
    assert not s.scale_get("dlz").any() and rec["D"] == 0.0 and rec["Q"] == 0.0 and rec["log_r"] == 0.0
    assert rec["status"] == "accepted" and s.scale()[kind]["accepted"] == 1
    assert _chain_state(s) == before
    s.close()


# ------------------------------------------------------------------------------------- 3. forced accept and reject ---
@pytest.mark.parametrize("want", ["accepted", "rejected"])
@pytest.mark.parametrize("kind", ["scale", "shift"])
def test_a_forced_decision(handles, kind, want):
    """300 x 4 with a prior on the moved coefficient of sd 0.01 placed so that the proposal runs towards it (accepted) or away
    from it (rejected).  On reject everything is byte for byte as before.  On accept a second theta_partial() leaves logpost
    byte-identical to the committed one, mu_star and mu are draw_beta's bits for beta', the shape block's gbar moved with the
    mean, and theta_finish, carry_f, draw_beta and factor run and check() passes."""
    from gpirt_amd import scale as SC
    seed = 8
    c = SB.state(300, 4)
    z, _ = SC.normals(seed, 1, kind)
    # scale: eps > 0 shrinks the slopes (towards 0); shift: delta > 0 raises the intercepts (b1 > 0)
    towards_low = (z > 0) if kind == "scale" else (z < 0)
    low = towards_low == (want == "accepted")
    pm, ps = c["pm"].copy(order="F"), c["ps"].copy(order="F")
    q = 1 if kind == "scale" else 0
    pm[q], ps[q] = (-50.0 if low else 50.0), 0.01
    from gpirt_amd.sampler import Sampler
    s = Sampler(handles(), c["y"], c["theta"], pm, ps, seed=seed, **FAST)
    s.init()
    s.shape_enable()
    s.draw_fstar()                                                  # (gbar holds a curve from here on)
    s.set("fstar", c["fstar"]); s.set("beta", c["beta"]); s.set("mu", c["mu"]); s.set("mu_star", c["mu_star"])
    s.scale_enable(0.03, 0.05)
    s.theta_partial()
    before = _chain_state(s)
    gbar = s.get("gbar")
    s.draw_scale(kind)
    rec = s.scale_get("record")
    assert rec["status"] == want and abs(rec["Q"]) > 100
    st = s.scale()[kind]
    assert (st["calls"], st["accepted"], st["failed"]) == (1, int(want == "accepted"), 0)
    if want == "rejected":
        assert _chain_state(s) == before and s.get("gbar").tobytes() == gbar.tobytes()
        s.close()
        return
    b, th = s.get("beta"), s.get("theta")
    assert b.tobytes() == s.scale_get("beta_prop").tobytes() and b.tobytes() != before["beta"]
    assert s.get("mu").tobytes() == np.asfortranarray(b[0][None, :] + th[:, None] * b[1][None, :]).tobytes()
    assert s.get("mu_star").tobytes() == np.asfortranarray(b[0][None, :] + SC.GRID[:, None] * b[1][None, :]).tobytes()
    assert s.get("gbar").tobytes() == np.asfortranarray(gbar + (s.get("mu_star") - c["mu_star"])).tobytes()
    committed = s.get("logpost")
    assert committed.tobytes() == s.scale_get("logpost_prop").tobytes() and committed.tobytes() != before["logpost"]
    s.theta_partial()
    assert s.get("logpost").tobytes() == committed.tobytes()
    s.theta_finish(); s.carry_f(); s.draw_beta(); s.factor()
    s.check()
    s.step(consistent=True, scale=("scale", "shift"))
    s.check()
    assert np.isfinite(s.get("f")).all() and np.isfinite(s.get("fstar")).all()
    s.close()


def test_a_failed_call_stays_byte_for_byte(handles):
    """300 x 4, a NaN planted in item 1's fstar column at a grid point in front of observed cells: logpost holds NaN for every
    respondent who answered item 1, lz is not finite, the call is failed and counted, nothing of the chain moves"""
    c = SB.state(300, 4)
    assert (~np.isnan(c["y"][:, 1])).any()
    fstar = c["fstar"].copy(order="F")
    fstar[400, 1] = np.nan
    s = _sampler(handles, c, 5, fstar=fstar)
    before = _chain_state(s)
    for t, kind in enumerate(("scale", "shift", "scale")):
        s.draw_scale(kind)
        rec = s.scale_get("record")
        assert rec["status"] == "failed" and rec["bad"] > 0
        assert _chain_state(s) == before
    assert np.isnan(s.scale_get("lz")).any()
    st = s.scale()
    assert (st["scale"]["calls"], st["scale"]["failed"], st["scale"]["accepted"]) == (2, 2, 0)
    assert (st["shift"]["calls"], st["shift"]["failed"], st["shift"]["accepted"]) == (1, 1, 0)
    assert s.scale_get("counts").tolist() == [[2, 1], [0, 0], [2, 1]]
    s.close()


# ------------------------------------------------------------------------------------------- 4. prior invariance ---
def test_prior_invariance_on_the_device(handles):
    """64 x 64, every y NaN (logpost is 0 and dlz exactly 0: the prior and the Jacobian decide), priors off centre: 100 replicates
    of 40 alternating calls, each from a fresh prior draw of beta set from the host; the five z-scores of
    tests/_scale_bounds.py within 5 (measured on one MI355X: 1.89, 54 % accepted; the NumPy chain: 1.42; without -m eps 21.7, the
    shift reversed 170)."""
    from gpirt_amd.sampler import Sampler
    m, reps, calls = SB.PI_M, 100, SB.PI_CALLS
    pm, ps = SB.pi_priors()
    y = np.full((64, m), np.nan, order="F")
    theta = np.round(np.linspace(-2, 2, 64), 2)
    s = Sampler(handles(), y, theta, pm, ps, seed=21, **FAST)
    s.init()
    s.scale_enable(*SB.PI_W)
    rng = np.random.default_rng(2)
    finals = np.empty((reps, 2, m))
    for r in range(reps):
        s.set("beta", np.asfortranarray(pm + ps * rng.standard_normal((2, m))))
        s.theta_partial()
        for t in range(calls):
            s.draw_scale(t % 2)
        finals[r] = s.get("beta")
    assert not s.scale_get("dlz").any()
    z = SB.pi_zscores(finals, pm, ps)
    st = s.scale()
    rate = (st["scale"]["accepted"] + st["shift"]["accepted"]) / (reps * calls)
    print(f"MEASURED prior invariance on the device: z = {np.round(z, 2).tolist()}, largest |z| / 5 = {np.abs(z).max() / SB.PI_SDS:.2f}, accepted {rate:.2f}")
    assert st["scale"]["calls"] == st["shift"]["calls"] == reps * calls // 2 and st["scale"]["failed"] == st["shift"]["failed"] == 0
    assert 0.2 < rate < 0.9
    assert np.abs(z).max() <= SB.PI_SDS
    s.close()


# ------------------------------------------------------------------------------------- 5. determinism, the parent ---
def test_two_runs_are_byte_identical(handles):
    """30 x {step(consistent=True, scale=both); draw_beta_centred()} at 256 x 8, twice: the chain and the move's own arrays byte
    for byte"""
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(256, 8, seed=6)
    out = []
    for _ in range(2):
        s = Sampler(handles(), y, th0, seed=12, **FAST)
        s.init()
        s.scale_enable()
        for _ in range(30):
            s.step(consistent=True, scale=("scale", "shift"))
            s.draw_beta_centred()
        s.check()
        st = _chain_state(s)
        for name in ("lz", "lz_prop", "dlz", "beta_prop", "fstar_prop", "logpost_prop", "counts"):
            st[name] = s.scale_get(name).tobytes()
        st["record"] = repr(s.scale_get("record"))
        out.append(st)
        cn = s.scale_get("counts")
        s.close()
    assert out[0] == out[1]
    assert cn[0].tolist() == [30, 30] and cn[2].tolist() == [0, 0]


def _five_steps(handle, y, th0, opts):
    from gpirt_amd.sampler import Sampler
    s = Sampler(handle, y, th0, seed=13, **opts)
    s.init()
    for _ in range(5):
        s.step()
    s.check()
    st = {k: s.get(k).tobytes() for k in ("theta", "beta", "f", "fstar")}
    s.close()
    return st


@pytest.mark.parametrize("name,opts", [("fast", dict(preset="fast")), ("default", dict())])
def test_a_sampler_that_never_enables_it_is_unchanged(handles, name, opts):
    """257 x 5, five steps under the fast preset and under the default options: theta, beta, f and f* are byte for byte what the
    library gave two versions ago (tests/golden/beta_centred_parent_257x5.json), also on a handle on which ANOTHER sampler ran
    the move"""
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(257, 5, seed=8)
    plain = _five_steps(handles(), y, th0, opts)
    h = handles()
    o = Sampler(h, y, th0, seed=99, **FAST)
    o.init()
    o.scale_enable()
    o.step(consistent=True, scale=("scale", "shift"))
    o.close()
    assert _five_steps(h, y, th0, opts) == plain
    want = json.load(open(GOLDEN))[name]
    assert {k: hashlib.sha256(v).hexdigest() for k, v in plain.items()} == want


def test_the_step_entry_is_the_stage_calls(handles):
    """step(consistent=True, scale=...) against the stage calls one by one, and scale=() against step(consistent=True)"""
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(96, 6, seed=2)
    out = []
    for mode in range(2):
        s = Sampler(handles(), y, th0, seed=4, **FAST)
        s.init()
        s.scale_enable()
        for _ in range(6):
            if mode == 0:
                s.step(consistent=True, scale=("shift", "scale"))     # (the order is the library's: the scale first)
            else:
                s.draw_f(); s.draw_fstar(); s.theta_partial(); s.draw_scale("scale"); s.draw_scale("shift")
                s.theta_finish(); s.carry_f(); s.draw_beta(); s.factor()
        out.append(_chain_state(s))
        s.close()
    assert out[0] == out[1]
    out = []
    for mode in range(2):
        s = Sampler(handles(), y, th0, seed=4, **FAST)
        s.init()
        if mode == 0:
            s.scale_enable()
        for _ in range(4):
            s.step(consistent=True, scale=()) if mode == 0 else s.step(consistent=True)
        out.append(_chain_state(s))
        s.close()
    assert out[0] == out[1]


# ----------------------------------------------------------------------------------------------------- 6. refusals ---
def test_every_refusal_names_its_reason(handles):
    from gpirt_amd import _lib
    from gpirt_amd.distributed import ShardedSampler
    from gpirt_amd.ops import RStream
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(64, 4, seed=2)

    def refused(call, word):
        with pytest.raises(_lib.GpirtError, match=word) as e:
            call()
        assert e.value.code == _lib.E_ARG

    s = Sampler(handles(), y, th0, seed=2, **FAST)
    refused(lambda: s.scale_enable(), "needs an initialised sampler")
    refused(lambda: s.draw_scale("scale"), "needs an initialised sampler")
    s.init()
    refused(lambda: s.draw_scale("scale"), "not enabled")
    refused(lambda: s.scale_get("counts"), "not enabled")
    refused(lambda: s.step(consistent=True, scale="scale"), "not enabled")
    for w in (-0.1, np.inf):
        refused(lambda: s.scale_enable(w, 0.1), "width = .* must be finite and >= 0")
        refused(lambda: s.scale_enable(0.1, w), "shift width")
    s.scale_enable()
    st = s.scale()
    assert st["on"] and st["scale"]["width"] == st["shift"]["width"] == 1.0 / np.sqrt(64.0)
    refused(lambda: s.draw_scale("scale"), "logpost is not current")          # init's draw_fstar wrote fstar
    s.theta_partial()
    refused(lambda: s.draw_scale(2), "kind = 2")
    refused(lambda: s.scale_width("shift", np.nan), "must be finite and >= 0")
    refused(lambda: s.scale_get("record"), "one gpirt_sampler_draw_scale call")
    with pytest.raises(ValueError, match="scale"):
        s.draw_scale("tilt")
    with pytest.raises(ValueError, match="consistent=True"):
        s.step(scale="scale")
    s.draw_scale("scale")
    s.draw_scale("shift")                                                      # the entry keeps the note
    with pytest.raises(_lib.GpirtError, match="unknown scale array"):
        s._get_into("gpirt_sampler_scale_get", "nothing", np.empty(1))
    for writer in (lambda: s.set("beta", s.get("beta")), s.theta_finish, s.draw_beta, s.draw_fstar, s.draw_f, s.carry_f,
                   s.draw_beta_centred, lambda: s.pop_set((np.arange(64) % 2).astype(np.int32), SB.pop_table())):
        s.theta_partial()
        writer()
        refused(lambda: s.draw_scale("scale"), "logpost is not current")
    s.theta_partial()
    s.draw_scale("scale")                                                      # behind a plain step's stages: not refused
    s.close()
    s = Sampler(handles(), y, th0, rng="reference", rstream=RStream(3))
    s.init()
    refused(lambda: s.scale_enable(), "R's stream has no such draw")
    s.close()
    s = Sampler(handles(), y, th0, seed=2, item0=4, m_total=8, **FAST)
    s.init()
    refused(lambda: s.scale_enable(), "item shard")
    s.close()
    s = Sampler(handles(), y, th0, seed=2, **FAST)
    s.init()
    s.scale_enable()
    s.set_theta_block(y[:32], 0, 4)
    s.theta_partial()
    refused(lambda: s.draw_scale("scale"), "set_theta_block is in use")
    s.close()
    with pytest.raises(ValueError, match="not offered for item shards"):
        ShardedSampler.scale_enable(object())
    with pytest.raises(ValueError, match="not offered for item shards"):
        ShardedSampler.draw_scale(ShardedSampler.__new__(ShardedSampler), "scale")
    for sd in (np.inf, 0.0, -1.0, np.nan):
        ps = np.full((2, 4), 3.0)
        ps[1, 2] = sd
        s = Sampler(handles(), y, th0, None, ps, seed=2, **FAST)
        s.init()
        refused(lambda: s.scale_enable(), "prior sd of beta is not finite and > 0")
        s.close()


# ------------------------------------------------------------------------------------------------------ 7. the run ---
def test_run_none_is_beta_run_both_draw_for_draw():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpirt_amd import beta as Bt, scale as SC
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(96, 6, seed=2)
    a = SC.run(y, 10, 10, chains=2, seed=3, update="none")
    b = Bt.run(y, 10, 10, chains=2, seed=3, update="both")
    assert a["theta"].tobytes() == np.ascontiguousarray(b["theta"]).tobytes()
    assert np.array_equal(a["beta_draws"], np.moveaxis(b["beta_draws"][..., 1:], -1, 1))
    assert a["counts"] == [{}, {}] and a["update"] == "none"
    both = SC.run(y, 10, 60, chains=2, seed=3, update="both")
    for per in both["counts"]:
        for kd in ("scale", "shift"):
            assert per[kd]["calls"] == 70 and per[kd]["failed"] == 0 and 0.0 <= per[kd]["accept_rate"] <= 1.0
    assert both["series"]["S"].shape == (2, 10) and both["diag"]["beta"]["rhat"].shape == (2, 6)
    with pytest.raises(ValueError, match="both"):
        SC.run(y, 2, 2, update="tilt")


def test_mixing_of_the_scale_with_and_without_the_move():
    """384 x 6 on bumped_responses, consistent steps with draw_beta_centred, 200 + 600, two chains with the same seeds both ways.
    A FINDING, NOT AN ASSERTION: the expectation was ESS(S) with the move >= without, S = mean_j log|b1_j|, and the measurement
    contradicts it.  Measured on one MI355X: without the move S has split-R-hat 2.49 and Geyer's ESS 119 of 1200; with it
    split-R-hat 1.085 and ESS 35.  Without the move each chain fluctuates quickly about a scale of its own (a high within-chain
    ESS, summed over chains that disagree); with it the chains agree and each walks over the whole range, slowly.  sd(theta):
    R-hat 1.27 -> 1.003, ESS 343 -> 533; mean(theta): ESS 123 -> 236; the slopes one by one stay unconverged (R-hat 1.5 .. 5.5
    without, 2.1 .. 4.9 with).  Acceptance 0.32 (scale) and 0.26 (shift) at the adapted width 0.204.  The move is exact (the
    invariance and quadrature tests hold it to that), so it stays; what is asserted here is that the runs are sound."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import _amp_centred_bounds as CB
    from gpirt_amd import scale as SC
    y, th0 = CB.bumped_responses(384, 6)
    ess = {}
    for mode in ("none", "both"):
        res = SC.run(y, 600, 200, chains=2, seed=4, update=mode, consistent=True, theta_init=np.stack([th0, th0]))
        d = res["diag"]
        ess[mode] = float(d["S"]["ess"])
        print(f"MEASURED mixing {mode}: S rhat {float(d['S']['rhat']):.3f} ess {ess[mode]:.1f}; sd(theta) rhat {float(d['sd_theta']['rhat']):.3f} "
              f"ess {float(d['sd_theta']['ess']):.1f}; mean(theta) rhat {float(d['mean_theta']['rhat']):.3f} ess {float(d['mean_theta']['ess']):.1f}; "
              f"slopes rhat {np.round(d['beta']['rhat'][1], 3).tolist()} ess {np.round(d['beta']['ess'][1], 1).tolist()}; "
              f"intercepts rhat {np.round(d['beta']['rhat'][0], 3).tolist()} ess {np.round(d['beta']['ess'][0], 1).tolist()}; "
              f"counts {res['counts']}; {res['seconds']:.2f} s")
        assert np.isfinite(ess[mode]) and np.isfinite(res["theta"]).all() and np.isfinite(res["beta_draws"]).all()
        for per in res["counts"]:
            assert all(e["failed"] == 0 and e["calls"] == 800 for e in per.values()) and len(per) == (2 if mode == "both" else 0)
    print(f"FINDING ESS(S) with the move {ess['both']:.1f}, without {ess['none']:.1f}: the expectation with >= without is "
          f"{'met' if ess['both'] >= ess['none'] else 'NOT met'} (see the docstring)")
