"""The consistent step on the device (include/gpirt_hip.h "a consistent step", csrc/carry.hip, csrc/sampler.hip,
gpirt_amd.consistent): the carry stage bit for bit against carry_exact with the device's normals, its counters, shard invariance,
step(consistent=True) against the seven stage calls, the effect on the prior quadratic form, prior_quad against
prior_quad_exact, the refusals.  Every handle is the test's own."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ITEM = dict(rng="item", theta_stabilise=True)
FAST = dict(rng="item", fstar_fused=True, kstar_rank=64, theta_stabilise=True)
SWITCHES = ("GPIRT_FACTOR_LR", "GPIRT_NU_LR", "GPIRT_FSTAR_FREE")
N3, M3 = 300, 7                                       # 300: no multiple of 64 or 256, two row tiles; 7: less than one column tile


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


def _grid(k):
    return -5.0 + np.asarray(k, dtype=np.float64) * 0.01


def _constructed(n=N3, m_total=12, seed=77):
    """theta with grid points, duplicates, both grid ends, an off-grid value and a NaN; random fstar, mu_star, f over m_total
    items (the tests take column ranges of them)"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 1001, n)
    k[:8] = (0, 1000, 417, 417, 417, 0, 1000, 3)
    k[256:259] = (612, 612, 1000)                      # duplicates across the row tiles' edge
    theta = _grid(k)
    theta[11] = np.nan
    theta[12] = 0.123456
    theta[299] = np.nextafter(theta[299], 9.0)         # the last row: one ulp beside a grid point
    return dict(theta=theta, off=3, fstar=np.asfortranarray(rng.normal(size=(1001, m_total))),
                mu_star=np.asfortranarray(rng.normal(size=(1001, m_total))), f=np.asfortranarray(rng.normal(size=(n, m_total))))


def _sampler(handle, n, m, seed, item0=0, m_total=0, **kw):
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=900 + n + m)
    s = Sampler(handle, y, th0, seed=seed, item0=item0, m_total=m_total, **dict(ITEM, **kw))
    s.init()
    s.check()
    return s


def _load(s, c, cols):
    s.set("theta", c["theta"])
    for k in ("fstar", "mu_star", "f"):
        s.set(k, np.asfortranarray(c[k][:, cols]))


# ------------------------------------------------------------------------------------------------------ 3. bits ---
@pytest.mark.parametrize("item0", [0, 5])
def test_carry_bits_counters_and_determinism(handles, item0):
    from gpirt_amd import consistent as CS
    h = handles()
    seed, c = 41, _constructed()
    cols = slice(item0, item0 + M3)
    s = _sampler(h, N3, M3, seed, item0=item0, m_total=12 if item0 else 0)
    twin = _sampler(h, N3, M3, seed, item0=item0, m_total=12 if item0 else 0)
    it = s.iteration + 1
    z = CS.normals(h, seed, it, item0, M3, N3)
    assert z.shape == (N3, M3) and np.isfinite(z).all() and abs(z.mean()) < 0.1 and abs(z.std() - 1.0) < 0.1
    rng = np.random.default_rng(3)
    amps = [None] if item0 else [None, np.ones(M3), rng.uniform(0.05, 20.0, M3)]      # (amp_set is refused for an item shard)
    calls = 0
    for amp in amps:
        s.amp_set(amp)
        twin.amp_set(amp)
        for nugget in (0, 1):
            _load(s, c, cols)
            _load(twin, c, cols)
            s.carry_f(bool(nugget))
            calls += 1
            want = CS.carry_exact(c["theta"], c["fstar"][:, cols], c["mu_star"][:, cols], c["f"][:, cols], z, amp=amp, nugget=bool(nugget))
            got = s.get("f")
            assert got.tobytes() == np.asfortranarray(want).tobytes(), (item0, nugget, None if amp is None else amp[:2])
            assert got[[11, 12, 299]].tobytes() == np.asfortranarray(c["f"][:, cols])[[11, 12, 299]].tobytes()
            st = s.carry_stats()
            assert (st["calls"], st["off_grid"], st["nonfinite"]) == (calls, 3, 0)
            assert (st["total_off_grid"], st["total_nonfinite"]) == (3 * calls, 0)
            # nothing else moved, and the chain's counter stayed
            assert s.get("theta").tobytes() == c["theta"].tobytes() and s.iteration == it - 1
            assert s.get("fstar").tobytes() == np.asfortranarray(c["fstar"][:, cols]).tobytes()
            # a second identical call on a copy of the state: identical bytes
            twin.carry_f(bool(nugget))
            assert twin.get("f").tobytes() == got.tobytes()
    # a non-finite fstar cell is carried as it is and counted once per respondent on its grid point
    bad = dict(c, fstar=c["fstar"].copy())
    bad["fstar"][417, item0 + 2] = np.inf
    bad["fstar"][3, item0 + 6] = np.nan
    s.amp_set(None)
    _load(s, bad, cols)
    s.carry_f(True)
    st = s.carry_stats()
    cnt = CS.counters_exact(bad["theta"], bad["fstar"][:, cols])
    assert cnt["off_grid"] == 3 and cnt["nonfinite"] >= 4          # (rows 2, 3, 4 sit on grid point 417, row 7 on 3)
    assert (st["off_grid"], st["nonfinite"], st["total_nonfinite"], st["calls"]) == (3, cnt["nonfinite"], cnt["nonfinite"], calls + 1)
    got = s.get("f")
    want = CS.carry_exact(bad["theta"], bad["fstar"][:, cols], bad["mu_star"][:, cols], bad["f"][:, cols], z)
    assert np.isinf(got[2:5, 2]).all() and np.isnan(got[7, 6]) and np.array_equal(got, want, equal_nan=True)
    assert int((~np.isfinite(got)).sum()) == cnt["nonfinite"]
    s.close(); twin.close()


# ------------------------------------------------------------------------------------------- 4. shard invariance ---
def test_a_shard_carries_its_columns_to_the_whole_samplers_bits(handles):
    h = handles()
    seed, c = 43, _constructed(m_total=M3)
    whole = _sampler(h, N3, M3, seed)
    shard = _sampler(h, N3, 4, seed, item0=3, m_total=M3)
    _load(whole, c, slice(0, M3))
    _load(shard, c, slice(3, 7))
    whole.carry_f(True)
    shard.carry_f(True)
    fw, fs = whole.get("f"), shard.get("f")
    assert fs.tobytes() == np.asfortranarray(fw[:, 3:7]).tobytes()
    assert fw[:, 0].tobytes() != fw[:, 3].tobytes()
    whole.close(); shard.close()


# --------------------------------------------------------------------------------------------------- 5. wiring ---
STAGES = ("draw_f", "draw_fstar", "theta_partial", "theta_finish", "carry_f", "draw_beta", "factor")


def _same_state(a, b, what):
    for k in ("theta", "beta", "f", "mu", "mu_star", "fstar"):
        assert a.get(k).tobytes() == b.get(k).tobytes(), (what, k)
    assert a.iteration == b.iteration


@pytest.mark.parametrize("form", ["fused", "double_solve", "fast_2048"])
def test_the_consistent_step_is_the_seven_stage_calls(handles, form):
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    h = handles()
    if form == "fast_2048":
        y, th0 = make_responses(2048, 8, seed=21)
        kw = dict(preset="fast")
    else:
        y, th0 = make_responses(256, 16, seed=21)
        kw = dict(ITEM, fstar_fused=(form == "fused"))
    a, b = (Sampler(h, y, th0, seed=9, **kw) for _ in range(2))
    for s in (a, b):
        s.init()
    _same_state(a, b, "init")
    for it in range(3):
        a.step(consistent=True)
        for st in STAGES:
            getattr(b, st)()
        a.check(); b.check()
        _same_state(a, b, f"step {it + 1}")
    assert a.carry_stats()["calls"] == b.carry_stats()["calls"] == 3 and a.carry_stats()["total_off_grid"] == 0
    if form == "fast_2048":                             # the structured paths ran under both drivers
        assert a.factor_lr_count == b.factor_lr_count == 3 and a.nu_lr_draws == b.nu_lr_draws and a.nu_lr_draws >= 2
        assert a.fstar_free_draws == b.fstar_free_draws and a.fstar_free_draws >= 1
    # the carry is what parts it from the reference's step, whose f stays at the old theta
    c = Sampler(h, y, th0, seed=9, **kw)
    c.init()
    c.step()
    c.check()
    d = Sampler(h, y, th0, seed=9, **kw)
    d.init()
    d.step(consistent=True)
    assert c.get("theta").tobytes() == d.get("theta").tobytes() and c.get("f").tobytes() != d.get("f").tobytes()
    # timing: the six stages as before, the carry as the seventh
    d.enable_timing(True)
    d.step(consistent=True)
    t = d.stage_times()
    assert list(t) == ["draw_f", "draw_fstar", "theta_gemm", "theta_sample", "draw_beta", "factor", "carry"]
    assert all(v >= 0.0 for v in t.values()) and t["carry"] > 0.0 and t["carry"] == d.carry_stats()["time_ms"]
    d.step()
    assert "carry" not in d.stage_times()
    for s in (a, b, c, d):
        s.close()


def test_one_consistent_step_structured_factor_on_and_off(handles):
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    h = handles()
    y, th0 = make_responses(2048, 8, seed=22)
    a, b = (Sampler(h, y, th0, seed=5, **dict(FAST, factor_structured=fs)) for fs in (True, False))
    for s in (a, b):
        s.init()
        s.step(consistent=True)
        s.check()
    assert (a.factor_lr_count, b.factor_lr_count) == (1, 0)
    assert a.get("theta").tobytes() == b.get("theta").tobytes() and a.get("beta").tobytes() == b.get("beta").tobytes()
    fa, fb = a.get("f"), b.get("f")
    gap = float(np.abs(fa - fb).max()) / max(1.0, float(np.abs(fb).max()))
    print(f"MEASURED one consistent step at 2048 x 8, structured factor on / off: |f - f| / max(1, max|f|) {gap:.2e}")
    assert gap <= 1e-9
    a.close(); b.close()


# ------------------------------------------------------------------------------------- 6. the effect, on the device ---
def _q_series(s, steps, consistent):
    out = []
    for _ in range(steps):
        s.step(consistent=consistent)
        out.append(float(s.prior_quad().mean()))
    s.check()
    return np.array(out)


def test_effect_on_the_prior_quadratic_form(handles):
    """make_responses(256, 16), item RNG, 30 steps, one seed: the mean over items of || L^-1 f_j ||^2 / n over steps 6 .. 30 lies
    in [0.8, 1.25] with the consistent step and above 20 with the reference's (the CPU's 256 x 16 chains: 0.945 .. 1.064 and
    149 .. 232).  With amplitudes fixed at 0.5 (f scaled with them at the start, so the state begins as a prior draw under
    the amplitude): 10 steps, the same interval over steps 6 .. 10 for q / (n a^2)."""
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    h = handles()
    y, th0 = make_responses(256, 16, seed=31)
    q = {}
    for consistent in (True, False):
        s = Sampler(h, y, th0, seed=13, **ITEM)
        s.init()
        q[consistent] = _q_series(s, 30, consistent)[5:]
        print(f"MEASURED prior_quad().mean() over steps 6..30, consistent={consistent}: {q[consistent].min():.3f} .. {q[consistent].max():.3f}")
        s.close()
    s = Sampler(h, y, th0, seed=13, **ITEM)
    s.init()
    s.amp_set(0.5)
    s.set("f", 0.5 * s.get("f"))
    qa = _q_series(s, 10, True)[5:]
    print(f"MEASURED prior_quad().mean() over steps 6..10, amplitudes 0.5: {qa.min():.3f} .. {qa.max():.3f}")
    s.close()
    assert (q[True] >= 0.8).all() and (q[True] <= 1.25).all()
    assert (q[False] > 20.0).all()
    assert (qa >= 0.8).all() and (qa <= 1.25).all()


# ------------------------------------------------------------------------------------------------ 7. prior_quad ---
@contextlib.contextmanager
def _eligible_at_every_n(handle):
    with contextlib.ExitStack() as st:
        for k in SWITCHES:
            st.enter_context(handle.config(k, 3))
        yield


@pytest.mark.parametrize("case", ["se_dense", "se_structured", "matern52_dense", "se_amplitudes"])
def test_prior_quad_against_the_numpy_statement(handles, case):
    """Relative 1e-9 against prior_quad_exact at n = 300, m = 7 under an SE and a Matern 5/2 kernel.  The structured factor needs
    the bordered layout, which n % 64 != 0 does not have: that case runs at n = 320 (two row tiles, five 64-row blocks), where
    the factor in place IS a structured one when prior_quad is called."""
    from gpirt_amd import consistent as CS
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    kernel = dict(family="matern52", length_scale=0.7) if case.startswith("matern52") else None
    h = handles(kernel)
    structured = case == "se_structured"
    N3 = 320 if structured else 300
    y, th0 = make_responses(N3, M3, seed=51)
    kw = dict(FAST, factor_structured=True) if structured else dict(ITEM, fstar_fused=True)
    s = Sampler(h, y, th0, seed=3, **kw)
    s.init()
    rng = np.random.default_rng(8)
    # a smooth part plus roughness: both ends of S's spectrum carry weight
    f = np.asfortranarray(np.sin(th0)[:, None] * rng.normal(size=(1, M3)) + 0.05 * rng.normal(size=(N3, M3)))
    amp = rng.uniform(0.2, 5.0, M3) if case == "se_amplitudes" else None
    with _eligible_at_every_n(h) if structured else contextlib.nullcontext():
        if structured:
            s.factor()                                  # (init's factor is the dense one: this one is structured)
            assert s.factor_lr_count == 1
        s.set("f", f)
        if amp is not None:
            s.amp_set(amp)
        theta, it, d0 = s.get("theta"), s.iteration, s.dense_factor_count
        got = s.prior_quad()
        # documented: a structured factor is replaced by the dense one (one dense factorisation), otherwise none is enqueued
        assert s.dense_factor_count - d0 == (1 if structured else 0)
        again = s.prior_quad()
        assert s.dense_factor_count - d0 == (1 if structured else 0) and again.tobytes() == got.tobytes()
    assert s.get("f").tobytes() == f.tobytes() and s.get("theta").tobytes() == theta.tobytes() and s.iteration == it
    assert theta.tobytes() == th0.tobytes()
    want = CS.prior_quad_exact(th0, f, kernel, amp=amp)
    rel = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"MEASURED {case}: prior_quad {got.min():.4g} .. {got.max():.4g}, max relative gap to the NumPy statement {rel:.2e}")
    assert got.shape == (M3,) and np.all(np.abs(got - want) <= 1e-9 * np.abs(want))
    s.check()
    s.close()


# ------------------------------------------------------------------------------------------------- 8. refusals ---
def test_refusals_name_their_reason(handles):
    from gpirt_amd import _lib
    from gpirt_amd.ops import RStream
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    h = handles()
    y, th0 = make_responses(40, 3, seed=2)
    s = Sampler(h, y, th0, seed=1, **ITEM)
    for call in (lambda: s.carry_f(), lambda: s.step(consistent=True), lambda: s.prior_quad()):
        with pytest.raises(_lib.GpirtError, match=r"needs an initialised sampler \(gpirt_sampler_init\)"):
            call()
    s.init()
    for call in (lambda: s.carry_f(nugget=2), lambda: s.step(consistent=True, nugget=2)):
        with pytest.raises(_lib.GpirtError, match="nugget = 2, it must be 0 or 1"):
            call()
    f0, it0 = s.get("f"), s.iteration
    assert s.carry_stats() == dict(calls=0, off_grid=0, nonfinite=0, total_off_grid=0, total_nonfinite=0, time_ms=0.0)
    r = Sampler(h, y, th0, rng="reference", rstream=RStream(7))
    r.init()
    for call in (lambda: r.carry_f(), lambda: r.step(consistent=True)):
        with pytest.raises(_lib.GpirtError, match="R's stream has no such draw"):
            call()
    assert r.iteration == 0 and s.get("f").tobytes() == f0.tobytes() and s.iteration == it0
    r.step()                                            # the reference's step is what it was
    r.check()
    s.close(); r.close()
