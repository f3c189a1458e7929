"""The structured factor (gpirt_amd/csrc/factor_lr.hip): with gpirt_options.factor_structured a
factorisation builds only L's 512-column diagonal parts and the 64 node rows K(c, theta) L^-T, from theta alone.
GPIRT_FACTOR_LR: 1 = the default rule (n >= 2048 and eligible), 2 = always the dense factor, 3 = at every eligible n (the rule
also asks what the structured nu = L z and C from theta alone ask, so the small sizes here run with all three switches at 3).

Bounds (tests/test_factor_lr_cpu.py has the NumPy statement's figures): 1e-10 on the parts, 1e-9 on the node rows and on f*
relative to max|f*|, 1e-10 max(1, max|f|) on f.  m = 8."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAST = dict(rng="item", fstar_fused=True, kstar_rank=64, theta_stabilise=True)
M = 8
SWITCH = "GPIRT_FACTOR_LR"
SWITCHES = (SWITCH, "GPIRT_NU_LR", "GPIRT_FSTAR_FREE")
KINDS = ["grid_normal", "grid_uniform", "off_grid", "sorted", "all_equal", "half_minus5_half_plus5", "two_points_0.01_apart"]


def theta_case(kind, n):
    rng = np.random.default_rng(2000 + n)
    g = -5.0 + np.arange(1001, dtype=np.float64) * 0.01
    normal = lambda: g[np.clip(np.rint((rng.standard_normal(n) + 5.0) / 0.01).astype(int), 0, 1000)]
    return {"grid_normal": normal, "grid_uniform": lambda: g[rng.integers(0, 1001, n)], "off_grid": lambda: rng.uniform(-5.0, 5.0, n),
            "sorted": lambda: np.sort(normal()), "all_equal": lambda: np.full(n, g[617]),
            "half_minus5_half_plus5": lambda: np.where(np.arange(n) < n // 2, -5.0, 5.0),
            "two_points_0.01_apart": lambda: np.where(np.arange(n) % 2 == 0, g[400], g[401])}[kind]()


@contextlib.contextmanager
def eligible_at_every_n(handle):
    with contextlib.ExitStack() as st:
        for k in SWITCHES:
            st.enter_context(handle.config(k, 3))
        yield


def _sampler(handle, n, m=M, structured=True, seed=17, **kw):
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=311 + n)
    return Sampler(handle, y, th0, seed=seed, **dict(FAST, factor_structured=structured, **kw))


def _parts_of(L):
    n = L.shape[0]
    return [L[p:p + 512, p:p + 512] for p in range(0, n, 512)]


@pytest.mark.parametrize("n", [64, 512, 576, 1088, 1536])
def test_parts_and_node_rows_against_the_dense_factor(handle, n):
    s = _sampler(handle, n)
    s.init()
    with eligible_at_every_n(handle):
        for kind in KINDS:
            s.set("theta", theta_case(kind, n))
            c0, d0 = s.factor_lr_count, s.dense_factor_count
            s.factor()
            s.check()
            parts, rows = s.factor_lr_parts(), np.array(s.nu_lr_rows())
            assert (s.factor_lr_count - c0, s.dense_factor_count - d0) == (1, 0)
            with handle.config(SWITCH, 2):
                s.factor()
                s.check()
            assert (s.factor_lr_count - c0, s.dense_factor_count - d0) == (1, 1)
            L, rows_dense = np.array(s.get("L")), np.array(s.nu_lr_rows())
            assert s.dense_factor_count - d0 == 1
            dense = _parts_of(L)
            assert [p.shape for p in parts] == [p.shape for p in dense]
            gap_parts = max(float(np.abs(a - b).max()) for a, b in zip(parts, dense))
            gap_rows = float(np.abs(rows - rows_dense).max())
            pivot = min(float(np.diag(a).min()) for a in parts)
            print(f"MEASURED {kind} n={n}: parts {gap_parts:.2e}, node rows {gap_rows:.2e}, smallest pivot {pivot:.4f}")
            for a in parts:
                assert np.array_equal(a, np.tril(a)), "strict upper triangle inside a part"
            assert pivot >= 0.03
            assert gap_parts <= 1e-10
            assert gap_rows <= 1e-9
    s.close()


def test_three_whole_steps_against_the_option_off(handle):
    n = 1088
    a, b = _sampler(handle, n), _sampler(handle, n, structured=False)
    with eligible_at_every_n(handle):
        for c in (a, b):
            c.init()
        for it in range(3):
            for c in (a, b):
                c.step()
                c.check()
            fa, fb, sa, sb = a.get("f"), b.get("f"), a.get("fstar"), b.get("fstar")
            gap_f = float(np.abs(fa - fb).max()) / max(1.0, float(np.abs(fb).max()))
            gap_s = float(np.abs(sa - sb).max()) / float(np.abs(sb).max())
            print(f"MEASURED step {it + 1} at {n} x {M}: |f - f_dense| / max(1, max|f|) {gap_f:.2e}, |f* - f*_dense| / max|f*| {gap_s:.2e}")
            assert np.array_equal(a.get("theta"), b.get("theta"))
            assert np.array_equal(a.get("ess_k"), b.get("ess_k"))
            assert gap_f <= 1e-10
            assert gap_s <= 1e-9
    assert (a.factor_lr_count, b.factor_lr_count) == (3, 0)
    assert a.dense_factor_count == 1 and b.dense_factor_count == 4          # (init's factor is the dense one)
    a.close(); b.close()


def test_the_dense_factor_is_formed_on_demand(handle):
    n = 1088
    a, b = _sampler(handle, n), _sampler(handle, n, structured=False)
    fused = _sampler(handle, n, structured=False, kstar_rank=0)
    with eligible_at_every_n(handle):
        for c in (a, b, fused):
            c.init()
        a.factor(); b.factor()
        d0 = a.dense_factor_count
        La, Lb = np.array(a.get("L")), np.array(b.get("L"))
        assert a.dense_factor_count == d0 + 1
        gap = float(np.abs(La - Lb).max())
        print(f"MEASURED n={n}: |get('L') behind a structured factor - dense L| {gap:.2e}")
        assert gap <= 1e-10
        assert np.array_equal(np.array(a.get("L")), La) and a.dense_factor_count == d0 + 1      # no second factorisation
        # copy_state_from hands the whole factor on
        c0 = a.factor_lr_count
        a.factor()
        assert a.factor_lr_count == c0 + 1
        a.draw_f(); a.draw_fstar(); a.check()
        fused.copy_state_from(a)
        fused.draw_fstar(); fused.check()
        src, got = a.get("fstar"), fused.get("fstar")
        gap = float(np.abs(got - src).max()) / float(np.abs(src).max())
        print(f"MEASURED n={n}: |f*(fused, copied state) - f*(source)| / max|f*| {gap:.2e}")
        assert gap <= 1e-9
        # the factor in place belongs to the theta it was built from, whatever theta holds now
        theta_old = np.array(a.get("theta"))
        a.factor()
        b.set("theta", theta_old); b.factor()
        a.set("theta", np.roll(theta_old, 7))
        gap = float(np.abs(np.array(a.get("L")) - np.array(b.get("L"))).max())
        print(f"MEASURED n={n}: |get('L') after set('theta') - dense L of the old theta| {gap:.2e}")
        assert gap <= 1e-10
    for c in (a, b, fused):
        c.close()


def _structured_factors(s):
    before = s.factor_lr_count
    s.factor()
    s.check()
    return s.factor_lr_count - before


def test_fall_backs_take_the_dense_factor_and_say_so(handle):
    from gpirt_amd import ell as E
    from gpirt_amd.ops import Handle
    n = 576
    assert handle.config_get(SWITCH) == 1
    with eligible_at_every_n(handle):
        s = _sampler(handle, n)
        s.init()
        assert _structured_factors(s) == 1                       # (the control: this sampler is eligible)
        with handle.config(SWITCH, 2):
            assert _structured_factors(s) == 0
        th = np.array(s.get("theta")); th[3] = 5.5               # a theta outside the nodes' interval
        s.set("theta", th)
        assert _structured_factors(s) == 0
        s.close()
        for kw in (dict(structured=False), dict(kernel_fp32=True), dict(kstar_rank=0), dict(kstar_rank=128)):
            s = _sampler(handle, n, **kw)
            s.init()
            assert _structured_factors(s) == 0, kw
            s.close()
    s = _sampler(handle, 1088)                                   # the default rule starts at n = 2048
    s.init()
    assert _structured_factors(s) == 0
    s.close()
    hm = Handle(kernel="matern52")
    try:
        with eligible_at_every_n(hm):
            s = _sampler(hm, n, kstar_rank=0)
            s.init()
            assert _structured_factors(s) == 0
            s.close()
    finally:
        hm.close()
    lo, hi, points = 0.7, 2.8, 5
    he = Handle(kernel=dict(family="se", length_scale=float(E.grid(lo, hi, points)[2])))
    try:
        with eligible_at_every_n(he):
            s = _sampler(he, n)
            s.init()
            assert _structured_factors(s) == 1
            s.ell_enable(lo, hi, points, width=2)                # the length scale is being sampled: every factor is dense
            assert _structured_factors(s) == 0
            s.close()
    finally:
        he.close()


def test_item_shards_and_repeated_runs_give_the_same_bits(handle):
    n, m = 1088, 8
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=5)
    kw = dict(FAST, factor_structured=True)
    a = Sampler(handle, y, th0, seed=5, **kw)
    shards = [Sampler(handle, y[:, j0:j0 + 4], th0, seed=5, item0=j0, m_total=m, **kw) for j0 in (0, 4)]
    with eligible_at_every_n(handle):
        a.init()
        for j0, c in zip((0, 4), shards):
            c.init()
            for k in ("f", "mu", "beta"):
                c.set(k, a.get(k)[:, j0:j0 + 4])
        a.factor()
        parts, rows = a.factor_lr_parts(), np.array(a.nu_lr_rows())
        it = a.iteration
        a.factor()                                               # the same sampler once more: the same bits
        a.set_iteration(it)                                      # (draw_f's normals are keyed by the iteration: the shards' one)
        assert all(np.array_equal(p, q) for p, q in zip(parts, a.factor_lr_parts())) and np.array_equal(rows, np.array(a.nu_lr_rows()))
        a.draw_f(); a.check()
        for j0, c in zip((0, 4), shards):
            c.factor()
            assert all(np.array_equal(p, q) for p, q in zip(parts, c.factor_lr_parts())), j0
            assert np.array_equal(rows, np.array(c.nu_lr_rows())), j0
            c.draw_f(); c.check()
            assert np.array_equal(c.get("f"), a.get("f")[:, j0:j0 + 4]), j0
    assert [c.factor_lr_count for c in [a] + shards] == [2, 1, 1]
    a.close()
    for c in shards:
        c.close()


def test_a_nan_in_theta_is_reported_by_check():
    """set("theta") looks at the host array: a NaN is not inside [-5, 5], so the factorisation that follows is the dense one
    and check() reports its failed pivot.  Nothing hangs and nothing faults."""
    from gpirt_amd.ops import Handle
    n = 576
    h = Handle()
    try:
        with eligible_at_every_n(h):
            s = _sampler(h, n)
            s.init()
            th = np.array(s.get("theta"))
            th[100] = np.nan
            s.set("theta", th)
            before = s.factor_lr_count
            with pytest.raises(RuntimeError):
                s.factor()
                s.check()
            assert s.factor_lr_count == before
            s.close()
    finally:
        h.close()
