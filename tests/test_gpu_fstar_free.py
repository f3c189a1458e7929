"""The rank-64 draw_fstar's C = S^-1 K(theta, c) from theta alone (gpirt_amd/csrc/fstar_free.hip):
C = V M with V the Lagrange basis of the 64 nodes at theta and M = F (F^T (V^T V) F + 0.001 I)^-1 F^T, instead of the transposed
solve through L.  GPIRT_FSTAR_FREE: 1 = the default rule (n >= 2048 and eligible), 2 = always through L, 3 = at every eligible n.

One draw_fstar under the switch at 3 against one under 2 from the same sampler state: s must be the same bits (G = B^T B is
formed as before), mean and f* agree to 1e-9 max(1, max|.|) for a generic theta and to the forward error of S x = f,
8 n u cond(S), for a theta on one point, on two points 0.01 apart and at +-5 (tests/test_gpu_fstar_ranks.py's patterns and
bound).  m = 8; n = 320 and 1088."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAST = dict(rng="item", fstar_fused=True, kstar_rank=64, theta_stabilise=True)
M = 8
U = 2.0 ** -53
SWITCH = "GPIRT_FSTAR_FREE"
OUT = ("s", "mean", "fstar")


def _off_grid(n, seed):
    """theta_init inside [-5, 5], on no grid point and on no node"""
    r = np.random.default_rng(seed)
    return np.clip(1.7 * r.standard_normal(n), -4.99, 4.99) + 1e-3 * r.random(n) * 0.37


def _sampler(handle, n, m=M, theta=None, seed=17, y_seed=311, **kw):
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=y_seed + n)
    return Sampler(handle, y, th0 if theta is None else theta, seed=seed, **dict(FAST, **kw))


def _both(handle, s, modes=(3, 2), side=False):
    """draw_fstar under each mode of the switch on the state `s` is in: ((s, mean, fstar), calls that took the new path) per
    mode.  side=False: C is formed inside draw_fstar; side=True: by the chain draw_f starts on the sampler's own stream
    (draw_f does not depend on the switch: the same f follows the same f0 both times)."""
    f0 = s.get("f")
    out = []
    for mode in modes:
        s.set("f", f0)                                   # (whatever was derived from the factor is formed again)
        before = s.fstar_free_draws
        with handle.config(SWITCH, mode):
            if side:
                s.draw_f()
            s.draw_fstar()
            s.check()
        out.append(({k: np.array(s.get(k)) for k in OUT}, s.fstar_free_draws - before))
    return out


def _gaps(new, old):
    return {k: float(np.abs(new[k] - old[k]).max()) / max(1.0, float(np.abs(old[k]).max())) for k in ("mean", "fstar")}


def _patterns(n):
    g = -5.0 + np.arange(1001, dtype=np.float64) * 0.01
    one = np.full(n, g[617])
    two = np.where(np.arange(n) % 2 == 0, g[400], g[401])
    ends = np.where(np.arange(n) < n // 2, -5.0, 5.0)
    return {"one_point": one, "two_points_0.01_apart": two, "plus_minus_5": ends}


@pytest.mark.parametrize("side", [False, True], ids=["in_draw_fstar", "beside_draw_f"])
@pytest.mark.parametrize("n", [320, 1088])
@pytest.mark.parametrize("start", ["grid", "off_grid"])
def test_generic_theta(handle, start, n, side):
    s = _sampler(handle, n, theta=_off_grid(n, n) if start == "off_grid" else None)
    s.init()
    if start == "grid":
        for _ in range(2):
            s.step()
        s.check()
        kk = (s.get("theta") + 5.0) / 0.01
        assert np.abs(kk - np.rint(kk)).max() < 1e-9
    (new, c3), (old, c2) = _both(handle, s, side=side)
    s.close()
    assert (c3, c2) == (1, 0)
    g = _gaps(new, old)
    print(f"MEASURED theta {start} n={n} {'side' if side else 'inline'}: |mean - mean_L| {g['mean']:.2e}  |f* - f*_L| {g['fstar']:.2e}"
          f"  (relative to max(1, max|.|)); max|f*| {np.abs(old['fstar']).max():.3f}")
    assert np.array_equal(new["s"], old["s"])
    assert np.isfinite(new["mean"]).all() and np.isfinite(new["fstar"]).all()
    assert g["mean"] <= 1e-9 and g["fstar"] <= 1e-9, g


@pytest.mark.parametrize("n", [320, 1088])
@pytest.mark.parametrize("pattern", ["one_point", "two_points_0.01_apart", "plus_minus_5"])
def test_constructed_theta(handle, pattern, n):
    s = _sampler(handle, n)
    s.init()
    s.draw_f()
    s.set("theta", _patterns(n)[pattern])
    s.factor()
    (new, c3), (old, c2) = _both(handle, s)
    cond = float(np.linalg.cond(np.array(s.get("L")), 2) ** 2)         # cond_2(S) = cond_2(L)^2, of the device's own factor
    s.close()
    assert (c3, c2) == (1, 0)
    tol = 8 * n * U * cond
    g = _gaps(new, old)
    print(f"MEASURED {pattern} n={n}: |mean - mean_L| {g['mean']:.2e}  |f* - f*_L| {g['fstar']:.2e}  (tolerance {tol:.2e}, cond(S) {cond:.2e})")
    assert np.array_equal(new["s"], old["s"])
    assert np.isfinite(new["mean"]).all() and np.isfinite(new["fstar"]).all()
    assert g["mean"] <= tol and g["fstar"] <= tol, (g, tol)


def test_an_item_shard_draws_the_same_fstar_as_the_full_problem(handle):
    n, m = 1088, 16
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=5)
    a = Sampler(handle, y, th0, seed=5, **FAST)
    shards = [Sampler(handle, y[:, j0:j0 + 8], th0, seed=5, item0=j0, m_total=m, **FAST) for j0 in (0, 8)]
    with handle.config(SWITCH, 3):
        a.init()
        for j0, c in zip((0, 8), shards):
            c.init()
            for k in ("f", "mu", "beta"):
                c.set(k, a.get(k)[:, j0:j0 + 8])
            c.set("mu_star", a.get("mu_star")[:, j0:j0 + 8])
        before = [c.fstar_free_draws for c in [a] + shards]          # (init draws an f* of its own)
        a.draw_f(); a.draw_fstar(); a.check()
        full = a.get("fstar")
        for j0, c in zip((0, 8), shards):
            c.draw_f(); c.draw_fstar(); c.check()
            assert np.array_equal(c.get("f"), a.get("f")[:, j0:j0 + 8])
            assert np.array_equal(c.get("fstar"), full[:, j0:j0 + 8]), j0
    assert [c.fstar_free_draws - b for c, b in zip([a] + shards, before)] == [1, 1, 1]
    a.close()
    for c in shards:
        c.close()


def _falls_back(handle, s, modes=(3, 2), side=False):
    (new, c_new), (old, c_old) = _both(handle, s, modes=modes, side=side)
    assert (c_new, c_old) == (0, 0), (c_new, c_old)
    for k in OUT:                                           # (bytes: a theta that L does not belong to gives NaN cells in both)
        assert new[k].tobytes() == old[k].tobytes(), k


def test_fall_backs_take_the_chain_through_L_and_say_so(handle):
    from gpirt_amd import ell as E
    from gpirt_amd.ops import Handle
    n = 320
    assert handle.config_get(SWITCH) == 1
    for kw in (dict(kernel_fp32=True), dict(kstar_rank=128)):
        for side in (False, True):
            s = _sampler(handle, n, **kw)
            s.init()
            _falls_back(handle, s, side=side)
            s.close()
    hm = Handle(kernel="matern52")                          # no rank form: the full solve, whatever the switch says
    try:
        s = _sampler(hm, n, kstar_rank=0)
        s.init()
        _falls_back(hm, s)
        s.close()
    finally:
        hm.close()
    # theta set from outside with no factorisation behind it: L need not be the factor of K(theta, theta)
    s = _sampler(handle, n)
    s.init()
    s.set("theta", np.roll(s.get("theta"), 7))
    _falls_back(handle, s)
    s.factor()                                              # ... and with one behind it the new path is back
    (_, c3), (_, c2) = _both(handle, s)
    assert (c3, c2) == (1, 0)
    s.close()
    # the default rule starts at n = 2048
    s = _sampler(handle, 1088)
    s.init()
    _falls_back(handle, s, modes=(1, 2))
    _falls_back(handle, s, modes=(1, 2), side=True)
    s.close()
    # the length scale is being sampled: F belongs to a kernel that moves
    lo, hi, points = 0.7, 2.8, 5                            # (rank 64 passes its certificate at 0.7)
    he = Handle(kernel=dict(family="se", length_scale=float(E.grid(lo, hi, points)[2])))
    try:
        s = _sampler(he, n)
        s.init()
        s.ell_enable(lo, hi, points, width=2)
        _falls_back(he, s)
        _falls_back(he, s, side=True)
        s.ell_enable(on=False)                              # off again: the new path, with F for the kernel as it stands
        (new, c3), (old, c2) = _both(he, s)
        assert (c3, c2) == (1, 0)
        g = _gaps(new, old)
        assert np.array_equal(new["s"], old["s"]) and g["mean"] <= 1e-9 and g["fstar"] <= 1e-9, g
        s.close()
    finally:
        he.close()


def test_three_whole_steps_under_the_default_rule_against_the_fused_form(handle):
    n = 2112
    assert handle.config_get(SWITCH) == 1
    a = _sampler(handle, n)
    b = _sampler(handle, n, kstar_rank=0)
    for c in (a, b):
        c.init()
    before = a.fstar_free_draws                             # (init draws an f* of its own)
    for it in range(3):
        for c in (a, b):
            c.step()
            c.check()
        fa, fb = a.get("fstar"), b.get("fstar")
        gap = float(np.abs(fa - fb).max()) / float(np.abs(fb).max())
        print(f"MEASURED step {it + 1} at {n} x {M}: |f* - f*_fused| / max|f*| {gap:.2e}")
        assert np.array_equal(a.get("theta"), b.get("theta"))
        assert np.array_equal(a.get("f"), b.get("f"))
        assert gap <= 1e-9
    assert a.fstar_free_draws - before == 3 and b.fstar_free_draws == 0
    a.close(); b.close()
