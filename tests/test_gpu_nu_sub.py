"""draw_f's structured product in parts of its own width (gpirt_amd/csrc/nu_lr.hip, GPIRT_NU_SUB = 64, 128, 256 or 512; the
factor's parts stay 512 wide) with the rank-64 term accumulated in the launch of the diagonal parts:

    nu[P, :] = L[P, P] Z[P, :] + V[P, :] sum_{Q < P} Bt[:, Q] Z[Q, :]      for parts P of GPIRT_NU_SUB columns.

Against the dense product (GPIRT_NU_LR=2) on the same sampler state the bound is tests/test_gpu_nu_lr.py's
1e-10 * max(1, max|nu|), on nu and on f after the slice update, at every width: the identity behind the product holds for any
cut into multiples of 64 (tests/test_nu_sub_cpu.py: 2e-13 .. 5e-12 on the CPU at every width).  Everything else here is
equality of bits: item shards, repeated draws, poisoned allocations, a width changed on a live sampler."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAST = dict(rng="item", fstar_fused=True, kstar_rank=64, theta_stabilise=True)
BOUND = 1e-10
WIDTHS = (64, 128, 256, 512)
GRID = -5.0 + 0.01 * np.arange(1001)


def _theta(start, n, th0):
    r = np.random.default_rng(7000 + n)
    if start == "grid":
        return th0                                  # (two steps follow: draw_theta's values are grid values)
    if start == "sorted":
        return np.sort(GRID[np.clip(np.rint((r.standard_normal(n) + 5.0) / 0.01).astype(int), 0, 1000)])
    if start == "all_equal":
        return np.full(n, GRID[617])
    if start == "off_grid":
        return r.uniform(-5.0, 5.0, n)
    raise ValueError(start)


def _draw(handle, s, f0, mode, width=None):
    """one draw_f from the state with f = f0 under GPIRT_NU_LR = mode [and GPIRT_NU_SUB = width]: (nu, f, ess_k)"""
    s.set("f", f0)
    before = s.nu_lr_draws
    with handle.config("GPIRT_NU_LR", mode):
        if width is None:
            s.draw_f()
        else:
            with handle.config("GPIRT_NU_SUB", width):
                s.draw_f()
        s.check()
    assert s.nu_lr_draws - before == (1 if mode == 3 else 0), (mode, width, s.nu_lr_draws, before)
    return s.get("nu"), s.get("f"), s.get("ess_k")


def _sampler(handle, n, m, seed, theta=None, **extra):
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=seed)
    kw = dict(FAST)
    kw.update(extra)
    s = Sampler(handle, y, th0 if theta is None else theta(th0), seed=17, **kw)
    s.init()
    return s


@pytest.mark.parametrize("m", [3, 70])
@pytest.mark.parametrize("n", [64, 128, 192, 320, 576, 1088])
@pytest.mark.parametrize("start", ["grid", "sorted", "all_equal", "off_grid"])
def test_every_width_against_the_dense_product_on_the_same_state(handle, start, n, m):
    s = _sampler(handle, n, m, 311 + n, theta=lambda th0: _theta(start, n, th0))
    if start == "grid":
        with handle.config("GPIRT_NU_LR", 3):
            for _ in range(2):
                s.step()
        s.check()
        kk = (s.get("theta") + 5.0) / 0.01
        assert np.abs(kk - np.rint(kk)).max() < 1e-9
    f0 = s.get("f")
    nu2, f2, _ = _draw(handle, s, f0, 2)
    scale = max(1.0, float(np.abs(nu2).max()))
    got = {w: _draw(handle, s, f0, 3, w) for w in WIDTHS}
    s.close()
    for w, (nu3, f3, _) in got.items():
        dnu, df = float(np.abs(nu3 - nu2).max()), float(np.abs(f3 - f2).max())
        msg = "n = %d, m = %d, theta %s, width %d: max|nu_lr - nu_dense| = %.3e, max|f_lr - f_dense| = %.3e, max|nu| = %.3f" % (
            n, m, start, w, dnu, df, float(np.abs(nu2).max()))
        print(msg)
        assert np.isfinite(nu3).all() and np.isfinite(f3).all(), msg
        assert dnu <= BOUND * scale, msg
        assert df <= BOUND * scale, msg


@pytest.mark.parametrize("width", WIDTHS)
def test_an_item_shard_draws_the_same_f_at_every_width(handle, width):
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    n, m, j0 = 320, 96, 64
    y, th0 = make_responses(n, m, seed=5)
    a = Sampler(handle, y, th0, seed=5, **FAST)
    c = Sampler(handle, y[:, j0:m], th0, seed=5, item0=j0, m_total=m, **FAST)
    a.init()
    c.init()
    for k in ("f", "mu", "beta"):                          # the same chain state for the shard's columns
        c.set(k, a.get(k)[:, j0:])
    nu_a, f_a, k_a = _draw(handle, a, a.get("f"), 3, width)
    nu_c, f_c, k_c = _draw(handle, c, c.get("f"), 3, width)
    a.close(); c.close()
    assert np.array_equal(nu_c, nu_a[:, j0:])
    assert np.array_equal(f_c, f_a[:, j0:])
    assert np.array_equal(k_c, k_a[j0:])


def test_the_same_state_drawn_twice_gives_equal_bits(handle):
    s = _sampler(handle, 576, 70, 23)
    f0 = s.get("f")
    for w in WIDTHS:
        first, second = _draw(handle, s, f0, 3, w), _draw(handle, s, f0, 3, w)
        assert all(np.array_equal(x, y) for x, y in zip(first, second)), w
    s.close()


def test_a_width_changed_on_a_live_sampler_gives_what_a_fresh_one_gives(handle):
    n, m = 1088, 70
    fresh = {}
    for w in (64, 512):
        s = _sampler(handle, n, m, 29)
        fresh[w] = _draw(handle, s, s.get("f"), 3, w)
        s.close()
    s = _sampler(handle, n, m, 29)
    f0 = s.get("f")
    for w in (64, 512, 64):                                # (the narrow draw leaves 16 slabs, the wide one rewrites two of them)
        got = _draw(handle, s, f0, 3, w)
        assert all(np.array_equal(x, y) for x, y in zip(got, fresh[w])), w
    s.close()


def test_the_first_draw_of_a_fresh_sampler_does_not_read_poison():
    import torch
    from gpirt_amd import _lib
    from gpirt_amd.ops import Handle
    lib = _lib.load()
    out = {}
    for poison in (False, True):
        torch.cuda.synchronize()
        h = Handle()
        try:
            _lib.check(lib.gpirt_debug_poison_allocs(h._h, int(poison)))
            for w in WIDTHS:
                s = _sampler(h, 320, 70, 41)
                out[poison, w] = _draw(h, s, s.get("f"), 3, w)
                s.close()
        finally:
            h.close()
    for w in WIDTHS:
        assert np.isfinite(out[True, w][0]).all(), w
        assert all(np.array_equal(x, y) for x, y in zip(out[False, w], out[True, w])), w


def test_an_invalid_width_is_refused_and_the_draws_stay_structured(handle):
    from gpirt_amd._lib import GpirtError
    s = _sampler(handle, 320, 3, 9)
    f0 = s.get("f")
    default = handle.config_get("GPIRT_NU_SUB")
    assert default in WIDTHS
    for bad in (0, 32, 96, 1024, -64):
        with pytest.raises(GpirtError):
            handle.config_set("GPIRT_NU_SUB", bad)
        assert handle.config_get("GPIRT_NU_SUB") == default
    before = s.nu_lr_draws
    _draw(handle, s, f0, 3)
    _draw(handle, s, f0, 3, 256)
    assert s.nu_lr_draws == before + 2
    s.close()
