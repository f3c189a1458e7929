"""draw_f's slice kernel with y packed and mu formed again from theta and beta (gpirt_amd/csrc/ess_lin.hip, GPIRT_ESS_PACK,
library version 143) against the kernel that reads y and mu.

Everything here is equality of bits: f, the rejection counts and the error code of Handle.draw_f_linear (or of a sampler under
GPIRT_ESS_PACK=1 / 3) against Handle.draw_f (GPIRT_ESS_PACK=2) on mu = b0 + theta * b1, formed on the host as a separate
multiply and add, with the same seed and iteration.  L = sigma I is built on the device, so nu = sigma z is common to both.

Orders: 2049 (the first of the class, most rows of a lane past the end), 4100, 8191 and 8192 (the last row of the last lane,
the end of theta in LDS and of the mask word); m = 5, and once m = 2 x (CU count) + 3 under GPIRT_ESS_PACK=3, where a
work-group strides over more than one item and the last ones take fewer."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GRID = -5.0 + 0.01 * np.arange(1001)
ORDERS = (2049, 4100, 8191, 8192)
_L = {}                                   # n -> (identity on the device, its current diagonal value)


def _eye(n, sigma):
    import torch
    if n not in _L:
        _L.clear()                        # (one order at a time: 8192^2 doubles are 512 MB)
        _L[n] = torch.zeros((n, n), dtype=torch.float64, device="cuda").T
    _L[n].diagonal().fill_(sigma)
    return _L[n]


def _state(n, m, nan_frac, seed):
    """f, y (+1 / -1 / NaN), theta on the grid, beta (2 x m) and mu = b0 + theta * b1 as two roundings"""
    r = np.random.default_rng(seed)
    F = np.asfortranarray(r.standard_normal((n, m)))
    Y = np.asfortranarray(np.where(r.random((n, m)) < 0.5, 1.0, -1.0))
    Y[r.random((n, m)) < nan_frac] = np.nan
    theta = GRID[r.integers(0, 1001, n)]
    beta = np.asfortranarray(np.vstack([r.standard_normal(m), 1.0 + 0.5 * r.standard_normal(m)]))
    return F, Y, theta, beta


def _mu(theta, beta):
    prod = theta[:, None] * beta[1][None, :]
    return np.asfortranarray(beta[0][None, :] + prod)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _draw(handle, n, F, Y, theta, beta, sigma, seed, it, packed):
    """(error code, f', k) of one draw through the C entry itself: a failing draw still hands back f and k"""
    import torch
    from gpirt_amd.ops import _ld, _p, to_device, to_host
    m = F.shape[1]
    L = _eye(n, sigma)
    f, y = to_device(F), to_device(Y)
    k = torch.full((m,), -1, dtype=torch.int32, device="cuda")
    if packed:
        th, be = to_device(theta), to_device(beta)
        rc = handle.lib.gpirt_draw_f_linear(handle._h, _p(f), _p(y), _p(L), _ld(L), _p(th), _p(be), n, m, seed, it, _p(k))
    else:
        mu = to_device(_mu(theta, beta))
        rc = handle.lib.gpirt_draw_f(handle._h, _p(f), _p(y), _p(L), _ld(L), _p(mu), n, m, seed, it, _p(k))
    torch.cuda.synchronize()
    return int(rc), to_host(f), k.cpu().numpy()


def _same(handle, n, F, Y, theta, beta, sigma, seed, it, what, modes=(1, 3)):
    """the packed kernel under each mode against the kernel that reads y and mu; returns the old path's (rc, f, k)"""
    old = _draw(handle, n, F, Y, theta, beta, sigma, seed, it, False)
    for mode in modes:
        with handle.config("GPIRT_ESS_PACK", mode):
            new = _draw(handle, n, F, Y, theta, beta, sigma, seed, it, True)
        assert new[0] == old[0], (what, mode, "error code", new[0], old[0])
        bad = np.flatnonzero(new[2] != old[2])
        assert bad.size == 0, (what, mode, "k", [(int(j), int(new[2][j]), int(old[2][j])) for j in bad[:8]])
        diff = np.argwhere(_bits(new[1]) != _bits(old[1]))
        assert diff.size == 0, (what, mode, "f", len(diff), diff[:4].tolist())
    return old


@pytest.mark.parametrize("nan_frac", [0.05, 0.5])
@pytest.mark.parametrize("n", ORDERS)
def test_random_y_every_order(handle, n, nan_frac):
    F, Y, theta, beta = _state(n, 5, nan_frac, 4100 + n)
    rc, f, k = _same(handle, n, F, Y, theta, beta, 1.0, 77, 3, ("default", n, nan_frac))
    assert rc == 0 and not np.array_equal(f, F)
    with handle.config("GPIRT_ESS_SCREEN", 2):              # every trial point in full precision
        rc2, f2, k2 = _same(handle, n, F, Y, theta, beta, 1.0, 77, 3, ("screen off", n, nan_frac))
    assert rc2 == 0 and np.array_equal(k2, k) and np.array_equal(_bits(f2), _bits(f))
    with handle.config("GPIRT_LL_EXACT", 1):                # the term as written, through the library's exp and log
        rc3, _, _ = _same(handle, n, F, Y, theta, beta, 1.0, 77, 3, ("ll exact", n, nan_frac))
        assert rc3 == 0
        with handle.config("GPIRT_ESS_SCREEN", 2):
            _same(handle, n, F, Y, theta, beta, 1.0, 77, 3, ("ll exact, screen off", n, nan_frac))


def test_a_striding_work_group_takes_several_items(handle):
    import torch
    n = 2049
    m = 2 * torch.cuda.get_device_properties(0).multi_processor_count + 3
    F, Y, theta, beta = _state(n, m, 0.05, 99)
    rc, _, k = _same(handle, n, F, Y, theta, beta, 1.0, 5, 9, ("striding", m))
    assert rc == 0 and k.max() >= 1


def test_mask_layout_every_bit_position(handle):
    """bit e of a lane's word is row lane + 512 e, bit 16 + e its sign: a column whose only observed row is that one (positive,
    then negative), for a lane of the first wave and one of the last, at every e; a column with no observed row and one with
    none missing"""
    n = 8192
    rows = [lane + 512 * e for e in range(16) for lane in (5, 505)]
    m = 2 * len(rows) + 2
    F, _, theta, beta = _state(n, m, 0.0, 31)
    F *= 3.0                                                 # (one row decides the column: let it matter)
    Y = np.full((n, m), np.nan, order="F")
    for q, i in enumerate(rows):
        Y[i, 2 * q] = 1.0
        Y[i, 2 * q + 1] = -1.0
    Y[:, m - 1] = np.where(np.arange(n) % 3 == 0, -1.0, 1.0)  # none missing; column m - 2: every row missing
    rc, f, k = _same(handle, n, F, Y, theta, beta, 1.0, 13, 2, "mask layout")
    assert rc == 0 and k[m - 2] == 0
    # the single rows do decide: a column and its twin with the sign flipped do not all agree
    assert any(k[2 * q] != k[2 * q + 1] or not np.array_equal(f[:, 2 * q], f[:, 2 * q + 1]) for q in range(len(rows)))


@pytest.mark.parametrize("n", [2049, 8192])
def test_overflow_and_nan_states(handle, n):
    """the states of tests/test_gpu_draw_f_constructed.py with a linear mu: the current state beyond the overflow of exp (an
    observed row at a = -720), trial points beyond it (sigma = 1000), a NaN in f at an observed and at a missing row"""
    m = 6
    F, Y, theta, beta = _state(n, m, 0.05, 600 + n)
    mu = _mu(theta, beta)
    i_obs, i_mis, i_end = 7, 700, n - 1                      # (the last row: the last lane's last counted bit at n = 8192)
    Y[i_obs, :] = 1.0
    Y[i_end, :] = 1.0
    Y[i_mis, :] = np.nan
    F[i_obs, 0] = -720.0 - mu[i_obs, 0]                      # column 0: the current state overflows
    F[i_end, 1] = -720.0 - mu[i_end, 1]                      # column 1: the same in the last row
    F[i_mis, 2] = np.nan                                     # column 2: NaN where no answer is: the row does not count
    F[i_obs, 3] = np.nan                                     # column 3: NaN at an observed row: the item fails
    F[i_end, 4] = np.nan                                     # column 4: the same in the last row
    ok = [0, 1, 2, 5]
    for ll_exact in (1, 0):
        for screen in (1, 2):
            with handle.config("GPIRT_LL_EXACT", ll_exact), handle.config("GPIRT_ESS_SCREEN", screen):
                what = ("nan states", n, ll_exact, screen)
                rc, f, k = _same(handle, n, F, Y, theta, beta, 1.0, 21, 4, what)
                assert rc != 0, what                         # (columns 3 and 4 never accept)
                assert np.isnan(f[i_mis, 2]) and np.isfinite(np.delete(f[:, 2], i_mis)).all()
                # without the failing columns: no error, and the overflowing rows are there
                rc, f, k = _same(handle, n, np.asfortranarray(F[:, ok]), np.asfortranarray(Y[:, ok]), theta,
                                 np.asfortranarray(beta[:, ok]), 1.0, 21, 4, what + ("ok columns",))
                assert rc == 0, what
                # trial points beyond the overflow: under the written term the screen must hand such a point over
                rc, f, k = _same(handle, n, np.asfortranarray(F[:, ok]), np.asfortranarray(Y[:, ok]), theta,
                                 np.asfortranarray(beta[:, ok]), 1000.0, 22, 4, what + ("sigma 1000",))
                assert rc == 0, what


def test_sampler_takes_the_packed_kernel_only_while_mu_is_linear(handle):
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    n, m = 2304, 6
    y, th0 = make_responses(n, m, seed=143)
    names = ("theta", "beta", "f", "fstar", "mu")

    def run(mode):
        with handle.config("GPIRT_ESS_PACK", mode):
            s = Sampler(handle, y, th0, seed=17, rng="item", fstar_fused=True, kstar_rank=64, theta_stabilise=True)
            s.init()
            for _ in range(10):
                s.step()
            s.check()
            first = {k: s.get(k) for k in names}
            draws = [s.ess_pack_draws]
            # an entry that writes beta clears the flag: the next draw_f reads mu and y
            s.set("beta", s.get("beta"))
            s.draw_f()
            s.check()
            draws.append(s.ess_pack_draws)
            after_set = s.get("f")
            # a step behind it: its draw_f still reads mu (no draw_beta since), its draw_beta sets the flag for the next one
            s.step()
            draws.append(s.ess_pack_draws)
            s.step()
            s.check()
            draws.append(s.ess_pack_draws)
            last = {k: s.get(k) for k in names}
        return first, after_set, last, draws

    a = run(1)
    b = run(2)
    c = run(3)
    assert a[3] == [10, 10, 10, 11] and c[3] == [10, 10, 10, 11] and b[3] == [0, 0, 0, 0], (a[3], b[3], c[3])
    for other in (a, c):
        for k in names:
            assert np.array_equal(_bits(other[0][k]), _bits(b[0][k])), ("ten steps", k)
            assert np.array_equal(_bits(other[2][k]), _bits(b[2][k])), ("after the setter", k)
        assert np.array_equal(_bits(other[1]), _bits(b[1])), "draw_f behind the setter"


def test_refused_orders(handle):
    import torch
    from gpirt_amd.ops import _ld, _p, to_device
    for n in (2048, 8193):
        F, Y, theta, beta = _state(n, 2, 0.05, n)
        L = _eye(n, 1.0)
        f = to_device(F)
        before = f.clone()
        rc = handle.lib.gpirt_draw_f_linear(handle._h, _p(f), _p(to_device(Y)), _p(L), _ld(L), _p(to_device(theta)),
                                            _p(to_device(beta)), n, 2, 1, 1, C.c_void_p(0))
        torch.cuda.synchronize()
        assert rc != 0 and torch.equal(f, before), n
