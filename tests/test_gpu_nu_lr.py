"""draw_f's structured product (gpirt_amd/csrc/nu_lr.hip, item-keyed RNG): nu = L z from L's 512-column diagonal parts and
the 64 node rows K(c_64, theta) L^-T that every bordered factorisation carries below the factor,

    nu[P, :] = L[P, P] Z[P, :] + V[P, :] sum_{Q < P} Bt[:, Q] Z[Q, :].

GPIRT_NU_LR: 1 = the default rule (n >= 2048 and eligible), 2 = always the dense product, 3 = at every eligible n.  The bound
on |nu_structured - nu_dense| is 1e-10 * max(1, max|nu|): ten times the figures NumPy gives for the identity on the CPU
(1.5e-12 .. 9e-12) and ten times inside the 1e-9 every oracle comparison of f uses."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAST = dict(rng="item", fstar_fused=True, kstar_rank=64, theta_stabilise=True)
BOUND = 1e-10


def _off_grid(n, seed):
    """theta_init inside [-5, 5], on no grid point and on no node"""
    r = np.random.default_rng(seed)
    return np.clip(1.7 * r.standard_normal(n), -4.99, 4.99) + 1e-3 * r.random(n) * 0.37


def _both(handle, s):
    """draw_f under GPIRT_NU_LR=3 and =2 on the state `s` is in: (nu, f, ess_k) of each; s is left after the dense draw"""
    f0 = s.get("f")
    out = []
    for mode in (3, 2):
        s.set("f", f0)
        before = s.nu_lr_draws
        with handle.config("GPIRT_NU_LR", mode):
            s.draw_f()
            s.check()
        assert s.nu_lr_draws - before == (1 if mode == 3 else 0), (mode, s.nu_lr_draws, before)
        out.append((s.get("nu"), s.get("f"), s.get("ess_k")))
    return out


def _assert_close(lr, dense, what):
    (nu3, f3, k3), (nu2, f2, k2) = lr, dense
    scale = max(1.0, float(np.abs(nu2).max()))
    dnu, df = float(np.abs(nu3 - nu2).max()), float(np.abs(f3 - f2).max())
    msg = "%s: max|nu_lr - nu_dense| = %.3e, max|f_lr - f_dense| = %.3e, max|nu| = %.3f" % (what, dnu, df, float(np.abs(nu2).max()))
    print(msg)
    assert np.isfinite(nu3).all() and np.isfinite(f3).all(), msg
    assert dnu <= BOUND * scale, msg
    assert df <= BOUND * scale, msg
    assert np.array_equal(k3, k2), msg


@pytest.mark.parametrize("n,m", [(1088, 3), (1536, 70)])
@pytest.mark.parametrize("start", ["grid", "off_grid"])
def test_structured_product_against_the_dense_one_on_the_same_state(handle, n, m, start):
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=311 + n)
    if start == "off_grid":
        th0 = _off_grid(n, n)
    s = Sampler(handle, y, th0, seed=17, **FAST)
    s.init()
    if start == "grid":
        with handle.config("GPIRT_NU_LR", 3):
            for _ in range(2):
                s.step()
        s.check()
        kk = (s.get("theta") + 5.0) / 0.01
        assert np.abs(kk - np.rint(kk)).max() < 1e-9
    lr, dense = _both(handle, s)
    s.close()
    _assert_close(lr, dense, "n = %d, m = %d, theta %s" % (n, m, start))


def test_f_and_the_node_rows_do_not_depend_on_the_draw_fstar_form(handle):
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    n, m = 1088, 5
    y, th0 = make_responses(n, m, seed=77)
    kw = dict(rng="item", seed=23, theta_stabilise=True)
    forms = dict(double_solve=dict(fstar_fused=False, kstar_rank=0), fused=dict(fstar_fused=True, kstar_rank=0),
                 lowrank=dict(fstar_fused=True, kstar_rank=64), rank48=dict(fstar_fused=True, kstar_rank=48))
    S = {k: Sampler(handle, y, th0, **v, **kw) for k, v in forms.items()}
    with handle.config("GPIRT_NU_LR", 3):
        for c in S.values():
            c.init()
            for _ in range(2):
                c.step()
            c.check()
            assert c.nu_lr_draws == 2
    ref = S["double_solve"]
    th, f, beta, rows = ref.get("theta"), ref.get("f"), ref.get("beta"), ref.nu_lr_rows()
    assert np.isfinite(rows).all() and np.abs(rows).max() > 0.0
    for k, c in S.items():
        assert np.array_equal(c.get("theta"), th), k
        assert np.array_equal(c.get("f"), f), k
        assert np.array_equal(c.get("beta"), beta), k
        assert np.array_equal(c.nu_lr_rows(), rows), k            # layouts: behind the grid rows, alone (r = 64), in front of r = 48
    for c in S.values():
        c.close()


def test_an_item_shard_draws_the_same_f_as_the_full_problem(handle):
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    n, m = 1088, 128
    y, th0 = make_responses(n, m, seed=5)
    a = Sampler(handle, y, th0, seed=5, **FAST)
    c = Sampler(handle, y[:, 64:m], th0, seed=5, item0=64, m_total=m, **FAST)
    with handle.config("GPIRT_NU_LR", 3):
        a.init()
        c.init()
        for k in ("f", "mu", "beta"):                      # the same chain state for the shard's columns, then the same theta path
            c.set(k, a.get(k)[:, 64:])
        for _ in range(2):
            a.draw_f(); c.draw_f()
            assert np.array_equal(c.get("f"), a.get("f")[:, 64:])
            assert np.array_equal(c.get("ess_k"), a.get("ess_k")[64:])
            a.draw_fstar(); a.theta_partial(); a.theta_finish(); a.draw_beta(); a.factor()
            c.set("theta", a.get("theta"))
            c.set("mu", a.get("mu")[:, 64:])
            c.factor()                                     # (the shard's factor of the full problem's theta)
            a.check(); c.check()
    assert a.nu_lr_draws == 2 and c.nu_lr_draws == 2
    a.close(); c.close()


def _draws_after(handle, n, m, steps=2, theta=None, **extra):
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=9)
    if theta is not None:
        th0 = theta(th0)
    kw = dict(FAST)
    kw.update(extra)
    s = Sampler(handle, y, th0, seed=3, **kw)
    s.init()
    counts = []
    for _ in range(steps):
        s.step()
        counts.append(s.nu_lr_draws)
    s.check()
    s.close()
    return counts


def test_fall_backs_take_the_dense_product_and_say_so(handle):
    from gpirt_amd.ops import Handle
    assert handle.config_get("GPIRT_NU_LR") == 1
    hm = Handle(kernel="matern52")
    try:
        assert _draws_after(hm, 2048, 2, kstar_rank=0) == [0, 0]              # no rank form: the certificate refuses it
    finally:
        hm.close()
    assert _draws_after(handle, 2048, 2, kernel_fp32=True) == [0, 0]          # K built in fp32: the identity holds to 6e-8 only

    def one_outside(th):
        th = th.copy()
        th[5] = 5.3
        return th
    assert _draws_after(handle, 2048, 2, steps=3, theta=one_outside) == [0, 1, 2]   # draw_theta's values are grid values
    assert _draws_after(handle, 1000, 2) == [0, 0]                            # n % 64 != 0: no bordered layout
    assert _draws_after(handle, 1088, 2) == [0, 0]                            # below the default rule's 2048
    assert _draws_after(handle, 2048, 2) == [1, 2]


def test_after_a_restore_the_rows_are_rebuilt_and_the_product_is_structured(handle):
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    n, m = 1088, 3
    y, th0 = make_responses(n, m, seed=41)
    a = Sampler(handle, y, th0, seed=29, **FAST)
    a.init()
    for _ in range(2):
        a.step()
    a.check()
    state = {k: a.get(k) for k in ("theta", "f", "beta", "mu", "mu_star", "L")}
    it = a.iteration
    a.close()
    b = Sampler(handle, y, th0, seed=29, **FAST)
    b.init()
    for k in ("f", "beta", "mu", "mu_star", "theta", "L"):        # theta, then the factor that belongs to it: the rows are stale
        b.set(k, state[k])
    b.set_iteration(it)
    lr, dense = _both(handle, b)
    b.close()
    _assert_close(lr, dense, "n = %d, m = %d after set(theta) + set(L)" % (n, m))


def test_metric_size_respondents_with_few_items_against_the_oracle(handle, oracle):
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    from tests import _oracle_parallel as P
    n, m, seed = 8192, 8, 11
    y, th0 = make_responses(n, m, seed=20240)
    s = Sampler(handle, y, th0, seed=seed, **FAST)
    s.init()
    for _ in range(2):
        s.step()
    s.check()
    assert s.nu_lr_draws == 2
    it = s.iteration + 1
    f0, mu0, L0 = s.get("f"), s.get("mu"), s.get("L")
    s.draw_f()
    s.check()
    assert s.nu_lr_draws == 3
    f1, k_dev = s.get("f"), s.get("ess_k")
    s.close()
    f_ref, k_ref = P.draw_f(seed, it, f0, y, L0, mu0, P.host_cores())
    df, scale = float(np.abs(f1 - f_ref).max()), max(1.0, float(np.abs(f_ref).max()))
    msg = "n = 8192, m = 8: max|f - f_oracle| = %.3e, max|f| = %.3f, count mismatches %d" % (df, scale, int(np.count_nonzero(k_dev != k_ref)))
    print(msg)
    assert np.array_equal(k_dev, k_ref), msg
    assert df <= 1e-9 * scale, msg
