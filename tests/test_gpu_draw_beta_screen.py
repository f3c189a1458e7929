"""draw_beta from registers with the single-precision screen (csrc/stages.hip draw_beta_reg_kernel, GPIRT_BETA_SCREEN=1) against
draw_beta_kernel (GPIRT_BETA_SCREEN=2): every decision is the full-precision one, so beta, mu and mu_star are equal bit for bit.

On the constructed columns of tests/_stage_exact.py the PATH of every decision is known in advance from the long-double
reference alone: full precision (1) at the tied step of every tie_* column (|r - log u| = 1e-6 or 1e-9 lies inside every
band) and wherever the proposal's or the current state's sum overflows, the screen (0) everywhere else -- the screen gives a
verdict from a distance of 4 LL_SCREEN_ERR n on (its own sums are within one band each of the full ones and it asks for two
bands), and every untied, finite decision of these columns is at least twice that far from log u.

The random states say how often full precision is needed (printed, not asserted) and cross every size class of the
dispatch; a sampler's draw_beta() is compared at 257 x 21 on the constructed columns and at 2048 x 8 behind one step."""
import numpy as np
import pytest

import _stage_exact as X

pytestmark = pytest.mark.gpu

SWITCH = "GPIRT_BETA_SCREEN"


def _draw(handle, switch, beta, theta, y, f, pm, ps, step, seed, it):
    from gpirt_amd.ops import to_device, to_host
    bd = to_device(np.asfortranarray(beta))
    with handle.config(SWITCH, switch):
        _, path = handle.draw_beta(bd, to_device(theta), to_device(np.asfortranarray(y)), to_device(np.asfortranarray(f)),
                                   to_device(np.asfortranarray(pm)), to_device(np.asfortranarray(ps)),
                                   to_device(np.asfortranarray(step)), seed, it, paths=True)
    return to_host(bd), path.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("n", X.BETA_ORDERS)
def test_constructed_columns_bits_and_paths(handle, n):
    c = X.draw_beta_cases(n)
    args = (c["beta"], c["theta"], c["y"], c["f"], c["pm"], c["ps"], c["step"], c["seed"], c["it"])
    new, path = _draw(handle, 1, *args)
    old, path_old = _draw(handle, 2, *args)
    assert _same_bits(new, old), (n, np.argwhere(new != old))
    assert (path_old == -1).all()                              # draw_beta_kernel records nothing
    ref = X.draw_beta_reference(n)
    verdict_from = 4 * X.LL_SCREEN_ERR * n                     # |r - log u| from which the screen is sure to decide
    tied = {nm: k for nm, k, _ in X.BETA_TIES}
    smallest, skipped = np.inf, []
    for j, (nm, r) in enumerate(zip(c["names"], ref)):
        for k in range(2):
            over = any(r["overflow"][k])
            if over or tied.get(nm) == k:
                assert path[k, j] == 1, (n, nm, k, "full precision expected", path[k, j])
                continue
            if r["margin"][k] < verdict_from:
                skipped.append((nm, k, r["margin"][k]))
                continue
            smallest = min(smallest, r["margin"][k])
            assert path[k, j] == 0, (n, nm, k, "the screen's verdict expected", path[k, j], r["margin"][k])
    print(f"MEASURED n={n}: smallest margin of a screened decision {smallest:.4g} against {verdict_from:.4g}; "
          f"full-precision decisions {int((path == 1).sum())} of {path.size}")
    assert not skipped, skipped
    assert smallest >= 2.0 * verdict_from


def _random_state(n, m, step, seed):
    rng = np.random.default_rng(seed)
    theta = np.clip(rng.normal(size=n), -4.9, 4.9)
    beta = np.asfortranarray(np.stack([rng.normal(size=m) * 0.5, rng.uniform(0.6, 1.4, size=m)]))
    f = np.asfortranarray(rng.normal(size=(n, m)) * 0.5)
    pr = 1.0 / (1.0 + np.exp(-(f + beta[0][None, :] + theta[:, None] * beta[1][None, :])))
    y = np.where(rng.random((n, m)) < pr, 1.0, -1.0)
    y[rng.random((n, m)) < 0.06] = np.nan
    pm, ps = np.zeros((2, m), order="F"), np.full((2, m), 3.0, order="F")
    return beta, theta, np.asfortranarray(y), f, pm, ps, np.full((2, m), step, order="F")


@pytest.mark.parametrize("n", (255, 2048, 8191, 8192, 8193))
def test_random_states_bits(handle, n):
    m = 16
    for q, step in enumerate((0.02, 0.1, 0.5)):
        st = _random_state(n, m, step, 9000 + 10 * n + q)
        new, path = _draw(handle, 1, *st, 31 + q, 2 + q)
        old, _ = _draw(handle, 2, *st, 31 + q, 2 + q)
        moved = int((new != st[0]).sum())
        assert _same_bits(new, old), (n, step, np.argwhere(new != old))
        if n > 8192:
            assert (path == -1).all(), (n, path)               # beyond 32 rows per thread: draw_beta_kernel
            print(f"MEASURED n={n} step={step}: draw_beta_kernel; accepted {moved} of {2 * m}")
        else:
            assert ((path == 0) | (path == 1)).all(), (n, path)
            print(f"MEASURED n={n} step={step}: full-precision share {float((path == 1).mean()):.3f}; accepted {moved} of {2 * m}")


def test_y_outside_the_contract_takes_the_old_kernel(handle):
    """the stand-alone entry checks y itself: a 2.0 among the answers is multiplied by draw_beta_kernel, as before"""
    st = list(_random_state(300, 4, 0.1, 5))
    st[2][7, 1] = 2.0
    new, path = _draw(handle, 1, *st, 3, 1)
    old, _ = _draw(handle, 2, *st, 3, 1)
    assert _same_bits(new, old) and (path == -1).all()


def test_nan_in_f_at_an_observed_row_rejects_twice(handle):
    st = list(_random_state(1000, 3, 0.1, 6))
    st[2][500, 1] = 1.0
    st[3][500, 1] = np.nan
    for sw in (1, 2):
        out, path = _draw(handle, sw, *st, 4, 1)
        assert _same_bits(out[:, 1], st[0][:, 1]), (sw, out[:, 1], st[0][:, 1])
        if sw == 1:
            assert (path[:, 1] == 1).all(), path                # a NaN fails both comparisons of the screen


def _sampler_outputs(handle, switch, n, m):
    """beta, mu, mu_star behind Sampler.draw_beta() under `switch`; the state in front of it is made under switch 2 both times:
    at 257 x 21 the constructed columns, at 2048 x 8 whatever one step of the chain leaves"""
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    with handle.config(SWITCH, 2):
        if n == 257:
            c = X.draw_beta_cases(257)
            assert len(c["names"]) == m
            s = Sampler(handle, c["y"], c["theta"], c["pm"], c["ps"], c["step"], rng="item", seed=c["seed"])
            s.init()
            s.set("theta", c["theta"]); s.set("f", c["f"]); s.set("beta", c["beta"])
            s.set_iteration(c["it"] - 1)
        else:
            y, th0 = make_responses(n, m, seed=300 + n)
            s = Sampler(handle, y, th0, rng="item", seed=17)
            s.init()
            s.step()
            s.get("beta")                                       # (nothing of the step is still pending)
    with handle.config(SWITCH, switch):
        s.draw_beta()
        out = tuple(s.get(k) for k in ("beta", "mu", "mu_star"))
    s.close()
    return out


@pytest.mark.parametrize("n,m", ((257, 21), (2048, 8)))
def test_sampler_draw_beta_bits(handle, n, m):
    new, old = _sampler_outputs(handle, 1, n, m), _sampler_outputs(handle, 2, n, m)
    for name, a, b in zip(("beta", "mu", "mu_star"), new, old):
        assert _same_bits(a, b), (n, m, name, int((a != b).sum()))
