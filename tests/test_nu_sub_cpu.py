"""draw_f's structured product in parts narrower than the factor's (gpirt_amd/factor_lr.py: sub_parts + nu, csrc/nu_lr.hip's
GPIRT_NU_SUB): the NumPy statement at the widths 64, 128, 256 and 512 against SciPy's dense factor,

    nu[P, :] = L[P, P] Z[P, :] + V[P, :] sum_{Q < P} Bt[:, Q] Z[Q, :]      for parts P of `width` columns,

with L[P, P] the width-wide diagonal blocks inside the structured factor's 512-column parts and Bt its node rows.  The identity
L[R, Q] = V[R, :] Bt[:, Q] holds for every row block strictly below every column block, so the bound does not depend on the
width: tests/test_gpu_nu_lr.py's 1e-10 x max(1, max|nu|) (measured on the CPU: 2e-13 .. 5e-12 at every width)."""
import functools

import numpy as np
import pytest
from scipy.linalg import cholesky

from gpirt_amd import factor_lr as FL
from gpirt_amd import fstar_free as FF
from gpirt_amd.kernel import kernel_matrix
from tests.test_factor_lr_cpu import KINDS, theta_case

BOUND = 1e-10
COLS = 4


@functools.lru_cache(maxsize=None)
def _case(kind, n):
    """(parts, Bt, V, Z, nu_dense) of one theta: the structured factor and SciPy's L Z, computed once for the four widths"""
    theta = theta_case(kind, n)
    L = cholesky(kernel_matrix(theta, theta) + FF.JITTER * np.eye(n), lower=True)
    parts, Bt, V = FL.structured_factor(theta, F=FF.kernel_factor())
    Z = np.random.default_rng(5).standard_normal((n, COLS))
    out = (parts, Bt, V, Z, L @ Z)
    for a in (Bt, V, Z, out[4], *parts):
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("width", FL.SUB_WIDTHS)
@pytest.mark.parametrize("n", [576, 1088])
@pytest.mark.parametrize("kind", KINDS)
def test_every_width_gives_the_dense_product(kind, n, width):
    parts, Bt, V, Z, nu_dense = _case(kind, n)
    sub = FL.sub_parts(parts, width)
    assert sum(b.shape[0] for b in sub) == n and len(sub) == sum(-(-p.shape[0] // width) for p in parts)
    assert all(b.shape[0] == b.shape[1] and np.array_equal(b, np.tril(b)) for b in sub)
    got = FL.nu(sub, Bt, V, Z, part=width)
    gap, scale = float(np.abs(got - nu_dense).max()), max(1.0, float(np.abs(nu_dense).max()))
    print(f"MEASURED {kind} n={n} width={width}: max|nu - L Z| = {gap:.2e}, max|nu| = {float(np.abs(nu_dense).max()):.2f}")
    assert np.isfinite(got).all()
    assert gap <= BOUND * scale


def test_the_factor_width_is_the_parts_themselves_and_other_widths_are_refused():
    parts, _, _, _, _ = _case("off_grid", 576)
    assert all(np.array_equal(a, b) for a, b in zip(FL.sub_parts(parts, FL.PART), parts))
    for bad in (0, 32, 96, 1024):
        with pytest.raises(ValueError):
            FL.sub_parts(parts, bad)
