"""The structured factor from theta alone (gpirt_amd/factor_lr.py, csrc/factor_lr.hip): the NumPy statement against SciPy's
dense Cholesky of S = K(theta, theta) + 0.001 I -- the 512-column diagonal parts, the 64 node rows K(c, theta) L^-T, nu = L Z
for four columns through the structured product, and draw_fstar's s on the 1001 grid points.

Bounds: 1e-10 on the parts, the project's 1e-9 on the node rows and s, tests/test_gpu_nu_lr.py's 1e-10 x max(1, max|nu|) on
nu.  Every pivot of every part is >= 0.03 (sqrt(0.001) = 0.0316 by construction: S_PP = eps (I + X^T X))."""
import functools

import numpy as np
import pytest
from scipy.linalg import cholesky, solve_triangular

from gpirt_amd import factor_lr as FL
from gpirt_amd import fstar_free as FF
from gpirt_amd.kernel import kernel_matrix

NGRID = 1001
KINDS = ["grid_normal", "grid_uniform", "off_grid", "sorted", "all_equal", "half_minus5_half_plus5", "two_points_0.01_apart"]


def _grid():
    return -5.0 + np.arange(NGRID, dtype=np.float64) * 0.01


def theta_case(kind, n):
    rng = np.random.default_rng(2000 + n)
    g = _grid()
    if kind == "grid_normal":
        return g[np.clip(np.rint((rng.standard_normal(n) + 5.0) / 0.01).astype(int), 0, NGRID - 1)]
    if kind == "grid_uniform":
        return g[rng.integers(0, NGRID, n)]
    if kind == "off_grid":
        return rng.uniform(-5.0, 5.0, n)
    if kind == "sorted":
        return np.sort(g[np.clip(np.rint((rng.standard_normal(n) + 5.0) / 0.01).astype(int), 0, NGRID - 1)])
    if kind == "all_equal":
        return np.full(n, g[617])
    if kind == "half_minus5_half_plus5":
        return np.where(np.arange(n) < n // 2, -5.0, 5.0)
    if kind == "two_points_0.01_apart":
        return np.where(np.arange(n) % 2 == 0, g[400], g[401])
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def _factor():
    return FF.kernel_factor()


@functools.lru_cache(maxsize=None)
def _vstar():
    return FF.basis(_grid())


@pytest.mark.parametrize("n", [576, 1088])
@pytest.mark.parametrize("kind", KINDS)
def test_structured_factor_against_dense(kind, n):
    theta = theta_case(kind, n)
    c, _ = FF.nodes()
    L = cholesky(kernel_matrix(theta, theta) + FF.JITTER * np.eye(n), lower=True)
    Bt_dense = solve_triangular(L, kernel_matrix(theta, c), lower=True).T
    parts, Bt, V = FL.structured_factor(theta, F=_factor())
    assert len(parts) == (n + FL.PART - 1) // FL.PART and Bt.shape == (64, n)
    gap_parts, pivot = 0.0, np.inf
    for q, Lpp in enumerate(parts):
        p = q * FL.PART
        w = Lpp.shape[0]
        assert np.array_equal(Lpp, np.tril(Lpp))
        gap_parts = max(gap_parts, float(np.abs(Lpp - L[p:p + w, p:p + w]).max()))
        pivot = min(pivot, float(np.diag(Lpp).min()))
    gap_rows = float(np.abs(Bt - Bt_dense).max())
    Z = np.random.default_rng(5).standard_normal((n, 4))
    nu_dense = L @ Z
    gap_nu = float(np.abs(FL.nu(parts, Bt, V, Z) - nu_dense).max())
    nu_max = float(np.abs(nu_dense).max())
    gap_s = float(np.abs(FL.s_grid(Bt, _vstar()) - FL.s_grid(Bt_dense, _vstar())).max())
    print(f"MEASURED {kind} n={n}: parts {gap_parts:.2e}, node rows {gap_rows:.2e}, nu {gap_nu:.2e} (max|nu| {nu_max:.2f}), "
          f"s {gap_s:.2e}, smallest pivot {pivot:.4f}")
    assert pivot >= 0.03
    assert gap_parts <= 1e-10
    assert gap_rows <= 1e-9
    assert gap_nu <= 1e-10 * max(1.0, nu_max)
    assert gap_s <= 1e-9
