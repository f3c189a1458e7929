"""draw_fstar's C = S^-1 K(theta, c) from theta alone, C = V M (gpirt_amd/fstar_free.py, csrc/fstar_free.hip): the NumPy
statement against the dense solve (scipy's cho_solve in fp64), through what draw_fstar makes of C: mean = V* (C^T f).

Generic theta (normal on the grid, off the grid): 1e-9 x max(1, max|mean|), the project's bound on f*.  Constructed theta
(one point, two points 0.01 apart, +-5; tests/test_gpu_fstar_ranks.py::test_constructed_theta): the forward error of
S x = f, 8 n u cond(S) -- replacing K by its interpolant INSIDE an inverse turns a 1e-15 entrywise difference into
lambda_max / eps of it, which the generic bound does not cover and this one does.
The closed form Kcc - eps M for G = B^T B is not asserted anywhere: the library does not use it."""
import functools

import numpy as np
import pytest
from scipy.linalg import cho_factor, cho_solve

from gpirt_amd import fstar_free as FF
from gpirt_amd.kernel import kernel_matrix

U = 2.0 ** -53
M_ITEMS = 8
NGRID = 1001


def _grid():
    return -5.0 + np.arange(NGRID, dtype=np.float64) * 0.01


@functools.lru_cache(maxsize=None)
def _factor():
    return FF.kernel_factor()


def _theta(kind, n):
    rng = np.random.default_rng(1000 + n)
    g = _grid()
    if kind == "grid_normal":
        return g[np.clip(np.rint((rng.standard_normal(n) + 5.0) / 0.01).astype(int), 0, NGRID - 1)]
    if kind == "off_grid":
        return rng.uniform(-5.0, 5.0, n)
    if kind == "one_point":
        return np.full(n, g[617])
    if kind == "two_points_0.01_apart":
        return np.where(np.arange(n) % 2 == 0, g[400], g[401])
    if kind == "plus_minus_5":
        return np.where(np.arange(n) < n // 2, -5.0, 5.0)
    raise ValueError(kind)


def _means(theta):
    """(mean through C = V M, mean through the dense solve, cond(S)); f = a smooth curve of theta plus noise, per item"""
    n = theta.shape[0]
    rng = np.random.default_rng(7)
    f = np.sin(theta[:, None] * rng.uniform(0.3, 1.5, M_ITEMS)[None, :]) + 0.3 * rng.standard_normal((n, M_ITEMS))
    c, _ = FF.nodes()
    S = kernel_matrix(theta, theta) + FF.JITTER * np.eye(n)
    Vstar = FF.basis(_grid())
    C_dense = cho_solve(cho_factor(S, lower=True), kernel_matrix(theta, c))
    C_free = FF.c_from_theta(theta, F=_factor())
    return Vstar @ (C_free.T @ f), Vstar @ (C_dense.T @ f), float(np.linalg.cond(S, 2))


def test_factor_reproduces_the_node_kernel():
    c, _ = FF.nodes()
    F = _factor()
    assert F.shape == (64, 64) and np.isfinite(F).all()
    assert np.abs(F @ F.T - kernel_matrix(c, c)).max() <= 64 * U


def test_small_matrix_is_symmetric():
    V = FF.basis(_theta("grid_normal", 320))
    Mm = FF.small_matrix(V, _factor())
    assert np.array_equal(Mm, Mm.T)


@pytest.mark.parametrize("n", [320, 1088])
@pytest.mark.parametrize("kind", ["grid_normal", "off_grid"])
def test_generic_theta(kind, n):
    got, ref, cond = _means(_theta(kind, n))
    gap = float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max()))
    print(f"MEASURED {kind} n={n}: |mean(V M) - mean(dense)| {gap:.2e} relative to max(1, max|mean|); cond(S) {cond:.2e}")
    assert gap <= 1e-9


@pytest.mark.parametrize("kind", ["one_point", "two_points_0.01_apart", "plus_minus_5"])
def test_constructed_theta(kind):
    n = 320
    got, ref, cond = _means(_theta(kind, n))
    gap = float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max()))
    tol = 8 * n * U * cond
    print(f"MEASURED {kind} n={n}: |mean(V M) - mean(dense)| {gap:.2e} (tolerance {tol:.2e}); cond(S) {cond:.2e}")
    assert np.isfinite(got).all() and gap <= tol
