"""The structured factor in parts narrower than 512 (gpirt_amd/factor_lr.py with part = 64, 128, 256; csrc/factor_lr.hip,
DESIGN.md section 48): both NumPy statements against SciPy's dense Cholesky of S = K(theta, theta) + 0.001 I.  n = 576 and
1088 leave a ragged last part at 128 and at 256.

Bounds, those of tests/test_factor_lr_cpu.py: 1e-10 on the parts, 1e-9 on the node rows against K(c, theta) L^-T,
1e-10 x max(1, max|nu|) on nu through the structured product at the same width, every pivot >= 0.03; the two statements agree
with each other within the same bounds."""
import functools

import numpy as np
import pytest
from scipy.linalg import cholesky, solve_triangular

from gpirt_amd import factor_lr as FL
from gpirt_amd import fstar_free as FF
from gpirt_amd.kernel import kernel_matrix

NGRID = 1001
KINDS = ["grid_normal", "grid_uniform", "off_grid", "sorted", "all_equal", "half_minus5_half_plus5", "two_points_0.01_apart"]
SIZES = [576, 1088]
WIDTHS = [64, 128, 256]


def theta_case(kind, n):
    rng = np.random.default_rng(2000 + n)
    g = -5.0 + np.arange(NGRID, dtype=np.float64) * 0.01
    normal = lambda: g[np.clip(np.rint((rng.standard_normal(n) + 5.0) / 0.01).astype(int), 0, NGRID - 1)]
    return {"grid_normal": normal, "grid_uniform": lambda: g[rng.integers(0, NGRID, n)], "off_grid": lambda: rng.uniform(-5.0, 5.0, n),
            "sorted": lambda: np.sort(normal()), "all_equal": lambda: np.full(n, g[617]),
            "half_minus5_half_plus5": lambda: np.where(np.arange(n) < n // 2, -5.0, 5.0),
            "two_points_0.01_apart": lambda: np.where(np.arange(n) % 2 == 0, g[400], g[401])}[kind]()


@functools.lru_cache(maxsize=None)
def _factor():
    return FF.kernel_factor()


@functools.lru_cache(maxsize=None)
def _dense(kind, n):
    """(theta, L, K(c, theta) L^-T, Z, L Z): computed once per case and shared by the widths; nobody writes to them"""
    theta = theta_case(kind, n)
    c, _ = FF.nodes()
    L = cholesky(kernel_matrix(theta, theta) + FF.JITTER * np.eye(n), lower=True)
    Bt = solve_triangular(L, kernel_matrix(theta, c), lower=True).T
    Z = np.random.default_rng(5).standard_normal((n, 4))
    out = (theta, L, Bt, Z, L @ Z)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_narrow_parts_against_dense(kind, n, w):
    theta, L, Bt_dense, Z, nu_dense = _dense(kind, n)
    nu_max = float(np.abs(nu_dense).max())
    results = {}
    for name, fn in (("plain", FL.structured_factor), ("fused", FL.structured_factor_fused)):
        parts, Bt, V = fn(theta, part=w, F=_factor())
        assert [p.shape[0] for p in parts] == [min(w, n - p) for p in range(0, n, w)] and Bt.shape == (64, n)
        gap_parts, pivot = 0.0, np.inf
        for q, Lpp in enumerate(parts):
            p = q * w
            assert np.array_equal(Lpp, np.tril(Lpp))
            gap_parts = max(gap_parts, float(np.abs(Lpp - L[p:p + w, p:p + w]).max()))
            pivot = min(pivot, float(np.diag(Lpp).min()))
        gap_rows = float(np.abs(Bt - Bt_dense).max())
        gap_nu = float(np.abs(FL.nu(parts, Bt, V, Z, part=w) - nu_dense).max())
        print(f"MEASURED {name} {kind} n={n} w={w}: parts {gap_parts:.2e}, node rows {gap_rows:.2e}, nu {gap_nu:.2e} "
              f"(max|nu| {nu_max:.2f}), smallest pivot {pivot:.4f}")
        assert pivot >= 0.03
        assert gap_parts <= 1e-10
        assert gap_rows <= 1e-9
        assert gap_nu <= 1e-10 * max(1.0, nu_max)
        results[name] = (parts, Bt)
    (pa, Ba), (pb, Bb) = results["plain"], results["fused"]
    assert max(float(np.abs(a - b).max()) for a, b in zip(pa, pb)) <= 1e-10
    assert float(np.abs(Ba - Bb).max()) <= 1e-9


def test_the_widths_agree_on_the_blocks_they_share():
    """a w-wide part's leading 64 x 64 block is the dense factor's there at every width: the widths differ in rounding only"""
    n, kind = 1088, "off_grid"
    theta = _dense(kind, n)[0]
    ref = FL.structured_factor(theta, F=_factor())[0]
    for w in WIDTHS:
        parts = FL.structured_factor(theta, part=w, F=_factor())[0]
        wide = FL.sub_parts(ref, w)
        assert len(parts) == len(wide)
        assert max(float(np.abs(a - b).max()) for a, b in zip(parts, wide)) <= 1e-10
