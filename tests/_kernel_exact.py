"""Long-double references of the covariance kernels (gpirt_amd.kernel, csrc/se_kernel.hip) and of draw_fstar under a kernel,
for tests/test_kernel_cpu.py and tests/test_gpu_kernel.py.  The CPU oracle knows the reference's unit squared exponential
alone, so everything here is stated in np.longdouble (the x87 80-bit format, as in tests/_stage_exact.py).

  kernel_ld          K(x1, x2) for a family and a length scale, from the fp64 inputs
  certificate        max |K(theta, c) V^T - K(theta, theta*)| over the grid, V rounded to fp64: gpirt_kernel_check's figure
  fstar_kernel_exact tests/_stage_exact.py's fstar_rank_exact with the kernel as an argument
  k_tolerance        the derived bound on |device K - kernel_ld| per family (below)

THE BOUND on one entry of K, u = 2^-53.  The default kernel (squared exponential, length scale 1) keeps
tests/test_gpu_ops.py::test_se_kernel's 4e-16.  Every other form adds roundings of the ARGUMENT; a relative error delta of the
argument x of a factor g(x) moves the value by at most delta |x g'(x)|:
  * "se" at a length scale: r = d (1 / ell) -- 1 / ell rounds once on the host, the product once: two relative errors of
    r, four of x = r^2 / 2 in exp(-x), each at most u max_x x e^-x = u / e:  SE_BASE + 4 u / e.
  * "matern52", k = (1 + a + a^2 / 3) e^-a: a = sqrt5 (|d| (1 / ell)) carries five relative roundings (d, 1 / ell, the
    product, the constant sqrt 5, the product); |a k'(a)| = (a^2 / 3)(1 + a) e^-a <= 0.6044 (at a = 1 + sqrt 3): 3.03 u.  The
    polynomial: a a, the constant 1 / 3, its product, 1 + a and the sum, five roundings of intermediates p <= the polynomial,
    and p e^-a <= 1: 5 u.  exp within one ulp of its value (2 u relative at the most), the final product u, the jitter's sum
    on the diagonal u of 1.001:  (3.03 + 5 + 2 + 1 + 1.001) u < 12.1 u.
  * "matern32", k = (1 + a) e^-a: the same five roundings of a, |a k'(a)| = a^2 e^-a <= 4 e^-2 = 0.5414: 2.71 u; 1 + a: u;
    exp 2 u, the product u, the jitter 1.001 u:  < 7.8 u.
kernel_ld itself is good to 2^-63.
"""
from __future__ import annotations

import functools
import math

import numpy as np

from _stage_exact import LD, _backward, _forward, cheb_basis, grid

U = 2.0 ** -53
SE_BASE = 4e-16                       # tests/test_gpu_ops.py::test_se_kernel
FAMILIES = ("se", "matern52", "matern32")
LENGTH_SCALES = (0.35, 1.0, 2.5)


def kernel_ld(family, ell, x1, x2):
    """K(x1, x2) in long double from the fp64 inputs: k(|x1_i - x2_j| / ell)"""
    d = np.asarray(x1, dtype=np.float64).astype(LD).reshape(-1, 1) - np.asarray(x2, dtype=np.float64).astype(LD).reshape(1, -1)
    r = np.abs(d) / LD(float(ell))
    if family == "se":
        return np.exp(LD(-0.5) * r * r)
    if family == "matern52":
        a = np.sqrt(LD(5)) * r
        return (LD(1) + a + a * a / LD(3)) * np.exp(-a)
    if family == "matern32":
        a = np.sqrt(LD(3)) * r
        return (LD(1) + a) * np.exp(-a)
    raise ValueError(family)


def k_tolerance(family, ell):
    if family == "se":
        return SE_BASE if float(ell) == 1.0 else SE_BASE + 4 * U / math.e
    if family == "matern52":
        return 12.1 * U
    if family == "matern32":
        return 7.8 * U
    raise ValueError(family)


@functools.lru_cache(maxsize=None)
def certificate(family, ell, r):
    """max |K(theta, c) V^T - K(theta, theta*)| over theta and theta* on the whole grid, V rounded to fp64 as the device
    holds it: the figure of gpirt_kernel_check"""
    c, V = cheb_basis(r)
    V64 = V.astype(np.float64).astype(LD)
    g = grid()
    return float(np.abs(kernel_ld(family, ell, g, c) @ V64.T - kernel_ld(family, ell, g, g)).max())


def certificate_line():
    """the certificate of ("se", 1, r = 48): a rank passes when its certificate is no larger"""
    return certificate("se", 1.0, 48)


def min_rank(family, ell):
    """the first multiple of 16 in 16..128 whose certificate passes (0: none)"""
    for r in range(16, 129, 16):
        if certificate(family, ell, r) <= certificate_line():
            return r
    return 0


def fstar_kernel_exact(family, ell, theta, L, f, mu_star, r, z):
    """fstar_rank_exact (tests/_stage_exact.py) under a kernel: draw_fstar (src/draw-fstar.cpp:10-31) in long double through the
    rank-r form (r = 0: the full form), the device's own factor L as an input, V rounded to fp64 first.  Returns s, mean
    (without mu*), fstar, q and cond = cond_2(S)."""
    Ld = np.asarray(L, dtype=np.float64).astype(LD)
    fL = np.asarray(f, dtype=np.float64).astype(LD)
    if r > 0:
        c, V = cheb_basis(r)
        V = V.astype(np.float64).astype(LD)
        B = _forward(Ld, kernel_ld(family, ell, theta, c))
        W = B @ V.T
        Cm = _backward(Ld, B)
        mean = V @ (Cm.T @ fL)
    else:
        W = _forward(Ld, kernel_ld(family, ell, theta, grid()))
        mean = W.T @ _forward(Ld, fL)
    q = (W * W).sum(axis=0)
    s = LD(1) - np.sqrt(np.maximum(q, LD(0)))
    zL, muL = np.asarray(z, dtype=np.float64).astype(LD), np.asarray(mu_star, dtype=np.float64).astype(LD)
    m0 = mean + muL
    fstar = np.where(s[:, None] > 0, m0 + s[:, None] * zL, np.where(s[:, None] == 0, m0, LD("nan")))
    return dict(s=s, mean=mean, fstar=fstar, q=q, cond=float(np.linalg.cond(np.asarray(L, dtype=np.float64), 2) ** 2))
