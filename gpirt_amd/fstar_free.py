"""draw_fstar's C = S^-1 U from theta alone (csrc/fstar_free.hip): the NumPy statement.

S = K(theta, theta) + eps I, U = K(theta, c) with c the 64 Chebyshev nodes of the rank-64 form.  With V the Lagrange basis
of the nodes at theta (n x 64) the kernel matrix is K(theta, theta) = V Kcc V^T and U = V Kcc, Kcc = K(c, c), to rounding
(the rank-64 certificate).  Let Kcc = F F^T (F = Q sqrt(max(Lambda, 0)) from the symmetric eigendecomposition) and Y = V F:
    S = Y Y^T + eps I,     C = S^-1 Y F^T = Y (Y^T Y + eps I)^-1 F^T = V M,
    M = F (F^T (V^T V) F + eps I)^-1 F^T                               (64 x 64, symmetric, positive semi-definite)
With A = F^T (V^T V) F + eps I = R R^T (Cholesky) and X = R^-1 F^T:  M = X^T X -- one Gram product over n, one 64 x 64
factorisation and solve, one n x 64 x 64 product, and nothing of the factor L of S.

G = B^T B (B = L^-1 U), the other thing draw_fstar needs from the factor, is NOT taken from the closed form Kcc - eps M:
that difference is not positive semi-definite in floating point and s = 1 - sqrt(v^T G v) is wrong by 1e-5 where the
quadratic form is near 0.  The library keeps the product over the node rows for G.
"""
from __future__ import annotations

import numpy as np

from .kernel import kernel_matrix

RANK = 64
JITTER = 1.0e-3
_LD = np.longdouble
_PI = _LD("3.141592653589793238462643383279502884")


def nodes(r: int = RANK):
    """(nodes fp64, barycentric weights fp64): 5 cos((2k + 1) pi / 2r) and (-1)^k sin((2k + 1) pi / 2r), as the device holds them"""
    a = (2 * np.arange(r, dtype=_LD) + 1) * _PI / (2 * r)
    c = (_LD(5) * np.cos(a)).astype(np.float64)
    w = (np.where(np.arange(r) % 2 == 1, _LD(-1), _LD(1)) * np.sin(a)).astype(np.float64)
    return c, w


def basis(theta, r: int = RANK) -> np.ndarray:
    """V[i, k] = l_k(theta_i), the barycentric form in fp64 (csrc/nu_lr.hip, nu_basis_kernel): a theta on a node gets that node's
    unit row; theta is clamped to [-5, 5]"""
    c, w = nodes(r)
    t = np.clip(np.asarray(theta, dtype=np.float64), -5.0, 5.0)
    d = t[:, None] - c[None, :]
    hit = d == 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(hit, 0.0, w[None, :] / d)
        V = q / q.sum(axis=1, keepdims=True)
    rows = hit.any(axis=1)
    V[rows] = hit[rows].astype(np.float64)
    return V


def jacobi_eigh(A, sweeps: int = 60):
    """(eigenvalues, eigenvectors) of a symmetric matrix by cyclic Jacobi rotations in long double -- what the library runs on
    the host once per kernel (Kcc's small eigenvalues are far below fp64's rounding of its large ones)"""
    A = np.array(A, dtype=_LD)
    n = A.shape[0]
    Q = np.eye(n, dtype=_LD)
    for _ in range(sweeps):
        off = np.sqrt(((A - np.diag(np.diag(A))) ** 2).sum())
        if off <= np.finfo(_LD).eps * np.sqrt((np.diag(A) ** 2).sum()):
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                if A[p, q] == 0:
                    continue
                th = (A[q, q] - A[p, p]) / (2 * A[p, q])
                t = np.sign(th) / (abs(th) + np.sqrt(th * th + 1)) if th != 0 else _LD(1)
                c = 1 / np.sqrt(t * t + 1)
                s = t * c
                Ap, Aq = A[:, p].copy(), A[:, q].copy()
                A[:, p], A[:, q] = c * Ap - s * Aq, s * Ap + c * Aq
                Ap, Aq = A[p, :].copy(), A[q, :].copy()
                A[p, :], A[q, :] = c * Ap - s * Aq, s * Ap + c * Aq
                Qp, Qq = Q[:, p].copy(), Q[:, q].copy()
                Q[:, p], Q[:, q] = c * Qp - s * Qq, s * Qp + c * Qq
    return np.diag(A).copy(), Q


def kernel_factor(family="se", length_scale=1.0, r: int = RANK) -> np.ndarray:
    """F (r x r, fp64) with K(c, c) = F F^T: Q sqrt(Lambda), negative eigenvalues clipped to 0"""
    c, _ = nodes(r)
    lam, Q = jacobi_eigh(kernel_matrix(c, c, family, length_scale))
    return (Q * np.sqrt(np.maximum(lam, 0))[None, :]).astype(np.float64)


def small_matrix(V, F, eps: float = JITTER) -> np.ndarray:
    """M = F (F^T (V^T V) F + eps I)^-1 F^T through the Cholesky factor of the inner matrix, fp64"""
    H = F.T @ ((V.T @ V) @ F)
    A = H + eps * np.eye(F.shape[0])
    R = np.linalg.cholesky(np.tril(A) + np.tril(A, -1).T)
    X = np.linalg.solve(R, F.T)
    return X.T @ X


def c_from_theta(theta, family="se", length_scale=1.0, eps: float = JITTER, F=None) -> np.ndarray:
    """C = S^-1 K(theta, c) (n x 64) as V M: no factor of S is formed"""
    V = basis(theta)
    if F is None:
        F = kernel_factor(family, length_scale)
    return V @ small_matrix(V, F, eps)
