"""The fast preset's structured factor (csrc/factor_lr.hip): the NumPy statement.

What a steady iteration of the fast preset reads of the factor L of S = K(theta, theta) + eps I is only its 512-column
diagonal parts L[P, P] (draw_f's structured nu = L z, gpirt_amd/csrc/nu_lr.hip) and the 64 node rows Bt = K(c, theta) L^-T
below it (nu_lr's records and draw_fstar's G = B^T B).  Both follow from theta alone by the rank-64 form
K(theta, theta) = V Kcc V^T, Kcc = F F^T (fstar_free.py): for the part P = [p, p + w) with G_P = V[<p]^T V[<p] the Gram of
the basis rows in front of it (G_0 = 0)

    H_P  = F^T G_P F,   A_P = H_P + eps I = R_P R_P^T,   Xh_P = R_P^-1 F^T        (64 x 64)
    X_P  = Xh_P V[P]^T                                                             (64 x w)
    S_PP = eps (I + X_P^T X_P)       the Schur complement of S in front of P, formed without a subtraction
    L_PP = chol(S_PP)                every pivot >= sqrt(eps)
    Bt[:, P] = eps Xh_P^T (X_P L_PP^-T)

(Woodbury on the leading block: Kcc - sum_{Q < P} Bt_Q Bt_Q^T = eps F (H_P + eps I)^-1 F^T.)  The parts depend on each other
through the running Gram alone.  The triangle of L below the parts is never formed.

All of it holds for any cut into multiples of 64: `part` is 512 or, since library version 140, the width draw_f's product
reads the parts at (GPIRT_FLR_NARROW; tests/test_factor_lr_narrow_cpu.py).  Below 512 the device adds
the running Gram in two levels (whole 512-column stretches, then the parts inside the last one) where this statement adds part
by part: the same sum to rounding.
"""
from __future__ import annotations

import numpy as np
from scipy.linalg import solve_triangular

from .fstar_free import JITTER, RANK, basis, kernel_factor

PART = 512


def structured_factor(theta, family="se", length_scale=1.0, eps: float = JITTER, part: int = PART, F=None):
    """(parts, Bt, V): the lower-triangular diagonal parts L[P, P] in part order, the node rows (64 x n) and the basis at theta"""
    V = basis(theta)
    n = V.shape[0]
    if F is None:
        F = kernel_factor(family, length_scale)
    I = np.eye(RANK)
    G = np.zeros((RANK, RANK))
    parts, Bt = [], np.empty((RANK, n))
    for p in range(0, n, part):
        Vp = V[p:p + part]
        A = F.T @ (G @ F) + eps * I
        R = np.linalg.cholesky(np.tril(A) + np.tril(A, -1).T)
        Xh = solve_triangular(R, F.T, lower=True)
        X = Xh @ Vp.T
        Lpp = np.linalg.cholesky(eps * (np.eye(Vp.shape[0]) + X.T @ X))
        Y = solve_triangular(Lpp, X.T, lower=True).T                 # X L_PP^-T
        parts.append(Lpp)
        Bt[:, p:p + part] = eps * (Xh.T @ Y)
        G = G + Vp.T @ Vp
    return parts, Bt, V


def structured_factor_fused(theta, family="se", length_scale=1.0, eps: float = JITTER, part: int = PART, F=None, block: int = 64):
    """The same three results by the schedule of csrc/factor_lr.hip's flr_round_kernel: a part is
    factored in rounds of `block` columns, one "launch" a round, its 64 border rows X_P riding along.

    Launch k reads only what the launches before it wrote (`old` below) and every tile is written by one item:
      * lazy update: each tile (i, j), k <= j <= i, and each border block j >= k first takes panel k - 1 off itself,
        C(i, j) -= L(i, k - 1) L(j, k - 1)^T and X(:, j) -= X(:, k - 1) L(j, k - 1)^T; in launch 0 the tile is formed as
        eps X_i^T X_j from X_b = Xh V[P_b]^T instead, and the border blocks are written;
      * ownerless pivot tile: tile (k, k) is written by nobody in launch k -- every item of block column k reads it, applies
        the same update, adds eps on the diagonal, factors it and solves its own rows against the factor;
      * late placement: the pivot's factor waits in a workspace and goes into tile (k, k) in launch k + 1, when nobody reads
        the tile any more (the last pivot's behind the last launch)."""
    V = basis(theta)
    n = V.shape[0]
    if F is None:
        F = kernel_factor(family, length_scale)
    I = np.eye(RANK)
    G = np.zeros((RANK, RANK))
    parts, Bt = [], np.empty((RANK, n))
    for p in range(0, n, part):
        Vp = V[p:p + part]
        w = Vp.shape[0]
        if w % block:
            raise ValueError("a part is a whole number of blocks")
        nb = w // block
        A = F.T @ (G @ F) + eps * I
        R = np.linalg.cholesky(np.tril(A) + np.tril(A, -1).T)
        Xh = solve_triangular(R, F.T, lower=True)
        b = lambda j: slice(block * j, block * (j + 1))
        xblock = lambda j: Xh @ Vp[b(j)].T
        C = np.full((w, w), np.nan)              # the part of L: tiles on and below the block diagonal
        X = np.full((RANK, w), np.nan)           # the border
        Dw = [None] * nb                         # the pivots' factors until they are placed
        for k in range(nb):
            old, Xold = C.copy(), X.copy()
            if k == 0:
                tile = lambda i, j: eps * (xblock(i).T @ xblock(j))
                border = xblock
            else:
                tile = lambda i, j: old[b(i), b(j)] - old[b(i), b(k - 1)] @ old[b(j), b(k - 1)].T
                border = lambda j: Xold[:, b(j)] - Xold[:, b(k - 1)] @ old[b(j), b(k - 1)].T
            # every item of block column k forms the pivot block itself; nobody writes tile (k, k) in this launch
            D = np.tril(tile(k, k)) + eps * np.eye(block)
            Lkk = np.linalg.cholesky(D + np.tril(D, -1).T)
            for i in range(k + 1, nb):
                C[b(i), b(k)] = solve_triangular(Lkk, tile(i, k).T, lower=True).T
            X[:, b(k)] = solve_triangular(Lkk, border(k).T, lower=True).T
            Dw[k] = Lkk
            for j in range(k + 1, nb):
                X[:, b(j)] = border(j)
                for i in range(j, nb):
                    C[b(i), b(j)] = np.tril(tile(i, j)) if i == j else tile(i, j)
            if k >= 1:
                C[b(k - 1), b(k - 1)] = Dw[k - 1]
        C[b(nb - 1), b(nb - 1)] = Dw[nb - 1]
        parts.append(np.tril(C))
        Bt[:, p:p + part] = eps * (Xh.T @ X)
        G = G + Vp.T @ Vp
    return parts, Bt, V


SUB_WIDTHS = (64, 128, 256, 512)        # GPIRT_NU_SUB: the part widths of draw_f's product (the factor's parts stay PART wide)


def sub_parts(parts, width: int, part: int = PART):
    """The `width`-wide diagonal blocks of L that lie inside its `part`-wide diagonal parts, in order: what csrc/nu_lr.hip
    reads of the factor at GPIRT_NU_SUB = width (nu(sub_parts(parts, w), Bt, V, Z, part=w)).  The last block of a ragged last
    part is whatever is left of it."""
    if width not in SUB_WIDTHS or part % width:
        raise ValueError("the product's part width is 64, 128, 256 or 512 and divides the factor's")
    return [Lpp[q:q + width, q:q + width] for Lpp in parts for q in range(0, Lpp.shape[0], width)]


def nu(parts, Bt, V, Z, part: int = PART) -> np.ndarray:
    """nu = L Z from the parts and the node rows alone (csrc/nu_lr.hip): L[P, P] Z[P] + V[P] sum_{Q < P} Bt[:, Q] Z[Q]"""
    out = np.empty_like(Z)
    T = np.zeros((RANK, Z.shape[1]))
    for q, Lpp in enumerate(parts):
        p = q * part
        out[p:p + part] = Lpp @ Z[p:p + part] + V[p:p + part] @ T
        T = T + Bt[:, p:p + part] @ Z[p:p + part]
    return out


def s_grid(Bt, Vstar) -> np.ndarray:
    """draw_fstar's s = 1 - sqrt(v^T G v) at the rows v of Vstar, G = B^T B the product over the node rows"""
    G = Bt @ Bt.T
    return 1.0 - np.sqrt(np.maximum(np.einsum("jk,kl,jl->j", Vstar, G, Vstar), 0.0))
