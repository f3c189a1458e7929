"""Helpers of tests/test_gpu_factor_shapes.py: the host reference (LAPACK, fp64) and the guard-band frame.

Reference: S = K(theta, theta) + 0.001 I built in NumPy from grid-valued theta, factored by scipy.linalg.cholesky
(dpotrf), solved by scipy.linalg.solve_triangular (dtrtrs).  Nothing here reads the library under test.

Frame: a column-major matrix with a chosen leading dimension and base offset, cut out of a larger device buffer that is
filled with one recognisable NaN.  Whatever lies outside the matrix -- a band in front of the first column, the rows
n .. ld - 1 of every column, a band behind the last column -- must hold that NaN bit for bit after a call, and because
the padding is NaN, a padding value that leaks into a result shows there as NaN.
"""
import numpy as np

SENTINEL = 0x7FF8C0DEFACE5EED          # a quiet NaN with a payload no arithmetic produces
JITTER = 0.001


def theta_grid(n, seed):
    """Grid-valued theta (the recipe of tests/test_gpu_ops.py): differences are exact multiples of 0.01."""
    rng = np.random.default_rng(seed)
    k = np.clip(np.rint((rng.standard_normal(n) + 5.0) / 0.01), 0, 1000)
    return -5.0 + k * 0.01


def spd_matrix(theta):
    """K(theta, theta) + 0.001 I, Fortran order."""
    d = theta[:, None] - theta[None, :]
    np.square(d, out=d)
    d *= -0.5
    np.exp(d, out=d)
    d[np.diag_indices(len(theta))] += JITTER
    return np.asfortranarray(d)


def lapack_factor(S):
    """tril(dpotrf('L', S)); S is left alone."""
    import scipy.linalg as sl
    L = sl.cholesky(S, lower=True, overwrite_a=False, check_finite=False)
    return np.asfortranarray(np.tril(L))


def lapack_info(S):
    """dpotrf's info for S (0: positive definite; k: the leading minor of order k is not)."""
    import scipy.linalg.lapack as ll
    _, info = ll.dpotrf(S, lower=1, overwrite_a=0, clean=0)
    return int(info)


def lapack_solve(L, B, trans):
    import scipy.linalg as sl
    return sl.solve_triangular(L, B, lower=True, trans=1 if trans else 0, check_finite=False)


def factor_errors(L, Lref, S):
    """(max|L - Lref|, ||L L^T - S||_F / ||S||_F, strict upper triangle all zero) -- the three checks of
    test_potrf_matches_oracle.  The residual is formed by dsyrk on the lower triangle (S is symmetric), in a copy."""
    import scipy.linalg.blas as bl
    upper_zero = not np.triu(L, 1).any()
    err = float(np.abs(L - Lref).max())
    snorm = float(np.linalg.norm(S))
    R = bl.dsyrk(1.0, np.asfortranarray(L), beta=-1.0, c=np.array(S, order="F"), lower=1, overwrite_c=1)
    R = np.tril(R)
    dg = np.diag(R).copy()
    np.square(R, out=R)
    ss = 2.0 * float(R.sum()) - float(np.sum(dg * dg))
    return err, float(np.sqrt(ss)) / snorm, upper_zero


class Frame:
    """rows x cols column-major fp64 matrix with leading dimension ld, `offset` doubles behind a 16-byte aligned address,
    inside a sentinel-filled device buffer.  .view is the torch tensor to hand to gpirt_amd.ops (strides (1, ld))."""

    def __init__(self, rows, cols, ld=None, offset=0, fill=None):
        import torch
        ld = rows if ld is None else ld
        assert ld >= rows and rows > 0 and cols > 0
        self.rows, self.cols, self.ld, self.offset = rows, cols, ld, offset
        band = 2 * ((ld + 64) // 2) + 64                     # even: the base is 16-byte aligned exactly when offset is even
        self.start = band + offset
        self.total = self.start + ld * cols + band
        self.raw = torch.full((self.total,), SENTINEL, dtype=torch.int64, device="cuda")
        assert self.raw.data_ptr() % 16 == 0
        self.view = self.raw.view(torch.float64).as_strided((rows, cols), (1, ld), self.start)
        assert self.view.data_ptr() % 16 == (8 * offset) % 16
        if fill is not None:
            self.put(fill)

    def put(self, host):
        from gpirt_amd.ops import to_device
        host = np.asarray(host, dtype=np.float64)
        assert host.shape == (self.rows, self.cols)
        self.view.copy_(to_device(host))
        return self

    def get(self):
        from gpirt_amd.ops import to_host
        return to_host(self.view)

    def guard_damage(self):
        """Number of guard words that no longer hold the sentinel (0 = nothing outside the matrix was written)."""
        raw = self.raw.cpu().numpy()
        guard = np.ones(self.total, dtype=bool)
        body = guard[self.start:self.start + self.ld * self.cols].reshape(self.cols, self.ld)
        body[:, :self.rows] = False
        return int(np.count_nonzero(raw[guard] != SENTINEL))

    def assert_intact(self, what=""):
        bad = self.guard_damage()
        assert bad == 0, (f"{what}: {bad} words outside the {self.rows} x {self.cols} matrix (ld {self.ld}, "
                          f"offset {self.offset}) were written")
