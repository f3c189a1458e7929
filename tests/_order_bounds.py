"""Bounds for comparing the device's order block (csrc/order.hip) with gpirt_amd.shape.order_from_draws, derived from each
case's own curves.

above, cross, depth_sum, set_counts, draws, skipped and u are compared with ==: every decision behind them is an fp64
comparison of a max / min of ONE subtraction on the same g, and depth_sum adds the same doubles in the same draw order.
The easiness e_j = sum_k w_k / (1 + exp(-g[k, j])) differs by rounding alone.  EPS = 2^-52, first order, counts rounded up:
  w_k       the host's double weights against the long-double ones: 520 EPS (tests/_shape_bounds.py)
  exp(-g)   within 2 ulp; through 1 / (1 + t) that is 2 EPS t / (1 + t) <= 2 EPS of the term
  1 + t     one rounding, 0.5 EPS; the division another 0.5                          -> 523 EPS of each (positive) term
  the sum   1001 positive terms in a fixed order: at most 1003 EPS of the sum (1000 additions with second-order slack)
  the reference runs in long double (2^-64 an operation) and is rounded to fp64 once: 0.5
together below 1530 EPS e.  Where exp(-g) overflows in fp64 (g < -709.78) the device's term is exactly 0 and the long double's is
below w_k 2^-1023: an absolute 1e-300 covers all 1001 of them.
easier[a, b] is decided on the device's own e; against the long-double statement it can differ only where |e_a - e_b| is
within the two items' bounds, so pairs further apart than gap_needed() must agree.
"""
import numpy as np

from gpirt_amd import shape as SH

EPS = float(np.finfo(np.float64).eps)
EXACT = ("above", "cross", "depth_sum", "set_counts")


def e_bound(e_ld):
    """bound on |device e - long double e| per item, from the long-double e of the same curves"""
    return 1530.0 * EPS * np.asarray(e_ld, dtype=np.float64) + 1e-300


def check_exact(got, want, label=""):
    for k in EXACT:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (label, k, a.shape, b.shape, a.dtype, b.dtype)
        assert (a == b).all(), (label, k, int((a != b).sum()))
    assert (got["draws"], got["skipped"]) == (want["draws"], want["skipped"]), label


def check_easiness(dev_e, want, label="", need_all=True):
    """dev_e: the device's e after each counted draw (S x m); want: order_from_draws of the same curves.  e within e_bound; the
    long-double easier decisions for every pair further apart than twice the bound; need_all: no pair may be closer."""
    dev_e = np.asarray(dev_e, dtype=np.float64)
    ld = want["e_draws"]
    assert dev_e.shape == ld.shape, (label, dev_e.shape, ld.shape)
    bd = e_bound(ld)
    gap = np.abs(dev_e - np.asarray(ld, dtype=np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"MEASURED {label} e: observed / bound = {float((gap / bd).max()):.3g}")
    assert (gap <= bd).all(), (label, float((gap / bd).max()))
    m = dev_e.shape[1]
    off = ~np.eye(m, dtype=bool)
    easier_dev = np.zeros((m, m), dtype=np.uint32)
    for row_dev, row_ld, b in zip(dev_e, ld, bd):
        far = np.abs(row_ld[:, None] - row_ld[None, :]) > 2.0 * np.maximum(b[:, None], b[None, :])
        if need_all:
            assert far[off].all(), (label, "a pair's easiness gap is inside the bound: pick another seed")
        d_dev, d_ld = row_dev[:, None] > row_dev[None, :], row_ld[:, None] > row_ld[None, :]
        assert (d_dev == d_ld)[far & off].all(), label
        easier_dev += d_dev.astype(np.uint32)
    return easier_dev
