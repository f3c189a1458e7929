"""The fused schedule of the structured factor (gpirt_amd/factor_lr.py: structured_factor_fused; csrc/factor_lr.hip's
flr_round_kernel) against the existing NumPy statement: lazy update by the previous panel, a pivot tile
nobody owns, the pivot's factor placed one launch late.  It is the same factorisation in another order of launches, so the
bounds are the ones tests/test_factor_lr_cpu.py holds the statement to against SciPy's dense Cholesky: 1e-10 on the parts,
1e-9 on the node rows, every pivot >= 0.03.

576: a full part and one block; 960: seven blocks behind a full part; 1088: two full parts and one block."""
import functools

import numpy as np
import pytest

from gpirt_amd import factor_lr as FL
from gpirt_amd import fstar_free as FF
from test_factor_lr_cpu import KINDS, theta_case


@functools.lru_cache(maxsize=None)
def _factor():
    return FF.kernel_factor()


@pytest.mark.parametrize("n", [576, 960, 1088])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_schedule_against_the_statement(kind, n):
    theta = theta_case(kind, n)
    parts, Bt, V = FL.structured_factor(theta, F=_factor())
    fparts, fBt, fV = FL.structured_factor_fused(theta, F=_factor())
    assert [a.shape for a in fparts] == [a.shape for a in parts] and fBt.shape == Bt.shape
    assert np.array_equal(fV, V)
    for a in fparts:
        assert np.isfinite(a).all()                       # (a tile read before it was written would be NaN)
        assert np.array_equal(a, np.tril(a))
    gap_parts = max(float(np.abs(a - b).max()) for a, b in zip(fparts, parts))
    gap_rows = float(np.abs(fBt - Bt).max())
    pivot = min(float(np.diag(a).min()) for a in fparts)
    print(f"MEASURED {kind} n={n}: fused schedule against the statement, parts {gap_parts:.2e}, node rows {gap_rows:.2e}, "
          f"smallest pivot {pivot:.4f}")
    assert pivot >= 0.03
    assert gap_parts <= 1e-10
    assert gap_rows <= 1e-9
