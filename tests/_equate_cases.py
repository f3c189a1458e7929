"""The constructed f* that tests/test_gpu_equate.py sets on the device and tests/test_equate_cpu.py checks against the keep
conditions of tests/_equate_bounds.py: logistic curves of positive slope and a few non-monotone ones, |f*| <= 4, form Y easier
than form X, the two forms interleaved over the columns with three columns outside both."""
import numpy as np

NG = 1001
TH = -5.0 + np.arange(NG) * 0.01
# (M_X, M_Y): the lane edges of the row kernel (M + 1 = 2, 3, 64, 65, 66, 128, 129) and the tile edges of the product
SHAPES = [(1, 1), (1, 2), (2, 63), (63, 64), (64, 65), (65, 1), (127, 128)]


def forms(Mx, My, m=None, seed=0):
    """interleaved disjoint forms over m = M_X + M_Y + 3 columns (or m given); columns 0 and m - 1 are outside both"""
    m = Mx + My + 3 if m is None else m
    rng = np.random.default_rng(1000 * Mx + My + seed)
    pick = rng.permutation(np.arange(1, m - 1))[:Mx + My]
    return np.sort(pick[:Mx]), np.sort(pick[Mx:]), m


def curves(m, x, y, seed, shift=0.8):
    """f* (1001 x m): a (theta - b) clipped to [-4, 4], a in (0.4, 1.6), Y's items easier by `shift`; every seventh column
    3 sin(c theta + phase) instead; grid row 777 unlike its neighbours; the columns outside both forms at 4"""
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(0.4, 1.6, m), rng.normal(size=m)
    b[y] -= shift
    f = np.clip(a[None, :] * (TH[:, None] - b[None, :]), -4.0, 4.0)
    wav = np.arange(m) % 7 == 3
    f[:, wav] = 3.0 * np.sin(rng.uniform(0.3, 1.0, wav.sum())[None, :] * TH[:, None] + rng.uniform(0, 6, wav.sum())[None, :])
    f[777] = rng.uniform(-3.0, 3.0, m)
    out = np.ones(m, dtype=bool)
    out[x] = out[y] = False
    f[:, out] = 4.0
    return f


def small_case(Mx, My):
    x, y, m = forms(Mx, My)
    return x, y, [curves(m, x, y, 100 + Mx), curves(m, x, y, 200 + My)]
