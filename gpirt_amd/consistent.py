"""A consistent step beside the reference's (include/gpirt_hip.h, "a consistent step"; csrc/carry.hip; Sampler.carry_f,
Sampler.step(consistent=True), Sampler.prior_quad).

The reference's iteration moves theta and keeps f (quirk Q3 of SURVEY.md): after a step, f[i, :] is the GP's value at
respondent i's OLD position while mu, L and everything built on them belong to the new one.  The carry stage, between draw_theta
and draw_beta, makes the pair consistent: given the curve on the grid, theta's draw is the reference's own, and f then becomes
that curve at the new theta plus the model's nugget,

    f_ij = (fstar[k_i, j] - mu_star[k_i, j]) + sd_j z_ij,   sd_j = a_j sqrt(0.001),   k_i the grid index of theta_i.

It is exact up to two named approximations: f* is the reference's conditional mean plus independent noise of sd s, about 1e-6,
not a joint draw; and the nugget is redrawn from its prior (sd 0.03 logits), not tilted by the likelihood.  The next draw_f is
an exact update of f | theta, y.

`carry_exact` is the NumPy statement of the stage and holds the same bits given the device's normals (`normals`);
`prior_quad_exact` is the statistic that shows the effect, Q_j = f_j^T S(theta)^-1 f_j / (n a_j^2): near 1 for a state that is
consistent with its prior, in the hundreds after the reference's step, some 30 times too small after a carry without the nugget.
"""
from __future__ import annotations

import numpy as np

from ._lib import ST_CARRY

SQRT_JITTER = 0.031622776601683794        # sqrt(0.001), correctly rounded: the jitter's square root


def carry_exact(theta, fstar, mu_star, f, z, amp=None, nugget=True) -> np.ndarray:
    """The carry as gpirt_sampler_carry_f states it.  theta (n), fstar and mu_star (1001 x m), f (n x m), z (n x m: the
    normals of `normals`; not read with nugget=False, None allowed then), amp (m amplitudes or None: 1.0 exactly).  Returns the
    new f (fp64, a copy): a row whose theta is no grid point (NaN included) keeps its f byte for byte; every other row is
    g = fstar[k_i] - mu_star[k_i] (one fp64 subtraction), plus sd_j z_ij with nugget (one multiplication, one addition)."""
    from .quantiles import grid_index
    fstar = np.asarray(fstar, dtype=np.float64)
    mu_star = np.asarray(mu_star, dtype=np.float64)
    out = np.array(f, dtype=np.float64, copy=True, order="F")
    k = grid_index(theta)
    on = k >= 0
    with np.errstate(invalid="ignore", over="ignore"):
        g = fstar[k[on], :] - mu_star[k[on], :]
        if nugget:
            m = out.shape[1]
            a = np.ones(m) if amp is None else np.broadcast_to(np.asarray(amp, dtype=np.float64), (m,))
            sd = a * SQRT_JITTER
            g = g + sd[None, :] * np.asarray(z, dtype=np.float64)[on, :]
    out[on, :] = g
    return out


def counters_exact(theta, fstar) -> dict:
    """What one carry counts: off_grid (rows whose theta is no grid point) and nonfinite (non-finite fstar cells carried)."""
    from .quantiles import grid_index
    k = grid_index(theta)
    on = k >= 0
    return dict(off_grid=int((~on).sum()), nonfinite=int((~np.isfinite(np.asarray(fstar, dtype=np.float64)[k[on], :])).sum()))


def normals(handle, seed, it, item0, m, n) -> np.ndarray:
    """z (n x m) of the carry that closes iteration `it` (counted from 1: Sampler.iteration + 1 in front of the stage's
    factor): qnorm(item_uniform(seed, it, GPIRT_ST_CARRY, item0 + j, i)), from the device (Handle.item_normals)."""
    from .ops import to_host
    return np.asfortranarray(to_host(handle.item_normals(int(seed), int(it), ST_CARRY, int(item0), int(m), int(n))))


def prior_quad_exact(theta, f, kernel, amp=None) -> np.ndarray:
    """Q_j = || L^-1 f_j ||^2 / (n a_j^2), L = chol(K(theta, theta) + 0.001 I) under `kernel` (a gpirt_amd.kernel argument):
    the factor in fp64, the forward substitution and the sums in long double (gpirt_amd.ell.factor, solve_lower); m values,
    fp64.  What Sampler.prior_quad() returns for a sampler whose factor belongs to theta."""
    from . import ell as EL
    from . import kernel as K
    family, length_scale = K.spec(kernel)
    f = np.asarray(f, dtype=np.float64)
    n, m = f.shape
    nu = EL.solve_lower(EL.factor(theta, family, length_scale), f)
    q = (nu * nu).sum(axis=0)
    a = np.ones(m, dtype=EL.LD) if amp is None else np.broadcast_to(np.asarray(amp, dtype=np.float64), (m,)).astype(EL.LD)
    return (q / (EL.LD(n) * a * a)).astype(np.float64)
