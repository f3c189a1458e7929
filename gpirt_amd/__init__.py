"""gpirt_amd -- MI355X-native (gfx950) implementation of the GP linear-algebra hot path of
duckmayr/gpirt's gpirtMCMC(), behind the reference's own boundary.

Layout:
  csrc/            hand-written HIP kernels + the C ABI (include/gpirt_hip.h) -> libgpirt_hip.so
  _lib.py          ctypes binding of that C ABI (fails loudly when the library / GPU is missing)
  ops.py           operator-level host API (K, chol, trmm, trsm, draw_f, draw_fstar, ...)
  sampler.py       gpirtMCMC() mirror of the reference's R entry point, and the stage-driven Sampler
  chains.py ... groups.py     host side of the on-device posterior functionals (chains, quantiles, ppc, ranks, score,
                   shape, sumscore, equate, loo, acf, groups): the C structs, the pooling of chains and the NumPy statement each is tested against
  kernel.py        the covariance kernel of a handle (length scale, Matern 5/2 and 3/2): the NumPy statement, the rank
                   certificate, one run per kernel and their comparison by elpd_loo
  ell.py           the kernel's length scale as a parameter of the chain (a whitened Metropolis update on a grid): the
                   NumPy statement of one update, the exact conditional posterior, the one-call run
  amp.py           per-item GP amplitudes, fixed or sampled in the chain (one launch updates every item on a grid): the
                   NumPy statement of one update, the exact conditional posterior per item, the one-call run
  consistent.py    the consistent step beside the reference's (f carried to the new theta plus the model's nugget) and the
                   prior check: the NumPy statement of the carry, the device's normals, the exact prior quadratic form
  pop.py           a population prior for theta, a table per group, fixed or with the groups' means and sds sampled by exact
                   Gibbs on two grids: the NumPy statement of one update, the exact conditional masses, the one-call run
  scale.py         the collapsed scale and shift move on the linear mean with theta summed out: the NumPy statement of one
                   call, the collapsed target, the one-call run
  ordinal.py       ordinal (graded) responses under the cumulative-logit model, the thresholds sampled by exact Gibbs on a grid
                   inside a random window: the NumPy statement of every swapped stage in long double, the one-call run
  distributed.py   item-column sharding over torch.distributed (RCCL), one process per GPU
  response_matrix.py, synthetic.py   host-side data preparation
"""
from .response_matrix import as_response_matrix, is_response_matrix, response_matrix  # noqa: F401
from .sampler import Sampler, gpirtMCMC  # noqa: F401

__all__ = ["gpirtMCMC", "Sampler", "response_matrix", "as_response_matrix", "is_response_matrix"]
